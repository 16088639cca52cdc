"""The token-noise rule without a GPU: the NumPy reference of tests/token_noise_cases.py against a scalar restatement
in Python integers, its replace rate, ranges and independence statistics -- the same checks turned on four mutants,
each of which at least one check must reject -- then csrc/dropout_philox.h (what the kernels compile) built for the
host alone and put through the same checks and an id-for-id comparison over the case table, and the command-line
refusals."""
import math
import os
import subprocess

import numpy as np
import pytest

import dropout_cases as C
import token_noise_cases as TN
from conftest import PKG


# ---- a scalar restatement, Python integers only ----------------------------------------------------------------
def philox_scalar(counter, key, rounds=10):
    c0, c1, c2, c3 = counter
    k0, k1 = key
    for _ in range(rounds):
        p0, p1 = C.M0 * c0, C.M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & 0xFFFFFFFF, (p0 >> 32) ^ c3 ^ k1, p0 & 0xFFFFFFFF
        k0, k1 = (k0 + C.W0) & 0xFFFFFFFF, (k1 + C.W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def noise_scalar(tok, n, j, S, K, T, R, seed, stream, step, rank):
    if not 0 <= tok < K:
        return tok
    out = philox_scalar((n * S + j, 0x40000000 | stream, step, rank), (seed & 0xFFFFFFFF, seed >> 32))
    if (out[0] & 0xFFFF) >= T:
        return tok
    lo, hi = (0, K - 1) if R == 0 else (max(0, tok - R), min(K - 1, tok + R))
    return lo + ((out[1] * (hi - lo + 1)) >> 32)


class Reference:
    """The implementation under test, as the checks see it; mutants override one piece."""
    mutant = {}

    def noise(self, ids, K, T, R, seed, stream, step, rank):
        return TN.noise(ids, K, T, R, seed, stream, step, rank, **self.mutant)

    def window(self, hr, offs, W, K, T, R, seed, step, rank):
        """The corrupted hr tokens offs[n] ... offs[n] + W - 1 of every sample, as a windowed launch shows them."""
        full = self.noise(hr, K, T, R, seed, 0, step, rank)
        return np.take_along_axis(full, np.asarray(offs)[:, None] + np.arange(W)[None, :], 1)


# ---- the checks --------------------------------------------------------------------------------------------------
def check_by_hand(impl):
    rng = np.random.default_rng(1)
    for K, R, T, stream, step, rank in TN.HOST_CASES:
        ids = TN.tokens(TN.N, TN.S_HR, K, rng)
        ids[1, 5], ids[2, 6] = -1, K                       # outside [0, K): pass through
        got = impl.noise(ids, K, T, R, TN.SEED, stream, step, rank)
        want = [[noise_scalar(int(ids[n, j]), n, j, TN.S_HR, K, T, R, TN.SEED, stream, step, rank)
                 for j in range(TN.S_HR)] for n in range(TN.N)]
        assert got.tolist() == want, (K, R, T, stream, step, rank)
        assert got[1, 5] == -1 and got[2, 6] == K


def _replaced(impl, K, T, seed, stream, step, rank, N=4):
    """Which of STAT_N tokens were replaced: with R = 0 the new id does not depend on the old one, so a token was
    replaced iff the all-zeros and the all-ones stream come out equal there."""
    S = TN.STAT_N // N
    a = impl.noise(np.zeros((N, S), dtype=np.int64), K, T, 0, seed, stream, step, rank)
    b = impl.noise(np.ones((N, S), dtype=np.int64), K, T, 0, seed, stream, step, rank)
    return a == b


def check_replace_rate(impl):
    worst = 0.0
    for T in TN.STAT_TS:
        q = T / 65536.0
        sigma = math.sqrt(TN.STAT_N * q * (1.0 - q))
        for stream, step, rank in TN.STAT_STREAMS:
            rep = _replaced(impl, 8192, T, C.SEED, stream, step, rank)
            dev = abs(int(rep.sum()) - TN.STAT_N * q) / sigma
            worst = max(worst, dev)
            assert dev <= TN.SIGMAS, (T, stream, step, rank, dev)
    return worst


def check_ranges(impl):
    rng = np.random.default_rng(2)
    for K in TN.KS:
        for R in TN.RS:
            ids = TN.tokens(8, 512, K, rng)
            out = impl.noise(ids, K, 58982, R, TN.SEED, 0, 3, 1)
            lo = np.maximum(ids - R, 0) if R else np.zeros_like(ids)
            hi = np.minimum(ids + R, K - 1) if R else np.full_like(ids, K - 1)
            assert ((out >= lo) & (out <= hi)).all(), (K, R)
            assert (out != ids).any()
            if R:                                           # both clamps fired: tokens at 0 and K - 1 were replaced
                for col in (0, 3):
                    assert (out[:, col] <= R).all() and (out[:, col] != 0).any()
                for col in (2, 511):
                    assert (out[:, col] >= K - 1 - R).all() and (out[:, col] != K - 1).any()
    out = impl.noise(np.zeros((2, 256), dtype=np.int64), 5, 58982, 0, TN.SEED, 1, 1, 0)
    assert sorted(set(out.flatten().tolist())) == [0, 1, 2, 3, 4]          # R = 0, K = 5: every code occurs


def check_independence(impl):
    """Stream, step and rank each change the noise: two independent Bernoulli(q) decisions disagree with share
    2 q (1 - q)."""
    worst = 0.0
    T = 32768
    q = T / 65536.0
    d = 2.0 * q * (1.0 - q)
    sigma = math.sqrt(TN.STAT_N * d * (1.0 - d))
    base = _replaced(impl, 8192, T, C.SEED, 0, 1, 0)
    for stream, step, rank in ((1, 1, 0), (0, 2, 0), (0, 1, 1)):
        other = _replaced(impl, 8192, T, C.SEED, stream, step, rank)
        dev = abs(int((base != other).sum()) - TN.STAT_N * d) / sigma
        worst = max(worst, dev)
        assert dev <= TN.SIGMAS, (stream, step, rank, dev)
    return worst


def check_window_invariance(impl):
    """The same hr token seen through two windows is corrupted identically, and as the whole stream is."""
    rng = np.random.default_rng(3)
    K, T, R, W = 513, 32768, 7, 16
    hr = TN.tokens(TN.N, TN.S_HR, K, rng)
    full = impl.noise(hr, K, T, R, TN.SEED, 0, 4, 1)
    a = impl.window(hr, [0, 5, 21], W, K, T, R, TN.SEED, 4, 1)
    b = impl.window(hr, [8, 9, 10], W, K, T, R, TN.SEED, 4, 1)
    assert np.array_equal(a[0, 8:], b[0, :8]) and np.array_equal(a[1, 4:], b[1, :12])
    assert np.array_equal(b[2, 11:], a[2, :5])
    for win, offs in ((a, (0, 5, 21)), (b, (8, 9, 10))):
        for n, o in enumerate(offs):
            assert np.array_equal(win[n], full[n, o:o + W])


CHECKS = (check_by_hand, check_replace_rate, check_ranges, check_independence, check_window_invariance)


# ---- the reference passes ----------------------------------------------------------------------------------------
def test_reference_against_the_scalar_restatement():
    check_by_hand(Reference())


def test_replace_rate():
    print(f"MEASURED token-noise replace-rate worst deviation {check_replace_rate(Reference()):.2f} sigma "
          f"(bound {TN.SIGMAS})")


def test_replacements_stay_in_range_and_cover_a_small_codebook():
    check_ranges(Reference())


def test_streams_steps_and_ranks_differ():
    print(f"MEASURED token-noise independence worst deviation {check_independence(Reference()):.2f} sigma "
          f"(bound {TN.SIGMAS})")
    ids = TN.tokens(TN.N, TN.S_HR, 513, np.random.default_rng(4))
    outs = [TN.noise(ids, 513, 32768, 7, TN.SEED, *s) for s in TN.STREAMS]
    for i in range(len(outs)):
        for j in range(i + 1, len(outs)):
            assert not np.array_equal(outs[i], outs[j]), (TN.STREAMS[i], TN.STREAMS[j])


def test_window_invariance():
    check_window_invariance(Reference())


# ---- the mutants are rejected ------------------------------------------------------------------------------------
class WindowIndexMutant(Reference):
    def window(self, hr, offs, W, K, T, R, seed, step, rank):
        hr = np.asarray(hr)
        shown = np.take_along_axis(hr, np.asarray(offs)[:, None] + np.arange(W)[None, :], 1)
        return TN.noise(shown, K, T, R, seed, 0, step, rank)           # keyed on n W + w


def _mutant(name):
    if name == "window index instead of absolute index":
        return WindowIndexMutant()
    m = Reference()
    m.mutant = {"no clamp": {"no_clamp": True}, "modulo instead of multiply-high": {"modulo": True},
                "decision from out[1]": {"decide_from_1": True}}[name]
    return m


@pytest.mark.parametrize("name", ["window index instead of absolute index", "no clamp",
                                  "modulo instead of multiply-high", "decision from out[1]"])
def test_mutant_is_rejected(name):
    rejected_by = []
    for check in CHECKS:
        try:
            check(_mutant(name))
        except AssertionError:
            rejected_by.append(check.__name__)
    print(f"mutant {name}: rejected by {rejected_by}")
    assert rejected_by, f"no check tells the mutant {name} from the definition"


# ---- the kernels' own header, compiled for the host --------------------------------------------------------------
HOST_PROGRAM = r'''
#include <stdio.h>
#include <stdlib.h>
#include "dropout_philox.h"
// stdin: K T R seed_lo seed_hi stream step rank N S, then N S ids; stdout: the corrupted ids; repeated until EOF
int main() {
    long long K, T, R, lo, hi, stream, step, rank, N, S;
    while (scanf("%lld %lld %lld %lld %lld %lld %lld %lld %lld %lld", &K, &T, &R, &lo, &hi, &stream, &step, &rank, &N,
                 &S) == 10) {
        for (long long n = 0; n < N; ++n)
            for (long long j = 0; j < S; ++j) {
                long long id;
                if (scanf("%lld", &id) != 1) return 1;
                printf("%lld\n", (long long)qarig::token_noise_id(id, (uint32_t)(n * S + j), (uint32_t)stream, (int)K,
                                                                  (uint32_t)T, (int)R, (uint32_t)step, (uint32_t)rank,
                                                                  (uint32_t)lo, (uint32_t)hi));
            }
    }
    printf("%u %u %u\n", QARIG_TOKEN_NOISE_DOMAIN, QARIG_TOKEN_NOISE_STREAMS, qarig::token_noise_c1(1u));
    return 0;
}
'''


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    cxx = "/opt/rocm/lib/llvm/bin/clang++"
    assert os.path.exists(cxx)
    d = tmp_path_factory.mktemp("token_noise_host")
    src = d / "token_noise_host.cpp"
    src.write_text(HOST_PROGRAM)
    exe = str(d / "token_noise_host")
    subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-Wno-pass-failed",
                    "-I", os.path.join(PKG, "csrc"), str(src), "-o", exe], check=True, capture_output=True, text=True)
    return exe


class Header(Reference):
    """csrc/dropout_philox.h on the host, one process per call."""

    def __init__(self, exe):
        self.exe = exe
        self.tail = None

    def noise(self, ids, K, T, R, seed, stream, step, rank):
        ids = np.asarray(ids, dtype=np.int64)
        N, S = ids.shape
        text = f"{K} {T} {R} {seed & 0xFFFFFFFF} {seed >> 32} {stream} {step} {rank} {N} {S}\n" + \
            "\n".join(map(str, ids.flatten().tolist())) + "\n"
        out = subprocess.run([self.exe], input=text, check=True, capture_output=True, text=True).stdout.split("\n")
        self.tail = out[N * S]
        return np.array(list(map(int, out[:N * S])), dtype=np.int64).reshape(N, S)


def test_kernel_header_on_the_host(host_exe):
    impl = Header(host_exe)
    rng = np.random.default_rng(5)
    for K, R, T, stream, step, rank in TN.HOST_CASES:              # id for id with the NumPy rule
        ids = TN.tokens(TN.N, TN.S_HR, K, rng)
        ids[0, 7], ids[1, 8] = -3, K + 2
        got = impl.noise(ids, K, T, R, TN.SEED, stream, step, rank)
        want = TN.noise(ids, K, T, R, TN.SEED, stream, step, rank)
        assert np.array_equal(got, want), (K, R, T, stream, step, rank)
        assert (got != ids).any() or T == 1
    assert impl.tail.split() == [str(TN.DOMAIN), "2", str(TN.DOMAIN | 1)]
    from qarig import ops
    assert ops.TOKEN_NOISE_STREAMS == 2
    for check in CHECKS:
        check(impl)


def test_domains_of_the_second_counter_word_are_disjoint():
    """Residual dropout: site ordinals 0 ... 2 + layers (far below 2^30); attention: bit 31 set; token noise:
    bit 30 set, bit 31 clear."""
    from qarig.dropout import ATTN_DROPOUT_MAX_KEYS, ATTN_DROPOUT_SITES
    noise_words = {TN.DOMAIN | s for s in (0, 1)}
    assert all(w >> 30 == 1 for w in noise_words)
    attn_lo = 0x80000000
    attn_hi = 0x80000000 | (ATTN_DROPOUT_SITES - 1) << 23 | (ATTN_DROPOUT_MAX_KEYS - 1) >> 3
    assert attn_lo >> 31 == 1 and attn_hi < 1 << 32 and max(noise_words) < attn_lo
    import torch  # noqa: F401  (models imports it)
    from models.Transformer import Transformer
    m = Transformer(use_encoder=True, use_pos_cond=True, num_enc_layers=2, num_dec_layers=2, num_enc_embedding=8,
                    num_dec_embedding=9, self_attn_heads=2, cross_attn_heads=2, transformer_in_dim=16,
                    transformer_out_dim=9, transformer_hidden_dim=32)
    assert 2 + len(m._residual_layers()) < min(noise_words)


# ---- the command line ----------------------------------------------------------------------------------------------
def test_command_line_arguments_and_refusals():
    import argparse
    from qarig import cli_common as cc
    p = argparse.ArgumentParser()
    cc.add_dropout_args(p)
    cc.add_token_noise_args(p)
    got = vars(p.parse_args([]))
    assert (got["input_noise"], got["cond_noise"], got["noise_range"], got["dropout_seed"]) == (0.0, 0.0, 0, 0)
    got = vars(p.parse_args(["--input-noise", "0.1", "--cond-noise", "0.25", "--noise-range", "3", "--dropout-seed",
                             "0x5EED"]))
    assert (got["input_noise"], got["cond_noise"], got["noise_range"], got["dropout_seed"]) == (0.1, 0.25, 3, 0x5EED)
    for flag in ("--input-noise", "--cond-noise"):
        for bad in ("0.91", "1", "-0.1", "nan", "1e-6", "x"):          # P outside (0, 0.9]
            with pytest.raises(SystemExit):
                p.parse_args([flag, bad])
    for bad in ("-1", "1.5", "x"):                                       # R < 0
        with pytest.raises(SystemExit):
            p.parse_args(["--noise-range", bad])
    assert cc.check_token_noise_args(0.0, 0.0, 0, 0) == (0.0, 0.0, 0, 0)
    assert cc.check_token_noise_args(0.1, 0.9, 7, 5, k_lr=8, k_hr=512) == (0.1, 0.9, 7, 5)
    for bad in ((0.95, 0, 0), (0, float("nan"), 0), (0.1, 0.1, -1), (1e-6, 0, 0)):
        with pytest.raises(ValueError):
            cc.check_token_noise_args(*bad, 0)
    with pytest.raises(ValueError, match="--train-base-model"):
        cc.check_token_noise_args(0.1, 0.1, 0, 0, train_base_model=True)
    assert cc.check_token_noise_args(0.1, 0.0, 0, 0, train_base_model=True) == (0.1, 0.0, 0, 0)
    for r in (8, 9, 512):                                                # R at or above the smaller codebook
        with pytest.raises(ValueError, match="use 0"):
            cc.check_token_noise_args(0.1, 0.1, r, 0, k_lr=8, k_hr=512)
    from qarig.dropout import TokenNoise, threshold_and_scale
    st = TokenNoise.probabilities(0.1, 0.0, 3)
    assert st.t_input == threshold_and_scale(0.1)[0] and st.t_cond == 0 and st.key is None and st[1] is None
    for bad in ((0.95, 0, 0), (0, 1.0, 0), (0.1, 0, -2), (0.1, 0, 1.5)):
        with pytest.raises(ValueError):
            TokenNoise.probabilities(*bad)
