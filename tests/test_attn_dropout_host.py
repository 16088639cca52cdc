"""The attention-probability dropout mask without a GPU: csrc/dropout_philox.h (the text the attention kernels
compile) built for the host alone and its keep function compared with the NumPy restatement of
tests/attn_dropout_cases.py over a grid of (site, step, rank, n, h, i, j); the same comparison turned on four mutants,
each of which it must reject; independence from the residual sites under one seed; the keep rate; and the refusals of
the command-line checker."""
import argparse
import math
import os
import subprocess

import numpy as np
import pytest

import attn_dropout_cases as AD
import dropout_cases as C
from conftest import PKG

HOST_PROGRAM = r'''
#include <stdio.h>
#include "dropout_philox.h"
// stdin: lines "n H h Sq i j site T step rank seed_lo seed_hi"; stdout: one keep bit per line read
int main() {
    unsigned n, H, h, Sq, i, j, site, T, step, rank, lo, hi;
    while (scanf("%u %u %u %u %u %u %u %u %u %u %u %u", &n, &H, &h, &Sq, &i, &j, &site, &T, &step, &rank, &lo, &hi) == 12) {
        const bool keep = qarig::attn_dropout_keep(n, H, h, Sq, i, j, site, T, step, rank, lo, hi);
        // the pieces the kernels use, against the composed function
        uint32_t w[4];
        qarig::philox4x32_10(qarig::attn_dropout_c0(n, H, h, Sq, i), qarig::attn_dropout_c1(site, j), step, rank, lo, hi, w);
        const bool bit = (qarig::attn_dropout_keep8(w, T) >> (j & 7)) & 1u;
        if (bit != keep) return 3;
        putchar(keep ? '1' : '0');
    }
    putchar('\n');
    printf("%u %d\n", QARIG_ATTN_DROPOUT_SITES, QARIG_ATTN_DROPOUT_MAX_SK);
    return 0;
}
'''

H, SQ = 5, 70
THRESHOLDS = (6554, 32768)


def _grid():
    """(n, h, i, j, site, T, step, rank) rows: every stream of AD.STREAMS (site 255 among them), keys around the
    call boundary j = 7 / 8 and further ones, several queries, heads and sequences."""
    rows = []
    for site, step, rank in AD.STREAMS:
        for t in THRESHOLDS:
            for n in (0, 1):
                for h in (0, 3):
                    for i in (0, 1, 7, 8, 69):
                        for j in (0, 1, 6, 7, 8, 9, 15, 16, 63, 64, 200):
                            rows.append((n, h, i, j, site, t, step, rank))
    return np.array(rows, dtype=np.int64)


@pytest.fixture(scope="module")
def header_bits(tmp_path_factory):
    cxx = "/opt/rocm/lib/llvm/bin/clang++"
    assert os.path.exists(cxx)
    tmp = tmp_path_factory.mktemp("attn_dropout_host")
    src = tmp / "attn_philox_host.cpp"
    src.write_text(HOST_PROGRAM)
    exe = str(tmp / "attn_philox_host")
    subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-Wno-pass-failed",
                    "-I", os.path.join(PKG, "csrc"), str(src), "-o", exe], check=True, capture_output=True, text=True)
    g = _grid()
    lo, hi = AD.SEED & 0xFFFFFFFF, AD.SEED >> 32
    assert lo and hi
    text = "".join(f"{n} {H} {h} {SQ} {i} {j} {site} {t} {step} {rank} {lo} {hi}\n" for n, h, i, j, site, t, step, rank in g)
    out = subprocess.run([exe], input=text, check=True, capture_output=True, text=True).stdout.splitlines()
    bits = np.array([c == "1" for c in out[0]])
    assert bits.size == len(g)
    return g, bits, out[1]


def _numpy_bits(g, **mutant):
    out = np.zeros(len(g), dtype=bool)
    for site, step, rank in AD.STREAMS:
        for t in THRESHOLDS:
            sel = (g[:, 4] == site) & (g[:, 5] == t) & (g[:, 6] == step) & (g[:, 7] == rank)
            r = g[sel]
            out[sel] = AD.keep_elements(r[:, 0], r[:, 1], r[:, 2], r[:, 3], H, SQ, t, AD.SEED, site, step, rank, **mutant)
    return out


def test_header_keep_function_matches_the_numpy_mask(header_bits):
    g, bits, limits = header_bits
    assert np.array_equal(bits, _numpy_bits(g))
    assert 0.2 < bits.mean() < 0.95                  # both values occur: the comparison is not vacuous
    assert limits.split() == [str(AD.MAX_SITE + 1), str(AD.MAX_SK)]
    from qarig import dropout as D, ops
    assert (D.ATTN_DROPOUT_SITES, D.ATTN_DROPOUT_MAX_KEYS) == (AD.MAX_SITE + 1, AD.MAX_SK)
    assert ops.ATTN_DROPOUT_SITES is D.ATTN_DROPOUT_SITES


def test_dense_mask_matches_the_per_element_form():
    for site, step, rank in AD.STREAMS[:3] + AD.STREAMS[-1:]:
        m = AD.mask(2, 3, 9, 21, 32768, AD.SEED, site, step, rank)
        n, h, i, j = np.meshgrid(np.arange(2), np.arange(3), np.arange(9), np.arange(21), indexing="ij")
        assert np.array_equal(m, AD.keep_elements(n, h, i, j, 3, 9, 32768, AD.SEED, site, step, rank))


@pytest.mark.parametrize("name", ["swap_ij", "no_high_bit", "shift2", "no_step"])
def test_mutant_is_rejected(header_bits, name):
    g, bits, _ = header_bits
    differ = int((bits != _numpy_bits(g, **{name: True})).sum())
    print(f"mutant {name}: {differ} of {len(g)} grid elements differ from the header")
    assert differ > len(g) // 20


def test_residual_site_and_attention_site_differ():
    """Residual site k reads counter (e >> 3, k, step, rank); attention site k with N = H = 1 has
    c0 = i: the same first word, and only the second word (high bit, site field) tells the two apart."""
    t = 32768
    for k in (0, 1, 5):
        res = C.mask(8 * 4096, t, AD.SEED, k, 3, 0).reshape(4096, 8)
        att = AD.mask(1, 1, 4096, 8, t, AD.SEED, k, 3, 0)[0, 0]
        d = 0.5                                       # two independent fair masks disagree on half the elements
        sigma = math.sqrt(res.size * d * (1 - d))
        assert abs(int((res != att).sum()) - res.size * d) <= C.SIGMAS * sigma, k


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_keep_rate(p):
    t, _ = C.threshold_and_scale(p)
    m = AD.mask(2, 4, 512, 256, t, AD.SEED, 3, 11, 1)           # 2^20 elements
    assert m.size == 1 << 20
    qk = 1.0 - t / 65536.0
    dev = abs(int(m.sum()) - m.size * qk) / math.sqrt(m.size * qk * (1 - qk))
    print(f"MEASURED attention dropout keep-rate deviation at p={p}: {dev:.2f} sigma (bound {C.SIGMAS})")
    assert dev <= C.SIGMAS


def test_command_line_checker_refusals():
    from qarig import cli_common as cc
    p = argparse.ArgumentParser()
    cc.add_attn_dropout_args(p)
    assert vars(p.parse_args([])) == {"attn_dropout": 0.0}
    assert vars(p.parse_args(["--attn-dropout", "0.1"])) == {"attn_dropout": 0.1}
    for bad in ("0.91", "1", "-0.1", "nan", "1e-6", "x"):             # T outside [1, 58982]
        with pytest.raises(argparse.ArgumentTypeError):
            cc.attn_dropout_arg(bad)
    assert cc.check_attn_dropout_args(0.0, 0) == (0.0, 0)
    assert cc.check_attn_dropout_args(0.5, 7, sites=256, batch=64, heads=64, seq_q=256, seq_k=1 << 26) == (0.5, 7)
    assert cc.check_attn_dropout_args(0.0, 7, sites=1000) == (0.0, 7)         # off: nothing to refuse
    for bad in (dict(attn_dropout=0.95), dict(attn_dropout=float("nan")), dict(dropout_seed=-1),
                dict(dropout_seed=2 ** 64), dict(sites=257), dict(seq_k=(1 << 26) + 1),
                dict(batch=1 << 16, heads=1 << 8, seq_q=1 << 8)):
        args = dict(attn_dropout=0.5, dropout_seed=7)
        args.update(bad)
        with pytest.raises(ValueError):
            cc.check_attn_dropout_args(**args)
