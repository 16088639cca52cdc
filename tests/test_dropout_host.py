"""The dropout mask's definition without a GPU: the NumPy reference of tests/dropout_cases.py against the known
answers of Philox4x32-10, a scalar restatement in Python integers (the element layout for e = 0 ... 15), the
(T, s) rule of qarig.dropout, keep-rate and independence statistics -- and the same checks turned on five
mutants, each of which at least one check must reject.  Last, csrc/dropout_philox.h (what the kernel compiles)
built for the host alone and compared with the reference word for word."""
import math
import os
import struct
import subprocess

import numpy as np
import pytest

import dropout_cases as C
from conftest import PKG


# ---- a scalar restatement, Python integers only --------------------------------------------------------------
def philox_scalar(counter, key, rounds=10):
    c0, c1, c2, c3 = counter
    k0, k1 = key
    for _ in range(rounds):
        p0, p1 = C.M0 * c0, C.M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & 0xFFFFFFFF, (p0 >> 32) ^ c3 ^ k1, p0 & 0xFFFFFFFF
        k0, k1 = (k0 + C.W0) & 0xFFFFFFFF, (k1 + C.W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def value_scalar(e, seed, site, step, rank):
    w = philox_scalar((e >> 3, site, step, rank), (seed & 0xFFFFFFFF, seed >> 32))[(e & 7) >> 1]
    return (w >> 16) if e & 1 else (w & 0xFFFF)


class Reference:
    """The implementation under test, as the checks see it; mutants override one piece."""
    rounds = 10
    mutant = {}
    strict = False

    def philox(self, counter, key):
        return tuple(int(w) for w in C.philox4x32(*counter, *key, rounds=self.rounds))

    def mask(self, n, t, seed, site, step, rank):
        return C.mask(n, t, seed, site, step, rank, strict=self.strict, rounds=self.rounds, **self.mutant)

    def threshold_and_scale(self, p):
        return C.threshold_and_scale(p)


# ---- the checks ----------------------------------------------------------------------------------------------
def check_known_answers(impl):
    for counter, key, want in C.KNOWN_ANSWERS:
        got = impl.philox(counter, key)
        assert got == want, (" ".join(f"{w:08x}" for w in got), " ".join(f"{w:08x}" for w in want))


def check_layout(impl):
    # seed 0, site = step = rank = 0: call 0 is the first known answer, 6627e8d5 e169c58d bc57ac4c 9b00dbd8, so by
    # hand e = 0 ... 7 read e8d5 6627 c58d e169 ac4c bc57 dbd8 9b00
    by_hand = [0xe8d5, 0x6627, 0xc58d, 0xe169, 0xac4c, 0xbc57, 0xdbd8, 0x9b00]
    assert [value_scalar(e, 0, 0, 0, 0) for e in range(8)] == by_hand
    # at T = 0x9b00 element 7 sits exactly on the threshold: kept (>=); at T = 0x9b01 it is dropped
    for t, keep7 in ((0x9b00, True), (0x9b01, False)):
        want = [v >= t for v in by_hand]
        assert want == [True, False, True, True, True, True, True, keep7]
        assert impl.mask(8, t, 0, 0, 0, 0).tolist() == want
    # e = 0 ... 15 (two calls) on a stream with every counter and key word in use
    seed, site, step, rank = C.KERNEL_SEED, 5, 7, 2
    vals = [value_scalar(e, seed, site, step, rank) for e in range(16)]
    for t in (C.GOOD_T[0.1], C.GOOD_T[0.5], C.GOOD_T[0.9], sorted(vals)[8]):
        assert impl.mask(16, t, seed, site, step, rank).tolist() == [v >= t for v in vals], t
    for n in (1, 7, 9, 15):      # a partial last call
        assert impl.mask(n, C.GOOD_T[0.5], seed, site, step, rank).tolist() == [v >= C.GOOD_T[0.5] for v in vals[:n]]


def check_threshold_and_scale(impl):
    for p in C.GOOD_PS:
        t, s = impl.threshold_and_scale(p)
        assert t == C.GOOD_T[p] and 0 < t <= C.MAX_T
        want = struct.unpack("f", struct.pack("f", 65536.0 / (65536.0 - t)))[0]      # double, rounded to fp32 once
        assert float(s) == want and float(np.float32(s)) == float(s), (p, float(s), want)
    for p in C.BAD_PS:
        with pytest.raises(ValueError):
            impl.threshold_and_scale(p)


def _masks(impl, p):
    t = C.GOOD_T[p] if p in C.GOOD_T else C.threshold_and_scale(p)[0]
    return t, {s: impl.mask(C.STAT_N, t, C.SEED, *s) for s in C.STAT_STREAMS}


def check_keep_rate(impl):
    worst = 0.0
    for p in C.STAT_PS:
        t, masks = _masks(impl, p)
        q = 1.0 - t / 65536.0
        sigma = math.sqrt(C.STAT_N * q * (1.0 - q))
        for stream, m in masks.items():
            dev = abs(int(m.sum()) - C.STAT_N * q) / sigma
            worst = max(worst, dev)
            assert dev <= C.SIGMAS, (p, stream, dev)
    return worst


def check_independence(impl):
    worst = 0.0
    for p in C.STAT_PS:
        t, masks = _masks(impl, p)
        q = 1.0 - t / 65536.0
        d = 2.0 * q * (1.0 - q)                       # two independent Bernoulli(q) masks disagree with this share
        sigma = math.sqrt(C.STAT_N * d * (1.0 - d))
        base = masks[(0, 1, 0)]
        for stream in ((1, 1, 0), (0, 2, 0), (0, 1, 1)):
            dev = abs(int((base != masks[stream]).sum()) - C.STAT_N * d) / sigma
            worst = max(worst, dev)
            assert dev <= C.SIGMAS, (p, stream, dev)
    return worst


CHECKS = (check_known_answers, check_layout, check_threshold_and_scale, check_keep_rate, check_independence)


# ---- the reference passes ------------------------------------------------------------------------------------
def test_known_answers():
    check_known_answers(Reference())
    for counter, key, want in C.KNOWN_ANSWERS:
        assert philox_scalar(counter, key) == want


def test_element_layout():
    check_layout(Reference())


def test_threshold_and_scale_reference_and_product():
    check_threshold_and_scale(Reference())
    from qarig import dropout as D

    class Product(Reference):
        def threshold_and_scale(self, p):
            return D.threshold_and_scale(p)

    check_threshold_and_scale(Product())
    assert D.MAX_THRESHOLD == C.MAX_T
    for p in (0.003, 0.1, 0.2, 0.333, 0.77, 0.9):
        t, s = D.threshold_and_scale(p)
        tr, sr = C.threshold_and_scale(p)
        assert t == tr and s == float(sr) and type(t) is int and type(s) is float
    assert D.DropoutKey.threshold_and_scale(0.1) == D.threshold_and_scale(0.1)


def test_keep_rate():
    print(f"MEASURED dropout keep-rate worst deviation {check_keep_rate(Reference()):.2f} sigma (bound {C.SIGMAS})")


def test_independence_of_site_step_rank():
    print(f"MEASURED dropout independence worst deviation {check_independence(Reference()):.2f} sigma "
          f"(bound {C.SIGMAS})")


# ---- the mutants are rejected --------------------------------------------------------------------------------
def _mutant(name):
    m = Reference()
    if name.startswith("no_"):
        m.mutant = {"drop": (name[3:],)}
    elif name == "halves_swapped":
        m.mutant = {"swap_halves": True}
    elif name == "strict_compare":
        m.strict = True
    elif name == "scale_from_p":
        m.threshold_and_scale = lambda p: (C.threshold_and_scale(p)[0], np.float32(1.0 / (1.0 - p)))
    elif name == "seven_rounds":
        m.rounds = 7
    return m


@pytest.mark.parametrize("name", ["no_site", "no_step", "no_rank", "halves_swapped", "strict_compare", "scale_from_p",
                                  "seven_rounds"])
def test_mutant_is_rejected(name):
    rejected_by = []
    for check in CHECKS:
        try:
            check(_mutant(name))
        except AssertionError:
            rejected_by.append(check.__name__)
    print(f"mutant {name}: rejected by {rejected_by}")
    assert rejected_by, f"no check tells the mutant {name} from the definition"


def test_command_line_argument_types():
    import argparse
    from qarig import cli_common as cc
    p = argparse.ArgumentParser()
    cc.add_dropout_args(p)
    assert vars(p.parse_args([])) == {"dropout": 0.0, "dropout_seed": 0}
    got = vars(p.parse_args(["--dropout", "0.1", "--dropout-seed", "0x5EED"]))
    assert got == {"dropout": 0.1, "dropout_seed": 0x5EED}
    assert cc.dropout_arg("0") == 0.0 and cc.dropout_arg("0.9") == 0.9
    assert cc.dropout_seed_arg(str(2 ** 64 - 1)) == 2 ** 64 - 1
    for bad in ("0.91", "1", "-0.1", "nan", "1e-6", "x"):
        with pytest.raises(argparse.ArgumentTypeError):
            cc.dropout_arg(bad)
    for bad in ("-1", str(2 ** 64), "1.5", "x"):
        with pytest.raises(argparse.ArgumentTypeError):
            cc.dropout_seed_arg(bad)
    assert cc.check_dropout_args(0.0, 0) == (0.0, 0) and cc.check_dropout_args(0.5, 7) == (0.5, 7)
    for bad in ((0.95, 0), (float("nan"), 0), (0.1, -1), (0.1, 2 ** 64)):
        with pytest.raises(ValueError):
            cc.check_dropout_args(*bad)


# ---- the kernel's own header, compiled for the host ----------------------------------------------------------
HOST_PROGRAM = r'''
#include <stdio.h>
#include "dropout_philox.h"
int main() {
    const uint32_t kat[3][6] = {{0, 0, 0, 0, 0, 0},
                                {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu},
                                {0x243f6a88u, 0x85a308d3u, 0x13198a2e, 0x03707344u, 0xa4093822u, 0x299f31d0u}};
    uint32_t r[4];
    for (int i = 0; i < 3; ++i) {
        qarig::philox4x32_10(kat[i][0], kat[i][1], kat[i][2], kat[i][3], kat[i][4], kat[i][5], r);
        printf("%08x %08x %08x %08x\n", r[0], r[1], r[2], r[3]);
    }
    // keep-bits of e = 0 ... 4095 at three thresholds: seed 0x0123456789abcdef, site 5, step 7, rank 2
    const uint32_t ts[3] = {6554u, 32768u, 58982u};
    for (int t = 0; t < 3; ++t) {
        for (uint32_t e = 0; e < 4096; ++e) {
            qarig::philox4x32_10(e >> 3, 5u, 7u, 2u, 0x89abcdefu, 0x01234567u, r);
            putchar(qarig::dropout_value(r[(e & 7) >> 1], (int)(e & 7), ts[t]) ? '1' : '0');
        }
        putchar('\n');
    }
    printf("%u %d %d\n", QARIG_DROPOUT_MAX_THRESHOLD, QARIG_DROPOUT_BLOCK, QARIG_DROPOUT_MAX_BLOCKS);
    return 0;
}
'''


def test_kernel_header_on_the_host(tmp_path):
    cxx = "/opt/rocm/lib/llvm/bin/clang++"
    assert os.path.exists(cxx)
    src = tmp_path / "philox_host.cpp"
    src.write_text(HOST_PROGRAM)
    exe = str(tmp_path / "philox_host")
    subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-Wno-pass-failed",
                    "-I", os.path.join(PKG, "csrc"), str(src), "-o", exe], check=True, capture_output=True, text=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()
    for line, (_, _, want) in zip(out[:3], C.KNOWN_ANSWERS):
        assert line == " ".join(f"{w:08x}" for w in want)
    for line, t in zip(out[3:6], (6554, 32768, 58982)):
        want = C.mask(4096, t, C.KERNEL_SEED, 5, 7, 2)
        assert line == "".join("1" if k else "0" for k in want)
    from qarig import ops
    t_max, block, blocks = map(int, out[6].split())
    assert t_max == C.MAX_T == ops.DROPOUT_MAX_THRESHOLD and block * blocks * 8 == ops.DROPOUT_SWEEP
