"""Host side of global-norm gradient clipping (qarig_grad_clip_coef, qarig_adam_clip_step,
FlatAdam.enable_grad_clip, --clip-grad-norm / --max-skipped-steps): the fp64 definition against
torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW, the NumPy emulation of both kernels against the tolerances the
GPU tests assert (tests/grad_clip_cases.py derives them), the mutants those tolerances must reject, and the flag
checks.  No GPU."""
import math
import os
import re
import types

import numpy as np
import pytest
import torch

import adamw_cases as A
import grad_clip_cases as C
from conftest import PKG

CASES = list(C.cases())


# ---- the definition ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("betas", A.BETAS)
def test_definition_is_clip_grad_norm_then_adamw(betas):
    """Five steps in double on the CPU, two parameter groups (decayed / not), one global clip over both.  The
    gradients alternate between a norm above the threshold and one below it."""
    rng = np.random.default_rng(11)
    n, steps, lam, max_norm = 64 + 5, 5, 0.1, 4.0
    p0 = rng.standard_normal(n)
    grads = [rng.standard_normal(n) * (1.0 if t % 2 == 0 else 0.25) for t in range(steps)]
    mask = (rng.random((n + 7) // 8) < 0.5).astype(np.uint8)
    mask[-1] = 1
    dec = A.element_mask(mask, n)
    a = torch.nn.Parameter(torch.from_numpy(p0[dec].copy()))
    b = torch.nn.Parameter(torch.from_numpy(p0[~dec].copy()))
    opt = torch.optim.AdamW([dict(params=[a], weight_decay=lam), dict(params=[b], weight_decay=0.0)], lr=A.LR,
                            betas=betas, eps=A.EPS)
    scalars = [dict(step_size=A.LR / (1 - betas[0] ** t), bc2_sqrt=math.sqrt(1 - betas[1] ** t), ema_w=0.0,
                    decay=A.LR * lam) for t in range(1, steps + 1)]
    # coefficients in double here (the fp32 rounding of coef is the entry's, checked on the emulation below)
    norms = [C.norm_ref64(g) for g in grads]
    coefs = [min(1.0, max_norm / (x + 1e-6)) for x in norms]
    assert any(c < 1 for c in coefs) and any(c == 1 for c in coefs)
    ref = C.clip_adamw_ref64(p0, grads, mask, scalars, betas[0], betas[1], A.EPS, 1.0, max_norm, coefs=coefs)
    for t, g in enumerate(grads):
        a.grad = torch.from_numpy(g[dec].copy())
        b.grad = torch.from_numpy(g[~dec].copy())
        total = torch.nn.utils.clip_grad_norm_([a, b], max_norm)
        assert abs(float(total) - norms[t]) <= 1e-12 * norms[t]
        opt.step()
        want = np.empty(n)
        want[dec], want[~dec] = a.detach().numpy(), b.detach().numpy()
        rel = np.abs(ref[t]["p"] - want).max() / np.abs(want).max()
        assert rel <= 1e-12, (t, rel)
        assert abs(C.coef_def(norms[t], max_norm) - coefs[t]) <= 2.0 ** -24 * coefs[t]
    unclipped = A.adamw_ref64(p0, grads, mask, scalars, betas[0], betas[1], A.EPS)
    assert np.abs(unclipped[-1]["m"] - ref[-1]["m"]).max() > 1e-3        # the clip did something


def test_coefficient_rule():
    assert C.coef_def(10.0, float("inf")) == 1.0
    assert C.coef_def(0.0, 1.0) == 1.0                      # 1 / 1e-6 clamps to 1
    assert C.coef_def(2.0, 1.0) == A.f32(1.0 / (2.0 + 1e-6))
    assert C.coef_def(1.0, 1.0) == A.f32(1.0 / (1.0 + 1e-6)) < 1.0
    assert C.coef_def(float("inf"), 1.0) == 0.0 and C.coef_def(float("nan"), 1.0) == 0.0


def test_skip_rule_of_the_definition():
    x = C.make_inputs(CASES[0], nan_step=1)
    ref = C.clip_adamw_ref64(x["p"], x["grads"], x["mask"], x["scalars"], x["beta1"], x["beta2"], x["eps"],
                             x["grad_scale"], x["max_norm"], ema=x["ema"])
    assert [r["skipped"] for r in ref] == [False, True, False]
    for k in ("p", "m", "v", "ema"):
        assert np.array_equal(ref[0][k], ref[1][k]) and not np.array_equal(ref[1][k], ref[2][k])
    first = C.clip_adamw_ref64(x["p"], x["grads"][1:], x["mask"], x["scalars"][1:], x["beta1"], x["beta2"], x["eps"],
                               x["grad_scale"], x["max_norm"], ema=x["ema"])
    assert first[0]["skipped"] and np.array_equal(first[0]["p"], x["p"].astype(np.float64))
    assert not first[0]["m"].any() and np.array_equal(first[0]["ema"], x["ema"].astype(np.float64))


# ---- the norm: bound, emulation, the fp32 mutant ---------------------------------------------------------------
def test_norm_bound_is_below_2_pow_minus_40_at_every_test_size():
    for n in C.NORM_SIZES + [4101, 78_226_440]:
        assert C.bound_norm(n) < 2.0 ** -40, n
    assert C.grid(C.SWEEP) == (C.PARTIALS, 1) and C.grid(C.SWEEP + 1) == (C.PARTIALS, 2)
    assert C.grid(3 * C.SWEEP + 7)[1] == 4 and C.grid(1) == (1, 1) and C.grid(1025) == (2, 1)


def test_library_constant_matches_the_header():
    src = open(os.path.join(PKG, "csrc", "optim.hip")).read()
    assert int(re.search(r"GRAD_NORM_PARTIALS\s*=\s*(\d+)\s*;", src).group(1)) == C.PARTIALS
    from qarig import ops
    assert ops.GRAD_NORM_PARTIALS == C.PARTIALS


@pytest.mark.parametrize("n", [1, 3, 4, 5, 255, 257, 1023, 1025, 4101, 3 * 1024 + 2, C.SWEEP + 1])
def test_norm_emulation_meets_its_bound_and_fp32_accumulation_does_not(n):
    rng = np.random.default_rng(n)
    worst32 = 0.0
    for scale in (1.0, 2.0 ** -10, 2.0 ** 10):
        for gs in (1.0, 0.5, 2.0 ** -10):
            g = (rng.standard_normal(n) * scale).astype(np.float32)
            ref = C.norm_ref64(g, gs)
            got = C.norm_emulate(g, gs)
            assert abs(got - ref) <= C.bound_norm(n) * ref, (n, scale, gs, got, ref)
            worst32 = max(worst32, abs(C.norm_emulate(g, gs, np.float32) - ref) / (C.bound_norm(n) * ref))
    if n >= 255:
        assert worst32 > 1.0, worst32           # the fp32 accumulator leaves the bound (by orders of magnitude)
        print(f"n={n}: fp32 accumulation off by {worst32:.3g} bounds")


def test_norm_emulation_on_exact_and_extreme_data():
    for j, k in ((0, 0), (1, 3), (5, -7), (8, 10), (10, 0)):
        g, want = C.exact_power_data(j, k)
        assert C.norm_emulate(g) == want == C.norm_ref64(g)
    big = np.full(1025, 1e30, np.float32)
    assert math.isfinite(C.norm_emulate(big)) and not math.isfinite(C.norm_emulate(big, accum=np.float32))
    assert C.coef_def(C.norm_emulate(big), 1.0) > 0.0
    small = np.full(1025, 1e-30, np.float32)
    assert C.norm_emulate(small) > 0.0 and C.norm_emulate(small, accum=np.float32) == 0.0
    for bad in (np.nan, np.inf, -np.inf):
        for at in (0, 1024, 1023):
            g = np.ones(1025, np.float32)
            g[at] = bad
            assert not math.isfinite(C.norm_emulate(g))


# ---- the chain: emulation inside, mutants outside ------------------------------------------------------------
def _chain(case, mutant=None, nan_step=None, with_ema=True):
    x = C.make_inputs(case, nan_step=nan_step)
    ema = x["ema"] if with_ema else None
    got = C.clip_emulate32(x["p"], x["grads"], x["mask"], x["scalars"], x["beta1"], x["beta2"], x["eps"],
                           x["grad_scale"], x["max_norm"], ema=ema, mutant=mutant)
    # the correct arithmetic is compared with the definition fed its own coefficient (as the GPU tests do); a
    # mutant with the definition's own
    own = mutant is None
    ref = C.clip_adamw_ref64(x["p"], x["grads"], x["mask"], x["scalars"], x["beta1"], x["beta2"], x["eps"],
                             x["grad_scale"], x["max_norm"], ema=ema,
                             coefs=[g["coef"] for g in got] if own else None,
                             norms=[g["norm"] for g in got] if own else None)
    return x, ref, got


@pytest.mark.parametrize("nan_step", [None, 1])
@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_emulation_meets_the_tolerances(case, nan_step):
    x, ref, got = _chain(case, nan_step=nan_step)
    r = C.worst_ratios(ref, got)
    print("emulation {}: worst / bound  p {:.4f}  m {:.4f}  v {:.4f}  ema {:.4f}".format(
        case["id"], r["p"], r["m"], r["v"], r["ema"]))
    assert all(0.0 <= v <= 1.0 for v in r.values()), r
    assert r["p"] > 0 and r["m"] > 0 and r["v"] > 0 and r["ema"] > 0
    for t, g in enumerate(got):
        if nan_step == t:
            assert g["skipped"] and g["coef"] == 0.0
            continue
        want = C.norm_ref64(x["grads"][t], x["grad_scale"])
        assert abs(g["norm"] - want) <= C.bound_norm(4101) * want
        assert g["coef"] == C.coef_def(g["norm"], x["max_norm"])
    if nan_step is None:        # by construction: the outer steps clip, the middle one does not
        assert [g["coef"] < 1 for g in got] == [True, False, True]
    else:
        for k in ("p", "m", "v", "ema"):
            assert np.array_equal(got[0][k].view(np.int32), got[1][k].view(np.int32))


# ---- the emulation is the source: csrc/adam_element.h on the host, called as the clip instantiation calls it -----
@pytest.fixture(scope="module")
def element_exe(tmp_path_factory):
    return A.build_element_program(tmp_path_factory.mktemp("adam_element"))


@pytest.mark.parametrize("nan_step", [None, 1])
@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_kernel_element_on_the_host_is_the_emulation(case, nan_step, element_exe):
    """The kernels' element function compiled for the host, fed what adam_groups_kernel<*, true> feeds it: the
    gradient argument fp32(g * grad_scale), the scale argument coef, norm and coef those of clip_emulate32's own
    step; a step with a norm that is not finite leaves the state alone.  p, m, v and ema after every step carry
    clip_emulate32's bits."""
    x = C.make_inputs(case, nan_step=nan_step)
    want = C.clip_emulate32(x["p"], x["grads"], x["mask"], x["scalars"], x["beta1"], x["beta2"], x["eps"],
                            x["grad_scale"], x["max_norm"], ema=x["ema"])
    steps = [dict(s, g=g, pre=x["grad_scale"], scale=w["coef"], skipped=not math.isfinite(w["norm"]))
             for g, s, w in zip(x["grads"], x["scalars"], want)]
    assert [s["skipped"] for s in steps] == [t == nan_step for t in range(C.STEPS)]
    got = A.run_element_program(element_exe, x["p"], x["ema"], A.element_mask(x["mask"], x["p"].shape[0]),
                                x["beta1"], x["beta2"], x["eps"], steps, clip=True)
    for t, (a, b) in enumerate(zip(got, want)):
        for k in ("p", "m", "v", "ema"):
            assert np.array_equal(a[k], b[k].view(np.uint32)), (t, k)
    assert not np.array_equal(got[-1]["p"], x["p"].view(np.uint32))


def _rejected(case, mutant):
    """Does the mutant leave a tolerance on this case?  The norm's for the accumulation mutant, the chain's for
    the others (with a NaN in the second step for the two skip mutants)."""
    if mutant == "fp32_accumulation":
        x, _, got = _chain(case, mutant)
        return max(abs(g["norm"] - C.norm_ref64(gr, x["grad_scale"])) /
                   (C.bound_norm(4101) * C.norm_ref64(gr, x["grad_scale"])) for g, gr in zip(got, x["grads"]))
    nan_step = 1 if mutant.startswith("skip_") else None
    _, ref, got = _chain(case, mutant, nan_step=nan_step)
    return max(C.worst_ratios(ref, got).values())


@pytest.mark.parametrize("mutant", C.MUTANTS)
def test_tolerances_reject_the_mutant(mutant):
    rejected = {}
    for case in CASES:
        r = _rejected(case, mutant)
        if not r <= 1.0:
            rejected[case["id"]] = r
    print(f"{mutant}: rejected on {len(rejected)} of {len(CASES)} cases, worst ratio "
          f"{max(rejected.values(), default=0.0):.3g}")
    for case in CASES:
        # the unscaled norm is the right one at grad_scale 1: it must fall wherever the scale is not 1
        if mutant != "norm_unscaled" or case["grad_scale"] != 1.0:
            assert case["id"] in rejected, (mutant, case["id"])
    assert rejected


def test_mutants_list_is_the_one_the_feature_names():
    assert set(C.MUTANTS) == {"norm_unscaled", "coef_unclamped", "coef_twice", "per_parameter_norms",
                              "fp32_accumulation", "skip_decays_moments", "skip_per_element"}


# ---- flags and the optimizer's argument checks ---------------------------------------------------------------
def test_clip_flag_parsing():
    import argparse
    from qarig import cli_common as cc
    p = argparse.ArgumentParser()
    cc.add_grad_clip_args(p)
    d = vars(p.parse_args([]))
    assert d["clip_grad_norm"] is None and d["max_skipped_steps"] == 10
    d = vars(p.parse_args(["--clip-grad-norm", "1.5", "--max-skipped-steps", "0"]))
    assert d["clip_grad_norm"] == 1.5 and d["max_skipped_steps"] == 0
    assert vars(p.parse_args(["--clip-grad-norm", "inf"]))["clip_grad_norm"] == float("inf")
    for bad in (["--clip-grad-norm", "0"], ["--clip-grad-norm", "-1"], ["--clip-grad-norm", "nan"],
                ["--clip-grad-norm", "x"], ["--clip-grad-norm", "-inf"], ["--max-skipped-steps", "-1"],
                ["--max-skipped-steps", "1.5"], ["--max-skipped-steps", "x"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)


def test_check_grad_clip_args():
    from qarig import cli_common as cc
    assert cc.check_grad_clip_args(None, 10) == (None, 10)
    assert cc.check_grad_clip_args(2, 0) == (2.0, 0)
    assert cc.check_grad_clip_args(float("inf"), 3) == (float("inf"), 3)
    for bad in [(0.0, 10), (-1.0, 10), (float("nan"), 10), (1.0, -1), (1.0, 1.5), (None, -2), (1.0, True)]:
        with pytest.raises(ValueError):
            cc.check_grad_clip_args(*bad)


@pytest.mark.parametrize("c", [0.0, -1.0, float("nan"), -float("inf")])
def test_enable_grad_clip_rejects_values_outside_its_range(c):
    from qarig.optim import FlatAdam
    with pytest.raises(ValueError):         # the check comes before anything touches the optimizer
        FlatAdam.enable_grad_clip(types.SimpleNamespace(), c)


def test_clip_stats_needs_the_clip():
    from qarig.optim import FlatAdam
    with pytest.raises(RuntimeError, match="enable_grad_clip"):
        FlatAdam.clip_stats(types.SimpleNamespace(clip_max_norm=None))
