"""Host side of FlatAdam's EMA: the weight schedule against exact fractions, argument checks, and an fp32
emulation of the kernel's two-branch lerp against the error bound the GPU test (tests/test_gpu_ema.py) asserts --
the bound has to be one the specified arithmetic meets before the GPU is asked to meet it."""
import types
from fractions import Fraction

import numpy as np
import pytest

U = 2.0 ** -24          # unit round-off of fp32
STEPS = 5


def ema_w_sets():
    """The per-step weights of the GPU test: the warm-up sequence of decay 0.999 (0.9, 0.818..., ...: the
    w >= 0.5 branch) and {0.3, 0.5, 0.7} cycled (both branches and the boundary)."""
    from qarig.optim import ema_weight
    warm = [ema_weight(c, 0.999, True) for c in range(STEPS)]
    mixed = [float(np.float32(w)) for w in (0.3, 0.5, 0.7, 0.3, 0.5)]
    return {"warmup": warm, "mixed": mixed}


def lerp_f32(e, p, w):
    """The kernel's expression, every operation rounded to fp32 (no contraction, as the library is built)."""
    e, p, w = e.astype(np.float32), p.astype(np.float32), np.float32(w)
    if w < np.float32(0.5):
        return (e + w * (p - e)).astype(np.float32)
    return (p - (p - e) * (np.float32(1.0) - w)).astype(np.float32)


def ema_bound_check(e0, p_steps, e_steps, ws):
    """Worst error, in units of 2^-24 M, of the fp32 EMA sequence `e_steps` against the fp64 recurrence fed the
    same fp32 parameters `p_steps`; M is the largest max(|e|, |p|) each element saw (both sequences)."""
    ref = e0.astype(np.float64)
    M = np.abs(ref)
    for p, w in zip(p_steps, ws):
        p64 = p.astype(np.float64)
        ref = ref + float(w) * (p64 - ref)
        M = np.maximum(M, np.maximum(np.abs(ref), np.abs(p64)))
    for e in e_steps:
        M = np.maximum(M, np.abs(e.astype(np.float64)))
    err = np.abs(e_steps[-1].astype(np.float64) - ref)
    M = np.maximum(M, np.finfo(np.float32).tiny)
    return float((err / (U * M)).max())


@pytest.mark.parametrize("warmup", [True, False])
@pytest.mark.parametrize("decay", [0.9, 0.999, 0.9999])
def test_ema_weight_against_exact_fractions(decay, warmup):
    from qarig.optim import ema_weight
    d = Fraction(decay)              # the double the caller passed, exactly
    for count in (0, 1, 9, 10 ** 3, 10 ** 6):
        want = 1 - (min(d, Fraction(1 + count, 10 + count)) if warmup else d)
        got = ema_weight(count, decay, warmup)
        assert got == float(np.float32(got)), "not an fp32 value"
        # one rounding to double, one to float: half an fp32 ulp plus half a double ulp, relative
        assert abs(Fraction(got) - want) <= want * Fraction(2.0 ** -24 + 2.0 ** -52)
        # never below the asymptotic weight (beyond the one rounding to fp32)
        assert got >= float(np.float32(1.0 - decay))
    if warmup:
        assert ema_weight(0, decay, True) == float(np.float32(0.9))
        assert ema_weight(10 ** 6, 0.9, True) == float(np.float32(1.0 - 0.9))
    else:
        assert ema_weight(0, decay, False) == ema_weight(10 ** 6, decay, False)


def test_ema_weight_is_monotone_down_to_one_minus_decay():
    from qarig.optim import ema_weight
    ws = [ema_weight(c, 0.999, True) for c in range(0, 20000, 7)]
    assert all(a >= b for a, b in zip(ws, ws[1:]))
    assert ws[-1] == float(np.float32(1.0 - 0.999))


@pytest.mark.parametrize("decay", [0.0, 1.0, -0.1, 1.5, float("nan")])
def test_enable_ema_rejects_decay_outside_unit_interval(decay):
    from qarig.optim import FlatAdam
    # the check comes before anything touches the optimizer (a FlatAdam itself needs a GPU)
    with pytest.raises(ValueError):
        FlatAdam.enable_ema(types.SimpleNamespace(), decay)


def test_lerp_emulation_exact_cases():
    rng = np.random.default_rng(0)
    e = rng.standard_normal(1000).astype(np.float32)
    p = rng.standard_normal(1000).astype(np.float32)
    assert np.array_equal(lerp_f32(e, p, 1.0), p)
    assert np.array_equal(lerp_f32(e, p, 0.0), e)
    for w in (0.0, 0.3, 0.5, 0.9, 1.0):
        assert np.array_equal(lerp_f32(e, e.copy(), w), e)


@pytest.mark.parametrize("scale", [1e-3, 1.0, 1e3])
@pytest.mark.parametrize("wset", ["warmup", "mixed"])
def test_fp32_lerp_emulation_meets_the_gpu_tests_bound(wset, scale):
    """Each branch commits at most 3 * 2^-24 * M per step (difference, product, sum; the difference's error is
    scaled by min(w, 1 - w) <= 1/2 of |p - e| <= 2M), earlier error contracts by (1 - w): 4 * T * 2^-24 * M
    covers T steps with room for second-order terms."""
    ws = ema_w_sets()[wset]
    rng = np.random.default_rng(1)
    n = 1 << 16
    e0 = (rng.standard_normal(n) * scale).astype(np.float32)
    p = (rng.standard_normal(n) * scale).astype(np.float32)
    e, p_steps, e_steps = e0, [], []
    for w in ws:
        # parameters that move like an Adam step of lr 1e-3 * scale, mixed signs
        p = (p + np.float32(1e-3 * scale) * np.sign(rng.standard_normal(n)).astype(np.float32)).astype(np.float32)
        e = lerp_f32(e, p, w)
        p_steps.append(p)
        e_steps.append(e)
    worst = ema_bound_check(e0, p_steps, e_steps, ws)
    print(f"{wset} scale {scale}: worst {worst:.3f} x 2^-24 M (bound {4 * STEPS})")
    assert worst <= 4 * STEPS
