"""Shared by tests/test_grad_clip_host.py and tests/test_gpu_grad_clip*.py (no GPU needed to import): the fp64
definition of qarig_grad_clip_coef and qarig_adam_clip_step (include/qarig.h), a NumPy emulation of both kernels in
their operation order (with the mutants the host test must see rejected), the shared inputs and the tolerances.

The definition.  s_i = fp32(g_i * grad_scale) (the value Adam uses), norm = sqrt(sum s_i^2) in fp64,
coef = fp32(min(1, max_norm / (norm + 1e-6))), a norm that is not finite skips the step (p, m, v, ema keep their
values), otherwise adamw_cases.adamw_ref64 with gi = g * grad_scale * coef in fp64.

Tolerance of the norm, with u64 = 2^-53.  Every term is >= 0 and exact (the square of a 24-bit value), so a sum of
A additions in any fixed order is off by at most A u64 relative (each addition (1 + d), |d| <= u64, on a
non-negative partial sum; A u64 << 1, second order left to the slack below).  The documented order gives, for n
elements on B = min(ceil(n / 1024), PARTIALS) workgroups:
    per lane   4 * trips + 3      trips = ceil(ceil(n / 4) / (256 B)) vectors of 4 elements, plus the n % 4 tail
    butterfly  6,   waves 3       stage 1
    stage 2    ceil(B / 256) + 6 + 3
The root halves the relative error of the sum and adds one rounding.  The reference the tests compare with is
itself a pairwise fp64 sum (at most log2(n) <= 40 roundings on the sum, 20 on the norm) and a root: 21 units, and
the test's subtraction is exact to first order.  So
    |norm - ref| <= (A / 2 + 1 + 21 + 1) u64 |ref|            (one unit of slack for the second order)
which is below 2^-40 at every size the tests use (asserted in test_grad_clip_host.py): an fp32 accumulator, off by
2^-24 per addition, cannot pass.

Tolerances of the Adam outputs: adamw_cases's counts with gi carrying TWO roundings (g * grad_scale, then * coef)
where it carried one; coef itself is an input of both sides (the definition is fed the checked sequence's own
coefficient), so it contributes nothing.
  m   gi enters once:                      (3 + 1) T -> (4 + 1) T                              bound_m = 5 T
  v   gi enters twice:                     (5 + 1) T -> (7 + 1) T                              bound_v = 8 T
  p   mn carries 5 t u S (was 4 t), denom half of v's relative error, 4 t (was 3 t), plus 3; the quotient and the
      product 2: |d upd| <= (9 t + 5) u S; pd and pn one rounding each, the old error passes: per step
      (9 t + 5 + 2 + 1) u M_p, summed over t = 1 ... T:                                 bound_p = 4.5 T (T + 1) + 8 T
  ema as adamw_cases:                                                                   bound_ema = bound_p + 4 T
A skipped step adds nothing on either side (T still counts it: the bounds only grow).  Nothing here was fitted to
what a GPU gives."""
import math
import os
import re

import numpy as np

import adamw_cases as A

U = A.U
U64 = 2.0 ** -53
BLOCK = 256
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARTIALS = int(re.search(r"#define\s+QARIG_GRAD_NORM_PARTIALS\s+(\d+)",
                         open(os.path.join(ROOT, "include", "qarig.h")).read()).group(1))
SWEEP = PARTIALS * 4 * BLOCK            # elements one trip of the capped grid covers
NORM_SIZES = [1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, SWEEP - 1, SWEEP, SWEEP + 1, 3 * SWEEP + 7]
STEPS = A.STEPS
MAX_NORM = 20.0                         # against gradient norms of about 61, 15 and 61 times grad_scale
PARAM_SPLIT = (0, 1000, 3000)           # where the "parameters" of the per-parameter mutant start


def f32(x):
    return A.f32(x)


def bound_m(T):
    return 5.0 * T


def bound_v(T):
    return 8.0 * T


def bound_p(T):
    return 4.5 * T * (T + 1) + 8.0 * T


def bound_ema(T):
    return bound_p(T) + 4.0 * T


def grid(n):
    """(workgroups, trips per lane) of the norm kernel at n elements."""
    blocks = min((n + 4 * BLOCK - 1) // (4 * BLOCK), PARTIALS)
    nvec = (n + 3) // 4
    return blocks, (nvec + blocks * BLOCK - 1) // (blocks * BLOCK)


def norm_additions(n):
    blocks, trips = grid(n)
    return (4 * trips + 3) + 6 + 3 + ((blocks + BLOCK - 1) // BLOCK + 6 + 3)


def bound_norm(n):
    """Relative bound on |norm - pairwise fp64 reference|, in absolute terms (not units of u64)."""
    return (norm_additions(n) / 2.0 + 1.0 + 21.0 + 1.0) * U64


# ---- the definition ------------------------------------------------------------------------------------------
def scaled64(g, grad_scale):
    """s_i as fp64: fp32(g_i * grad_scale) for fp32 data (NumPy or torch), the plain product for fp64 data."""
    if isinstance(g, np.ndarray):
        if g.dtype == np.float32:
            return (g * np.float32(grad_scale)).astype(np.float64)
        return g.astype(np.float64) * float(grad_scale)
    import torch
    if g.dtype == torch.float32:
        return (g * float(grad_scale)).double()      # (a Python scalar keeps the fp32 product)
    return g.double() * float(grad_scale)


def norm_ref64(g, grad_scale=1.0):
    s = scaled64(g, grad_scale)
    return float(np.sqrt((s * s).sum())) if isinstance(s, np.ndarray) else float((s * s).sum().sqrt())


def coef_def(norm, max_norm):
    """fp32(min(1, max_norm / (norm + 1e-6))) evaluated in double; 0 for a norm that is not finite."""
    if not math.isfinite(norm):
        return 0.0
    return f32(min(1.0, float(max_norm) / (norm + 1e-6)))


def _maxima(prev, new):
    if prev is None:
        return new
    mx = A._xp(new["p"])[3]
    for k in ("Mm", "Mv", "Mp", "Me"):
        if new[k] is not None:
            new[k] = mx(new[k], prev[k])
    return new


def clip_adamw_ref64(p, grads, mask, scalars, beta1, beta2, eps, grad_scale, max_norm, ema=None, coefs=None,
                     norms=None):
    """The definition chained over len(grads) steps.  coefs / norms: per step, the coefficient and norm to use in
    the place of the definition's own (the checked sequence's: its rounding of the norm is checked separately).
    Returns one dict per step as adamw_ref64 (running maxima carried across the steps) plus norm, coef, skipped."""
    n = p.shape[0]
    zero_mask = mask
    if mask is None and isinstance(p, np.ndarray):
        zero_mask = np.zeros((n + 7) // 8, np.uint8)
    elif mask is None:
        import torch
        zero_mask = torch.zeros((n + 7) // 8, dtype=torch.uint8, device=p.device)
    out, cur = [], None
    for t, (g, s) in enumerate(zip(grads, scalars)):
        norm = norm_ref64(g, grad_scale) if norms is None else float(norms[t])
        coef = coef_def(norm, max_norm) if coefs is None else float(coefs[t])
        if not math.isfinite(norm):
            if cur is None:         # skipped before any step: the inputs, zero moments
                z = A.adamw_ref64(p, [p * 0.0], zero_mask, [dict(s, step_size=0.0, decay=0.0, ema_w=0.0)], beta1,
                                  beta2, eps, 1.0, ema=ema)[0]
                cur = z
            out.append(dict(cur, norm=norm, coef=coef, skipped=True))
            continue
        step = A.adamw_ref64(p if cur is None else cur["p"], [g], zero_mask, [s], beta1, beta2, eps,
                             float(grad_scale) * coef, ema=ema if cur is None else cur["ema"],
                             m=None if cur is None else cur["m"], v=None if cur is None else cur["v"])[0]
        cur = _maxima(cur, step)
        out.append(dict(cur, norm=norm, coef=coef, skipped=False))
    return out


# ---- the kernels' arithmetic, operation by operation ---------------------------------------------------------
def _butterfly(x):
    """x: (..., 64) -> every lane's sum after the xor butterfly with offsets 32 ... 1."""
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        x = x + x[..., lane ^ o]
    return x


def _block_sum(acc):
    """acc: (blocks, 256) per-thread accumulators -> (blocks,) in the kernel's order."""
    w = _butterfly(acc.reshape(acc.shape[0], 4, 64))[..., 0]
    return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]


def norm_emulate(g, grad_scale=1.0, accum=np.float64):
    """qarig_grad_clip_coef's norm in the documented order.  accum = np.float32 is the mutant that accumulates
    the squares in fp32 (terms, partials and all)."""
    n = g.shape[0]
    s = (g.astype(np.float32) * np.float32(grad_scale)).astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        sq = (s.astype(accum) * s.astype(accum)).astype(accum)
        blocks, trips = grid(n)
        lanes = blocks * BLOCK
        nvec = n // 4
        rows = np.zeros((trips * lanes, 4), accum)           # (adding +0 changes no bit of a sum >= 0)
        rows[:nvec] = sq[:4 * nvec].reshape(nvec, 4)
        rows = rows.reshape(trips, lanes, 4)
        acc = np.zeros(lanes, accum)
        for t in range(trips):
            for k in range(4):
                acc = acc + rows[t, :, k]
        for i in range(4 * nvec, n):
            acc[nvec % lanes] = acc[nvec % lanes] + sq[i]
        partials = _block_sum(acc.reshape(blocks, BLOCK))
        rounds = (blocks + BLOCK - 1) // BLOCK
        pad = np.zeros(rounds * BLOCK, accum)
        pad[:blocks] = partials
        acc2 = np.zeros(BLOCK, accum)
        for r in range(rounds):
            acc2 = acc2 + pad[r * BLOCK:(r + 1) * BLOCK]
        total = _block_sum(acc2.reshape(1, BLOCK))[0]
        return float(np.sqrt(np.float64(total)))


MUTANTS = ("norm_unscaled", "coef_unclamped", "coef_twice", "per_parameter_norms", "fp32_accumulation",
           "skip_decays_moments", "skip_per_element")


def clip_emulate32(p, grads, mask, scalars, beta1, beta2, eps, grad_scale, max_norm, ema=None, mutant=None):
    """Both kernels in NumPy, step by step: the norm in its order, the coefficient in double rounded once, then
    adamw_emulate32 on the pre-scaled gradient fp32(g * grad_scale) with coef in grad_scale's place (the kernel's
    two roundings).  Returns one dict(p, m, v, ema, norm, coef, skipped) per step."""
    F = np.float32
    n = p.shape[0]
    zero_mask = mask if mask is not None else np.zeros((n + 7) // 8, np.uint8)
    cur = dict(p=p.astype(F), m=np.zeros(n, F), v=np.zeros(n, F), ema=None if ema is None else ema.astype(F))
    out = []
    for g, s in zip(grads, scalars):
        gs_norm = 1.0 if mutant == "norm_unscaled" else grad_scale
        norm = norm_emulate(g, gs_norm, np.float32 if mutant == "fp32_accumulation" else np.float64)
        skipped = not math.isfinite(norm)
        if skipped:
            coef = np.full(n, 0.0)
        elif mutant == "per_parameter_norms":
            coef = np.empty(n)
            edges = [e for e in PARAM_SPLIT if e < n] + [n]
            for lo, hi in zip(edges, edges[1:]):
                coef[lo:hi] = coef_def(norm_emulate(g[lo:hi], grad_scale), max_norm)
        elif mutant == "coef_unclamped":
            coef = np.full(n, f32(float(max_norm) / (norm + 1e-6)))
        else:
            coef = np.full(n, coef_def(norm, max_norm))
        with np.errstate(over="ignore", invalid="ignore"):
            pre = (g.astype(F) * F(grad_scale)).astype(F)
            if mutant == "coef_twice":
                pre = (pre * coef.astype(F)).astype(F)
            pre = (pre * coef.astype(F)).astype(F)          # the second rounding; adamw_emulate32 then multiplies by 1
        if skipped and mutant == "skip_decays_moments":
            nxt = A.adamw_emulate32(cur["p"], [np.zeros(n, F)], zero_mask, [dict(s, step_size=0.0, decay=0.0,
                                                                                 ema_w=0.0)], beta1, beta2, eps,
                                    1.0, ema=cur["ema"], m=cur["m"], v=cur["v"])[0]
            nxt["p"] = cur["p"]
        elif skipped and mutant == "skip_per_element":
            ok = np.isfinite(g)
            with np.errstate(invalid="ignore"):
                full = A.adamw_emulate32(cur["p"], [np.where(ok, g, 0).astype(F) * F(grad_scale)], zero_mask, [s],
                                         beta1, beta2, eps, 1.0, ema=cur["ema"], m=cur["m"], v=cur["v"])[0]
            nxt = {k: (None if full[k] is None else np.where(ok, full[k], cur[k])) for k in ("p", "m", "v", "ema")}
        elif skipped:
            nxt = dict(cur)
        else:
            nxt = A.adamw_emulate32(cur["p"], [pre], zero_mask, [s], beta1, beta2, eps, 1.0, ema=cur["ema"],
                                    m=cur["m"], v=cur["v"])[0]
        cur = nxt
        out.append(dict(cur, norm=norm, coef=float(coef[0]), skipped=skipped))
    return out


def worst_ratios(ref_steps, got_steps):
    """adamw_cases.worst_ratios with this file's bounds: {output: worst |got - ref| / (bound(T) u M)}."""
    ab, _, _, maximum, _ = A._xp(ref_steps[0]["p"])
    is_np = isinstance(ref_steps[0]["p"], np.ndarray)
    f64 = (lambda a: a.astype(np.float64)) if is_np else (lambda a: a.double())
    tiny = float(np.finfo(np.float32).tiny)
    worst = {"p": 0.0, "m": 0.0, "v": 0.0, "ema": 0.0}
    seen = {k: None for k in worst}
    for T, (r, g) in enumerate(zip(ref_steps, got_steps), 1):
        for key, mag, bound in (("p", "Mp", bound_p), ("m", "Mm", bound_m), ("v", "Mv", bound_v),
                                ("ema", "Me", bound_ema)):
            if r[key] is None or g.get(key) is None:
                continue
            got = f64(g[key])
            seen[key] = ab(got) if seen[key] is None else maximum(seen[key], ab(got))
            M = maximum(maximum(r[mag], seen[key]), r[mag] * 0.0 + tiny)
            ratio = float((ab(got - r[key]) / (bound(T) * U * M)).max())
            if not ratio <= worst[key]:         # (a NaN takes the place)
                worst[key] = ratio
    return worst


# ---- the shared inputs ---------------------------------------------------------------------------------------
def cases():
    return A.cases()


def make_inputs(case, n=4101, steps=STEPS, nan_step=None):
    """adamw_cases.make_inputs with the second step's gradient a quarter of the others (so that under MAX_NORM
    the first and third steps clip and the second does not, at grad_scale 1 and 0.5 alike), and, for
    nan_step = t (0-based), one NaN in that step's gradient."""
    x = A.make_inputs(case, n=n, steps=steps)
    if steps > 1:
        x["grads"][1] = x["grads"][1] * np.float32(0.25)
    if nan_step is not None:
        x["grads"][nan_step] = x["grads"][nan_step].copy()
        x["grads"][nan_step][n // 3] = np.nan
    x["max_norm"] = MAX_NORM
    return x


def exact_power_data(j, k):
    """4^j entries equal to 2^k: the norm is 2^(k + j) exactly, in any summation order."""
    return np.full(4 ** j, 2.0 ** k, np.float32), 2.0 ** (k + j)
