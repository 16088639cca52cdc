"""Shared by tests/test_adamw_host.py and tests/test_gpu_adamw*.py (no GPU needed to import): the definition of
qarig_adamw_step (include/qarig.h) in fp64, an fp32 NumPy emulation of the kernel in its operation order (with the
mutants the host test must see rejected), the shared inputs, and the tolerances.

The reference is the definition evaluated in fp64 ON THE fp32 SCALARS THE ENTRY RECEIVES (beta1, beta2, eps,
step_size, bc2_sqrt, ema_w, decay, grad_scale): how the host rounds lr / (1 - beta1^t) and lr * lambda to fp32 is
not the kernel's error and is checked separately (against torch.optim.AdamW, in double).

Tolerances, counted in roundings of u = 2^-24 relative to the magnitude sum of the terms of each output, for
step T of a chain that starts from exact inputs.  Every count below is the first-order count plus one unit per
step for what the first order leaves out (magnitudes taken as running maxima, products of errors).

  m   gi = g * grad_scale (1 rounding, enters with weight w or 1 - (1 - w) = w), gi - m (1), the product (1), the
      sum (1); 1 - beta1 and 1 - w are exact for beta1 in [0.5, 1) (Sterbenz).  With M_m = |m_old| + |gi| each is
      at most u M_m and the weights sum to at most 3 (w <= 1/2 in the first branch, 1 - w <= 1/2 in the second);
      the error m carries in contracts by beta1.                                 |dm|  <= (3 + 1) T  u M_m
  v   terms v beta2 and (1 - beta2) gi gi, all positive, so M_v = vn: gi twice (2), two products (2), v beta2 (1),
      the sum (1), against vn at most 5 u vn; the old error contracts by beta2.  |dv|  <= (5 + 1) T  u M_v
  p   upd = step_size (mn / denom), denom = sqrt(vn) / bc2_sqrt + eps.  mn carries (3 + 1) t u M_m, i.e.
      4 t u S with S = step_size M_m / denom >= |upd|; denom carries half of v's relative error (3 t u) plus
      the root, the quotient and the sum (3 u); the quotient mn / denom and the product by step_size add 2 u:
      |d upd| <= (7 t + 5) u S.  pd = fma(-decay, p, p) is one rounding (u |pd|), pn = pd - upd one more
      (u |pn|), the old error of p passes through (1 - decay) <= 1.  With M_p = max(|p_old|, |pn|) + S, per
      step (7 t + 5 + 2 + 1) u M_p, summed over t = 1 ... T:                     |dp|  <= (3.5 T (T + 1) + 8 T)  u M_p
  ema the two-branch lerp commits at most 3 u max(|e|, |pn|) per step (tests/test_ema_host.py), takes in pn's
      error with weight ema_w <= 1 and contracts its own by 1 - ema_w:           |de|  <= (bound_p(T) + 4 T)  u M_e
      with M_e = max(M_p, |e| seen so far).

All magnitudes are per element and running maxima over the steps so far, over the reference and the checked
sequence both.  Nothing here was fitted to what a GPU gives; tests/test_adamw_host.py checks that the emulation
(the specified arithmetic) stays inside, and the GPU tests print their worst figures before asserting."""
import math
import struct

import numpy as np

U = 2.0 ** -24
STEPS = 3
LR = 1e-3
EPS = 1e-8
LAMBDAS = (1e-2, 0.1, 1.0)
BETAS = ((0.5, 0.999), (0.9, 0.999))
SCALES = (1.0, 2.0 ** -10, 2.0 ** 10)
EMA_WS = (0.9, 0.3, 0.5)            # both branches of the lerp and the boundary


def f32(x):
    """The double x rounded to fp32 once, as a Python float."""
    return struct.unpack("f", struct.pack("f", float(x)))[0]


def bound_m(T):
    return 4.0 * T


def bound_v(T):
    return 6.0 * T


def bound_p(T):
    return 3.5 * T * (T + 1) + 8.0 * T


def bound_ema(T):
    return bound_p(T) + 4.0 * T


def step_scalars(t, lr, lam, betas, ema_w=0.0):
    """The fp32 scalars FlatAdam hands the entry at 1-based step t: each computed in double, rounded once."""
    b1, b2 = betas
    return dict(step_size=f32(lr / (1 - b1 ** t)), bc2_sqrt=f32(math.sqrt(1 - b2 ** t)), ema_w=f32(ema_w),
                decay=f32(lr * lam))


def _xp(x):
    """(abs, sqrt, where, maximum, repeat-each-8) of the array library x belongs to: NumPy or torch."""
    if isinstance(x, np.ndarray):
        return np.abs, np.sqrt, np.where, np.maximum, lambda a: np.repeat(a, 8)
    import torch
    return torch.abs, torch.sqrt, torch.where, torch.maximum, lambda a: torch.repeat_interleave(a, 8)


def element_mask(mask, n):
    """Per element: is it decayed?  mask has ceil(n / 8) entries, one per group of 8."""
    rep = _xp(mask)[4]
    return rep(mask != 0)[:n]


def adamw_ref64(p, grads, mask, scalars, beta1, beta2, eps, grad_scale=1.0, ema=None, m=None, v=None):
    """The definition, chained over len(grads) steps in fp64.  p, grads[t], ema, m, v: arrays (NumPy or torch) of
    n elements, converted to fp64 here; mask: ceil(n / 8) group flags; scalars[t]: dict(step_size, bc2_sqrt, ema_w,
    decay) of step t + 1; beta1, beta2, eps, grad_scale: the values the entry receives.  Returns one dict per step:
    p, m, v, ema (None without one) and the magnitudes the tolerances are stated in (Mm, Mv, Mp, Me: running
    maxima)."""
    ab, sqrt, where, maximum, _ = _xp(p)
    f64 = (lambda a: a.astype(np.float64)) if isinstance(p, np.ndarray) else (lambda a: a.double())
    n = p.shape[0]
    dec = element_mask(mask, n)
    p = f64(p)
    m = p * 0.0 if m is None else f64(m)
    v = p * 0.0 if v is None else f64(v)
    e = None if ema is None else f64(ema)
    b1, b2, eps, gs = float(beta1), float(beta2), float(eps), float(grad_scale)
    w = 1.0 - b1
    Mm, Mv, Mp = p * 0.0, p * 0.0, ab(p)
    Me = None if e is None else maximum(ab(e), Mp)
    out = []
    for g, s in zip(grads, scalars):
        gi = f64(g) * gs
        pd = where(dec, p - float(s["decay"]) * p, p)
        Mm = maximum(Mm, ab(m) + ab(gi))
        mn = m + w * (gi - m)
        vn = v * b2 + (1.0 - b2) * gi * gi
        denom = sqrt(vn) / float(s["bc2_sqrt"]) + eps
        pn = pd - float(s["step_size"]) * (mn / denom)
        Mv = maximum(Mv, vn)
        Mp = maximum(Mp, maximum(ab(p), ab(pn)) + float(s["step_size"]) * Mm / denom)
        if e is not None:
            e = e + float(s["ema_w"]) * (pn - e)
            Me = maximum(maximum(Me, Mp), ab(e))
        p, m, v = pn, mn, vn
        out.append(dict(p=p, m=m, v=v, ema=e, Mm=Mm, Mv=Mv, Mp=Mp, Me=Me))
    return out


MUTANTS = ("decay_after_update", "step_size_times_lambda", "coupled_l2", "decay_unmasked", "mask_plus_8",
           "mask_shift_2", "ema_towards_pd")


def adamw_emulate32(p, grads, mask, scalars, beta1, beta2, eps, grad_scale=1.0, ema=None, m=None, v=None,
                    mutant=None, lam=None):
    """The kernel's arithmetic in NumPy fp32, operation by operation in its order (no contraction except the one
    fma, which is taken in double -- the product of two floats is exact there -- and rounded to fp32; NumPy's fp32
    division and square root are correctly rounded, as the library's are).  Returns one dict(p, m, v, ema) per
    step.  mutant: one of MUTANTS, a wrong AdamW the tolerances have to reject (lam: lambda, for the two mutants
    that need it apart from decay)."""
    F = np.float32
    n = p.shape[0]
    groups = (n + 7) // 8
    mk = np.asarray(mask) != 0
    i = np.arange(n)
    if mutant == "mask_plus_8":
        dec = np.concatenate((mk, [False]))[(i + 8) >> 3]
    elif mutant == "mask_shift_2":
        dec = np.concatenate((mk, np.zeros(groups + 2, dtype=bool)))[i >> 2]
    elif mutant == "decay_unmasked":
        dec = np.ones(n, dtype=bool)
    else:
        dec = mk[i >> 3]
    p = p.astype(F)
    m = np.zeros(n, F) if m is None else m.astype(F)
    v = np.zeros(n, F) if v is None else v.astype(F)
    e = None if ema is None else ema.astype(F)
    b1, b2, eps, gs = F(beta1), F(beta2), F(eps), F(grad_scale)
    one, half = F(1.0), F(0.5)
    w = one - b1

    def fma_decay(c, x):
        return (x.astype(np.float64) * (-float(c)) + x.astype(np.float64)).astype(F)

    def lerp(a, b, t):
        return (a + t * (b - a)).astype(F) if t < half else (b - (b - a) * (one - t)).astype(F)

    out = []
    for t, (g, s) in enumerate(zip(grads, scalars), 1):
        step, bc2, ew, c = F(s["step_size"]), F(s["bc2_sqrt"]), F(s["ema_w"]), F(s["decay"])
        if mutant == "step_size_times_lambda":
            c = F(f32(float(step) * lam))
        gi = (g.astype(F) * gs).astype(F)
        if mutant == "coupled_l2":
            gi = (gi + F(lam) * p).astype(F)
            pd = p
        elif mutant == "decay_after_update":
            pd = p
        else:
            pd = np.where(dec, fma_decay(c, p), p)
        mn = lerp(m, gi, w)
        vn = (v * b2 + (one - b2) * gi * gi).astype(F)
        denom = (np.sqrt(vn) / bc2 + eps).astype(F)
        pn = (pd - step * (mn / denom)).astype(F)
        if mutant == "decay_after_update":
            pn = np.where(dec, fma_decay(c, pn), pn)
        if e is not None:
            e = lerp(e, pd if mutant == "ema_towards_pd" else pn, ew)
        p, m, v = pn, mn, vn
        out.append(dict(p=p, m=m, v=v, ema=e))
    return out


# ---- the kernels' own element function, compiled for the host ---------------------------------------------------
# csrc/adam_element.h chained over the steps for every element, the way the kernels of csrc/optim.hip call it:
# `clip` = 0 passes (g, scale) as adam_kernel and adam_groups_kernel<*, false> do, `clip` = 1 passes
# (fp32(g * pre), scale) as adam_groups_kernel<*, true> does, and a step marked skipped leaves the state alone, as
# that kernel's early return does.  Everything travels as the hex words of the fp32 values.  Input: n, steps, ema,
# clip, beta1, beta2, eps; p[n]; ema[n] (if ema); decayed[n]; per step: skipped, step_size, bc2_sqrt, ema_w, decay,
# pre, scale, g[n].  Output: per step five lines, p m v ema and the shadow pack_bf16x2 makes of p.
ELEMENT_PROGRAM = r'''
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "adam_element.h"

static uint32_t word() {
    unsigned w = 0;
    if (scanf("%x", &w) != 1) { fprintf(stderr, "short input\n"); exit(2); }
    return (uint32_t)w;
}
static float real() {
    const uint32_t w = word();
    float f;
    memcpy(&f, &w, 4);
    return f;
}
static void read_into(std::vector<float>& a) { for (float& x : a) x = real(); }
static void print(const std::vector<float>& a) {
    for (float x : a) {
        uint32_t w;
        memcpy(&w, &x, 4);
        printf("%08x ", (unsigned)w);
    }
    putchar('\n');
}

template <bool EMA>
static void run(size_t n, int steps, bool clip, float beta1, float beta2, float eps) {
    std::vector<float> p(n), e(n, 0.0f), m(n, 0.0f), v(n, 0.0f), g(n);
    std::vector<uint32_t> dec(n);
    read_into(p);
    if (EMA) read_into(e);
    for (uint32_t& d : dec) d = word();
    for (int t = 0; t < steps; ++t) {
        const bool skipped = word() != 0;
        const float step_size = real(), bc2_sqrt = real(), ema_w = real(), decay = real(), pre = real(),
                    scale = real();
        read_into(g);
        for (size_t i = 0; i < n && !skipped; ++i)
            p[i] = qarig::adam_element<EMA>(p[i], clip ? g[i] * pre : g[i], m[i], v[i], e[i], dec[i] != 0, beta1,
                                            beta2, eps, step_size, bc2_sqrt, ema_w, decay, scale);
        print(p);
        print(m);
        print(v);
        print(e);
        for (size_t i = 0; i < n; ++i) printf("%04x ", qarig::pack_bf16x2(p[i], 0.0f) & 0xffffu);
        putchar('\n');
    }
}

int main() {
    const size_t n = word();
    const int steps = (int)word();
    const bool ema = word() != 0, clip = word() != 0;
    const float beta1 = real(), beta2 = real(), eps = real();
    if (ema) run<true>(n, steps, clip, beta1, beta2, eps);
    else run<false>(n, steps, clip, beta1, beta2, eps);
    return 0;
}
'''


def build_element_program(workdir):
    """Compiles ELEMENT_PROGRAM against csrc/adam_element.h with the host compiler; returns the executable."""
    import os
    import subprocess
    cxx = "/opt/rocm/lib/llvm/bin/clang++"
    assert os.path.exists(cxx)
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                        "quantized-autoregression-image-generator_amd", "csrc")
    src = os.path.join(str(workdir), "adam_element_host.cpp")
    with open(src, "w") as f:
        f.write(ELEMENT_PROGRAM)
    exe = os.path.join(str(workdir), "adam_element_host")
    subprocess.run([cxx, "-O1", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-I", csrc, src, "-o", exe],
                   check=True, capture_output=True, text=True)
    return exe


def run_element_program(exe, p, ema, decayed, beta1, beta2, eps, steps, clip=False):
    """steps: one dict(g, step_size, bc2_sqrt, ema_w, decay, scale[, pre, skipped]) per step.  Returns one
    dict(p, m, v, ema, shadow) of uint32 arrays (the bits; shadow: the 16 of p's bf16) per step; ema is None
    without one."""
    import subprocess

    def words(a):
        return " ".join(f"{w:08x}" for w in np.ascontiguousarray(a, np.float32).view(np.uint32).tolist())

    n = p.shape[0]
    lines = [f"{n:x} {len(steps):x} {int(ema is not None):x} {int(clip):x} " + words([beta1, beta2, eps]), words(p)]
    if ema is not None:
        lines.append(words(ema))
    lines.append(" ".join("1" if d else "0" for d in decayed))
    for s in steps:
        lines.append(f"{int(bool(s.get('skipped', False))):x} " + words(
            [s["step_size"], s["bc2_sqrt"], s["ema_w"], s["decay"], s.get("pre", 1.0), s["scale"]]))
        lines.append(words(s["g"]))
    out = subprocess.run([exe], input="\n".join(lines) + "\n", check=True, capture_output=True,
                         text=True).stdout.splitlines()
    assert len(out) == 5 * len(steps)
    rows = [np.array([int(w, 16) for w in line.split()], dtype=np.uint32) for line in out]
    assert all(r.shape == (n,) for r in rows)
    return [dict(p=rows[5 * t], m=rows[5 * t + 1], v=rows[5 * t + 2], ema=rows[5 * t + 3] if ema is not None else None,
                 shadow=rows[5 * t + 4]) for t in range(len(steps))]


def worst_ratios(ref_steps, got_steps):
    """{output: worst over steps and elements of |got - ref| / (bound(T) u M)}: at most 1 inside the tolerance.
    got_steps[t]: dict(p, m, v, ema) of arrays of the reference's library, any float dtype.  The magnitudes also
    take in what the checked sequence holds."""
    ab, _, _, maximum, _ = _xp(ref_steps[0]["p"])
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


def cases():
    """The shared inputs: every (scale of p, lambda, betas), n = 4101 elements (512 full groups and a partial
    one), a random group mask, Gaussian gradients with exact zeros, an EMA that starts off the parameters, and
    grad_scale 0.5 on every other case."""
    k = 0
    for scale in SCALES:
        for lam in LAMBDAS:
            for betas in BETAS:
                yield dict(id=f"scale{scale:g}-lam{lam:g}-b{betas[0]:g}", scale=scale, lam=lam, betas=betas,
                           grad_scale=0.5 if k % 2 else 1.0, seed=k)
                k += 1


def make_inputs(case, n=4101, steps=STEPS):
    rng = np.random.default_rng(1000 + case["seed"])
    p = (rng.standard_normal(n) * case["scale"]).astype(np.float32)
    p[:4] = [0.0, -0.0, case["scale"], -case["scale"]][:min(4, n)]
    ema = (p + rng.standard_normal(n).astype(np.float32) * np.float32(1e-2 * case["scale"])).astype(np.float32)
    grads = []
    for _ in range(steps):
        g = rng.standard_normal(n).astype(np.float32)
        g[rng.random(n) < 0.1] = 0.0
        grads.append(g)
    mask = (rng.random((n + 7) // 8) < 0.5).astype(np.uint8)
    b1, b2 = f32(case["betas"][0]), f32(case["betas"][1])
    scalars = [step_scalars(t, LR, case["lam"], case["betas"], EMA_WS[(t - 1) % len(EMA_WS)])
               for t in range(1, steps + 1)]
    return dict(p=p, ema=ema, grads=grads, mask=mask, scalars=scalars, beta1=b1, beta2=b2, eps=f32(EPS),
                grad_scale=case["grad_scale"])


def masks(n, seed=0):
    """The GPU test's group masks for n elements, by name."""
    groups = (n + 7) // 8
    rng = np.random.default_rng(seed + n)
    first, last = np.zeros(groups, np.uint8), np.zeros(groups, np.uint8)
    first[0] = 1
    last[-1] = 1
    return {"zeros": np.zeros(groups, np.uint8), "ones": np.ones(groups, np.uint8),
            "alternating": (np.arange(groups) % 2).astype(np.uint8), "first": first, "last": last,
            "random": (rng.random(groups) < 0.5).astype(np.uint8) * np.uint8(255 if seed % 2 else 1)}
