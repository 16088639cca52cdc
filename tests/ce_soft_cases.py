"""Inputs, fp64 reference, measures, CPU emulation, tolerances and mutants shared by tests/test_gpu_ce_soft.py
(ce_reg_rows_kernel<., ., true> + mean2_kernel of csrc/loss.hip on an MI355X, through qarig_cross_entropy_soft_fwd) and
tests/test_ce_soft_host.py (the same pieces on the CPU).  The logits and helpers are row_kernel_cases' and
ce_reg_cases', by import.

WHAT IS UNDER TEST.  SOM-neighbour soft targets in the fused cross-entropy launch.  The leading K
classes are codes on the SOM axis, classes K .. C - 1 are special.  Per row with target t < K, w the fp32 table
w[d] = fp32(exp(-d^2 / 2 sigma^2)), d = 0 .. R, and mx, s, logs, lse, p, nll, u as in ce_reg_cases:
    lo = max(0, t - R)   hi = min(K - 1, t + R)   q[j] = w[|j - t|] / sum_{i = lo .. hi} w[|i - t|], lo <= j <= hi
    h = logs - sum_j q[j] (x[j] - mx)             obj = (1 - eps - nu) nll + eps u + nu h + zeta lse^2
    d obj / d x[c] = p (1 + 2 zeta lse) - (1 - eps - nu) [c == t] - eps / C - nu q[c]
    loss = {mean obj, mean nll}                   dlogits = (d obj / d x) / M
A row with t >= K takes nu = 0.  A term whose coefficient is 0 is not evaluated: a -inf logit outside the window
(or behind a table entry of exactly 0) never meets a 0 factor.  A -inf logit inside the window gives h = +inf.

CASES.  ce_case(37, C), C in SOFT_CLASSES, each with K = C - 1 and K = C and each R in SOFT_RANGES (sigma = R / 2, the
command line's default): 54 cases; and two of unit rows only, (255 | 257, 41) at K = 40, R = 2, whose mean objective is
finite (every (37, C) case holds a +inf row).  SoftCase forces, on rows that are neither peak_target nor masked (their
logits are built around their own targets), the targets 0, 1, R - 1, R, K - 1 - R, K - R, K - 1, K (special, where
K < C), 64 (window astride the lane wrap 63 | 64) and 256 (astride the end of the four-trip body), each clamped into
[0, C - 1]; R = 31 at C = 3 and C = 41 makes the window the whole axis.  Every case at every (eps, zeta, nu) of
SOFT_GRID; SOFT_BITS_POINT (nu = 0) is only for the bit comparison with qarig_cross_entropy_reg_fwd.

MEASURES: those of ce_reg_cases, with nu q[c] added to the element scale of dlogits (and (1 - eps - nu) on the target
term); the row gradient sum as there; the fp64 reference is taken on the fp32 logits and the fp32 table.

TOLERANCES.  SOFT_TOL_U[(output, family, grid index)] and SOFT_MEAN_TOL_U[(mean, grid index)] are ceil(2 x the worst
error of `soft_emulate`) over every case -- the kernel's fp32 arithmetic on the CPU in the kernel's summation orders
(reg_emulate's, plus: one table entry and one logit per lane, the normaliser by the 64-lane butterfly, q by one
correctly rounded division, the weighted shifted sum by a second butterfly, the objective by one more fmaf, nu q by one
product); the factor 2 is for the hardware exp / log (row_kernel_cases' rule).  The emulation's figure stands beside
each entry, tests/test_ce_soft_host.py recomputes the table; it is not taken from the kernel and is not to be widened.

+INF ROWS.  A masked row's objective is +inf at eps > 0 (u), and at eps = 0 where one of its -inf logits lies inside its
window (h).  SOFT_INF_ROWS_EPS and SOFT_INF_ROWS_NB are those counts over the 54 cases per grid point; no other entry
of any output is excused from an error figure.

MUTANTS (`SOFT_MUTANTS`; the host test proves each rejected on these inputs, and by which cells): the window not
clamped at K - 1 (mass on <end>), no renormalisation at the ends of the axis, a special target smoothed, nu missing
from the target coefficient, nu q missing from the gradient, the window t - R .. t + R - 1, the table indexed by
j - lo, and the nu term summed over every column (0 * -inf on a masked column outside the window)."""
import functools
import math

import torch

from ce_reg_cases import _mean_err, _row_err, f32
from row_kernel_cases import (CE_FAMILIES, CE_M, U, _chunks, butterfly, ce_case, exp32, fma32, log32,  # noqa: F401
                              mean_emulate, row_sum, within, worse, worst_or_exact)

SOFT_CLASSES = (3, 41, 64, 65, 200, 256, 257, 513, 8193)
SOFT_RANGES = (1, 2, 31)
SOFT_GRID = ((0.0, 0.0, 0.2), (0.1, 0.0, 0.2), (0.1, 1e-4, 0.3), (0.5, 1e-2, 0.4))
SOFT_BITS_POINT = (0.1, 1e-4, 0.0)
SOFT_ROW_OUTPUTS = ("obj", "nll", "dlogits")
SOFT_MEAN_M, SOFT_MEAN_CKR = (255, 257), (41, 40, 2)    # no masked rows: the only cases whose mean objective is finite
SOFT_FORCED_ROWS = ("unit", "offset", "peak_other", "ties")
SOFT_INF_ROWS_EPS = 5 * 2 * len(SOFT_RANGES) * len(SOFT_CLASSES)     # every masked row of every case, eps > 0
SOFT_INF_ROWS_NB = 146           # masked rows with a -inf logit inside their window (window_inf_rows), all cases

# ---- tolerances: ceil(2 x emulation worst), see the module docstring; (output, family, index into SOFT_GRID) ----
SOFT_TOL_U = {
    ('obj', 'masked', 0): 4,                # 2 x 1.713 u
    ('obj', 'offset', 0): 6,                # 2 x 2.749 u
    ('obj', 'peak_other', 0): 12,           # 2 x 5.762 u
    ('obj', 'peak_target', 0): 21,          # 2 x 10.154 u
    ('obj', 'ties', 0): 2,                  # 2 x 0.828 u
    ('obj', 'unit', 0): 6,                  # 2 x 2.736 u
    ('nll', 'masked', 0): 3,                # 2 x 1.388 u
    ('nll', 'offset', 0): 3,                # 2 x 1.213 u
    ('nll', 'peak_other', 0): 13,           # 2 x 6.147 u
    ('nll', 'peak_target', 0): 21,          # 2 x 10.352 u
    ('nll', 'ties', 0): 2,                  # 2 x 0.828 u
    ('nll', 'unit', 0): 4,                  # 2 x 1.921 u
    ('dlogits', 'masked', 0): 64,           # 2 x 31.750 u
    ('dlogits', 'offset', 0): 36,           # 2 x 17.837 u
    ('dlogits', 'peak_other', 0): 78,       # 2 x 38.853 u
    ('dlogits', 'peak_target', 0): 76,      # 2 x 37.780 u
    ('dlogits', 'ties', 0): 18,             # 2 x 8.532 u
    ('dlogits', 'unit', 0): 70,             # 2 x 34.678 u
    ('obj', 'masked', 1): 0,                # 2 x 0.000 u
    ('obj', 'offset', 1): 5,                # 2 x 2.434 u
    ('obj', 'peak_other', 1): 7,            # 2 x 3.408 u
    ('obj', 'peak_target', 1): 10,          # 2 x 4.714 u
    ('obj', 'ties', 1): 2,                  # 2 x 0.828 u
    ('obj', 'unit', 1): 6,                  # 2 x 2.654 u
    ('nll', 'masked', 1): 3,                # 2 x 1.388 u
    ('nll', 'offset', 1): 3,                # 2 x 1.213 u
    ('nll', 'peak_other', 1): 13,           # 2 x 6.147 u
    ('nll', 'peak_target', 1): 21,          # 2 x 10.352 u
    ('nll', 'ties', 1): 2,                  # 2 x 0.828 u
    ('nll', 'unit', 1): 4,                  # 2 x 1.921 u
    ('dlogits', 'masked', 1): 32,           # 2 x 15.780 u
    ('dlogits', 'offset', 1): 25,           # 2 x 12.067 u
    ('dlogits', 'peak_other', 1): 18,       # 2 x 8.569 u
    ('dlogits', 'peak_target', 1): 35,      # 2 x 17.320 u
    ('dlogits', 'ties', 1): 15,             # 2 x 7.109 u
    ('dlogits', 'unit', 1): 33,             # 2 x 16.448 u
    ('obj', 'masked', 2): 0,                # 2 x 0.000 u
    ('obj', 'offset', 2): 5,                # 2 x 2.495 u
    ('obj', 'peak_other', 2): 7,            # 2 x 3.040 u
    ('obj', 'peak_target', 2): 8,           # 2 x 3.776 u
    ('obj', 'ties', 2): 3,                  # 2 x 1.483 u
    ('obj', 'unit', 2): 7,                  # 2 x 3.117 u
    ('nll', 'masked', 2): 3,                # 2 x 1.388 u
    ('nll', 'offset', 2): 3,                # 2 x 1.213 u
    ('nll', 'peak_other', 2): 13,           # 2 x 6.147 u
    ('nll', 'peak_target', 2): 21,          # 2 x 10.352 u
    ('nll', 'ties', 2): 2,                  # 2 x 0.828 u
    ('nll', 'unit', 2): 4,                  # 2 x 1.921 u
    ('dlogits', 'masked', 2): 31,           # 2 x 15.058 u
    ('dlogits', 'offset', 2): 25,           # 2 x 12.204 u
    ('dlogits', 'peak_other', 2): 18,       # 2 x 8.927 u
    ('dlogits', 'peak_target', 2): 36,      # 2 x 17.857 u
    ('dlogits', 'ties', 2): 17,             # 2 x 8.203 u
    ('dlogits', 'unit', 2): 34,             # 2 x 16.683 u
    ('obj', 'masked', 3): 0,                # 2 x 0.000 u
    ('obj', 'offset', 3): 5,                # 2 x 2.162 u
    ('obj', 'peak_other', 3): 6,            # 2 x 2.802 u
    ('obj', 'peak_target', 3): 5,           # 2 x 2.499 u
    ('obj', 'ties', 3): 3,                  # 2 x 1.408 u
    ('obj', 'unit', 3): 7,                  # 2 x 3.165 u
    ('nll', 'masked', 3): 3,                # 2 x 1.388 u
    ('nll', 'offset', 3): 3,                # 2 x 1.213 u
    ('nll', 'peak_other', 3): 13,           # 2 x 6.147 u
    ('nll', 'peak_target', 3): 21,          # 2 x 10.352 u
    ('nll', 'ties', 3): 2,                  # 2 x 0.828 u
    ('nll', 'unit', 3): 4,                  # 2 x 1.921 u
    ('dlogits', 'masked', 3): 28,           # 2 x 13.713 u
    ('dlogits', 'offset', 3): 18,           # 2 x 8.604 u
    ('dlogits', 'peak_other', 3): 13,       # 2 x 6.301 u
    ('dlogits', 'peak_target', 3): 27,      # 2 x 13.065 u
    ('dlogits', 'ties', 3): 15,             # 2 x 7.231 u
    ('dlogits', 'unit', 3): 22,             # 2 x 10.770 u
}
SOFT_MEAN_TOL_U = {
    ('mean_nll', 0): 5,                     # 2 x 2.004 u
    ('mean_obj', 0): 4,                     # 2 x 1.605 u
    ('mean_nll', 1): 5,                     # 2 x 2.004 u
    ('mean_obj', 1): 1,                     # 2 x 0.499 u
    ('mean_nll', 2): 5,                     # 2 x 2.004 u
    ('mean_obj', 2): 4,                     # 2 x 1.792 u
    ('mean_nll', 3): 5,                     # 2 x 2.004 u
    ('mean_obj', 3): 4,                     # 2 x 1.801 u
}


class SoftCase:
    """One (C, K, R): the logits of ce_case(37, C), the forced targets, the fp32 table."""

    def __init__(self, C, K, R, M=CE_M):
        c = ce_case(M, C, M == CE_M)
        self.M, self.C, self.K, self.R = c.M, C, K, R
        self.x, self.family, self.rows = c.x, c.family, c.rows
        self.w = soft_table(R, R / 2.0)
        self.forced = forced_targets(C, K, R)
        free = [r for r, f in enumerate(c.family) if f in SOFT_FORCED_ROWS]
        t = c.t.clone()
        self.forced_rows = []
        for i, v in enumerate(self.forced):
            r = free[(5 * i) % len(free)]          # 5 is coprime to 28, 255 and 257: distinct rows, spread over the families
            assert r not in self.forced_rows and math.isfinite(float(c.x[r, v]))
            t[r] = v
            self.forced_rows.append(r)
        self.t = t

    def bad_targets(self):
        t = self.t.clone()
        t[3], t[30] = self.C, -1
        return t


def soft_table(R, sigma):
    """w[d] = exp(-d^2 / (2 sigma^2)), d = 0 .. R: fp64, rounded once to fp32."""
    d = torch.arange(R + 1, dtype=torch.float64)
    return torch.exp(-(d * d) / (2.0 * sigma * sigma)).float()


def forced_targets(C, K, R):
    raw = [0, 1, R - 1, R, K - 1 - R, K - R, K - 1] + ([K] if K < C else []) + [64, 256]
    return [min(max(v, 0), C - 1) for v in raw]


@functools.lru_cache(maxsize=None)
def soft_case(C, K, R, M=CE_M):
    return SoftCase(C, K, R, M)


def soft_cases(classes=SOFT_CLASSES):
    """The (37, C) cases, then the two unit-only cases either side of mean2_kernel's 256-row trip."""
    return [soft_case(C, K, R) for C in classes for K in (C - 1, C) for R in SOFT_RANGES] + \
        [soft_case(*SOFT_MEAN_CKR, M) for M in SOFT_MEAN_M]


def window(t, C, K, R, w, mutant=None):
    """(inside (M, C) bool, table value per column (M, C), in w's dtype, 0 outside): the window of every row, with
    the rule 'a table entry of exactly 0 is no window column' applied."""
    cols = torch.arange(C)[None, :]
    tt = t[:, None]
    dist = (cols - tt).abs()
    top = C if mutant == "no_clamp_end" else K
    soft_row = torch.ones_like(tt, dtype=torch.bool) if mutant == "special_smoothed" else tt < K
    inside = (dist <= R) & (cols < top) & soft_row
    if mutant == "short_window":
        inside &= cols - tt <= R - 1
    idx = dist
    if mutant == "table_by_lo":
        idx = cols - (tt - R).clamp_min(0)
    wv = torch.where(inside, w[idx.clamp(0, R)], torch.zeros((), dtype=w.dtype))
    return wv > 0, wv


def soft_ref_uncached(x, t, K, R, w, eps, zeta, nu):
    """fp64 on the fp32 logits and the fp32 table: {obj, nll, lse, nur (M,), p, hot, q, dlogits (M, C), mean_obj,
    mean_nll}.  Zero coefficients skipped, per row."""
    eps, zeta, nu = f32(eps), f32(zeta), f32(nu)
    M, C = x.shape
    ar = torch.arange(M)
    xd = x.double()
    mx = xd.max(1).values
    d = xd - mx[:, None]
    logs = torch.log(torch.exp(d).sum(1))
    lse = mx + logs
    p = torch.exp(d - logs[:, None])
    nll = logs - d[ar, t]
    inside, wv = window(t, C, K, R, w.double())
    z = wv.sum(1)
    q = torch.where(inside, wv / z.clamp_min(1e-300)[:, None], torch.zeros_like(wv))
    nur = nu * (t < K).double()
    h = logs - torch.where(inside, q * d, torch.zeros_like(d)).sum(1)
    obj = (1.0 - eps - nur) * nll
    if eps > 0:
        obj = obj + eps * (logs - d.sum(1) / C)
    obj = torch.where(nur > 0, obj + nur * h, obj)
    if zeta > 0:
        obj = obj + zeta * lse * lse
    hot = torch.zeros_like(p)
    hot[ar, t] = 1.0
    g = p * (1.0 + 2.0 * zeta * lse)[:, None] - (1.0 - eps - nur)[:, None] * hot - eps / C - nur[:, None] * q
    return {"obj": obj, "nll": nll, "lse": lse, "nur": nur, "p": p, "hot": hot, "q": q, "dlogits": g / M,
            "mean_obj": obj.mean(), "mean_nll": nll.mean()}


@functools.lru_cache(maxsize=None)
def _ref_of_case(C, K, R, M, gi):
    c = soft_case(C, K, R, M)
    return soft_ref_uncached(c.x, c.t, K, R, c.w, *SOFT_GRID[gi])


def soft_ref(c, gi):
    """The reference of case c at SOFT_GRID[gi]: computed once, shared, never modified."""
    return _ref_of_case(c.C, c.K, c.R, c.M, gi)


def window_inf_rows(c):
    """The rows of c whose window holds a -inf logit: by the definition alone (no arithmetic)."""
    inside, _ = window(c.t, c.C, c.K, c.R, c.w)
    return torch.nonzero((inside & torch.isinf(c.x)).any(1)).flatten().tolist()


SOFT_MUTANTS = ("no_clamp_end", "no_renorm", "special_smoothed", "no_nu_hot", "no_nuq_grad", "short_window",
                "table_by_lo", "nu_multiplied")


def _lanes(v):
    """(M, C) with at most one non-zero per lane residue -> (M, 64): what each lane holds (the sum adds zeros)."""
    return _chunks(v).sum(1)


def soft_emulate(x, t, K, R, w, eps, zeta, nu, mutant=None):
    """ce_reg_rows_kernel<., ., true> + mean2_kernel in fp32 on the CPU.  Returns (row obj, row nll, dlogits, mean obj,
    mean nll).  On a row with t >= K, and at every row where K = 0 would hold, operation for operation reg_emulate."""
    M, C = x.shape
    ar = torch.arange(M)
    e32, z32, n32 = (torch.tensor(v, dtype=torch.float32) for v in (eps, zeta, nu))
    Cf = torch.tensor(float(C))
    mx = x.max(1).values
    d = x - mx[:, None]
    s = row_sum(exp32(d))
    logs = log32(s)
    nll = logs - (x[ar, t] - mx)
    inside, wv = window(t, C, K, R, w, mutant)
    soft = (t < K) if mutant != "special_smoothed" else torch.ones(M, dtype=torch.bool)
    if mutant == "no_renorm":
        zsum = (w.sum() + w[1:].sum()).expand(M)          # the whole window's mass, whatever was clamped away
    else:
        zsum = butterfly(_lanes(wv))
    zero = torch.zeros(())
    q = torch.where(inside, wv / zsum[:, None], zero)
    nur = torch.where(soft, n32, zero)
    hot = (1.0 - e32 if eps > 0 else torch.tensor(1.0)) - (torch.zeros(M) if mutant == "no_nu_hot" else nur)
    obj = hot * nll
    if eps > 0:
        u = logs - row_sum(d) / Cf
        obj = fma32(e32, u, obj)
    if mutant == "nu_multiplied":
        hs = row_sum(q * d)
    else:
        hs = butterfly(_lanes(torch.where(inside, q * d, zero)))
    obj = torch.where(soft, fma32(n32, logs - hs, obj), obj)
    f = torch.ones(M)
    if zeta > 0:
        lse = mx + logs
        zl = z32 * lse
        obj = fma32(zl, lse, obj)
        f = fma32(torch.tensor(2.0), zl, torch.tensor(1.0))
    p = exp32(d - logs[:, None])
    oh = torch.zeros_like(p)
    oh[ar, t] = 1.0
    hh = oh * hot[:, None]
    g = fma32(p, f[:, None], -hh) if zeta > 0 else p - hh
    if eps > 0:
        g = g - e32 / Cf
    if mutant != "no_nuq_grad":
        g = g - torch.where(inside, n32 * q, zero)
    inv_m = torch.tensor(1.0) / torch.tensor(float(M))
    return obj, nll, g * inv_m, mean_emulate(obj, inv_m), mean_emulate(nll, inv_m)


def soft_measures(c, gi, obj, nll, dlogits, mean_obj, mean_nll, ref=None):
    """{"obj", "nll", "dlogits", "dsum": (M,) errors in u (dlogits: the worst element of the row; both None without
    dlogits), "mean_obj", "mean_nll": floats, "inf_rows": the rows whose reference objective is +inf}."""
    eps, zeta, _ = (f32(v) for v in SOFT_GRID[gi])
    ref = soft_ref(c, gi) if ref is None else ref
    out = {"obj": _row_err(obj, ref["obj"]), "nll": _row_err(nll, ref["nll"]), "dlogits": None, "dsum": None,
           "mean_obj": _mean_err(mean_obj, ref["mean_obj"], ref["obj"]),
           "mean_nll": _mean_err(mean_nll, ref["mean_nll"], ref["nll"]),
           "inf_rows": torch.nonzero(torch.isinf(ref["obj"])).flatten().tolist()}
    if dlogits is not None:
        nur = ref["nur"][:, None]
        scale = (ref["p"] * (1.0 + 2.0 * zeta * ref["lse"].abs())[:, None] + (1.0 - eps - nur) * ref["hot"] + eps / c.C +
                 nur * ref["q"]) / c.M
        out["dlogits"] = worst_or_exact((dlogits.double() - ref["dlogits"]).abs(), scale).max(1).values
        out["dsum"] = worst_or_exact((dlogits.double().sum(1) - ref["dlogits"].sum(1)).abs(), scale.sum(1))
    return out


def soft_verdicts(impl, cases=None, grid=None):
    """({(output, family, gi): worst u, ("mean_obj" | "mean_nll", gi): worst u}, judged, excused) of an
    implementation with soft_emulate's signature over every case and grid point of the GPU test.  judged counts the
    (case, grid point, row, output) entries that entered a cell, excused those among them whose reference is +inf
    (they must be +inf, and count as 0 or inf)."""
    worst, judged, excused = {}, 0, 0
    for gi in (range(len(SOFT_GRID)) if grid is None else grid):
        for c in (soft_cases() if cases is None else cases):
            m = soft_measures(c, gi, *impl(c.x, c.t, c.K, c.R, c.w, *SOFT_GRID[gi]))
            for fam in set(c.family):
                r = c.rows(fam)
                for k in ("obj", "nll", "dlogits", "dsum"):
                    key = (k, fam, gi)
                    worst[key] = worse(worst.get(key, 0.0), float(m[k][r].max()))
                    judged += len(r)
            excused += len(m["inf_rows"])
            for k in ("mean_obj", "mean_nll"):
                worst[(k, gi)] = worse(worst.get((k, gi), 0.0), m[k])
    return worst, judged, excused


def tolerance_of(w):
    return math.ceil(2 * w)


def soft_tol(key):
    if len(key) == 2:
        return SOFT_MEAN_TOL_U[key]
    return SOFT_TOL_U[("dlogits",) + key[1:] if key[0] == "dsum" else key]


def soft_failures(worst):
    return sorted((k for k, w in worst.items() if not within(w, soft_tol(k))), key=str)


MUTANT_CLASSES = (3, 41, 65, 257)        # a subset of the GPU test's cases that already rejects every mutant


def mutant_failures(mutant):
    """Cells of the GPU test that reject a mutant (on the cases of MUTANT_CLASSES: a cell that fails on some of the
    cases fails on all of them, its figure is a maximum)."""
    return soft_failures(soft_verdicts(lambda *a: soft_emulate(*a, mutant=mutant), cases=soft_cases(MUTANT_CLASSES))[0])


if __name__ == "__main__":
    table = soft_verdicts(soft_emulate)[0]
    print("SOFT_TOL_U = {")
    for k in sorted((k for k in table if len(k) == 3 and k[0] != "dsum"),
                    key=lambda k: (k[2], SOFT_ROW_OUTPUTS.index(k[0]), k[1])):
        print(f"    {k!r}: {tolerance_of(table[k])},".ljust(44) + f"# 2 x {table[k]:.3f} u")
    print("}\nSOFT_MEAN_TOL_U = {")
    for k in sorted((k for k in table if len(k) == 2), key=lambda k: (k[1], k[0])):
        print(f"    {k!r}: {tolerance_of(table[k])},".ljust(44) + f"# 2 x {table[k]:.3f} u")
    print("}")
    print("SOFT_INF_ROWS_NB =", sum(len(window_inf_rows(c)) for c in soft_cases()))
    for k in sorted((k for k in table if k[0] == "dsum"), key=str):
        print("dsum", k, f"{table[k]:.3f}", "of", soft_tol(k) if SOFT_TOL_U else "-")
    if SOFT_TOL_U:
        for m in SOFT_MUTANTS:
            print(m, mutant_failures(m))
