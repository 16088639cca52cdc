"""Inputs, fp64 reference, measures, CPU emulation, tolerances and mutants shared by tests/test_gpu_ce_reg.py
(ce_reg_rows_kernel + mean2_kernel of csrc/loss.hip on an MI355X, through qarig_cross_entropy_reg_fwd) and
tests/test_ce_reg_host.py (the same pieces on the CPU).  The inputs and helpers are row_kernel_cases', by import.

WHAT IS UNDER TEST.  Cross-entropy with label smoothing eps and z-loss zeta in the fused launch.  Per row, with
mx = max x, s = sum exp(x - mx), logs = log s, lse = mx + logs, p = exp((x - mx) - logs):
    nll = logs - (x[t] - mx)        u = logs - (1 / C) sum (x - mx)        obj = (1 - eps) nll + eps u + zeta lse^2
    d obj / d x[c] = p (1 + 2 zeta lse) - (1 - eps) [c == t] - eps / C
    loss = {mean obj, mean nll}     dlogits = (d obj / d x) / M
which is F.cross_entropy(x, t, label_smoothing=eps) + zeta mean(logsumexp(x)^2).  A term whose coefficient is 0 is
not evaluated: eps = 0 on a row with -inf entries gives the plain, finite loss, not 0 * inf.

CASES.  ce_case(37, C), C in REG_CLASSES: the unit / offset (+-100, 1000) / peak / ties / masked rows of
row_kernel_cases with targets at column 0, at C - 1 and inside the last 64-chunk; 200 / 256 / 257 straddle the point
where only some lanes take the kernel's four-trip body.  The mean shapes (1 | 255 | 256 | 257 | 16385) x 41.  Every
case at every (eps, zeta) of REG_GRID.

MEASURES, u = 2^-24, against fp64 on the same fp32 inputs (eps and zeta as the fp32 values the entry receives):
  row objective, row nll   |err| / (u max(1, |ref|)); where the reference is +inf the result must be +inf
  dlogits, per element     |err| / (u (p (1 + 2 zeta |lse|) + (1 - eps) [c == t] + eps / C) / M); a scale of exactly 0
                           (masked columns at eps = 0) demands the reference itself
  row gradient sum         |sum got - sum ref| / (u sum of the element scales)
  the two means            |err| / (u mean |ref rows|); +inf where the reference is

TOLERANCES.  REG_TOL_U[(output, family, grid index)] and REG_MEAN_TOL_U[(mean, grid index)] are ceil(2 x the worst
error of `reg_emulate`) -- the intended fp32 arithmetic on the CPU: the kernel's lane partial sums in ascending trips,
the 64-lane butterfly, fmaf where the kernel has one, correctly rounded exp / log / division -- over every case; the
factor 2 is for the hardware exp / log (row_kernel_cases' rule).  The emulation's figure stands beside each entry,
tests/test_ce_reg_host.py recomputes the table; it is not taken from the kernel and is not to be widened.  The row
gradient sum takes dlogits' tolerance: a sum of elements each within tol x its scale is within tol x the summed scale.

MUTANTS (`REG_MUTANTS`; the host test proves each rejected on these inputs, and by which cells): the unshifted
sum x - C mx, eps / C missing from the gradient, (1 - eps) missing on the gradient's target term, zeta lse for
2 zeta lse in the gradient factor, the eps term multiplied rather than skipped at eps = 0, a dropped last partial
64-chunk, a mean that stops at 256 rows."""
import functools
import math

import torch

from row_kernel_cases import (CE_FAMILIES, CE_M, CE_MEAN_SHAPES, U, butterfly, ce_case, exp32, fma32, log32,  # noqa: F401
                              mean_emulate, row_sum, within, worse, worst_or_exact)

REG_CLASSES = (3, 41, 64, 65, 200, 256, 257, 513, 8193)
REG_GRID = ((0.0, 0.0), (0.1, 0.0), (0.0, 1e-4), (0.1, 1e-4), (0.5, 1e-2))
REG_ROW_OUTPUTS = ("obj", "nll", "dlogits")
REG_INF_ROWS = 5 * len(REG_CLASSES)          # masked rows: a +inf row objective at every grid point with eps > 0

# ---- tolerances: ceil(2 x emulation worst), see the module docstring; (output, family, index into REG_GRID) ----
REG_TOL_U = {
    ('obj', 'masked', 0): 3,                # 2 x 1.388 u
    ('obj', 'offset', 0): 3,                # 2 x 1.213 u
    ('obj', 'peak_other', 0): 4,            # 2 x 1.551 u
    ('obj', 'peak_target', 0): 21,          # 2 x 10.352 u
    ('obj', 'ties', 0): 2,                  # 2 x 0.828 u
    ('obj', 'unit', 0): 8,                  # 2 x 3.912 u
    ('nll', 'masked', 0): 3,                # 2 x 1.388 u
    ('nll', 'offset', 0): 3,                # 2 x 1.213 u
    ('nll', 'peak_other', 0): 4,            # 2 x 1.551 u
    ('nll', 'peak_target', 0): 21,          # 2 x 10.352 u
    ('nll', 'ties', 0): 2,                  # 2 x 0.828 u
    ('nll', 'unit', 0): 8,                  # 2 x 3.912 u
    ('dlogits', 'masked', 0): 64,           # 2 x 31.750 u
    ('dlogits', 'offset', 0): 36,           # 2 x 17.837 u
    ('dlogits', 'peak_other', 0): 78,       # 2 x 38.853 u
    ('dlogits', 'peak_target', 0): 76,      # 2 x 37.780 u
    ('dlogits', 'ties', 0): 18,             # 2 x 8.532 u
    ('dlogits', 'unit', 0): 70,             # 2 x 34.678 u
    ('obj', 'masked', 1): 0,                # 2 x 0.000 u
    ('obj', 'offset', 1): 4,                # 2 x 1.818 u
    ('obj', 'peak_other', 1): 5,            # 2 x 2.474 u
    ('obj', 'peak_target', 1): 10,          # 2 x 4.645 u
    ('obj', 'ties', 1): 2,                  # 2 x 0.828 u
    ('obj', 'unit', 1): 8,                  # 2 x 3.777 u
    ('nll', 'masked', 1): 3,                # 2 x 1.388 u
    ('nll', 'offset', 1): 3,                # 2 x 1.213 u
    ('nll', 'peak_other', 1): 4,            # 2 x 1.551 u
    ('nll', 'peak_target', 1): 21,          # 2 x 10.352 u
    ('nll', 'ties', 1): 2,                  # 2 x 0.828 u
    ('nll', 'unit', 1): 8,                  # 2 x 3.912 u
    ('dlogits', 'masked', 1): 32,           # 2 x 15.780 u
    ('dlogits', 'offset', 1): 25,           # 2 x 12.067 u
    ('dlogits', 'peak_other', 1): 18,       # 2 x 8.569 u
    ('dlogits', 'peak_target', 1): 35,      # 2 x 17.320 u
    ('dlogits', 'ties', 1): 15,             # 2 x 7.109 u
    ('dlogits', 'unit', 1): 33,             # 2 x 16.448 u
    ('obj', 'masked', 2): 4,                # 2 x 1.597 u
    ('obj', 'offset', 2): 3,                # 2 x 1.487 u
    ('obj', 'peak_other', 2): 4,            # 2 x 1.961 u
    ('obj', 'peak_target', 2): 21,          # 2 x 10.350 u
    ('obj', 'ties', 2): 3,                  # 2 x 1.371 u
    ('obj', 'unit', 2): 8,                  # 2 x 3.899 u
    ('nll', 'masked', 2): 3,                # 2 x 1.388 u
    ('nll', 'offset', 2): 3,                # 2 x 1.213 u
    ('nll', 'peak_other', 2): 4,            # 2 x 1.551 u
    ('nll', 'peak_target', 2): 21,          # 2 x 10.352 u
    ('nll', 'ties', 2): 2,                  # 2 x 0.828 u
    ('nll', 'unit', 2): 8,                  # 2 x 3.912 u
    ('dlogits', 'masked', 2): 64,           # 2 x 31.722 u
    ('dlogits', 'offset', 2): 37,           # 2 x 18.093 u
    ('dlogits', 'peak_other', 2): 78,       # 2 x 38.686 u
    ('dlogits', 'peak_target', 2): 77,      # 2 x 38.041 u
    ('dlogits', 'ties', 2): 18,             # 2 x 8.594 u
    ('dlogits', 'unit', 2): 73,             # 2 x 36.037 u
    ('obj', 'masked', 3): 0,                # 2 x 0.000 u
    ('obj', 'offset', 3): 4,                # 2 x 1.841 u
    ('obj', 'peak_other', 3): 7,            # 2 x 3.040 u
    ('obj', 'peak_target', 3): 11,          # 2 x 5.054 u
    ('obj', 'ties', 3): 3,                  # 2 x 1.371 u
    ('obj', 'unit', 3): 9,                  # 2 x 4.304 u
    ('nll', 'masked', 3): 3,                # 2 x 1.388 u
    ('nll', 'offset', 3): 3,                # 2 x 1.213 u
    ('nll', 'peak_other', 3): 4,            # 2 x 1.551 u
    ('nll', 'peak_target', 3): 21,          # 2 x 10.352 u
    ('nll', 'ties', 3): 2,                  # 2 x 0.828 u
    ('nll', 'unit', 3): 8,                  # 2 x 3.912 u
    ('dlogits', 'masked', 3): 31,           # 2 x 15.058 u
    ('dlogits', 'offset', 3): 25,           # 2 x 12.204 u
    ('dlogits', 'peak_other', 3): 18,       # 2 x 8.927 u
    ('dlogits', 'peak_target', 3): 36,      # 2 x 17.857 u
    ('dlogits', 'ties', 3): 17,             # 2 x 8.203 u
    ('dlogits', 'unit', 3): 34,             # 2 x 16.683 u
    ('obj', 'masked', 4): 0,                # 2 x 0.000 u
    ('obj', 'offset', 4): 5,                # 2 x 2.185 u
    ('obj', 'peak_other', 4): 5,            # 2 x 2.131 u
    ('obj', 'peak_target', 4): 5,           # 2 x 2.499 u
    ('obj', 'ties', 4): 3,                  # 2 x 1.408 u
    ('obj', 'unit', 4): 8,                  # 2 x 3.698 u
    ('nll', 'masked', 4): 3,                # 2 x 1.388 u
    ('nll', 'offset', 4): 3,                # 2 x 1.213 u
    ('nll', 'peak_other', 4): 4,            # 2 x 1.551 u
    ('nll', 'peak_target', 4): 21,          # 2 x 10.352 u
    ('nll', 'ties', 4): 2,                  # 2 x 0.828 u
    ('nll', 'unit', 4): 8,                  # 2 x 3.912 u
    ('dlogits', 'masked', 4): 28,           # 2 x 13.713 u
    ('dlogits', 'offset', 4): 18,           # 2 x 8.604 u
    ('dlogits', 'peak_other', 4): 13,       # 2 x 6.301 u
    ('dlogits', 'peak_target', 4): 27,      # 2 x 13.065 u
    ('dlogits', 'ties', 4): 15,             # 2 x 7.231 u
    ('dlogits', 'unit', 4): 22,             # 2 x 10.770 u
}
REG_MEAN_TOL_U = {
    ('mean_nll', 0): 4,                     # 2 x 1.784 u
    ('mean_obj', 0): 4,                     # 2 x 1.784 u
    ('mean_nll', 1): 4,                     # 2 x 1.784 u
    ('mean_obj', 1): 2,                     # 2 x 0.918 u
    ('mean_nll', 2): 4,                     # 2 x 1.784 u
    ('mean_obj', 2): 4,                     # 2 x 1.535 u
    ('mean_nll', 3): 4,                     # 2 x 1.784 u
    ('mean_obj', 3): 3,                     # 2 x 1.093 u
    ('mean_nll', 4): 4,                     # 2 x 1.784 u
    ('mean_obj', 4): 2,                     # 2 x 0.825 u
}


def f32(v):
    """The fp32 value a float argument of the C entry arrives as."""
    return float(torch.tensor(v, dtype=torch.float32))


def reg_cases():
    return [ce_case(CE_M, C) for C in REG_CLASSES] + [ce_case(M, C, False) for M, C in CE_MEAN_SHAPES]


def reg_ref_uncached(x, t, eps, zeta):
    """fp64 on fp32 inputs: {obj, nll, lse (M,), p, dlogits (M, C), mean_obj, mean_nll}.  Zero coefficients skipped."""
    eps, zeta = f32(eps), f32(zeta)
    M, C = x.shape
    ar = torch.arange(M)
    xd = x.double()
    mx = xd.max(1).values
    d = xd - mx[:, None]
    logs = torch.log(torch.exp(d).sum(1))
    lse = mx + logs
    p = torch.exp(d - logs[:, None])
    nll = logs - d[ar, t]
    obj = nll.clone()
    if eps > 0:
        obj = (1.0 - eps) * nll + eps * (logs - d.sum(1) / C)
    if zeta > 0:
        obj = obj + zeta * lse * lse
    hot = torch.zeros_like(p)
    hot[ar, t] = 1.0
    g = p * (1.0 + 2.0 * zeta * lse)[:, None] - (1.0 - eps) * hot - eps / C
    return {"obj": obj, "nll": nll, "lse": lse, "p": p, "hot": hot, "dlogits": g / M, "mean_obj": obj.mean(),
            "mean_nll": nll.mean()}


@functools.lru_cache(maxsize=None)
def _ref_of_case(M, C, mixed, gi):
    c = ce_case(M, C, mixed)
    return reg_ref_uncached(c.x, c.t, *REG_GRID[gi])


def reg_ref(c, gi):
    """The reference of case c at REG_GRID[gi]: computed once, shared, never modified."""
    return _ref_of_case(c.M, c.C, len(set(c.family)) > 1, gi)


def _drop_tail(v, fill):
    C = v.shape[1]
    if C % 64 == 0 or C < 64:
        return v
    v = v.clone()
    v[:, (C // 64) * 64:] = fill
    return v


REG_MUTANTS = ("unshifted", "no_eps_grad", "no_one_minus_eps", "single_zeta", "eps_multiplied", "drop_tail", "mean_256")


def reg_emulate(x, t, eps, zeta, mutant=None):
    """ce_reg_rows_kernel + mean2_kernel in fp32 on the CPU.  Returns (row obj, row nll, dlogits, mean obj, mean nll).
    At eps = zeta = 0 operation for operation row_kernel_cases.ce_emulate."""
    M, C = x.shape
    ar = torch.arange(M)
    e32, z32 = torch.tensor(eps, dtype=torch.float32), torch.tensor(zeta, dtype=torch.float32)
    Cf = torch.tensor(float(C))
    drop = mutant == "drop_tail"
    xm = _drop_tail(x, -math.inf) if drop else x
    mx = xm.max(1).values
    d = xm - mx[:, None]
    s = row_sum(exp32(d))
    logs = log32(s)
    nll = logs - (x[ar, t] - mx)
    obj = nll
    f = torch.ones(M)
    has_eps = eps > 0 or mutant == "eps_multiplied"
    if has_eps:
        if mutant == "unshifted":
            sh = row_sum(x) - Cf * mx
        else:
            sh = row_sum(_drop_tail(x - mx[:, None], 0.0) if drop else d)
        u = logs - sh / Cf
        obj = fma32(e32, u, (1.0 - e32) * nll)
    if zeta > 0:
        lse = mx + logs
        zl = z32 * lse
        obj = fma32(zl, lse, obj)
        f = zl + 1.0 if mutant == "single_zeta" else fma32(torch.tensor(2.0), zl, torch.tensor(1.0))
    p = exp32((x - mx[:, None]) - logs[:, None])
    hot = torch.zeros_like(p)
    hot[ar, t] = 1.0
    h = hot * (1.0 - e32) if (has_eps and mutant != "no_one_minus_eps") else hot
    g = fma32(p, f[:, None], -h) if zeta > 0 else p - h
    if has_eps and mutant != "no_eps_grad":
        g = g - e32 / Cf
    inv_m = torch.tensor(1.0) / torch.tensor(float(M))
    stop = mutant == "mean_256"
    return obj, nll, g * inv_m, mean_emulate(obj, inv_m, stop), mean_emulate(nll, inv_m, stop)


def _row_err(got, ref):
    """|err| / (u max(1, |ref|)); a +inf reference demands +inf (error 0) and is counted by the caller."""
    inf = torch.isinf(ref)
    err = (got.double() - torch.where(inf, torch.zeros_like(ref), ref)).abs() / (U * ref.abs().clamp_min(1.0))
    return torch.where(inf, torch.where(got.double() == ref, torch.zeros_like(ref), torch.full_like(ref, math.inf)),
                       err)


def _mean_err(got, ref, rows):
    if math.isinf(float(ref)):
        return 0.0 if float(got) == float(ref) else math.inf
    return float((got.double() - ref).abs() / (U * rows.abs().mean()))


def reg_measures(c, gi, obj, nll, dlogits, mean_obj, mean_nll, t=None):
    """{"obj", "nll", "dlogits", "dsum": (M,) errors in u (dlogits: the worst element of the row; both None without
    dlogits), "mean_obj", "mean_nll": floats, "inf_rows": the rows whose reference objective is +inf}."""
    eps, zeta = (f32(v) for v in REG_GRID[gi])
    ref = reg_ref(c, gi) if t is None else reg_ref_uncached(c.x, t, *REG_GRID[gi])
    out = {"obj": _row_err(obj, ref["obj"]), "nll": _row_err(nll, ref["nll"]), "dlogits": None, "dsum": None,
           "mean_obj": _mean_err(mean_obj, ref["mean_obj"], ref["obj"]),
           "mean_nll": _mean_err(mean_nll, ref["mean_nll"], ref["nll"]),
           "inf_rows": torch.nonzero(torch.isinf(ref["obj"])).flatten().tolist()}
    if dlogits is not None:
        scale = (ref["p"] * (1.0 + 2.0 * zeta * ref["lse"].abs())[:, None] + (1.0 - eps) * ref["hot"] + eps / c.C) / c.M
        out["dlogits"] = worst_or_exact((dlogits.double() - ref["dlogits"]).abs(), scale).max(1).values
        out["dsum"] = worst_or_exact((dlogits.double().sum(1) - ref["dlogits"].sum(1)).abs(), scale.sum(1))
    return out


def reg_verdicts(impl, cases=None, grid=None):
    """({(output, family, gi): worst u, ("mean_obj" | "mean_nll", gi): worst u}, judged, excused) of an
    implementation with reg_emulate's signature over every case and grid point of the GPU test.  judged counts the
    (case, grid point, row, output) entries that entered a cell, excused those among them whose reference is +inf
    (they must be +inf, and count as 0 or inf)."""
    worst, judged, excused = {}, 0, 0
    for gi in (range(len(REG_GRID)) if grid is None else grid):
        for c in (reg_cases() if cases is None else cases):
            m = reg_measures(c, gi, *impl(c.x, c.t, *REG_GRID[gi]))
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


def reg_emulation_worst():
    return reg_verdicts(reg_emulate)[0]


def tolerance_of(w):
    return math.ceil(2 * w)


def reg_tol(key):
    if len(key) == 2:
        return REG_MEAN_TOL_U[key]
    return REG_TOL_U[("dlogits",) + key[1:] if key[0] == "dsum" else key]


def reg_failures(worst):
    return sorted((k for k, w in worst.items() if not within(w, reg_tol(k))), key=str)


def mutant_failures(mutant):
    """The cells of the GPU test that reject a mutant."""
    return reg_failures(reg_verdicts(lambda x, t, e, z: reg_emulate(x, t, e, z, mutant))[0])


if __name__ == "__main__":
    table = reg_emulation_worst()
    print("REG_TOL_U = {")
    for k in sorted((k for k in table if len(k) == 3 and k[0] != "dsum"), key=lambda k: (k[2], REG_ROW_OUTPUTS.index(k[0]), k[1])):
        print(f"    {k!r}: {tolerance_of(table[k])},".ljust(44) + f"# 2 x {table[k]:.3f} u")
    print("}\nREG_MEAN_TOL_U = {")
    for k in sorted((k for k in table if len(k) == 2), key=lambda k: (k[1], k[0])):
        print(f"    {k!r}: {tolerance_of(table[k])},".ljust(44) + f"# 2 x {table[k]:.3f} u")
    print("}")
    for k in sorted((k for k in table if k[0] == "dsum"), key=str):
        print("dsum", k, f"{table[k]:.3f}", "of", reg_tol(k) if REG_TOL_U else "-")
    if REG_TOL_U:
        for m in REG_MUTANTS:
            print(m, mutant_failures(m))
