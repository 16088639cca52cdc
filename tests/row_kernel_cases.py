"""Inputs, fp64 references, per-row measures, CPU emulations and tolerances shared by tests/test_gpu_row_kernels.py
(the row-reduction kernels of csrc/norm.hip and csrc/loss.hip and the LayerNorm prologue of csrc/decode.hip on an
MI355X) and tests/test_row_kernels_host.py (the same pieces on the CPU).

WHAT IS UNDER TEST.  layernorm_fwd_kernel / layernorm_bwd_kernel (one wave per row, two-pass variance, a register
form for D = 256 NV and a scalar form for every other D or a pointer off 16 bytes), ce_reg_rows_kernel<false, false,
false> + mean2_kernel (cross-entropy and its gradient; the per-row losses land in `row_ws`), mse_partial_kernel +
mean2_kernel, and the
LayerNorm the decode step's Linear kernels apply on the way in.  Unit-scale Gaussian rows judged by one global
max|err| / max|ref| cannot see a one-pass variance, a loss rounded at the magnitude of the logits, a row that is only
wrong next to a larger one, or a loop that never takes its second trip.  The families below can.

LAYERNORM ROWS (a case is one (39, D) matrix; 39 is no multiple of the 4 rows of a workgroup):
  unit      randn
  offset    randn + c, c in +-{10, 100, 1000}: a one-pass variance E[x^2] - mean^2 loses rstd here
  scaled    randn 2^s, s in [-20, 20]: rows of very different magnitude, eps in play at the small end
  outlier   randn with one element times 1e4, at lane 0, lane 63, the last column, the last partial 64-chunk
  const     one small integer in every column: the sum is exact, the correctly rounded quotient by D is the integer,
            the variance is 0 -- y == beta | shift | 0 and rstd == 1 / sqrtf(eps) BIT FOR BIT
  nonfinite a copy with one NaN in one row and one inf in another: every other row of every output is unchanged
CROSS-ENTROPY ROWS ((37, C) logits): unit (3 randn), offset (+100, -100, +1000), peak_target / peak_other (+20 at /
  off the target), ties (all logits equal: loss log C, p 1 / C), masked (-inf entries off the target: p == 0 exactly);
  targets at column 0, at C - 1 and inside the last 64-chunk.
MSE DATA: unit; offset (both operands 1000 + k 2^-10: the difference is exact); mixed (per-element scales 2^[-10, 10]).

MEASURES, u = 2^-24, against fp64 on the same fp32 inputs; every row on its own scale:
  mean |mean - ref| / (u mean_c |x|);  rstd |rstd - ref| / (u ref);  y, dx, dy_xhat max_c |got - ref| / (u max_c |ref|)
  row loss |err| / (u max(1, ref));  dlogits |err| / (u (p_ref + [c == t]) / M) per element;  mean loss and MSE loss
  |err| / (u mean |ref rows|) and |err| / (u ref).  Where the scale is exactly 0 the result must equal the reference.

TOLERANCES.  Every entry of LN_TOL_U, CE_TOL_U and MSE_TOL_U is TWICE the worst error of the intended arithmetic
emulated in fp32 on the CPU (`ln_fwd_emulate`, `ln_bwd_emulate`, `ce_emulate`, `mse_emulate`: the kernels' lane
partial sums and 64-lane butterfly, correctly rounded division, sqrt, exp and log) over everything the GPU test
runs, rounded up to a whole u (`ln_emulation_worst`, `ce_emulation_worst`, `mse_emulation_worst`;
tests/test_row_kernels_host.py recomputes them).  They are not taken from a kernel and are not to be widened: the
factor 2 is for the hardware exp / log / rsq (about 1 ulp each) and for the decode kernels' other summation order.
dpred takes the derived 2 u: a - b rounds once and the quotient of 2 (a - b) by n once (a bare product with a
rounded 1 / n would round three times and reach 2.77 u on these inputs; the kernel corrects it by a Newton step).

MUTANTS (`MUTANTS`; the host test proves each is rejected on the GPU test's own inputs, and by which family):
one-pass variance (offset), loss = (mx + log s) - x[t] with p = exp(x - lse) -- the row kernel before this file
existed -- (CE offset), a dropped last partial 64-chunk, a mean that stops at 256 rows, an MSE of one grid trip.

Measured on an MI355X (profiles/row_kernels_measured.txt):
116 (kernel, output, family) figures, 0 above its tolerance; 13 bit-exact.  The GPU sits at the emulation's own worst
in most cells (same lane order, correctly rounded division and root): y offset 764 u of 1529, rstd outlier 3.01 u of 7,
CE dlogits 38.9 u of 78; dpred 1.99 u of the derived 2 (2.77 u with mse_partial_kernel's earlier bare product).
CE offset rows before -> after the shifted form: row loss 311 -> 1.21 u (tolerance 3), dlogits 510 -> 17.9 u
(tolerance 36); ties at |x| = 1000: 313 -> 1.26 u."""
import functools
import math
import zlib

import torch

U = 2.0 ** -24
EPS = 1e-5
EPS32 = float(torch.tensor(EPS, dtype=torch.float32))          # what the C entry receives

# ---- shapes the GPU test runs -----------------------------------------------------------------------------------
LN_M = 39
LN_WIDTHS = (256, 512, 1024, 2048, 768, 100, 65, 63, 32, 1)
LN_UNALIGNED_D = 512
LN_FORMS = ("plain", "affine", "rows", "table")
LN_TABLE_ROWS = 7
LN_FWD_VEC = (256, 512, 1024, 2048)          # qarig_layernorm_fwd: case 1, 2, 4, 8
LN_BWD_VEC = (256, 512, 1024)                # qarig_layernorm_bwd: case 1, 2, 4
LN_FAMILIES = ("unit", "offset", "scaled", "outlier", "const")
LN_OFFSETS = (10.0, -10.0, 100.0, -100.0, 1000.0, -1000.0)
LN_EXPONENTS = tuple(range(-20, 21, 5))
OUTLIER = 1e4
LN_BAD_ROWS = (5, 22)                        # the NaN and the inf of `nonfinite`

DEC_M = (1, 4, 16)
DEC_K = (256, 512, 1024)
DEC_FORMS = ("affine", "rows", "one_row")
DEC_FAMILIES = ("unit", "offset", "scaled", "const")

CE_M = 37
CE_CLASSES = (3, 41, 64, 65, 513, 8193)
CE_MEAN_SHAPES = ((1, 41), (255, 41), (256, 41), (257, 41), (16385, 41))
CE_FAMILIES = ("unit", "offset", "peak_target", "peak_other", "ties", "masked")
CE_OFFSETS = (100.0, -100.0, 1000.0)
CE_BAD_ROWS = (3, 30)                        # get t = C and t = -1

MSE_GRID = 1024 * 256                        # elements one grid trip of mse_partial_kernel covers
MSE_SIZES = (1, 255, 257, MSE_GRID, MSE_GRID + 1, 2 * MSE_GRID + 77)
MSE_FAMILIES = ("unit", "offset", "mixed")
MSE_DPRED_TOL_U = 2.0                        # derived: a - b rounds once, the quotient of 2 (a - b) by n once

# ---- tolerances: ceil(2 x emulation worst), see the module docstring -------------------------------------------
LN_TOL_U = {
    ('mean', 'unit'): 1,                # 2 x 0.377 u
    ('mean', 'offset'): 5,              # 2 x 2.140 u
    ('mean', 'scaled'): 1,              # 2 x 0.354 u
    ('mean', 'outlier'): 6,             # 2 x 2.595 u
    ('mean', 'const'): 0,               # 2 x 0.000 u
    ('rstd', 'unit'): 3,                # 2 x 1.323 u
    ('rstd', 'offset'): 4,              # 2 x 1.974 u
    ('rstd', 'scaled'): 4,              # 2 x 1.626 u
    ('rstd', 'outlier'): 7,             # 2 x 3.013 u
    ('rstd', 'const'): 2,               # 2 x 0.700 u
    ('y', 'unit'): 6,                   # 2 x 2.610 u
    ('y', 'offset'): 1529,              # 2 x 764.385 u
    ('y', 'scaled'): 7,                 # 2 x 3.201 u
    ('y', 'outlier'): 8,                # 2 x 3.604 u
    ('y', 'const'): 0,                  # 2 x 0.000 u
    ('dx', 'unit'): 7,                  # 2 x 3.384 u
    ('dx', 'offset'): 393,              # 2 x 196.311 u
    ('dx', 'scaled'): 8,                # 2 x 3.769 u
    ('dx', 'outlier'): 772,             # 2 x 385.511 u
    ('dx', 'const'): 6,                 # 2 x 2.918 u
    ('dy_xhat', 'unit'): 30,            # 2 x 14.552 u
    ('dy_xhat', 'offset'): 121809,      # 2 x 60904.114 u
    ('dy_xhat', 'scaled'): 27,          # 2 x 13.227 u
    ('dy_xhat', 'outlier'): 183,        # 2 x 91.276 u
    ('dy_xhat', 'const'): 0,            # 2 x 0.000 u
}
CE_TOL_U = {
    ('loss', 'unit'): 8,                # 2 x 3.912 u
    ('loss', 'offset'): 3,              # 2 x 1.213 u
    ('loss', 'peak_target'): 21,        # 2 x 10.352 u
    ('loss', 'peak_other'): 4,          # 2 x 1.551 u
    ('loss', 'ties'): 2,                # 2 x 0.828 u
    ('loss', 'masked'): 3,              # 2 x 1.388 u
    ('dlogits', 'unit'): 70,            # 2 x 34.678 u
    ('dlogits', 'offset'): 36,          # 2 x 17.837 u
    ('dlogits', 'peak_target'): 76,     # 2 x 37.780 u
    ('dlogits', 'peak_other'): 78,      # 2 x 38.853 u
    ('dlogits', 'ties'): 18,            # 2 x 8.532 u
    ('dlogits', 'masked'): 58,          # 2 x 28.972 u
}
CE_MEAN_TOL_U = 4                       # 2 x 1.784 u
MSE_TOL_U = {
    ('loss', 'unit'): 3,                # 2 x 1.381 u
    ('loss', 'offset'): 4,              # 2 x 1.699 u
    ('loss', 'mixed'): 4,               # 2 x 1.608 u
}


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def fma32(a, b, c):
    """fmaf: the product is exact in fp64, the sum rounds there once more before fp32 (2^-29 relative at worst)."""
    return (a.double() * b.double() + c.double()).float()


def exp32(v):
    """expf / logf rounded once (through fp64: the same on every host, unlike a vectorised fp32 routine)."""
    return torch.exp(v.double()).float()


def log32(v):
    return torch.log(v.double()).float()


def butterfly(v):
    """wave_sum of csrc/qarig_common.h on (R, 64) lane values: v += shfl_xor(v, o), o = 32 ... 1."""
    lane = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lane ^ o]
    return v[:, 0]


def _chunks(v, fill=0.0):
    """(R, C) -> (R, ceil(C / 64), 64): column c sits on lane c % 64 at trip c // 64; the padding adds nothing."""
    R, C = v.shape
    n = -(-C // 64)
    out = torch.full((R, n * 64), fill, dtype=v.dtype)
    out[:, :C] = v
    return out.view(R, n, 64)


def _drop_tail(v, fill=0.0):
    """The mutant: the last, partial 64-chunk of every row never enters the reduction."""
    C = v.shape[1]
    if C % 64 == 0 or C < 64:
        return v
    v = v.clone()
    v[:, (C // 64) * 64:] = fill
    return v


def row_sum(v, vec=False, drop_tail=False):
    """Sum over the columns as the row kernels form it: per lane in ascending trips, then the butterfly.
    vec: the register form, lane l holds columns 4 (64 i + l) ... + 3 of trip i and adds (x + y) + (z + w)."""
    if vec:
        q = v.view(v.shape[0], -1, 64, 4)
        acc = torch.zeros((v.shape[0], 64))
        for i in range(q.shape[1]):
            acc = acc + ((q[:, i, :, 0] + q[:, i, :, 1]) + (q[:, i, :, 2] + q[:, i, :, 3]))
        return butterfly(acc)
    ch = _chunks(_drop_tail(v) if drop_tail else v)
    acc = torch.zeros((v.shape[0], 64))
    for k in range(ch.shape[1]):
        acc = acc + ch[:, k]
    return butterfly(acc)


def row_dot(a, b, vec=False, drop_tail=False):
    """sum_c a b with one fmaf per column, lanes and trips as in row_sum."""
    acc = torch.zeros((a.shape[0], 64))
    if vec:
        qa, qb = a.view(a.shape[0], -1, 64, 4), b.view(a.shape[0], -1, 64, 4)
        for i in range(qa.shape[1]):
            for j in range(4):
                acc = fma32(qa[:, i, :, j], qb[:, i, :, j], acc)
        return butterfly(acc)
    if drop_tail:
        a, b = _drop_tail(a), _drop_tail(b)
    ca, cb = _chunks(a), _chunks(b)
    for k in range(ca.shape[1]):
        acc = fma32(ca[:, k], cb[:, k], acc)
    return butterfly(acc)


def worse(a, b):
    """The larger of two error figures; a NaN is the worst there is and stays."""
    return a if a != a or b <= a else b


def within(w, tol):
    return bool(w <= tol)          # a NaN is not


def worst_or_exact(err, den):
    """err / (u den) per entry; where the scale is exactly 0 the result must be the reference: 0 or inf."""
    zero = den == 0
    out = err / (U * torch.where(zero, torch.ones_like(den), den))
    return torch.where(zero, torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, math.inf)), out)


# ==== LayerNorm ==================================================================================================

class LNCase:
    """x (M, D) fp32 with `family[r]` naming row r's family, the operands of the four forms, the two dy and dx_add."""

    def __init__(self, D, M=LN_M, tag="train", families=LN_FAMILIES):
        gen = _gen("ln", tag, M, D)
        self.M, self.D = M, D
        fams, param = [], []
        if tag == "train":
            assert M == LN_M
            spec = [("unit", None)] * 6 + [("offset", c) for c in LN_OFFSETS * 2] + \
                   [("scaled", s) for s in LN_EXPONENTS] + [("outlier", k) for k in (0, 1, 2, 3) * 2] + \
                   [("const", c) for c in (3, -7, 12, 1)]
            perm = torch.randperm(M, generator=gen).tolist()
            spec = [spec[i] for i in perm]
        else:       # the decode rows: the families in turn
            spec = []
            for r in range(M):
                f = families[r % len(families)]
                i = r // len(families)
                spec.append((f, {"unit": None, "offset": (1000.0, -100.0, 10.0, -1000.0)[i % 4],
                                 "scaled": (-20, 20, -10, 5)[i % 4], "const": (3, -7, 12, 1)[i % 4]}[f]))
        x = torch.randn((M, D), generator=gen)
        last = D - 1
        self.outlier_cols = (0, min(63, last), last, 64 * (last // 64) + (last % 64) // 2)
        for r, (f, a) in enumerate(spec):
            fams.append(f)
            param.append(a)
            if f == "offset":
                x[r] += a
            elif f == "scaled":
                x[r] *= 2.0 ** a
            elif f == "outlier":
                x[r, self.outlier_cols[a]] *= OUTLIER
            elif f == "const":
                x[r] = float(a)
        self.x, self.family, self.param = x, tuple(fams), tuple(param)
        self.gamma = torch.randn(D, generator=gen) * 0.5 + 1.0
        self.beta = torch.randn(D, generator=gen)
        self.scale = torch.randn((M, D), generator=gen) * 0.5 + 1.0
        self.shift = torch.randn((M, D), generator=gen)
        P = LN_TABLE_ROWS
        self.tab_scale = torch.randn((P, D), generator=gen) * 0.5 + 1.0
        self.tab_shift = torch.randn((P, D), generator=gen)
        # permuted, repeated, with 0 and P - 1
        self.mod_idx = ((5 * torch.arange(M) + 6) % P).to(torch.int32)
        self.dy = {"full": torch.randn((M, D), generator=gen), "onehot": torch.zeros((M, D))}
        hot = (37 * torch.arange(M) + 11) % D
        self.dy["onehot"][torch.arange(M), hot] = torch.randn(M, generator=gen) + 2.0
        self.dx_add = torch.randn((M, D), generator=gen)

    def rows(self, family):
        return [r for r, f in enumerate(self.family) if f == family]

    def operands(self, form):
        """(gamma, beta, scale, shift, mod_idx) as the entry takes them, and the (M, D) multiplier and addend."""
        one, zero = torch.ones((self.M, self.D)), torch.zeros((self.M, self.D))
        if form == "plain":
            return (None,) * 5, one, zero
        if form == "affine":
            mul, add = self.gamma.expand(self.M, -1), self.beta.expand(self.M, -1)
            return (self.gamma, self.beta, None, None, None), mul, add
        if form == "rows":
            return (None, None, self.scale, self.shift, None), self.scale, self.shift
        idx = self.mod_idx.long()
        return (None, None, self.tab_scale, self.tab_shift, self.mod_idx), self.tab_scale[idx], self.tab_shift[idx]

    def nonfinite(self):
        x = self.x.clone()
        x[LN_BAD_ROWS[0], self.D // 3] = float("nan")
        x[LN_BAD_ROWS[1], self.D - 1] = float("inf")
        return x


@functools.lru_cache(maxsize=None)
def ln_case(D, M=LN_M, tag="train"):
    return LNCase(D, M, tag, LN_FAMILIES if tag == "train" else DEC_FAMILIES)


def ln_fwd_ref(x, mul, add):
    """fp64 LayerNorm (biased variance, eps inside the root) of fp32 x: mean, rstd (M,), xhat, y (M, D)."""
    xd = x.double()
    mean = xd.mean(1)
    xc = xd - mean[:, None]
    rstd = 1.0 / torch.sqrt((xc * xc).mean(1) + EPS32)
    xhat = xc * rstd[:, None]
    return mean, rstd, xhat, mul.double() * xhat + add.double()


def ln_bwd_ref(x, dy, mul, dx_add=None):
    """fp64: dx = rstd (g - mean(g) - xhat mean(g xhat)), g = dy mul; dy_xhat = dy xhat."""
    _, rstd, xhat, _ = ln_fwd_ref(x, mul, mul)
    g = dy.double() * mul.double()
    dx = rstd[:, None] * (g - g.mean(1, keepdim=True) - xhat * (g * xhat).mean(1, keepdim=True))
    if dx_add is not None:
        dx = dx + dx_add.double()
    return dx, dy.double() * xhat


def ln_fwd_emulate(x, form, mul, add, vec, mutant=None):
    """layernorm_fwd_kernel in fp32 on the CPU: two passes, the kernel's lane sums, IEEE division and root.
    mutant: "one_pass" (var = E[x^2] - mean^2) or "drop_tail"."""
    D = x.shape[1]
    drop = mutant == "drop_tail"
    vec = vec and not drop
    Df = torch.tensor(float(D))
    mean = row_sum(x, vec, drop) / Df
    xc = x - mean[:, None]
    if mutant == "one_pass":
        var = row_dot(x, x, vec) / Df - mean * mean
    else:
        var = row_dot(xc, xc, vec, drop) / Df
    rstd = 1.0 / torch.sqrt(var + torch.tensor(EPS, dtype=torch.float32))
    h = xc * rstd[:, None]
    y = h if form == "plain" else (h * mul + add)       # h * g + b and g * h + b round alike
    return mean, rstd, y


def ln_bwd_emulate(x, dy, mean, rstd, form, mul, dx_add, vec, mutant=None):
    """layernorm_bwd_kernel in fp32 on the CPU, fed with a forward's mean and rstd."""
    D = x.shape[1]
    drop = mutant == "drop_tail"
    vec = vec and not drop
    Df = torch.tensor(float(D))
    h = (x - mean[:, None]) * rstd[:, None]
    g = dy if form == "plain" else dy * mul
    s1 = (row_sum(g, vec, drop) / Df)[:, None]
    s2 = (row_dot(g, h, vec, drop) / Df)[:, None]
    r = rstd[:, None] * ((g - s1) - h * s2)
    if dx_add is not None:
        r = dx_add + r
    return r, dy * h


def ln_measures(x, got, ref):
    """{output: (M,) errors in u}: got / ref hold any of mean, rstd, y, dx, dy_xhat."""
    out = {}
    for k in got:
        err = (got[k].double() - ref[k]).abs()
        if k == "mean":
            out[k] = worst_or_exact(err, x.double().abs().mean(1))
        elif k == "rstd":
            out[k] = worst_or_exact(err, ref[k])
        else:
            out[k] = worst_or_exact(err.max(1).values, ref[k].abs().max(1).values)
    return out


def ln_runs():
    """Every LayerNorm run of the GPU test: (case, fwd_vec, bwd_vec, label)."""
    runs = [(ln_case(D), D in LN_FWD_VEC, D in LN_BWD_VEC, f"D={D}") for D in LN_WIDTHS]
    runs.append((ln_case(LN_UNALIGNED_D, tag="train"), False, False, f"D={LN_UNALIGNED_D} unaligned"))
    return runs


BWD_ARMS = tuple((kind, add) for kind in ("full", "onehot") for add in (False, True))


def ln_verdicts(fwd, bwd, runs=None, decode=True):
    """Runs every LayerNorm assertion of the GPU test on an implementation given as two functions with the
    emulations' signatures, and returns {(output, family): worst u} (const rows of the forward outputs appear as
    0 when bit-exact, inf when not).  This is what both the tolerances and the mutant proofs are made of."""
    worst = {}

    def note(c, m):
        for k, e in m.items():
            for fam in set(c.family):
                worst[(k, fam)] = worse(worst.get((k, fam), 0.0), float(e[c.rows(fam)].max()))

    for c, fv, bv, _ in (ln_runs() if runs is None else runs):
        for form in LN_FORMS:
            _, mul, add = c.operands(form)
            rm, rr, _, ry = ln_fwd_ref(c.x, mul, add)
            mean, rstd, y = fwd(c.x, form, mul, add, fv)
            note(c, ln_measures(c.x, {"mean": mean, "rstd": rstd, "y": y}, {"mean": rm, "rstd": rr, "y": ry}))
            for kind, with_add in BWD_ARMS:
                a = c.dx_add if with_add else None
                rdx, rdh = ln_bwd_ref(c.x, c.dy[kind], mul, a)
                dx, dh = bwd(c.x, c.dy[kind], mean, rstd, form, mul, a, bv)
                note(c, ln_measures(c.x, {"dx": dx, "dy_xhat": dh}, {"dx": rdx, "dy_xhat": rdh}))
    if decode:
        for K in DEC_K:
            c = ln_case(K, max(DEC_M), "decode")
            for form in DEC_FORMS:
                mul, add = dec_operands(c, form)
                _, _, _, ry = ln_fwd_ref(c.x, mul, add)
                _, _, y = fwd(c.x, "affine", mul, add, False)
                note(c, ln_measures(c.x, {"y": y}, {"y": ry}))
    return worst


def dec_operands(c, form):
    """The (M, K) multiplier and addend of a decode form: gamma / beta, scale / shift rows, or ONE scale / shift row."""
    if form == "affine":
        return c.gamma.expand(c.M, -1), c.beta.expand(c.M, -1)
    if form == "rows":
        return c.scale, c.shift
    return c.scale[0].expand(c.M, -1), c.shift[0].expand(c.M, -1)


def dec_kappa(K):
    """Row n of the selector weight is one-hot at kappa(n) = (37 n + 11) mod K, N = K: onto (37 is odd)."""
    return (37 * torch.arange(K) + 11) % K


def dec_weight(K):
    W = torch.zeros((K, K))
    W[torch.arange(K), dec_kappa(K)] = 1.0
    return W


def ln_emulation_worst():
    return ln_verdicts(ln_fwd_emulate, ln_bwd_emulate)


def tolerance_of(worst):
    return math.ceil(2 * worst)


def ln_failures(worst):
    """The (output, family) pairs of a verdict table that the GPU test would fail."""
    return sorted(k for k, w in worst.items() if not within(w, LN_TOL_U[k]))


# ==== cross-entropy ==============================================================================================

class CECase:
    """logits (M, C) fp32, target (M,) int64, family[r]."""

    def __init__(self, M, C, mixed=True):
        gen = _gen("ce", M, C, mixed)
        self.M, self.C = M, C
        x = 3.0 * torch.randn((M, C), generator=gen)
        last = C - 1
        places = (0, last, 64 * (last // 64) + (last % 64) // 2)
        t = torch.randint(0, C, (M,), generator=gen)
        fams = ["unit"] * M
        if mixed:
            assert M == CE_M
            spec = ["unit"] * 11 + ["offset"] * 9 + ["peak_target"] * 4 + ["peak_other"] * 4 + ["ties"] * 4 + \
                   ["masked"] * 5
            perm = torch.randperm(M, generator=gen).tolist()
            fams = [spec[i] for i in perm]
            seen = {}
            for r, f in enumerate(fams):
                i = seen[f] = seen.get(f, -1) + 1
                if i < 3 or f in ("offset", "masked"):
                    t[r] = places[i % 3]                     # every family meets the three target places
                tr = int(t[r])
                if f == "offset":
                    x[r] += CE_OFFSETS[i // 3]
                elif f == "peak_target":
                    x[r, tr] += 20.0
                elif f == "peak_other":
                    x[r, (tr + 1 + i % (C - 1)) % C] += 20.0
                elif f == "ties":
                    x[r] = (2.5, -100.0, 1000.0, 0.0)[i % 4]
                elif f == "masked":
                    n = max(1, min(5, C // 3))
                    cols = (tr + 1 + torch.arange(n) * max(1, (C - 1) // n)) % C
                    cols = cols[cols != tr]
                    x[r, cols] = -math.inf
        self.x, self.t, self.family = x, t, tuple(fams)

    def rows(self, family):
        return [r for r, f in enumerate(self.family) if f == family]

    def bad_targets(self):
        t = self.t.clone()
        t[CE_BAD_ROWS[0]] = self.C
        t[CE_BAD_ROWS[1]] = -1
        return t


@functools.lru_cache(maxsize=None)
def ce_case(M, C, mixed=True):
    return CECase(M, C, mixed)


def ce_cases():
    return [ce_case(CE_M, C) for C in CE_CLASSES] + [ce_case(M, C, False) for M, C in CE_MEAN_SHAPES]


def ce_ref(x, t):
    """fp64: row losses (M,), softmax (M, C), dlogits of the mean loss (M, C), the mean loss."""
    xd = x.double()
    lse = torch.logsumexp(xd, 1)
    loss = lse - xd[torch.arange(x.shape[0]), t]
    p = torch.exp(xd - lse[:, None])
    hot = torch.zeros_like(p)
    hot[torch.arange(x.shape[0]), t] = 1.0
    return loss, p, (p - hot) / x.shape[0], loss.mean()


def mean_emulate(v, inv, stop_at_256=False):
    """mean2_kernel, one block: 256 strided partial sums, a tree, times inv.  The mutant never takes a second trip."""
    n = v.shape[0]
    trips = -(-n // 256)
    pad = torch.zeros(trips * 256)
    pad[:n] = v
    pad = pad.view(trips, 256)
    s = torch.zeros(256)
    for k in range(1 if stop_at_256 else trips):
        s = s + pad[k]
    o = 128
    while o > 0:
        s = s[:o] + s[o:2 * o]
        o >>= 1
    return s[0] * inv


def ce_emulate(x, t, mutant=None):
    """The plain cross-entropy (ce_reg_rows_kernel<false, false, false> + mean2_kernel) in fp32 on the CPU, the shifted form: loss = log s - (x[t] - mx),
    p = exp((x - mx) - log s).  mutant "lse": loss = (mx + log s) - x[t], p = exp(x - (mx + log s));
    "drop_tail", "mean_256" as named.  Returns row losses, dlogits, the mean loss."""
    M, C = x.shape
    drop = mutant == "drop_tail"
    xm = _drop_tail(x, -math.inf) if drop else x
    mx = xm.max(1).values
    e = exp32(xm - mx[:, None])
    s = row_sum(e)
    logs = log32(s)
    xt = x[torch.arange(M), t]
    if mutant == "lse":
        lse = mx + logs
        loss = lse - xt
        p = exp32(x - lse[:, None])
    else:
        loss = logs - (xt - mx)
        p = exp32((x - mx[:, None]) - logs[:, None])
    hot = torch.zeros_like(p)
    hot[torch.arange(M), t] = 1.0
    inv_m = torch.tensor(1.0) / torch.tensor(float(M))
    return loss, (p - hot) * inv_m, mean_emulate(loss, inv_m, mutant == "mean_256")


def ce_measures(c, loss, dlogits, mean, t=None):
    """(row loss errors (M,), dlogits errors per row (M,): the worst element, gradient-sum errors (M,) in units of
    the summed per-element scale, the mean loss error), all in u."""
    t = c.t if t is None else t
    rl, rp, rd, rmean = ce_ref(c.x, t)
    e_loss = (loss.double() - rl).abs() / (U * rl.clamp_min(1.0))
    out = [e_loss, None, None, float((mean.double() - rmean).abs() / (U * rl.abs().mean()))]
    if dlogits is not None:
        hot = torch.zeros_like(rp)
        hot[torch.arange(c.M), t] = 1.0
        scale = (rp + hot) / c.M
        out[1] = worst_or_exact((dlogits.double() - rd).abs(), scale).max(1).values
        out[2] = dlogits.double().sum(1).abs() / (U * scale.sum(1))
    return out


def ce_verdicts(impl, cases=None):
    """{("loss" | "dlogits" | "dsum", family): worst u} and {"mean": worst u} of an implementation with ce_emulate's
    signature over every cross-entropy case of the GPU test."""
    worst = {}
    for c in (ce_cases() if cases is None else cases):
        loss, d, mean = impl(c.x, c.t)
        e_loss, e_d, e_sum, e_mean = ce_measures(c, loss, d, mean)
        for fam in set(c.family):
            r = c.rows(fam)
            for k, e in (("loss", e_loss), ("dlogits", e_d), ("dsum", e_sum)):
                worst[(k, fam)] = worse(worst.get((k, fam), 0.0), float(e[r].max()))
        worst["mean"] = worse(worst.get("mean", 0.0), e_mean)
    return worst


def ce_emulation_worst():
    return ce_verdicts(ce_emulate)


def ce_tol(key):
    """The gradient sum of a row is bounded by the summed per-element bound: dlogits' tolerance on the summed scale."""
    if key == "mean":
        return CE_MEAN_TOL_U
    return CE_TOL_U[("dlogits", key[1]) if key[0] == "dsum" else key]


def ce_failures(worst):
    return sorted((k for k, w in worst.items() if not within(w, ce_tol(k))), key=str)


# ==== MSE ========================================================================================================

@functools.lru_cache(maxsize=None)
def mse_case(n, family):
    """(pred, target) (n,) fp32."""
    gen = _gen("mse", n, family)
    if family == "unit":
        return torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    if family == "offset":
        ka = torch.randint(-512, 513, (n,), generator=gen)
        kb = torch.randint(-512, 513, (n,), generator=gen)
        kb = torch.where(kb == ka, kb + 1, kb)
        return 1000.0 + ka.float() * 2.0 ** -10, 1000.0 + kb.float() * 2.0 ** -10
    sc = torch.exp2(torch.randint(-10, 11, (n,), generator=gen).float())
    return torch.randn(n, generator=gen) * sc, torch.randn(n, generator=gen) * sc


def mse_ref(a, b):
    d = a.double() - b.double()
    return (d * d).mean(), 2.0 * d / a.numel()


def mse_emulate(a, b, mutant=None):
    """mse_partial_kernel + mean2_kernel: 1024 x 256 threads, one fmaf per element in ascending grid trips, a tree
    per block, then the mean of the 1024 partial sums.  mutant "one_trip": elements past the first trip are lost."""
    n = a.numel()
    inv_n = torch.tensor(1.0) / torch.tensor(float(n))
    d = a - b
    trips = -(-n // MSE_GRID)
    pad = torch.zeros(trips * MSE_GRID)
    pad[:n] = d
    pad = pad.view(trips, 1024, 256)
    s = torch.zeros((1024, 256))
    for k in range(1 if mutant == "one_trip" else trips):
        s = fma32(pad[k], pad[k], s)
    o = 128
    while o > 0:
        s = s[:, :o] + s[:, o:2 * o]
        o >>= 1
    t2 = 2.0 * d                                   # exact
    q = t2 * inv_n
    dp = fma32(fma32(-q, torch.tensor(float(n)), t2), inv_n, q)      # one Newton step: the quotient, once rounded
    if mutant == "one_trip":
        dp[MSE_GRID:] = 0.0
    return mean_emulate(s[:, 0], inv_n), dp


def mse_measures(a, b, loss, dpred):
    """(loss error, worst dpred error) in u, each relative to its own reference."""
    rl, rd = mse_ref(a, b)
    e = float(worst_or_exact((loss.double() - rl).abs().reshape(1), rl.reshape(1)))
    if dpred is None:
        return e, None
    return e, float(worst_or_exact((dpred.double() - rd).abs(), rd.abs()).max())


def mse_verdicts(impl):
    """{("loss" | "dpred", family): worst u} over every MSE case of the GPU test."""
    worst = {}
    for fam in MSE_FAMILIES:
        for n in MSE_SIZES:
            a, b = mse_case(n, fam)
            e, ed = mse_measures(a, b, *impl(a, b))
            worst[("loss", fam)] = worse(worst.get(("loss", fam), 0.0), e)
            worst[("dpred", fam)] = worse(worst.get(("dpred", fam), 0.0), ed)
    return worst


def mse_emulation_worst():
    return mse_verdicts(mse_emulate)


def mse_tol(key):
    return MSE_DPRED_TOL_U if key[0] == "dpred" else MSE_TOL_U[key]


def mse_failures(worst):
    return sorted(k for k, w in worst.items() if not within(w, mse_tol(k)))


MUTANTS = ("one_pass", "lse", "drop_tail", "mean_256", "one_trip")


def mutant_verdicts(mutant):
    """{"ln" | "ce" | "mse": failed keys} of a mutant over the GPU test's inputs (the kernels it does not touch are
    left out)."""
    out = {}
    if mutant in ("one_pass", "drop_tail"):
        out["ln"] = ln_failures(ln_verdicts(lambda *a: ln_fwd_emulate(*a, mutant=mutant),
                                            lambda *a: ln_bwd_emulate(*a, mutant=mutant), decode=False))
    if mutant in ("lse", "drop_tail", "mean_256"):
        out["ce"] = ce_failures(ce_verdicts(lambda x, t: ce_emulate(x, t, mutant)))
    if mutant == "one_trip":
        out["mse"] = mse_failures(mse_verdicts(lambda a, b: mse_emulate(a, b, mutant)))
    return out


if __name__ == "__main__":
    for name, table in (("LN_TOL_U", ln_emulation_worst()), ("CE_TOL_U", ce_emulation_worst()),
                        ("MSE_TOL_U", mse_emulation_worst())):
        print(name)
        for k in sorted(table, key=str):
            print(f"    {k!r}: {tolerance_of(table[k])},      # 2 x {table[k]:.3f} u")
    for m in MUTANTS:
        print(m, mutant_verdicts(m))
