"""Inputs, references, error measure, tolerances and a CPU emulation shared by tests/test_gpu_gemm_selectors.py (the
fp32-result GEMM kernels on an MI355X) and tests/test_gemm_selectors_host.py (the same pieces on the CPU).

WHAT IS UNDER TEST.  csrc/gemm_x3.hip splits every fp32 operand into three bf16 pieces v = h + m + l (round-to-nearest
remainders) and forms a product as six bf16 MFMAs per 16-k step, accumulated in fp32 in the order
lh, hl, mm, mh, hm, hh (A piece first; KERNEL_ORDER).  The product is C(m, n) = sum_k A(m, k) B(n, k): A is held
(M, K) and B (N, K) here, whatever layout the kernel is handed.  A Gaussian product judged by max|err| / max|ref|
cannot see a missing or misrouted LOW piece: it moves the result by ~2^-17 of one term.  The five families below can.

"Full" values are randn * 2^randint(-8, 8): all 24 significant bits in play, mixed signs and magnitudes.
kappa(x) = (p x + c) mod K with odd p coprime to K (p = 37 for the power-of-two K used) is onto 0 .. K-1 once x has
run through K values, and sends neighbouring rows to different k octets, 16-k steps, 32-k tiles and split-K slabs.

  1 `pow2`   B's column n holds 2^e(n), e in [-12, 12], at k = kappa(n) and zeros elsewhere; A is full.  The answer
             A(m, kappa(n)) 2^e(n) is exact, and the kernels' order reaches it exactly: l w, + m w, + h w are partial
             sums of pieces of one value (not every order is: h w + l w rounds).  BIT-EXACT, torch.equal.
  2 `prod`   the same with a full value b(n): C(m, n) = A(m, kappa(n)) b(n), ONE full x full product that holds all
             six cross terms of one (row, k) against one (column, k).  Measure |C - ref| / (u |ref|) per element.
  3 `few`    T = 4 full values per column of B, one in each quarter of K (distinct 16-k steps, 32-k tiles and, under
             split-K, slabs), so the accumulator carries across them.  Measure |C - ref| / (u sum_k |A||B|) per
             element, with `accumulate` |out| joins the sum.
     Each of 1-3 has a MIRROR arm: one-hot / few-term ROWS of A against a full B, which puts B's m and l planes and
     A's one-hot h plane under test.
  4 `scale`  a dense Gaussian product (A0 ~ N(0, 1), B0 ~ 0.05 N(0, 1)) with row m of A scaled by 2^s(m) and column n
             of B by 2^t(n), s, t in [-30, 30]: the split, every product and every addition commute with a power of
             two, so the result is C0(m, n) 2^(s(m) + t(n)) BIT FOR BIT, C0 being the same kernel's result on the
             unscaled operands -- every row and column is checked, not only those a global max|ref| sees.  C0 itself
             must hold the fp32 kernels' global tolerance 2e-6 sqrt(max(1, K / 512)) against fp64.
  5 `nonfinite`  one inf in A(i, k), one NaN in B(j, k'): row i and column j of C non-finite, every other element
             bit-identical to the clean run.

DOMAIN.  All operand magnitudes here are >= 2^-100 (or zero).  Below about 2^-100 the l piece (~2^-17 |v| and less)
drops under 2^-126, the smallest normal bf16; the conversion and the matrix core may flush such a piece, h + m + l
no longer equals v, and the product falls back to two-piece accuracy.  gemm_x3 does not promise more there.

TOLERANCES, u = 2^-24.  Families 1, 4 and 5 take none.  PROD_TOL_U and FEW_TOL_U are TWICE the worst error of the
faithful CPU emulation (`emulate` / `emulate_terms`: pieces by .bfloat16() remainders, each piece product exact in
fp32, one fp32 addition per product in the kernels' order per 16-k step, slabs summed in ascending order, then
`out`) on the GPU test's own inputs, over all its shapes, arms and split counts, rounded up to a whole u
(`emulation_worst`; tests/test_gemm_selectors_host.py recomputes them).  They are not taken from a kernel and are not
to be widened.  The emulation rounds to nearest after every product; the matrix core rounds once per instruction, but
it first aligns the accumulator and the products to the largest exponent and drops what lies below one guard bit
(tools/mfma_rounding_probe.hip), which costs the small-terms accumulator up to 1 u when hh arrives.  Measured
(profiles/r15_gemm_selectors.txt): family 3 at the emulation's 8.07 u, family 2 at 2.77 u where the emulation has 1.71 u,
0.69 of the tolerance; the fp32-MFMA kernels 1.00 u (one correctly rounded product) and 4.3 u."""
import functools
import math
import zlib

import torch

U = 2.0 ** -24
H, M_, L = 0, 1, 2
KERNEL_ORDER = ((L, H), (H, L), (M_, M_), (M_, H), (H, M_), (H, H))       # (A piece, B piece): lh hl mm mh hm hh
INEXACT_ORDER = ((H, H), (L, H), (H, L), (M_, H), (H, M_), (M_, M_))      # h w + l w rounds: family 1 fails on it
T_FEW = 4
PROD_TOL_U = 4.0      # 2 x 1.71 u (emulation_worst("prod")), rounded up
FEW_TOL_U = 17.0      # 2 x 8.07 u (emulation_worst("few")), rounded up

LAYOUTS = ((True, True), (True, False), (False, True), (False, False))       # (a_kcontig, b_kcontig)
GROUPED_LAYOUTS = ((True, True), (True, False), (False, False))              # the host refuses (xc, kc)
SKINNY_MAX_ROWS = 512      # csrc/gemm.hip: M <= 512, both operands [X][K], K % 256 == 0 -> the skinny kernel


def shapes_for(shapes, ak, bk):
    """(M, N, K, splitk) list of one layout.  gemm_dispatch sends (kc, kc) products of M <= 512 rows and K % 256 == 0
    to the skinny-M kernel before it looks at any option, so the K = 256 shapes would never reach the kernel under
    test in that layout: there K becomes 192 (two splits) or 384 (four), every other dispatch condition unchanged."""
    out = []
    for (M, N, K, sk) in shapes:
        if ak and bk and M <= SKINNY_MAX_ROWS and K % 256 == 0:
            K = {2: 192, 4: 384}[sk]
        out.append((M, N, K, sk))
    return out


HALF_SHAPES = ((256, 512, 64, 1), (256, 512, 256, 2), (512, 512, 256, 4))
FULL_SHAPES = ((512, 1024, 64, 1), (512, 1024, 256, 2), (1024, 1024, 512, 4))
AUTO_SHAPES = ((2048, 1536, 64, 1),)
ALL_SHAPES = HALF_SHAPES + FULL_SHAPES + AUTO_SHAPES
# kernel -> (options, shapes); the fp32-MFMA kernels are the control arm: same inputs, same assertions
KERNELS = {
    "x3half": ({"gemm_x3": 1}, HALF_SHAPES),            # gemm_x3_half_kernel: < 192 tile-splits of 128, >= 32 of 64
    "x3full": ({"gemm_x3": 2}, FULL_SHAPES),            # gemm_x3_kernel (the half form asks for == 1): >= 32 tiles
    "x3auto": ({"gemm_x3": 1}, AUTO_SHAPES),            # gemm_x3_kernel by dispatch: 192 tiles, the half form steps aside
    "f32": ({"gemm_x3": 0}, ALL_SHAPES),
    "f32ring": ({"gemm_x3": 0, "gemm_tile64": 0}, ALL_SHAPES),
    "f32regs": ({"gemm_x3": 0, "gemm_dma": 0}, ALL_SHAPES),
}
GROUPED_SHAPES = ((2, 512, 512, 64, 1), (3, 512, 512, 256, 2))      # G, M, N, K, splitk: G tiles splitk >= 32 workgroups
GROUPED_KERNELS = {"x3grouped": {"gemm_x3": 1}, "f32grouped": {"gemm_x3": 0}}


def routes_to(kernel, M, N, K, sk, ak, bk):
    """The dispatch arithmetic of csrc/gemm.hip gemm_dispatch for an aligned, dense, plain-epilogue product: does
    (shape, split, layout) under the kernel's options reach the kernel the case is named after?"""
    if ak and bk and M <= SKINNY_MAX_ROWS and K % 256 == 0:
        return False
    t128 = -(-M // 128) * -(-N // 128)
    per = -(-(-(-K // sk)) // 32) * 32                   # ceil(K / sk), rounded up to whole 32-deep k-tiles
    whole = K % 32 == 0 and K % per == 0
    half = t128 * sk < 192 and (M // 64) * (N // 64) * sk >= 32 and M % 64 == 0 and N % 64 == 0 and whole
    full = M % 128 == 0 and N % 128 == 0 and t128 >= 32 and whole
    if kernel == "x3half":
        return half
    if kernel == "x3full":
        return full
    if kernel == "x3auto":
        return full and not half
    return True


def grouped_routes_to_x3(G, M, N, K, sk):
    return M % 128 == 0 and N % 128 == 0 and K % sk == 0 and (K // sk) % 32 == 0 and G * (M // 128) * (N // 128) * sk >= 32


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def full(shape, gen):
    """fp32 values with all 24 significant bits in play."""
    return torch.randn(shape, generator=gen) * torch.exp2(torch.randint(-8, 9, shape, generator=gen).float())


def stride_of(K):
    p = 37
    while math.gcd(p, K) != 1:
        p += 2
    return p


def kappa(X, K, c):
    """(X,) positions (p x + c) mod K: onto 0 .. K-1 when X >= K."""
    return (stride_of(K) * torch.arange(X) + c) % K


def split3(v):
    """v = h + m + l exactly, as x3_split forms the pieces."""
    h = v.bfloat16().float()
    r = v - h
    m = r.bfloat16().float()
    return h, m, (r - m).bfloat16().float()


class Sparse:
    """Families 1-3: a few-term operand S (X rows of T nonzeros `val` at columns `pos`, ascending) against a full one
    D (Y, K).  S is B and D is A, or the other way round in the mirror arm.  A (M, K), B (N, K) fp32; ref, denom
    (M, N) fp64: the closed-form gather and its absolute-sum scale; out (M, N): what `accumulate` adds to (family 3)."""

    def __init__(self, family, M, N, K, mirror, g=0):
        assert K % 32 == 0 and K <= min(M, N), "kappa must be onto: K <= min(M, N)"
        self.family, self.M, self.N, self.K, self.mirror = family, M, N, K, mirror
        gen = _gen("sparse", family, M, N, K, mirror, g)
        X, Y = (M, N) if mirror else (N, M)
        c = 11 + 5 * g
        if family == "few":
            q = K // T_FEW
            assert q % 16 == 0
            self.pos = torch.stack([t * q + kappa(X, q, c + 7 * t) for t in range(T_FEW)], 1)
            self.val = full((X, T_FEW), gen)
        else:
            self.pos = kappa(X, K, c)[:, None]
            self.val = (torch.exp2(torch.randint(-12, 13, (X, 1), generator=gen).float()) if family == "pow2"
                        else full((X, 1), gen))
        self.D = full((Y, K), gen)
        self.S = torch.zeros((X, K)).scatter_(1, self.pos, self.val)
        self.A, self.B = (self.S, self.D) if mirror else (self.D, self.S)
        Dd, vd = self.D.double(), self.val.double()
        terms = [Dd[:, self.pos[:, t]] * vd[None, :, t] for t in range(self.pos.shape[1])]      # (Y, X) each
        ref, den = sum(terms), sum(t.abs() for t in terms)
        self.ref, self.denom = (ref.t().contiguous(), den.t().contiguous()) if mirror else (ref, den)
        self.out = full((M, N), gen) if family == "few" else None

    def positions(self, m, n):
        return tuple(int(k) for k in self.pos[m if self.mirror else n])

    def target(self, accumulate=False):
        """(ref, denom) of a run, `out` included when it accumulates."""
        if not accumulate:
            return self.ref, self.denom
        return self.ref + self.out.double(), self.denom + self.out.double().abs()


@functools.lru_cache(maxsize=None)
def sparse_case(family, M, N, K, mirror, g=0):
    return Sparse(family, M, N, K, mirror, g)


class Dense:
    """Families 4 and 5: A0 ~ N(0, 1) (M, K), B0 ~ 0.05 N(0, 1) (N, K), the row / column exponents s, t and the fp64
    product of the unscaled operands."""

    def __init__(self, M, N, K, g=0):
        gen = _gen("dense", M, N, K, g)
        self.M, self.N, self.K = M, N, K
        self.A0 = torch.randn((M, K), generator=gen)
        self.B0 = torch.randn((N, K), generator=gen) * 0.05
        self.s = torch.randint(-30, 31, (M,), generator=gen).float()
        self.t = torch.randint(-30, 31, (N,), generator=gen).float()
        self.A = self.A0 * torch.exp2(self.s)[:, None]
        self.B = self.B0 * torch.exp2(self.t)[:, None]
        self.scale = torch.exp2(self.s[:, None] + self.t[None, :])
        self.ref0 = self.A0.double() @ self.B0.double().t()
        self.global_tol = 2e-6 * max(1.0, K / 512) ** 0.5
        # where family 5 puts its inf (A) and its NaN (B)
        self.bad_a, self.bad_b = (M // 2 + 3, 17 % K), (N - 2, K - 5)

    def nonfinite(self):
        A, B = self.A0.clone(), self.B0.clone()
        A[self.bad_a] = float("inf")
        B[self.bad_b] = float("nan")
        return A, B


@functools.lru_cache(maxsize=None)
def dense_case(M, N, K, g=0):
    return Dense(M, N, K, g)


def global_err(C, ref):
    """max|C - ref| / max|ref| (the measure of tests/conftest.py rel_err)."""
    return float((C.double() - ref).abs().max() / ref.abs().max())


def errors_u(C, ref, denom):
    """Per element, |C - ref| in units of u times the element's own scale."""
    return (C.double() - ref).abs() / (U * denom)


def worst_u(C, ref, denom):
    return float(errors_u(C, ref, denom).max())


def failing(C, case, bad, limit=6):
    """The first few (m, n, positions of the few-term side) of the elements marked in `bad`, with got and wanted."""
    idx = bad.nonzero()[:limit]
    return [(int(m), int(n), case.positions(int(m), int(n)), float(C[m, n]), float(case.ref[m, n])) for m, n in idx]


# ---- the kernels' arithmetic on the CPU ------------------------------------------------------------------------------

DROPS = {"drop_lh": (L, H), "drop_hl": (H, L), "drop_mm": (M_, M_), "drop_mh": (M_, H), "drop_hm": (H, M_)}
PLANE_FAULTS = ("rot_l_a", "rot_l_b", "swap_rows_l_a", "swap_rows_l_b", "mm_other_half", "shift_m_b")
MUTANTS = tuple(DROPS) + PLANE_FAULTS


def _rot8(p):
    """k -> the next k inside each group of 8."""
    k = torch.arange(p.shape[1])
    return p[:, (k & ~7) | ((k + 1) & 7)]


def _swap_rows(p):
    """rows 5 and 20 of every 32 exchanged."""
    r = torch.arange(p.shape[0])
    src = torch.where(r % 32 == 5, r + 15, torch.where(r % 32 == 20, r - 15, r))
    return p[src.clamp_max(p.shape[0] - 1)]


def emulate(A, B, order=KERNEL_ORDER, mutant=None, splitk=1, out=None):
    """The six-term sum of gemm_x3 on A (M, K), B (N, K) in fp32 on the CPU: per split-K slab and per 16-k step the
    piece products of `order`, one fp32 addition per product; the slabs summed in ascending order from zero; then `out`.
    mutant: one of MUTANTS -- a small term dropped, A's / B's l plane rotated in k or with two rows of every 32
    exchanged, the mm term reading B's m plane of the other k half, B's m plane shifted by one column."""
    Mr, K = A.shape
    assert B.shape[1] == K and K % (16 * splitk) == 0 and (mutant is None or mutant in MUTANTS)
    pa, pb = list(split3(A)), list(split3(B))
    for x in pa + pb:
        assert torch.isfinite(x).all()
    if mutant == "rot_l_a":
        pa[L] = _rot8(pa[L])
    elif mutant == "rot_l_b":
        pb[L] = _rot8(pb[L])
    elif mutant == "swap_rows_l_a":
        pa[L] = _swap_rows(pa[L])
    elif mutant == "swap_rows_l_b":
        pb[L] = _swap_rows(pb[L])
    elif mutant == "shift_m_b":
        pb[M_] = pb[M_].roll(-1, 0)
    terms = []
    for (i, j) in order:
        if mutant in DROPS and DROPS[mutant] == (i, j):
            continue
        bj = pb[j]
        if mutant == "mm_other_half" and (i, j) == (M_, M_):
            bj = bj[:, torch.arange(K) ^ 8]
        terms.append((pa[i].t().contiguous(), bj.t().contiguous()))       # (K, M), (K, N)
    per = K // splitk
    total = torch.zeros((Mr, B.shape[0]))
    for z in range(splitk):
        acc = torch.zeros((Mr, B.shape[0]))
        for k0 in range(z * per, (z + 1) * per, 16):
            for ta, tb in terms:
                for k in range(k0, k0 + 16):
                    acc += ta[k][:, None] * tb[k][None, :]        # 8 x 8 significant bits: the product is exact
        total = total + acc
    return total if out is None else out + total


def emulate_terms(case, order=KERNEL_ORDER, splitk=1, accumulate=False):
    """`emulate` of a Sparse case without the zero products (they add nothing): the terms of a row lie in distinct
    16-k steps in ascending order, so per slab the sum runs over the terms and, inside each, over `order`.  Equal to
    emulate(case.A, case.B, ...) bit for bit (the host test checks it); cheap enough for the GPU test's shapes."""
    assert case.K % (16 * splitk) == 0
    step = case.pos // 16
    assert (step[:, 1:] > step[:, :-1]).all()
    dp, vp = split3(case.D), split3(case.val)
    per = case.K // splitk
    Y, X = case.D.shape[0], case.val.shape[0]
    total = torch.zeros((Y, X))
    for z in range(splitk):
        acc = torch.zeros((Y, X))
        for t in range(case.pos.shape[1]):
            here = (case.pos[:, t] // per == z).float()[None, :]
            for (i, j) in order:
                pd, pv = (dp[j], vp[i]) if case.mirror else (dp[i], vp[j])
                acc += pd[:, case.pos[:, t]] * (pv[:, t][None, :] * here)
        total = total + acc
    total = total.t().contiguous() if case.mirror else total
    return total + case.out if accumulate else total


def emulation_worst(family):
    """The worst per-element error (in u) of the faithful emulation over everything the GPU test runs of a family:
    every shape of every layout, both arms, its split count, with and without `accumulate` (family 3), every group."""
    shapes = {s for ak, bk in LAYOUTS for s in shapes_for(ALL_SHAPES, ak, bk)}
    cases = [(M, N, K, sk, 0) for (M, N, K, sk) in shapes] + \
            [(M, N, K, sk, g) for (G, M, N, K, sk) in GROUPED_SHAPES for g in range(G)]
    worst = 0.0
    for (M, N, K, sk, g) in sorted(cases):
        for mirror in (False, True):
            c = sparse_case(family, M, N, K, mirror, g)
            for acc in ((False, True) if family == "few" else (False,)):
                ref, den = c.target(acc)
                worst = max(worst, worst_u(emulate_terms(c, splitk=sk, accumulate=acc), ref, den))
    return worst


if __name__ == "__main__":
    for fam in ("prod", "few"):
        w = emulation_worst(fam)
        print(f"{fam}: faithful emulation worst {w:.3f} u -> tolerance {math.ceil(2 * w)} u")
