"""Shared inputs, longdouble references, derived tolerances and check families of the k-nearest-neighbour tests
(csrc/knn.hip qarig_knn_smallest / qarig_ball_count, qarig/gen_eval.py manifold_metrics).  The families take a
*backend* with knn(q, x, k, shift, self_offset) -> (d2, idx) and ball(q, x, r2, shift, self_offset) -> count on NumPy
arrays: the GPU ops (tests/test_gpu_gen_knn.py) or the NumPy emulation of the two entries' definitions in this file
(tests/test_gen_knn_host.py, which also feeds the families eleven mutants of it: a family that accepts a wrong kernel
proves nothing).

Reference.  d2_ref(i, j) = sum_c (q_ic - x_jc)^2 by direct differences in np.longdouble (the shift cancels); where
longdouble is not wider than fp64 every bound is doubled (SLACK, as in gen_eval_cases).

Tolerance, per pair (derived, not tuned).  With a_i = fl(q_i - shift), b_j = fl(x_j - shift), u = 2^-53 and
A_ij = sum_c |a_ic| |b_jc|, the kernel's d2 = (|a_i|^2 + |b_j|^2) - 2 a_i . b_j obeys
    |got - ref| <= (D + 8) u (|a_i|^2 + |b_j|^2 + 2 A_ij):
each of the three sums of D products commits at most D roundings relative to its absolute-value sum (D - 1 additions in
any order -- the MFMA's ascending steps of four, the norms' strided lanes and butterfly -- and one rounding per
product, fused or not); the shift subtraction commits one rounding per factor, two per product; the addition of the
norms and the final subtraction commit one each, relative to at most the bracket.  That is D + 4 per sum at most, the
remaining 4 u cover second-order terms.

An order statistic moves by at most the largest perturbation of its row: the t-th smallest value of a row is checked
against the reference's t-th smallest within the row's largest pair bound.  A returned index may differ from the
reference's only where the reference's neighbouring order statistics lie within twice that bound of each other; a
pair may be counted inside a ball or outside only where |d2_ref - r2_j| is within its bound.  Both excuses are capped
at 1 % of a case's entries, and the inputs are chosen so that the reference excuses none (ambiguities(), asserted on
the host): in effect indices and counts must be equal.

Exact families.  Integer features in -3 ... 3 and an integer shift make every difference, product, sum and distance
exact in fp64 in any order: bit equality with a stable lexsort by (value, index) and with the brute-force count is
demanded, with ties by the hundred (rows repeat at small D) and radii that sit exactly on distances.

Shapes.  The kernel's column block is 64 x rows, its query block 64 rows (16 per wave), its feature chunk 32 and the
MFMA step 4; a workgroup sweeps 4 column blocks, so nx = 257 is the first size whose x axis is split over workgroups
and merged.  DIMS adds 31, 32, 33 (the chunk's edges) to the sizes around 4, 16, 64 and 128."""
import functools

import numpy as np

LD = np.longdouble
WIDE = np.finfo(LD).eps < np.finfo(np.float64).eps
SLACK = 1.0 if WIDE else 2.0
U = 2.0 ** -53

DIMS = (1, 3, 4, 5, 16, 17, 31, 32, 33, 63, 64, 65, 130)
NQS = (1, 2, 15, 16, 17, 65)
NXS = (9, 16, 17, 63, 64, 65, 129, 257)
KS = (1, 3, 8)
K_MAIN = 3
OFFSETS = (0.0, 1000.0)
BIG = dict(nq=70, nx=1100, D=1024, k=5)
EXCUSE_CAP = 0.01
COL_BLOCK = 64

MUTANTS = ("self_not_excluded", "self_by_value", "tie_high_index", "ball_strict", "query_radius", "k_plus_1",
           "partial_block_dropped", "padded_rows_candidates", "shift_ignored", "shift_on_padding", "f32_row_map")


# ---------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------
def rows(kind, n, D, seed, offset=0.0):
    """Rows 0.7 N(0,1) + 0.3 (+ offset), seeded per (seed, n, D); or small integers in -3 ... 3."""
    rng = np.random.default_rng([seed, n, D, 0 if kind == "gauss" else 1])
    if kind == "gauss":
        return rng.standard_normal((n, D)) * 0.7 + 0.3 + offset
    return rng.integers(-3, 4, size=(n, D)).astype(np.float64)


def shift_of(x):
    """The mean of the first 8 x rows, as GenerationScorer takes the first real batch's."""
    return x[:8].mean(axis=0)


@functools.lru_cache(maxsize=None)
def case(nq, nx, D, offset, own, k=K_MAIN):
    """One real-valued case.  own: the queries ARE x rows self_offset ... self_offset + nq - 1 (self_offset = nx - nq,
    the largest allowed) and self is excluded; otherwise an independent query set and self_offset = -1.  Holds the
    longdouble reference, the pair bounds and the radii (the midpoint between an x row's k-th and (k+1)-th own
    reference distance; every membership is judged against the longdouble d2_ref(q, x) and these radii).  Arrays are
    shared between tests: nobody writes to them."""
    x = rows("gauss", nx, D, 1, offset)
    self_offset = nx - nq if own else -1
    q = x[self_offset:self_offset + nq] if own else rows("gauss", nq, D, 2, offset)
    shift = shift_of(x)
    ref = ref_d2(q, x)
    if nx * nx * D <= 1 << 24:
        own_d2 = ref_d2(x, x).astype(np.float64)
    else:       # the largest case: fp64 Gram form about the shift; only the radii come from it, no check is made against it
        b = x - shift
        own_d2 = (b * b).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2.0 * (b @ b.T)
    np.fill_diagonal(own_d2, np.inf)
    s = np.sort(own_d2, axis=1)
    r2 = 0.5 * (s[:, k - 1] + s[:, k]) if nx >= k + 2 else None
    c = dict(q=q, x=x, shift=shift, self_offset=self_offset, k=k, ref=ref, bound=pair_bound(q, x, shift), r2=r2,
             cand=candidates(nq, nx, self_offset))
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def candidates(nq, nx, self_offset):
    m = np.ones((nq, nx), bool)
    if self_offset >= 0:
        m[np.arange(nq), self_offset + np.arange(nq)] = False
    return m


# ---------------------------------------------------------------------------------------------------------------
# references and bounds
# ---------------------------------------------------------------------------------------------------------------
def ref_d2(q, x):
    """(nq, nx) longdouble squared distances by direct differences, a query row at a time."""
    xl = x.astype(LD)
    out = np.empty((q.shape[0], x.shape[0]), LD)
    for i in range(q.shape[0]):
        d = xl - q[i].astype(LD)
        out[i] = (d * d).sum(axis=1)
    return out


def pair_bound(q, x, shift, D=None):
    a = np.abs(q - (0 if shift is None else shift))
    b = np.abs(x - (0 if shift is None else shift))
    D = q.shape[1] if D is None else D
    return SLACK * (D + 8) * U * ((a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] + 2.0 * (a @ b.T))


def ref_smallest(ref, cand, k):
    """(values, indices, the (k+1)-th value or inf) of the reference under (value, index) order, candidates only."""
    d = np.where(cand, ref.astype(np.float64), np.inf)
    order = np.lexsort((np.broadcast_to(np.arange(d.shape[1]), d.shape), d), axis=1)
    s = np.take_along_axis(d, order, axis=1)
    nxt = s[:, k] if d.shape[1] > k else np.full(d.shape[0], np.inf)
    return s[:, :k], order[:, :k].astype(np.int32), nxt


def ambiguities(c):
    """(ambiguous (row, rank) entries, undecided pairs) of the reference alone: entries whose neighbouring reference
    order statistics lie within twice the row's bound, pairs with |d2_ref - r2_j| within their bound."""
    vals, _, nxt = ref_smallest(c["ref"], c["cand"], c["k"])
    rb = np.where(c["cand"], c["bound"], 0.0).max(axis=1)
    gaps = np.diff(np.concatenate((vals, nxt[:, None]), axis=1), axis=1)
    amb = int((gaps <= 2 * rb[:, None]).sum())
    und = 0
    if c["r2"] is not None:
        und = int((c["cand"] & (np.abs(c["ref"].astype(np.float64) - c["r2"][None, :]) <= c["bound"])).sum())
    return amb, und


def ref_metrics(real, gen, k):
    """Brute-force precision / recall / density / coverage in fp64 NumPy (direct differences)."""
    def d2(a, b):
        return ((a[:, None, :] - b[None, :, :]) ** 2).sum(axis=2)

    def radii(a):
        d = d2(a, a)
        np.fill_diagonal(d, np.inf)
        return np.sort(d, axis=1)[:, k - 1]
    rr, rg = radii(real), radii(gen)
    gr = d2(gen, real)                                   # (m, n)
    in_real = (gr <= rr[None, :]).sum(axis=1)
    in_gen = (gr.T <= rg[None, :]).sum(axis=1)
    return {"precision": float((in_real > 0).mean()), "recall": float((in_gen > 0).mean()),
            "density": float(in_real.sum() / (k * gen.shape[0])),
            "coverage": float((gr.min(axis=0) <= rr).mean())}


# ---------------------------------------------------------------------------------------------------------------
# NumPy emulation of the two entries' definitions, and its mutants
# ---------------------------------------------------------------------------------------------------------------
def _norms(a):
    """|a_r|^2 in the kernel's order: lane l sums the features l, l + 64, ... ascending, then a butterfly."""
    s = np.zeros((a.shape[0], 64))
    for c in range(a.shape[1]):
        s[:, c % 64] = s[:, c % 64] + a[:, c] * a[:, c]
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, lanes ^ o]
    return s[:, 0]


def emulate_d2(q, x, shift, mutant=None):
    """(ceil(nq / 16) 16, ceil(nx / 64) 64) squared distances as the kernel forms them: operands zero past the
    extents after the shift subtraction, the inner product in ascending steps of four from zero, (|a|^2 + |b|^2) -
    2 a.b.  Padded rows and columns are there for the mutants that use them."""
    (nq, D), nx = q.shape, x.shape[0]
    sh = np.zeros(D) if shift is None or mutant == "shift_ignored" else shift
    Dp = -(-D // 4) * 4
    a, b = np.zeros((-(-nq // 16) * 16, Dp)), np.zeros((-(-nx // COL_BLOCK) * COL_BLOCK, Dp))
    a[:nq, :D] = q - sh
    b[:nx, :D] = x - sh
    na, nb = _norms(a[:, :D]), _norms(b[:, :D])
    if mutant == "shift_on_padding":                     # 0 - shift in the padded features of the MFMA operands
        a[:nq, D:] = 0.0 - sh[np.arange(D, Dp) % D]
        b[:nx, D:] = 0.0 - sh[np.arange(D, Dp) % D]
    dot = np.zeros((a.shape[0], b.shape[0]))
    for c in range(0, Dp, 4):
        dot = dot + a[:, c:c + 4] @ b[:, c:c + 4].T
    if mutant == "f32_row_map":          # register g of lane group h holds row h + 4 g; taken for row 4 h + g
        w = np.empty_like(dot)
        for r0 in range(0, dot.shape[0], 16):
            for h in range(4):
                for g in range(4):
                    w[r0 + 4 * h + g] = dot[r0 + h + 4 * g]
        dot = w
    return (na[:, None] + nb[None, :]) - 2.0 * dot


def _emulated_candidates(d2, nq, nx, self_offset, mutant):
    cols = d2.shape[1] if mutant == "padded_rows_candidates" else nx
    if mutant == "partial_block_dropped":
        cols = nx // COL_BLOCK * COL_BLOCK if nx % COL_BLOCK else nx
    ok = np.zeros((nq, d2.shape[1]), bool)
    ok[:, :cols] = True
    if self_offset >= 0 and mutant != "self_not_excluded":
        me = self_offset + np.arange(nq)
        if mutant == "self_by_value":
            ok &= d2[:nq] != d2[np.arange(nq), me][:, None]
        else:
            ok[np.arange(nq), me] = False
    return ok


def emulate_knn(q, x, k, shift=None, self_offset=-1, mutant=None):
    nq, nx = q.shape[0], x.shape[0]
    d2 = emulate_d2(q, x, shift, mutant)
    ok = _emulated_candidates(d2, nq, nx, self_offset, mutant)
    d = d2[:nq].copy()
    with np.errstate(invalid="ignore"):
        ok &= ~np.isnan(d)                               # ordinary <: a NaN never enters a list
    d[~ok] = np.inf
    index = np.broadcast_to(np.arange(d.shape[1]), d.shape)
    order = np.lexsort((-index if mutant == "tie_high_index" else index, d), axis=1)
    if mutant == "k_plus_1":
        order = np.concatenate((order[:, :k - 1], order[:, k:k + 1]), axis=1)
    order = order[:, :k]
    vals = np.take_along_axis(d, order, axis=1)
    taken = np.take_along_axis(ok, order, axis=1)
    return np.where(taken, vals, np.inf), np.where(taken, order, -1).astype(np.int32)


def emulate_ball(q, x, r2, shift=None, self_offset=-1, mutant=None):
    nq, nx = q.shape[0], x.shape[0]
    d2 = emulate_d2(q, x, shift, mutant)
    ok = _emulated_candidates(d2, nq, nx, self_offset, mutant)
    rad = np.concatenate((r2, np.full(d2.shape[1] - nx, r2[-1])))[None, :]
    if mutant == "query_radius":
        rad = r2[np.arange(nq) % nx][:, None]
    with np.errstate(invalid="ignore"):
        inside = d2[:nq] < rad if mutant == "ball_strict" else d2[:nq] <= rad
    return (inside & ok).sum(axis=1).astype(np.int32)


class EmulatedBackend:
    def __init__(self, mutant=None):
        self.mutant = mutant

    def knn(self, q, x, k, shift=None, self_offset=-1):
        return emulate_knn(q, x, k, shift, self_offset, self.mutant)

    def ball(self, q, x, r2, shift=None, self_offset=-1):
        return emulate_ball(q, x, r2, shift, self_offset, self.mutant)


# ---------------------------------------------------------------------------------------------------------------
# The check families.  Each returns the worst observed fraction of its tolerance (0 where bit equality is demanded).
# ---------------------------------------------------------------------------------------------------------------
def _bits(v):
    return np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)


def check_case(backend, c, what, shift="case"):
    """knn_smallest and ball_count of a backend on case c against the reference.  shift: what the backend is given
    (the bounds are always those of the case's own shift)."""
    q, x, k, so = c["q"], c["x"], c["k"], c["self_offset"]
    shift = c["shift"] if isinstance(shift, str) else shift
    nq, nx = q.shape[0], x.shape[0]
    d2, idx = backend.knn(q, x, k, shift, so)
    assert d2.shape == (nq, k) and idx.shape == (nq, k) and d2.dtype == np.float64 and idx.dtype == np.int32, \
        f"{what}: outputs {d2.shape} {d2.dtype}, {idx.shape} {idx.dtype}"
    vals, ridx, nxt = ref_smallest(c["ref"], c["cand"], k)
    rb = np.where(c["cand"], c["bound"], 0.0).max(axis=1)[:, None]
    err = np.abs(d2.astype(LD) - vals.astype(LD)).astype(np.float64)
    frac = float((err / rb).max())
    print(f"{what}: worst value error {frac:.3f} of its bound")
    assert (err <= rb).all(), f"{what}: the t-th smallest value is off by up to {frac:.3g} of the row's bound"
    assert (np.diff(d2, axis=1) >= 0).all(), f"{what}: values do not ascend"
    assert ((idx >= 0) & (idx < nx)).all(), f"{what}: an index outside 0 ... {nx - 1}"
    assert np.take_along_axis(c["cand"], idx.astype(np.int64), axis=1).all(), f"{what}: an excluded row was returned"
    assert (np.sort(idx, axis=1)[:, 1:] != np.sort(idx, axis=1)[:, :-1]).all(), f"{what}: a row returned twice"
    # the returned index's own reference distance is the returned value, within that pair's bound
    own = np.abs(d2.astype(LD) - np.take_along_axis(c["ref"], idx.astype(np.int64), axis=1)).astype(np.float64)
    own_bound = np.take_along_axis(c["bound"], idx.astype(np.int64), axis=1)
    assert (own <= own_bound).all(), f"{what}: a returned value is not the distance to the returned index " \
                                     f"({(own / own_bound).max():.3g} of the pair's bound)"
    frac = max(frac, float((own / own_bound).max()))
    gaps = np.diff(np.concatenate((vals, nxt[:, None]), axis=1), axis=1)
    close = gaps <= 2 * rb                                                  # rank t and t + 1 within twice the bound
    excusable = close.copy()
    excusable[:, 1:] |= close[:, :-1]
    wrong = idx != ridx
    assert not (wrong & ~excusable).any(), \
        f"{what}: {(wrong & ~excusable).sum()} indices differ from the reference's where its order is unambiguous"
    assert wrong.sum() <= EXCUSE_CAP * idx.size, f"{what}: {wrong.sum()} of {idx.size} indices excused"
    if c["r2"] is None:
        return frac
    count = backend.ball(q, x, c["r2"], shift, so)
    assert count.shape == (nq,) and count.dtype == np.int32, f"{what}: counts {count.shape} {count.dtype}"
    ref64 = c["ref"].astype(np.float64)
    want = (c["cand"] & (ref64 <= c["r2"][None, :])).sum(axis=1)
    undecided = (c["cand"] & (np.abs(ref64 - c["r2"][None, :]) <= c["bound"])).sum(axis=1)
    assert (np.abs(count - want) <= undecided).all(), \
        f"{what}: counts differ from the reference's at rows {np.flatnonzero(np.abs(count - want) > undecided)[:6]}"
    assert np.abs(count - want).sum() <= EXCUSE_CAP * c["cand"].sum(), f"{what}: too many pairs excused"
    return frac


def family_values(backend, D, nqs=NQS, nxs=NXS, offsets=OFFSETS):
    """Every (nq, nx) at feature count D, with and without the offset of 1000, k = 3: an independent query set, and --
    where nq <= nx -- the queries as x rows with self excluded."""
    worst = 0.0
    for nq in nqs:
        for nx in nxs:
            for off in offsets:
                worst = max(worst, check_case(backend, case(nq, nx, D, off, False), f"nq={nq} nx={nx} D={D} +{off:g}"))
                if nq <= nx:
                    worst = max(worst, check_case(backend, case(nq, nx, D, off, True),
                                                  f"nq={nq} nx={nx} D={D} +{off:g} self"))
    return worst


def family_other_k(backend):
    worst = 0.0
    for k in KS:
        for nq, nx, D in ((17, 65, 33), (65, 257, 17), (2, 9, 5)):
            if nx < k + 2:
                continue
            for own in (False, True):
                worst = max(worst, check_case(backend, case(nq, nx, D, 1000.0, own, k),
                                              f"k={k} nq={nq} nx={nx} D={D} self={own}"))
    return worst


def family_big(backend):
    b = BIG
    return max(check_case(backend, case(b["nq"], b["nx"], b["D"], 0.0, False, b["k"]), "big"),
               check_case(backend, case(b["nq"], b["nx"], b["D"], 1000.0, True, b["k"]), "big +1000 self"))


def family_exact(backend):
    """Integer data: bit equality of values, indices (ties to the lower index) and counts (<=, the x row's radius,
    self excluded by index although duplicates of it sit at distance 0)."""
    for D, nq, nx in ((1, 9, 9), (1, 17, 65), (3, 16, 64), (3, 65, 257), (5, 17, 129), (17, 15, 63), (33, 2, 17),
                      (130, 65, 65)):
        x = rows("int", nx, D, 3)
        shift = np.random.default_rng([4, D]).integers(-2, 3, size=D).astype(np.float64)
        for own in (False, True):
            so = nx - nq if own else -1
            q = x[so:so + nq] if own else rows("int", nq, D, 5)
            d = ((q[:, None, :] - x[None, :, :]) ** 2).sum(axis=2)                  # exact
            cand = candidates(nq, nx, so)
            for k in KS:
                if nx - own < k:
                    continue
                what = f"int D={D} nq={nq} nx={nx} k={k} self={own}"
                vals, ridx, _ = ref_smallest(d, cand, k)
                d2, idx = backend.knn(q, x, k, shift, so)
                assert np.array_equal(_bits(d2), _bits(vals)), f"{what}: values differ on integer data"
                assert np.array_equal(idx, ridx), f"{what}: indices differ from the stable sort's (ties!)"
                own_d = ((x[:, None, :] - x[None, :, :]) ** 2).sum(axis=2)
                np.fill_diagonal(own_d, np.inf)
                r2 = np.sort(own_d, axis=1)[:, min(k, nx - 1) - 1]                 # radii that sit ON distances
                want = (cand & (d <= r2[None, :])).sum(axis=1)
                got = backend.ball(q, x, r2, shift, so)
                assert np.array_equal(got, want), f"{what}: counts differ from the brute-force count"
    return 0.0


def family_properties(backend):
    """Bits: queries split over calls, x reversed, a set's own radii (the symmetry of d2 between the two entries),
    two identical calls."""
    for nx, D, k, off in ((257, 33, 3, 0.0), (129, 130, 5, 1000.0), (65, 5, 1, 0.0)):
        x = rows("gauss", nx, D, 6, off)
        shift = shift_of(x)
        d2, idx = backend.knn(x, x, k, shift, 0)
        again = backend.knn(x, x, k, shift, 0)
        assert np.array_equal(_bits(d2), _bits(again[0])) and np.array_equal(idx, again[1]), "two calls, other bits"
        for cuts in ((0, 1, 70, nx), (0, 64, 65, min(128, nx), nx)):
            parts = [backend.knn(x[lo:hi], x, k, shift, lo) for lo, hi in zip(cuts, cuts[1:]) if hi > lo]
            assert np.array_equal(_bits(np.concatenate([p[0] for p in parts])), _bits(d2)) and \
                np.array_equal(np.concatenate([p[1] for p in parts]), idx), \
                f"nx={nx} D={D}: the queries split at {cuts} give other bits than one call"
        r2 = np.ascontiguousarray(d2[:, k - 1])
        count = backend.ball(x, x, r2, shift, 0)
        assert np.array_equal(count, backend.ball(x, x, r2, shift, 0))
        assert int(count.sum()) == nx * k, \
            f"nx={nx} D={D} k={k}: the own-radius counts sum to {int(count.sum())}, not n k = {nx * k}: d2(i, j) " \
            f"and d2(j, i) differ between the entries"
        parts = [backend.ball(x[lo:hi], x, r2, shift, lo) for lo, hi in ((0, 40), (40, nx))]
        assert np.array_equal(np.concatenate(parts), count)
        q = rows("gauss", 17, D, 7, off)
        fwd = backend.knn(q, x, k, shift, -1)
        rev = backend.knn(q, x[::-1].copy(), k, shift, -1)
        assert np.array_equal(_bits(fwd[0]), _bits(rev[0])), f"nx={nx} D={D}: x reversed gives other value bits"
        assert np.array_equal(nx - 1 - rev[1], fwd[1]), f"nx={nx} D={D}: x reversed gives other neighbours"
        assert np.array_equal(backend.ball(q, x, r2, shift, -1),
                              backend.ball(q, x[::-1].copy(), r2[::-1].copy(), shift, -1))
    return 0.0


def family_nan(backend):
    """A NaN row of x is never a neighbour and never inside a ball; a NaN query row returns +inf / -1 and 0."""
    nx, D, k = 70, 17, 3
    x = rows("gauss", nx, D, 8)
    q = rows("gauss", 18, D, 9)
    shift = shift_of(x)
    clean = backend.knn(q, np.delete(x, 66, axis=0), k, shift, -1)
    r2 = np.full(nx, 1e300)
    xn = x.copy()
    xn[66, 5] = np.nan
    d2, idx = backend.knn(q, xn, k, shift, -1)
    assert not (idx == 66).any() and np.isfinite(d2).all()
    assert np.array_equal(_bits(d2), _bits(clean[0])) and np.array_equal(np.where(idx > 66, idx - 1, idx), clean[1])
    assert np.array_equal(backend.ball(q, xn, r2, shift, -1), np.full(18, nx - 1, np.int32))
    r2n = r2.copy()
    r2n[3] = np.nan                                       # a NaN radius holds nobody either
    assert np.array_equal(backend.ball(q, x, r2n, shift, -1), np.full(18, nx - 1, np.int32))
    qn = q.copy()
    qn[16, 0] = np.nan
    d2, idx = backend.knn(qn, x, k, shift, -1)
    full = backend.knn(q, x, k, shift, -1)
    keep = np.arange(18) != 16
    assert np.isposinf(d2[16]).all() and (idx[16] == -1).all()
    assert np.array_equal(_bits(d2[keep]), _bits(full[0][keep])) and np.array_equal(idx[keep], full[1][keep])
    count = backend.ball(qn, x, r2, shift, -1)
    assert count[16] == 0 and (count[keep] == nx).all()
    return 0.0


def family_shift_matters(backend):
    """Offset data with the shift ignored must miss the bound: what makes the shift's handling testable."""
    for nq, nx, D in ((17, 65, 1), (17, 65, 33), (65, 257, 130)):
        c = case(nq, nx, D, 1000.0, False)
        try:
            check_case(backend, c, f"shift ignored nq={nq} nx={nx} D={D}", shift=None)
        except AssertionError:
            continue
        raise AssertionError(f"nq={nq} nx={nx} D={D}: offset data passed the bound WITHOUT its shift")
    return 0.0
