"""Shared inputs, NumPy references and tolerances of the generation-evaluation tests (csrc/moments.hip,
qarig/gen_eval.py).  The check families below take a *backend* -- the GPU ops (tests/test_gpu_gen_eval.py) or the NumPy
emulation of the two kernels' definitions in this file (tests/test_gen_eval_host.py, which also feeds them mutants of
that emulation: a family that accepts a wrong kernel proves nothing).

References.  Sums and Gram matrices are computed in np.longdouble where that is wider than fp64 (x86: 64-bit
significand); elsewhere in fp64 with every bound doubled (the reference then carries the same error as the kernel).

Gram tolerance, per element (derived, not tuned).  With a_r = f_r - shift and n_total rows accumulated,
    |got(i,j) - ref(i,j)| <= (n_total + 4) u A(i,j),   u = 2^-53,   A(i,j) = sum_r |a_ri| |a_rj|:
any summation order of n products commits at most (n - 1) roundings, each relative to a partial sum bounded by A;
each product is rounded once (the MFMA fuses it: at most one rounding either way), and each factor carries the rounding
of the shift subtraction (2 u); the remaining u covers second-order terms.  The same argument with one factor gives
    |got_sum(c) - ref_sum(c)| <= (n_total + 2) u S(c),   S(c) = sum_r |a_rc|.

mean / cov tolerance (FeatureMoments: one pass, shifted).  mean = shift + sum / n, cov = (G - s s^T / n) / (n - 1):
    |d mean(c)|  <= (n + 4) u S(c) / n + 2 u |mean(c)|      (the sum's bound, the division, the final addition)
    |d cov(i,j)| <= [ (n + 6) u A(i,j) + (2 n + 8) u S(i) S(j) / n ] / (n - 1).
First term: the Gram bound plus the roundings of the subtraction and of the division by n - 1, both relative to at most
A.  Second term, the one-pass cancellation: s_i s_j / n has the two sums' errors, (n + 2) u S each against a factor
|s| <= S, and the roundings of the product, of the division by n and of the subtraction it enters (relative to at most
S(i) S(j) / n).  With the shift near the data's mean, S(i) S(j) / n is of the size of A(i,j), so nothing is lost
against a two-pass covariance; without a shift it grows with (mean / sigma)^2.

Integer-valued inputs (|value| < 2^10, integer |shift| <= 8): every a, product (< 2^22) and partial sum (< 2^22 n, far
below 2^53 at these n) is exact in fp64, in any order, fused or not -- the tests demand bit equality there.  The
integers are drawn per (row, column), so no two rows or columns agree and a wrong lane map cannot pass."""
import numpy as np

LD = np.longdouble
WIDE = np.finfo(LD).eps < np.finfo(np.float64).eps
SLACK = 1.0 if WIDE else 2.0
U = 2.0 ** -53
TILE = 16

DIMS = (1, 15, 16, 17, 33, 48)
ROWS = (1, 2, 3, 4, 5, 65)
BIG = (5, 1024)                                   # (n, D)
POOL_SHAPES = ((3, 2, 4, 4), (2, 4, 8, 8), (1, 3, 8, 16))
POOLS = (1, 2, 4)
FM_CASE = dict(n=96, D=32, batches=(40, 40, 16))


def features(kind, n, D, seed):
    rng = np.random.default_rng([seed, n, D, 0 if kind == "gauss" else 1])
    if kind == "gauss":
        return rng.standard_normal((n, D)) * 0.7 + 0.3
    return rng.integers(-1023, 1024, size=(n, D)).astype(np.float64)


def shift_for(kind, D, seed):
    rng = np.random.default_rng([seed, D, 7])
    if kind == "gauss":
        return 0.3 + 0.05 * rng.standard_normal(D)
    return rng.integers(-8, 9, size=D).astype(np.float64)


def maintained(D):
    """Mask of the Gram elements moments_add maintains: floor(j / 16) >= floor(i / 16)."""
    t = np.arange(D) // TILE
    return t[None, :] >= t[:, None]


def ref_moments(f, shift=None):
    """(sum, gram) in longdouble and (S, A), the absolute-value sums of the bounds, of all rows of f about shift."""
    a = f.astype(LD) - (0 if shift is None else shift.astype(LD))
    a64 = np.abs(a).astype(np.float64)
    return a.sum(axis=0), a.T @ a, a64.sum(axis=0), a64.T @ a64


def gram_tol(n_total, A):
    return SLACK * (n_total + 4) * U * A


def sum_tol(n_total, S):
    return SLACK * (n_total + 2) * U * S


def ref_mean_cov(f):
    """Two-pass mean and covariance in longdouble."""
    x = f.astype(LD)
    m = x.sum(axis=0) / x.shape[0]
    d = x - m
    return m, d.T @ d / (x.shape[0] - 1)


def mean_cov_tol(f, shift):
    n = f.shape[0]
    _, _, S, A = ref_moments(f, shift)
    m = np.abs(ref_mean_cov(f)[0]).astype(np.float64)
    return (SLACK * ((n + 4) * U * S / n + 2 * U * m),
            SLACK * ((n + 6) * U * A + (2 * n + 8) * U * np.outer(S, S) / n) / (n - 1))


def ref_pool(z, P):
    """(N, D) longdouble block means of (N,C,H,W), and the mean |z| of every block."""
    N, C, H, W = z.shape
    b = z.astype(LD).reshape(N, C, H // P, P, W // P, P)
    return b.mean(axis=(3, 5)).reshape(N, -1), np.abs(b).mean(axis=(3, 5)).reshape(N, -1).astype(np.float64)


def pool_input(kind, shape, seed):
    rng = np.random.default_rng([seed, *shape])
    if kind == "gauss":
        return (rng.standard_normal(shape) * 0.7 + 0.3).astype(np.float32)
    # multiples of 16: their block sums divide by P^2 <= 16 exactly
    return (16 * rng.integers(-63, 64, size=shape)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------
# NumPy emulation of the kernels' definitions, and its mutants
# ---------------------------------------------------------------------------------------------------------------
MUTANTS = ("f32_row_map", "row_col_swapped", "shift_ignored", "shift_on_tail_rows", "lower_tiles_written",
           "partial_tile_dropped", "pool_block_transposed")


def emulate_pool(z, P, mutant=None):
    N, C, H, W = z.shape
    out = np.zeros((N, C, H // P, W // P))
    for y in range(P):                    # raster order inside the block
        for x in range(P):
            out = out + z[:, :, y::P, x::P].astype(np.float64)
    out = out / float(P * P)
    if mutant == "pool_block_transposed":
        out = out.transpose(0, 1, 3, 2)
    return np.ascontiguousarray(out).reshape(N, -1)


def emulate_moments_add(f, shift, state, mutant=None):
    """qarig_moments_add on NumPy arrays state = [count (1,) int64, sum (D,), gram (D,D)], modified in place: the
    operands zero-padded to whole tiles and whole steps of four rows, one 16 x 16 tile at a time over the upper
    triangle of tiles, the rows in ascending steps."""
    count, total, gram = state
    n, D = f.shape
    T = -(-D // TILE)
    sh = np.zeros(D) if shift is None or mutant == "shift_ignored" else shift
    a = np.zeros((-(-n // 4) * 4, T * TILE))
    a[:n, :D] = f - sh
    if mutant == "shift_on_tail_rows":
        a[n:, :D] = 0.0 - sh
    count += n
    for r in range(n):
        total += a[r, :D]
    for ti in range(T):
        for tj in range(T):
            if tj < ti and mutant != "lower_tiles_written":
                continue
            if mutant == "partial_tile_dropped" and (tj + 1) * TILE > D:
                continue
            c = np.zeros((TILE, TILE))
            rows, cols = min(TILE, D - ti * TILE), min(TILE, D - tj * TILE)
            c[:rows, :cols] = gram[ti * TILE:ti * TILE + rows, tj * TILE:tj * TILE + cols]
            for k in range(0, a.shape[0], 4):
                c = c + a[k:k + 4, ti * TILE:(ti + 1) * TILE].T @ a[k:k + 4, tj * TILE:(tj + 1) * TILE]
            if mutant == "row_col_swapped":
                c = c.T.copy()
            if mutant == "f32_row_map":      # register q of lane group h holds row h + 4 q; stored as row 4 h + q
                w = np.empty_like(c)
                for h in range(4):
                    for q in range(4):
                        w[4 * h + q] = c[h + 4 * q]
                c = w
            gram[ti * TILE:ti * TILE + rows, tj * TILE:tj * TILE + cols] = c[:rows, :cols]


class EmulatedBackend:
    def __init__(self, mutant=None):
        self.mutant = mutant

    def moments(self, batches, shift, D, gram_init=None):
        state = [np.zeros(1, np.int64), np.zeros(D), np.zeros((D, D)) if gram_init is None else gram_init.copy()]
        for f in batches:
            emulate_moments_add(f, shift, state, self.mutant)
        return int(state[0][0]), state[1], state[2]

    def pool(self, z, P):
        return emulate_pool(z, P, self.mutant)

    def feature_moments(self, dim, shift):
        from qarig import gen_eval
        backend = self

        class M:
            def __init__(self):
                self.state = [np.zeros(1, np.int64), np.zeros(dim), np.zeros((dim, dim))]

            def add(self, f):
                emulate_moments_add(f, shift, self.state, backend.mutant)

            def result(self):
                mean, cov = gen_eval.moments_to_mean_cov(int(self.state[0][0]), self.state[1],
                                                         gen_eval.mirror_triangle(self.state[2]), shift)
                return {"count": int(self.state[0][0]), "mean": mean, "cov": cov}
        return M()


# ---------------------------------------------------------------------------------------------------------------
# The check families.  Each returns the worst observed fraction of its tolerance (0 where bit equality is demanded).
# ---------------------------------------------------------------------------------------------------------------
def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def check_against_reference(got, batches, shift, kind, what):
    """(count, sum, gram) of a backend against the reference of the concatenated batches, on the maintained set."""
    count, total, gram = got
    f = np.concatenate(batches)
    n, D = f.shape
    rs, rg, S, A = ref_moments(f, shift)
    keep = maintained(D)
    assert count == n, f"{what}: count {count}, expected {n}"
    if kind == "int":
        assert np.array_equal(total, rs.astype(np.float64)), f"{what}: sum differs on integer data"
        bad = np.argwhere(keep & (gram != rg.astype(np.float64)))
        assert bad.size == 0, f"{what}: gram differs on integer data at {bad[:4].tolist()} ({len(bad)} elements)"
        return 0.0
    es = np.abs(total.astype(LD) - rs).astype(np.float64)
    eg = np.abs(gram.astype(LD) - rg).astype(np.float64)
    ts, tg = sum_tol(n, S), gram_tol(n, A)
    assert (es <= ts).all(), f"{what}: sum off by up to {(es / np.maximum(ts, 1e-300)).max():.3g} of its bound"
    assert (eg <= tg)[keep].all(), \
        f"{what}: gram off by up to {(eg / np.maximum(tg, 1e-300))[keep].max():.3g} of its bound"
    return float(max((es / np.maximum(ts, 1e-300)).max(), (eg / np.maximum(tg, 1e-300))[keep].max()))


def family_elements(backend, D, rows=ROWS):
    worst = 0.0
    for n in rows:
        for kind in ("gauss", "int"):
            for with_shift in (False, True):
                f = features(kind, n, D, seed=11)
                shift = shift_for(kind, D, seed=12) if with_shift else None
                got = backend.moments([f], shift, D)
                worst = max(worst, check_against_reference(got, [f], shift, kind,
                                                           f"n={n} D={D} {kind} shift={with_shift}"))
    return worst


def family_accumulate(backend, D=33):
    worst = 0.0
    for kind in ("gauss", "int"):
        f = features(kind, 16, D, seed=21)
        shift = shift_for(kind, D, seed=22)
        parts = [f[:5], f[5:9], f[9:]]
        three = backend.moments(parts, shift, D)
        again = backend.moments(parts, shift, D)
        one = backend.moments([f], shift, D)
        worst = max(worst, check_against_reference(three, parts, shift, kind, f"5+4+7 rows {kind}"),
                    check_against_reference(one, [f], shift, kind, f"16 rows {kind}"))
        keep = maintained(D)
        assert three[0] == again[0] and np.array_equal(_bits(three[1]), _bits(again[1])) and \
            np.array_equal(_bits(three[2])[keep], _bits(again[2])[keep]), f"{kind}: the same calls, other bits"
        if kind == "int":
            assert np.array_equal(three[1], one[1]) and np.array_equal(three[2][keep], one[2][keep])
    return worst


def family_untouched(backend, dims=(33, 48), n=5):
    """Elements outside the maintained set keep their bits -- NaNs with distinct payloads, and finite sentinels (a
    NaN survives an addition with its payload, a finite value does not) -- and the maintained ones start from what
    the accumulator held."""
    for D in dims:
        f = features("int", n, D, seed=31)
        shift = shift_for("int", D, seed=32)
        keep = maintained(D)
        idx = np.arange(D * D, dtype=np.uint64).reshape(D, D)
        nan_pattern = (np.uint64(0x7FF8_0000_DEAD_0000) + idx).view(np.float64)
        sentinel = 12345.0 + idx.astype(np.float64)
        want = ref_moments(f, shift)[1].astype(np.float64)
        for name, fill in (("NaN", nan_pattern), ("finite", sentinel)):
            init = np.where(keep, 0.0, fill)
            count, total, gram = backend.moments([f], shift, D, gram_init=init)
            assert np.array_equal(_bits(gram)[~keep], _bits(fill)[~keep]), \
                f"D={D}: elements outside the maintained set lost their {name} bits"
            assert np.array_equal(gram[keep], want[keep]), f"D={D}: maintained elements differ ({name} fill)"
            assert count == n and np.array_equal(total, ref_moments(f, shift)[0].astype(np.float64))
        # a NaN-filled accumulator stays NaN where it is maintained and bit-identical elsewhere
        count, total, gram = backend.moments([f], shift, D, gram_init=nan_pattern)
        assert np.array_equal(_bits(gram)[~keep], _bits(nan_pattern)[~keep]) and np.isnan(gram[keep]).all()
    return 0.0


def family_pool(backend):
    worst = 0.0
    for shape in POOL_SHAPES:
        for P in POOLS:
            for kind in ("gauss", "int"):
                z = pool_input(kind, shape, seed=41)
                got = backend.pool(z, P)
                ref, mean_abs = ref_pool(z, P)
                assert got.shape == ref.shape and got.dtype == np.float64, (got.shape, got.dtype, ref.shape)
                if kind == "int":
                    assert np.array_equal(got, ref.astype(np.float64)), f"pool {P} of {shape}: integer data differ"
                    continue
                err = np.abs(got.astype(LD) - ref).astype(np.float64)
                tol = SLACK * P * P * U * mean_abs
                assert (err <= tol).all(), f"pool {P} of {shape}: off by {(err / tol).max():.3g} of the bound"
                worst = max(worst, float((err / np.maximum(tol, 1e-300)).max()))
    return worst


def family_feature_moments(backend, to_backend=lambda x: x):
    """FeatureMoments' mean and cov (one pass, shifted, mirrored) against the longdouble two-pass values, on two
    Gaussian sets fed in batches; to_backend turns a NumPy array into what the backend's add() takes."""
    n, D, batches = FM_CASE["n"], FM_CASE["D"], FM_CASE["batches"]
    worst = 0.0
    first = features("gauss", n, D, seed=51)
    shift = first[:batches[0]].mean(axis=0)              # the mean of the first batch, as GenerationScorer takes it
    for seed, scale in ((51, 1.0), (52, 1.7)):
        f = features("gauss", n, D, seed=seed) * scale
        m = backend.feature_moments(D, shift)
        lo = 0
        for b in batches:
            m.add(to_backend(f[lo:lo + b]))
            lo += b
        r = m.result()
        rm, rc = ref_mean_cov(f)
        tm, tc = mean_cov_tol(f, shift)
        em = np.abs(r["mean"].astype(LD) - rm).astype(np.float64)
        ec = np.abs(r["cov"].astype(LD) - rc).astype(np.float64)
        assert r["count"] == n
        assert (em <= tm).all(), f"mean off by {(em / tm).max():.3g} of its bound"
        assert (ec <= tc).all(), f"cov off by {(ec / tc).max():.3g} of its bound"
        assert np.array_equal(r["cov"], r["cov"].T)
        worst = max(worst, float((em / tm).max()), float((ec / tc).max()))
    return worst
