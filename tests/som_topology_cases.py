"""Host restatement of the top-2 search and its reductions (qarig_bmu_top2 / qarig_topology_rows /
qarig_code_lag_profile, include/qarig.h), the input families of the topology tests and the mutants those
families must tell from the definition.  Test infrastructure only.

fp32 fma.  `fma32` forms the product in float64 (exact: 24 + 24 bits), adds the accumulator in float64 and rounds
to float32.  The float64 sum is itself rounded, so the result is rounded twice: where the float64 sum lands exactly
half way between two float32 values although the exact sum lies to one side, rounding it again breaks the tie to
even instead of towards the exact sum (about one operation in 2^29 on random data).  fma32 repairs exactly that
case from the TwoSum residual of the float64 add, so it is the correctly rounded fma on every finite input; the
integer-valued families never come near it, every product and sum there being an exact small integer.
"""
import math

import numpy as np

F32, F64 = np.float32, np.float64

MUTANTS = ("second_by_t", "ties_to_higher", "second_may_equal_first", "second_above_first_only",
           "gap_without_abs", "ratio_bin_fp32", "no_clamp")


def fma32(a, b, c):
    """Correctly rounded fp32 a * b + c of float32 arrays (see the module docstring)."""
    p = a.astype(F64) * b.astype(F64)
    c64 = c.astype(F64)
    s = p + c64
    bb = s - p
    err = (p - (s - bb)) + (c64 - bb)                 # exact sum = s + err
    r = s.astype(F32)
    r64 = r.astype(F64)
    with np.errstate(over="ignore", invalid="ignore"):
        up = np.nextafter(r, F32(np.inf)).astype(F64)
        dn = np.nextafter(r, F32(-np.inf)).astype(F64)
        tie_up = (s == (r64 + up) / 2) & (err != 0)   # s half way between r and the float above it
        tie_dn = (s == (r64 + dn) / 2) & (err != 0)
        r = np.where(tie_up & (err > 0), up.astype(F32), r)
        r = np.where(tie_dn & (err < 0), dn.astype(F32), r)
    return r


def patch_rows(x, patch):
    """(N,C,H,W) -> (N * gh * gw, C * pH * pW), patchify's order (channel, row, column; the grid truncates)."""
    N, C, H, W = x.shape
    pH, pW = patch
    gh, gw = H // pH, W // pW
    v = x[:, :, :gh * pH, :gw * pW].reshape(N, C, gh, pH, gw, pW)
    return np.ascontiguousarray(v.transpose(0, 2, 4, 1, 3, 5).reshape(N * gh * gw, C * pH * pW))


def rows_image(rows, N, C, H, W, patch, fill=0.0):
    """Inverse of patch_rows for an (N,C,H,W) latent; positions outside the patch grid get `fill`."""
    pH, pW = patch
    gh, gw = H // pH, W // pW
    x = np.full((N, C, H, W), fill, dtype=F32)
    v = rows.reshape(N, gh, gw, C, pH, pW).transpose(0, 3, 1, 4, 2, 5).reshape(N, C, gh * pH, gw * pW)
    x[:, :, :gh * pH, :gw * pW] = v
    return x


def distances(rows, w, clamp=True):
    """(d, t) fp32 (R,K) of the literal definition: w2 / x2 by ascending fma chains, acc the ascending chain of
    -2 w[k][e] x[r][e], t = acc + w2, d = sqrtf(max(t + x2, 0))."""
    rows, w = rows.astype(F32), w.astype(F32)
    R, D = rows.shape
    K = w.shape[0]
    w2 = np.zeros(K, F32)
    x2 = np.zeros(R, F32)
    for e in range(D):
        w2 = fma32(w[:, e], w[:, e], w2)
        x2 = fma32(rows[:, e], rows[:, e], x2)
    m2 = (F32(-2.0) * w).astype(F32)
    acc = np.zeros((R, K), F32)
    for e in range(D):
        acc = fma32(np.broadcast_to(m2[None, :, e], (R, K)), np.broadcast_to(rows[:, e, None], (R, K)), acc)
    t = (acc + w2[None, :]).astype(F32)
    s = (t + x2[:, None]).astype(F32)
    with np.errstate(invalid="ignore"):
        d = np.sqrt(np.maximum(s, F32(0.0)) if clamp else s).astype(F32)
    return d, t, s


def emulate_top2(x, w, patch, mutant=None):
    """(idx1, idx2, d1, d2) of the definition: candidates in (d, k) order, the minimum and the minimum over
    k != idx1.  `mutant` names one of the wrong readings in MUTANTS (those of the search)."""
    rows = patch_rows(np.asarray(x, F32), patch)
    d, t, _ = distances(rows, np.asarray(w, F32), clamp=mutant != "no_clamp")
    R, K = d.shape
    ar = np.arange(R)
    key = np.where(np.isnan(d), F32(np.inf), d)
    if mutant == "ties_to_higher":
        order = (K - 1 - np.argsort(key[:, ::-1], axis=1, kind="stable"))[:, :2]
    else:
        order = np.argsort(key, axis=1, kind="stable")[:, :2]
    i1, i2 = order[:, 0].copy(), order[:, 1].copy()
    if mutant == "second_by_t":
        tt = t.copy()
        tt[ar, i1] = np.inf
        i2 = np.argmin(tt, axis=1)
    elif mutant == "second_may_equal_first":
        i2 = i1.copy()
    elif mutant == "second_above_first_only":
        dd = key.copy()
        dd[np.arange(K)[None, :] <= i1[:, None]] = np.inf
        i2 = np.where(i1 == K - 1, i2, np.argmin(dd, axis=1))
    return i1.astype(np.int64), i2.astype(np.int64), d[ar, i1], d[ar, i2]


def emulate_rows(i1, i2, d1, d2, K, mutant=None):
    """(gap_hist [K], ratio_hist [32]) of qarig_topology_rows; mutants: gap_without_abs (negative gaps are lost),
    ratio_bin_fp32."""
    gap = (i1 - i2) if mutant == "gap_without_abs" else np.abs(i1 - i2)
    gap_hist = np.bincount(gap[(gap >= 0) & (gap < K)], minlength=K).astype(np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        if mutant == "ratio_bin_fp32":
            q = ((F32(32.0) * d1.astype(F32)) / d2.astype(F32)).astype(F64)
        else:
            q = 32.0 * d1.astype(F64) / d2.astype(F64)
    q = np.where(np.isnan(q), 32.0, q)
    bins = np.minimum(31, np.floor(np.minimum(q, 32.0))).astype(np.int64)
    return gap_hist, np.bincount(bins, minlength=32).astype(np.int64)


def ratio_traps(count=8):
    """(d1, d2) fp32 pairs with d1 < d2 whose bin differs between the fp64 quotient and the fp32 one: the fp32
    division rounds 32 d1 / d2 up to an integer that the quotient stays below.  Found by a fixed search."""
    rng = np.random.default_rng(1234)
    d1s, d2s = [], []
    while len(d1s) < count:
        d2 = rng.uniform(0.5, 4.0, 4096).astype(F32)
        j = rng.integers(1, 31, 4096)
        d1 = np.nextafter((j.astype(F64) * d2.astype(F64) / 32.0).astype(F32), F32(0.0))
        q64 = np.floor(32.0 * d1.astype(F64) / d2.astype(F64))
        q32 = np.floor(((F32(32.0) * d1) / d2).astype(F64))
        for a, b in zip(d1[q64 != q32], d2[q64 != q32]):
            d1s.append(a)
            d2s.append(b)
    return np.array(d1s[:count], F32), np.array(d2s[:count], F32)


def lag_profile(w):
    """longdouble [K]: [r] = sum_t |w_t - w_{t+r}|, summed directly."""
    w = np.asarray(w, F32).astype(np.longdouble)
    K = w.shape[0]
    out = np.zeros(K, np.longdouble)
    for r in range(1, K):
        diff = w[:K - r] - w[r:]
        out[r] = np.sqrt((diff * diff).sum(axis=1)).sum()
    return out


# ---------------------------------------------------------------------------------------------------- shapes
def search_plan(K, D):
    """The code ranges the search kernel stages together (csrc/bmu.hip bmu_top2_launch): K <= 1,024 codes resident
    in LDS where they fit 160 KB, else chunks of 512 / 256 / 128 codes; D > 64 reads the codebook from memory."""
    S = (D + 3) // 4 * 4
    if D > 64 or (K <= 1024 and 4096 + K * (S + 1) * 4 <= 160 * 1024):
        return K
    return 512 if S <= 16 else 256 if S <= 36 else 128


def edge_positions(K, D):
    """Codes on either side of everything the kernel splits the code axis by: the ends, every chunk boundary."""
    chunk = search_plan(K, D)
    pos = {0, K - 1}
    for b in range(chunk, K, chunk):
        pos.update((b - 1, b))
    return sorted(pos)


# (K, C, pH, pW, N, H, W): every K, D and row count the GPU tests name; rows = N (H // pH) (W // pW).
SHAPES = [
    (2, 4, 1, 1, 1, 7, 9),          # D 4, 63 rows
    (3, 3, 2, 2, 1, 16, 16),        # D 12, 64 rows
    (33, 4, 2, 2, 1, 2, 254),       # D 16, 127 rows
    (512, 4, 2, 2, 2, 16, 16),      # 128 rows
    (513, 4, 3, 3, 1, 9, 129),      # D 36, 129 rows
    (513, 4, 1, 1, 3, 1, 43),       # D 4, 129 rows in three images
    (1024, 4, 3, 3, 1, 9, 63),      # the largest resident image (152 KB of codes), 63 rows
    (1024, 4, 2, 2, 1, 6, 86),      # D 16 resident, 129 rows
    (1025, 4, 1, 1, 1, 1, 1),       # one row
    (1025, 4, 2, 2, 1, 2, 254),     # D 16 in chunks of 512, 127 rows
    (1025, 4, 3, 3, 2, 3, 96),      # D 36 in chunks of 256, 64 rows
    (2049, 2, 2, 3, 2, 5, 96),      # pH != pW, D 12, the grid truncates H, 128 rows
    (33, 8, 3, 3, 1, 9, 63),        # D 72: the any-D form
]


def shape_id(s):
    K, C, pH, pW, N, H, W = s
    return f"K{K}-D{C * pH * pW}-p{pH}x{pW}-R{N * (H // pH) * (W // pW)}"


def _case(shape, rows, w):
    K, C, pH, pW, N, H, W = shape
    # (what the patch grid leaves out of the latent is filled with a value no search may read)
    return {"x": rows_image(rows.astype(F32), N, C, H, W, (pH, pW), fill=777.0), "w": np.ascontiguousarray(w, F32),
            "patch": (pH, pW), "images": N}


def _dims(shape):
    K, C, pH, pW, N, H, W = shape
    return K, C * pH * pW, N * (H // pH) * (W // pW)


FAMILIES = ("gaussian", "integer", "duplicates", "rows_equal_code", "near_ties", "edges", "offset")


def make_case(family, shape, seed=0):
    """One input of a family at a shape: {"x" (N,C,H,W), "w" (K,D), "patch", "images"}."""
    K, D, R = _dims(shape)
    rng = np.random.default_rng(1000 * FAMILIES.index(family) + seed)
    if family == "gaussian":
        return _case(shape, rng.standard_normal((R, D)), rng.standard_normal((K, D)))
    if family == "integer":                                   # |v| <= 8: every chain exact, ties everywhere
        return _case(shape, rng.integers(-8, 9, (R, D)), rng.integers(-8, 9, (K, D)))
    if family == "duplicates":                                # (0, K-1), (5, 6), a triple (8, 9, 11)
        w = rng.standard_normal((K, D)).astype(F32)
        groups = [(0, K - 1)] + ([(5, 6)] if K > 6 else []) + ([(8, 9, 11)] if K > 11 else [])
        for g in groups:
            for k in g[1:]:
                w[k] = w[g[0]]
        rows = rng.standard_normal((R, D)).astype(F32)
        for r in range(R):                                    # most rows sit beside a duplicated code
            if r % 4:
                rows[r] = w[groups[r % len(groups)][0]] + F32(0.01) * rows[r]
        return _case(shape, rows, w)
    if family == "rows_equal_code":
        w = rng.standard_normal((K, D)).astype(F32)
        return _case(shape, w[(7 * np.arange(R) + 3) % K], w)
    if family == "near_ties":
        # Zero rows: acc = 0, so t = |w|^2 and d = sqrtf(|w|^2).  Code A = (1.25, 0, ...) has |w|^2 = 1.5625;
        # code B = (1.25, 3.45e-4, 0, ...) has the next float above it, and sqrtf maps both to 1.25.  B sits at the
        # lower index (code 0, A at K - 1): by (d, k) it comes before A, by t after it.  A third code Z =
        # (0, ..., 0, 0.5) is the best of the zero rows (d = 0.5), so A and B compete for second there.  The other
        # half of the rows is (0, ..., 0, -8): still orthogonal to A and B, so t = |w|^2 again, and the add of
        # |x|^2 = 64 swallows the one-ulp difference; Z is farther (8.5), so A and B compete for first.  Every
        # other code lies around (4, ..., 4), far from both kinds of row.
        assert D >= 4
        w = (F32(4.0) + rng.standard_normal((K, D))).astype(F32)
        a = np.zeros(D, F32)
        a[0] = 1.25
        b = a.copy()
        b[1] = F32(3.45e-4)
        w[0], w[K - 1] = b, a
        rows = np.zeros((R, D), F32)
        rows[(R + 1) // 2:, D - 1] = F32(-8.0)
        if K > 2:
            pos = edge_positions(K, D)
            mid = pos[len(pos) // 2] if len(pos) > 2 else 1
            w[mid] = 0.0
            w[mid][D - 1] = F32(0.5)
        return _case(shape, rows, w)
    if family == "edges":
        # pairs of codes a hair apart at the ends of the code axis and across every chunk boundary; rows at a
        # quarter and three quarters of the way, so each of the pair is the best once and the second once
        w = rng.standard_normal((K, D)).astype(F32)
        pos = edge_positions(K, D)
        pairs = [(pos[0], pos[-1])] + [(p, p + 1) for p in pos[1:-1:2] if p + 1 in pos]
        used, live = set(), []
        for a, b in pairs:
            if a in used and b in used:
                continue
            if b in used:
                a, b = b, a
            delta = np.zeros(D, F32)
            delta[len(live) % D] = F32(2.0 ** -5)
            w[b] = w[a] + delta
            used.update((a, b))
            live.append((a, b))
        rows = rng.standard_normal((R, D)).astype(F32)
        for r in range(R):
            a, b = live[(r // 2) % len(live)]
            rows[r] = w[a] + (F32(0.25) if r % 2 == 0 else F32(0.75)) * (w[b] - w[a])
        return _case(shape, rows, w)
    if family == "offset":
        # mean 100, spread 1: |x|^2 ~ 10^4 D swamps the distances, so neighbouring t collapse in the add and the
        # sum goes negative for rows next to a code (every third row), where the clamp has to hold
        w = (F32(100.0) + rng.standard_normal((K, D))).astype(F32)
        rows = (F32(100.0) + rng.standard_normal((R, D))).astype(F32)
        near = np.arange(R) % 3 == 0
        rows[near] = w[(5 * np.arange(R) + 1) % K][near] + (F32(2.0 ** -10) * rng.standard_normal((R, D))[near]).astype(F32)
        return _case(shape, rows, w)
    raise KeyError(family)


def line_codebook(K, D, v=3):
    """w_t = t v e_0-ish: integer codes on a line through the origin, direction (v, 0, ..., 0)."""
    w = np.zeros((K, D), F32)
    w[:, 0] = np.arange(K, dtype=F32) * F32(v)
    return w


def line_lag_half(K):
    """lag_half of a line codebook, by hand: the mean distance at lag r is r |v|, the mean over all pairs
    |v| (K + 1) / 3, so the first r with r >= (K + 1) / 6."""
    return max(1, math.ceil((K + 1) / 6))
