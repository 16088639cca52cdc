"""qarig_bmu_top2, qarig_topology_rows and qarig_code_lag_profile on the GPU against their host restatement
(tests/som_topology_cases.py), at the smallest shapes that reach every path of the search kernel: the resident and
the chunked form, each register width (D <= 4, 16, 64, any), one row, 63 ... 129 rows, several images."""
import math

import numpy as np
import pytest
import torch

import som_topology_cases as T

pytestmark = pytest.mark.gpu

PAD = 64
U = 2.0 ** -53
WORST = {}       # worst |error| / bound per check so far (printed by the tests that measure it)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _top2_guarded(x, w, patch):
    """qarig_bmu_top2 through the C ABI into buffers filled with -1 / NaN and followed by PAD guard elements each:
    every output element must be overwritten and no guard element touched.  Returns the four outputs (NumPy)."""
    from qarig import _lib
    N, C, H, W = x.shape
    K, D = w.shape
    rows = N * (H // patch[0]) * (W // patch[1])
    idx = torch.full((2, rows + PAD), -1, dtype=torch.int64, device="cuda")
    d = torch.full((2, rows + PAD), float("nan"), dtype=torch.float32, device="cuda")
    xd, wd = _dev(x), _dev(w)
    _lib.check(_lib.load().qarig_bmu_top2(xd.data_ptr(), N, C, H, W, patch[0], patch[1], wd.data_ptr(), K, D,
                                          idx[0].data_ptr(), idx[1].data_ptr(), d[0].data_ptr(), d[1].data_ptr(),
                                          _lib.stream()), "qarig_bmu_top2")
    idx, d = idx.cpu().numpy(), d.cpu().numpy()
    assert (idx[:, rows:] == -1).all() and np.isnan(d[:, rows:]).all(), "guard band written"
    assert (idx[:, :rows] >= 0).all() and (idx[:, :rows] < K).all() and not np.isnan(d[:, :rows]).any(), \
        "an output element was not written"
    return idx[0, :rows], idx[1, :rows], d[0, :rows], d[1, :rows]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("shape", T.SHAPES, ids=T.shape_id)
@pytest.mark.parametrize("family", T.FAMILIES)
def test_top2_is_the_definition_bit_for_bit(family, shape):
    from qarig import ops
    c = T.make_case(family, shape)
    want = T.emulate_top2(c["x"], c["w"], c["patch"])
    got = _top2_guarded(c["x"], c["w"], c["patch"])
    K = c["w"].shape[0]
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.array_equal(_bits(got[2]), _bits(want[2])) and np.array_equal(_bits(got[3]), _bits(want[3]))
    first = ops.bmu(_dev(c["x"]), _dev(c["w"]), c["patch"]).cpu().numpy()
    assert np.array_equal(first, got[0]), "idx1 differs from ops.bmu"
    # what follows from the order, on every input
    assert (got[0] != got[1]).all() and (got[2] <= got[3]).all()
    tie = got[2] == got[3]
    assert (got[1][tie] > got[0][tie]).all()
    if family == "rows_equal_code":
        assert (got[2] == 0).all()
    if family == "duplicates":
        assert tie.sum() >= len(tie) // 2
    rows = len(got[0])
    if family == "near_ties":            # B (code 0) and A (code K - 1) take the places they compete for
        assert 0 in got[1 if K > 2 else 0] and (rows == 1 or K - 1 in got[1])
    if family == "edges" and rows >= 4 * len(T.edge_positions(*c["w"].shape)):
        for p in T.edge_positions(*c["w"].shape):
            assert p in got[0] and p in got[1], f"code {p} is never the best / the second"


def test_wrapper_returns_the_same_and_refuses_what_the_abi_refuses():
    from qarig import ops
    c = T.make_case("gaussian", T.SHAPES[2])
    want = _top2_guarded(c["x"], c["w"], c["patch"])
    x, w = _dev(c["x"]), _dev(c["w"])
    got = ops.bmu_top2(x, w, c["patch"])
    assert got[0].dtype == got[1].dtype == torch.int64 and got[2].dtype == got[3].dtype == torch.float32
    for g, v in zip(got, want):
        assert np.array_equal(g.cpu().numpy().view(np.uint32 if v.dtype == np.float32 else np.int64),
                              v.view(np.uint32 if v.dtype == np.float32 else np.int64))
    # a non-contiguous latent is searched as its contiguous copy (as ops.bmu does)
    xt = x.transpose(2, 3).contiguous().transpose(2, 3)
    assert not xt.is_contiguous() and torch.equal(ops.bmu_top2(xt, w, c["patch"])[1], got[1])
    with pytest.raises(RuntimeError, match="2 <= K"):
        ops.bmu_top2(x, w[:1], c["patch"])
    with pytest.raises(RuntimeError, match="2 <= K"):
        ops.bmu_top2(x, torch.zeros(16385, 16, device="cuda"), c["patch"])
    with pytest.raises(RuntimeError, match="codebook width"):
        ops.bmu_top2(x, w[:, :12].contiguous(), c["patch"])
    with pytest.raises(RuntimeError):
        ops.bmu_top2(x.cpu(), w, c["patch"])
    i1, i2, d1, d2 = got
    gap, ratio = torch.zeros(33, dtype=torch.int64, device="cuda"), torch.zeros(32, dtype=torch.int64, device="cuda")
    both = torch.stack([i1, i2], 1)
    with pytest.raises(ValueError, match="contiguous"):
        ops.topology_rows(both[:, 0], i2, d1, d2, 1, gap, ratio)
    with pytest.raises(ValueError, match="contiguous"):
        ops.topology_rows(i1, i2, d1, d2.double(), 1, gap, ratio)
    with pytest.raises(ValueError, match="images"):
        ops.topology_rows(i1, i2, d1, d2, 2, gap, ratio)             # 127 rows are not two images
    with pytest.raises(ValueError):
        ops.topology_rows(i1, i2, d1, d2, 1, gap, ratio[:16])
    with pytest.raises(RuntimeError, match="2 <= K"):
        ops.code_lag_profile(w[:1])
    assert int(gap.sum()) == 0 and int(ratio.sum()) == 0            # nothing was launched by the refused calls


def test_batch_of_images_does_not_change_a_row_or_an_image():
    """The same four images as four N = 1 calls and as one N = 4 call: 33 rows per image, so the images start at
    different lanes of different workgroups in the batched call."""
    from qarig import ops
    rng = np.random.default_rng(5)
    K, patch = 513, (2, 2)
    w = _dev(rng.standard_normal((K, 16)).astype(np.float32))
    x = _dev(rng.standard_normal((4, 4, 6, 22)).astype(np.float32))
    hist = lambda: (torch.zeros(K, dtype=torch.int64, device="cuda"),      # noqa: E731
                    torch.zeros(32, dtype=torch.int64, device="cuda"))
    ga, ra = hist()
    whole = ops.bmu_top2(x, w, patch)
    sums = ops.topology_rows(*whole, 4, ga, ra)
    gb, rb = hist()
    for n in range(4):
        one = ops.bmu_top2(x[n:n + 1], w, patch)
        for a, b in zip(one, whole):
            assert torch.equal(a.view(torch.int32), b[33 * n:33 * n + 33].view(torch.int32))
        s = ops.topology_rows(*one, 1, gb, rb)
        assert torch.equal(s.view(torch.int64), sums[n:n + 1].view(torch.int64))
    assert torch.equal(ga, gb) and torch.equal(ra, rb) and int(ga.sum()) == 132 and int(ga[0]) == 0


def _rows_check(name, i1, i2, d1, d2, images, K, exact=()):
    """ops.topology_rows on given rows against np.bincount of the restatement's integers and math.fsum of the fp32
    values; `exact` names the sums (0: d1, 1: d2, 2: d1^2) that must be bit-equal."""
    from qarig import ops
    rows = len(i1)
    seq = rows // images
    gap = torch.zeros(K + PAD, dtype=torch.int64, device="cuda")
    ratio = torch.zeros(32 + PAD, dtype=torch.int64, device="cuda")
    sums = torch.full((images + 1, 3), float("nan"), dtype=torch.float64, device="cuda")
    gap[:K] += 2                      # the histograms are added to, not written
    ops.topology_rows(_dev(i1), _dev(i2), _dev(d1), _dev(d2), images, gap[:K], ratio[:32], sums[:images])
    gh, rh = T.emulate_rows(i1, i2, d1, d2, K)
    assert np.array_equal(gap[:K].cpu().numpy() - 2, gh) and np.array_equal(ratio[:32].cpu().numpy(), rh)
    assert int(gap[K:].sum()) == 0 and int(ratio[32:].sum()) == 0 and bool(sums[images:].isnan().all())
    got = sums[:images].cpu().numpy()
    n_ops = math.ceil(seq / 256) + 8
    for n in range(images):
        a, b = d1[n * seq:(n + 1) * seq].astype(np.float64), d2[n * seq:(n + 1) * seq].astype(np.float64)
        for j, terms in enumerate((a, b, a * a)):
            ref = math.fsum(terms)
            bound = n_ops * U / (1 - n_ops * U) * ref + 2.0 ** -1074
            err = abs(got[n, j] - ref)
            WORST[f"topology_rows sum {j}"] = max(WORST.get(f"topology_rows sum {j}", 0.0), err / bound)
            assert err <= bound, (name, n, j, err, bound)
            if j in exact:
                assert got[n, j] == ref, (name, n, j)
    ops.check_index_flag(torch.device("cuda", 0), name)
    print(f"{name}: worst |error| / bound so far", {k: round(v, 3) for k, v in WORST.items() if k.startswith("topology")})
    return gh, rh


@pytest.mark.parametrize("family", T.FAMILIES)
def test_topology_rows_counts_exactly_and_sums_within_the_derived_bound(family):
    """Histograms: exactly np.bincount of the restatement's integers.  Sums: against math.fsum of the fp32 values.
    Bound, from the operation count: thread t adds rows t, t + 256, ... of the image (ceil(seq / 256) - 1 rounded
    additions after the first), the butterfly adds 6 more, the four waves 3 more: no term passes through more than
    n = ceil(seq / 256) + 8 rounded additions, all terms are non-negative, the squares d1 * d1 are exact in fp64, so
    |error| <= n u / (1 - n u) * sum|term| with u = 2^-53.  The worst ratio seen is printed.
    Integer family: d1 and d2 are fp32 square roots of integers below 2^13 with at least 2^-23 of resolution, so
    their fp64 sums are exact in any order and must be bit-equal; the squares of those roots carry 48 bits each and
    their sum need not be exact -- the bit-equal check of all three sums is made where every distance is a small
    dyadic number (test_line_codebook_has_no_topographic_error)."""
    shape = T.SHAPES[5] if family != "near_ties" else T.SHAPES[4]       # three images of 43 rows / one of 129
    c = T.make_case(family, shape)
    want = T.emulate_top2(c["x"], c["w"], c["patch"])
    _rows_check(family, *want, c["images"], c["w"].shape[0], exact=(0, 1) if family == "integer" else ())


def test_topology_rows_ratio_bins_and_long_images():
    i = np.arange(8, dtype=np.int64)
    d1, d2 = T.ratio_traps()
    _, rh = _rows_check("traps", i, i + 1, d1, d2, 1, 64)
    _, bad = T.emulate_rows(i, i + 1, d1, d2, 64, mutant="ratio_bin_fp32")
    assert not np.array_equal(rh, bad)
    # d2 == 0 (then d1 == 0), d1 == d2, d1 == 0 < d2
    _, rh = _rows_check("zeros", i[:4], i[:4] + 3, np.array([0, 0, 1.5, 0], np.float32),
                        np.array([0, 0, 1.5, 2], np.float32), 2, 64)
    assert rh[31] == 3 and rh[0] == 1
    # more rows than threads: 2 images of 700 rows, gaps on both sides
    rng = np.random.default_rng(3)
    i1 = rng.integers(0, 64, 1400)
    i2 = (i1 + rng.integers(1, 64, 1400)) % 64
    d2 = rng.uniform(0.5, 3.0, 1400).astype(np.float32)
    d1 = (d2 * rng.uniform(0, 1, 1400).astype(np.float32)).astype(np.float32)
    _rows_check("long", i1, i2, d1, d2, 2, 64)
    # gaps on both sides of the 8,192 bins a workgroup counts in LDS before it adds them to memory
    i1 = rng.integers(0, 16384, 1400)
    i2 = (i1 + rng.integers(1, 16384, 1400)) % 16384
    i1[:4], i2[:4] = [0, 8192, 16383, 8191], [8191, 0, 0, 16383]
    gh, _ = _rows_check("wide", i1, i2, d1, d2, 2, 16384)
    assert gh[8191] >= 1 and gh[8192] >= 2 and gh[16383] >= 1


def test_out_of_range_indices_are_flagged_not_counted():
    from qarig import ops
    i1 = torch.tensor([0, 5, -1, 2], device="cuda")
    i2 = torch.tensor([1, 9, 0, 3], device="cuda")
    d = torch.ones(4, device="cuda")
    gap, ratio = torch.zeros(8, dtype=torch.int64, device="cuda"), torch.zeros(32, dtype=torch.int64, device="cuda")
    ops.topology_rows(i1, i2, d, d, 1, gap, ratio)
    assert gap.tolist() == [0, 2, 0, 0, 0, 0, 0, 0]
    with pytest.raises(IndexError):
        ops.check_index_flag(torch.device("cuda", 0), "test")


@pytest.mark.parametrize("K", [2, 3, 64, 513])
@pytest.mark.parametrize("D", [4, 12, 36])
def test_code_lag_profile_within_the_derived_bound(K, D):
    """Against a NumPy longdouble direct sum.  Bound per lag r, from the operations: a distance takes D
    differences (one rounding each, so (1 + u)^2 on its square), D fma (one rounding each on the partial sum of
    non-negative terms) and a square root (one rounding; it halves the relative error of its argument): at most
    (D + 2) / 2 + 1 = D / 2 + 2 roundings' worth.  The sum over the lag's K - r distances: thread t adds pairs t,
    t + 256, ... then the butterfly (6) and the four waves (3): at most ceil((K - r) / 256) + 8 rounded additions
    per term.  So |error| <= (D / 2 + 10 + ceil((K - r) / 256)) u lag_sum[r], u = 2^-53, first order; the
    reference's own error, (D + K) 2^-64 relative, is added."""
    from qarig import ops
    rng = np.random.default_rng(K * 100 + D)
    w = rng.standard_normal((K, D)).astype(np.float32)
    out = torch.full((K + PAD,), float("nan"), dtype=torch.float64, device="cuda")
    got = ops.code_lag_profile(_dev(w)).cpu().numpy()
    ref = T.lag_profile(w)
    assert got.shape == (K,) and got[0] == 0.0
    for r in range(1, K):
        n = D / 2 + 10 + math.ceil((K - r) / 256)
        bound = float(ref[r]) * (n * U * (1 + 64 * U) + (D + K) * 2.0 ** -64)
        err = abs(float(np.longdouble(got[r]) - ref[r]))
        WORST["code_lag_profile"] = max(WORST.get("code_lag_profile", 0.0), err / bound)
        assert err <= bound, (r, err, bound)
    print(f"K {K} D {D}: worst |error| / bound so far {WORST['code_lag_profile']:.3f}")
    # through the ABI: slot 0 and the guard band stay as they were
    from qarig import _lib
    wd = _dev(w)
    _lib.check(_lib.load().qarig_code_lag_profile(wd.data_ptr(), K, D, out.data_ptr(), _lib.stream()), "lag")
    o = out.cpu().numpy()
    assert np.isnan(o[0]) and np.isnan(o[K:]).all() and np.array_equal(o[1:K], got[1:])
    # codes on a line, w_t = t e_0: every distance an exact integer, lag_sum[r] = (K - r) r bit for bit
    line = ops.code_lag_profile(_dev(T.line_codebook(K, D, v=1))).cpu().numpy()
    assert np.array_equal(line, np.array([(K - r) * r for r in range(K)], np.float64))


SECOND_MEAN = (63 * 2.25 + 3.75) / 64


def _line_scorer(perm):
    """64 codes on a line (w_t = 3 t e_0) stored in the order `perm`, two latents of 64 one-pixel patches at
    t + 1/4 along the line: the best unit is the code at t, the second the one at t + 1 (at t - 1 for the last)."""
    from models.Codebook import Codebook
    from qarig.topology import TopologyScorer
    K = 64
    w = T.line_codebook(K, 4, v=3)
    cb = Codebook(patch_dim=(1, 1), image_dim=(8, 8), image_channel=4, num_embeddings=K)
    with torch.no_grad():
        cb.codebook.weight.copy_(torch.from_numpy(w[perm]))
    rows = np.zeros((2 * K, 4), np.float32)
    rows[:, 0] = 3.0 * (np.tile(np.arange(K), 2) + 0.25)
    z = _dev(T.rows_image(rows, 2, 4, 8, 8, (1, 1)))
    s = TopologyScorer({"line": cb.cuda()})
    s.add_batch(z[:1])
    s.add_batch(z[1:])
    return s.result()["line"]


def test_line_codebook_has_no_topographic_error():
    K = 64
    b = _line_scorer(np.arange(K))
    assert b["rows"] == 2 * K and b["topographic_error"] == 0.0 and b["within"][1] == 1.0 and b["mean_gap"] == 1.0
    assert b["median_gap"] == 1 and b["lag"]["lag_half"] == T.line_lag_half(K) == 11
    assert b["lag"]["mean_distance"] == {r: 3.0 * r for r in range(1, K)}
    assert b["lag"]["all_pairs_mean"] == 3.0 * (K + 1) / 3
    # every distance is dyadic (0.75 to the best, 2.25 to the second, 3.75 for the last code, whose second lies
    # behind it): all three sums are exact in any order, so they are bit-equal
    assert b["quantisation_error"] == 0.75 and b["second_error"] == SECOND_MEAN and b["quantisation_mse"] == 0.5625
    assert b["per_image_quantisation_error"] == [0.75, 0.75]
    # 32 * 0.75 / 2.25 = 10.67, 32 * 0.75 / 3.75 = 6.4
    assert b["ratio_hist"][10] == 2 * (K - 1) and b["ratio_hist"][6] == 2 and sum(b["ratio_hist"]) == 2 * K


def test_permuted_line_codebook_shows_in_the_gap_histogram():
    """The same codes in a scrambled order: the latent geometry -- distances, the lag-free all-pairs mean -- is
    what it was, the index gaps are those of the permutation, computed here on the host."""
    K = 64
    perm = np.random.default_rng(11).permutation(K)          # code j holds line position perm[j]
    inv = np.argsort(perm)                                   # line position t is code inv[t]
    t = np.arange(K)
    second = np.where(t == K - 1, K - 2, t + 1)
    gaps = np.abs(inv[t] - inv[second])
    hist = np.bincount(gaps, minlength=K) * 2
    b = _line_scorer(perm)
    from qarig.topology import topology_block
    want = topology_block(hist.tolist(), b["ratio_hist"], [[0.75 * K, SECOND_MEAN * K, 0.5625 * K]] * 2, 2 * K)
    for key in ("topographic_error", "within", "mean_gap", "median_gap"):
        assert b[key] == want[key], key
    assert b["topographic_error"] == 1.0 - int(hist[1]) / (2 * K) and b["topographic_error"] > 0.9
    assert b["quantisation_error"] == 0.75 and b["second_error"] == SECOND_MEAN
    assert b["lag"]["all_pairs_mean"] == pytest.approx(3.0 * (K + 1) / 3, rel=1e-14)


def test_recon_scorer_adds_the_block_only_on_request():
    import test_gpu_recon_eval as G
    from qarig import recon_eval
    from qarig.topology import TopologyScorer
    torch.manual_seed(0)
    dec = G._decoder().cuda()
    cbs = {"lr": G._codebook(8, 8).cuda(), "hr": G._codebook(2, 16).cuda()}
    z = torch.from_numpy(G._latents(6, 1)).cuda()
    plain, topo = recon_eval.ReconScorer(dec, cbs), recon_eval.ReconScorer(dec, cbs, topology=True)
    alone = TopologyScorer(cbs)
    for i in range(0, 6, 4):
        plain.add_batch(z[i:i + 4])
        topo.add_batch(z[i:i + 4])
    for i in range(0, 6, 1):
        alone.add_batch(z[i:i + 1])
    p, t, a = plain.result(), topo.result(), alone.result()
    for name in cbs:
        assert set(p["codebooks"][name]) == {"latent", "vs_decoder", "usage"}
        assert set(t["codebooks"][name]) == {"latent", "vs_decoder", "usage", "topology"}
        for key in ("latent", "vs_decoder", "usage"):
            assert p["codebooks"][name][key] == t["codebooks"][name][key]
        assert t["codebooks"][name]["topology"] == a[name]                 # batch 4 + 2 against batch 1: bit-equal
        assert "per_image_quantisation_error" not in recon_eval.without_per_image(t["codebooks"][name])["topology"]
    assert a["hr"]["rows"] == 6 * 16 and a["lr"]["rows"] == 6 and len(a["hr"]["lag"]["mean_distance"]) == 15
