"""CPU half of the generation-evaluation tests: frechet_distance against closed forms, the check families of
tests/gen_eval_cases.py accepting a NumPy emulation of the two kernels' definitions and rejecting seven mutants of it
(so that the GPU tests, which run the same families, can tell a wrong kernel), the one-pass shifted covariance against
the two-pass longdouble one, the C-ABI entries refusing bad arguments without a device, and the command line's
argument handling."""
import numpy as np
import pytest

import gen_eval_cases as G
from qarig import gen_eval
from qarig.gen_eval import frechet_distance

D = 16


def _spd(rng, d=D, scale=1.0):
    b = rng.standard_normal((d, 3 * d))
    return scale * (b @ b.T) / (3 * d)


def _rotation(rng, d=D):
    q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    return q


def _zero_floor(c1, c2):
    """What a zero eigenvalue of c1^1/2 c2 c1^1/2 =: M can cost: perturbed by eps |M| it moves its square root by at
    most sqrt(eps |M|) <= 2^-26 sqrt(|c1| |c2|); D eigenvalues, twice in the trace."""
    return 2 * c1.shape[0] * 2.0 ** -26 * np.sqrt(np.linalg.norm(c1, 2) * np.linalg.norm(c2, 2))


def test_identical_sets_give_zero():
    rng = np.random.default_rng(0)
    c, m = _spd(rng), rng.standard_normal(D)
    r = frechet_distance(m, c, m, c)
    print(f"identical sets: fd = {r['fd']:.3e}, bound {2 * D * 2.0 ** -26 * np.linalg.norm(c, 2):.3e}")
    assert set(r) == {"fd", "mean_term", "cov_term", "clipped"}
    assert r["mean_term"] == 0.0 and abs(r["fd"]) <= 2 * D * 2.0 ** -26 * np.linalg.norm(c, 2)
    assert r["clipped"] <= 0.0


def test_equal_covariances_give_the_squared_mean_distance():
    rng = np.random.default_rng(1)
    c, m, delta = _spd(rng), rng.standard_normal(D), rng.standard_normal(D)
    r = frechet_distance(m, c, m + delta, c)
    want = float((((m + delta) - m) ** 2).sum())
    assert r["mean_term"] == pytest.approx(want, rel=1e-12)
    assert abs(r["cov_term"]) <= _zero_floor(c, c) and r["fd"] == r["mean_term"] + r["cov_term"]


@pytest.mark.parametrize("s1,s2", [(1.0, 2.0), (0.5, 3.0), (2.0, 2.0)])
def test_scaled_identities(s1, s2):
    eye = np.eye(D)
    r = frechet_distance(np.zeros(D), s1 * s1 * eye, np.zeros(D), s2 * s2 * eye)
    assert r["fd"] == pytest.approx(D * (s1 - s2) ** 2, rel=1e-12, abs=1e-13)      # I against 4 I: 16.0
    assert r["clipped"] == 0.0


def test_commuting_covariances():
    rng = np.random.default_rng(2)
    q = _rotation(rng)
    a, b = rng.uniform(0.2, 3.0, D), rng.uniform(0.2, 3.0, D)
    r = frechet_distance(np.zeros(D), (q * a) @ q.T, np.zeros(D), (q * b) @ q.T)
    want = float(((np.sqrt(a) - np.sqrt(b)) ** 2).sum())
    # every eigenvalue is well away from zero: relative accuracy D u cond, far inside 1e-12 of the traces
    assert abs(r["fd"] - want) <= 1e-12 * float(a.sum() + b.sum())


def test_rank_deficient_pair():
    rng = np.random.default_rng(3)
    q = _rotation(rng)
    a = np.concatenate((rng.uniform(0.5, 2.0, 4), np.zeros(D - 4)))
    b = np.concatenate((rng.uniform(0.5, 2.0, 2), np.zeros(2), rng.uniform(0.5, 2.0, 2), np.zeros(D - 6)))
    c1, c2 = (q * a) @ q.T, (q * b) @ q.T
    r = frechet_distance(np.zeros(D), c1, np.zeros(D), c2)
    want = float(((np.sqrt(a) - np.sqrt(b)) ** 2).sum())
    assert abs(r["fd"] - want) <= _zero_floor(c1, c2)
    assert -1e-12 <= r["clipped"] <= 0.0
    # the sample covariance of fewer rows than features, against itself
    x = rng.standard_normal((6, D))
    c = np.cov(x, rowvar=False)
    assert abs(frechet_distance(x.mean(0), c, x.mean(0), c)["fd"]) <= 2 * D * 2.0 ** -26 * np.linalg.norm(c, 2)


def test_agreement_with_scipy_sqrtm():
    linalg = pytest.importorskip("scipy.linalg")
    rng = np.random.default_rng(4)
    c1, c2 = _spd(rng), _spd(rng, scale=2.5)
    m1, m2 = rng.standard_normal(D), rng.standard_normal(D)
    root = linalg.sqrtm(c1 @ c2)
    want = float(((m1 - m2) ** 2).sum() + np.trace(c1) + np.trace(c2) - 2.0 * np.trace(root).real)
    assert frechet_distance(m1, c1, m2, c2)["fd"] == pytest.approx(want, rel=1e-10)


def test_frechet_distance_refuses_mismatched_shapes():
    with pytest.raises(ValueError):
        frechet_distance(np.zeros(3), np.eye(3), np.zeros(4), np.eye(4))
    with pytest.raises(ValueError):
        frechet_distance(np.zeros(3), np.eye(4), np.zeros(3), np.eye(4))


def test_mirror_and_moment_arithmetic():
    rng = np.random.default_rng(5)
    x = rng.standard_normal((9, 35))
    full = x.T @ x
    half = np.where(G.maintained(35), full, np.nan)
    assert np.array_equal(gen_eval.mirror_triangle(half), np.where(G.maintained(35), full, full.T))
    shift = rng.standard_normal(35)
    a = x - shift
    mean, cov = gen_eval.moments_to_mean_cov(9, a.sum(0), a.T @ a, shift)
    assert np.abs(mean - x.mean(0)).max() <= 1e-14 and np.abs(cov - np.cov(x, rowvar=False)).max() <= 1e-13
    for n in (0, 1):
        with pytest.raises(ValueError):
            gen_eval.moments_to_mean_cov(n, np.zeros(3), np.zeros((3, 3)))
    with pytest.raises(ValueError):
        gen_eval.FeatureMoments(4).result()
    with pytest.raises(ValueError):
        gen_eval.FeatureMoments(1025)
    assert "not fid" in gen_eval.NOTE.lower()


# --- the families on the emulation and on its mutants ----------------------------------------------------------
@pytest.mark.parametrize("dim", G.DIMS)
def test_families_accept_the_emulation_elements(dim):
    worst = G.family_elements(G.EmulatedBackend(), dim)
    print(f"emulation, D = {dim}: worst fraction of the bound {worst:.3f}")


def test_families_accept_the_emulation_rest():
    e = G.EmulatedBackend()
    n, big = G.BIG
    w = [G.family_elements(e, big, rows=(n,)), G.family_accumulate(e), G.family_untouched(e), G.family_pool(e),
         G.family_feature_moments(e)]
    print("emulation: worst fractions (D = 1024, accumulate, untouched, pool, mean / cov): " +
          ", ".join(f"{v:.3f}" for v in w))


# which family has to catch which mutant (at the smallest shapes that can: the GPU tests run exactly these)
CATCHES = {
    "f32_row_map": lambda b: G.family_elements(b, 16),
    "row_col_swapped": lambda b: G.family_elements(b, 33),
    "shift_ignored": lambda b: G.family_elements(b, 15),
    "shift_on_tail_rows": lambda b: G.family_elements(b, 17, rows=(1, 2, 3, 5, 65)),
    "lower_tiles_written": G.family_untouched,
    "partial_tile_dropped": lambda b: G.family_elements(b, 17),
    "pool_block_transposed": G.family_pool,
}


@pytest.mark.parametrize("mutant", G.MUTANTS)
def test_families_reject_the_mutant(mutant):
    with pytest.raises(AssertionError) as e:
        CATCHES[mutant](G.EmulatedBackend(mutant))
    print(f"{mutant}: {e.value}")


@pytest.mark.parametrize("mutant", ["f32_row_map", "row_col_swapped"])
def test_lane_map_mutants_fail_on_integer_data_alone(mutant):
    """The bit-equality half of the element family is what the issue relies on for the lane map."""
    f = G.features("int", 4, 33, seed=11)
    got = G.EmulatedBackend(mutant).moments([f], None, 33)
    with pytest.raises(AssertionError):
        G.check_against_reference(got, [f], None, "int", mutant)
    G.check_against_reference(G.EmulatedBackend().moments([f], None, 33), [f], None, "int", "unmutated")


def test_one_pass_shifted_covariance_against_two_pass():
    """On the GPU test's own inputs and batches; and the tolerance is not so loose that an unshifted one-pass
    covariance of offset data would pass it."""
    worst = G.family_feature_moments(G.EmulatedBackend())
    print(f"one-pass shifted mean / cov: worst fraction of the derived tolerance {worst:.3f}")
    f = G.features("gauss", 96, 32, seed=51) + 1.0e4
    shift = f[:40].mean(axis=0)
    state = [np.zeros(1, np.int64), np.zeros(32), np.zeros((32, 32))]
    G.emulate_moments_add(f, None, state)
    _, cov = gen_eval.moments_to_mean_cov(96, state[1], gen_eval.mirror_triangle(state[2]))
    err = np.abs(cov.astype(G.LD) - G.ref_mean_cov(f)[1]).astype(np.float64)
    assert (err > G.mean_cov_tol(f, shift)[1]).any()


# --- the C ABI without a device ----------------------------------------------------------------------------------
def test_entries_refuse_bad_arguments_without_a_device():
    """Every call below is refused before any launch (X is a made-up address that is never dereferenced)."""
    from qarig import _lib
    h = _lib.load()
    X = 0x7f0000000000

    def pool(N=2, C=4, H=8, W=8, P=2, null=None):
        a = [X, N, C, H, W, P, X + (1 << 30), None]
        if null is not None:
            a[null] = None
        return h.qarig_pool_features(*a)

    for null in (0, 6):
        assert pool(null=null) == -1 and "null" in _lib.last_error()
    for P in (0, -1, 3, 5, 16):
        assert pool(P=P) == -1 and "pool" in _lib.last_error(), P
    assert pool(H=8, W=12, P=8) == -1                                  # divides H, not W
    assert pool(C=17, P=1) == -1 and "1088" in _lib.last_error() and "1024" in _lib.last_error()
    assert pool(C=1025, H=1, W=1, P=1) == -1
    for N in (0, -3, 2 ** 25):
        assert pool(N=N) == -1, N
    assert pool(C=0) == -1 and pool(H=0) == -1 and pool(W=-8) == -1
    assert h.qarig_pool_features(X, 2, 4, 8, 8, 2, X + 2 * 4 * 8 * 8 * 4 - 8, None) == -1 and "alias" in _lib.last_error()

    def moments(n=8, D=32, f=X, shift=X + (1 << 30), count=X + (2 << 30), total=X + (3 << 30), gram=X + (4 << 30)):
        return h.qarig_moments_add(f, n, D, shift, count, total, gram, None)

    for kw in ({"f": None}, {"count": None}, {"total": None}, {"gram": None}):
        assert moments(**kw) == -1 and "null" in _lib.last_error(), kw
    for D_ in (0, -1, 1025, 2 ** 30):
        assert moments(D=D_) == -1 and "D" in _lib.last_error(), D_
    for n in (0, -1, 2 ** 20 + 1, 2 ** 31 - 1):
        assert moments(n=n) == -1 and "n =" in _lib.last_error(), n
    nbytes = 8 * 32 * 8
    for kw in ({"count": X}, {"total": X + nbytes - 8}, {"gram": X + 8}, {"gram": X - 8}, {"total": X - 8 * 32 + 8}):
        assert moments(**kw) == -1 and "alias" in _lib.last_error(), kw


def test_ops_refuse_cpu_tensors():
    import torch
    from qarig import ops
    with pytest.raises(RuntimeError):
        ops.pool_features(torch.zeros(1, 2, 4, 4), 2)
    state = (torch.zeros(1, dtype=torch.int64), torch.zeros(4, dtype=torch.float64),
             torch.zeros(4, 4, dtype=torch.float64))
    with pytest.raises(RuntimeError):
        ops.moments_add(torch.zeros(3, 4, dtype=torch.float64), state)
    with pytest.raises(RuntimeError):
        gen_eval.FeatureMoments(4).add(torch.zeros(3, 4, dtype=torch.float64))


# --- the command lines -------------------------------------------------------------------------------------------
def test_evaluate_generation_arguments():
    import evaluate_generation as EG
    a = EG.parse_args(["--real-dataset-path", "d.json", "--generated-latents", "g.npy"])
    assert a["device"] == "cpu" and a["space"] == "latent" and a["feature_pool"] == 1 and a["batch_size"] == 64
    assert a["hr_codebook_path"] is None and a["decoder_path"] is None and a["max_batches"] is None
    assert a["out_json"] is None
    a = EG.parse_args(["--device", "cuda", "--real-dataset-path", "d.json", "--generated-latents", "g.npy",
                       "--hr-codebook-path", "hr.pt", "--decoder-path", "dec.pt", "--space", "image",
                       "--feature-pool", "4", "--batch-size", "8", "--max-batches", "3", "--out-json", "o/r.json"])
    assert (a["space"], a["feature_pool"], a["batch_size"], a["max_batches"]) == ("image", 4, 8, 3)
    for bad in (["--generated-latents", "g.npy"], ["--real-dataset-path", "d.json"],
                ["--real-dataset-path", "d.json", "--generated-latents", "g.npy", "--space", "image"],
                ["--real-dataset-path", "d.json", "--generated-latents", "g.npy", "--feature-pool", "0"]):
        with pytest.raises(SystemExit):
            EG.parse_args(bad)
    assert EG.feature_dim((4, 8, 8), 4) == 16 and EG.feature_dim((4, 16, 16), 1) == 1024
    with pytest.raises(SystemExit) as e:
        EG.feature_dim((4, 32, 32), 1)
    assert "--feature-pool" in str(e.value) and "4,096" in str(e.value)
    with pytest.raises(SystemExit):
        EG.feature_dim((4, 8, 8), 3)
    assert "single-process" in EG.__doc__.lower() and "not fid" in EG.__doc__.lower()


def test_generate_images_knows_save_latents():
    import generate_images as gi
    base = ["--decoder-path", "d.pt", "--config-path", "c.json", "--out-dir", "out"]
    assert "save_latents" not in gi.parse_args(base)              # absent unless given: older parses are unchanged
    assert str(gi.parse_args(base + ["--save-latents", "z/l.npy"])["save_latents"]) == "z/l.npy"
