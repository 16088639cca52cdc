"""qarig_knn_smallest / qarig_ball_count, FeatureBank, manifold_metrics and nearest_real on the GPU against the
longdouble references and derived tolerances of tests/gen_knn_cases.py -- the same check families that
tests/test_gen_knn_host.py shows to reject a wrong row map, a dropped shift, a dropped column block, a wrong tie rule,
... on a NumPy emulation.  Integer inputs bit for bit."""
import numpy as np
import pytest
import torch

import gen_knn_cases as K
from qarig import _lib, gen_eval, ops

pytestmark = pytest.mark.gpu


def _dev(x):
    return None if x is None else torch.from_numpy(np.array(x, order="C")).cuda()       # a copy: cases are read-only


class GpuBackend:
    def knn(self, q, x, k, shift=None, self_offset=-1):
        d2, idx = ops.knn_smallest(_dev(q), _dev(x), k, _dev(shift), self_offset)
        return d2.cpu().numpy(), idx.cpu().numpy()

    def ball(self, q, x, r2, shift=None, self_offset=-1):
        return ops.ball_count(_dev(q), _dev(x), _dev(r2), _dev(shift), self_offset).cpu().numpy()


@pytest.mark.parametrize("dim", K.DIMS)
def test_values_indices_and_counts(dim):
    worst = K.family_values(GpuBackend(), dim)
    print(f"knn_smallest / ball_count D = {dim}: worst fraction of the bound {worst:.3f}")
    assert worst < 1


def test_other_k():
    worst = K.family_other_k(GpuBackend())
    print(f"k in {K.KS}: worst fraction of the bound {worst:.3f}")
    assert worst < 1


def test_the_largest_dim():
    worst = K.family_big(GpuBackend())
    print(f"nq = 70, nx = 1100, D = 1024, k = 5: worst fraction of the bound {worst:.3f}")
    assert worst < 1


def test_integer_data_bit_for_bit():
    K.family_exact(GpuBackend())


def test_split_reversed_symmetric_and_repeatable():
    K.family_properties(GpuBackend())


def test_nan_rows():
    K.family_nan(GpuBackend())


def test_offset_data_without_its_shift_misses_the_bound():
    K.family_shift_matters(GpuBackend())


def test_guard_elements_keep_their_bits():
    """Outputs sit inside larger buffers whose other elements hold distinct NaN payloads / sentinels."""
    lib = _lib.load()
    for nq, nx, D, k, so in ((17, 65, 5, 3, -1), (65, 257, 33, 8, 3), (1, 9, 1, 1, 0)):
        x = _dev(K.rows("gauss", nx, D, 11))
        q = x[so:so + nq] if so >= 0 else _dev(K.rows("gauss", nq, D, 12))
        shift = _dev(K.shift_of(x.cpu().numpy()))
        G = 64
        dpat = (np.uint64(0x7FF8_0000_BEEF_0000) + np.arange(2 * G + nq * k, dtype=np.uint64)).view(np.float64)
        ipat = (-1_000_000 - np.arange(2 * G + nq * k)).astype(np.int32)
        cpat = (-2_000_000 - np.arange(2 * G + nq)).astype(np.int32)
        nb = lib.qarig_knn_workspace_bytes(nq, nx, D, k)
        wpat = np.full(nb + 2 * G, 0xA5, np.uint8)
        d2, idx, cnt, ws = _dev(dpat), _dev(ipat), _dev(cpat), _dev(wpat)
        assert ws.data_ptr() % 16 == 0
        st = lib.qarig_knn_smallest(q.data_ptr(), nq, x.data_ptr(), nx, D, shift.data_ptr(), k, so,
                                    d2.data_ptr() + 8 * G, idx.data_ptr() + 4 * G, ws.data_ptr() + G, nb,
                                    _lib.stream())
        assert st == 0, _lib.last_error()
        want = ops.knn_smallest(q, x, k, shift, so)
        r2 = want[0][:, k - 1].new_full((nx,), 1.0) * float(want[0].max())
        st = lib.qarig_ball_count(q.data_ptr(), nq, x.data_ptr(), nx, D, shift.data_ptr(), r2.data_ptr(), so,
                                  cnt.data_ptr() + 4 * G, ws.data_ptr() + G, nb, _lib.stream())
        assert st == 0, _lib.last_error()
        torch.cuda.synchronize()
        d2h, idxh, cnth, wsh = d2.cpu().numpy(), idx.cpu().numpy(), cnt.cpu().numpy(), ws.cpu().numpy()
        for got, pat in ((d2h.view(np.uint64), dpat.view(np.uint64)), (idxh, ipat), (cnth, cpat), (wsh, wpat)):
            assert np.array_equal(got[:G], pat[:G]) and np.array_equal(got[-G:], pat[-G:]), (nq, nx, D, k)
        assert np.array_equal(d2h[G:-G].view(np.uint64), want[0].cpu().numpy().ravel().view(np.uint64))
        assert np.array_equal(idxh[G:-G], want[1].cpu().numpy().ravel())
        assert np.array_equal(cnth[G:-G], ops.ball_count(q, x, r2, shift, so).cpu().numpy())


def test_refusals_return_the_code_without_launching():
    lib = _lib.load()
    nq, nx, D, k = 16, 64, 32, 3
    x = torch.zeros((nx, D), dtype=torch.float64, device="cuda")
    q = torch.zeros((nq, D), dtype=torch.float64, device="cuda")
    shift = torch.zeros(D, dtype=torch.float64, device="cuda")
    r2 = torch.ones(nx, dtype=torch.float64, device="cuda")
    d2 = torch.full((nq, k), 7.0, dtype=torch.float64, device="cuda")
    idx = torch.full((nq, k), 7, dtype=torch.int32, device="cuda")
    cnt = torch.full((nq,), 7, dtype=torch.int32, device="cuda")
    nb = lib.qarig_knn_workspace_bytes(nq, nx, D, k)
    ws = torch.zeros(nb, dtype=torch.uint8, device="cuda")
    p = lambda t: None if t is None else t.data_ptr()      # noqa: E731

    def knn(nq=nq, nx=nx, D=D, k=k, so=-1, q=q, x=x, shift=shift, d2=d2, idx=idx, ws=ws, nws=nb):
        return lib.qarig_knn_smallest(p(q), nq, p(x), nx, D, p(shift), k, so, p(d2), p(idx), p(ws), nws, _lib.stream())

    def ball(nq=nq, nx=nx, D=D, so=-1, q=q, x=x, shift=shift, r2=r2, cnt=cnt, ws=ws, nws=nb):
        return lib.qarig_ball_count(p(q), nq, p(x), nx, D, p(shift), p(r2), so, p(cnt), p(ws), nws, _lib.stream())

    for fn in (knn, ball):
        for kw in ({"D": 0}, {"D": 1025}, {"nq": 0}, {"nq": 2 ** 20 + 1}, {"nx": 0}, {"nx": 2 ** 20 + 1}, {"so": -2},
                   {"so": nx - nq + 1}, {"q": None}, {"x": None}, {"ws": None}, {"ws": x}, {"ws": shift}):
            assert fn(**kw) == -1, (fn.__name__, kw, _lib.last_error())
        assert fn(nws=nb - 1) == -3 and "workspace" in _lib.last_error()
    for kw in ({"k": 0}, {"k": 9}, {"d2": None}, {"idx": None}, {"d2": x}, {"idx": q}, {"d2": shift},
               {"nq": 1, "nx": 3, "so": 0}):
        assert knn(**kw) == -1, (kw, _lib.last_error())
    for kw in ({"r2": None}, {"cnt": None}, {"cnt": r2}, {"cnt": q}, {"nq": 1, "nx": 1, "so": 0}):
        assert ball(**kw) == -1, (kw, _lib.last_error())
    torch.cuda.synchronize()
    assert (d2 == 7.0).all() and (idx == 7).all() and (cnt == 7).all()
    for bad in (dict(k=0), dict(k=9)):
        with pytest.raises(ValueError):
            ops.knn_smallest(q, x, **bad)
    with pytest.raises(ValueError):
        ops.knn_smallest(q, x[:, :8].contiguous(), 1)
    with pytest.raises(ValueError):
        ops.knn_smallest(q.float(), x, 1)
    with pytest.raises(ValueError):
        ops.knn_smallest(q, x, 1, self_offset=nx - nq + 1)
    with pytest.raises(ValueError):
        ops.ball_count(q, x, r2[:-1])
    with pytest.raises(RuntimeError):
        ops.knn_smallest(q.cpu(), x, 1)
    # a shift may be absent, and sub-views are made contiguous
    wide = torch.randn((nx, 2 * D), dtype=torch.float64, device="cuda")
    a = ops.knn_smallest(wide[:nq, :D], wide[:, :D], 2)
    b = ops.knn_smallest(wide[:nq, :D].contiguous(), wide[:, :D].contiguous(), 2, torch.zeros_like(shift))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# --- the metrics -----------------------------------------------------------------------------------------------
def _metrics(real, gen, k, shift=None):
    return gen_eval.manifold_metrics(_dev(real), _dev(gen), k, _dev(shift))


def test_manifold_metrics_against_brute_force():
    rng = np.random.default_rng(0)
    for n, m, D, k in ((40, 30, 6, 3), (130, 70, 33, 5), (9, 300, 3, 1)):
        real = rng.standard_normal((n, D)) + 0.3
        gen = 1.2 * rng.standard_normal((m, D)) + 0.5
        got = _metrics(real, gen, k, K.shift_of(real))
        want = K.ref_metrics(real, gen, k)
        print(f"n={n} m={m} D={D} k={k}: {got}")
        assert got == want and set(got) == {"precision", "recall", "density", "coverage"}
        assert all(isinstance(v, float) for v in got.values())


def test_manifold_metrics_closed_forms():
    rng = np.random.default_rng(1)
    a = rng.standard_normal((40, 6))
    same = _metrics(a, a.copy(), 3)
    assert same["precision"] == same["recall"] == same["coverage"] == 1.0 and same["density"] > 1.0
    assert _metrics(a, a + 100.0, 3) == {"precision": 0.0, "recall": 0.0, "density": 0.0, "coverage": 0.0}
    two = np.concatenate((a[:20], a[20:] + np.array([100.0, 0, 0, 0, 0, 0])))
    half = _metrics(two, two[:20].copy(), 3, K.shift_of(two))
    assert half["precision"] == 1.0 and half["recall"] == 0.5 and half["coverage"] == 0.5
    with pytest.raises(ValueError):
        _metrics(a[:3], a, 3)


def test_nearest_real_and_quantiles():
    rng = np.random.default_rng(2)
    real, gen = rng.standard_normal((90, 17)), rng.standard_normal((33, 17))
    idx, d2 = gen_eval.nearest_real(_dev(gen), _dev(real), _dev(K.shift_of(real)))
    ref = ((gen[:, None, :] - real[None, :, :]) ** 2).sum(axis=2)
    assert idx.dtype == torch.int32 and np.array_equal(idx.cpu().numpy(), ref.argmin(axis=1))
    assert np.allclose(d2.cpu().numpy(), ref.min(axis=1), rtol=1e-12, atol=0)
    qs = gen_eval.nn_quantiles(d2)
    s = np.sqrt(np.sort(d2.cpu().numpy()))
    assert qs == {"min": s[0], "q01": s[0], "q10": s[3], "q50": s[16]}


def test_feature_bank_in_uneven_batches():
    f = _dev(K.rows("gauss", 50, 9, 13))
    one, many, small = gen_eval.FeatureBank(9, 64), gen_eval.FeatureBank(9, 64), gen_eval.FeatureBank(9, 20)
    one.add(f)
    for lo, hi in ((0, 1), (1, 18), (18, 18), (18, 47), (47, 50)):
        many.add(f[lo:hi])
        small.add(f[lo:hi])
    assert many.count == one.count == 50 and many.dropped == 0 and torch.equal(many.rows(), one.rows())
    assert many.rows().data_ptr() == many._buf.data_ptr() and tuple(many._buf.shape) == (64, 9)
    assert small.count == 20 and small.dropped == 30 and torch.equal(small.rows(), f[:20])
    a = gen_eval.manifold_metrics(one, many, 3)
    assert a["precision"] == a["recall"] == a["coverage"] == 1.0
    with pytest.raises(ValueError):
        one.add(f[:, :8])


def test_scorer_keeps_no_bank_without_knn_and_reports_the_manifold_with_it():
    g = torch.Generator().manual_seed(3)
    real = torch.tanh(torch.randn((24, 4, 8, 8), generator=g)).cuda()
    gen = torch.tanh(torch.randn((10, 4, 8, 8), generator=g)).cuda()
    plain, knn = gen_eval.GenerationScorer(4), gen_eval.GenerationScorer(4, knn=3, knn_max_samples=20)
    for s in (plain, knn):
        s.add(real[:10], "real")
        s.add(real[10:], "real")
        s.add(gen, "generated")
    rp, rk = plain.result(), knn.result()
    assert plain._banks == {} and "manifold" not in rp
    assert {k: v for k, v in rk.items() if k != "manifold"}.keys() == rp.keys()
    assert rk["fd_real_generated"] == rp["fd_real_generated"] and rk["counts"] == rp["counts"]
    m = rk["manifold"]
    assert set(m) == {"k", "counts", "dropped", "real_generated", "real_split", "nn_generated_real", "nn_real_split",
                      "note"}
    assert m["k"] == 3 and m["counts"] == {"real": 20, "real_a": 10, "real_b": 10, "generated": 10}
    assert m["dropped"] == {"real": 4, "real_a": 2, "real_b": 2, "generated": 0}
    fr, fg = knn.features(real).cpu().numpy(), knn.features(gen).cpu().numpy()
    assert m["real_generated"] == K.ref_metrics(fr[:20], fg, 3)
    assert m["real_split"] == K.ref_metrics(fr[0:20:2], fr[1:20:2], 3)
    assert set(m["nn_generated_real"]) == set(m["nn_real_split"]) == {"min", "q01", "q10", "q50"}
    d = np.sqrt(((fg[:, None] - fr[None, :20]) ** 2).sum(axis=2).min(axis=1))
    assert m["nn_generated_real"]["min"] == pytest.approx(d.min(), rel=1e-12)
    assert "depend on k" in m["note"]
    line = gen_eval.summary_line("t", rk)
    assert line.startswith(gen_eval.summary_line("t", rp)) and "precision=" in line and "real_split" in line
    few = gen_eval.GenerationScorer(4, knn=3)
    few.add(real[:6], "real")
    few.add(gen, "generated")
    with pytest.raises(ValueError) as e:
        few.result()
    assert "at least 4 samples" in str(e.value) and "real_a" in str(e.value)
