"""ops.ssim_fwd_maps, ops.ssim_bwd and QF.ssim_loss on the GPU against the fp64 NumPy reference of
tests/ssim_loss_cases.py (a direct taps x taps scatter; tests/test_ssim_loss_host.py checks it against autograd).

Tolerance, per element (ssim_loss_cases.within): |da - dx_ref| <= 2^-23 |dx_ref| + 1e-9 mag, with mag the sum of
the magnitudes of the terms of dx.  Every test prints its worst |da - dx_ref| / mag before and after the fp32
allowance; measured on an MI355X (profiles/r22_ssim_loss_tests.txt): at most 5.9e-8 mag before it (the fp32 rounding
itself), at most 2.5e-12 mag after it (identical images, where dx_ref is 0), bound 1e-9.  The reference of a case is
computed once and shared."""
import ctypes

import numpy as np
import pytest
import torch

import recon_metric_cases as R
import ssim_loss_cases as S

pytestmark = pytest.mark.gpu


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _kw(wname):
    return {} if wname == "gauss11" else {"window": list(S.window(wname))}


def _grad(x, y, g, **kw):
    from qarig import ops
    a, b = _dev(x), _dev(y)
    _, maps = ops.ssim_fwd_maps(a, b, **kw)
    return ops.ssim_bwd(a, b, maps, _dev(g), **kw).cpu().numpy()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32 if a.dtype == np.float32 else np.int64)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


@pytest.mark.parametrize("shape", R.SSIM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_forward_with_maps_gives_the_bits_of_ssim(shape):
    from qarig import ops
    for N in R.SSIM_BATCHES:
        for k, family in enumerate(R.FAMILIES):
            x, y = R.make_pair(family, (N, *shape), seed=10 + k)
            a, b = _dev(x), _dev(y)
            out, maps = ops.ssim_fwd_maps(a, b)
            C, H, W = shape
            assert out.dtype == maps.dtype == torch.float64 and maps.shape == (3, N, C, H - 10, W - 10)
            assert _same_bits(out.cpu().numpy(), ops.ssim(a, b).cpu().numpy()), (family, N)
            # the maps themselves: the reference's formulas in another order, a few fp64 roundings through 1 / (B1 B2)
            want = np.stack(S.ref_maps(x, y, S.window("gauss11"))[1:])
            got = maps.cpu().numpy()
            assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max(), family
    x, y = R.make_pair("noise", (2, 3, 26, 23), seed=30)
    kw = {"window": list(R.uniform_window(7)), "data_range": 1.0}
    out, maps = ops.ssim_fwd_maps(_dev(x), _dev(y), **kw)
    assert _same_bits(out.cpu().numpy(), ops.ssim(_dev(x), _dev(y), **kw).cpu().numpy()) and maps.shape[3:] == (20, 17)


def _check_case(family, wname, N, C, H, W):
    x, y, g, dx, mag = S.case(family, wname, N, C, H, W)
    da = _grad(x, y, g, **_kw(wname))
    assert da.dtype == np.float32 and da.shape == x.shape
    worst = float(S.excess(da, dx, mag).max())
    raw = float((np.abs(da - dx) / np.where(mag > 0, mag, 1.0)).max())
    print(f"ssim_bwd {family} {wname} {N}x{C}x{H}x{W}: |da - dx| <= {raw:.2e} mag, after the fp32 allowance "
          f"{worst:.2e} mag (bound {S.MAG:.0e}); |dx| / mag >= {float((np.abs(dx) / mag).min()):.1e}")
    assert S.within(da, dx, mag), (family, worst)
    if family == "identical":
        assert (np.abs(da) <= S.MAG * mag).all()
    assert _same_bits(da, _grad(x, y, g, **_kw(wname))), family                   # two runs: equal bits


@pytest.mark.parametrize("N", S.BWD_BATCHES)
@pytest.mark.parametrize("shape", S.BWD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_backward_matches_the_fp64_reference(shape, N):
    for family in R.FAMILIES:
        _check_case(family, "gauss11", N, *shape)


@pytest.mark.parametrize("name", sorted(S.WINDOW_CASES))
def test_backward_with_other_windows(name):
    """7 uniform taps; the asymmetric 5 taps (a flipped window fails here: tests/test_ssim_loss_host.py); one tap;
    15 taps on 15 x 31 pixels, the largest halo over a single row of positions."""
    for family in R.FAMILIES:
        _check_case(family, *S.WINDOW_CASES[name])


def test_gradient_of_an_image_depends_on_that_image_alone():
    x, y = R.make_pair("noise", (5, 3, 43, 59), seed=40)
    g = S.g_for(5)
    whole = _grad(x, y, g)
    assert _same_bits(whole, np.concatenate([_grad(x[:2], y[:2], g[:2]), _grad(x[2:], y[2:], g[2:])]))
    # g[n] = 0: exact zeros for that image, the others unchanged
    g0 = g.copy()
    g0[3] = 0.0
    got = _grad(x, y, g0)
    assert (got[3] == 0).all() and _same_bits(np.delete(got, 3, 0), np.delete(whole, 3, 0))
    # a NaN pixel: that image's gradient is non-finite under the windows that hold the pixel, i.e. within 10
    # pixels of it in its channel; every other image keeps its bits
    xn = x.copy()
    xn[2, 1, 17, 30] = np.nan
    got = _grad(xn, y, g)
    assert _same_bits(np.delete(got, 2, 0), np.delete(whole, 2, 0))
    under = np.zeros((43, 59), bool)
    under[7:28, 20:41] = True            # the positions 7 ... 17 x 20 ... 30 hold the pixel; their windows reach here
    assert np.isnan(got[2, 1][under]).all()
    assert np.isfinite(got[2, 1][~under]).all() and _same_bits(got[2, 1][~under], whole[2, 1][~under])
    assert _same_bits(got[2, 0], whole[2, 0]) and _same_bits(got[2, 2], whole[2, 2])


def test_launches_write_their_outputs_in_full_and_nothing_beside_them():
    from qarig import _lib
    h = _lib.load()
    N, C, H, W = 3, 3, 27, 26
    x, y, g, dx, mag = S.case("noise", "gauss11", N, C, H, W)
    a, b, gd = _dev(x), _dev(y), _dev(g)
    win = (ctypes.c_double * 11)(*S.window("gauss11"))
    wp = ctypes.cast(win, ctypes.c_void_p)
    n_maps = h.qarig_ssim_maps_bytes(N, C, H, W, 11) // 8
    assert n_maps == 3 * N * C * 17 * 16
    guard = 64
    maps = torch.full((n_maps + 2 * guard,), float("nan"), dtype=torch.float64, device="cuda")
    out = torch.full((N + 2,), float("nan"), dtype=torch.float64, device="cuda")
    need = h.qarig_ssim_workspace_bytes(N, C, H, W, 11)
    ws = torch.full((need + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    _lib.check(h.qarig_ssim_fwd_maps(a.data_ptr(), b.data_ptr(), N, C, H, W, wp, 11, R.C1, R.C2, out[1:].data_ptr(),
                                     maps[guard:].data_ptr(), ws.data_ptr(), need, _lib.stream()), "qarig_ssim_fwd_maps")
    got = maps.cpu().numpy()
    assert np.isnan(got[:guard]).all() and np.isnan(got[-guard:]).all() and np.isfinite(got[guard:-guard]).all()
    o = out.cpu().numpy()
    assert np.isnan(o[0]) and np.isnan(o[-1]) and np.abs(o[1:-1] - R.ref_ssim(x, y, S.window("gauss11"))).max() <= R.SSIM_TOL
    assert (ws[need:] == 0x5A).all()
    row = W
    da = torch.full((N * C * H * W + 2 * row,), float("nan"), dtype=torch.float32, device="cuda")
    _lib.check(h.qarig_ssim_bwd(a.data_ptr(), b.data_ptr(), maps[guard:].data_ptr(), gd.data_ptr(), N, C, H, W, wp, 11,
                                da[row:].data_ptr(), _lib.stream()), "qarig_ssim_bwd")
    got = da.cpu().numpy()
    assert np.isnan(got[:row]).all() and np.isnan(got[-row:]).all()
    inner = got[row:-row].reshape(N, C, H, W)
    assert np.isfinite(inner).all() and S.within(inner, dx, mag)
    assert np.isnan(maps[:guard].cpu().numpy()).all()                                # the backward only reads them


def test_ssim_loss_value_and_gradient():
    from qarig import functional as QF
    N, C, H, W = 3, 3, 26, 27
    x, y = R.make_pair("noise", (N, C, H, W), seed=60)
    pred = _dev(x).requires_grad_(True)
    target = _dev(y).requires_grad_(True)
    loss = QF.ssim_loss(pred, target)
    assert loss.dtype == torch.float32 and loss.dim() == 0
    want = 1.0 - float(R.ref_ssim(x, y, S.window("gauss11")).mean())
    assert abs(float(loss.detach()) - want) <= 2.0 ** -23 * want + 1e-10
    loss.backward()
    assert target.grad is None
    dx, mag = S.ref_ssim_grad(x, y, S.window("gauss11"), np.full(N, -1.0 / N))
    worst = float(S.excess(pred.grad.cpu().numpy(), dx, mag).max())
    print(f"ssim_loss gradient: worst excess {worst:.2e} mag")
    assert S.within(pred.grad.cpu().numpy(), dx, mag)
    # per-image weights through ssim_index, other keyword arguments, gradients accumulate into .grad as usual
    pred.grad = None
    g = S.g_for(N)
    idx = QF.ssim_index(pred, target, window=list(S.window("asym5")))
    assert idx.dtype == torch.float64 and idx.shape == (N,)
    assert np.abs(idx.detach().cpu().numpy() - R.ref_ssim(x, y, S.window("asym5"))).max() <= R.SSIM_TOL
    (idx * _dev(g)).sum().backward()
    dx, mag = S.ref_ssim_grad(x, y, S.window("asym5"), g)
    assert S.within(pred.grad.cpu().numpy(), dx, mag)
    with torch.no_grad():
        assert torch.equal(QF.ssim_index(pred, target), QF.ssim_index(pred.detach(), target.detach()))
