"""ops.ssim and ops.pair_error on the GPU against the fp64 NumPy references of tests/recon_metric_cases.py.

SSIM tolerance, per image: |delta| <= 1e-10.  Each window moment carries about 22 fp64 roundings of terms <= 1,
about 2.4e-15 absolute; divided by denominators >= c2 = 3.6e-3 that is below 7e-13, and two fp64 orderings of the
reference differ by <= 3.4e-13 on the CPU (tests/test_recon_metrics_host.py prints it).  1e-10 leaves two orders
of magnitude and still rejects window moments kept in fp32 (same file: off by 1e-7 ... 1e-4).

pair_error: the two sums are sums of E non-negative terms, each rounded once, so any summation order is within
E 2^-52 relative of the exact sum; the maximum is exact."""
import ctypes

import numpy as np
import pytest
import torch

import recon_metric_cases as R

pytestmark = pytest.mark.gpu

WIN = R.gaussian_window()


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _ssim(x, y, **kw):
    from qarig import ops
    return ops.ssim(_dev(x), _dev(y), **kw).cpu().numpy()


def _pair(x, y):
    from qarig import ops
    return ops.pair_error(_dev(x), _dev(y)).cpu().numpy()


def _same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.int64), np.asarray(b).view(np.int64))


@pytest.mark.parametrize("N", R.SSIM_BATCHES)
@pytest.mark.parametrize("shape", R.SSIM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_ssim_matches_the_fp64_reference(shape, N):
    for k, family in enumerate(R.FAMILIES):
        x, y = R.make_pair(family, (N, *shape), seed=10 + k)
        got, want = _ssim(x, y), R.ref_ssim(x, y, WIN)
        err = float(np.abs(got - want).max())
        print(f"ssim {family} {N}x{shape}: |delta| {err:.2e}, scores {want.min():.6f} ... {want.max():.6f}")
        assert got.dtype == np.float64 and got.shape == (N,)
        assert err <= R.SSIM_TOL, (family, err)
        assert _same_bits(got, _ssim(x, y)), family                    # two runs: equal bits
        if family == "anticorrelated":
            assert (got < 0).all()
        if family == "identical":
            assert np.abs(got - 1.0).max() <= R.SSIM_TOL


@pytest.mark.parametrize("shape", R.SSIM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_ssim_sees_one_changed_pixel_wherever_it_is(shape):
    """One image per position, changed in that pixel alone.  Under the Gaussian a corner pixel weighs 1e-6 in one
    output of thousands, below the tolerance; under 7 uniform taps it weighs 1/49, and dropping it shows."""
    C, H, W = shape
    for win, kw in ((WIN, {}), (R.uniform_window(7), {"window": list(R.uniform_window(7))})):
        spots = R.one_pixel_positions(H, W, len(win))
        x, _ = R.make_pair("identical", (1, C, H, W), seed=21)
        x = np.repeat(x, len(spots), axis=0)
        y = x.copy()
        for n, (r, c) in enumerate(spots):
            y[n, C - 1, r, c] += -1.0 if y[n, C - 1, r, c] > 0 else 1.0
        got, want = _ssim(x, y, **kw), R.ref_ssim(x, y, win)
        assert np.abs(got - want).max() <= R.SSIM_TOL
        if kw:
            assert (want < 1.0 - 1e-7).all() and (got < 1.0 - 1e-7).all(), (spots, want)


def test_ssim_uniform_window_of_seven_taps():
    N, C, H, W, taps = R.SSIM_UNIFORM_CASE
    u = R.uniform_window(taps)
    for k, family in enumerate(R.FAMILIES):
        x, y = R.make_pair(family, (N, C, H, W), seed=30 + k)
        got = _ssim(x, y, window=list(u))
        assert np.abs(got - R.ref_ssim(x, y, u)).max() <= R.SSIM_TOL, family
    # the Gaussian of other sizes, and another data range: the constants follow
    x, y = R.make_pair("noise", (2, 3, 20, 21), seed=36)
    for taps, sigma in ((1, 1.5), (3, 0.8), (15, 2.0)):
        got = _ssim(x, y, taps=taps, sigma=sigma, data_range=1.0)
        want = R.ref_ssim(x, y, R.gaussian_window(taps, sigma), c1=0.01 ** 2, c2=0.03 ** 2)
        assert np.abs(got - want).max() <= R.SSIM_TOL, taps


def test_ssim_of_an_image_does_not_depend_on_its_batch():
    x, y = R.make_pair("noise", (5, 3, 43, 59), seed=40)
    whole = _ssim(x, y)
    assert _same_bits(whole, np.concatenate([_ssim(x[:2], y[:2]), _ssim(x[2:], y[2:])]))
    assert _same_bits(whole, np.concatenate([_ssim(x[n:n + 1], y[n:n + 1]) for n in range(5)]))
    for bad in (np.nan, np.inf):
        xn = x.copy()
        xn[2, 1, 17, 30] = bad
        got = _ssim(xn, y)
        assert np.isnan(got[2]) and _same_bits(np.delete(got, 2), np.delete(whole, 2))


def test_ssim_refuses_images_smaller_than_the_window():
    x = np.zeros((1, 1, 10, 40), np.float32)
    with pytest.raises(RuntimeError, match="10 x 40"):
        _ssim(x, x)


def _raw_ssim(a, b, out_ptr, ws):
    from qarig import _lib
    N, C, H, W = a.shape
    win = (ctypes.c_double * 11)(*WIN)
    _lib.check(_lib.load().qarig_ssim(a.data_ptr(), b.data_ptr(), N, C, H, W, ctypes.cast(win, ctypes.c_void_p), 11,
                                      R.C1, R.C2, out_ptr, ws.data_ptr(), ws.numel(), _lib.stream()), "qarig_ssim")


def _raw_pair(a, b, out_ptr, ws):
    from qarig import _lib
    N, E = a.shape
    _lib.check(_lib.load().qarig_pair_error(a.data_ptr(), b.data_ptr(), N, E, out_ptr, ws.data_ptr(), ws.numel(),
                                            _lib.stream()), "qarig_pair_error")


def test_launches_write_their_outputs_in_full_and_nothing_beside_them():
    from qarig import _lib
    h = _lib.load()
    N = 3
    x, y = R.make_pair("noise", (N, 3, 27, 26), seed=50)
    a, b = _dev(x), _dev(y)
    out = torch.full((N + 2,), float("nan"), dtype=torch.float64, device="cuda")
    need = h.qarig_ssim_workspace_bytes(N, 3, 27, 26, 11)
    ws = torch.full((need + 64,), 0x5A, dtype=torch.uint8, device="cuda")      # exactly sized, then a guard
    _raw_ssim(a, b, out[1:].data_ptr(), ws[:need])
    got = out.cpu().numpy()
    assert np.isnan(got[0]) and np.isnan(got[-1]) and np.abs(got[1:-1] - R.ref_ssim(x, y, WIN)).max() <= R.SSIM_TOL
    assert (ws[need:] == 0x5A).all()
    E = R.PE_CHUNK + 5
    x, y = R.make_pair("noise", (N, E), seed=51)
    a, b = _dev(x), _dev(y)
    out = torch.full((N + 2, 3), float("nan"), dtype=torch.float64, device="cuda")
    need = h.qarig_pair_error_workspace_bytes(N, E)
    ws = torch.full((need + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    _raw_pair(a, b, out[1:].data_ptr(), ws[:need])
    got = out.cpu().numpy()
    assert np.isnan(got[0]).all() and np.isnan(got[-1]).all() and R.pair_error_close(got[1:-1], R.ref_pair_error(x, y), E)
    assert (ws[need:] == 0x5A).all()


@pytest.mark.parametrize("E", R.PAIR_SIZES)
def test_pair_error_matches_the_fp64_reference(E):
    from qarig import ops
    for N in R.PAIR_BATCHES:
        x, y = R.make_pair("noise", (N, E), seed=60 + N)
        y[N - 1, E - 1] = x[N - 1, E - 1] - 1.5 if x[N - 1, E - 1] > 0 else x[N - 1, E - 1] + 1.5    # the last element
        want = R.ref_pair_error(x, y)
        got = _pair(x, y)
        assert got.dtype == np.float64 and got.shape == (N, 3)
        assert R.pair_error_close(got, want, E), (N, got, want)
        assert _same_bits(got, _pair(x, y))                             # two runs: equal bits
        # base pointers offset by one float (4-byte aligned only): the same values in the same order
        bufs = [torch.empty(N * E + 1, dtype=torch.float32, device="cuda") for _ in range(2)]
        for buf, v in zip(bufs, (x, y)):
            buf[1:].copy_(_dev(v).flatten())
        a, b = (buf[1:].view(N, E) for buf in bufs)
        assert a.data_ptr() % 16 == 4 and a.is_contiguous()
        assert _same_bits(ops.pair_error(a, b).cpu().numpy(), got)
        assert _same_bits(ops.pair_error(a, _dev(y)).cpu().numpy(), got)       # one side aligned, one not
    # identical images: exact zeros; a single differing element, at each end
    x, _ = R.make_pair("identical", (2, E), seed=70)
    assert (_pair(x, x) == 0).all()
    y = x.copy()
    y[0, 0] += 0.5
    y[1, E - 1] -= 0.5
    got = _pair(x, y)
    assert R.pair_error_close(got, R.ref_pair_error(x, y), E) and (got[:, 2] > 0.49).all()


def test_pair_error_of_an_image_does_not_depend_on_its_batch():
    E = 2 * R.PE_CHUNK + 3                   # odd: the images of a batch start at different alignments
    x, y = R.make_pair("noise", (5, E), seed=80)
    whole = _pair(x, y)
    assert R.pair_error_close(whole, R.ref_pair_error(x, y), E)
    assert _same_bits(whole, np.concatenate([_pair(x[:2], y[:2]), _pair(x[2:], y[2:])]))
    for bad in (np.nan, np.inf, -np.inf):
        xn = x.copy()
        xn[3, R.PE_CHUNK + 1] = bad
        got = _pair(xn, y)
        assert _same_bits(np.delete(got, 3, axis=0), np.delete(whole, 3, axis=0))
        if bad != bad:
            assert np.isnan(got[3]).all()
        else:
            assert (got[3] == np.inf).all()
    # images as (N,C,H,W): E is the product of the other axes
    x4, y4 = R.make_pair("noise", (2, 3, 7, 9), seed=81)
    assert R.pair_error_close(_pair(x4, y4), R.ref_pair_error(x4, y4), 3 * 7 * 9)


def test_batches_of_more_than_2_31_elements():
    """The last image of a batch lies past element 2^31 of its tensor: its values must be its own.  Both operands
    are views of ONE buffer of 11.5 GB (the least that holds an fp32 batch past 2^31 elements plus the shift
    between the views), handed back to the device when the test ends.  A few set elements, then constant planes:
    the expected numbers are closed forms (tests/test_recon_metrics_host.py pins the reference to them)."""
    from qarig import ops
    H = W = 26800
    P = H * W                                                              # 3 P > 2^31
    buf = torch.zeros(4 * P, dtype=torch.float32, device="cuda")
    try:
        # pair_error: b is a shifted by 4 elements, b[i] = buf[i + 4]; two images of E elements, 2 E > 2^31
        E = 2 ** 30 + 8
        a, b = buf[:2 * E].view(2, E), buf[4:2 * E + 4].view(2, E)
        buf[E] = 1.0              # a[1][0], and b[0][E - 4]
        buf[2 * E - 1] = 0.5      # a[1][E - 1], and b[1][E - 5]
        buf[2 * E + 3] = 0.25     # b[1][E - 1] alone
        got = ops.pair_error(a, b).cpu().numpy()
        assert np.array_equal(got, [[1, 1, 1], [1 + 0.0625 + 0.25, 1 + 0.25 + 0.5, 1]]), got
        # ssim: b is a shifted by one plane, b[n] = plane n + 1; three images of one channel, 3 P > 2^31
        planes = buf.view(4, 1, H, W)
        for n, v in enumerate((0.25, -0.5, 0.25, 0.25)):
            planes[n].fill_(v)
        got = ops.ssim(planes[:3], planes[1:]).cpu().numpy()
        other = (2 * 0.25 * -0.5 + R.C1) / (0.25 ** 2 + 0.5 ** 2 + R.C1)
        assert np.abs(got - [other, other, 1.0]).max() <= R.SSIM_TOL, got
    finally:
        del buf
        a = b = planes = None
        torch.cuda.empty_cache()


def test_ops_refuse_cpu_tensors():
    from qarig import ops
    x = torch.zeros(1, 1, 11, 11)
    with pytest.raises(RuntimeError):
        ops.ssim(x, x.cuda())
    with pytest.raises(RuntimeError):
        ops.pair_error(x.cuda(), x)
