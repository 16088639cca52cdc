"""CPU half of the SSIM-loss tests: the NumPy reference of tests/ssim_loss_cases.py against torch autograd in fp64,
the mutants that the GPU test's tolerance has to reject on the GPU test's own inputs, and the argument checks of
the new entries, the ops and the training flag, without a device.

Reference against autograd: both are fp64 evaluations of the same sums in two orders, which is what the second
term of the GPU tolerance, 1e-9 mag, is granted for; the same bound is used here.  Measured: <= 1e-15 mag on five
families and 3.7e-11 mag on identical images, where the reference is exactly 0 and autograd's chain through
xx - mx^2 and 1 / (B1 B2) leaves its own rounding (the test prints each figure)."""
import ctypes

import numpy as np
import pytest
import torch

import recon_metric_cases as R
import ssim_loss_cases as S

REF_TOL = S.MAG


@pytest.mark.parametrize("wname,shape", [("gauss11", (2, 2, 19, 23)), ("uniform7", (3, 1, 12, 9)),
                                         ("asym5", (2, 2, 9, 14)), ("one", (2, 3, 5, 6))])
@pytest.mark.parametrize("family", R.FAMILIES)
def test_reference_matches_torch_autograd_in_fp64(family, wname, shape):
    win = S.window(wname)
    x, y = R.make_pair(family, shape, seed=5)
    g = S.g_for(shape[0])
    dx, mag = S.ref_ssim_grad(x, y, win, g)
    xt = torch.from_numpy(x).double().requires_grad_(True)
    s = S.torch_ssim(xt, torch.from_numpy(y).double(), win)
    assert np.abs(s.detach().numpy() - R.ref_ssim(x, y, win)).max() <= 1e-12
    (s * torch.from_numpy(g)).sum().backward()
    auto = xt.grad.numpy()
    worst = float((np.abs(dx - auto) / mag).max())
    print(f"{family} {wname}: reference against autograd {worst:.2e} mag; cancellation |dx| / mag >= "
          f"{float((np.abs(dx) / mag).min()):.1e}")
    assert worst <= REF_TOL
    assert (mag > 0).all() and (np.abs(dx) <= mag * (1 + 1e-12)).all()


def test_tolerance_helper():
    dx = np.array([1.0, -2.0, 0.0, 0.0])
    mag = np.array([10.0, 10.0, 1.0, 0.0])
    assert S.within(dx, dx, mag)
    assert S.within(dx + [2.0 ** -23 + 9e-9, 0, 9e-10, 0], dx, mag)
    assert not S.within(dx + [2.0 ** -23 + 1.1e-8, 0, 0, 0], dx, mag)
    assert not S.within(dx + [0, 0, 1.1e-9, 0], dx, mag)
    assert not S.within(dx + [0, 0, 0, 1e-300], dx, mag)                 # mag 0: exact or nothing
    assert not S.within(np.array([np.nan, -2.0, 0, 0]), dx, mag)


def _rejected(family, cases, **mutant):
    """The worst excess (in units of mag) of the mutant over the cases' inputs: the tolerance rejects it where
    this is above 1e-9."""
    worst = 0.0
    for wname, N, C, H, W in cases:
        x, y, g, dx, mag = S.case(family, wname, N, C, H, W)
        bad, _ = S.ref_ssim_grad(x, y, S.window(wname), g, **mutant)
        worst = max(worst, float(S.excess(bad, dx, mag).max()))
    return worst


MAIN_CASES = [("gauss11", 3, *shape) for shape in S.BWD_SHAPES]


@pytest.mark.parametrize("mutant", ["moments", "maps"])
@pytest.mark.parametrize("family", [f for f in R.FAMILIES if f != "identical"])
def test_fp32_moments_and_fp32_maps_fail_the_gpu_tolerance(family, mutant):
    """Why the maps cost 24 bytes per position: either rounding misses the bound, in every family that can show
    it.  Identical images cannot: x and y have the same moments in any precision, so A1 = B1 and A2 = B2 hold
    exactly, P = 0 and R = -2 Q (a power of two apart, so rounding keeps it), and 2 x Q + y R = 0 term by term."""
    worst = _rejected(family, MAIN_CASES, **{mutant: np.float32})
    print(f"{family}: fp32 {mutant} are off by {worst:.2e} mag, {worst / S.MAG:.0f} times the bound")
    assert worst > S.MAG


# (on identical images every term P + 2 x Q + y R is zero by itself -- each window's score is at its maximum --
#  so no rearrangement of the sum can show there)
@pytest.mark.parametrize("family", [f for f in R.FAMILIES if f != "identical"])
def test_structural_mutants_fail_the_gpu_tolerance(family):
    asym = [S.WINDOW_CASES["asym5"]]
    flipped = _rejected(family, asym, flipped=True)
    dropped = min(_rejected(family, [c], drop_last_row=True) for c in MAIN_CASES + asym)
    per_batch = min(_rejected(family, [c], g_per_batch=True) for c in MAIN_CASES + asym)
    print(f"{family}: flipped window {flipped:.2e}, dropped last row {dropped:.2e}, g per batch {per_batch:.2e} mag")
    assert flipped > S.MAG and dropped > S.MAG and per_batch > S.MAG
    # the symmetric windows cannot tell the two orders apart: that is what the asymmetric case is for
    assert _rejected(family, MAIN_CASES[:2], flipped=True) <= S.MAG


def test_cases_cover_the_kernel_edges():
    for shape in S.BWD_SHAPES:
        assert min(shape[1:]) >= 11
    oh = [(H - 10, W - 10) for _, H, W in S.BWD_SHAPES]
    assert (1, 1) in oh and (16, 17) in oh and (17, 16) in oh            # output tile edge and one past it
    assert any(H == 16 and W == 17 for _, H, W in S.BWD_SHAPES)          # input tile edge and one past it
    assert any(H > 32 and W > 48 for _, H, W in S.BWD_SHAPES)            # several tiles, ragged
    assert S.WINDOW_CASES["gauss15"][3:] == (15, 31) and len(S.window("gauss15")) == 15
    assert abs(S.window("asym5").sum() - 1.0) < 1e-15 and list(S.window("asym5")) != list(S.window("asym5")[::-1])
    g = S.g_for(3)
    assert (g < 0).any() and (g > 0).any() and np.abs(g).max() / np.abs(g).min() >= 1000


def test_new_entries_refuse_bad_arguments_without_a_device():
    """Every call below is refused before any launch (the addresses are made up and never dereferenced)."""
    from qarig import _lib
    h = _lib.load()
    X = 0x7f0000000000
    A, B, MAPS, G, DA, OUT, WS = (X + k * (1 << 32) for k in range(7))
    win = (ctypes.c_double * 15)(*([1.0 / 15] * 15))
    wp = ctypes.cast(win, ctypes.c_void_p)
    big = 1 << 40

    def fwd(N=2, C=3, H=32, W=32, taps=11, ws_bytes=big, **ptrs):
        p = {**dict(a=A, b=B, win=wp, out=OUT, maps=MAPS, ws=WS), **ptrs}
        return h.qarig_ssim_fwd_maps(p["a"], p["b"], N, C, H, W, p["win"], taps, R.C1, R.C2, p["out"], p["maps"],
                                     p["ws"], ws_bytes, None)

    def bwd(N=2, C=3, H=32, W=32, taps=11, **ptrs):
        p = {**dict(a=A, b=B, maps=MAPS, g=G, win=wp, da=DA), **ptrs}
        return h.qarig_ssim_bwd(p["a"], p["b"], p["maps"], p["g"], N, C, H, W, p["win"], taps, p["da"], None)

    for call, names in ((fwd, ("a", "b", "win", "out", "maps", "ws")), (bwd, ("a", "b", "maps", "g", "win", "da"))):
        for taps in (0, 2, 10, 16, 17, -1):
            assert call(taps=taps) == -1 and "taps" in _lib.last_error(), taps
        assert call(H=10, W=32) == -1 and "10 x 32" in _lib.last_error() and "11" in _lib.last_error()
        assert call(H=32, W=7, taps=9) == -1 and "32 x 7" in _lib.last_error()
        for name in names:
            assert call(**{name: None}) == -1 and "null" in _lib.last_error(), name
        for N, C, H, W in ((0, 3, 32, 32), (2, 0, 32, 32), (2 ** 25, 1, 32, 32), (2 ** 20, 2 ** 10, 2 ** 10, 2 ** 10),
                           (2 ** 20, 2 ** 11, 11, 11)):                  # the last: 2^31 workgroups
            assert call(N=N, C=C, H=H, W=W) == -1, (N, C, H, W)
            assert h.qarig_ssim_maps_bytes(N, C, H, W, 11) == 0
        assert call(a=A + 2) == -1 and "aligned" in _lib.last_error()
        assert call(maps=MAPS + 4) == -1 and "aligned" in _lib.last_error()
    assert fwd(ws_bytes=h.qarig_ssim_workspace_bytes(2, 3, 32, 32, 11) - 1) == -1 and "workspace" in _lib.last_error()
    assert fwd(maps=A) == -1 and "alias" in _lib.last_error()
    for name in ("a", "b", "maps", "g"):
        assert bwd(da=dict(a=A, b=B, maps=MAPS, g=G)[name]) == -1 and "alias" in _lib.last_error(), name
    assert bwd(g=G + 4) == -1 and "aligned" in _lib.last_error()
    # the size of the maps: three doubles per valid position; 0 for what the entries refuse
    assert h.qarig_ssim_maps_bytes(2, 3, 32, 32, 11) == 3 * 2 * 3 * 22 * 22 * 8
    assert h.qarig_ssim_maps_bytes(1, 1, 11, 11, 11) == 24 and h.qarig_ssim_maps_bytes(1, 1, 15, 31, 15) == 24 * 17
    assert h.qarig_ssim_maps_bytes(2, 3, 17, 18, 1) == 3 * 2 * 3 * 17 * 18 * 8
    for taps in (0, 2, 16, -1):
        assert h.qarig_ssim_maps_bytes(2, 3, 32, 32, taps) == 0
    assert h.qarig_ssim_maps_bytes(2, 3, 10, 32, 11) == 0
    # 2^20 x (2^11 - 1) planes of one 16 x 16 tile each stay below 2^31 workgroups; of 17 x 11 pixels they do not
    assert h.qarig_ssim_maps_bytes(2 ** 20, 2 ** 11 - 1, 11, 11, 11) == 3 * 2 ** 20 * (2 ** 11 - 1) * 8
    assert h.qarig_ssim_maps_bytes(2 ** 20, 2 ** 11 - 1, 17, 11, 11) == 0
    assert bwd(N=2 ** 20, C=2 ** 11 - 1, H=17, W=11) == -1 and "2^31" in _lib.last_error()


def test_ops_and_loss_refuse_cpu_tensors_and_mismatched_maps():
    from qarig import functional as QF
    from qarig import ops
    x = torch.zeros(2, 1, 12, 12)
    for call in (lambda: ops.ssim_fwd_maps(x, x), lambda: QF.ssim_index(x, x), lambda: QF.ssim_loss(x, x),
                 lambda: QF.ssim_loss(x.requires_grad_(True), x.detach()),
                 lambda: ops.ssim_bwd(x, x, torch.zeros(3, 2, 1, 2, 2, dtype=torch.float64),
                                      torch.zeros(2, dtype=torch.float64))):
        with pytest.raises(RuntimeError, match="MI355X"):
            call()


@pytest.mark.parametrize("text", ["-0.5", "nan", "inf", "-inf", "much"])
def test_training_flag_refuses_bad_weights(text, capsys):
    import train_autoencoder as TA
    base = ["--dataset-path", "d.json", "--config-path", "c.json", "--out-dir", "o"]
    with pytest.raises(SystemExit):
        TA.parse_args(base + ["--ssim-weight", text])
    assert "--ssim-weight" in capsys.readouterr().err


def test_training_flag_defaults_to_off():
    import train_autoencoder as TA
    base = ["--dataset-path", "d.json", "--config-path", "c.json", "--out-dir", "o"]
    assert TA.parse_args(base)["ssim_weight"] == 0.0
    assert TA.parse_args(base + ["--ssim-weight", "0.5"])["ssim_weight"] == 0.5
    assert TA.parse_args(base + ["--ssim-weight", "0"])["ssim_weight"] == 0.0
