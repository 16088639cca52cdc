"""CPU half of the reconstruction-metric tests: the fp64 references of tests/recon_metric_cases.py against a
second ordering and against closed forms, an fp32-moment mutant rejected by the GPU test's own tolerance and
inputs, the host arithmetic of qarig/recon_eval.py on hand-made numbers, evaluate_reconstruction.py's argument
parsing, and the new C-ABI entries refusing bad arguments without a device."""
import ctypes
import math

import numpy as np
import pytest

import recon_metric_cases as R

WIN = R.gaussian_window()


@pytest.mark.parametrize("family", R.FAMILIES)
def test_direct_window_sum_agrees_with_a_separable_evaluation(family):
    worst = 0.0
    for shape in R.SSIM_SHAPES:
        x, y = R.make_pair(family, (2, *shape), seed=3)
        worst = max(worst, float(np.abs(R.ref_ssim(x, y, WIN) - R.ref_ssim_separable(x, y, WIN)).max()))
    N, C, H, W, taps = R.SSIM_UNIFORM_CASE
    x, y = R.make_pair(family, (N, C, H, W), seed=4)
    u = R.uniform_window(taps)
    worst = max(worst, float(np.abs(R.ref_ssim(x, y, u) - R.ref_ssim_separable(x, y, u)).max()))
    print(f"{family}: two fp64 orderings differ by {worst:.2e}")
    assert worst <= 1e-12


@pytest.mark.parametrize("alpha,beta", [(0.25, -0.5), (0.9, 0.9), (1.0, -1.0), (0.0, 0.75), (0.3, 0.31)])
def test_constant_images_give_the_closed_form(alpha, beta):
    x = np.full((1, 3, 26, 27), alpha, np.float32)
    y = np.full((1, 3, 26, 27), beta, np.float32)
    a, b = float(np.float32(alpha)), float(np.float32(beta))
    want = (2 * a * b + R.C1) / (a * a + b * b + R.C1)
    assert abs(float(R.ref_ssim(x, y, WIN)[0]) - want) <= 1e-12


def test_identical_images_give_one():
    for shape in R.SSIM_SHAPES:
        x, _ = R.make_pair("identical", (2, *shape), seed=5)
        assert np.abs(R.ref_ssim(x, x, WIN) - 1.0).max() <= 1e-12


@pytest.mark.parametrize("family", ["near_constant", "negated"])
def test_fp32_moments_fail_the_gpu_tolerance(family):
    """A tolerance that the wrong arithmetic passes proves nothing: on these families the GPU test's bound must
    reject window moments kept in fp32."""
    worst = 0.0
    for shape in R.SSIM_SHAPES:
        x, y = R.make_pair(family, (3, *shape), seed=7)
        worst = max(worst, float(np.abs(R.ref_ssim(x, y, WIN, dtype=np.float32) - R.ref_ssim(x, y, WIN)).max()))
    print(f"{family}: fp32 moments are off by {worst:.2e}")
    assert worst > R.SSIM_TOL


def test_pair_error_reference_and_bound():
    x, y = R.make_pair("noise", (2, 1027), seed=1)
    want = R.ref_pair_error(x, y)
    d = x.astype(np.float64) - y.astype(np.float64)
    assert want[0, 0] == pytest.approx(float((d[0] ** 2).sum()), rel=1e-13) and want[1, 2] == np.abs(d[1]).max()
    assert R.pair_error_close(want, want, 1027)
    off = want.copy()
    off[0, 0] *= 1.0 + 1e-9
    assert not R.pair_error_close(off, want, 1027)
    off = want.copy()
    off[1, 2] = np.nextafter(off[1, 2], 1.0)
    assert not R.pair_error_close(off, want, 1027)
    z, _ = R.make_pair("identical", (1, 64), seed=2)
    assert (R.ref_pair_error(z, z) == 0).all()
    for E in (R.PE_CHUNK - 1, R.PE_CHUNK, R.PE_CHUNK + 1, R.PE_TRIP, 2 * R.PE_CHUNK + 1):
        assert E in R.PAIR_SIZES


def test_error_block_arithmetic():
    from qarig import recon_eval
    # two images of 4 elements: squared errors 0.04 and 0.12, absolute 0.4 and 0.6, maxima 0.1 and 0.3
    b = recon_eval.error_block([[0.04, 0.4, 0.1], [0.12, 0.6, 0.3]], 4, 2.0, ssim=[0.5, 0.25])
    assert b["mse"] == pytest.approx(0.02, rel=1e-15) and b["mae"] == pytest.approx(0.125, rel=1e-15)
    assert b["max_abs"] == 0.3 and b["per_image_mse"] == [0.01, 0.03]
    assert b["psnr"] == pytest.approx(10 * math.log10(4.0 / 0.02), rel=1e-15)        # 23.0103 dB
    assert b["ssim"] == 0.375 and b["per_image_ssim"] == [0.5, 0.25]
    z = recon_eval.error_block([[0.0, 0.0, 0.0]], 16, 2.0)
    assert z["mse"] == 0.0 and z["psnr"] is None and "ssim" not in z
    # a NaN or an inf in one image reaches the totals and leaves the other image's entry alone
    bad = recon_eval.error_block([[math.nan, math.nan, math.nan], [0.12, 0.6, 0.3]], 4, 2.0)
    assert bad["mse"] != bad["mse"] and bad["psnr"] != bad["psnr"] and bad["max_abs"] != bad["max_abs"]
    assert bad["per_image_mse"][1] == 0.03
    bad = recon_eval.error_block([[0.12, 0.6, 0.3], [math.inf, math.inf, math.inf]], 4, 2.0)
    assert bad["mse"] == math.inf and bad["psnr"] == -math.inf and bad["max_abs"] == math.inf
    # data_range 1: 10 log10(1 / 0.25)
    assert recon_eval.error_block([[1.0, 2.0, 0.5]], 4, 1.0)["psnr"] == pytest.approx(6.020599913279624, rel=1e-14)


def test_usage_block_arithmetic():
    from qarig import recon_eval
    u = recon_eval.usage_block([2, 2, 0, 4, 0, 0, 0, 0])
    assert (u["codes"], u["used"], u["dead"]) == (8, 3, 5) and u["counts"] == [2, 2, 0, 4, 0, 0, 0, 0]
    assert u["entropy_bits"] == pytest.approx(1.5, rel=1e-15)                 # 1/4, 1/4, 1/2
    assert u["perplexity"] == pytest.approx(2.0 ** 1.5, rel=1e-15) and u["max_share"] == 0.5
    flat = recon_eval.usage_block([3] * 16)
    assert flat["perplexity"] == pytest.approx(16.0, rel=1e-14) and flat["dead"] == 0
    one = recon_eval.usage_block([0, 7])
    assert one["perplexity"] == 1.0 and one["entropy_bits"] == 0.0 and one["max_share"] == 1.0 and one["dead"] == 1


def test_summary_line_and_per_image_stripping():
    from qarig import recon_eval
    e = recon_eval.error_block([[0.04, 0.4, 0.1]], 4, 2.0, ssim=[0.5])
    block = {"latent": recon_eval.error_block([[0.0, 0.0, 0.0]], 4, 2.0), "vs_decoder": e,
             "usage": recon_eval.usage_block([1, 0, 3])}
    line = recon_eval.recon_summary_line("Val", block)
    assert line.startswith("Val Latent MSE: 0.000000 | PSNR: 26.021 | SSIM: 0.50000 | used: 2 / 3 | perplexity: ")
    slim = recon_eval.without_per_image(block)
    assert set(slim["vs_decoder"]) == {"mse", "mae", "max_abs", "psnr", "ssim"} and slim["usage"] == block["usage"]
    assert "per_image_mse" in block["vs_decoder"]                             # the original is left alone
    assert recon_eval.recon_summary_line("Eval autoencoder", {"vs_image": e}).startswith("Eval autoencoder Image MSE: ")


def test_evaluate_reconstruction_arguments():
    import evaluate_reconstruction as ER
    a = ER.parse_args(["--dataset-path", "d.json", "--decoder-path", "dec.pt"])
    assert a["codebook_path"] == [] and a["with_images"] is False and a["data_range"] == 2.0
    assert a["device"] == "cpu" and a["max_batches"] is None and a["out_json"] is None and a["batch_size"] == 8
    a = ER.parse_args(["--device", "cuda", "--dataset-path", "d.json", "--decoder-path", "dec.pt", "--codebook-path",
                       "a/cb.pt", "--codebook-path", "b/cb.pt", "--codebook-path", "hr.pt", "--with-images",
                       "--batch-size", "3", "--max-batches", "2", "--data-range", "1.0", "--out-json", "o/r.json"])
    assert [str(p) for p in a["codebook_path"]] == ["a/cb.pt", "b/cb.pt", "hr.pt"] and a["with_images"] is True
    assert (a["batch_size"], a["max_batches"], a["data_range"]) == (3, 2, 1.0)
    assert ER.codebook_names(a["codebook_path"]) == ["cb", "cb_2", "hr"]
    assert ER.codebook_names(["x/cb.pt", "y/cb.pt", "z/cb.pt", "cb_2.pt"]) == ["cb", "cb_2", "cb_3", "cb_2_2"]
    with pytest.raises(SystemExit):
        ER.parse_args(["--decoder-path", "dec.pt"])
    from qarig import cli_common as cc
    with pytest.raises(SystemExit):
        cc.require_gpu("cpu")
    assert "single-process" in ER.__doc__.lower()


def test_new_entries_refuse_bad_arguments_without_a_device():
    """Every call below is refused before any launch (X is a made-up address that is never dereferenced), so the
    test is as safe on a box with a GPU as on one without."""
    from qarig import _lib
    h = _lib.load()
    X = 0x7f0000000000
    win = (ctypes.c_double * 15)(*([1.0 / 15] * 15))
    wp = ctypes.cast(win, ctypes.c_void_p)
    big = 1 << 40

    def ssim(N=2, C=3, H=32, W=32, taps=11, ws_bytes=big, null=None):
        a = [X, X, N, C, H, W, wp, taps, R.C1, R.C2, X, X, ws_bytes, None]
        if null is not None:
            a[null] = None
        return h.qarig_ssim(*a)

    for taps in (0, 2, 10, 16, 17, -1):                        # even, out of range
        assert ssim(taps=taps) == -1 and "taps" in _lib.last_error(), taps
        assert h.qarig_ssim_workspace_bytes(2, 3, 32, 32, taps) == 0
    assert ssim(H=10, W=32) == -1
    assert "10 x 32" in _lib.last_error() and "11" in _lib.last_error()      # both values named
    assert ssim(H=32, W=7, taps=9) == -1 and "32 x 7" in _lib.last_error() and "9" in _lib.last_error()
    for null in (0, 1, 6, 10, 11):
        assert ssim(null=null) == -1 and "null" in _lib.last_error()
    for N, C, H, W in ((0, 3, 32, 32), (2, 0, 32, 32), (2 ** 25, 1, 32, 32), (2 ** 20, 2 ** 10, 2 ** 10, 2 ** 10)):
        assert ssim(N=N, C=C, H=H, W=W) == -1
    need = h.qarig_ssim_workspace_bytes(2, 3, 32, 32, 11)
    assert need == 2 * 3 * 2 * 2 * 8                           # 22 x 22 outputs: 2 x 2 tiles of 16 x 16
    assert h.qarig_ssim_workspace_bytes(1, 1, 11, 11, 11) == 8 and h.qarig_ssim_workspace_bytes(1, 1, 27, 26, 11) == 16
    assert ssim(ws_bytes=need - 1) == -1 and "workspace" in _lib.last_error()
    assert ssim(ws_bytes=0) == -1
    # the size query answers 0 for exactly what the entry refuses
    for N, C, H, W in ((0, 3, 32, 32), (2 ** 25, 1, 32, 32), (2 ** 20, 2 ** 10, 2 ** 10, 2 ** 10), (2, 3, 10, 32),
                       (2 ** 20, 2 ** 11, 11, 11)):             # the last: 2^31 workgroups
        assert h.qarig_ssim_workspace_bytes(N, C, H, W, 11) == 0 and ssim(N=N, C=C, H=H, W=W) == -1, (N, C, H, W)
    assert h.qarig_ssim_workspace_bytes(2 ** 20, 2 ** 11 - 1, 11, 11, 11) == 2 ** 20 * (2 ** 11 - 1) * 8

    def pair(N=2, E=5000, ws_bytes=big, null=None, a_ptr=X):
        a = [a_ptr, X, N, E, X, X, ws_bytes, None]
        if null is not None:
            a[null] = None
        return h.qarig_pair_error(*a)

    for null in (0, 1, 4, 5):
        assert pair(null=null) == -1 and "null" in _lib.last_error()
    for N, E in ((0, 8), (2, 0), (-1, 8), (2 ** 25, 8), (4, 2 ** 39), (2 ** 20, 2 ** 24)):
        assert pair(N=N, E=E) == -1, (N, E)
    assert pair(a_ptr=X + 2) == -1 and "aligned" in _lib.last_error()
    need = h.qarig_pair_error_workspace_bytes(2, 5000)
    assert need == 2 * 2 * 3 * 8                               # two chunks of R.PE_CHUNK elements per image
    assert h.qarig_pair_error_workspace_bytes(1, R.PE_CHUNK) == 24
    assert h.qarig_pair_error_workspace_bytes(1, R.PE_CHUNK + 1) == 48 and h.qarig_pair_error_workspace_bytes(0, 8) == 0
    assert pair(ws_bytes=need - 1) == -1 and "workspace" in _lib.last_error()
    assert pair(ws_bytes=0) == -1
    for N, E in ((0, 8), (2, 0), (2 ** 25, 8), (4, 2 ** 39), (2 ** 20, 2 ** 24), (2 ** 24, 2 ** 16 + 1)):
        assert h.qarig_pair_error_workspace_bytes(N, E) == 0 and pair(N=N, E=E) == -1, (N, E)
    assert h.qarig_pair_error_workspace_bytes(2 ** 24, 2 ** 16) == 2 ** 24 * 16 * 24


def test_ops_refuse_cpu_tensors():
    import torch
    from qarig import ops
    x = torch.zeros(1, 1, 11, 11)
    with pytest.raises(RuntimeError):
        ops.ssim(x, x)
    with pytest.raises(RuntimeError):
        ops.pair_error(x, x)
    w = ops.gaussian_window(11, 1.5)
    assert w == list(R.gaussian_window(11, 1.5)) or np.abs(np.array(w) - R.gaussian_window(11, 1.5)).max() < 1e-16
    assert abs(math.fsum(w) - 1.0) < 1e-15 and w[5] == max(w) and w[0] == w[10]
