"""Kernel-routing decisions of the fp32 GEMM that the host can check without a GPU: which products go to the
64 x 64-tile kernel (qarig_gemm_tile64) and the reduction splits the host picks for them."""
from conftest import PKG  # noqa: F401  (puts the package on sys.path)


def test_long_k_weight_gradient_stays_on_the_ring():
    """The 512 x 512 weight gradient over 16,384 rows (16 tiles of 128 x 128, K = 16,384) goes to the 128-tile
    ring at 32 splits of 512, not to the 64-tile kernel; the short-K shapes that kernel was built for keep it."""
    from qarig import _lib, ops
    lib = _lib.load()
    assert lib.qarig_gemm_tile64(512, 512, 16384) == 0
    assert lib.qarig_gemm_tile64(512, 512, 4096) == 0
    assert ops._tile64_splitk(512, 512, 16384) == 0
    assert ops.pick_splitk(512, 512, 16384) == 32
    # 16 tiles of 128 up to K = 2,048, and any small grid up to K = 1,024: still the 64-tile kernel
    assert lib.qarig_gemm_tile64(512, 512, 2048) == 1 and ops.pick_splitk(512, 512, 2048) == 4
    assert lib.qarig_gemm_tile64(512, 512, 1024) == 1
    assert lib.qarig_gemm_tile64(2048, 512, 512) == 1 and ops.auto_splitk(2048, 512, 512) == 1
    assert lib.qarig_gemm_tile64(2048, 512, 2048) == 0 and lib.qarig_gemm_tile64(16384, 2048, 512) == 0
    # the other weight gradients of the step keep their splits
    assert ops.pick_splitk(2048, 512, 16384) == 8 and ops.pick_splitk(512, 2048, 16384) == 8


def test_tile64_option_still_forces_and_disables():
    from qarig import _lib
    lib = _lib.load()
    old = _lib.set_option("gemm_tile64", 1)
    try:
        assert lib.qarig_gemm_tile64(512, 512, 16384) == 1
        _lib.set_option("gemm_tile64", 0)
        assert lib.qarig_gemm_tile64(2048, 512, 512) == 0
    finally:
        _lib.set_option("gemm_tile64", old)
    assert lib.qarig_gemm_tile64(512, 512, 16384) == 0
