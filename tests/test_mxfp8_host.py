"""The "mxfp8" precision mode on the host side (no GPU): the mode switch, and which product shapes
the MX-e4m3 GEMM takes (include/qarig.h qarig_gemm_mx_supported)."""
import pytest


@pytest.fixture
def restore_precision():
    from qarig import ops
    old = ops.PRECISION
    yield ops
    ops.PRECISION = old


def test_set_precision_accepts_mxfp8(restore_precision):
    ops = restore_precision
    ops.set_precision("mxfp8")
    assert ops.PRECISION == "mxfp8" and ops.lp_mode()
    assert "mxfp8" in ops.PRECISIONS
    with pytest.raises(ValueError):
        ops.set_precision("mxfp4")


# config-5 products (profiles/r03_c5_gemm_by_shape.txt) as the MX nodes issue them: forward and input
# gradients (M tokens, N, K), weight gradients (N, K, M tokens) with the split the node picks
C5_ROWS = (32768, 8192, 4224)
C5_WIDTHS = ((2048, 512), (512, 2048), (8320, 2048), (2048, 8320), (512, 512))


def test_gemm_mx_supported_covers_config5_products():
    from qarig import functional_lp as FL
    from qarig import ops
    for M in C5_ROWS:
        for N, K in C5_WIDTHS:
            assert ops.mx_supported(M, N, K), (M, N, K)
            sk = FL._mx_splitk((N // 128) * (K // 128), M)
            assert ops.mx_supported(N, K, M, sk), (N, K, M, sk)
            assert M % sk == 0 and (M // sk) % 128 == 0
    # the 4,224-row weight gradients split by a divisor of 33 tiles (the bf16 path's 6 is not one)
    assert FL._mx_splitk(16 * 4, 4224) == 3


@pytest.mark.parametrize("M,N,K,splitk", [(100, 128, 128, 1), (128, 96, 128, 1), (128, 128, 64, 1),
                                          (128, 128, 8193, 1), (128, 128, 512, 3), (128, 128, 384, 2),
                                          (0, 128, 128, 1)])
def test_gemm_mx_refuses_ragged_shapes(M, N, K, splitk):
    from qarig import ops
    assert not ops.mx_supported(M, N, K, splitk)


def test_mx_entry_points_validate_without_a_gpu():
    from qarig import _lib
    h = _lib.load()
    assert h.qarig_gemm_mx_workspace_bytes(256, 512, 4) == 4 * 256 * 512 * 4
    assert h.qarig_mx_quant_workspace_bytes(1000, 256) == (1024 // 64) * 256 * 4
    assert h.qarig_mx_quant(None, 128, 0, 128, 128, None, None, None, None, None, 0, None, 0, None) == -1
    assert h.qarig_mx_quant(1 << 12, 100, 0, 128, 100, None, None, None, None, None, 0, None, 0, None) == -1
    assert h.qarig_gemm_mx(None, 0, None, 0, None, 0, None, 0, None, 0, 128, 128, 128, None, None, 0, None, 0,
                           0, None, 0, 0, 0, 1, 0, None, 0, None, 0, None, 0, None) == -1
    assert "null operand" in _lib.last_error()
