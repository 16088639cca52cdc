"""Which position-table shapes the training forward sends to the strided-groups ring launch
(qarig_gemm_f32_strided), and what that entry refuses, checked on the host without a GPU."""
from conftest import PKG  # noqa: F401  (puts the package on sys.path)


def test_table_shapes_that_take_the_strided_ring():
    from qarig import ops
    assert ops.gemm_strided_supported(384, 512, 512)          # BASELINE config 2: 384 positions, D = 512
    assert ops.gemm_strided_supported(128, 256, 256)
    assert not ops.gemm_strided_supported(200, 256, 256)      # rows no multiple of 128: the skinny launch
    assert not ops.gemm_strided_supported(385, 512, 512)
    assert not ops.gemm_strided_supported(384, 192, 192)      # output columns no multiple of 128
    assert not ops.gemm_strided_supported(384, 256, 200)      # half a k-tile
    # the training forward takes it where the launch gives every CU a workgroup
    assert ops.table_forward_ring(42, 384, 512)               # config 2: 504 tiles
    assert not ops.table_forward_ring(30, 256, 512)           # config 4's encoder table: 240 tiles, skinny as before
    assert not ops.table_forward_ring(42, 200, 512)


def test_strided_entry_validates_before_it_launches():
    from qarig import _lib
    lib = _lib.load()
    a = 4096                                                    # a 16-B aligned stand-in address: nothing is launched
    ok_tail = (2, 128, 128, 64, 0, None)
    assert lib.qarig_gemm_f32_strided(None, 64, a, 64, 128 * 64, a, 128, 128 * 128, None, 0, *ok_tail) == -1
    assert "null operand" in _lib.last_error()
    assert lib.qarig_gemm_f32_strided(a, 64, a, 64, 128 * 64, a, 128, 128 * 128, None, 0, 2, 100, 128, 64, 0,
                                      None) == -1
    assert "128" in _lib.last_error()
    # groups that overlap: a weight stride shorter than one weight, an output stride shorter than one output
    assert lib.qarig_gemm_f32_strided(a, 64, a, 64, 64 * 64, a, 128, 128 * 128, None, 0, *ok_tail) == -1
    assert "overlap" in _lib.last_error()
    assert lib.qarig_gemm_f32_strided(a, 64, a, 64, 128 * 64, a, 128, 64 * 128, None, 0, *ok_tail) == -1
    assert "overlap" in _lib.last_error()
    assert lib.qarig_gemm_f32_strided(a + 4, 64, a, 64, 128 * 64, a, 128, 128 * 128, None, 0, *ok_tail) == -1
    assert "aligned" in _lib.last_error()
    assert lib.qarig_gemm_f32_strided(a, 64, a, 64, 128 * 64, a, 128, 128 * 128, None, 0, 0, 128, 128, 64, 0,
                                      None) == -1
    assert "groups" in _lib.last_error()
