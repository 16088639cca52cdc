"""Which weight-gradient shapes qarig_gemm_f32 sends through its ragged route (ring on the first 128 q output
rows, tail kernels on the last r), the reduction split callers pick for them and the workspace they are given,
checked on the host without a GPU."""
from conftest import PKG  # noqa: F401  (puts the package on sys.path)


def test_which_weight_gradients_take_the_ragged_route():
    from qarig import _lib, ops
    lib = _lib.load()
    # (output rows, output columns, reduction length)
    assert lib.qarig_gemm_ragged_tn(513, 2048, 16384) == 1        # BASELINE config 2's classifier
    assert lib.qarig_gemm_ragged_tn(385, 128, 4096) == 1          # the smallest eligible one
    assert lib.qarig_gemm_ragged_tn(264, 256, 4096) == 1          # q = 2, r = 8
    assert lib.qarig_gemm_ragged_tn(265, 256, 4096) == 0          # r = 9: the padded / guarded paths stay
    assert lib.qarig_gemm_ragged_tn(512, 2048, 16384) == 0        # nothing ragged
    assert lib.qarig_gemm_ragged_tn(129, 256, 4096) == 0          # q = 1: not a wide output layer
    assert lib.qarig_gemm_ragged_tn(513, 2048, 2048) == 0         # config 4's 2,048-row shard: as before
    assert lib.qarig_gemm_ragged_tn(513, 2000, 16384) == 0        # ragged columns
    assert lib.qarig_gemm_ragged_tn(513, 2048, 16392) == 0        # half a k-tile
    # the split is chosen for the rows the ring runs: the 512-row product's, one split per XCD
    assert ops.wgrad_ring_rows(513, 2048, 16384) == 512
    assert ops.pick_splitk(ops.wgrad_ring_rows(513, 2048, 16384), 2048, 16384) == ops.pick_splitk(512, 2048, 16384) == 8
    assert ops.wgrad_ring_rows(640, 2048, 16384) == 640 and ops.wgrad_ring_rows(513, 2048, 2048) == 513


def test_which_forward_products_take_the_ragged_route():
    from qarig import _lib, ops
    lib = _lib.load()
    # (rows, output columns, reduction length)
    assert lib.qarig_gemm_ragged_nt(16384, 513, 2048) == 1        # BASELINE config 2's classifier
    assert lib.qarig_gemm_ragged_nt(4096, 385, 128) == 1          # the smallest eligible one
    assert lib.qarig_gemm_ragged_nt(4096, 264, 2048) == 1         # r = 8: 8 x 2048 weights fill the LDS buffer
    assert lib.qarig_gemm_ragged_nt(4096, 264, 2064) == 0         # ... and no more
    assert lib.qarig_gemm_ragged_nt(4096, 265, 272) == 0          # r = 9
    assert lib.qarig_gemm_ragged_nt(4096, 129, 272) == 0          # q = 1
    assert lib.qarig_gemm_ragged_nt(2048, 513, 2048) == 0         # config 4's 2,048-row shard: as before
    assert lib.qarig_gemm_ragged_nt(4100, 513, 2048) == 0         # ragged rows
    assert lib.qarig_gemm_ragged_nt(4096, 513, 2056) == 0         # half a k-tile
    # the Linear nodes drop their padded copies only where forward and weight gradient both route
    assert ops.ragged_output_native(16384, 513, 2048)
    assert not ops.ragged_output_native(16384, 513, 272)          # weight gradient columns no multiple of 128
    assert not ops.ragged_output_native(2048, 513, 2048)


def test_workspace_covers_the_tail_partials():
    from qarig import _lib
    lib = _lib.load()
    ring = lambda M, N, s: (s * M * N * 4 if s > 1 else 0) + max(s, 1) * M * 4   # noqa: E731
    # unchanged for whole tiles and for shapes the route never takes
    assert lib.qarig_gemm_workspace_bytes(512, 2048, 8) == ring(512, 2048, 8)
    assert lib.qarig_gemm_workspace_bytes(640, 2048, 4) == ring(640, 2048, 4)
    assert lib.qarig_gemm_workspace_bytes(129, 256, 2) == ring(129, 256, 2)
    # ragged rows: 128 row-block partials of r x N outputs and r row sums behind the ring's share
    for M, N, s in ((513, 2048, 8), (264, 256, 1), (385, 128, 4)):
        r = M % 128
        assert lib.qarig_gemm_workspace_bytes(M, N, s) == ring(M, N, s) + 128 * r * (N + 1) * 4
        assert lib.qarig_gemm_workspace_bytes(M, N, s) >= ring(M - r, N, s) + 128 * r * (N + 1) * 4


def test_cross_entropy_ld_entry_validates_its_leading_dimensions():
    from qarig import _lib
    lib = _lib.load()
    a = 4096                                                    # a stand-in address: nothing is launched
    assert lib.qarig_cross_entropy_ld_fwd(a, 512, a, 4, 513, a, a, 528, a, a, None) == -1      # logits rows overlap
    assert "leading dimensions" in _lib.last_error()
    assert lib.qarig_cross_entropy_ld_fwd(a, 528, a, 4, 513, a, a, 512, a, a, None) == -1      # gradient rows overlap
    assert "leading dimensions" in _lib.last_error()
    assert lib.qarig_cross_entropy_ld_fwd(None, 528, a, 4, 513, a, a, 528, a, a, None) == -1
    assert "bad arguments" in _lib.last_error()
