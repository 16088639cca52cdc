"""Host side of the chunked coarse-pass BMU search (K > 1024): image and workspace sizes, and the argument checks of
qarig_bmu_fwd_coarse_ws, none of which touches a GPU."""
from conftest import PKG  # noqa: F401  (puts the package on sys.path)


def _lib():
    import build as qbuild
    qbuild.build_lib(verbose=False)
    from qarig import _lib
    return _lib.load(), _lib


def test_prepared_image_and_workspace_sizes():
    h, _ = _lib()
    assert h.qarig_bmu_prepare_bytes(8192, 4) > 0
    assert h.qarig_bmu_prepare_bytes(1056, 4) > 0
    assert h.qarig_bmu_prepare_bytes(16416, 4) == 0
    assert h.qarig_bmu_prepare_bytes(8192, 20) == 0
    assert h.qarig_bmu_prepare_bytes(512, 16) == 512 * 100 + 16          # the single-image layout is unchanged
    assert h.qarig_bmu_prepare_bytes(1024, 16) == 1024 * 100 + 16
    # chunk-major: every chunk's planes + |w|^2 (100 B per code) and a 16-B header slot
    assert h.qarig_bmu_prepare_bytes(8192, 4) == 8192 * 100 + 16 * 16
    assert h.qarig_bmu_prepare_bytes(1056, 4) == 1056 * 100 + 3 * 16
    assert h.qarig_bmu_coarse_workspace_bytes(8192, 8192) > 0
    assert h.qarig_bmu_coarse_workspace_bytes(8192, 1024) == 0
    assert h.qarig_bmu_coarse_workspace_bytes(8192, 16416) == 0
    # the dispatcher's workspace covers the chunked form
    for rows, K in ((8192, 8192), (64, 2048), (32768, 16384), (2652, 1056)):
        assert h.qarig_bmu_workspace_bytes(rows, K) >= h.qarig_bmu_coarse_workspace_bytes(rows, K) > 0


def test_coarse_ws_entry_checks_its_arguments_without_a_gpu():
    h, lib = _lib()
    X = 0x7f0000000000           # a fake, 16-B aligned device address: never dereferenced on the host
    need = h.qarig_bmu_coarse_workspace_bytes(8192, 8192)
    args = (2, 4, 64, 64, 1, 1)
    assert h.qarig_bmu_fwd_coarse_ws(None, *args, X, 8192, 4, X, None, None, X, need, None) == -1
    assert "null pointer" in lib.last_error()
    assert h.qarig_bmu_fwd_coarse_ws(X, *args, None, 8192, 4, X, None, None, X, need, None) == -1
    assert h.qarig_bmu_fwd_coarse_ws(X, *args, X, 8192, 4, None, None, None, X, need, None) == -1
    assert h.qarig_bmu_fwd_coarse_ws(X, *args, X, 8192, 4, X, None, None, X, need - 1, None) == -3
    assert "workspace too small" in lib.last_error()
    assert h.qarig_bmu_fwd_coarse_ws(X, *args, X, 8192, 4, X, None, None, None, need, None) == -3
    # K the coarse form does not take: not a multiple of 32, beyond 16,384; the plain entry keeps its K <= 1024
    assert h.qarig_bmu_fwd_coarse_ws(X, *args, X, 8200, 4, X, None, None, X, 1 << 40, None) == -1
    assert h.qarig_bmu_fwd_coarse_ws(X, *args, X, 16416, 4, X, None, None, X, 1 << 40, None) == -1
    assert h.qarig_bmu_fwd_coarse(X, *args, X, 8192, 4, X, None, None, None) == -1
    assert "<= 1024" in lib.last_error()
