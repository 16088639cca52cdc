"""Scratch sizes of the conv entry points (csrc/conv.hip): the *_workspace_bytes_n functions answer from the plan
that also drives the ring launches (conv_ring_plan), so a size promises slabs exactly where a launch would split.
Host arithmetic only: no GPU is touched."""
from conftest import PKG  # noqa: F401  (puts the package on sys.path)

# (N, Cin, H, W, Cout, k, stride) -> bytes
FWD = [
    ((1, 64, 16, 16, 128, 3, 1), 557056),
    ((4, 256, 32, 32, 128, 3, 1), 17956864),
    ((2, 512, 16, 16, 256, 3, 1), 8912896),
    ((4, 512, 32, 32, 512, 3, 1), 42991616),       # one 512 -> 512 layer of the README decoder at 4 images
    ((32, 512, 32, 32, 512, 3, 1), 9437184),       # fills the chip: no parts
    ((4, 256, 64, 64, 3, 3, 1), 27648),            # direct kernel
    ((2, 128, 32, 32, 256, 3, 2), 3276800),        # stride-2 forward
    ((1, 256, 32, 32, 128, 3, 2), 2228224),
    ((1, 60, 16, 16, 128, 3, 1), 276480),          # Cin % 16
    ((1, 64, 16, 16, 128, 4, 1), 524288),          # not 3x3
    ((1, 64, 8, 8, 128, 3, 1), 294912),            # half a pixel tile
    ((1, 64, 64, 6, 128, 3, 1), 294912),           # W % 4: the launch keeps off the ring, so no slabs
]
# (N, Cin, H, W, Cout) -> bytes
CONVT = [
    ((4, 256, 16, 16, 128), 10485760),
    ((1, 512, 32, 32, 256), 41943040),
    ((16, 512, 32, 32, 256), 8388608),
    ((1, 64, 8, 8, 3), 12288),
]
CONVT_DGRAD = [
    ((1, 512, 32, 32, 256), 25165824),
    ((2, 128, 16, 16, 128), 3145728),
    ((1, 256, 16, 16, 64), 2097152),
    ((8, 128, 4, 4, 16), 131072),
    ((1, 128, 64, 6, 64), 524288),                 # W % 4
]
# (N, Cin, H, W, Cout, k, stride) -> bytes
DGRAD = [
    ((1, 128, 16, 16, 128, 3, 1), 1114112),
    ((2, 512, 16, 16, 256, 3, 1), 13107200),
    ((2, 128, 32, 32, 256, 3, 2), 1179648),        # the stride-2 input gradient is never split
    ((1, 128, 64, 6, 64, 3, 1), 294912),           # W % 4
]
# (Cg, K2, P) -> bytes
WGRAD = [((3, 2304, 65536), 1769472), ((512, 4608, 4096), 56623104)]


def _lib():
    import build as qbuild
    qbuild.build_lib(verbose=False)
    from qarig import _lib
    return _lib.load(), _lib


def _families(h):
    """(sized function, its table, the base size of an argument tuple)"""
    return [
        (h.qarig_conv2d_fwd_workspace_bytes_n, FWD, lambda a: h.qarig_conv2d_fwd_workspace_bytes(a[1], a[4], a[5])),
        (h.qarig_conv_transpose2d_workspace_bytes_n, CONVT, lambda a: h.qarig_conv_transpose2d_workspace_bytes(a[1], a[4])),
        (h.qarig_conv_transpose2d_bwd_data_workspace_bytes_n, CONVT_DGRAD,
         lambda a: h.qarig_conv_transpose2d_workspace_bytes(a[1], a[4])),
        (h.qarig_conv2d_bwd_data_workspace_bytes_n, DGRAD,
         lambda a: h.qarig_conv2d_bwd_data_workspace_bytes(a[1], a[4], a[5])),
    ]


def test_workspace_sizes_of_the_conv_entry_points():
    h, _ = _lib()
    for fn, table, _base in _families(h):
        for args, want in table:
            assert fn(*args) == want, (fn.__name__, args)
    for args, want in WGRAD:
        assert h.qarig_conv_wgrad_workspace_bytes(*args) == want, args


def test_workspace_sizes_promise_no_slabs_with_the_ring_switched_off():
    h, lib = _lib()
    split = 0
    for fn, table, base in _families(h):
        split += sum(fn(*args) > base(args) for args, _ in table)
    assert split >= 12                               # the tables do hold split geometries
    old = lib.set_option("conv_ring", 0)
    try:
        for fn, table, base in _families(h):
            for args, _ in table:
                assert fn(*args) == base(args), (fn.__name__, args)
    finally:
        lib.set_option("conv_ring", old)
    assert h.qarig_conv2d_fwd_workspace_bytes_n(4, 512, 32, 32, 512, 3, 1) == 42991616


def test_workspace_size_is_the_base_where_the_input_is_too_large_for_the_ring():
    """256 workgroups over 9,216 k-tiles would run in two parts, but 2 GB of input is past the ring's 32-bit buffer
    offsets: the launch takes the gather kernel, so no slabs are promised; half the channels fit."""
    h, _ = _lib()
    assert h.qarig_conv2d_fwd_workspace_bytes_n(8, 16384, 64, 64, 128, 3, 1) == \
        h.qarig_conv2d_fwd_workspace_bytes(16384, 128, 3)
    assert h.qarig_conv2d_fwd_workspace_bytes_n(8, 8192, 64, 64, 128, 3, 1) > \
        h.qarig_conv2d_fwd_workspace_bytes(8192, 128, 3)
