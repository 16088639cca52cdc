"""ops.dropout (csrc/dropout.hip) against the NumPy reference of tests/dropout_cases.py, bit for bit: the output is
one correctly rounded fp32 multiply or +0, so the tolerance is zero.  Sizes around one Philox call (8 elements), the
16-byte vector, a workgroup's worth of calls, and one size just past a full sweep of the capped grid (the
grid-stride loop wraps); every alignment of x and y that picks another path; in place; special values; canaries
either side of y; the step read from the device key; argument errors."""
import numpy as np
import pytest
import torch

import dropout_cases as C

pytestmark = pytest.mark.gpu

CANARY = np.float32(-12345.678)
PAD = 8        # canary elements either side of y (and of x); 8 floats keep the 16-byte phase of the base


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _key(seed, step, rank):
    from qarig.dropout import DropoutKey
    k = DropoutKey(seed, rank, torch.device("cuda", 0))
    k.set_step(step)
    return k


def _launch(x_np, t, s, site, key, x_off=0, y_off=0, inplace=False):
    """Runs ops.dropout on a copy of x_np placed x_off floats past a 16-byte boundary, into a y placed y_off
    floats past one (or in place); returns (y as numpy, x afterwards as numpy) after checking the canaries."""
    from qarig import ops
    n = x_np.size
    xbuf = torch.full((n + 2 * PAD + 1,), float(CANARY), dtype=torch.float32, device="cuda")
    assert xbuf.data_ptr() % 16 == 0
    x = xbuf[PAD + x_off:PAD + x_off + n]
    x.copy_(torch.from_numpy(np.array(x_np)))       # (a copy: the shared inputs are read-only arrays)
    assert x.data_ptr() % 16 == 4 * x_off
    if inplace:
        ybuf, y, y_off = xbuf, x, x_off
    else:
        ybuf = torch.full((n + 2 * PAD + 1,), float(CANARY), dtype=torch.float32, device="cuda")
        y = ybuf[PAD + y_off:PAD + y_off + n]
        assert y.data_ptr() % 16 == 4 * y_off
    out = ops.dropout(x, t, float(s), site, key.buffer, out=y)
    assert out.data_ptr() == y.data_ptr()
    host = ybuf.cpu().numpy()
    lo, hi = host[:PAD + y_off], host[PAD + y_off + n:]
    assert np.array_equal(_bits(lo), _bits(np.full_like(lo, CANARY))), "canary before y overwritten"
    assert np.array_equal(_bits(hi), _bits(np.full_like(hi, CANARY))), "canary behind y overwritten"
    return host[PAD + y_off:PAD + y_off + n].copy(), x.cpu().numpy()


def _assert_bits(got, want, what):
    gb, wb = _bits(got), _bits(want)
    bad = np.flatnonzero(gb != wb)
    assert bad.size == 0, (f"{what}: {bad.size} of {gb.size} differ, first at {bad[:5]}: got {got[bad[:5]]} "
                           f"want {want[bad[:5]]}")


@pytest.mark.parametrize("p", C.KERNEL_PS)
def test_against_reference_every_size_and_alignment(p):
    t, s = C.threshold_and_scale(p)
    rng = np.random.default_rng(int(p * 100))
    site, step, rank = 5, 7, 2
    key = _key(C.KERNEL_SEED, step, rank)
    dropped = kept = 0
    for n in C.KERNEL_NS:
        x = C.special_values(n, rng)
        want = C.apply(x, t, s, C.KERNEL_SEED, site, step, rank)
        for x_off, y_off in ((0, 0), (1, 0), (0, 1), (1, 1), (3, 2)):
            got, x_after = _launch(x, t, s, site, key, x_off, y_off)
            _assert_bits(got, want, f"n={n} p={p} x_off={x_off} y_off={y_off}")
            _assert_bits(x_after, x, "x changed by an out-of-place launch")
        for off in (0, 1):
            got, _ = _launch(x, t, s, site, key, off, inplace=True)
            _assert_bits(got, want, f"in place n={n} p={p} off={off}")
        keep = C.mask(n, t, C.KERNEL_SEED, site, step, rank)
        dropped += int((~keep).sum())
        kept += int(keep.sum())
    assert dropped > 0 and kept > 0


def test_sites_steps_ranks_and_seed_words():
    """Two sites, two steps, two ranks: each stream is the reference's, and they all differ from one another; both
    halves of the 64-bit seed reach the key."""
    t, s = C.threshold_and_scale(0.5)
    n = 2051
    x = np.random.default_rng(1).standard_normal(n).astype(np.float32)
    outs = {}
    for site, step, rank in C.KERNEL_STREAMS:
        got, _ = _launch(x, t, s, site, _key(C.KERNEL_SEED, step, rank), 0, 0)
        _assert_bits(got, C.apply(x, t, s, C.KERNEL_SEED, site, step, rank), f"stream {(site, step, rank)}")
        outs[(site, step, rank)] = got
    keys = list(outs)
    for i in range(len(keys)):
        for j in range(i):
            assert not np.array_equal(outs[keys[i]], outs[keys[j]])
    for seed in (0, 1, 1 << 32, 0xFFFFFFFFFFFFFFFF):
        got, _ = _launch(x, t, s, 0, _key(seed, 1, 0), 0, 0)
        _assert_bits(got, C.apply(x, t, s, seed, 0, 1, 0), f"seed {seed:#x}")
    # site and rank words with the top bit set
    got, _ = _launch(x, t, s, 0xFFFFFFFF, _key(C.SEED, 0xFFFFFFFF, 0x80000000), 0, 0)
    _assert_bits(got, C.apply(x, t, s, C.SEED, 0xFFFFFFFF, 0xFFFFFFFF, 0x80000000), "32-bit counter words")


def test_step_is_read_from_the_device_buffer():
    """Two launches with a set_step between them, nothing else changed (same key object, same buffer address)."""
    from qarig import ops
    t, s = C.threshold_and_scale(0.25)
    x_np = np.random.default_rng(2).standard_normal(4096 + 3).astype(np.float32)
    x = torch.from_numpy(x_np).cuda()
    key = _key(C.SEED, 1, 0)
    addr = key.buffer.data_ptr()
    y1 = ops.dropout(x, t, float(s), 3, key.buffer)
    key.set_step(2)
    y2 = ops.dropout(x, t, float(s), 3, key.buffer)
    key.set_step(1)
    y3 = ops.dropout(x, t, float(s), 3, key.buffer)
    assert key.buffer.data_ptr() == addr and key.buffer.dtype == torch.int32 and key.buffer.shape == (4,)
    _assert_bits(y1.cpu().numpy(), C.apply(x_np, t, s, C.SEED, 3, 1, 0), "step 1")
    _assert_bits(y2.cpu().numpy(), C.apply(x_np, t, s, C.SEED, 3, 2, 0), "step 2")
    assert torch.equal(y1, y3) and not torch.equal(y1, y2)
    assert key.buffer.tolist() == [C.SEED, 0, 1, 0]


@pytest.fixture(scope="module")
def wrap_case():
    """One n just past a full sweep of the capped grid (ops.DROPOUT_SWEEP = 8192 workgroups x 256 threads x 8
    elements): two more workgroups' worth and an odd tail.  Input and reference are made once."""
    from qarig import ops
    n = ops.DROPOUT_SWEEP + 2 * 256 * 8 + 5
    t, s = C.threshold_and_scale(0.1)
    x = np.random.default_rng(3).standard_normal(n).astype(np.float32)
    want = C.apply(x, t, s, C.SEED, 1, 2, 0)
    want.setflags(write=False)
    x.setflags(write=False)
    return n, t, s, x, want


@pytest.mark.parametrize("x_off,y_off", [(0, 0), (1, 1)])
def test_grid_stride_loop_wraps(wrap_case, x_off, y_off):
    n, t, s, x, want = wrap_case
    got, _ = _launch(x, t, s, 1, _key(C.SEED, 2, 0), x_off, y_off)
    _assert_bits(got, want, f"n={n} x_off={x_off} y_off={y_off}")
    _assert_bits(got[-(2 * 256 * 8 + 5):], want[-(2 * 256 * 8 + 5):], "the wrapped part")


def test_argument_errors_return_the_code():
    """Null pointers and out-of-range scalars, all caught by the host check: -1, a message, and no launch."""
    from qarig import _lib, ops
    lib = _lib.load()
    x = torch.zeros(64, dtype=torch.float32, device="cuda")
    y = torch.zeros(64, dtype=torch.float32, device="cuda")
    key = _key(1, 1, 0)
    px, py, pk = x.data_ptr(), y.data_ptr(), key.buffer.data_ptr()
    st = _lib.stream()
    bad = [(None, py, 64, 100, 1.0, 0, pk), (px, None, 64, 100, 1.0, 0, pk), (px, py, 64, 100, 1.0, 0, None),
           (px, py, 0, 100, 1.0, 0, pk), (px, py, -5, 100, 1.0, 0, pk), (px, py, (1 << 34) + 1, 100, 1.0, 0, pk),
           (px, py, 64, 0, 1.0, 0, pk), (px, py, 64, C.MAX_T + 1, 1.0, 0, pk), (px, py, 64, 65536, 1.0, 0, pk),
           (px, px + 16, 32, 100, 1.0, 0, pk)]          # partial overlap
    for a in bad:
        assert lib.qarig_dropout(*a, st) == -1, a
        assert "dropout" in _lib.last_error()
    torch.cuda.synchronize()
    assert float(x.abs().sum()) == 0 and float(y.abs().sum()) == 0
    # and the Python layer: wrong dtype, not contiguous, CPU tensors, threshold out of range
    with pytest.raises(TypeError):
        ops.dropout(x.double(), 100, 1.0, 0, key.buffer)
    with pytest.raises(TypeError):
        ops.dropout(x.view(8, 8).t(), 100, 1.0, 0, key.buffer)
    with pytest.raises(TypeError):
        ops.dropout(x, 100, 1.0, 0, key.buffer.float())
    with pytest.raises(RuntimeError):
        ops.dropout(x.cpu(), 100, 1.0, 0, key.buffer)
    for t in (0, C.MAX_T + 1, -1):
        with pytest.raises(ValueError):
            ops.dropout(x, t, 1.0, 0, key.buffer)
