"""decode_attention_kernel<HD> (csrc/decode.hip) -- the one kernel behind every attention of cached
generation, reached through ops.attention_decode and ops.window_attention -- against fp64
softmax(q k^T / sqrt(d)) v at every attended length, on both cache layouts, in every form, and on caches
whose rows at or beyond the attended length hold NaN: nothing a caller leaves there may reach the result.

P = 64 U is the number of keys the wave covers per pass (U = 4 / 2 / 1 keys per lane for head dim
<= 16 / 32 / 64).  B = 3 and H = 5 (3 at head dim 64) are no multiples of the 4 heads of a workgroup.
Tolerance: rel_err < 1e-5, the bound this kernel carries in test_gpu_kvcache.py and test_gpu_window_graph.py."""
import math

import pytest
import torch

from conftest import rel_err

pytestmark = pytest.mark.gpu

DIMS = (4, 8, 16, 32, 64)
LAYOUTS = ("row_major", "head_major")
B = 3
TOL = 1e-5
NAN = float("nan")


def _heads(d):
    return 3 if d == 64 else 5


def _pass(d):
    return 256 if d <= 16 else (128 if d == 32 else 64)


def _randn(*shape, seed):
    """Unit-scale data drawn on the CPU (the same numbers on every machine), on the device."""
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).cuda()


def _ref(q, k, v, H):
    """fp64 softmax(q k^T / sqrt(d)) v of one query row per sequence: q (B, D), k / v (B, S, D) -> (B, D)."""
    n, D = q.shape
    d = D // H
    qh = q.double().view(n, H, 1, d)
    kh = k.double().view(n, -1, H, d).transpose(1, 2)
    vh = v.double().view(n, -1, H, d).transpose(1, 2)
    return (torch.softmax(qh @ kh.transpose(-1, -2) / d ** 0.5, dim=-1) @ vh).reshape(n, D)


def _alloc(n, rows, H, d, layout, fill):
    shape = (n, rows, H * d) if layout == "row_major" else (n, H, rows, d)
    return torch.full(shape, fill, device="cuda")


def _put(cache, rows, x):
    """cache rows [0, rows) <- x (B, rows, D)."""
    if cache.dim() == 3:
        cache[:, :rows] = x[:, :rows]
    else:
        n, H, _, d = cache.shape
        cache[:, :, :rows] = x[:, :rows].reshape(n, rows, H, d).permute(0, 2, 1, 3)


def _as_rows(cache):
    """A (B, rows, D) copy of either layout."""
    if cache.dim() == 3:
        return cache.clone()
    n, H, rows, d = cache.shape
    return cache.permute(0, 2, 1, 3).reshape(n, rows, H * d)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    """Bit-for-bit equality, NaN payloads included (torch.equal calls NaN unequal to itself)."""
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _len_dev(n):
    return torch.tensor([n], dtype=torch.int32, device="cuda")


# ---- 1. every length, one appended token at a time ---------------------------------------------------------

@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("d", DIMS)
def test_length_sweep_appending_into_a_nan_cache(d, layout):
    """Sk = 1 .. 2P + 3 by appending token after token, the length in a device word: every pass boundary, lanes
    without keys, the stale (NaN) slot the appended row replaces, NaN rows past the length, the cache's last row."""
    from qarig import ops
    H, P = _heads(d), _pass(d)
    D, T = H * d, 2 * _pass(d) + 3
    q, k, v = (_randn(T, B, D, seed=100 * d + i) for i in range(3))
    kc, vc = _alloc(B, T, H, d, layout, NAN), _alloc(B, T, H, d, layout, NAN)
    ln = _len_dev(0)
    outs = []
    for t in range(T):                      # nothing is read back inside the loop
        ln.fill_(t)
        outs.append(ops.attention_decode(q[t], k[t], v[t], kc, vc, 0, H, len_dev=ln))
    got = torch.stack(outs, 1)              # (B, T, D)
    assert not torch.isnan(got).any(), f"NaN at steps {torch.isnan(got).any(2).any(0).nonzero().flatten().tolist()}"
    kk, vv = k.transpose(0, 1), v.transpose(0, 1)               # (B, T, D)
    assert torch.equal(_as_rows(kc), kk) and torch.equal(_as_rows(vc), vv)      # the cache is k / v, bit for bit
    # row t of causal attention over the whole sequence is step t's result: one batched fp64 evaluation
    qh, kh, vh = (x.transpose(0, 1).double().view(B, T, H, d).transpose(1, 2) for x in (q, k, v))
    s = qh @ kh.transpose(-1, -2) / d ** 0.5
    s = s.masked_fill(torch.ones(T, T, dtype=torch.bool, device="cuda").triu(1), -math.inf)
    want = (torch.softmax(s, -1) @ vh).transpose(1, 2).reshape(B, T, D)
    # rel_err's definition (max|a-b| / max|b|) per step, i.e. per call of the kernel, in one evaluation
    err = (got.double() - want).abs().amax((0, 2)) / want.abs().amax((0, 2))
    worst = int(err.argmax())
    print(f"d={d} {layout}: worst step Sk={worst + 1} rel_err {float(err[worst]):.2e}")
    assert float(err[worst]) < TOL, f"Sk = {worst + 1} (P = {P}): rel_err {float(err[worst]):.2e}"
    assert rel_err(got, want) < TOL


# ---- 2. every form at the edge lengths ------------------------------------------------------------------------

def _edge_lengths(d):
    P = _pass(d)
    return sorted({1, 2, 63, 64, 65, P - 1, P, P + 1, 2 * P})


@pytest.mark.parametrize("d", DIMS)
def test_forms_at_edge_lengths(d):
    """Read-only (host and device length, both layouts, a strided batch view), append (both layouts: the cache
    changes in row L alone), o_mul per sequence and shared, and window_attention with and without a pad row, at
    Sk in {1, 2, 63, 64, 65, P-1, P, P+1, 2P}, on one random cache whose rows from Sk on hold NaN."""
    from qarig import ops
    H, P = _heads(d), _pass(d)
    D, Lmax = H * d, 2 * _pass(d) + 2
    q = _randn(B, D, seed=200 * d)
    k, v = _randn(B, 2 * P, D, seed=200 * d + 1), _randn(B, 2 * P, D, seed=200 * d + 2)
    mul = _randn(B, D, seed=200 * d + 3)
    mul0 = mul[0].contiguous()
    for Sk in _edge_lengths(d):
        L = Sk - 1
        want = _ref(q, k[:, :Sk], v[:, :Sk], H)
        k_new, v_new = k[:, L].contiguous(), v[:, L].contiguous()
        ln = _len_dev(Sk)
        ro = {}
        for layout in LAYOUTS:
            tag = f"d={d} Sk={Sk} {layout}"
            kc, vc = _alloc(B, Lmax, H, d, layout, NAN), _alloc(B, Lmax, H, d, layout, NAN)
            _put(kc, Sk, k), _put(vc, Sk, v)
            k0, v0 = kc.clone(), vc.clone()
            # read-only: host length, device length (the host one is then ignored), the output factor
            ro[layout] = ops.attention_decode(q, None, None, kc, vc, Sk, H)
            assert rel_err(ro[layout], want) < TOL, tag
            assert rel_err(ops.attention_decode(q, None, None, kc, vc, 0, H, len_dev=ln), want) < TOL, tag
            assert rel_err(ops.attention_decode(q, None, None, kc, vc, Sk, H, o_mul=mul), want * mul) < TOL, tag
            assert rel_err(ops.attention_decode(q, None, None, kc, vc, Sk, H, o_mul=mul0), want * mul0) < TOL, tag
            assert _same_bits(kc, k0) and _same_bits(vc, v0), tag + ": a read-only call wrote to the cache"
            # a strided batch view: the sequences in between hold NaN throughout
            kw, vw = _alloc(2 * B - 1, Lmax, H, d, layout, NAN), _alloc(2 * B - 1, Lmax, H, d, layout, NAN)
            kw[::2], vw[::2] = kc, vc
            assert rel_err(ops.attention_decode(q, None, None, kw[::2], vw[::2], Sk, H), want) < TOL, tag
            assert rel_err(ops.attention_decode(q, None, None, kw[::2], vw[::2], 0, H, len_dev=ln), want) < TOL, tag
            # append: slot L holds stale NaN, the new row comes from k_new / v_new
            for om, factor in ((None, 1.0), (mul, mul), (mul0, mul0)):
                kc, vc = _alloc(B, Lmax, H, d, layout, NAN), _alloc(B, Lmax, H, d, layout, NAN)
                _put(kc, L, k), _put(vc, L, v)
                k0, v0 = _as_rows(kc), _as_rows(vc)
                got = ops.attention_decode(q, k_new, v_new, kc, vc, L, H, o_mul=om)
                assert rel_err(got, want * factor) < TOL, tag
                for c, c0, new in ((_as_rows(kc), k0, k_new), (_as_rows(vc), v0, v_new)):
                    changed = (_bits(c) != _bits(c0)).any(2)        # (B, Lmax): rows with any bit changed
                    assert changed[:, L].all() and int(changed.sum()) == B, tag + ": rows other than L changed"
                    assert torch.equal(c[:, L], new), tag
        assert _same_bits(ro["row_major"], ro["head_major"])        # a layout is addressing only
        # the slid window's attention is the same kernel, read-only and row-major: the same bits
        for rows in (Sk, Sk + 1):
            kwin, vwin = torch.empty(B, rows, D, device="cuda"), torch.empty(B, rows, D, device="cuda")
            kwin[:, :Sk], vwin[:, :Sk] = k[:, :Sk], v[:, :Sk]
            kwin[:, Sk:], vwin[:, Sk:] = 1e4, NAN                   # the pad row
            assert _same_bits(ops.window_attention(q, kwin, vwin, Sk, H), ro["row_major"]), f"d={d} Sk={Sk} rows={rows}"
            gotm = ops.window_attention(q, kwin, vwin, Sk, H, o_mul=mul)
            assert rel_err(gotm, want * mul) < TOL, f"d={d} Sk={Sk} rows={rows}"


# ---- 3. one dominant key ------------------------------------------------------------------------------------

def _fma(a, b, c):
    """fp32 fused multiply-add on the CPU: the fp64 product of two fp32 numbers is exact."""
    return (a.double() * b.double() + c.double()).float()


def _kernel_restated_fp32(q, k, v, H):
    """decode_attention_kernel's arithmetic in fp32 torch on the CPU: the fmaf chain of q.k, base-2 scores
    t = dot * (log2(e) / sqrt(d)), lane = key % 64 with a running (m, l, o) over its keys in key order, then the
    wave's maximum and the sums of l and o scaled by 2^(m - M).  (The wave sums run in torch's order, not the
    butterfly's.)  What this misses against fp64 is what fp32 can give for the inputs, whatever the kernel does."""
    n, D = q.shape
    d, S = D // H, k.shape[1]
    c2 = torch.tensor(1.4426950408889634, dtype=torch.float32) / torch.tensor(d ** 0.5, dtype=torch.float32)
    steps = -(-S // 64)
    pad = lambda x: torch.cat((x, x.new_zeros(n, steps * 64 - S, D)), 1).view(n, steps, 64, H, d).permute(0, 3, 1, 2, 4)
    kh, vh = pad(k), pad(v)                             # (n, H, steps, 64, d)
    qh = q.view(n, H, 1, 1, d)
    dot = torch.zeros(n, H, steps, 64)
    for c in range(d):
        dot = _fma(qh[..., c], kh[..., c], dot)
    t = dot * c2
    valid = (torch.arange(steps)[:, None] * 64 + torch.arange(64)[None]) < S
    m, l, ov = torch.full((n, H, 64), -math.inf), torch.zeros(n, H, 64), torch.zeros(n, H, 64, d)
    for s in range(steps):
        mn = torch.maximum(m, t[:, :, s])
        alpha, pr = torch.exp2(m - mn), torch.exp2(t[:, :, s] - mn)
        l = torch.where(valid[s], l * alpha + pr, l)
        ov = torch.where(valid[s][:, None], _fma(pr[..., None], vh[:, :, s], ov * alpha[..., None]), ov)
        m = torch.where(valid[s], mn, m)
    sc = torch.where(m == -math.inf, torch.zeros(()), torch.exp2(m - m.amax(-1, keepdim=True)))
    return ((ov * sc[..., None]).sum(2) / (l * sc).sum(2)[..., None]).reshape(n, D)


# k[j] = FACTOR[d] * q.  The issue's factor 3 stands for every head dim: the fp32 restatement above, on the CPU,
# for these very inputs, stays under TOL / 3 = 3.3e-6 against fp64 with room to spare.  Its rel_err at the five
# positions (first, last cached, fresh, first of the second pass, ragged last pass):
#   d =  4: 2.27e-07 1.34e-07 2.06e-07 2.29e-07 2.11e-07
#   d =  8: 5.38e-07 1.48e-07 1.66e-07 3.01e-07 1.72e-07
#   d = 16: 1.92e-07 2.00e-07 1.62e-07 2.81e-07 1.65e-07
#   d = 32: 2.64e-07 1.90e-07 1.97e-07 3.85e-07 2.69e-07
#   d = 64: 1.18e-07 1.92e-07 2.73e-07 1.47e-07 1.18e-07
# test_dominant_key_inputs_are_within_reach_of_fp32 re-checks the condition wherever the suite runs.
FACTOR = {4: 3.0, 8: 3.0, 16: 3.0, 32: 3.0, 64: 3.0}


def _dominant_positions(d):
    P = _pass(d)
    return {"first": 0, "last_cached": P + 5, "fresh": P + 6, "second_pass_first": P, "ragged_last_pass": P + 3}


def _dominant_inputs(d, where):
    """CPU tensors q (B, D), k / v (B, Sk, D) with Sk = P + 7 unit-scale keys, of which key j is FACTOR[d] * q."""
    H, Sk = _heads(d), _pass(d) + 7
    j = _dominant_positions(d)[where]
    g = torch.Generator().manual_seed(300 * d + j)
    q, k, v = (torch.randn(*s, generator=g) for s in ((B, H * d), (B, Sk, H * d), (B, Sk, H * d)))
    k[:, j] = FACTOR[d] * q
    return q, k, v


POSITIONS = ("first", "last_cached", "fresh", "second_pass_first", "ragged_last_pass")


@pytest.mark.parametrize("where", POSITIONS)
@pytest.mark.parametrize("d", DIMS)
def test_dominant_key_inputs_are_within_reach_of_fp32(d, where):
    """The condition on the inputs of the next test, not a measurement of the kernel: runs on the CPU."""
    q, k, v = _dominant_inputs(d, where)
    H = _heads(d)
    want = _ref(q, k, v, H)
    err = rel_err(_kernel_restated_fp32(q, k, v, H), want)
    print(f"d={d} {where}: fp32 restatement rel_err {err:.2e}")
    assert err < TOL / 3


@pytest.mark.parametrize("where", POSITIONS)
@pytest.mark.parametrize("d", DIMS)
def test_one_dominant_key(d, where):
    """One key far above the rest -- the first, the last cached, the appended one, the first of the second
    pass, one inside the ragged last pass: the running-maximum rescale, and a wave combine whose lanes carry very
    different maxima.  Append form, Sk = P + 7, both layouts, stale NaN in slot L and NaN behind it."""
    from qarig import ops
    H, Sk = _heads(d), _pass(d) + 7
    L, Lmax = Sk - 1, Sk + 2
    q, k, v = (x.cuda() for x in _dominant_inputs(d, where))
    want = _ref(q, k, v, H)
    for layout in LAYOUTS:
        kc, vc = _alloc(B, Lmax, H, d, layout, NAN), _alloc(B, Lmax, H, d, layout, NAN)
        _put(kc, L, k), _put(vc, L, v)
        got = ops.attention_decode(q, k[:, L].contiguous(), v[:, L].contiguous(), kc, vc, L, H)
        err = rel_err(got, want)
        print(f"d={d} {where} {layout}: rel_err {err:.2e}")
        assert err < TOL, layout
        assert rel_err(ops.attention_decode(q, None, None, kc, vc, Sk, H), want) < TOL, layout   # read back


# ---- 4. a device length out of range ------------------------------------------------------------------------

SENTINEL = 777.0


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("d", DIMS)
def test_device_length_out_of_range_is_clamped(d, layout):
    """ctl[0] is clamped to [0, max_len - 1] when appending and to [0, max_len] when read-only.  The cache is the
    first max_len rows of a larger allocation whose other rows hold a sentinel: a wrong clamp lands there."""
    from qarig import ops
    H, extra = _heads(d), 4
    D, Lmax = H * d, _pass(d) + 5
    q = _randn(B, D, seed=400 * d)
    k, v = _randn(B, Lmax, D, seed=400 * d + 1), _randn(B, Lmax, D, seed=400 * d + 2)
    k_new, v_new = _randn(B, D, seed=400 * d + 3), _randn(B, D, seed=400 * d + 4)

    def caches():
        big = [_alloc(B, Lmax + extra, H, d, layout, SENTINEL) for _ in range(2)]
        views = [x[:, :Lmax] if layout == "row_major" else x[:, :, :Lmax] for x in big]
        _put(views[0], Lmax, k), _put(views[1], Lmax, v)
        return big, views

    def guard_intact(big):
        return all(bool(((x[:, Lmax:] if layout == "row_major" else x[:, :, Lmax:]) == SENTINEL).all()) for x in big)

    # read-only, len_dev = max_len + 5: every row of the cache, no row behind it
    big, (kc, vc) = caches()
    k0, v0 = kc.clone(), vc.clone()
    got = ops.attention_decode(q, None, None, kc, vc, 0, H, len_dev=_len_dev(Lmax + 5))
    assert rel_err(got, _ref(q, k, v, H)) < TOL
    assert _same_bits(got, ops.attention_decode(q, None, None, kc, vc, Lmax, H))
    assert guard_intact(big) and _same_bits(kc, k0) and _same_bits(vc, v0)
    # read-only, len_dev = -3: as len_dev = 0 (no key: the host refuses that length, the result is not defined)
    a = ops.attention_decode(q, None, None, kc, vc, 0, H, len_dev=_len_dev(-3))
    b = ops.attention_decode(q, None, None, kc, vc, 0, H, len_dev=_len_dev(0))
    assert torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(a.nan_to_num(), b.nan_to_num())
    assert guard_intact(big) and _same_bits(kc, k0) and _same_bits(vc, v0)

    # append, len_dev = max_len + 5: the new row lands in row max_len - 1 and is the last key
    big, (kc, vc) = caches()
    k0, v0 = _as_rows(kc), _as_rows(vc)
    got = ops.attention_decode(q, k_new, v_new, kc, vc, 0, H, len_dev=_len_dev(Lmax + 5))
    kx, vx = k.clone(), v.clone()
    kx[:, Lmax - 1], vx[:, Lmax - 1] = k_new, v_new
    assert rel_err(got, _ref(q, kx, vx, H)) < TOL
    assert guard_intact(big), "the appended row went behind the cache"
    assert torch.equal(_as_rows(kc), kx) and torch.equal(_as_rows(vc), vx)
    big2, (kc2, vc2) = caches()
    assert _same_bits(got, ops.attention_decode(q, k_new, v_new, kc2, vc2, Lmax - 1, H))

    # append, len_dev = -3: as length 0 -- row 0 is written, the new row is the only key
    big, (kc, vc) = caches()
    got = ops.attention_decode(q, k_new, v_new, kc, vc, 0, H, len_dev=_len_dev(-3))
    kx, vx = k.clone(), v.clone()
    kx[:, 0], vx[:, 0] = k_new, v_new
    assert rel_err(got, v_new) < TOL                    # softmax over one key
    assert guard_intact(big)
    assert torch.equal(_as_rows(kc), kx) and torch.equal(_as_rows(vc), vx)
    big2, (kc2, vc2) = caches()
    assert _same_bits(got, ops.attention_decode(q, k_new, v_new, kc2, vc2, 0, H))
