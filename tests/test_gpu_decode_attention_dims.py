"""decode_attention_grouped_kernel<G, C4> (csrc/decode.hip) -- the cache attention of every head dim that is a
multiple of 4 up to 128 other than 4, 8, 16, 32, 64 -- through ops.attention_decode and ops.window_attention against
fp64 softmax(q k^T / sqrt(d)) v.  A key's channels are shared by a group of 2 or 4 lanes and the head dim arrives at
run time inside a bucket (< 16, < 32, < 64, <= 128): rows are compact, so channels d ... bucket of a head are the next
head's data, the next row's, or nothing at all, and must never be read.

DIMS holds both ends of every bucket and every lane-group width.  P = ops.decode_attention_keys_per_pass(d) keys per
wave and pass.  B = 3 and H = 5 (3 above head dim 64) are no multiples of the 4 heads of a workgroup.
Tolerance: rel_err < 1e-5, the bound test_gpu_decode_attention.py and the kv-cache tests carry for this role."""
import math

import pytest
import torch

from conftest import rel_err

pytestmark = pytest.mark.gpu

DIMS = (12, 20, 28, 36, 48, 60, 68, 96, 124, 128)
SWEEP_DIMS = (12, 48, 96, 128)
LAYOUTS = ("row_major", "head_major")
B = 3
TOL = 1e-5
NAN = float("nan")


def _heads(d):
    return 3 if d > 64 else 5


def _pass(d):
    from qarig import ops
    P = ops.decode_attention_keys_per_pass(d)
    assert P > 0, f"head dim {d} unsupported"
    return P


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


def _first_rows(cache, rows):
    return cache[:, :rows] if cache.dim() == 3 else cache[:, :, :rows]


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


def _inside(rows, D):
    """A contiguous (rows, D) view in the middle of a NaN-filled buffer, and the buffer."""
    big = torch.full((rows + 2, D), NAN, device="cuda")
    return big[1:rows + 1], big


# ---- 1. every length, one appended token at a time ---------------------------------------------------------

@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("d", SWEEP_DIMS)
def test_length_sweep_appending_into_a_nan_cache(d, layout):
    """Sk = 1 .. 2P + 3 by appending token after token, the length in a device word: every pass boundary, groups
    without keys, the stale (NaN) slot the appended row replaces, NaN rows past the length, the cache's last row."""
    from qarig import ops
    H, P = _heads(d), _pass(d)
    D, T = H * d, 2 * P + 3
    q, k, v = (_randn(T, B, D, seed=100 * d + i) for i in range(3))
    kc, vc = _alloc(B, T, H, d, layout, NAN), _alloc(B, T, H, d, layout, NAN)
    ln = _len_dev(0)
    outs = []
    written = torch.zeros((2, T, B, T), dtype=torch.bool, device="cuda")    # (k|v, step, sequence, row) changed
    for t in range(T):                      # nothing is read back inside the loop
        ln.fill_(t)
        before = (_bits(_as_rows(kc)), _bits(_as_rows(vc)))
        outs.append(ops.attention_decode(q[t], k[t], v[t], kc, vc, 0, H, len_dev=ln))
        for i, c in enumerate((kc, vc)):
            written[i, t] = (_bits(_as_rows(c)) != before[i]).any(2)
    got = torch.stack(outs, 1)              # (B, T, D)
    assert not torch.isnan(got).any(), f"NaN at steps {torch.isnan(got).any(2).any(0).nonzero().flatten().tolist()}"
    # step t writes row t of every head (all of it: the slot held NaN) and nothing else
    only_own = torch.eye(T, dtype=torch.bool, device="cuda")[None, :, None, :].expand_as(written)
    assert torch.equal(written, only_own), "a step wrote outside its own row"
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
    D = H * d
    lengths = _edge_lengths(d)
    Smax = max(lengths)
    Lmax = Smax + 2
    q = _randn(B, D, seed=200 * d)
    k, v = _randn(B, Smax, D, seed=200 * d + 1), _randn(B, Smax, D, seed=200 * d + 2)
    mul = _randn(B, D, seed=200 * d + 3)
    mul0 = mul[0].contiguous()
    for Sk in lengths:
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
            err = rel_err(ro[layout], want)
            print(f"{tag}: read-only rel_err {err:.2e}")
            assert err < TOL, tag
            assert rel_err(ops.attention_decode(q, None, None, kc, vc, 0, H, len_dev=ln), want) < TOL, tag
            assert rel_err(ops.attention_decode(q, None, None, kc, vc, Sk, H, o_mul=mul), want * mul) < TOL, tag
            assert rel_err(ops.attention_decode(q, None, None, kc, vc, Sk, H, o_mul=mul0), want * mul0) < TOL, tag
            assert _same_bits(kc, k0) and _same_bits(vc, v0), tag + ": a read-only call wrote to the cache"
            # a strided batch view: the sequences in between hold NaN throughout
            kw, vw = _alloc(2 * B - 1, Lmax, H, d, layout, NAN), _alloc(2 * B - 1, Lmax, H, d, layout, NAN)
            kw[::2], vw[::2] = kc, vc
            assert rel_err(ops.attention_decode(q, None, None, kw[::2], vw[::2], Sk, H), want) < TOL, tag
            assert rel_err(ops.attention_decode(q, None, None, kw[::2], vw[::2], 0, H, len_dev=ln), want) < TOL, tag
            # append: slot L holds stale NaN, the new row comes from k_new / v_new; host and device length
            for om, factor in ((None, 1.0), (mul, mul), (mul0, mul0)):
                for dev_len in (False, True):
                    kc, vc = _alloc(B, Lmax, H, d, layout, NAN), _alloc(B, Lmax, H, d, layout, NAN)
                    _put(kc, L, k), _put(vc, L, v)
                    k0, v0 = _as_rows(kc), _as_rows(vc)
                    if dev_len:
                        got = ops.attention_decode(q, k_new, v_new, kc, vc, 0, H, len_dev=_len_dev(L), o_mul=om)
                    else:
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


# ---- 3. what lies next to the operands -----------------------------------------------------------------------

@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("d", DIMS)
def test_neighbours_of_the_operands_never_reach_the_result(d, layout):
    """q, k_new, v_new, o_mul, o and the caches are views inside larger buffers whose other elements hold NaN, and
    the cache is full (Sk = max_len): the channels d ... bucket of the last head of the last row lie behind the
    view.  (The row-major layout fixes the row stride at H * d, so an unused NaN head cannot sit between the rows:
    what follows the last row -- and, between two sequences, the batch stride's slack -- is poisoned instead; in
    the head-major layout a head's rows are followed by a NaN row before the next head begins.)  A kernel that
    loads a whole bucket reads NaN here, or the next head's finite data elsewhere, and misses the tolerance."""
    from qarig import ops
    H, P = _heads(d), _pass(d)
    D = H * d
    for Sk in (5, P + 3):
        L = Sk - 1
        qs, ks, vs, ms = (_randn(B, D, seed=500 * d + Sk + i) for i in range(4))
        k, v = _randn(B, Sk, D, seed=500 * d + Sk + 4), _randn(B, Sk, D, seed=500 * d + Sk + 5)
        k[:, L], v[:, L] = ks, vs
        want = _ref(qs, k, v, H)
        (q, _), (k_new, _), (v_new, _), (mul, _) = (_inside(B, D) for _ in range(4))
        q.copy_(qs), k_new.copy_(ks), v_new.copy_(vs), mul.copy_(ms)
        out, out_big = _inside(B, D)
        out_before = _bits(out_big).clone()

        def caches(rows_filled):
            """max_len = Sk rows inside Sk + 1 allocated (+ 1 slack sequence): everything else NaN."""
            big = [_alloc(B + 1, Sk + 1, H, d, layout, NAN) for _ in range(2)]
            views = [_first_rows(x[:B], Sk) for x in big]
            _put(views[0], rows_filled, k), _put(views[1], rows_filled, v)
            return big, views

        def outside(big):
            """Bits of everything that is not one of the cache's max_len rows."""
            return [torch.cat((_bits(x[B:]).flatten(),
                               _bits(x[:B, Sk:] if layout == "row_major" else x[:B, :, Sk:]).flatten())) for x in big]

        tag = f"d={d} Sk={Sk} {layout}"
        big, (kc, vc) = caches(Sk)
        guard = outside(big)
        got = ops.attention_decode(q, None, None, kc, vc, Sk, H, o_mul=mul, out=out)
        assert got.data_ptr() == out.data_ptr()
        assert torch.isfinite(out).all(), tag + ": read-only"
        err = rel_err(out, want * ms)
        print(f"{tag}: read-only rel_err {err:.2e}")
        assert err < TOL, tag
        assert all(torch.equal(a, b) for a, b in zip(outside(big), guard)), tag + ": wrote outside the cache"
        big, (kc, vc) = caches(L)
        out.fill_(NAN)
        ops.attention_decode(q, k_new, v_new, kc, vc, L, H, o_mul=mul, out=out)
        assert torch.isfinite(out).all(), tag + ": append"
        assert rel_err(out, want * ms) < TOL, tag
        assert all(torch.equal(a, b) for a, b in zip(outside(big), guard)), tag + ": wrote outside the cache"
        assert torch.equal(_as_rows(kc), k) and torch.equal(_as_rows(vc), v), tag
        # the result went to its B rows alone
        after = _bits(out_big)
        assert torch.equal(after[0], out_before[0]) and torch.equal(after[-1], out_before[-1]), tag
        if layout == "row_major":           # the slid window: token-major rows, a NaN pad row behind the keys
            kwin = torch.full((B + 1, Sk + 1, D), NAN, device="cuda")
            vwin = torch.full((B + 1, Sk + 1, D), NAN, device="cuda")
            kwin[:B, :Sk], vwin[:B, :Sk] = k, v
            out.fill_(NAN)
            ops.window_attention(q, kwin[:B], vwin[:B], Sk, H, o_mul=mul, out=out)
            assert torch.isfinite(out).all() and rel_err(out, want * ms) < TOL, tag + ": window"


# ---- 4. a device length out of range ------------------------------------------------------------------------

SENTINEL = 777.0


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("d", DIMS)
def test_device_length_out_of_range_is_clamped(d, layout):
    """ctl[0] is clamped to [0, max_len - 1] when appending and to [0, max_len] when read-only.  The cache is the
    first max_len rows of a larger allocation whose other rows are a guard band: a wrong clamp lands there."""
    from qarig import ops
    H, extra = _heads(d), 4
    D, Lmax = H * d, _pass(d) + 5
    q = _randn(B, D, seed=400 * d)
    k, v = _randn(B, Lmax, D, seed=400 * d + 1), _randn(B, Lmax, D, seed=400 * d + 2)
    k_new, v_new = _randn(B, D, seed=400 * d + 3), _randn(B, D, seed=400 * d + 4)

    def caches():
        big = [_alloc(B, Lmax + extra, H, d, layout, SENTINEL) for _ in range(2)]
        views = [_first_rows(x, Lmax) for x in big]
        _put(views[0], Lmax, k), _put(views[1], Lmax, v)
        return big, views

    band = _bits(torch.full((1,), SENTINEL, device="cuda"))

    def guard_intact(big):
        """The guard band, bit for bit."""
        return all(bool((_bits(x[:, Lmax:] if layout == "row_major" else x[:, :, Lmax:]) == band).all()) for x in big)

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


# ---- 5. the same bits on every run ---------------------------------------------------------------------------

@pytest.mark.parametrize("d", DIMS)
def test_two_launches_give_the_same_bits(d):
    """The combine over the wave runs in a fixed order, without atomics."""
    from qarig import ops
    H, P = _heads(d), _pass(d)
    D, Sk = H * d, 2 * P + 3
    q = _randn(B, D, seed=600 * d)
    k, v = _randn(B, Sk, D, seed=600 * d + 1), _randn(B, Sk, D, seed=600 * d + 2)
    mul = _randn(B, D, seed=600 * d + 3)
    for layout in LAYOUTS:
        kc, vc = _alloc(B, Sk, H, d, layout, NAN), _alloc(B, Sk, H, d, layout, NAN)
        _put(kc, Sk, k), _put(vc, Sk, v)
        a = ops.attention_decode(q, None, None, kc, vc, Sk, H, o_mul=mul)
        b = ops.attention_decode(q, None, None, kc, vc, Sk, H, o_mul=mul)
        assert _same_bits(a, b), layout
        k_new, v_new = k[:, Sk - 1].contiguous(), v[:, Sk - 1].contiguous()
        c = ops.attention_decode(q, k_new, v_new, kc, vc, Sk - 1, H, o_mul=mul)
        e = ops.attention_decode(q, k_new, v_new, kc, vc, Sk - 1, H, o_mul=mul)
        assert _same_bits(c, e), layout
        assert rel_err(c, _ref(q, k, v, H) * mul) < TOL
