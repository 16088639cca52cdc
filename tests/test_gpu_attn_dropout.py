"""Attention-probability dropout in the fused attention kernels on an MI355X (csrc/attention.hip, DROP = true).

1. The mask itself, read out exactly from the forward and from the dK/dV pass: with q = 0 every probability is 1 / Sk
   (Sk a power of two) and with p = 0.5 the scale is 2, so with V[j][c] = 2^(j // d) where c == j % d (0 elsewhere)
   o Sk / 2 is the keep bit-field of every (n, h, i); dO built the same way over the queries reads the mask out of dv.
2. o, lse, dq, dk, dv against the fp64 reference of tests/attn_dropout_cases.py on Gaussian inputs, per row, within
   attention_selectors.gaussian_tolerances + 2u (u = 2^-24: the rounding of the kept term and of the s / l product for
   o and dv, of s dPd and the subtraction's operand for dq and dk); lse within the plain tolerance and equal bit for
   bit to the plain entry's.
3. The bf16-product instantiations on selector inputs at p = 0.5 (multiplying by 2 is exact: the selector tolerances).
4. Rows whose visible keys are all dropped: o exactly +0, dq finite and within tolerance.
5. The refusals, and the plain entries' bits before and after a dropout call."""
import ctypes

import numpy as np
import pytest
import torch

import attention_selectors as A
import attn_dropout_cases as AD
import dropout_cases as C

pytestmark = pytest.mark.gpu

T_HALF, S_HALF = 32768, 2.0


@pytest.fixture
def bf16_mode():
    from qarig import ops
    old = ops.PRECISION
    ops.PRECISION = "bf16"
    yield ops
    ops.PRECISION = old


def _key(seed, step, rank):
    def i32(w):
        w &= 0xFFFFFFFF
        return w - (1 << 32) if w >= 1 << 31 else w
    return torch.tensor([i32(seed), i32(seed >> 32), i32(step), i32(rank)], dtype=torch.int32).cuda()


# ---- 1: the mask, read out exactly -------------------------------------------------------------------------------
def _bit_rows(S, d):
    """(S, d) fp32: row r holds 2^(r // d) in column r % d."""
    t = torch.zeros((S, d), dtype=torch.float32)
    r = torch.arange(S)
    t[r, r % d] = torch.pow(torch.tensor(2.0), (r // d).float())
    return t


def _fields(keep, d, axis):
    """keep (N,H,Sq,Sk) -> the integers the read-out must give: the sum over `axis` (3: keys, 2: queries) of
    keep * 2^(index // d), split by index % d -- (N, H, other, d) as float64."""
    keep = torch.from_numpy(keep).double()
    S = keep.shape[axis]
    w = _bit_rows(S, d).double()                       # (S, d)
    return keep @ w if axis == 3 else keep.transpose(2, 3) @ w


def _readout(ops, N, H, d, Sq, Sk, site, step, rank):
    key = _key(AD.SEED, step, rank)
    q = torch.zeros((N, Sq, H * d), dtype=torch.float32).cuda()
    k = torch.randn((N, Sk, H * d), generator=torch.Generator().manual_seed(1)).cuda()
    v = _bit_rows(Sk, d)[None, :, None, :].expand(N, Sk, H, d).reshape(N, Sk, H * d).contiguous().cuda()
    do = _bit_rows(Sq, d)[None, :, None, :].expand(N, Sq, H, d).reshape(N, Sq, H * d).contiguous().cuda()
    drop = (T_HALF, S_HALF, site, key)
    o, lse = ops.attention_fwd(q, k, v, H, False, dropout=drop)
    _, _, dv = ops.attention_bwd(q, k, v, o, do, lse, H, False, dropout=drop)
    return A.to_heads(o, H) * (Sk / 2), A.to_heads(dv, H) * (Sk / 2)


@pytest.mark.parametrize("site,step,rank", [(0, 1, 0), (5, 1, 0), (0, 7, 0), (0, 1, 2)])
@pytest.mark.parametrize("N,H,d,Sq,Sk", AD.READOUT_SHAPES)
@pytest.mark.parametrize("lp", [False, True], ids=["fp32", "lp"])
def test_mask_read_out_of_forward_and_dkv(lp, N, H, d, Sq, Sk, site, step, rank):
    from qarig import ops
    old = ops.PRECISION
    ops.PRECISION = "bf16" if lp else old
    try:
        got_o, got_dv = _readout(ops, N, H, d, Sq, Sk, site, step, rank)
    finally:
        ops.PRECISION = old
    keep = AD.mask(N, H, Sq, Sk, T_HALF, AD.SEED, site, step, rank)
    assert 0.4 < keep.mean() < 0.6
    assert torch.equal(got_o, _fields(keep, d, 3)), "forward: the keep bits differ from the reference mask"
    assert torch.equal(got_dv, _fields(keep, d, 2)), "dK/dV pass: the keep bits differ from the reference mask"


def test_read_out_streams_differ():
    """Two sites, two steps and two ranks draw four different masks (the read-out above is not one mask four times)."""
    masks = [AD.mask(1, 2, 9, 64, T_HALF, AD.SEED, *s) for s in [(0, 1, 0), (5, 1, 0), (0, 7, 0), (0, 1, 2)]]
    for a in range(4):
        for b in range(a + 1, 4):
            assert not np.array_equal(masks[a], masks[b])


# ---- 2 ... 4: against fp64 ----------------------------------------------------------------------------------------
def _run(ops, case, drop):
    q, k, v, do = (A.to_rows(t).cuda() for t in (case.q, case.k, case.v, case.do))
    o, lse = ops.attention_fwd(q, k, v, case.H, case.causal, dropout=drop)
    dq, dk, dv = ops.attention_bwd(q, k, v, o, do, lse, case.H, case.causal, dropout=drop)
    o0, lse0 = ops.attention_fwd(q, k, v, case.H, case.causal)
    got = {n: A.to_heads(t, case.H) for n, t in (("o", o), ("dq", dq), ("dk", dk), ("dv", dv))}
    got["lse"] = lse.double().cpu() * A.LN2
    return got, torch.equal(lse, lse0), o


def _check(case, p, site, step, rank, tol, lp=False):
    from qarig import ops
    t, s = C.threshold_and_scale(p)
    s = float(s)                                                  # the fp32 value the kernel receives
    keep = AD.mask(A.N_BATCH, case.H, case.Sq, case.Sk, t, AD.SEED, site, step, rank)
    ref, scale = AD.reference(case.q, case.k, case.v, case.do, case.causal, keep, s)
    got, lse_same, _ = _run(ops, case, (t, s, site, _key(AD.SEED, step, rank)))
    err = A.row_errors(got, ref, scale, case.floor)
    print(f"{'lp' if lp else 'fp32'} {case.kind} p={p} d={case.d} {case.Sq}x{case.Sk} H={case.H}: " +
          "  ".join(f"{n} {err[n] / A.U:.3g}u (tol {tol[n] / A.U:.4g}u)" for n in err))
    for n, x in got.items():
        assert torch.isfinite(x).all(), f"{n}: non-finite values"
    assert lse_same, "lse differs from the plain entry's"
    for n, e in err.items():
        assert e <= tol[n], f"{n}: worst row {e / A.U:.4g} u, tolerance {tol[n] / A.U:.4g} u"
    # rows whose visible keys are all dropped: o is exactly +0
    visible = torch.ones(case.Sq, case.Sk, dtype=torch.bool)
    if case.causal:
        visible = ~A._mask(case.Sq, case.Sk)
    dead = ~(torch.from_numpy(keep) & visible).any(-1)            # (N, H, Sq)
    rows = got["o"][dead]
    assert torch.equal(rows, torch.zeros_like(rows)) and not torch.signbit(rows).any()
    return int(dead.sum())


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("Sq,Sk,causal,H,d", AD.GAUSSIAN_SHAPES)
def test_gaussian_rows_fp32(Sq, Sk, causal, H, d, p):
    case = A.gaussian_case(Sq, Sk, H, d, causal)
    tol = {n: t + (0 if n == "lse" else 2 * A.U) for n, t in case.tolerances().items()}
    dead = _check(case, p, 3, 5, 1, tol)
    if causal and p == 0.5:
        assert dead > 0          # causal row 0 has one visible key: dropped in about half the (n, h)


@pytest.mark.parametrize("pattern", ["diag", "rand"])
@pytest.mark.parametrize("S", [65, 129])
@pytest.mark.parametrize("d", [8, 16])
def test_selector_rows_bf16_products(bf16_mode, d, S, pattern):
    case = A.selector_case(S, S, 3, d, True, pattern, False)
    _check(case, 0.5, 2, 9, 0, case.tolerances(True), lp=True)


# ---- 5: refusals, and the plain entries untouched ---------------------------------------------------------------
def _raw(case_d=8, H=2, S=16):
    g = torch.Generator().manual_seed(3)
    q, k, v, do = (torch.randn((1, S, H * case_d), generator=g).cuda() for _ in range(4))
    return q, k, v, do


@pytest.mark.parametrize("lp", [False, True], ids=["fp32", "lp"])
def test_refusals_without_a_launch(lp):
    from qarig import _lib
    from qarig.ops import ptr, stream
    lib = _lib.load()
    fwd = lib.qarig_attention_dropout_lp_fwd if lp else lib.qarig_attention_dropout_fwd
    bwd = lib.qarig_attention_dropout_lp_bwd if lp else lib.qarig_attention_dropout_bwd
    key = _key(AD.SEED, 1, 0)
    torch.cuda.synchronize()

    def both(d, H, threshold, site, keyp):
        S = 16
        q, k, v, do = _raw(d, H, S)
        o = torch.full_like(q, 7.0)
        lse = torch.full((1, H, S), 7.0).cuda()
        dq, dk, dv, delta = (torch.full_like(t, 7.0) for t in (q, k, v, lse))
        rf = fwd(ptr(q), ptr(k), ptr(v), 1, S, S, H, d, 1, float(d ** 0.5), ptr(o), ptr(lse), stream(), threshold, 2.0,
                 site, keyp)
        rb = bwd(ptr(q), ptr(k), ptr(v), ptr(o), ptr(do), ptr(lse), 1, S, S, H, d, 1, float(d ** 0.5), ptr(dq),
                 ptr(dk), ptr(dv), ptr(delta), stream(), threshold, 2.0, site, keyp)
        torch.cuda.synchronize()
        untouched = all(bool((t == 7.0).all()) for t in (o, lse, dq, dk, dv, delta))
        return rf, rb, untouched

    assert both(8, 2, T_HALF, 0, ptr(key)) == (0, 0, False)                    # the control: accepted and launched
    for args in ((128, 1, T_HALF, 0, ptr(key)), (8, 2, T_HALF, 256, ptr(key)), (8, 2, 0, 0, ptr(key)), (8, 2, 58983, 0, ptr(key)),
                 (8, 2, T_HALF, 0, ctypes.c_void_p(0))):
        assert both(*args) == (-1, -1, True), args


def test_head_dim_128_message():
    from qarig import ops
    q, k, v, _ = _raw(128, 1, 16)
    with pytest.raises(Exception, match="128"):
        ops.attention_fwd(q, k, v, 1, True, dropout=(T_HALF, S_HALF, 0, _key(1, 1, 0)))


def test_plain_entries_keep_their_bits_around_a_dropout_call():
    from qarig import ops
    case = A.gaussian_case(130, 130, 5, 8, True)
    q, k, v, do = (A.to_rows(t).cuda() for t in (case.q, case.k, case.v, case.do))

    def plain():
        o, lse = ops.attention_fwd(q, k, v, case.H, True)
        return (o, lse, *ops.attention_bwd(q, k, v, o, do, lse, case.H, True))

    before = plain()
    drop = (T_HALF, S_HALF, 1, _key(AD.SEED, 2, 0))
    o, lse = ops.attention_fwd(q, k, v, case.H, True, dropout=drop)
    ops.attention_bwd(q, k, v, o, do, lse, case.H, True, dropout=drop)
    assert not torch.equal(o, before[0])
    after = plain()
    for a, b in zip(before, after):
        assert torch.equal(a, b)
