"""Reduced-precision (bf16) forms of the Linear building blocks -- BASELINE config 5's
"bf16 MFMA attn/FFN" mode; opt-in (qarig.ops.set_precision("bf16")), never the fp32 parity path.

What changes against qarig.functional's fp32 nodes (same math, same parameters, same gradients
up to bf16 rounding of the GEMM operands):
 * every GEMM runs on csrc/gemm_lp.hip with bf16 operands IN HBM;
 * tensors that only GEMMs read are STORED in bf16 and never exist in fp32: the MLP hidden
   activation h, its pre-activation t1 (read back only for act'), and the hidden gradient dT1 --
   the 2048-wide tensors that dominate the step's HBM traffic.  They are written by the producing
   GEMM's epilogue (Cb / Pb outputs), not by a cast pass;
 * the narrow (512-wide) GEMM inputs that other kernels produce in fp32 (LayerNorm output,
   attention output, incoming gradients) are cast once per node; the cast of an incoming gradient
   also yields the bias gradient (column sums ride on the same pass: qarig_cast_colsum);
 * weights keep fp32 masters; ONE bf16 shadow per weight, as stored (N,K): a view of the flat bf16 image the
   Adam kernel writes beside the fp32 update (optim.FlatAdam.flat_shadow; before the first step, and for weights
   no FlatAdam owns, a cast cached until the next optimiser step): the forward reads it reduction-contiguous,
   the input gradient reduction-major (transposed on the LDS read), so no W^T copy exists;
 * weight gradients are TN products of the row-major bf16 activations as they lie (transposed on
   the LDS read), accumulated in fp32 straight into the parameter's .grad.
"""
import torch

from . import ops
from ._lib import f32c, require_cuda
from .functional import _2d, _grad_slot, _report_done


def _pad128(n):
    return (n + 127) // 128 * 128


def _shadow(w, transpose=False, pad_rows=0):
    """bf16 shadow of a weight (N,K): as stored, or transposed (K,N); optionally zero-padded to
    pad_rows output rows (ragged classifier widths).  Cached until the next optimiser step."""
    if pad_rows and pad_rows != w.shape[0]:
        key = ("p", w.data_ptr(), tuple(w.shape), pad_rows, transpose, w._version, ops.LP_EPOCH)
        hit = None if torch.cuda.is_current_stream_capturing() else ops._lp_get(key, w)
        if hit is not None:
            return hit
        wp = torch.zeros((pad_rows, w.shape[1]), dtype=torch.float32, device=w.device)
        wp[:w.shape[0]].copy_(w.detach())
        out = ops.cast_transpose_bf16(wp) if transpose else ops.cast_bf16(wp)
        if not torch.cuda.is_current_stream_capturing():
            ops._lp_put(key, w, out)
        return out
    if not transpose:
        owner = getattr(w, "_qarig_owner", None)
        if owner is not None and hasattr(owner, "shadow_of"):
            v = owner.shadow_of(w)           # written by the optimiser's own pass (optim.FlatAdam)
            if v is not None:
                return v
    wd = w.detach()
    wd._qarig_weight = True
    wd._qarig_src = w            # the cache entry is tied to the parameter, not to this temporary
    return ops.cast_transpose_bf16(wd, cache=True) if transpose else ops.cast_bf16(wd, cache=True)


def _cast_in(x2, shapes):
    """bf16 copy of a node's fp32 input (backward reads it) and, in "fp8" mode when every forward
    product of the node that reads x ((M, N, K) in `shapes`) fits the e4m3 kernel, its per-tensor
    e4m3 quantisation from the same pass: (xb, (x8, inv_scale) or None)."""
    if ops.PRECISION == "fp8" and all(ops.f8_supported(*s) for s in shapes):
        x8, sx, xb = ops.cast_fp8(x2, want_bf16=True)
        return xb, (x8, sx)
    return ops.cast_bf16(x2), None


def _fwd_nt(xq, xb, w, M, N, K, **epi):
    """The forward product x W^T of a node: bf16 operands, or -- with xq from _cast_in -- x and W
    quantised per tensor (W once per optimiser step) and multiplied on the fp8 MFMA.  Backward is
    the bf16 one either way."""
    if xq is not None:
        wd = w.detach()
        wd._qarig_weight = True
        wd._qarig_src = w
        w8, sw = ops.cast_fp8(wd, cache=True)
        ops.gemm_f8(xq[0], xq[1], w8, sw, M, N, K, **epi)
    else:
        ops.gemm_lp(xb, _shadow(w), 0, M, N, K, **epi)


def _ok(M, N, K):
    return bool(ops._lib.load().qarig_gemm_lp_supported(M, N, K, 1))


def _splitk(tiles, K):
    """K slices for a weight-gradient TN product: fill the chip, whole 64-deep tiles."""
    s = max(1, min(512 // max(1, tiles), K // 512, 32))
    while s > 1 and (K % s or (K // s) % 64):
        s -= 1
    return s


def _grad_into(p, n, Np, alloc, run):
    """The gradient of parameter p from a kernel that writes Np >= n rows (entries) of it:
    run(out, accumulate) launches it.  Accumulated straight into p.grad when that is a FlatAdam slot
    of the kernel's extent, else through a temporary from alloc().  Returns (gradient, or None when
    it went into the slot; what run returned)."""
    slot = _grad_slot(p)
    if slot is not None and Np == n:
        r = run(slot, True)
        _report_done(p)
        return None, r
    tmp = alloc()
    r = run(tmp, False)
    g = tmp[:n]
    if slot is not None:
        slot.add_(g)
        _report_done(p)
        return None, r
    return g, r


def _wgrad_into(w, Np, K, n_rows, device, gemm):
    """dW (n_rows, K) of w from gemm(C, accumulate), which writes (Np, K)."""
    return _grad_into(w, n_rows, Np, lambda: torch.empty((Np, K), dtype=torch.float32, device=device), gemm)[0]


def _wgrad(dTb, xb, w, n_rows):
    """dW (n_rows, K) = dT^T x over the token rows, fp32, accumulated into w.grad when it is a
    FlatAdam slot; dTb (M, Np >= n_rows) and xb (M, K) are the row-major bf16 activations."""
    M, Np = dTb.shape
    K = xb.shape[1]
    sk = _splitk((Np // 128) * (K // 128), M)
    if Np % 256 == 0 and K % 256 == 0:
        # 256 x 256-tile kernel (csrc/gemm_lp.hip: taken from 224 workgroups up): 2048 x 512 outputs
        # over 32768 rows measured 95 us there with 16 slices against 101 us on the 128-tiles with 8
        bt = (Np // 256) * (K // 256)
        s = 1
        while bt * s < 224:
            s *= 2
        if bt >= 16 and M % s == 0 and (M // s) % 64 == 0 and M // s >= 1024:
            sk = s
    return _wgrad_into(w, Np, K, n_rows, xb.device,
                       lambda C, acc: ops.gemm_lp(dTb, xb, 1, Np, K, M, C=C, splitk=sk, accumulate=acc))


def _bias_grad(src, b, n, want_cast):
    """Column sums of src (M, Np) -> bias gradient (first n columns); returns (db or None,
    bf16 copy of src or None)."""
    Np = src.shape[1]
    if b is None:
        return None, (ops.cast_bf16(src) if want_cast else None)
    return _grad_into(b, n, Np, lambda: torch.zeros(Np, dtype=torch.float32, device=src.device),
                      lambda out, acc: ops.cast_colsum(src, out, accumulate=acc, want_cast=want_cast))


def _mlp_lp_fwd(xq, xb, M, K, w1, b1, w2, b2, act1, act2, Np, device):
    """The two forward products of one MLP from x's bf16 copy (or its e4m3 form xq): (y (M, Np)
    fp32, t2 or None, t1b or None, hb)."""
    H, N = w1.shape[0], w2.shape[0]
    hb = torch.empty((M, H), dtype=torch.bfloat16, device=device)
    t1b = torch.empty((M, H), dtype=torch.bfloat16, device=device) if act1 else None
    _fwd_nt(xq, xb, w1, M, H, K, bias=b1, act=act1, Cb=hb, Pb=t1b)
    y = torch.empty((M, Np), dtype=torch.float32, device=device)
    t2 = torch.empty((M, Np), dtype=torch.float32, device=device) if act2 else None
    b2p = b2
    if Np != N and b2 is not None:
        b2p = torch.zeros(Np, dtype=torch.float32, device=device)
        b2p[:N].copy_(b2.detach())
    ops.gemm_lp(hb, _shadow(w2, pad_rows=Np), 0, M, Np, H, C=y, bias=b2p, preact=t2, act=act2)
    return y, t2, t1b, hb


def _mlp_lp_bwd(dT2, w1, b1, w2, b2, t1b, hb, xb, act1, N, Np, need, dx):
    """Backward of one MLP from dT2 (M, Np) fp32; need = needs_input_grad of (x, w1, b1, w2, b2).
    dx: None (no input gradient), or (tensor, accumulate).  Returns (dw1, db1, dw2, db2)."""
    M = dT2.shape[0]
    H, K = w1.shape
    db2, dT2b = _bias_grad(dT2, b2 if need[4] else None, N, True)
    dT1b = torch.empty((M, H), dtype=torch.bfloat16, device=dT2.device)
    ops.gemm_lp(dT2b, _shadow(w2, pad_rows=Np), 2, M, H, Np, gradz=t1b if act1 else None, gact=act1, Cb=dT1b)
    dw2 = _wgrad(dT2b, hb, w2, N) if need[3] else None
    db1, _ = _bias_grad(dT1b, b1 if need[2] else None, H, False)
    if dx is not None:
        ops.gemm_lp(dT1b, _shadow(w1), 2, M, K, H, C=dx[0], accumulate=dx[1])
    dw1 = _wgrad(dT1b, xb, w1, H) if need[1] else None
    return dw1, db1, dw2, db2


class _MLP2LP(torch.autograd.Function):
    """y = act2(act1(x W1^T + b1) W2^T + b2), reduced precision (see module docstring)."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, act1, act2):
        require_cuda(x, w1, w2)
        shp = x.shape
        x2 = _2d(f32c(x))
        M, K = x2.shape
        N = w2.shape[0]
        Np = _pad128(N)
        xb, xq = _cast_in(x2, [(M, w1.shape[0], K)])
        y, t2, t1b, hb = _mlp_lp_fwd(xq, xb, M, K, w1, b1, w2, b2, act1, act2, Np, x2.device)
        ctx.save_for_backward(xb, t1b if t1b is not None else hb, hb, t2 if t2 is not None else hb)
        ctx.cfg = (act1, act2, N, Np, shp)
        ctx.params = (w1, b1, w2, b2)
        if Np != N:
            y = y[:, :N].contiguous()
        return y.reshape(*shp[:-1], N)

    @staticmethod
    def backward(ctx, dy):
        xb, t1b, hb, t2 = ctx.saved_tensors
        act1, act2, N, Np, shp = ctx.cfg
        w1, b1, w2, b2 = ctx.params
        M, K = xb.shape
        dy2 = _2d(f32c(dy))
        if Np != N:
            pad = torch.zeros((M, Np), dtype=torch.float32, device=dy2.device)
            pad[:, :N].copy_(dy2)
            dy2 = pad
        dT2 = ops.act_bwd(dy2, t2, act2) if act2 else dy2
        dx = torch.empty((M, K), dtype=torch.float32, device=dy2.device) if ctx.needs_input_grad[0] else None
        dw1, db1, dw2, db2 = _mlp_lp_bwd(dT2, w1, b1, w2, b2, t1b, hb, xb, act1, N, Np, ctx.needs_input_grad[:5],
                                         (dx, False) if dx is not None else None)
        if dx is not None:
            dx = dx.reshape(shp)
        return dx, dw1, db1, dw2, db2, None, None


class _MLP2x3LP(torch.autograd.Function):
    """The q, k, v MLPs of a self-attention layer on their common input: one bf16 cast of the
    input, the three input gradients accumulated by the GEMM epilogues into one tensor."""

    @staticmethod
    def forward(ctx, x, act1, act2, *params):
        require_cuda(x, *params)
        shp = x.shape
        x2 = _2d(f32c(x))
        M, K = x2.shape
        xb, xq = _cast_in(x2, [(M, params[4 * i].shape[0], K) for i in range(3)])
        outs, saved = [], [xb]
        for i in range(3):
            w1, b1, w2, b2 = params[4 * i:4 * i + 4]
            N = w2.shape[0]
            y, t2, t1b, hb = _mlp_lp_fwd(xq, xb, M, K, w1, b1, w2, b2, act1, act2, N, x2.device)
            outs.append(y.reshape(*shp[:-1], N))
            saved += [t1b if t1b is not None else hb, hb, t2 if t2 is not None else hb]
        ctx.save_for_backward(*saved)
        ctx.cfg = (act1, act2, shp)
        ctx.params = params
        return tuple(outs)

    @staticmethod
    def backward(ctx, *dys):
        saved = ctx.saved_tensors
        act1, act2, shp = ctx.cfg
        xb = saved[0]
        M, K = xb.shape
        grads = []
        dx = None
        for i in range(3):
            w1, b1, w2, b2 = ctx.params[4 * i:4 * i + 4]
            t1b, hb, t2 = saved[1 + 3 * i:4 + 3 * i]
            N = w2.shape[0]
            ni = 3 + 4 * i
            dy2 = _2d(f32c(dys[i]))
            dT2 = ops.act_bwd(dy2, t2, act2) if act2 else dy2
            first = dx is None
            if ctx.needs_input_grad[0] and first:
                dx = torch.empty((M, K), dtype=torch.float32, device=dy2.device)
            need = (ctx.needs_input_grad[0], *ctx.needs_input_grad[ni:ni + 4])
            grads += _mlp_lp_bwd(dT2, w1, b1, w2, b2, t1b, hb, xb, act1, N, N, need,
                                 (dx, not first) if dx is not None else None)
        if dx is not None:
            dx = dx.reshape(shp)
        return (dx, None, None, *grads)


class _LinearActLP(torch.autograd.Function):
    """y = act(x W^T + b [+ residual]), reduced precision."""

    @staticmethod
    def forward(ctx, x, weight, bias, residual, act):
        require_cuda(x, weight)
        shp = x.shape
        x2 = _2d(f32c(x))
        M, K = x2.shape
        N = weight.shape[0]
        xb, xq = _cast_in(x2, [(M, N, K)])
        r2 = _2d(f32c(residual)) if residual is not None else None
        y = torch.empty((M, N), dtype=torch.float32, device=x2.device)
        t = torch.empty((M, N), dtype=torch.float32, device=x2.device) if act else None
        _fwd_nt(xq, xb, weight, M, N, K, C=y, bias=bias, residual=r2, preact=t, act=act)
        ctx.save_for_backward(xb, t if t is not None else xb)
        ctx.cfg = (act, residual is not None, shp)
        ctx.params = (weight, bias)
        return y.reshape(*shp[:-1], N)

    @staticmethod
    def backward(ctx, dy):
        xb, t = ctx.saved_tensors
        act, has_res, shp = ctx.cfg
        weight, bias = ctx.params
        M, K = xb.shape
        N = weight.shape[0]
        dy2 = _2d(f32c(dy))
        dT = ops.act_bwd(dy2, t, act) if act else dy2
        db, dTb = _bias_grad(dT, bias if (bias is not None and ctx.needs_input_grad[2]) else None, N, True)
        dx = dw = dr = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty((M, K), dtype=torch.float32, device=dy2.device)
            ops.gemm_lp(dTb, _shadow(weight), 2, M, K, N, C=dx)
            dx = dx.reshape(shp)
        if ctx.needs_input_grad[1]:
            dw = _wgrad(dTb, xb, weight, N)
        if has_res and ctx.needs_input_grad[3]:
            dr = dT.reshape(dy.shape)
        return dx, dw, db, dr, None


def mlp2_supported(x, w1, w2):
    M = x.numel() // x.shape[-1]
    K, H, N = w1.shape[1], w1.shape[0], w2.shape[0]
    Np = _pad128(N)
    # forward (M,H,K), (M,Np,H); d-input (M,H,Np), (M,K,H); d-weight (Np,H,M), (H,K,M)
    return (ops.lp_mode() and M >= 1024 and _ok(M, H, K) and _ok(M, Np, H) and _ok(M, H, Np)
            and _ok(M, K, H) and _ok(Np, H, M) and _ok(H, K, M))


def linear_supported(x, weight):
    M = x.numel() // x.shape[-1]
    N, K = weight.shape
    return (ops.lp_mode() and M >= 1024 and _ok(M, N, K) and _ok(M, K, N) and _ok(N, K, M))


# ---- "mxfp8": every product on MX-e4m3 operands ---------------------------------------------------
def _mx_splitk(tiles, K):
    """K slices for an MX weight gradient: the bf16 rule (_wgrad), on whole 128-deep tiles."""
    bt = tiles
    s = 1
    while bt * s < 224 and s < 32:
        s *= 2
    while s > 1 and (K % s or (K // s) % 128):
        s -= 1
    return s


def _mx_wgrad(dTt, xt, w, Np, K, n_rows):
    """dW (n_rows, K) = dT^T x from the transposed forms dTt (Np, Mp) and xt (K, Mp), accumulated into
    w.grad when it is a FlatAdam slot."""
    Mp = xt.q.shape[1]
    sk = _mx_splitk((Np // 128) * (K // 128), Mp)
    return _wgrad_into(w, Np, K, n_rows, xt.q.device,
                       lambda C, acc: ops.gemm_mx(dTt, xt, Np, K, Mp, C=C, splitk=sk, accumulate=acc))


def _mx_grad_in(dT, b, n):
    """Row and transposed forms of an incoming gradient dT (M, Np) and, from the same pass, the bias
    gradient (first n columns): (row form, transposed form, db or None)."""
    Np = dT.shape[1]
    if b is None:
        rf, tf = ops.mx_quant(dT, row=True, transposed=True)
        return rf, tf, None
    db, (rf, tf) = _grad_into(b, n, Np, lambda: torch.empty(Np, dtype=torch.float32, device=dT.device),
                              lambda out, acc: ops.mx_quant(dT, row=True, transposed=True, colsum=out, accumulate=acc))
    return rf, tf, db


def _mlp_mx_fwd(xr, M, K, w1, b1, w2, b2, act1, act2, Np, device):
    """The two forward products of one MLP from x's row form: (y (M, Np) fp32, t2 or None, t1b,
    h's transposed form)."""
    H = w1.shape[0]
    w1r, _ = ops.mx_weight(w1)
    w2r, _ = ops.mx_weight(w2, Np)
    hb = torch.empty((M, H), dtype=torch.bfloat16, device=device)
    t1b = torch.empty((M, H), dtype=torch.bfloat16, device=device) if act1 else None
    ops.gemm_mx(xr, w1r, M, H, K, bias=b1, act=act1, Cb=hb, Pb=t1b)
    hr, ht = ops.mx_quant(hb, row=True, transposed=True)
    y = torch.empty((M, Np), dtype=torch.float32, device=device)
    t2 = torch.empty((M, Np), dtype=torch.float32, device=device) if act2 else None
    b2p = b2
    if Np != w2.shape[0] and b2 is not None:
        b2p = torch.zeros(Np, dtype=torch.float32, device=device)
        b2p[:w2.shape[0]].copy_(b2.detach())
    ops.gemm_mx(hr, w2r, M, Np, H, C=y, bias=b2p, preact=t2, act=act2)
    return y, t2, t1b, ht


def _mlp_mx_bwd(dT2, w1, b1, w2, b2, t1b, ht, xt, act1, N, Np, need, dx):
    """Backward of one MLP from dT2 (M, Np) fp32; need = needs_input_grad of (x, w1, b1, w2, b2).
    dx: None (no input gradient), or (tensor, accumulate).  Returns (dw1, db1, dw2, db2)."""
    M = dT2.shape[0]
    H, K = w1.shape
    d2r, d2t, db2 = _mx_grad_in(dT2, b2 if need[4] else None, N)
    _, w2t = ops.mx_weight(w2, Np)
    dT1b = torch.empty((M, H), dtype=torch.bfloat16, device=dT2.device)
    ops.gemm_mx(d2r, w2t, M, H, Np, gradz=t1b if act1 else None, gact=act1, Cb=dT1b)
    dw2 = _mx_wgrad(d2t, ht, w2, Np, H, N) if need[3] else None
    del d2r, d2t
    d1r, d1t, db1 = _mx_grad_in(dT1b, b1 if need[2] else None, H)
    if dx is not None:
        _, w1t = ops.mx_weight(w1)
        ops.gemm_mx(d1r, w1t, M, K, H, C=dx[0], accumulate=dx[1])
    dw1 = _mx_wgrad(d1t, xt, w1, H, K, H) if need[1] else None
    return dw1, db1, dw2, db2


class _MLP2MX(torch.autograd.Function):
    """y = act2(act1(x W1^T + b1) W2^T + b2), all six products on MX-e4m3 operands."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, act1, act2):
        require_cuda(x, w1, w2)
        shp = x.shape
        x2 = _2d(f32c(x))
        M, K = x2.shape
        N = w2.shape[0]
        Np = _pad128(N)
        xr, xt = ops.mx_quant(x2, row=True, transposed=True)
        y, t2, t1b, ht = _mlp_mx_fwd(xr, M, K, w1, b1, w2, b2, act1, act2, Np, x2.device)
        ctx.save_for_backward(xt.q, xt.s, ht.q, ht.s, t1b if t1b is not None else ht.q,
                              t2 if t2 is not None else ht.q)
        ctx.cfg = (act1, act2, N, Np, shp)
        ctx.params = (w1, b1, w2, b2)
        if Np != N:
            y = y[:, :N].contiguous()
        return y.reshape(*shp[:-1], N)

    @staticmethod
    def backward(ctx, dy):
        xq, xs, hq, hs, t1b, t2 = ctx.saved_tensors
        act1, act2, N, Np, shp = ctx.cfg
        w1, b1, w2, b2 = ctx.params
        dy2 = _2d(f32c(dy))
        M = dy2.shape[0]
        if Np != N:
            pad = torch.zeros((M, Np), dtype=torch.float32, device=dy2.device)
            pad[:, :N].copy_(dy2)
            dy2 = pad
        dT2 = ops.act_bwd(dy2, t2, act2) if act2 else dy2
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty((M, w1.shape[1]), dtype=torch.float32, device=dy2.device)
        need = [ctx.needs_input_grad[i] for i in range(5)]
        dw1, db1, dw2, db2 = _mlp_mx_bwd(dT2, w1, b1, w2, b2, t1b if act1 else None, ops.MxOperand(hq, hs),
                                         ops.MxOperand(xq, xs), act1, N, Np, need,
                                         (dx, False) if dx is not None else None)
        if dx is not None:
            dx = dx.reshape(shp)
        return dx, dw1, db1, dw2, db2, None, None


class _MLP2x3MX(torch.autograd.Function):
    """The q, k, v MLPs on their common input in "mxfp8": one quantisation of the input, the three
    input gradients accumulated by the GEMM epilogues into one tensor."""

    @staticmethod
    def forward(ctx, x, act1, act2, *params):
        require_cuda(x, *params)
        shp = x.shape
        x2 = _2d(f32c(x))
        M, K = x2.shape
        xr, xt = ops.mx_quant(x2, row=True, transposed=True)
        outs, saved = [], [xt.q, xt.s]
        for i in range(3):
            w1, b1, w2, b2 = params[4 * i:4 * i + 4]
            N = w2.shape[0]
            y, t2, t1b, ht = _mlp_mx_fwd(xr, M, K, w1, b1, w2, b2, act1, act2, N, x2.device)
            outs.append(y.reshape(*shp[:-1], N))
            saved += [ht.q, ht.s, t1b if t1b is not None else ht.q, t2 if t2 is not None else ht.q]
        ctx.save_for_backward(*saved)
        ctx.cfg = (act1, act2, shp)
        ctx.params = params
        return tuple(outs)

    @staticmethod
    def backward(ctx, *dys):
        saved = ctx.saved_tensors
        act1, act2, shp = ctx.cfg
        xt = ops.MxOperand(saved[0], saved[1])
        K = ctx.params[0].shape[1]
        grads = []
        dx = None
        for i in range(3):
            w1, b1, w2, b2 = ctx.params[4 * i:4 * i + 4]
            hq, hs, t1b, t2 = saved[2 + 4 * i:6 + 4 * i]
            N = w2.shape[0]
            ni = 3 + 4 * i
            dy2 = _2d(f32c(dys[i]))
            M = dy2.shape[0]
            dT2 = ops.act_bwd(dy2, t2, act2) if act2 else dy2
            dxa = None
            if ctx.needs_input_grad[0]:
                first = dx is None
                if first:
                    dx = torch.empty((M, K), dtype=torch.float32, device=dy2.device)
                dxa = (dx, not first)
            need = [ctx.needs_input_grad[0]] + [ctx.needs_input_grad[ni + j] for j in range(4)]
            grads += list(_mlp_mx_bwd(dT2, w1, b1, w2, b2, t1b if act1 else None, ops.MxOperand(hq, hs), xt,
                                      act1, N, N, need, dxa))
        if dx is not None:
            dx = dx.reshape(shp)
        return (dx, None, None, *grads)


class _LinearActMX(torch.autograd.Function):
    """y = act(x W^T + b [+ residual]), the three products on MX-e4m3 operands."""

    @staticmethod
    def forward(ctx, x, weight, bias, residual, act):
        require_cuda(x, weight)
        shp = x.shape
        x2 = _2d(f32c(x))
        M, K = x2.shape
        N = weight.shape[0]
        xr, xt = ops.mx_quant(x2, row=True, transposed=True)
        wr, _ = ops.mx_weight(weight)
        r2 = _2d(f32c(residual)) if residual is not None else None
        y = torch.empty((M, N), dtype=torch.float32, device=x2.device)
        t = torch.empty((M, N), dtype=torch.float32, device=x2.device) if act else None
        ops.gemm_mx(xr, wr, M, N, K, C=y, bias=bias, residual=r2, preact=t, act=act)
        ctx.save_for_backward(xt.q, xt.s, t if t is not None else xt.q)
        ctx.cfg = (act, residual is not None, shp)
        ctx.params = (weight, bias)
        return y.reshape(*shp[:-1], N)

    @staticmethod
    def backward(ctx, dy):
        xq, xs, t = ctx.saved_tensors
        act, has_res, shp = ctx.cfg
        weight, bias = ctx.params
        N, K = weight.shape
        dy2 = _2d(f32c(dy))
        M = dy2.shape[0]
        dT = ops.act_bwd(dy2, t, act) if act else dy2
        dr_, dt_, db = _mx_grad_in(dT, bias if (bias is not None and ctx.needs_input_grad[2]) else None, N)
        dx = dw = dr = None
        if ctx.needs_input_grad[0]:
            _, wt = ops.mx_weight(weight)
            dx = torch.empty((M, K), dtype=torch.float32, device=dy2.device)
            ops.gemm_mx(dr_, wt, M, K, N, C=dx)
            dx = dx.reshape(shp)
        if ctx.needs_input_grad[1]:
            dw = _mx_wgrad(dt_, ops.MxOperand(xq, xs), weight, N, K, N)
        if has_res and ctx.needs_input_grad[3]:
            dr = dT.reshape(dy.shape)
        return dx, dw, db, dr, None


def _mx(M, N, K):
    return ops.mx_supported(M, N, K, 1)


def _mlp_mx_ok(M, K, H, N):
    """Every product of an MLP node on the MX kernel (quantised tensors need 128-multiple widths)."""
    Np, Mp = _pad128(N), _pad128(M)
    return (_mx(M, H, K) and _mx(M, Np, H) and _mx(M, H, Np) and _mx(M, K, H) and _mx(Np, H, Mp)
            and _mx(H, K, Mp))


def mlp2_node(x, w1, b1, w2, b2, act1, act2):
    """The reduced-precision MLP node of the current mode (callers checked mlp2_supported)."""
    M = x.numel() // x.shape[-1]
    if ops.PRECISION == "mxfp8" and _mlp_mx_ok(M, w1.shape[1], w1.shape[0], w2.shape[0]):
        return _MLP2MX.apply(x, w1, b1, w2, b2, act1, act2)
    return _MLP2LP.apply(x, w1, b1, w2, b2, act1, act2)


def mlp2x3_node(x, act1, act2, flat_params):
    M = x.numel() // x.shape[-1]
    if ops.PRECISION == "mxfp8" and all(
            _mlp_mx_ok(M, flat_params[4 * i].shape[1], flat_params[4 * i].shape[0], flat_params[4 * i + 2].shape[0])
            and flat_params[4 * i + 2].shape[0] % 128 == 0 for i in range(3)):
        return _MLP2x3MX.apply(x, act1, act2, *flat_params)
    return _MLP2x3LP.apply(x, act1, act2, *flat_params)


def linear_node(x, weight, bias, residual, act):
    M = x.numel() // x.shape[-1]
    N, K = weight.shape
    if ops.PRECISION == "mxfp8" and _mx(M, N, K) and _mx(M, K, N) and _mx(N, K, _pad128(M)):
        return _LinearActMX.apply(x, weight, bias, residual, act)
    return _LinearActLP.apply(x, weight, bias, residual, act)
