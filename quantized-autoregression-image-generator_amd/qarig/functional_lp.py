"""Reduced-precision forms of the Linear building blocks -- BASELINE config 5's "bf16 MFMA attn/FFN" mode and
what was built on it; opt-in (qarig.ops.set_precision("bf16" / "fp8" / "mxfp8")), never the fp32 parity path.

Two node shells, one backend per number format.

The shells are the part of an autograd node that no number format changes, written once:
 * the MLP shell (_mlp_forward / _mlp_backward): n two-layer MLPs on a common input.  It owns the 2-D reshape,
   the zero-padding of a ragged incoming gradient to the padded width, act2', the slice of needs_input_grad that
   belongs to each block, the rule "the first block writes dx, later blocks accumulate into it", and the slice
   and reshape of the outputs.  n = 1 with ragged widths padded to 128 is the single MLP (FFN, classifier);
   n = 3 at the widths as they are is the q, k, v MLPs of a self-attention layer;
 * the Linear shell (_linear_forward / _linear_backward): y = act(x W^T + b [+ residual]);
 * one backward of an MLP (_mlp_bwd) and of a Linear in terms of three products a backend supplies.

A backend (_BF16, _MX: a namespace of functions, no instances) says
 * prepare: how the node's fp32 input is turned into what the forward products read and what backward keeps;
 * nt / mlp_fwd: the forward product of a Linear, the two forward products of one MLP;
 * grad_in / dgrad / wgrad: an incoming gradient in the form the gradient products read, with the bias gradient
   from the same pass; the input-gradient product; the weight-gradient product;
 * pack / unpack: a kept operand as the tensors save_for_backward takes, and back.
The six node classes (_MLP2LP, _MLP2x3LP, _LinearActLP, _MLP2MX, _MLP2x3MX, _LinearActMX) bind a shell to a
backend (_mlp2_class, _mlp2x3_class, _linear_class); mlp2_node / mlp2x3_node / linear_node pick the class.

What changes against qarig.functional's fp32 nodes (same math, same parameters, same gradients
up to the rounding of the GEMM operands), in the bf16 backend:
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
   the LDS read), accumulated in fp32 straight into the parameter's .grad;
 * in "fp8" mode the forward products that read the node's input take it, and the weight, quantised per tensor
   to e4m3 where the e4m3 kernel takes their shapes; backward is the bf16 one either way.
The MX backend ("mxfp8") runs every product -- forward and both gradients -- on block-scaled MX-e4m3 operands:
each tensor is quantised once, in the row and the transposed form its products read, h and dT1 stay bf16.
"""
import torch

from . import ops
from ._lib import f32c, require_cuda
from .functional import _2d, _grad_slot, _report_done


def _pad128(n):
    return (n + 127) // 128 * 128


def _as_weight(w):
    """A detached alias of parameter w that qarig.ops treats as a weight: its images are cached, and the cache
    entry is tied to the parameter, not to this temporary."""
    wd = w.detach()
    wd._qarig_weight = True
    wd._qarig_src = w
    return wd


def _shadow(w, transpose=False, pad_rows=0):
    """bf16 shadow of a weight (N,K): as stored, or transposed (K,N); optionally zero-padded to
    pad_rows output rows (ragged classifier widths).  Cached until the next optimiser step."""
    if pad_rows and pad_rows != w.shape[0]:
        def padded():
            wp = torch.zeros((pad_rows, w.shape[1]), dtype=torch.float32, device=w.device)
            wp[:w.shape[0]].copy_(w.detach())
            return ops.cast_transpose_bf16(wp) if transpose else ops.cast_bf16(wp)
        return ops._lp_image("p", w, padded, extras=(pad_rows, transpose))
    if not transpose:
        owner = getattr(w, "_qarig_owner", None)
        if owner is not None and hasattr(owner, "shadow_of"):
            v = owner.shadow_of(w)           # written by the optimiser's own pass (optim.FlatAdam)
            if v is not None:
                return v
    wd = _as_weight(w)
    return ops.cast_transpose_bf16(wd, cache=True) if transpose else ops.cast_bf16(wd, cache=True)


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


def _mx_splitk(tiles, K):
    """K slices for an MX weight gradient: the bf16 rule (_BF16.wgrad), on whole 128-deep tiles."""
    bt = tiles
    s = 1
    while bt * s < 224 and s < 32:
        s *= 2
    while s > 1 and (K % s or (K // s) % 128):
        s -= 1
    return s


def _hidden_buffers(M, H, act1, device):
    """(h, t1 or None): the bf16 hidden activation and pre-activation the first product's epilogue writes."""
    hb = torch.empty((M, H), dtype=torch.bfloat16, device=device)
    return hb, torch.empty((M, H), dtype=torch.bfloat16, device=device) if act1 else None


def _output_buffers(M, Np, b2, act2, device):
    """(y (M, Np), t2 or None, b2 zero-padded to Np entries) of an MLP's second product."""
    y = torch.empty((M, Np), dtype=torch.float32, device=device)
    t2 = torch.empty((M, Np), dtype=torch.float32, device=device) if act2 else None
    b2p = b2
    if b2 is not None and Np != b2.shape[0]:
        b2p = torch.zeros(Np, dtype=torch.float32, device=device)
        b2p[:b2.shape[0]].copy_(b2.detach())
    return y, t2, b2p


# ---- the backends --------------------------------------------------------------------------------
class _BF16:
    """"bf16" and "fp8": bf16 operands in HBM.  A kept operand is the row-major bf16 tensor."""
    KEPT = 1                                    # tensors per kept operand
    pack = staticmethod(lambda xb: (xb,))
    unpack = staticmethod(lambda xb: xb)

    @staticmethod
    def prepare(x2, shapes):
        """((e4m3 form of x or None, bf16 copy), the bf16 copy for backward): the bf16 copy of a node's fp32
        input and, in "fp8" mode when every forward product of the node that reads x ((M, N, K) in `shapes`)
        fits the e4m3 kernel, its per-tensor e4m3 quantisation (x8, inv_scale) from the same pass."""
        if ops.PRECISION == "fp8" and all(ops.f8_supported(*s) for s in shapes):
            x8, sx, xb = ops.cast_fp8(x2, want_bf16=True)
            return ((x8, sx), xb), xb
        xb = ops.cast_bf16(x2)
        return (None, xb), xb

    @staticmethod
    def nt(xin, w, M, N, K, **epi):
        """The forward product x W^T of a node: bf16 operands, or -- with an e4m3 form from prepare -- x and W
        quantised per tensor (W once per optimiser step) and multiplied on the fp8 MFMA."""
        xq, xb = xin
        if xq is not None:
            w8, sw = ops.cast_fp8(_as_weight(w), cache=True)
            ops.gemm_f8(xq[0], xq[1], w8, sw, M, N, K, **epi)
        else:
            ops.gemm_lp(xb, _shadow(w), 0, M, N, K, **epi)

    @staticmethod
    def mlp_fwd(xin, M, K, w1, b1, w2, b2, act1, act2, Np, device):
        """The two forward products of one MLP: (y (M, Np) fp32, t2 or None, t1b or None, h kept)."""
        H = w1.shape[0]
        hb, t1b = _hidden_buffers(M, H, act1, device)
        _BF16.nt(xin, w1, M, H, K, bias=b1, act=act1, Cb=hb, Pb=t1b)
        y, t2, b2p = _output_buffers(M, Np, b2, act2, device)
        ops.gemm_lp(hb, _shadow(w2, pad_rows=Np), 0, M, Np, H, C=y, bias=b2p, preact=t2, act=act2)
        return y, t2, t1b, hb

    @staticmethod
    def grad_in(dT, b, n):
        """(bf16 form of an incoming gradient dT (M, Np): its cast when it is fp32, itself when it is bf16; db
        (first n column sums, from the same pass) or None when b is)."""
        Np = dT.shape[1]
        want_cast = dT.dtype != torch.bfloat16
        if b is None:
            return (ops.cast_bf16(dT) if want_cast else dT), None
        db, dTb = _grad_into(b, n, Np, lambda: torch.zeros(Np, dtype=torch.float32, device=dT.device),
                             lambda out, acc: ops.cast_colsum(dT, out, accumulate=acc, want_cast=want_cast))
        return (dTb if want_cast else dT), db

    @staticmethod
    def dgrad(dTb, w, pad_rows, M, N, K, **epi):
        """dT W over the (padded) output rows of w: (M, N) from dTb (M, K) and the shadow as stored (K, N)."""
        ops.gemm_lp(dTb, _shadow(w, pad_rows=pad_rows), 2, M, N, K, **epi)

    @staticmethod
    def wgrad(dTb, xb, w, Np, K, n_rows):
        """dW (n_rows, K) = dT^T x over the token rows, fp32, accumulated into w.grad when it is a
        FlatAdam slot; dTb (M, Np >= n_rows) and xb (M, K) are the row-major bf16 activations."""
        M = dTb.shape[0]
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


class _MX:
    """"mxfp8": every product on MX-e4m3 operands.  A kept operand is the transposed form (q, s) of a tensor:
    what its weight-gradient product reads."""
    KEPT = 2
    pack = staticmethod(lambda t: (t.q, t.s))
    unpack = staticmethod(ops.MxOperand)

    @staticmethod
    def prepare(x2, shapes):
        """(row form of x, its transposed form for backward), from one pass."""
        return ops.mx_quant(x2, row=True, transposed=True)

    @staticmethod
    def nt(xr, w, M, N, K, **epi):
        ops.gemm_mx(xr, ops.mx_weight(w)[0], M, N, K, **epi)

    @staticmethod
    def mlp_fwd(xr, M, K, w1, b1, w2, b2, act1, act2, Np, device):
        """The two forward products of one MLP from x's row form: (y (M, Np) fp32, t2 or None, t1b or None,
        h's transposed form)."""
        H = w1.shape[0]
        w1r, _ = ops.mx_weight(w1)
        w2r, _ = ops.mx_weight(w2, Np)
        hb, t1b = _hidden_buffers(M, H, act1, device)
        ops.gemm_mx(xr, w1r, M, H, K, bias=b1, act=act1, Cb=hb, Pb=t1b)
        hr, ht = ops.mx_quant(hb, row=True, transposed=True)
        y, t2, b2p = _output_buffers(M, Np, b2, act2, device)
        ops.gemm_mx(hr, w2r, M, Np, H, C=y, bias=b2p, preact=t2, act=act2)
        return y, t2, t1b, ht

    @staticmethod
    def grad_in(dT, b, n):
        """((row form, transposed form) of an incoming gradient dT (M, Np); db (first n column sums, from the
        same pass) or None when b is)."""
        Np = dT.shape[1]
        if b is None:
            return ops.mx_quant(dT, row=True, transposed=True), None
        db, forms = _grad_into(b, n, Np, lambda: torch.empty(Np, dtype=torch.float32, device=dT.device),
                               lambda out, acc: ops.mx_quant(dT, row=True, transposed=True, colsum=out,
                                                             accumulate=acc))
        return forms, db

    @staticmethod
    def dgrad(forms, w, pad_rows, M, N, K, **epi):
        ops.gemm_mx(forms[0], ops.mx_weight(w, pad_rows)[1], M, N, K, **epi)

    @staticmethod
    def wgrad(forms, xt, w, Np, K, n_rows):
        """dW (n_rows, K) = dT^T x from the transposed forms dTt (Np, Mp) and xt (K, Mp), accumulated into
        w.grad when it is a FlatAdam slot."""
        Mp = xt.q.shape[1]
        sk = _mx_splitk((Np // 128) * (K // 128), Mp)
        return _wgrad_into(w, Np, K, n_rows, xt.q.device,
                           lambda C, acc: ops.gemm_mx(forms[1], xt, Np, K, Mp, C=C, splitk=sk, accumulate=acc))


# ---- the shells ----------------------------------------------------------------------------------
def _mlp_bwd(B, dT2, w1, b1, w2, b2, t1b, hk, xk, act1, N, Np, need, dx):
    """Backward of one MLP from dT2 (M, Np) fp32; hk, xk: the kept operands of h and x; need =
    needs_input_grad of (x, w1, b1, w2, b2).  dx: None (no input gradient), or (tensor, accumulate).
    Returns (dw1, db1, dw2, db2)."""
    M = dT2.shape[0]
    H, K = w1.shape
    g2, db2 = B.grad_in(dT2, b2 if need[4] else None, N)
    dT1b = torch.empty((M, H), dtype=torch.bfloat16, device=dT2.device)
    B.dgrad(g2, w2, Np, M, H, Np, gradz=t1b, gact=act1, Cb=dT1b)
    dw2 = B.wgrad(g2, hk, w2, Np, H, N) if need[3] else None
    del g2
    g1, db1 = B.grad_in(dT1b, b1 if need[2] else None, H)
    if dx is not None:
        B.dgrad(g1, w1, 0, M, K, H, C=dx[0], accumulate=dx[1])
    dw1 = B.wgrad(g1, xk, w1, H, K, H) if need[1] else None
    return dw1, db1, dw2, db2


def _mlp_forward(B, ctx, x, act1, act2, params, first, pad):
    """y_i = act2(act1(x W1_i^T + b1_i) W2_i^T + b2_i) for the len(params) / 4 blocks (w1, b1, w2, b2) of
    `params` on their common input x: one preparation of x.  first: position of params[0] among the node's
    inputs; pad: ragged output widths run zero-padded to whole 128-column tiles.  Returns the outputs."""
    require_cuda(x, *params)
    shp = x.shape
    x2 = _2d(f32c(x))
    M, K = x2.shape
    n = len(params) // 4
    xin, xk = B.prepare(x2, [(M, params[4 * i].shape[0], K) for i in range(n)])
    outs, saved = [], [*B.pack(xk)]
    for i in range(n):
        w1, b1, w2, b2 = params[4 * i:4 * i + 4]
        N = w2.shape[0]
        Np = _pad128(N) if pad else N
        y, t2, t1b, hk = B.mlp_fwd(xin, M, K, w1, b1, w2, b2, act1, act2, Np, x2.device)
        if Np != N:
            y = y[:, :N].contiguous()
        outs.append(y.reshape(*shp[:-1], N))
        saved += [t2, t1b, *B.pack(hk)]
    ctx.save_for_backward(*saved)
    ctx.cfg = (act1, act2, shp, first, pad)
    ctx.params = params
    return outs


def _mlp_backward(B, ctx, dys):
    """(dx or None, [dw1, db1, dw2, db2 of every block]): the three input gradients are accumulated by the GEMM
    epilogues into one tensor -- the first block that runs writes it, later blocks add to it."""
    saved = ctx.saved_tensors
    act1, act2, shp, first, pad = ctx.cfg
    xk = B.unpack(*saved[:B.KEPT])
    per = 2 + B.KEPT                            # saved tensors per block: t2, t1b, the kept operand of h
    want_dx = ctx.needs_input_grad[0]
    dx, grads = None, []
    for i, dy in enumerate(dys):
        w1, b1, w2, b2 = ctx.params[4 * i:4 * i + 4]
        t2, t1b, *hk = saved[B.KEPT + per * i:B.KEPT + per * (i + 1)]
        N = w2.shape[0]
        Np = _pad128(N) if pad else N
        dy2 = _2d(f32c(dy))
        M = dy2.shape[0]
        if Np != N:
            padded = torch.zeros((M, Np), dtype=torch.float32, device=dy2.device)
            padded[:, :N].copy_(dy2)
            dy2 = padded
        dT2 = ops.act_bwd(dy2, t2, act2) if act2 else dy2
        accumulate = dx is not None
        if want_dx and not accumulate:
            dx = torch.empty((M, w1.shape[1]), dtype=torch.float32, device=dy2.device)
        ni = first + 4 * i                      # needs_input_grad index of w1
        need = (want_dx, *ctx.needs_input_grad[ni:ni + 4])
        grads += _mlp_bwd(B, dT2, w1, b1, w2, b2, t1b, B.unpack(*hk), xk, act1, N, Np, need,
                          (dx, accumulate) if want_dx else None)
    if dx is not None:
        dx = dx.reshape(shp)
    return dx, grads


def _linear_forward(B, ctx, x, weight, bias, residual, act):
    require_cuda(x, weight)
    shp = x.shape
    x2 = _2d(f32c(x))
    M, K = x2.shape
    N = weight.shape[0]
    xin, xk = B.prepare(x2, [(M, N, K)])
    r2 = _2d(f32c(residual)) if residual is not None else None
    y = torch.empty((M, N), dtype=torch.float32, device=x2.device)
    t = torch.empty((M, N), dtype=torch.float32, device=x2.device) if act else None
    B.nt(xin, weight, M, N, K, C=y, bias=bias, residual=r2, preact=t, act=act)
    ctx.save_for_backward(t, *B.pack(xk))
    ctx.cfg = (act, residual is not None, shp)
    ctx.params = (weight, bias)
    return y.reshape(*shp[:-1], N)


def _linear_backward(B, ctx, dy):
    t, *xk = ctx.saved_tensors
    act, has_res, shp = ctx.cfg
    weight, bias = ctx.params
    N, K = weight.shape
    dy2 = _2d(f32c(dy))
    M = dy2.shape[0]
    dT = ops.act_bwd(dy2, t, act) if act else dy2
    g, db = B.grad_in(dT, bias if (bias is not None and ctx.needs_input_grad[2]) else None, N)
    dx = dw = dr = None
    if ctx.needs_input_grad[0]:
        dx = torch.empty((M, K), dtype=torch.float32, device=dy2.device)
        B.dgrad(g, weight, 0, M, K, N, C=dx)
        dx = dx.reshape(shp)
    if ctx.needs_input_grad[1]:
        dw = B.wgrad(g, B.unpack(*xk), weight, N, K, N)
    if has_res and ctx.needs_input_grad[3]:
        dr = dT.reshape(dy.shape)
    return dx, dw, db, dr, None


# ---- the node classes: a shell bound to a backend ------------------------------------------------
# (forward and backward of a torch.autograd.Function are static and do not see the subclass: the backend is
# bound by closure)
def _node_class(name, doc, forward, backward):
    return type(name, (torch.autograd.Function,),
                {"__doc__": doc, "forward": staticmethod(forward), "backward": staticmethod(backward)})


def _mlp2_class(name, B, doc):
    def forward(ctx, x, w1, b1, w2, b2, act1, act2):
        return _mlp_forward(B, ctx, x, act1, act2, (w1, b1, w2, b2), 1, True)[0]

    def backward(ctx, dy):
        dx, grads = _mlp_backward(B, ctx, (dy,))
        return (dx, *grads, None, None)

    return _node_class(name, doc, forward, backward)


def _mlp2x3_class(name, B, doc):
    def forward(ctx, x, act1, act2, *params):
        return tuple(_mlp_forward(B, ctx, x, act1, act2, params, 3, False))

    def backward(ctx, *dys):
        dx, grads = _mlp_backward(B, ctx, dys)
        return (dx, None, None, *grads)

    return _node_class(name, doc, forward, backward)


def _linear_class(name, B, doc):
    return _node_class(name, doc, lambda ctx, *args: _linear_forward(B, ctx, *args),
                       lambda ctx, dy: _linear_backward(B, ctx, dy))


_MLP2LP = _mlp2_class("_MLP2LP", _BF16,
                      "y = act2(act1(x W1^T + b1) W2^T + b2), reduced precision (see module docstring).")
_MLP2x3LP = _mlp2x3_class("_MLP2x3LP", _BF16,
                          "The q, k, v MLPs of a self-attention layer on their common input: one bf16 cast of the "
                          "input, the three input gradients accumulated by the GEMM epilogues into one tensor.")
_LinearActLP = _linear_class("_LinearActLP", _BF16, "y = act(x W^T + b [+ residual]), reduced precision.")
_MLP2MX = _mlp2_class("_MLP2MX", _MX,
                      "y = act2(act1(x W1^T + b1) W2^T + b2), all six products on MX-e4m3 operands.")
_MLP2x3MX = _mlp2x3_class("_MLP2x3MX", _MX,
                          'The q, k, v MLPs on their common input in "mxfp8": one quantisation of the input, the '
                          "three input gradients accumulated by the GEMM epilogues into one tensor.")
_LinearActMX = _linear_class("_LinearActMX", _MX,
                             "y = act(x W^T + b [+ residual]), the three products on MX-e4m3 operands.")


# ---- which node: the predicates and the entry points ---------------------------------------------
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
