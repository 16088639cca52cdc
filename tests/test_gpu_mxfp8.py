"""Opt-in "mxfp8" mode (qarig.ops.PRECISION = "mxfp8"): every product of the reduced-precision Linear
nodes -- forward, input gradient, weight gradient -- on MX-e4m3 operands (include/qarig.h: e4m3
elements, one e8m0 scale per 32 elements along the reduction), v_mfma_scale_f32_32x32x64_f8f6f4 with
the scales applied in the instruction.  NOT the parity mode.
Pinned here: the quantiser bit for bit against the format's torch reference; the scale / fragment
map of the GEMM on exact data (per-row, per-block scales); the GEMM against fp64 of its own
dequantised operands; the routing of each node; nodes, a training step, 30 steps and graph replay
against fp32 / eager within the e4m3 budget (bounds stated per test)."""
import pytest
import torch

from conftest import rel_err

pytestmark = pytest.mark.gpu

F8 = torch.float8_e4m3fn


def _cos(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a * b).sum() / (a.norm() * b.norm()))


def _ref_exponent(amax):
    """Smallest e with amax <= 448 2^e (fp64, exact), clamped to [-127, 127]; 0 for amax == 0."""
    a = amax.double()
    _, x = torch.frexp(a)
    e = x.to(torch.int64) - 10
    for _ in range(3):
        e = torch.where(a > 448.0 * torch.pow(2.0, e.double()), e + 1, e)
    e = torch.where(a == 0, torch.zeros_like(e), e)
    return e.clamp(-127, 127)


def _ref_quant(x):
    """Row form of x (R, C) fp32: (bytes (R, C) uint8, scale bytes (R, C/32) uint8)."""
    R, C = x.shape
    xb = x.float().reshape(R, C // 32, 32)
    e = _ref_exponent(xb.abs().amax(-1))
    s = torch.pow(2.0, -e.double()).float()                       # exact powers of two
    q = (xb * s[..., None]).to(F8).view(torch.uint8).reshape(R, C)
    return q, (e + 127).to(torch.uint8)


def _dequant(op, rows=None):
    q = op.q.view(F8).double()
    s = torch.pow(2.0, op.s.double() - 127.0)
    out = (q.reshape(q.shape[0], -1, 32) * s[..., None]).reshape(q.shape)
    return out if rows is None else out[:rows]


@pytest.fixture
def mx_mode():
    from qarig import ops
    old = ops.PRECISION
    ops.PRECISION = "mxfp8"
    yield ops
    ops.PRECISION = old


def _awkward(R, C, g, dtype):
    """Random data with per-row magnitudes from 1e-30 to 1e30, zero blocks, blocks whose maximum is
    exactly 448 2^k and elements that land on e4m3 subnormals."""
    x = torch.randn((R, C), generator=g, dtype=torch.float64)
    mag = torch.logspace(-30, 30, R, dtype=torch.float64)[torch.randperm(R, generator=g)]
    x = (x * mag[:, None]).float()
    x[3, 32:64] = 0.0                                             # an all-zero row block
    x[:, 96:128] = 0.0                                            # an all-zero column strip
    x[5, :32] = torch.linspace(-1.0, 1.0, 32)
    x[5, 7] = 448.0 * 2.0 ** 3                                    # amax exactly 448 2^3
    x[6, 32:64] = 2.0 ** -12                                      # subnormal e4m3 next to 448 2^-3
    x[6, 40] = 448.0 * 2.0 ** -3
    x[7, :] = 448.0 * 2.0 ** -20
    x = x.to(dtype)
    return x


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("R,C", [(256, 256), (200, 384), (1000, 128)])
def test_mx_quant_matches_the_format_reference(dtype, R, C):
    from qarig import ops
    g = torch.Generator().manual_seed(R + C)
    x = _awkward(R, C, g, dtype)
    xd = x.cuda()
    want_q, want_s = _ref_quant(x.float())
    Rp = (R + 127) // 128 * 128
    xt = torch.zeros((C, Rp))
    xt[:, :R] = x.float().t()
    want_tq, want_ts = _ref_quant(xt)                             # padding: zeros, scale byte 127
    for row, tr in ((True, False), (False, True), (True, True)):
        cs = torch.full((C,), 5.0, device="cuda")
        rf, tf = ops.mx_quant(xd, row=row, transposed=tr, colsum=cs if tr else None)
        if row:
            assert torch.equal(rf.q.cpu(), want_q) and torch.equal(rf.s.cpu(), want_s)
        if tr:
            assert tf.q.shape == (C, Rp) and tf.s.shape == (C, Rp // 32)
            assert torch.equal(tf.q.cpu(), want_tq) and torch.equal(tf.s.cpu(), want_ts)
            assert Rp == R or int(tf.q[:, R:].max()) == 0
            ref = x.double().sum(0)
            err = (cs.double().cpu() - ref).abs() / x.double().abs().sum(0).clamp_min(1e-300)
            assert float(err.max()) <= 1e-6
    # accumulate into an existing column-sum slot
    y = torch.randn((256, 128), generator=g).cuda().to(dtype)
    cs = torch.ones(128, device="cuda")
    ops.mx_quant(y, row=False, transposed=True, colsum=cs, accumulate=True)
    assert rel_err(cs, y.double().sum(0) + 1.0) < 1e-6


def _scaled_ints(rows, K, g, lo=125, hi=129):
    """An exact MX operand: small integers (exact in e4m3) with random scale bytes per row and block."""
    from qarig import ops
    q = torch.randint(-4, 5, (rows, K), generator=g).float().to(F8).view(torch.uint8)
    s = torch.randint(lo, hi + 1, (rows, K // 32), generator=g).to(torch.uint8)
    return ops.MxOperand(q.cuda(), s.cuda())


@pytest.mark.parametrize("M,N,K,splitk", [(128, 128, 128, 1), (256, 384, 512, 1), (384, 128, 1024, 4),
                                          (4096, 4096, 256, 1), (2048, 2048, 1024, 4)])
def test_mx_scale_and_fragment_map_on_exact_data(M, N, K, splitk):
    """Products of integers in [-4, 4] times 2^(-4..4) over K <= 1024 span at most 23 bits: the dot-product
    unit's alignment and the fp32 accumulation keep them exactly, so any slip in which scale byte a lane
    feeds (op_sel, row, 32-block, k-tile) changes the result.  E = 127 must mean 1.  (4096 x 4096 takes
    the 256 x 256-tile kernel, 2048 x 2048 x 4 its split-K.)"""
    from qarig import ops
    g = torch.Generator().manual_seed(M + N + K + splitk)
    A = _scaled_ints(M, K, g)
    B = _scaled_ints(N, K, g)
    C = torch.full((M, N), float("nan"), device="cuda")
    ops.gemm_mx(A, B, M, N, K, C=C, splitk=splitk)
    assert torch.equal(C.double().cpu(), (_dequant(A) @ _dequant(B).t()).cpu())
    one = ops.MxOperand(A.q, torch.full_like(A.s, 127))
    ops.gemm_mx(one, ops.MxOperand(B.q, torch.full_like(B.s, 127)), M, N, K, C=C)
    assert torch.equal(C.double().cpu(), (A.q.view(F8).double() @ B.q.view(F8).double().t()).cpu())


def test_mx_epilogue_options_on_exact_data():
    from qarig import ops
    M, N, K = 256, 256, 512
    g = torch.Generator().manual_seed(9)
    A, B = _scaled_ints(M, K, g), _scaled_ints(N, K, g)
    P = (_dequant(A) @ _dequant(B).t()).float()
    bias = torch.randint(-3, 4, (N,), generator=g).float().cuda()
    R = torch.randint(-3, 4, (M, N), generator=g).float().cuda()
    C = torch.empty((M, N), device="cuda")
    pre = torch.empty((M, N), device="cuda")
    Cb = torch.empty((M, N), dtype=torch.bfloat16, device="cuda")
    Pb = torch.empty((M, N), dtype=torch.bfloat16, device="cuda")
    ops.gemm_mx(A, B, M, N, K, C=C, bias=bias, residual=R, preact=pre, act=1, Cb=Cb, Pb=Pb)
    t = P + bias + R
    assert torch.equal(pre, t)
    assert rel_err(C, torch.nn.functional.silu(t.double())) < 2e-6
    assert torch.equal(Cb, C.bfloat16()) and torch.equal(Pb, t.bfloat16())
    # act' fused into the input gradient (gradz in fp32 and in bf16), bf16 output only
    z = torch.randn((M, N), generator=g).cuda()
    for zz in (z, z.bfloat16()):
        Cz = torch.empty((M, N), dtype=torch.bfloat16, device="cuda")
        ops.gemm_mx(A, B, M, N, K, gradz=zz, gact=1, Cb=Cz)
        zf = zz.double()
        sg = torch.sigmoid(zf)
        want = P.double() * sg * (1 + zf * (1 - sg))
        assert rel_err(Cz.float(), want) < 4e-3
    # accumulate, plain and split
    for sk in (1, 4):
        D = R.clone()
        ops.gemm_mx(A, B, M, N, K, C=D, splitk=sk, accumulate=True)
        assert torch.equal(D, P + R)


@pytest.mark.parametrize("M,N,K,splitk", [(32768, 2048, 512, 1), (2048, 512, 32768, 4), (4224, 512, 2048, 1),
                                          (8320, 2048, 4224, 3)])
def test_mx_gemm_is_exact_on_its_quantised_operands(M, N, K, splitk):
    """Against fp64 of the dequantised operands: 6e-5 sqrt(K/512) of max|C|, as for gemm_f8 (the dot-product
    unit aligns each instruction's 64 products to the largest exponent first)."""
    from qarig import ops
    g = torch.Generator(device="cuda").manual_seed(K + splitk)
    x = torch.randn((M, K), device="cuda", generator=g)
    w = torch.randn((N, K), device="cuda", generator=g) * 0.05
    xr, _ = ops.mx_quant(x)
    wr, _ = ops.mx_quant(w)
    C = torch.empty((M, N), device="cuda")
    ops.gemm_mx(xr, wr, M, N, K, C=C, splitk=splitk)
    want = _dequant(xr) @ _dequant(wr).t()
    err = float((C.double() - want).abs().max() / want.abs().max())
    assert err < 6e-5 * max(1, K / 512) ** 0.5, err


def _mlp_data(g, M=2048, K=512, H=2048, N=512):
    x = torch.randn((4, M // 4, K), generator=g).cuda()
    w1, b1 = (torch.randn((H, K), generator=g) * 0.04).cuda(), (torch.randn(H, generator=g) * 0.1).cuda()
    w2, b2 = (torch.randn((N, H), generator=g) * 0.02).cuda(), (torch.randn(N, generator=g) * 0.1).cuda()
    dy = torch.randn((4, M // 4, N), generator=g).cuda()
    return x, w1, b1, w2, b2, dy


def test_mxfp8_mode_routes_every_product_to_the_mx_kernel(mx_mode, monkeypatch):
    ops = mx_mode
    from qarig import functional as QF
    calls, other = [], []
    real = ops.gemm_mx
    monkeypatch.setattr(ops, "gemm_mx", lambda A, B, M, N, K, **k: (calls.append((M, N, K)), real(A, B, M, N, K, **k))[1])
    monkeypatch.setattr(ops, "gemm_lp", lambda *a, **k: other.append(a))
    monkeypatch.setattr(ops, "gemm_f8", lambda *a, **k: other.append(a))
    g = torch.Generator().manual_seed(1)
    x, w1, b1, w2, b2, dy = _mlp_data(g)
    leaves = [t.clone().requires_grad_(True) for t in (x, w1, b1, w2, b2)]
    y = QF.mlp2(*leaves, 1, 0)
    assert type(y.grad_fn).__name__ == "_MLP2MXBackward"
    (y * dy).sum().backward()
    assert sorted(calls) == sorted([(2048, 2048, 512), (2048, 512, 2048),      # forward
                                    (2048, 2048, 512), (2048, 512, 2048),      # input gradients
                                    (512, 2048, 2048), (2048, 512, 2048)])     # weight gradients
    assert not other
    calls.clear()
    xl = x[..., :512].reshape(2048, 512).clone().requires_grad_(True)
    wl = w2[:, :512].clone().requires_grad_(True)
    QF.linear_act(xl, wl, b2.clone().requires_grad_(True), None, 1).sum().backward()
    assert sorted(calls) == sorted([(2048, 512, 512), (2048, 512, 512), (512, 512, 2048)]) and not other
    calls.clear()
    params = [t.clone().requires_grad_(True) for _ in range(3) for t in (w1, b1, w2, b2)]
    outs = QF.mlp2x3(x.clone().requires_grad_(True), [params[4 * i:4 * i + 4] for i in range(3)], 1, 0)
    sum((o * dy).sum() for o in outs).backward()
    assert len(calls) == 18 and not other


def _node_results(ops, mode, x, w1, b1, w2, b2, dy):
    from qarig import functional as QF
    ops.PRECISION = mode
    leaves = [t.clone().requires_grad_(True) for t in (x, w1, b1, w2, b2)]
    y = QF.mlp2(*leaves, 1, 0)
    (y * dy).sum().backward()
    return [y.detach()] + [t.grad for t in leaves]


def test_mx_nodes_track_fp32_nodes(mx_mode):
    """e4m3 keeps 3 mantissa bits (<= 6.25 % per element), now in every product: outputs and input gradients
    cosine > 0.997, weight and bias gradients > 0.99; the Linear node likewise."""
    ops = mx_mode
    g = torch.Generator().manual_seed(7)
    data = _mlp_data(g)
    f32 = _node_results(ops, "f32", *data)
    mx = _node_results(ops, "mxfp8", *data)
    for n, a, b in zip(["y", "dx", "dw1", "db1", "dw2", "db2"], mx, f32):
        c = _cos(a, b)
        assert c > (0.997 if n in ("y", "dx") else 0.99), (n, c)
    assert not torch.equal(mx[0], f32[0])
    from qarig import functional as QF
    x, w, b = data[0], data[3][:, :512].contiguous(), data[4]
    res = {}
    for mode in ("f32", "mxfp8"):
        ops.PRECISION = mode
        leaves = [t.clone().requires_grad_(True) for t in (x, w, b)]
        y = QF.linear_act(*leaves, None, 1)
        (y * data[5]).sum().backward()
        res[mode] = [y.detach()] + [t.grad for t in leaves]
    for n, a, c in zip(["y", "dx", "dw", "db"], res["mxfp8"], res["f32"]):
        assert _cos(a, c) > (0.997 if n in ("y", "dx") else 0.99), (n, _cos(a, c))


def test_mx_forward_beats_per_tensor_fp8_on_outlier_rows(mx_mode):
    """A few input rows 10^4 x the rest: one scale per tensor pushes the other rows into e4m3's subnormal
    range, one scale per 32 elements does not.  The Linear node's forward (one product, e4m3 in both
    modes), error on the ordinary rows.  (At 1000 x the two tie: 3.76 % against 3.74 %, the ordinary
    rows still mostly in e4m3's normal range under the per-tensor scale.)"""
    ops = mx_mode
    from qarig import functional as QF
    g = torch.Generator().manual_seed(8)
    x = torch.randn((2048, 512), generator=g).cuda()
    rows = torch.randperm(2048, generator=g)[:8].cuda()
    x[rows] *= 1e4
    keep = torch.ones(2048, dtype=torch.bool, device="cuda")
    keep[rows] = False
    w = (torch.randn((512, 512), generator=g) * 0.04).cuda().requires_grad_(True)
    b = torch.zeros(512, device="cuda")
    ys = {}
    for mode in ("f32", "fp8", "mxfp8"):
        ops.PRECISION = mode
        ys[mode] = QF.linear_act(x.clone().requires_grad_(True), w, b, None, 0).detach()[keep]
    err = {m: float((ys[m] - ys["f32"]).norm() / ys["f32"].norm()) for m in ("fp8", "mxfp8")}
    assert err["mxfp8"] <= err["fp8"], err


def test_mx_classifier_node_8193_columns(mx_mode):
    """The ragged classifier width goes through the 128-padding (8,320 rows of W2)."""
    ops = mx_mode
    g = torch.Generator().manual_seed(12)
    x, w1, b1, _, _, _ = _mlp_data(g)
    w2 = (torch.randn((8193, 2048), generator=g) * 0.02).cuda()
    b2 = (torch.randn(8193, generator=g) * 0.1).cuda()
    dy = torch.randn((4, 512, 8193), generator=g).cuda()
    f32 = _node_results(ops, "f32", x, w1, b1, w2, b2, dy)
    mx = _node_results(ops, "mxfp8", x, w1, b1, w2, b2, dy)
    assert mx[0].shape == f32[0].shape and mx[4].shape == (8193, 2048) and mx[5].shape == (8193,)
    for n, a, b in zip(["y", "dx", "dw1", "db1", "dw2", "db2"], mx, f32):
        c = _cos(a, b)
        assert c > (0.997 if n in ("y", "dx") else 0.99), (n, c)


def _narrow_model():
    from models.Transformer import Transformer
    torch.manual_seed(2)
    m = Transformer(use_encoder=False, use_pos_cond=True, num_enc_layers=None, num_dec_layers=2,
                    num_enc_embedding=None, num_dec_embedding=1024, self_attn_heads=16,
                    cross_attn_heads=None, transformer_in_dim=256, transformer_out_dim=513,
                    transformer_hidden_dim=1024).cuda()
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for p in m.parameters():
            if p.abs().max() == 0:
                p.copy_(torch.randn(p.shape, generator=g) * 0.02)
    return m, g


def test_mxfp8_train_steps_track_fp32():
    """One step: loss within 2e-2 relative, flat gradient cosine > 0.98.  30 steps on a fixed batch at lr 1e-4:
    the loss falls and ends within 1.5 % of the fp32 run's (measured 4.661 against 4.639; bf16 4.639, fp8
    4.646).  At lr 1e-3 the 30-step trajectory is chaotic in every reduced mode (fp32 0.83, bf16 0.64, fp8
    0.50, mxfp8 0.52), so that rate pins nothing."""
    from qarig import ops, pipeline
    from qarig.optim import FlatAdam
    res = {}
    for mode in ("f32", "mxfp8"):
        m, g = _narrow_model()
        opt = FlatAdam(m.parameters(), lr=1e-4, betas=(0.5, 0.999))
        x = torch.randint(0, 1024, (8, 128), generator=g).cuda()
        t = torch.randint(0, 513, (8, 128), generator=g).cuda()
        pos = torch.arange(128)[None].repeat(8, 1).cuda()
        old, ops.PRECISION = ops.PRECISION, mode
        losses = []
        try:
            for i in range(30):
                opt.zero_grad()
                losses.append(float(pipeline.train_step(m, opt, x, None, t, pos, dp=False).detach()))
                if i == 0:
                    g0 = opt.flat_grad.detach().clone()
        finally:
            ops.PRECISION = old
        res[mode] = (losses, g0)
    lf, gf = res["f32"]
    lm, gm = res["mxfp8"]
    assert abs(lm[0] - lf[0]) < 2e-2 * abs(lf[0]), (lm[0], lf[0])
    cos = _cos(gf, gm)
    assert cos > 0.98, cos
    assert not torch.equal(gf, gm)
    assert lm[-1] < 0.9 * lm[0], lm
    assert abs(lm[-1] - lf[-1]) < 0.015 * abs(lf[-1]), (lm[-1], lf[-1])


def test_mxfp8_graph_replay_matches_eager(mx_mode):
    """pipeline.GraphedTrainStep in "mxfp8": the MX weight copies are rebuilt inside the captured graph, so
    replayed steps see the weights Adam just wrote.  Same losses and parameters as the eager loop over 3
    steps, bit for bit (every kernel of the step is deterministic)."""
    from models.Codebook import Codebook
    from models.Transformer import Transformer
    from qarig import pipeline
    from qarig.optim import FlatAdam
    g = torch.Generator().manual_seed(4)
    lr_cb = Codebook(patch_dim=(16, 16), image_dim=(16, 16), image_channel=4, num_embeddings=128).cuda()
    hr_cb = Codebook(patch_dim=(1, 1), image_dim=(16, 16), image_channel=4, num_embeddings=128).cuda()
    with torch.no_grad():
        lr_cb.codebook.weight.copy_(torch.tanh(torch.randn((128, 1024), generator=g)))
        hr_cb.codebook.weight.copy_(torch.tanh(torch.randn((128, 4), generator=g)))
    zs = [torch.tanh(torch.randn((8, 4, 16, 16), generator=g)).cuda() for _ in range(3)]
    rands = [torch.randint(0, 257 - 256 + 1, (8,), generator=g) for _ in range(3)]
    runs = {}
    for warmup in (1, 10):
        torch.manual_seed(3)
        m = Transformer(use_encoder=False, use_pos_cond=True, num_enc_layers=None, num_dec_layers=1,
                        num_enc_embedding=None, num_dec_embedding=128 + 128, self_attn_heads=16,
                        cross_attn_heads=None, transformer_in_dim=256, transformer_out_dim=129,
                        transformer_hidden_dim=512).cuda()
        gi = torch.Generator().manual_seed(6)
        with torch.no_grad():
            for p in m.parameters():
                if p.abs().max() == 0:
                    p.copy_(torch.randn(p.shape, generator=gi) * 0.05)
        opt = FlatAdam(m.parameters(), lr=1e-2, betas=(0.5, 0.999))
        step = pipeline.GraphedTrainStep(m, opt, lr_cb, hr_cb, True, 256, warmup=warmup)
        losses = [float(step(z, r)) for z, r in zip(zs, rands)]
        assert (step.graph is not None) == (warmup == 1)
        runs[warmup] = (losses, [p.detach().clone() for p in m.parameters()])
    assert runs[1][0] == runs[10][0], (runs[1][0], runs[10][0])
    for a, b in zip(runs[1][1], runs[10][1]):
        assert torch.equal(a, b)
    assert runs[1][0][0] != runs[1][0][2]
