"""Ragged widths inside qarig_gemm_f32 (128 q + r, 1 <= r <= 8: the classifier's 513 = K_hr + 1 columns,
reference models/Transformer.py:82-102): weight gradient (the first 128 q output rows on the ring, the last
r rows on the tail kernels) and forward product (ring on 128 q columns, tail-column kernel), against fp64;
shapes on both sides of the routes' gates (q >= 2 and >= 4,096 token rows: tests/test_ragged_gemm_routing.py)
so that the routed and the unrouted paths meet the same bound; the cross-entropy entry with leading dimensions
against the dense entry, bit for bit; the input gradient over the zero columns that entry writes; the classifier
MLP node and one train step of a small model against fp64, and the same steps replayed from a captured graph."""
import pytest
import torch

from conftest import rel_err

pytestmark = pytest.mark.gpu

GEMM_TOL = 2e-6          # the project's bound for fp32 products: rel_err < 2e-6 * max(1, K/512)^0.5


@pytest.mark.parametrize("split", [1, 8])
@pytest.mark.parametrize("R", [256, 4096])
@pytest.mark.parametrize("N", [128, 256])
@pytest.mark.parametrize("q,r", [(1, 1), (1, 3), (2, 8), (4, 1), (3, 5)])
def test_ragged_weight_gradient_vs_fp64(q, r, N, R, split):
    from qarig import ops
    M = 128 * q + r
    ld = (M + 15) // 16 * 16
    g = torch.Generator().manual_seed(1000 * q + 100 * r + N + R + split)
    dT = torch.randn((R, ld), generator=g).cuda()            # A as stored: [reduction][output row], padded rows
    X = (torch.randn((R, N), generator=g) * 0.1).cuda()
    A = dT[:, :M]
    ref = A.double().cpu().t() @ X.double().cpu()
    rs_ref = A.double().cpu().sum(0)
    tol = GEMM_TOL * max(1, R / 512) ** 0.5

    def run(out0=None, rs0=None):
        buf = torch.full((M + 4, N), float("nan"), device="cuda")
        rsb = torch.full((M + 4,), float("nan"), device="cuda")
        if out0 is not None:
            buf[:M].copy_(out0)
            rsb[:M].copy_(rs0)
        ops.gemm(A, X, a_kcontig=False, b_kcontig=False, splitk=split, out=buf[:M], accumulate=out0 is not None,
                 a_rowsum=rsb[:M])
        assert torch.isnan(buf[M:]).all() and torch.isnan(rsb[M:]).all()     # nothing behind the true rows
        return buf[:M], rsb[:M]

    out, rs = run()
    print(f"rows {M} N {N} R {R} split {split}: dW {rel_err(out, ref):.2e} rowsum {rel_err(rs, rs_ref):.2e} tol {tol:.2e}")
    assert rel_err(out, ref) < tol
    assert rel_err(rs, rs_ref) < tol
    out2, rs2 = run()
    assert torch.equal(out, out2) and torch.equal(rs, rs2)    # fixed summation order: the same bits
    # accumulate into what the outputs hold (.grad slots)
    out0 = torch.randn((M, N), generator=g).cuda()
    rs0 = torch.randn((M,), generator=g).cuda()
    acc, rsa = run(out0, rs0)
    assert rel_err(acc, out0.double().cpu() + ref) < tol
    assert rel_err(rsa, rs0.double().cpu() + rs_ref) < tol
    acc2, rsa2 = run(out0, rs0)
    assert torch.equal(acc, acc2) and torch.equal(rsa, rsa2)
    # without row sums
    plain = ops.gemm(A, X, a_kcontig=False, b_kcontig=False, splitk=split)
    assert rel_err(plain, ref) < tol


@pytest.mark.parametrize("K", [64, 272, 528])              # 17 and 33 k-tiles: the ring's remainder bodies
@pytest.mark.parametrize("q,r", [(1, 1), (1, 3), (2, 8), (3, 1), (4, 1)])
@pytest.mark.parametrize("M", [128, 256, 4096])            # 4,096 rows and q >= 2: the ragged route
def test_ragged_forward_vs_fp64(M, q, r, K):
    from oracle import ref_models as rm
    from qarig import _lib, ops
    N = 128 * q + r
    assert bool(_lib.load().qarig_gemm_ragged_nt(M, N, K)) == (M >= 4096 and q >= 2)
    g = torch.Generator().manual_seed(M + 1000 * q + 100 * r + K)
    A = torch.randn((M, K), generator=g).cuda()
    B = (torch.randn((N, K), generator=g) * 0.1).cuda()
    bias = torch.randn((N,), generator=g).cuda()
    ref = A.double().cpu() @ B.double().cpu().t()
    tol = GEMM_TOL * max(1, K / 512) ** 0.5
    for ldc in ((N + 3) // 4 * 4, (N + 15) // 16 * 16, 2 * N):
        buf = torch.full((M, ldc), float("nan"), device="cuda")
        ops.gemm(A, B, out=buf[:, :N])
        assert torch.isnan(buf[:, N:]).all()                  # columns behind the true width untouched
        e0 = rel_err(buf[:, :N], ref)
        buf.fill_(float("nan"))
        ops.gemm(A, B, bias=bias, out=buf[:, :N])
        assert torch.isnan(buf[:, N:]).all()
        e1 = rel_err(buf[:, :N], ref + bias.double().cpu())
        buf.fill_(float("nan"))
        _, pre = ops.gemm(A, B, bias=bias, want_preact=True, act=1, out=buf[:, :N])
        assert torch.isnan(buf[:, N:]).all()
        e2 = rel_err(pre, ref + bias.double().cpu())
        e3 = rel_err(buf[:, :N], rm.activation(ref + bias.double().cpu(), "silu"))
        print(f"M {M} N {N} K {K} ldc {ldc}: plain {e0:.2e} bias {e1:.2e} preact {e2:.2e} silu {e3:.2e} tol {tol:.2e}")
        assert e0 < tol and e1 < tol and e2 < tol and e3 < 5e-6
        # (a dense pre-activation of odd width keeps the call above off the route; without it the call is
        #  routed at 4,096 rows) the same call twice: the same bits
        runs = []
        for _ in range(2):
            again = torch.full((M, ldc), float("nan"), device="cuda")
            ops.gemm(A, B, bias=bias, act=1, out=again[:, :N])
            assert torch.isnan(again[:, N:]).all()
            runs.append(again[:, :N])
        assert rel_err(runs[0], rm.activation(ref + bias.double().cpu(), "silu")) < 5e-6
        assert torch.equal(runs[0], runs[1])
        if M >= 4096 and q >= 2:
            # routed with a saved pre-activation: both outputs in rows of ldc floats, through the C entry
            out2 = torch.full((M, ldc), float("nan"), device="cuda")
            pre2 = torch.full((M, ldc), float("nan"), device="cuda")
            rc = _lib.load().qarig_gemm_f32(A.data_ptr(), K, 1, B.data_ptr(), K, 1, out2.data_ptr(), ldc, M, N, K,
                                            bias.data_ptr(), None, 0, pre2.data_ptr(), ldc, 1, None, 0, 0, 1, 0,
                                            None, None, 0, ops.stream())
            assert rc == 0, _lib.last_error()
            assert torch.isnan(out2[:, N:]).all() and torch.isnan(pre2[:, N:]).all()
            assert rel_err(pre2[:, :N], ref + bias.double().cpu()) < tol
            assert torch.equal(out2[:, :N], runs[0])


def test_nine_ragged_columns_keep_the_unrouted_bits():
    """r = 9 is no ragged shape: the product into rows of whole 4-float groups carries the bits of the
    same product into a dense output, on the kernels that ran it before."""
    from qarig import _lib, ops
    M, N, K = 4096, 2 * 128 + 9, 272
    assert _lib.load().qarig_gemm_ragged_nt(M, N, K) == 0
    g = torch.Generator().manual_seed(3)
    A = torch.randn((M, K), generator=g).cuda()
    B = (torch.randn((N, K), generator=g) * 0.1).cuda()
    buf = torch.full((M, 268), float("nan"), device="cuda")
    ops.gemm(A, B, out=buf[:, :N])
    assert torch.equal(buf[:, :N], ops.gemm(A, B)) and torch.isnan(buf[:, N:]).all()


def test_ragged_weight_gradient_tail_is_the_ring_rows_neighbour():
    """The routed product's first 128 q rows carry the bits of the 128 q-row product on its own."""
    from qarig import ops
    M, N, R = 513, 256, 4096
    assert ops.wgrad_ring_rows(M, N, R) == 512
    g = torch.Generator().manual_seed(5)
    dT = torch.randn((R, 528), generator=g).cuda()
    X = (torch.randn((R, N), generator=g) * 0.1).cuda()
    full = ops.gemm(dT[:, :M], X, a_kcontig=False, b_kcontig=False, splitk=8)
    head = ops.gemm(dT[:, :512], X, a_kcontig=False, b_kcontig=False, splitk=8)
    assert torch.equal(full[:512], head)


def test_classifier_mlp_backward_takes_the_ragged_route_and_matches_fp64():
    """_MLP2 with a 385 = 3 * 128 + 1 column output layer over 4,096 rows (the smallest eligible classifier):
    the weight and bias gradients land in the .grad slots through the ragged route, within the gradient bound
    tests/test_gpu_grouped.py uses (1e-5) of an fp64 evaluation."""
    from conftest import grad_err
    from oracle import ref_models as rm
    from qarig import functional as QF
    from qarig import ops
    Mrows, Din, H, Nout = 4096, 64, 128, 385
    assert ops.wgrad_ring_rows(Nout, H, Mrows) == 384
    g = torch.Generator().manual_seed(9)
    x = torch.randn((Mrows, Din), generator=g).cuda().requires_grad_(True)
    ps = [torch.nn.Parameter(t.cuda()) for t in (
        torch.randn((H, Din), generator=g) * 0.1, torch.randn((H,), generator=g) * 0.1,
        torch.randn((Nout, H), generator=g) * 0.1, torch.randn((Nout,), generator=g) * 0.1)]
    for p in ps:
        p.grad = torch.zeros_like(p)              # slots: gradients accumulate in place
    y = QF.mlp2(x, *ps, 1, 0)
    dy = torch.randn((Mrows, Nout), generator=g).cuda()
    y.backward(dy)
    x64 = x.detach().double().cpu().requires_grad_(True)
    p64 = [p.detach().double().cpu().requires_grad_(True) for p in ps]
    h64 = rm.activation(x64 @ p64[0].t() + p64[1], "silu")
    y64 = h64 @ p64[2].t() + p64[3]
    y64.backward(dy.double().cpu())
    assert rel_err(y, y64) < 5e-6
    for p, r in zip(ps, p64):
        assert grad_err(p.grad, r.grad) < 1e-5
    assert grad_err(x.grad, x64.grad) < 1e-5


def test_train_step_with_a_385_column_classifier_vs_fp64_oracle():
    """A base Transformer with in_dim 64, hidden 128, 2 layers and a K_hr = 384 codebook (classifier width
    385 = 3 * 128 + 1) on 16 x 256 tokens = 4,096 rows, the smallest shape whose classifier takes the ragged
    routes: one pipeline.train_step, loss and every parameter gradient against the fp64 oracle
    (oracle/ref_models.py) within the bound the grouped-MLP test uses for gradients (1e-5)."""
    from conftest import grad_err
    from models.Transformer import Transformer
    from oracle import ref_models as rm
    from qarig import ops, pipeline
    from qarig.optim import FlatAdam
    N, S, V = 16, 256, 385
    assert ops.ragged_output_native(N * S, V, 128)
    torch.manual_seed(1)
    m = Transformer(use_encoder=False, use_pos_cond=True, num_enc_layers=None, num_dec_layers=2,
                    num_enc_embedding=None, num_dec_embedding=V, self_attn_heads=4, cross_attn_heads=None,
                    transformer_in_dim=64, transformer_out_dim=V, transformer_hidden_dim=128)
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        for p in m.parameters():
            if p.abs().max() == 0:
                p.copy_(torch.randn(p.shape, generator=g) * 0.05)
    sd = {k: v.detach().double().clone().requires_grad_(True) for k, v in m.state_dict().items()}
    x = torch.randint(0, V, (N, S), generator=g)
    tgt = torch.randint(0, V, (N, S), generator=g)
    pos = torch.arange(S)[None].repeat(N, 1)
    cfg = dict(use_encoder=False, use_pos_cond=True, num_dec_layers=2, self_attn_heads=4, hidden_activation="silu")
    ref_loss = rm.cross_entropy(rm.transformer_forward(sd, cfg, x, None, pos), tgt)
    ref_loss.backward()
    m = m.cuda()
    opt = FlatAdam(m.parameters(), lr=1e-4, betas=(0.5, 0.999))
    before, strided = dict(ops.RAGGED_CALLS), ops.STRIDED_CALLS["gemm_strided"]
    loss = pipeline.train_step(m, opt, x.cuda(), None, tgt.cuda(), pos.cuda(), dp=False)
    # the step took the ragged routes: classifier forward on 385 columns, its weight gradient on 385 rows, the
    # cross-entropy launch on the logits where the GEMM left them
    assert {k: ops.RAGGED_CALLS[k] - before[k] for k in before} == {"forward": 1, "wgrad": 1, "ce_ld": 1}
    # no model of this size has a table for the strided ring forward (64 columns; 12 projections of 256
    # positions are far fewer than 256 tiles): tests/test_gpu_table_forward_ring.py asserts that route
    assert ops.STRIDED_CALLS["gemm_strided"] == strided
    assert abs(float(loss.detach()) - float(ref_loss.detach())) < 1e-5 * abs(float(ref_loss.detach()))
    worst = 0.0
    for k, p in m.named_parameters():
        e = grad_err(p.grad, sd[k].grad)
        worst = max(worst, e)
        print(f"{k}: {e:.2e}")
        assert e < 1e-5, k
    print(f"worst gradient error {worst:.2e}")


def _ce_call(entry, logits, ld, target, M, C, ld_grad, guard=64):
    """One launch of a cross-entropy entry through the C ABI: (loss, row_ws, dlogits buffer incl. guard, flag)."""
    from qarig import _lib, ops
    lib = _lib.load()
    loss = torch.full((1,), float("nan"), device="cuda")
    rows = torch.full((M + guard,), float("nan"), device="cuda")
    dl = torch.full((M * ld_grad + guard,), float("nan"), device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    if entry == "ld":
        rc = lib.qarig_cross_entropy_ld_fwd(logits.data_ptr(), ld, target.data_ptr(), M, C, loss.data_ptr(),
                                            dl.data_ptr(), ld_grad, rows.data_ptr(), flag.data_ptr(), ops.stream())
    else:
        rc = lib.qarig_cross_entropy_fwd(logits.data_ptr(), target.data_ptr(), M, C, loss.data_ptr(), dl.data_ptr(),
                                         rows.data_ptr(), flag.data_ptr(), ops.stream())
    assert rc == 0, _lib.last_error()
    return loss, rows, dl, flag


@pytest.mark.parametrize("C", [5, 130, 513])
@pytest.mark.parametrize("M", [1, 7, 64])
def test_cross_entropy_with_leading_dimensions_carries_the_dense_bits(M, C):
    g = torch.Generator().manual_seed(10 * M + C)
    dense = (torch.randn((M, C), generator=g) * 3).cuda()
    target = torch.randint(0, C, (M,), generator=g).cuda()
    loss0, rows0, dl0, flag0 = _ce_call("dense", dense, C, target, M, C, C)
    assert int(flag0) == 0
    for ld in sorted({C, C + 3, (C + 15) // 16 * 16 if C != 513 else 528}):
        buf = torch.full((M, ld), float("nan"), device="cuda")     # NaN pads: a read of them would show
        buf[:, :C].copy_(dense)
        loss, rows, dl, flag = _ce_call("ld", buf, ld, target, M, C, ld)
        assert int(flag) == 0
        assert torch.equal(loss, loss0) and torch.equal(rows[:M], rows0[:M])
        d2 = dl[:M * ld].view(M, ld)
        assert torch.equal(d2[:, :C], dl0[:M * C].view(M, C))
        assert (d2[:, C:] == 0).all() and not torch.signbit(d2[:, C:]).any()      # exact zeros
        assert torch.isnan(dl[M * ld:]).all() and torch.isnan(rows[M:]).all()     # nothing past ld * M
        assert torch.isnan(buf[:, C:]).all()
        # a target outside [0, C) still sets the flag
        bad = target.clone()
        bad[M // 2] = C
        assert int(_ce_call("ld", buf, ld, bad, M, C, ld)[3]) == 1
        bad[M // 2] = -1
        assert int(_ce_call("ld", buf, ld, bad, M, C, ld)[3]) == 1


def _ce_pair_call(entry, logits, ld, target, M, C, ld_grad, eps, zeta, nu=0.0, R=0, w=None, guard=64):
    """One launch of a two-loss cross-entropy entry ("fused", or "reg" / "soft" on dense logits) through the C ABI:
    (loss (2,), row_ws incl. guard, dlogits buffer incl. guard, flag)."""
    from qarig import _lib, ops
    lib = _lib.load()
    loss = torch.full((2,), float("nan"), device="cuda")
    rows = torch.full((2 * M + guard,), float("nan"), device="cuda")
    dl = torch.full((M * ld_grad + guard,), float("nan"), device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    wp = None if w is None else w.data_ptr()
    tail = (loss.data_ptr(), dl.data_ptr(), rows.data_ptr(), flag.data_ptr(), ops.stream())
    if entry == "fused":
        rc = lib.qarig_cross_entropy_fused_fwd(logits.data_ptr(), ld, target.data_ptr(), M, C, C - 1, eps, zeta, nu, R,
                                               wp, loss.data_ptr(), dl.data_ptr(), ld_grad, rows.data_ptr(),
                                               flag.data_ptr(), ops.stream())
    elif entry == "soft":
        rc = lib.qarig_cross_entropy_soft_fwd(logits.data_ptr(), target.data_ptr(), M, C, C - 1, eps, zeta, nu, R, wp,
                                              *tail)
    else:
        rc = lib.qarig_cross_entropy_reg_fwd(logits.data_ptr(), target.data_ptr(), M, C, eps, zeta, *tail)
    assert rc == 0, _lib.last_error()
    return loss, rows, dl, flag


@pytest.mark.parametrize("C", [5, 65, 513])
@pytest.mark.parametrize("M", [1, 7])
def test_regularised_cross_entropy_with_leading_dimensions_carries_the_dense_bits(M, C):
    """qarig_cross_entropy_fused_fwd on rows with a leading dimension, with label smoothing and z-loss and with
    soft targets on top (codes = C - 1): the bits of the reg / soft entry on the dense copy, exact +0 pads, nothing
    read or written outside."""
    from qarig import ops
    g = torch.Generator().manual_seed(10 * M + C)
    dense = (torch.randn((M, C), generator=g) * 3).cuda()
    target = torch.randint(0, C, (M,), generator=g).cuda()
    R = 1 if C == 5 else 2                  # codes = 4 holds no window of 2 R + 1 = 5
    w = ops.neighbour_weights(R, R / 2.0, "cuda")
    for entry, nu in (("reg", 0.0), ("soft", 0.2)):
        extra = (nu, R, w) if nu else ()
        loss0, rows0, dl0, flag0 = _ce_pair_call(entry, dense, C, target, M, C, C, 0.1, 1e-4, *extra)
        assert int(flag0) == 0
        for ld in sorted({C, C + 3} | ({528} if C == 513 else set())):
            buf = torch.full((M, ld), float("nan"), device="cuda")     # NaN pads: a read of them would show
            buf[:, :C].copy_(dense)
            loss, rows, dl, flag = _ce_pair_call("fused", buf, ld, target, M, C, ld, 0.1, 1e-4, *extra)
            assert int(flag) == 0
            assert torch.equal(loss, loss0) and not torch.equal(loss[0], loss[1])
            assert torch.equal(rows[:M], rows0[:M]) and torch.equal(rows[M:2 * M], rows0[M:2 * M])
            d2 = dl[:M * ld].view(M, ld)
            assert torch.equal(d2[:, :C], dl0[:M * C].view(M, C))
            assert (d2[:, C:] == 0).all() and not torch.signbit(d2[:, C:]).any()      # exact +0
            assert torch.isnan(dl[M * ld:]).all() and torch.isnan(rows[2 * M:]).all()  # nothing past ld * M, 2 M
            assert torch.isnan(buf[:, C:]).all()


def test_regularised_autograd_node_reads_the_logits_where_they_lie():
    """QF.cross_entropy with regularisers on the [:, :513] slice of a (64, 528) buffer: one strided launch, and the
    loss, the pair and the gradient of the dense call bit for bit."""
    from qarig import functional as QF
    from qarig import ops
    M, C = 64, 513
    g = torch.Generator().manual_seed(33)
    x = (torch.randn((M, C), generator=g) * 3).cuda()
    t = torch.randint(0, C, (M,), generator=g).cuda()
    dense = x.clone().requires_grad_(True)
    want = QF.cross_entropy(dense, t, 0.1, 1e-4)
    want.backward()
    buf = torch.full((M, 528), float("nan"), device="cuda")
    buf[:, :C].copy_(x)
    buf.requires_grad_(True)
    before = ops.RAGGED_CALLS["ce_ld"]
    loss = QF.cross_entropy(buf[:, :C], t, 0.1, 1e-4)
    assert ops.RAGGED_CALLS["ce_ld"] == before + 1
    loss.backward()
    assert torch.equal(loss.detach(), want.detach()) and torch.equal(loss.pair, want.pair)
    assert not torch.equal(loss.pair[0], loss.pair[1])
    assert torch.equal(buf.grad[:, :C], dense.grad)
    assert (buf.grad[:, C:] == 0).all()


def test_input_gradient_over_the_zero_columns_the_loss_writes():
    """dX = dlogits W with K' = K rounded up to 16 (513 -> 528): A is the (M, 528) gradient buffer of the
    cross-entropy entry, its pad columns written by that entry, B a zero-row-padded image of W; against fp64."""
    from qarig import ops
    M, C, Nout = 256, 513, 128
    g = torch.Generator().manual_seed(21)
    buf = torch.full((M, 528), float("nan"), device="cuda")
    buf[:, :C].copy_((torch.randn((M, C), generator=g) * 3).cuda())
    target = torch.randint(0, C, (M,), generator=g).cuda()
    W = (torch.randn((C, Nout), generator=g) * 0.1).cuda()
    Wp = torch.zeros((528, Nout), device="cuda")
    Wp[:C].copy_(W)
    _, dl = ops.cross_entropy_fwd(buf[:, :C], target)
    assert dl.shape == (M, 528)
    dX = ops.gemm(dl, Wp, a_kcontig=True, b_kcontig=False)
    ref = dl[:, :C].double().cpu() @ W.double().cpu()
    assert rel_err(dX, ref) < GEMM_TOL * max(1, 528 / 512) ** 0.5
    assert torch.equal(dX, ops.gemm(dl, Wp, a_kcontig=True, b_kcontig=False))


def _small_step_setup():
    """in_dim 64, hidden 128, 2 layers, K_lr = 16, K_hr = 384 (classifier width 385), 16 latents of 32 x 32 x 4:
    257-token sequences, windows of 256 -> 4,096 rows per step."""
    from models.Codebook import Codebook
    from models.Transformer import Transformer
    from qarig.optim import FlatAdam
    torch.manual_seed(3)
    g = torch.Generator().manual_seed(4)
    lr_cb = Codebook(patch_dim=(32, 32), image_dim=(32, 32), image_channel=4, num_embeddings=16).cuda()
    hr_cb = Codebook(patch_dim=(2, 2), image_dim=(32, 32), image_channel=4, num_embeddings=384).cuda()
    with torch.no_grad():
        lr_cb.codebook.weight.copy_(torch.tanh(torch.randn(lr_cb.codebook.weight.shape, generator=g)))
        hr_cb.codebook.weight.copy_(torch.tanh(torch.randn(hr_cb.codebook.weight.shape, generator=g)))
    m = Transformer(use_encoder=False, use_pos_cond=True, num_enc_layers=None, num_dec_layers=2,
                    num_enc_embedding=None, num_dec_embedding=16 + 384, self_attn_heads=4, cross_attn_heads=None,
                    transformer_in_dim=64, transformer_out_dim=385, transformer_hidden_dim=128).cuda()
    with torch.no_grad():
        for p in m.parameters():
            if p.abs().max() == 0:
                p.copy_((torch.randn(p.shape, generator=g) * 0.05).cuda())
    return lr_cb, hr_cb, m, FlatAdam(m.parameters(), lr=1e-3, betas=(0.5, 0.999))


def test_graphed_steps_equal_eager_steps_on_the_ragged_routes():
    """Three steps through pipeline.GraphedTrainStep (one eager warm-up, the capture, one replay) leave the bits
    of three eager pipeline.train_step calls, and both took the ragged routes."""
    from qarig import ops, pipeline
    g = torch.Generator().manual_seed(9)
    batches = [(torch.tanh(torch.randn((16, 4, 32, 32), generator=g)), torch.randint(0, 257 - 256 + 1, (16,), generator=g))
               for _ in range(3)]
    lr_cb, hr_cb, m, opt_e = _small_step_setup()
    before = dict(ops.RAGGED_CALLS)
    for z, rand in batches:
        hr_in, lr_in, hr_tg = pipeline.tokenize(z.cuda(), lr_cb, hr_cb, True)
        hr_in, hr_tg, pos = pipeline.slide(hr_in, hr_tg, 256, rand)
        assert hr_in.shape == (16, 256)
        pipeline.train_step(m, opt_e, hr_in, lr_in, hr_tg, pos, dp=False, pos_bound=257)
    assert {k: ops.RAGGED_CALLS[k] - before[k] for k in before} == {"forward": 3, "wgrad": 3, "ce_ld": 3}
    lr_cb, hr_cb, m, opt_g = _small_step_setup()
    before = dict(ops.RAGGED_CALLS)
    step = pipeline.GraphedTrainStep(m, opt_g, lr_cb, hr_cb, True, 256, warmup=1)
    for z, rand in batches:
        step(z.cuda(), rand)
    torch.cuda.synchronize()
    assert step.graph is not None
    assert all(ops.RAGGED_CALLS[k] > before[k] for k in before)      # (a replay runs no Python)
    assert torch.equal(opt_g.flat_param.view(torch.int32), opt_e.flat_param.view(torch.int32))
