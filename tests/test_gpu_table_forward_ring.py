"""Training forward of a position table's projections (ScaleLayer / ShiftLayer of every layer, reference
models/layers.py:100-153, 258-304) as ONE strided-groups launch on the fp32 ring
(qarig_gemm_f32_strided), against fp64 and against the skinny launch it replaces; tables whose row
count is no multiple of 128, and no-grad callers, keep the skinny launch and its bits."""
import pytest
import torch

from conftest import grad_err, rel_err

pytestmark = pytest.mark.gpu

GEMM_TOL = 2e-6          # the project's bound for fp32 products: rel_err < 2e-6 * max(1, K/512)^0.5
D = 256


def _operands(G, P, seed):
    g = torch.Generator().manual_seed(seed)
    tab = torch.randn((P, D), generator=g).cuda()
    W = (torch.randn((G, D, D), generator=g) * 0.1).cuda()
    b = torch.randn((G, D), generator=g).cuda()
    return tab, W, b


@pytest.mark.parametrize("P", [128, 384])
@pytest.mark.parametrize("G", [1, 5, 42])
def test_strided_ring_vs_fp64_and_skinny(G, P):
    from qarig import ops
    tab, W, b = _operands(G, P, 100 * G + P)
    tol = GEMM_TOL * max(1, D / 512) ** 0.5
    ref = torch.einsum("pk,gnk->gpn", tab.double().cpu(), W.double().cpu()) + b.double().cpu()[:, None, :]
    assert ops.gemm_strided_supported(P, D, D)
    out = ops.gemm_strided(tab, W, b)
    assert out.shape == (G, P, D)
    for i in range(G):
        assert rel_err(out[i], ref[i]) < tol, i
    skinny = ops.gemm_grouped_skinny(tab, W, b, shared_a=True)
    for i in range(G):
        assert rel_err(out[i], skinny[i]) < 2 * tol, i
    # repeated launch: the same bits
    assert torch.equal(out, ops.gemm_strided(tab, W, b))
    # a group's tiles do not depend on how many groups the launch carries
    last = ops.gemm_strided(tab, W[G - 1:].contiguous(), b[G - 1:].contiguous())
    assert torch.equal(out[G - 1], last[0])
    # no bias
    nb = ops.gemm_strided(tab, W)
    for i in (0, G - 1):
        assert rel_err(nb[i], ref[i] - b[i].double().cpu()) < tol


def test_strided_ring_refuses_what_it_cannot_run():
    from qarig import ops
    tab, W, b = _operands(2, 200, 7)
    assert not ops.gemm_strided_supported(200, D, D)
    with pytest.raises(RuntimeError, match="gemm_strided"):
        ops.gemm_strided(tab, W, b)
    assert not ops.gemm_strided_supported(128, D, 200)       # half a k-tile


def _params(W, b):
    ps = []
    for i in range(W.shape[0]):
        ps += [torch.nn.Parameter(W[i].clone()), torch.nn.Parameter(b[i].clone())]
    return ps


def test_table_projections_training_forward_takes_the_ring():
    """table_projections on 384 rows with gradients wanted and enough projections to fill the chip (258 tiles):
    one strided launch forward; outputs and every gradient against fp64 (1e-5: the bound
    tests/test_gpu_grouped.py uses for gradients)."""
    from qarig import functional as QF
    from qarig import ops
    G, P = 43, 384
    assert ops.table_forward_ring(G, P, D)
    tab, W, b = _operands(G, P, 11)
    tab.requires_grad_(True)
    ps = _params(W, b)
    n0 = ops.STRIDED_CALLS["gemm_strided"]
    outs = QF.table_projections(tab, ps)
    assert ops.STRIDED_CALLS["gemm_strided"] == n0 + 1
    g = torch.Generator().manual_seed(12)
    douts = [torch.randn((P, D), generator=g).cuda() for _ in range(G)]
    torch.autograd.backward(outs, douts)
    tab64 = tab.detach().double().cpu().requires_grad_(True)
    W64 = W.double().cpu().requires_grad_(True)
    b64 = b.double().cpu().requires_grad_(True)
    ref = torch.einsum("pk,gnk->gpn", tab64, W64) + b64[:, None, :]
    ref.backward(torch.stack([d.double().cpu() for d in douts]))
    tol = GEMM_TOL * max(1, D / 512) ** 0.5
    for i in range(G):
        assert rel_err(outs[i], ref[i]) < tol
        assert grad_err(ps[2 * i].grad, W64.grad[i]) < 1e-5
        assert grad_err(ps[2 * i + 1].grad, b64.grad[i]) < 1e-5
    assert grad_err(tab.grad, tab64.grad) < 1e-5


@pytest.mark.parametrize("G,P,grad", [(43, 200, True), (43, 384, False), (5, 384, True)])
def test_table_projections_other_callers_keep_the_skinny_bits(G, P, grad):
    """Rows that are no multiple of 128 (training), no-grad callers at any row count (generation) and launches
    of fewer tiles than the chip has CUs stay on qarig_gemm_grouped_skinny_f32: the same bits as that launch,
    and no strided launch."""
    from qarig import functional as QF
    from qarig import ops
    tab, W, b = _operands(G, P, 13 + P)
    ps = _params(W, b)
    want = ops.gemm_grouped_skinny(tab, W, b, shared_a=True)
    n0 = ops.STRIDED_CALLS["gemm_strided"]
    if grad:
        outs = QF.table_projections(tab, ps)
    else:
        with torch.no_grad():
            outs = QF.table_projections(tab, ps)
    assert ops.STRIDED_CALLS["gemm_strided"] == n0
    for i in range(G):
        assert torch.equal(outs[i].detach(), want[i])
