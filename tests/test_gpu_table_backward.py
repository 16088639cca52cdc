"""The backward kernels with the table sums inside (layernorm_bwd_table_kernel, mul_rows_bwd_table_kernel of
csrc/condtable.hip) against the composition they replace -- ops.layernorm_bwd(want_dy_xhat=True) + two
ops.segment_sum, ops.mul_rows_bwd + ops.segment_sum --, bit for bit, and against fp64.

SHAPES.  D in {256, 512} (one and two 16-B loads per lane and row), 150 token rows over P = 14 table positions whose
token counts are 0, 1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 31, 47, 0: empty first, middle-free and last positions, fewer
tokens than the 8 waves of a workgroup, and every remainder of the 4 sub-groups x 2 accumulators a position's tokens
are dealt to.  The index vector is shuffled, so no position's tokens are contiguous.  The rows are the off-unit-scale
families of tests/row_kernel_cases.py (unit, offset, scaled, const).

FP64 BOUNDS.  dx per row: row_kernel_cases.LN_TOL_U, as tests/test_gpu_row_kernels.py judges layernorm_bwd.  The
tables have no entry there; with u = 2^-24, n the position's token count and t the per-token terms:
  dshift[p] = sum dy            the terms are exact, n - 1 adds round:       |err| <= n u sum |dy|
  dscale[p] = sum dy xhat       each term within LN_TOL_U[dy_xhat] of its row's scale, then the adds:
                                |err| <= u (sum_r tol_r max_c |t_r| + n sum_r |t_r|)
  da = dy tab[p]                one rounding:                                |err| <= u |ref|
  dg[p] = sum dy a              each product rounds once, then the adds:     |err| <= (n + 1) u sum |dy a|
(first-order bounds with the worst-case n instead of the pairwise depth: generous in n, exact zeros stay exact)."""
import types

import pytest
import torch

import row_kernel_cases as R

pytestmark = pytest.mark.gpu

P = 14
COUNTS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 31, 47, 0)
M = sum(COUNTS)
WIDTHS = (256, 512)
U = R.U


class Case:
    def __init__(self, D):
        self.c = c = R.LNCase(D, M, "table_bwd", R.DEC_FAMILIES)
        gen = torch.Generator().manual_seed(1000 + D)
        idx = torch.cat([torch.full((n,), p, dtype=torch.int32) for p, n in enumerate(COUNTS)])
        self.idx = idx[torch.randperm(M, generator=gen)].contiguous()
        for p, n in enumerate(COUNTS):
            if n > 2:       # shuffled: the position's tokens are not one run
                t = (self.idx == p).nonzero().flatten()
                assert int(t[-1] - t[0]) >= n
        self.scale_tab = torch.randn((P, D), generator=gen) * 0.5 + 1.0
        self.shift_tab = torch.randn((P, D), generator=gen)
        self.gate_tab = torch.randn((P, D), generator=gen) * 0.5 + 1.0
        self.dy = c.dy["full"] * torch.exp2(torch.randint(-8, 9, (M, 1), generator=gen).float())
        self.a = c.x                       # the gate's other operand: the same off-unit-scale rows
        self.dx_add = c.dx_add


_CASES = {}


def case(D):
    if D not in _CASES:
        _CASES[D] = Case(D)
    return _CASES[D]


def _segment64(t, idx):
    """(P, D) fp64 sums of the rows of t per position, and of their absolute values."""
    out = torch.zeros((P, t.shape[1]), dtype=torch.float64)
    mag = torch.zeros_like(out)
    out.index_add_(0, idx.long(), t.double())
    mag.index_add_(0, idx.long(), t.double().abs())
    return out, mag


def _cond(idx, P_rows):
    from qarig import ops
    offsets, rows = ops.rowmap_build(idx, P_rows)
    return types.SimpleNamespace(idx=idx, offsets=offsets, rows=rows)


@pytest.mark.parametrize("with_add", (False, True), ids=("plain", "dx_add"))
@pytest.mark.parametrize("D", WIDTHS)
def test_layernorm_bwd_table(D, with_add):
    from qarig import ops
    k = case(D)
    c = k.c
    x, dy, st, sh = c.x.cuda(), k.dy.cuda(), k.scale_tab.cuda(), k.shift_tab.cuda()
    idx = k.idx.cuda()
    add = k.dx_add.cuda() if with_add else None
    cond = _cond(idx, P)
    _, mean, rstd = ops.layernorm_fwd(x, scale=st, shift=sh, mod_idx=idx)
    # the parent composition
    dx0, dyx = ops.layernorm_bwd(dy, x, mean, rstd, scale=st, want_dy_xhat=True, mod_idx=idx, dx_add=add)
    dscale0 = ops.segment_sum(dyx, cond.offsets, cond.rows)
    dshift0 = ops.segment_sum(dy, cond.offsets, cond.rows)
    assert ops.table_bwd_fused(M, P, D, dy, x, st, add)
    dx, dscale, dshift = ops.layernorm_bwd_table(dy, x, mean, rstd, st, cond.offsets, cond.rows, dx_add=add)
    assert torch.equal(dx, dx0), "dx differs from layernorm_bwd"
    assert torch.equal(dscale, dscale0), "dscale differs from segment_sum(dy * xhat)"
    assert torch.equal(dshift, dshift0), "dshift differs from segment_sum(dy)"
    empty = [p for p, n in enumerate(COUNTS) if n == 0]
    assert (dscale[empty] == 0).all() and (dshift[empty] == 0).all()
    again = ops.layernorm_bwd_table(dy, x, mean, rstd, st, cond.offsets, cond.rows, dx_add=add)
    assert all(torch.equal(a, b) for a, b in zip((dx, dscale, dshift), again)), "two launches differ"
    # fp64 on the same inputs
    mul = k.scale_tab[k.idx.long()]
    rdx, rdh = R.ln_bwd_ref(c.x, k.dy, mul, k.dx_add if with_add else None)
    errs = R.ln_measures(c.x, {"dx": dx.cpu()}, {"dx": rdx})["dx"]
    bad = []
    for fam in sorted(set(c.family)):
        w = float(errs[c.rows(fam)].max())
        print(f"MEASURED layernorm_bwd_table dx {fam} {w:.3f} {R.LN_TOL_U[('dx', fam)]}")
        if not R.within(w, R.LN_TOL_U[("dx", fam)]):
            bad.append((fam, w))
    assert not bad, (D, with_add, bad)
    n = torch.tensor(COUNTS, dtype=torch.float64)[:, None]
    ref_shift, mag_shift = _segment64(k.dy, k.idx)
    e = (dshift.cpu().double() - ref_shift).abs()
    bound = n * U * mag_shift
    print(f"MEASURED layernorm_bwd_table dshift worst/bound {float((e / bound.clamp_min(1e-300)).max()):.4f}")
    assert (e <= bound).all()
    ref_scale, mag_scale = _segment64(rdh, k.idx)
    tol = torch.tensor([R.LN_TOL_U[("dy_xhat", f)] for f in c.family], dtype=torch.float64)
    per_row = torch.zeros(P, dtype=torch.float64).index_add_(0, k.idx.long(), tol * rdh.abs().max(1).values)
    e = (dscale.cpu().double() - ref_scale).abs()
    bound = U * (per_row[:, None] + n * mag_scale)
    print(f"MEASURED layernorm_bwd_table dscale worst/bound {float((e / bound.clamp_min(1e-300)).max()):.4f}")
    assert (e <= bound).all()


@pytest.mark.parametrize("D", WIDTHS)
def test_mul_rows_bwd_table(D):
    from qarig import ops
    k = case(D)
    dy, a, gt, idx = k.dy.cuda(), k.a.cuda(), k.gate_tab.cuda(), k.idx.cuda()
    cond = _cond(idx, P)
    da0, dg_tok = ops.mul_rows_bwd(dy, a, gt, idx)
    dg0 = ops.segment_sum(dg_tok, cond.offsets, cond.rows)
    da, dg = ops.mul_rows_bwd_table(dy, a, gt, cond.offsets, cond.rows)
    assert torch.equal(da, da0), "da differs from mul_rows_bwd"
    assert torch.equal(dg, dg0), "dg differs from segment_sum(dy * a)"
    empty = [p for p, n in enumerate(COUNTS) if n == 0]
    assert (dg[empty] == 0).all()
    again = ops.mul_rows_bwd_table(dy, a, gt, cond.offsets, cond.rows)
    assert torch.equal(da, again[0]) and torch.equal(dg, again[1]), "two launches differ"
    ref_da = k.dy.double() * k.gate_tab[k.idx.long()].double()
    e = (da.cpu().double() - ref_da).abs()
    print(f"MEASURED mul_rows_bwd_table da worst u {float((e / (U * ref_da.abs()).clamp_min(1e-300)).max()):.4f}")
    assert (e <= U * ref_da.abs()).all()
    prod = k.dy.double() * k.a.double()
    ref_dg = torch.zeros((P, D), dtype=torch.float64).index_add_(0, k.idx.long(), prod)
    mag = torch.zeros((P, D), dtype=torch.float64).index_add_(0, k.idx.long(), prod.abs())
    n = torch.tensor(COUNTS, dtype=torch.float64)[:, None]
    e = (dg.cpu().double() - ref_dg).abs()
    bound = (n + 1) * U * mag
    print(f"MEASURED mul_rows_bwd_table dg worst/bound {float((e / bound.clamp_min(1e-300)).max()):.4f}")
    assert (e <= bound).all()


@pytest.mark.parametrize("D", WIDTHS)
def test_autograd_nodes_take_the_fused_path_and_fall_back_below_the_threshold(D):
    """Through qarig.functional: at M / P above ops.TABLE_BWD_MIN_TOKENS_PER_ROW both nodes count a fused call, with
    the same tokens spread over a table too long for that (the extra positions empty) a two-step call; both give the
    parent composition's bits."""
    from qarig import functional as QF
    from qarig import ops
    k = case(D)
    c = k.c
    idx = k.idx.cuda()
    dy, dskip = k.dy.cuda(), k.dx_add.cuda()
    long_P = M // ops.TABLE_BWD_MIN_TOKENS_PER_ROW + 1 + P
    assert M >= ops.TABLE_BWD_MIN_TOKENS_PER_ROW * P and M < ops.TABLE_BWD_MIN_TOKENS_PER_ROW * long_P
    for rows_P, path in ((P, "fused"), (long_P, "two_step")):
        pad = torch.zeros((rows_P - P, D))
        st = torch.cat((k.scale_tab, pad)).cuda().requires_grad_(True)
        sh = torch.cat((k.shift_tab, pad)).cuda().requires_grad_(True)
        gt = torch.cat((k.gate_tab, pad)).cuda().requires_grad_(True)
        x = c.x.cuda().requires_grad_(True)
        cond = _cond(idx, rows_P)
        before = dict(QF.TABLE_BWD_CALLS)
        y, skip = QF.layernorm_mod_table(x, st, sh, cond, with_skip=True)
        dx, dscale, dshift = torch.autograd.grad((y, skip), (x, st, sh), (dy, dskip))
        z = QF.mul_table(x, gt, cond)
        da, dg = torch.autograd.grad(z, (x, gt), dy)
        other = "two_step" if path == "fused" else "fused"
        assert QF.TABLE_BWD_CALLS[path] == before[path] + 2 and QF.TABLE_BWD_CALLS[other] == before[other], \
            (rows_P, path, before, QF.TABLE_BWD_CALLS)
        xd, std, gtd = x.detach(), st.detach(), gt.detach()
        _, mean, rstd = ops.layernorm_fwd(xd, scale=std, shift=sh.detach(), mod_idx=idx)
        dx0, dyx = ops.layernorm_bwd(dy, xd, mean, rstd, scale=std, want_dy_xhat=True, mod_idx=idx, dx_add=dskip)
        assert torch.equal(dx, dx0)
        assert torch.equal(dscale, ops.segment_sum(dyx, cond.offsets, cond.rows))
        assert torch.equal(dshift, ops.segment_sum(dy, cond.offsets, cond.rows))
        da0, dg_tok = ops.mul_rows_bwd(dy, xd, gtd, idx)
        assert torch.equal(da, da0) and torch.equal(dg, ops.segment_sum(dg_tok, cond.offsets, cond.rows))
        assert (dscale[P:] == 0).all() and (dshift[P:] == 0).all() and (dg[P:] == 0).all()
