"""token_score_kernel and score_reduce_kernel (csrc/score.hip) on an MI355X, through their C entries with a flag of
the test's own.  Inputs, references, measures and tolerances: tests/token_score_cases.py (and, through it, the
cross-entropy cases and CE_TOL_U of tests/row_kernel_cases.py, unchanged)."""
import numpy as np
import pytest
import torch

import row_kernel_cases as R
import token_score_cases as T

pytestmark = pytest.mark.gpu


def _score(x, t, ignore=T.IGNORE):
    """qarig_token_score with outputs pre-filled with values it never writes: (row_nll, row_rank, flag)."""
    from qarig import _lib
    M, C = x.shape
    nll = torch.full((M,), -7.0, dtype=torch.float32, device="cuda")
    rank = torch.full((M,), -7, dtype=torch.int32, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    _lib.check(_lib.load().qarig_token_score(_lib.ptr(x), _lib.ptr(t), M, C, ignore, _lib.ptr(nll), _lib.ptr(rank),
                                             _lib.ptr(flag), _lib.stream()), "qarig_token_score")
    return nll, rank, int(flag.item())


@pytest.mark.parametrize("C", R.CE_CLASSES)
def test_token_score_rows(C):
    c = R.ce_case(R.CE_M, C)
    x, t = c.x.cuda(), c.t.cuda()
    got = {}

    def impl(xc, tc):
        nll, rank, flag = _score(x, t)
        assert flag == 0
        got["nll"], got["rank"] = nll, rank
        return nll.cpu(), rank.cpu()

    notes = []
    bad = T.score_failures(impl, classes=(C,), notes=notes)
    for _, fam, w in notes:
        print(f"token_score C={C} {fam}: row_nll {w:.3f} u (tolerance {R.CE_TOL_U[('loss', fam)]})")
    assert not bad, bad
    nll, rank = got["nll"], got["rank"]
    ref_rank = T.score_ref(c.x, c.t)[1]
    assert torch.equal(rank.cpu(), ref_rank)
    ties = c.rows("ties")
    assert torch.equal(rank.cpu()[ties].long(), c.t[ties])
    assert torch.isfinite(nll).all()
    # the same bits on a second launch, and through the wrapper
    nll2, rank2, _ = _score(x, t)
    assert torch.equal(nll, nll2) and torch.equal(rank, rank2)
    from qarig import ops
    nll3, rank3 = ops.token_score(x, t)
    assert torch.equal(nll, nll3) and torch.equal(rank, rank3)

    # skipped rows: (0, -1), no flag, every other row unchanged
    nll_s, rank_s, flag_s = _score(x, T.skipped_targets(c).cuda())
    skip = list(T.SKIP_ROWS)
    keep = [r for r in range(c.M) if r not in skip]
    assert flag_s == 0
    assert (nll_s[skip] == 0).all() and (rank_s[skip] == -1).all()
    assert torch.equal(nll_s[keep], nll[keep]) and torch.equal(rank_s[keep], rank[keep])

    # t = C and t = -1: (0, -1) and the flag
    nll_b, rank_b, flag_b = _score(x, c.bad_targets().cuda())
    badr = list(R.CE_BAD_ROWS)
    keep = [r for r in range(c.M) if r not in badr]
    assert flag_b == 1
    assert (nll_b[badr] == 0).all() and (rank_b[badr] == -1).all()
    assert torch.equal(nll_b[keep], nll[keep]) and torch.equal(rank_b[keep], rank[keep])

    # a NaN in one row: every other row bit-unchanged
    xn = c.x.clone()
    xn[T.NAN_ROW, C // 2] = float("nan")
    nll_n, rank_n, flag_n = _score(xn.cuda(), t)
    keep = [r for r in range(c.M) if r != T.NAN_ROW]
    assert flag_n == 0
    assert torch.equal(nll_n[keep], nll[keep]) and torch.equal(rank_n[keep], rank[keep])


def _reduce(nll, rank, N, S, pos0, P, acc=None, topk=T.TOPK):
    from qarig import ops
    if acc is None:
        acc = (torch.zeros(N, dtype=torch.float64, device="cuda"), torch.zeros(P, dtype=torch.float64, device="cuda"),
               torch.zeros(P, dtype=torch.int64, device="cuda"), torch.zeros(3, dtype=torch.int64, device="cuda"))
    ops.score_reduce(nll, rank, N, S, pos0, topk, *acc)
    return acc


@pytest.mark.parametrize("N,S,pos0,P", T.REDUCE_SHAPES)
def test_score_reduce(N, S, pos0, P):
    nll, rank = T.reduce_inputs(N, S, "int")
    want = T.reduce_ref(nll, rank, N, S, pos0, P)
    nd, rd = nll.cuda(), rank.cuda()
    acc = _reduce(nd, rd, N, S, pos0, P)
    for g, w in zip(acc, want):
        assert np.array_equal(g.cpu().numpy(), w)
    _reduce(nd, rd, N, S, pos0, P, acc)                     # the accumulators add: a second call doubles them
    for g, w in zip(acc, want):
        assert np.array_equal(g.cpu().numpy(), 2 * w)
    # rows not 16-byte aligned: the total counts' scalar path
    if N * S > 1:
        pad_n = torch.cat((torch.zeros(1), nll)).cuda()[1:]
        pad_r = torch.cat((torch.zeros(1, dtype=torch.int32), rank)).cuda()[1:]
        for g, w in zip(_reduce(pad_n, pad_r, N, S, pos0, P), want):
            assert np.array_equal(g.cpu().numpy(), w)

    nll, rank = T.reduce_inputs(N, S, "gauss")
    nd, rd = nll.cuda(), rank.cuda()
    a, b = _reduce(nd, rd, N, S, pos0, P), _reduce(nd, rd, N, S, pos0, P)
    for g, h in zip(a, b):
        assert torch.equal(g, h)                            # two fresh runs: the same bits
    want = T.reduce_ref(nll, rank, N, S, pos0, P)
    (img_exact, img_bound), (col_exact, col_bound) = T.reduce_exact_and_bound(nll, N, S)
    img, pos = a[0].cpu().numpy(), a[1].cpu().numpy()
    print(f"score_reduce {(N, S)}: img err / bound {np.max(np.abs(img - img_exact) / np.maximum(img_bound, 1e-300)):.3f}, "
          f"pos err / bound {np.max(np.abs(pos[pos0:pos0 + S] - col_exact) / np.maximum(col_bound, 1e-300)):.3f}")
    assert (np.abs(img - img_exact) <= img_bound).all() and (np.abs(img - want[0]) <= img_bound).all()
    assert (np.abs(pos[pos0:pos0 + S] - col_exact) <= col_bound).all()
    assert (np.abs(pos - want[1])[pos0:pos0 + S] <= col_bound).all()
    assert (pos[:pos0] == 0).all() and (pos[pos0 + S:] == 0).all()
    assert np.array_equal(a[2].cpu().numpy(), want[2]) and np.array_equal(a[3].cpu().numpy(), want[3])
