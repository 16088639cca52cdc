"""CPU half of the held-out evaluation tests: the fp64 reference of tests/token_score_cases.py against a stable
sort, the three mutants rejected by the GPU test's own inputs, pipeline.eval_windows counting every position once,
and the two new C-ABI entries refusing bad arguments without a device."""
import ctypes

import numpy as np
import pytest
import torch

import row_kernel_cases as R
import token_score_cases as T


@pytest.mark.parametrize("C", R.CE_CLASSES)
def test_reference_rank_is_the_place_in_a_stable_descending_sort(C):
    c = R.ce_case(R.CE_M, C)
    nll, rank = T.score_ref(c.x, c.t)
    assert torch.equal(rank, T.rank_by_argsort(c.x, c.t))
    ties = c.rows("ties")
    assert torch.equal(rank[ties].long(), c.t[ties])          # all logits equal: the smaller indices go first
    for r in c.rows("masked"):                                # -inf entries never count
        finite = torch.isfinite(c.x[r])
        assert int(rank[r]) == int(((c.x[r] > c.x[r, c.t[r]]) & finite).sum())
    assert torch.isfinite(nll).all() and (nll >= 0).all()
    # skipped and out-of-range targets
    nll_s, rank_s = T.score_ref(c.x, T.skipped_targets(c))
    skip = list(T.SKIP_ROWS)
    assert (nll_s[skip] == 0).all() and (rank_s[skip] == -1).all()
    nll_b, rank_b = T.score_ref(c.x, c.bad_targets())
    assert (nll_b[list(R.CE_BAD_ROWS)] == 0).all() and (rank_b[list(R.CE_BAD_ROWS)] == -1).all()


def test_intended_arithmetic_passes_and_every_mutant_is_rejected():
    notes = []
    assert T.score_failures(T.score_emulate, notes=notes) == []
    assert len(notes) == len(R.CE_CLASSES) * len(R.CE_FAMILIES)
    for m in T.MUTANTS:
        bad = T.score_failures(lambda x, t: T.score_emulate(x, t, m))
        assert bad, f"mutant {m} passes the GPU test's inputs"
        if m != "drop_tail":
            assert "ties" in {b[1] for b in bad} and {b[2] for b in bad} == {"rank"}, (m, bad)
        else:
            assert any(b[2] == "rank" for b in bad) and any(b[2] == "nll" for b in bad), bad


@pytest.mark.parametrize("L,W", [(4, 4), (5, 4), (8, 4), (9, 4), (11, 4), (3, None)])
def test_eval_windows_cover_every_position_once(L, W):
    from qarig import pipeline
    wins = pipeline.eval_windows(L, W)
    if W is None or W >= L:
        assert wins == [(None, 0)]
        return
    assert len(wins) == -(-L // W)
    seen = np.zeros(L, dtype=int)
    for k, (start, skip) in enumerate(wins):
        assert start == min(k * W, L - W) and skip == k * W - start
        assert 0 <= start and start + W <= L and 0 <= skip < W
        seen[start + skip:start + W] += 1
    assert (seen == 1).all()


def test_eval_windows_longer_than_the_sequence():
    from qarig import pipeline
    assert pipeline.eval_windows(4, 9) == [(None, 0)]


def test_reduce_reference_is_consistent():
    for N, S, pos0, P in T.REDUCE_SHAPES:
        nll, rank = T.reduce_inputs(N, S, "int")
        assert (rank == -1).any() or N * S == 1
        img, pos, cnt, tot = T.reduce_ref(nll, rank, N, S, pos0, P)
        assert img.sum() == pos.sum() == float(nll.double().sum())
        assert cnt.sum() == tot[0] == int((rank >= 0).sum()) and tot[1] <= tot[2] <= tot[0]
        assert (pos[:pos0] == 0).all() and (pos[pos0 + S:] == 0).all()


def test_new_entries_refuse_bad_arguments_without_a_device():
    from qarig import _lib
    h = _lib.load()
    X = 0x7f0000000000
    assert h.qarig_token_score(None, None, 4, 8, -100, None, None, None, None) == -1
    assert "token_score" in _lib.last_error()
    for nulled in (0, 1, 5, 6, 7):
        a = [X, X, 4, 8, -100, X, X, X, None]
        a[nulled] = None
        assert h.qarig_token_score(*a) == -1
    assert h.qarig_token_score(X, X, 0, 8, -100, X, X, X, None) == -1
    assert h.qarig_token_score(X, X, 4, 2 ** 25, -100, X, X, X, None) == -1
    assert h.qarig_score_reduce(None, None, 2, 3, 0, 3, 5, None, None, None, None, None) == -1
    assert "score_reduce" in _lib.last_error()
    for nulled in (0, 1, 7, 8, 9, 10):
        a = [X, X, 2, 3, 0, 3, 5, X, X, X, X, None]
        a[nulled] = None
        assert h.qarig_score_reduce(*a) == -1
    for N, S, pos0, P, topk in ((0, 3, 0, 3, 5), (2, 0, 0, 3, 5), (2, 3, 1, 3, 5), (2, 3, -1, 3, 5), (2, 3, 0, 2, 5),
                                (2, 3, 0, 3, -1), (2 ** 20, 2 ** 20, 0, 2 ** 20, 5), (2, 3, 0, 2 ** 25, 5)):
        assert h.qarig_score_reduce(X, X, N, S, pos0, P, topk, X, X, X, X, None) == -1, (N, S, pos0, P, topk)
    assert isinstance(h.qarig_score_reduce, ctypes._CFuncPtr)
