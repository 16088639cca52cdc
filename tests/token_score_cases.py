"""References, mutants and inputs shared by tests/test_gpu_token_score.py (token_score_kernel / score_reduce_kernel
of csrc/score.hip on an MI355X) and tests/test_token_score_host.py (the same pieces on the CPU).

TOKEN SCORE.  The inputs are the (37, C) cross-entropy cases of tests/row_kernel_cases.py, C = 3 ... 8193, families
unit / offset / peak_target / peak_other / ties / masked, targets at column 0, at C - 1 and inside the last
64-chunk.  row_nll is judged like the cross-entropy kernel's row loss -- the kernel repeats its arithmetic --
against the fp64 log-sum-exp of the fp32 inputs, |err| / (u max(1, ref)) <= CE_TOL_U[('loss', family)], u = 2^-24.
row_rank is an integer and must equal #{c : x[c] > x[t]} + #{c < t : x[c] == x[t]} exactly: `ties` rows (all logits
equal) give t, -inf entries of `masked` rows never count.

MUTANTS (`MUTANTS`; the host test proves each is rejected by these inputs): the rank counted with >= (every tie
ahead of the target), ties broken to the larger index, and a sweep that drops the last partial 64-chunk of a row
(from the maximum, the sum and the rank).

SCORE REDUCE.  Shapes (N, S, pos0, P): one element; a window inside a longer sequence; S past four 64-lane trips with
a tail; N past one trip.  Small-integer nll sums are exact in fp64, so every output must EQUAL numpy.  On Gaussian
nll an n-term sum of the kernel makes at most n - 1 roundings, each at most 2^-53 of a partial sum that sum |v|
bounds, and the correctly rounded reference (math.fsum) one more: n 2^-53 sum |v| in all."""
import math

import numpy as np
import torch

import row_kernel_cases as R

IGNORE = -100
SKIP_ROWS = (0, 11, 36)                     # rows that get target == IGNORE in the skipped-row run
NAN_ROW = 17
MUTANTS = ("rank_ge", "ties_to_larger", "drop_tail")
REDUCE_SHAPES = ((1, 1, 0, 1), (3, 5, 2, 9), (5, 257, 0, 257), (70, 3, 0, 3))
TOPK = 5


def score_ref(x, t, ignore=IGNORE):
    """fp64 nll (M,) and the rank by its definition (M,) int32; (0, -1) for skipped and out-of-range targets."""
    M, C = x.shape
    ok = (t >= 0) & (t < C) & (t != ignore)
    tt = t.clamp(0, C - 1)
    rows = torch.arange(M)
    xt = x[rows, tt]
    nll = torch.logsumexp(x.double(), 1) - xt.double()
    cols = torch.arange(C)[None]
    rank = (x > xt[:, None]).sum(1) + ((x == xt[:, None]) & (cols < tt[:, None])).sum(1)
    return torch.where(ok, nll, torch.zeros_like(nll)), torch.where(ok, rank, -torch.ones_like(rank)).int()


def rank_by_argsort(x, t):
    """Place of the target in a STABLE descending sort of the row: equal logits keep their index order."""
    order = torch.argsort(x, dim=1, descending=True, stable=True)
    return (order == t[:, None]).int().argmax(1).int()


def score_emulate(x, t, mutant=None):
    """token_score_kernel on the CPU: the nll of row_kernel_cases.ce_emulate (the cross-entropy row kernel's fp32 arithmetic,
    which the kernel repeats) and the rank as the sweep counts it; `mutant` one of MUTANTS."""
    drop = mutant == "drop_tail"
    nll = R.ce_emulate(x, t, "drop_tail" if drop else None)[0]
    xs = R._drop_tail(x, -math.inf) if drop else x
    xt = x[torch.arange(x.shape[0]), t][:, None]
    cols, tc = torch.arange(x.shape[1])[None], t[:, None]
    if mutant == "rank_ge":
        rank = ((xs >= xt) & (cols != tc)).sum(1)
    elif mutant == "ties_to_larger":
        rank = (xs > xt).sum(1) + ((xs == xt) & (cols > tc)).sum(1)
    else:
        rank = (xs > xt).sum(1) + ((xs == xt) & (cols < tc)).sum(1)
    return nll, rank.int()


def score_failures(impl, classes=R.CE_CLASSES, notes=None):
    """What the GPU test asserts about row_nll and row_rank, run on an implementation (x, t) -> (nll fp32, rank):
    a list of (C, family, what, figure) it would fail.  notes (a list) receives every (C, family, worst u)."""
    bad = []
    for C in classes:
        c = R.ce_case(R.CE_M, C)
        nll, rank = impl(c.x, c.t)
        ref_nll, ref_rank = score_ref(c.x, c.t)
        e = (nll.double() - ref_nll).abs() / (R.U * ref_nll.clamp_min(1.0))
        for fam in R.CE_FAMILIES:
            r = c.rows(fam)
            w = float(e[r].max())
            if notes is not None:
                notes.append((C, fam, w))
            if not R.within(w, R.CE_TOL_U[("loss", fam)]):
                bad.append((C, fam, "nll", w))
            wrong = int((rank[r] != ref_rank[r]).sum())
            if wrong:
                bad.append((C, fam, "rank", wrong))
    return bad


def skipped_targets(c):
    t = c.t.clone()
    t[list(SKIP_ROWS)] = IGNORE
    return t


def reduce_inputs(N, S, kind):
    """row_nll fp32 (N S,) -- small non-negative integers ("int") or Gaussian ("gauss") -- and row_rank int32 in
    -1 ... 9, a sixth of them -1; rows with rank -1 carry nll 0, as token_score writes them."""
    gen = R._gen("score_reduce", N, S, kind)
    M = N * S
    rank = torch.randint(-1, 10, (M,), generator=gen).int()
    rank[torch.rand(M, generator=gen) < 1.0 / 6.0] = -1
    if kind == "int":
        nll = torch.randint(0, 8, (M,), generator=gen).float()
    else:
        nll = torch.randn(M, generator=gen) * 3.0
    nll[rank < 0] = 0.0
    return nll, rank


def reduce_ref(nll, rank, N, S, pos0, P, topk=TOPK):
    """numpy fp64 / int64: img_nll (N,), pos_nll (P,), pos_cnt (P,), totals (3,)."""
    v = nll.numpy().astype(np.float64).reshape(N, S)
    r = rank.numpy().reshape(N, S)
    pos_nll, pos_cnt = np.zeros(P), np.zeros(P, dtype=np.int64)
    pos_nll[pos0:pos0 + S] = v.sum(0)
    pos_cnt[pos0:pos0 + S] = (r >= 0).sum(0)
    totals = np.array([(r >= 0).sum(), (r == 0).sum(), ((r >= 0) & (r < topk)).sum()], dtype=np.int64)
    return v.sum(1), pos_nll, pos_cnt, totals


def reduce_exact_and_bound(nll, N, S):
    """Per image and per column: the correctly rounded sum (math.fsum) and the bound n 2^-53 sum |v|."""
    v = nll.numpy().astype(np.float64).reshape(N, S)
    img = np.array([math.fsum(row) for row in v]), S * 2.0 ** -53 * np.abs(v).sum(1)
    col = np.array([math.fsum(c) for c in v.T]), N * 2.0 ** -53 * np.abs(v).sum(0)
    return img, col
