"""qarig.sampling.filter_probs -- the one definition of top-k / nucleus (top-p) filtering every sampling path
uses, and the reference of the GPU tests -- against an independent numpy restatement (explicit loops over a
descending order with ties at the lower index).  No GPU."""
import math

import numpy as np
import pytest
import torch


def np_filter(p, top_k, top_p):
    """The definition, row by row: zero everything but the top_k largest non-zero entries (ties: lower index
    first); of those, in descending order, keep an entry iff the normalised mass strictly in front of it is
    < top_p.  Kept entries keep their values."""
    p = np.asarray(p, dtype=np.float64)
    out = np.array(p)
    for r in range(p.shape[0]):
        row = out[r]
        if top_k > 0:
            order = sorted(range(len(row)), key=lambda i: (-row[i], i))
            nz = [i for i in order if row[i] > 0]
            for i in nz[top_k:]:
                row[i] = 0.0
        if top_p < 1.0:
            order = sorted(range(len(row)), key=lambda i: (-row[i], i))
            nz = [i for i in order if row[i] > 0]
            total = sum(row[i] for i in nz)
            before = 0.0
            for n, i in enumerate(nz):
                keep = n == 0 or before / total < top_p
                before += row[i]
                if not keep:
                    row[i] = 0.0
    return out


def _rows(V, B=5, seed=0, end=None):
    g = torch.Generator().manual_seed(seed)
    p = torch.softmax(torch.randn((B, V), generator=g, dtype=torch.float64) * 3 / 0.7, dim=1)
    if end is not None:
        p[:, end] = 0.0
    return p


@pytest.mark.parametrize("V", [7, 41, 300])
@pytest.mark.parametrize("top_k,top_p", [(1, 1.0), (5, 1.0), (10 ** 6, 1.0), (0, 0.3), (0, 0.9), (0, 1.0),
                                         (5, 0.9), (3, 0.3), (50, 0.9), (1, 0.3)])
def test_filter_probs_is_the_definition(V, top_k, top_p):
    from qarig.sampling import filter_probs
    p = _rows(V, seed=V, end=V - 1)
    if top_k >= 10 ** 6:
        top_k = V + 3                                  # at least V: nothing to do
    got = filter_probs(p.clone(), top_k, top_p)
    want = np_filter(p.numpy(), top_k, top_p)
    assert np.array_equal(got.numpy(), want)           # only zeroing: surviving values are untouched
    nnz = (got > 0).sum(dim=1)
    assert (nnz >= 1).all()
    if top_k > 0:
        assert (nnz <= top_k).all()
    if top_p == 1.0 and top_k > 0:
        assert (nnz == min(top_k, V - 1)).all()
    # fp32 rows and a leading batch shape go through the same code
    got32 = filter_probs(p.float().reshape(1, *p.shape), top_k, top_p)
    assert got32.shape == (1, *p.shape) and got32.dtype == torch.float32
    if top_p == 1.0:                                   # (a cut on the mass may round differently in fp32)
        assert ((got32[0] > 0) == (got > 0)).all()
    assert torch.equal(got32[got32 > 0], p.float().reshape(1, *p.shape)[got32 > 0])


def test_equal_entries_go_to_the_lower_index():
    from qarig.sampling import filter_probs
    V, end = 41, 40
    p = torch.full((2, V), 1.0 / V, dtype=torch.float64)
    p[:, end] = 0.0                                     # generate mode: <end> zeroed, 40 equal entries
    k5 = filter_probs(p.clone(), 5, 1.0)
    assert (k5[:, :5] == 1.0 / V).all() and not k5[:, 5:].any()
    # q = 1/40 each: the mass in front of index 19 is 0.475 < 0.49, in front of index 20 it is 0.5
    p49 = filter_probs(p.clone(), 0, 0.49)
    assert (p49[:, :20] == 1.0 / V).all() and not p49[:, 20:].any()
    both = filter_probs(p.clone(), 5, 0.49)             # q = 1/5 each: 0, 0.2, 0.4 are < 0.49
    assert (both[:, :3] == 1.0 / V).all() and not both[:, 3:].any()
    assert np.array_equal(both.numpy(), np_filter(p.numpy(), 5, 0.49))
    # train mode: <end> is one of the equal entries
    t = torch.full((1, V), 1.0 / V, dtype=torch.float64)
    assert np.array_equal(filter_probs(t.clone(), 0, 0.49).numpy(), np_filter(t.numpy(), 0, 0.49))
    assert int((filter_probs(t.clone(), 0, 0.49) > 0).sum()) == 21          # 20 / 41 < 0.49 <= 21 / 41
    # ties in the middle of a row: the cut falls inside a run of equal values
    r = torch.tensor([[0.1, 0.2, 0.1, 0.2, 0.1, 0.2, 0.1, 0.0]], dtype=torch.float64)
    assert filter_probs(r.clone(), 2, 1.0).tolist() == [[0.0, 0.2, 0.0, 0.2, 0.0, 0.0, 0.0, 0.0]]
    assert filter_probs(r.clone(), 5, 1.0).tolist() == [[0.1, 0.2, 0.1, 0.2, 0.0, 0.2, 0.0, 0.0]]


def test_single_entry_and_at_least_one_survivor():
    from qarig.sampling import filter_probs
    one = torch.zeros((1, 9), dtype=torch.float64)
    one[0, 6] = 0.25
    for k, p_ in ((1, 1.0), (4, 1.0), (0, 0.01), (3, 1e-9), (0, 0.999)):
        assert torch.equal(filter_probs(one.clone(), k, p_), one)
    p = _rows(33, seed=1)
    tiny = filter_probs(p.clone(), 0, 1e-12)            # a nucleus smaller than the largest entry: that entry stays
    assert ((tiny > 0).sum(dim=1) == 1).all()
    assert torch.equal(tiny.argmax(dim=1), p.argmax(dim=1))
    assert torch.equal(tiny.max(dim=1).values, p.max(dim=1).values)


def test_off_returns_the_input_untouched():
    from qarig.sampling import filter_probs
    p = _rows(17, seed=2)
    keep = p.clone()
    assert filter_probs(p, 0, 1.0) is p and filter_probs(p) is p and torch.equal(p, keep)
    out = filter_probs(p, 3, 0.5)                       # and a filtered call does not write into its input
    assert out is not p and torch.equal(p, keep)


@pytest.mark.parametrize("top_k,top_p", [(-1, 1.0), (0, 0.0), (0, 1.5), (0, -0.1), (0, math.nan), (2.5, 1.0),
                                         (-3, 0.5)])
def test_invalid_values_raise(top_k, top_p):
    from qarig.sampling import filter_probs, generate_tokens
    with pytest.raises(ValueError):
        filter_probs(torch.ones(1, 4) / 4, top_k, top_p)
    with pytest.raises(ValueError):                    # refused before anything touches the model or a device
        generate_tokens(None, torch.zeros((1, 1), dtype=torch.int64), None, 4, 1.0, False, 8, end_token=3,
                        top_k=top_k, top_p=top_p)
