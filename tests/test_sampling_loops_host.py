"""The full-window chunk search of qarig.sampling.generate_tokens on the CPU (no GPU): the loop every GPU test of
the cached and fused paths uses as its reference, pinned here against recorded runs.

A stub model (no `decoder_layers`, so nothing is cacheable) returns logits that are a smooth function of the token
prefix and the positions; torch.multinomial is replaced by a chooser that depends only on the call number, the row
and the support of the probability row, so the result does not hang on a platform's generator or on last-bit
rounding.  Per case the test compares the returned tokens, every `decode` call (window shape, first and last
position, their dtype and `pos_bound`) and every draw (row count) with literals.

EXPECTED was recorded by running this file (`python tests/test_sampling_loops_host.py`) on the commit before the
loops were merged into one; it passes there unchanged.  No near ties: in every recorded run the probability
products of two competing candidate chunks differ by more than 1e-3 relative (`_min_gap`, asserted in the test
too), so the kept chunk does not depend on rounding either."""
import itertools

import pytest
import torch

from conftest import PKG  # noqa: F401  (puts the package on sys.path)

V, END, WINDOW, TOTAL, T = 11, 10, 6, 12, 0.8


class Stub:
    """What generate_tokens needs of a model that is not cacheable: use_encoder, use_pos_cond, encode, decode."""
    use_encoder = True
    use_pos_cond = True

    def __init__(self):
        self.calls = []

    def encode(self, lr):
        return lr.double()[:, :, None] * 0.01

    def decode(self, tokens, enc, pos, pos_bound=None):
        R, S = tokens.shape
        rec = f"{R}x{S}"
        feat = torch.cumsum(0.37 * tokens.double() + 1.0, dim=1) * 0.113
        if pos is not None:
            assert pos.shape == tokens.shape and bool((pos == pos[:1]).all())
            rec += f":{float(pos[0, 0]):g}-{float(pos[0, -1]):g}" + ("" if pos.dtype.is_floating_point else "i")
            feat = feat + 0.05 * pos.double()
        if pos_bound is not None:
            rec += f"<{pos_bound}"
        self.calls.append(rec)
        feat = feat + enc.sum(dim=(1, 2))[:, None]            # one encoder row per evaluated row
        v = torch.arange(V, dtype=torch.float64)
        return (2.0 * torch.sin(feat[..., None] * (0.9 + 0.21 * v) + v)).float()


class CondStub(Stub):
    """A model with `_cond` (a Transformer): whole-number positions as int64, and `pos_bound`."""

    def _cond(self):
        raise AssertionError("only its presence is read")


class Chooser:
    """torch.multinomial(probs, 1) replaced: row r of call c takes entry (7 c + c^2 // 2 + 3 r + 1) mod |support| of
    its support in index order.  Keeps (probs, choice) of every call."""

    def __init__(self):
        self.draws = []

    def __call__(self, probs, num_samples):
        assert num_samples == 1 and probs.dim() == 2
        c, out = len(self.draws), []
        for r, row in enumerate(probs):
            support = torch.nonzero(row > 0).flatten()
            out.append(int(support[(7 * c + c * c // 2 + 3 * r + 1) % len(support)]))
        out = torch.tensor(out, dtype=torch.int64)[:, None]
        self.draws.append((probs.double().clone(), out.flatten()))
        return out


def _cases():
    out = {}
    for (nb, bw), batch, slide, mode in itertools.product([(1, 1), (3, 2)], [False, True], [True, False],
                                                          ["generate", "train"]):
        name = f"{mode[:3]}-{nb}x{bw}-{'batch' if batch else 'seq'}-{'slide' if slide else 'whole'}"
        out[name] = dict(num_beam=nb, beam_width=bw, batch_beams=batch, slide=slide, mode=mode)
    base = dict(num_beam=3, beam_width=2, batch_beams=False, slide=True, mode="generate")
    out["prefix3-seq"] = dict(base, prefix=3)
    out["prefix3-batch"] = dict(base, prefix=3, batch_beams=True)
    out["prefix3-train"] = dict(base, prefix=3, mode="train")
    out["filtered"] = dict(base, top_k=3, top_p=0.9, shift=1)
    out["cond-seq"] = dict(base, model=CondStub)
    out["cond-batch"] = dict(base, model=CondStub, batch_beams=True)
    out["cond-whole"] = dict(base, model=CondStub, slide=False)
    return out


CASES = _cases()


def _run(case, patch):
    from qarig import sampling
    c = dict(CASES[case])
    model, chooser = c.pop("model", Stub)(), Chooser()
    g = torch.Generator().manual_seed(3)
    hr = torch.randint(0, V - 1, (2, c.pop("prefix", 1)), generator=g)
    lr = torch.randint(0, V - 1, (2, 4), generator=g)
    slide = c.pop("slide")
    patch(torch, "multinomial", chooser)
    out = sampling.generate_tokens(model, hr, lr, TOTAL, T, slide, WINDOW, END, use_kv_cache=True, **c)
    assert torch.equal(out[:, :hr.shape[1]], hr)
    rows = {d[1].numel() for d in chooser.draws}
    assert len(rows) == 1
    bw = c["beam_width"]         # the calls of one candidate chunk as one string
    calls = [" ".join(model.calls[i:i + bw]) for i in range(0, len(model.calls), bw)]
    got = dict(tokens=out.tolist(), calls=calls, draws=[len(chooser.draws), rows.pop()])
    return got, _min_gap(chooser.draws, c["num_beam"], c["beam_width"], c["batch_beams"])


def _min_gap(draws, num_beam, beam_width, batch_beams):
    """Smallest relative difference between the probability products of two candidate chunks that compete for one
    image's chunk position (fp64, from the rows the draws were made from)."""
    if num_beam == 1:
        return 1.0
    picked = [p[torch.arange(len(t)), t] for p, t in draws]
    per_chunk = beam_width * (1 if batch_beams else num_beam)
    gap = 1.0
    for c0 in range(0, len(picked), per_chunk):
        chunk = picked[c0:c0 + per_chunk]
        if batch_beams:     # rows image-major, the candidates of an image adjacent
            prods = torch.stack(chunk).prod(dim=0).view(-1, num_beam)
        else:               # candidate after candidate, beam_width draws each
            prods = torch.stack([torch.stack(chunk[b * beam_width:(b + 1) * beam_width]).prod(dim=0)
                                 for b in range(num_beam)], dim=1)
        for a, b in itertools.combinations(range(num_beam), 2):
            rel = (prods[:, a] - prods[:, b]).abs() / torch.maximum(prods[:, a], prods[:, b])
            gap = min(gap, float(rel.min()))
    return gap


EXPECTED = {
    "gen-1x1-seq-slide": dict(tokens=[[6, 1, 8, 7, 6, 7, 8, 1, 4, 9, 4, 1], [8, 4, 1, 0, 9, 0, 1, 4, 7, 2, 7, 4]],
        calls=["2x1:0-0", "2x2:0-2", "2x3:0-3", "2x4:0-4", "2x5:0-5", "2x5:2-6", "2x5:3-7", "2x5:4-8", "2x5:5-9",
               "2x5:6-10", "2x5:7-11"],
        draws=[11, 2]),
    "tra-1x1-seq-slide": dict(tokens=[[6, 1, 8, 6, 4, 4, 4, 6, 8, 1, 5, 0, 6], [8, 4, 0, 9, 7, 7, 7, 9, 0, 4, 8, 3, 9]],
        calls=["2x1:0-0", "2x2:0-1", "2x3:0-2", "2x4:0-3", "2x5:0-4", "2x5:1-5", "2x5:2-6", "2x5:3-7", "2x5:4-8",
               "2x5:5-9", "2x5:6-10", "2x5:7-11"],
        draws=[12, 2]),
    "gen-1x1-seq-whole": dict(tokens=[[6, 1, 8, 7, 6, 7, 8, 1, 4, 9, 4, 1], [8, 4, 1, 0, 9, 0, 1, 4, 7, 2, 7, 4]],
        calls=["2x1", "2x2", "2x3", "2x4", "2x5", "2x6", "2x7", "2x8", "2x9", "2x10", "2x11"],
        draws=[11, 2]),
    "tra-1x1-seq-whole": dict(tokens=[[6, 1, 8, 6, 4, 4, 4, 6, 8, 1, 5, 0, 6], [8, 4, 0, 9, 7, 7, 7, 9, 0, 4, 8, 3, 9]],
        calls=["2x1", "2x2", "2x3", "2x4", "2x5", "2x6", "2x7", "2x8", "2x9", "2x10", "2x11", "2x12"],
        draws=[12, 2]),
    "gen-3x2-seq-slide": dict(tokens=[[6, 7, 6, 9, 4, 7, 8, 9, 4, 7, 8, 7, 8], [8, 0, 1, 4, 1, 0, 1, 0, 9, 0, 1, 0, 9]],
        calls=3 * ["2x1:0-0 2x2:0-2"] + 3 * ["2x3:0-3 2x4:0-4"] + 3 * ["2x5:0-5 2x5:2-6"] + 3 * ["2x5:3-7 2x5:4-8"]
        + 3 * ["2x5:5-9 2x5:6-10"] + 3 * ["2x5:7-11 2x5:8-12"],
        draws=[36, 2]),
    "tra-3x2-seq-slide": dict(tokens=[[6, 1, 8, 1, 5, 0, 0, 0, 5, 4, 4, 1, 5], [8, 7, 7, 9, 0, 6, 3, 4, 0, 9, 0, 4, 8]],
        calls=3 * ["2x1:0-0 2x2:0-1"] + 3 * ["2x3:0-2 2x4:0-3"] + 3 * ["2x5:0-4 2x5:1-5"] + 3 * ["2x5:2-6 2x5:3-7"]
        + 3 * ["2x5:4-8 2x5:5-9"] + 3 * ["2x5:6-10 2x5:7-11"],
        draws=[36, 2]),
    "gen-3x2-seq-whole": dict(tokens=[[6, 7, 6, 1, 4, 1, 4, 9, 4, 7, 8, 7, 6], [8, 0, 1, 4, 1, 0, 1, 0, 9, 4, 7, 0, 1]],
        calls=3 * ["2x1 2x2"] + 3 * ["2x3 2x4"] + 3 * ["2x5 2x6"] + 3 * ["2x7 2x8"] + 3 * ["2x9 2x10"]
        + 3 * ["2x11 2x12"],
        draws=[36, 2]),
    "tra-3x2-seq-whole": dict(tokens=[[6, 1, 8, 1, 5, 0, 0, 0, 5, 4, 4, 3, 0], [8, 7, 7, 9, 0, 6, 3, 4, 0, 7, 7, 3, 9]],
        calls=3 * ["2x1 2x2"] + 3 * ["2x3 2x4"] + 3 * ["2x5 2x6"] + 3 * ["2x7 2x8"] + 3 * ["2x9 2x10"]
        + 3 * ["2x11 2x12"],
        draws=[36, 2]),
    "gen-3x2-batch-slide": dict(tokens=[[6, 1, 8, 0, 9, 0, 1, 1, 4, 5, 0, 4, 1],
                                        [8, 0, 7, 6, 5, 9, 0, 0, 3, 4, 9, 3, 0]],
        calls=["6x1:0-0 6x2:0-2", "6x3:0-3 6x4:0-4", "6x5:0-5 6x5:2-6", "6x5:3-7 6x5:4-8", "6x5:5-9 6x5:6-10",
               "6x5:7-11 6x5:8-12"],
        draws=[12, 6]),
    "tra-3x2-batch-slide": dict(tokens=[[6, 1, 8, 1, 0, 0, 0, 9, 0, 1, 5, 3, 9],
                                        [8, 5, 1, 7, 5, 8, 8, 4, 6, 5, 9, 9, 4]],
        calls=["6x1:0-0 6x2:0-1", "6x3:0-2 6x4:0-3", "6x5:0-4 6x5:1-5", "6x5:2-6 6x5:3-7", "6x5:4-8 6x5:5-9",
               "6x5:6-10 6x5:7-11"],
        draws=[12, 6]),
    "gen-3x2-batch-whole": dict(tokens=[[6, 1, 8, 0, 9, 0, 1, 1, 4, 5, 0, 7, 4],
                                        [8, 0, 7, 6, 5, 9, 0, 0, 3, 8, 3, 6, 3]],
        calls=["6x1 6x2", "6x3 6x4", "6x5 6x6", "6x7 6x8", "6x9 6x10", "6x11 6x12"],
        draws=[12, 6]),
    "tra-3x2-batch-whole": dict(tokens=[[6, 1, 8, 1, 0, 0, 0, 9, 0, 4, 8, 0, 6],
                                        [8, 5, 1, 7, 5, 5, 5, 4, 6, 0, 3, 4, 0]],
        calls=["6x1 6x2", "6x3 6x4", "6x5 6x6", "6x7 6x8", "6x9 6x10", "6x11 6x12"],
        draws=[12, 6]),
    "prefix3-seq": dict(tokens=[[6, 8, 7, 1, 8, 9, 4, 7, 8, 1, 8, 7, 8], [7, 0, 0, 0, 1, 4, 1, 0, 1, 0, 9, 0, 1]],
        calls=3 * ["2x3:0-3 2x4:0-4"] + 3 * ["2x5:0-5 2x5:2-6"] + 3 * ["2x5:3-7 2x5:4-8"] + 3 * ["2x5:5-9 2x5:6-10"]
        + 3 * ["2x5:7-11 2x5:8-12"],
        draws=[30, 2]),
    "prefix3-batch": dict(tokens=[[6, 8, 7, 4, 1, 0, 9, 0, 1, 1, 4, 9, 4], [7, 0, 0, 0, 7, 6, 5, 9, 0, 0, 3, 4, 9]],
        calls=["6x3:0-3 6x4:0-4", "6x5:0-5 6x5:2-6", "6x5:3-7 6x5:4-8", "6x5:5-9 6x5:6-10", "6x5:7-11 6x5:8-12"],
        draws=[10, 6]),
    "prefix3-train": dict(tokens=[[6, 8, 7, 6, 4, 0, 6, 0, 0, 0, 5, 4, 4, 1, 5],
                                  [7, 0, 0, 4, 0, 9, 0, 6, 3, 4, 0, 9, 0, 4, 8]],
        calls=3 * ["2x3:0-2 2x4:0-3"] + 3 * ["2x5:0-4 2x5:1-5"] + 3 * ["2x5:2-6 2x5:3-7"] + 3 * ["2x5:4-8 2x5:5-9"]
        + 3 * ["2x5:6-10 2x5:7-11"] + 3 * ["2x5:8-12 2x5:9-13"],
        draws=[36, 2]),
    "filtered": dict(tokens=[[6, 8, 7, 6, 1, 5, 1, 5, 10, 5, 9, 9, 8], [8, 7, 7, 6, 1, 5, 1, 5, 10, 5, 9, 9, 8]],
        calls=3 * ["2x1:0-0 2x2:0-2"] + 3 * ["2x3:0-3 2x4:0-4"] + 3 * ["2x5:0-5 2x5:2-6"] + 3 * ["2x5:3-7 2x5:4-8"]
        + 3 * ["2x5:5-9 2x5:6-10"] + 3 * ["2x5:7-11 2x5:8-12"],
        draws=[36, 2]),
    "cond-seq": dict(tokens=[[6, 7, 6, 9, 4, 7, 8, 9, 4, 7, 8, 7, 8], [8, 0, 1, 4, 1, 0, 1, 0, 9, 0, 1, 0, 9]],
        calls=3 * ["2x1:0-0i<16 2x2:0-2i<16"] + 3 * ["2x3:0-3i<16 2x4:0-4i<16"] + 3 * ["2x5:0-5i<16 2x5:2-6i<16"]
        + 3 * ["2x5:3-7i<16 2x5:4-8i<16"] + 3 * ["2x5:5-9i<16 2x5:6-10i<16"] + 3 * ["2x5:7-11i<16 2x5:8-12i<16"],
        draws=[36, 2]),
    "cond-batch": dict(tokens=[[6, 1, 8, 0, 9, 0, 1, 1, 4, 5, 0, 4, 1], [8, 0, 7, 6, 5, 9, 0, 0, 3, 4, 9, 3, 0]],
        calls=["6x1:0-0i<16 6x2:0-2i<16", "6x3:0-3i<16 6x4:0-4i<16", "6x5:0-5i<16 6x5:2-6i<16",
               "6x5:3-7i<16 6x5:4-8i<16", "6x5:5-9i<16 6x5:6-10i<16", "6x5:7-11i<16 6x5:8-12i<16"],
        draws=[12, 6]),
    "cond-whole": dict(tokens=[[6, 7, 6, 1, 4, 1, 4, 9, 4, 7, 8, 7, 6], [8, 0, 1, 4, 1, 0, 1, 0, 9, 4, 7, 0, 1]],
        calls=3 * ["2x1 2x2"] + 3 * ["2x3 2x4"] + 3 * ["2x5 2x6"] + 3 * ["2x7 2x8"] + 3 * ["2x9 2x10"]
        + 3 * ["2x11 2x12"],
        draws=[36, 2]),
}
# one candidate: --batch-beams takes the sequential loop (recorded: the same runs)
EXPECTED.update({name.replace("seq", "batch"): want for name, want in EXPECTED.items() if "-1x1-seq-" in name})


@pytest.mark.parametrize("case", list(CASES))
def test_full_window_search_reproduces_the_recorded_run(case, monkeypatch):
    got, gap = _run(case, monkeypatch.setattr)
    assert gap > 1e-3, f"candidate products within {gap} relative: the recorded choice would hang on rounding"
    want = EXPECTED[case]
    assert got["tokens"] == want["tokens"]
    assert got["calls"] == want["calls"]
    assert got["draws"] == want["draws"]


if __name__ == "__main__":          # the recording: prints EXPECTED's entries and the smallest gap
    real = torch.multinomial
    worst = 1.0
    for name in CASES:
        try:
            got, gap = _run(name, setattr)
        finally:
            torch.multinomial = real
        worst = min(worst, gap)
        runs = [[k, len(list(grp))] for k, grp in itertools.groupby(got["calls"])]
        calls = " + ".join(f'{n} * ["{k}"]' for k, n in runs)
        print(f'    "{name}": dict(tokens={got["tokens"]},\n        calls={calls},\n        draws={got["draws"]}),')
    print("smallest relative gap between competing products:", worst)
