"""SOM topology evaluation without a GPU: the host restatement of the top-2 search (tests/som_topology_cases.py)
against the committed C oracle, the mutants its input families must reject, and the pure host arithmetic of
qarig/topology.py on hand-made histograms."""
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

import som_topology_cases as T

F32 = np.float32
# K > 25: the oracle (like the reference's cdist) takes the direct form for at most 25 rows and codes, the
# definition under test is the matmul form.
HOST_SHAPES = [(33, 4, 1, 1, 1, 7, 9), (64, 3, 2, 2, 1, 16, 16), (48, 2, 2, 3, 2, 5, 12)]


def test_fma32_is_the_correctly_rounded_fma():
    rng = np.random.default_rng(0)
    a = rng.standard_normal(4000).astype(F32)
    b = rng.standard_normal(4000).astype(F32)
    c = (rng.standard_normal(4000) * 10.0 ** rng.integers(-9, 3, 4000)).astype(F32)
    # ties of the float64 sum: c half way between two floats, the product a tiny push to one side
    c[:1000] = (np.float64(1.0) + np.float64(2.0 ** -23) * rng.integers(0, 1000, 1000)).astype(F32)
    a[:1000] = (F32(2.0 ** -24) * (1 + rng.integers(0, 2, 1000))).astype(F32)       # 2^-24: exact half ulp of c
    b[:1000] = F32(1.0)
    a[500:1000] = (a[500:1000].astype(np.float64) * (1 + 2.0 ** -23)).astype(F32)   # ... plus a push past 53 bits
    got = T.fma32(a, b, c)
    for i in range(len(a)):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo = np.float32(float(exact))                 # float(Fraction) rounds once to float64; decide by hand
        cands = sorted({float(np.nextafter(lo, F32(-np.inf))), float(lo), float(np.nextafter(lo, F32(np.inf)))})
        best = min(cands, key=lambda v: (abs(Fraction(v) - exact), int(np.float32(v).view(np.uint32)) & 1))
        assert float(got[i]) == best, (i, a[i], b[i], c[i])


@pytest.mark.parametrize("shape", HOST_SHAPES, ids=T.shape_id)
@pytest.mark.parametrize("family", T.FAMILIES)
def test_emulation_equals_the_oracle(family, shape):
    """idx1 is the oracle's index; idx2 is the oracle's index once the best code is moved out of reach (1e18 in
    every element: a finite distance beyond every other), on the rows that share that best code."""
    from oracle import bmu as obmu
    c = T.make_case(family, shape)
    i1, i2, d1, d2 = T.emulate_top2(c["x"], c["w"], c["patch"])
    assert np.array_equal(obmu.bmu(c["x"], c["w"], c["patch"]), i1)
    rows = T.patch_rows(c["x"], c["patch"])
    D = rows.shape[1]
    for b in np.unique(i1):
        sel = np.flatnonzero(i1 == b)
        w = c["w"].copy()
        w[b] = 1e18
        second = obmu.bmu(rows[sel].reshape(len(sel), D, 1, 1), w, (1, 1))
        assert np.array_equal(second, i2[sel]), (family, b)
    assert (i1 != i2).all() and (d1 <= d2).all() and (i2[d1 == d2] > i1[d1 == d2]).all()
    if family == "rows_equal_code":
        assert (d1 == 0).all()


def test_families_reject_the_mutants(capsys):
    """Every mutant is told from the definition by at least one family; the table is printed."""
    d1t, d2t = T.ratio_traps()
    table = {}
    for family in T.FAMILIES:
        for shape in HOST_SHAPES[:2] + [(1025, 4, 2, 2, 1, 2, 254)]:
            c = T.make_case(family, shape)
            K = c["w"].shape[0]
            want = T.emulate_top2(c["x"], c["w"], c["patch"])
            hists = T.emulate_rows(*want, K)
            for m in T.MUTANTS:
                if m in ("gap_without_abs", "ratio_bin_fp32"):
                    got = T.emulate_rows(*want, K, mutant=m)
                    differs = any(not np.array_equal(a, b) for a, b in zip(got, hists))
                else:
                    got = T.emulate_top2(c["x"], c["w"], c["patch"], mutant=m)
                    differs = any(not np.array_equal(a, b, equal_nan=True) for a, b in zip(got, want))
                table.setdefault(m, set())
                if differs:
                    table[m].add(family)
    # the hand-made (d1, d2) pairs of the reduction tests
    i = np.arange(len(d1t), dtype=np.int64)
    if any(not np.array_equal(a, b) for a, b in zip(T.emulate_rows(i, i + 1, d1t, d2t, 64),
                                                    T.emulate_rows(i, i + 1, d1t, d2t, 64, mutant="ratio_bin_fp32"))):
        table["ratio_bin_fp32"].add("ratio_traps")
    with capsys.disabled():
        print("\nmutant                    rejected by")
        for m in T.MUTANTS:
            print(f"{m:25s} {', '.join(sorted(table[m])) or '-'}")
    for m in T.MUTANTS:
        assert table[m], f"no family rejects the mutant {m}"
    assert "near_ties" in table["second_by_t"] and "integer" in table["ties_to_higher"]
    assert "offset" in table["no_clamp"] and "ratio_traps" in table["ratio_bin_fp32"]


def test_edges_family_reaches_every_edge():
    for shape in [(1025, 4, 2, 2, 1, 2, 254), (1025, 4, 3, 3, 2, 3, 96), (2049, 2, 2, 3, 2, 5, 96), (3, 3, 2, 2, 1, 16, 16)]:
        c = T.make_case("edges", shape)
        i1, i2, _, _ = T.emulate_top2(c["x"], c["w"], c["patch"])
        K, D = c["w"].shape
        for p in T.edge_positions(K, D):
            assert p in i1 and p in i2, (shape, p)


def test_topology_block_on_hand_made_histograms():
    from qarig.topology import topology_block
    # K = 8, 10 rows in 2 images: gaps 1 x6, 2 x2, 5 x1, 7 x1
    gap = [0, 6, 2, 0, 0, 1, 0, 1]
    ratio = [0] * 32
    ratio[3], ratio[31] = 4, 6
    sums = [[1.5, 4.0, 0.75], [2.5, 6.0, 1.25]]
    b = topology_block(gap, ratio, sums, 10)
    assert b["rows"] == 10 and b["topographic_error"] == 1.0 - 6 / 10
    assert b["within"] == {1: 0.6, 2: 0.8, 4: 0.8} and list(b["within"]) == [1, 2, 4]
    # uniform second unit, K = 8, r = 2: t = 0..7 -> 2,3,4,4,4,4,3,2 of 7 -> 26 / 56
    assert b["within_uniform"][2] == 26 / 56 and b["within_uniform"][1] == 14 / 56 and b["within_uniform"][4] == 44 / 56
    assert b["mean_gap"] == (6 + 4 + 5 + 7) / 10 and b["median_gap"] == 1
    assert b["quantisation_error"] == 0.4 and b["second_error"] == 1.0 and b["quantisation_mse"] == 0.2
    assert b["ratio_hist"] == ratio and b["per_image_quantisation_error"] == [0.3, 0.5]
    # all gaps 1
    b = topology_block([0, 5, 0, 0], [0] * 31 + [5], [[0.0, 5.0, 0.0]], 5)
    assert b["topographic_error"] == 0.0 and b["within"] == {1: 1.0, 2: 1.0} and b["mean_gap"] == 1.0
    # K = 2: one radius, the uniform share is 1; d2 == 0 rows sit in bin 31
    b = topology_block([0, 3], [0] * 31 + [3], [[0.0, 0.0, 0.0]], 3)
    assert b["within"] == {1: 1.0} and b["within_uniform"] == {1: 1.0} and b["median_gap"] == 1
    assert b["quantisation_error"] == 0.0 and b["second_error"] == 0.0 and b["ratio_hist"][31] == 3
    # median: half of the rows at gap <= g
    assert topology_block([0, 2, 0, 2], [4] + [0] * 31, [[1.0, 1.0, 1.0]], 4)["median_gap"] == 1
    assert topology_block([0, 1, 0, 3], [4] + [0] * 31, [[1.0, 1.0, 1.0]], 4)["median_gap"] == 3
    for bad in (([1, 3], [0] * 31 + [4]), ([0, 3], [0] * 31 + [4]), ([0, 4], [4] * 2)):
        with pytest.raises(ValueError):
            topology_block(*bad, [[0.0, 0.0, 0.0]], 4)


def test_lag_block_on_hand_made_sums():
    from qarig.topology import lag_block
    # a line, K = 6, |v| = 3: lag_sum[r] = 3 r (K - r)
    K = 6
    lag = [0.0] + [3.0 * r * (K - r) for r in range(1, K)]
    b = lag_block(lag, K)
    assert b["mean_distance"] == {r: 3.0 * r for r in range(1, K)}
    assert b["all_pairs_mean"] == 3.0 * (K + 1) / 3 and b["lag_half"] == T.line_lag_half(K) == 2
    # K = 2
    b = lag_block([0.0, 4.0], 2)
    assert b == {"mean_distance": {1: 4.0}, "all_pairs_mean": 4.0, "lag_half": 1}
    # all codes equal: no lag reaches half of nothing
    assert lag_block([0.0] * 5, 5)["lag_half"] is None
    # only lags up to 64 are listed, every lag counts
    K = 100
    b = lag_block([0.0] + [float(K - r) for r in range(1, K)], K)
    assert list(b["mean_distance"]) == list(range(1, 65)) and b["all_pairs_mean"] == 1.0 and b["lag_half"] == 1
    with pytest.raises(ValueError):
        lag_block([0.0, 1.0], 3)


def test_line_lag_half_by_hand():
    for K in (2, 3, 5, 6, 11, 64, 513):
        mean = [r for r in range(K)]
        allp = sum(r * (K - r) for r in range(1, K)) / (K * (K - 1) // 2)
        assert T.line_lag_half(K) == next(r for r in range(1, K) if mean[r] >= allp / 2)


def test_summary_line():
    from qarig.topology import topology_summary_line
    block = {"topographic_error": 0.25, "within": {1: 0.75, 2: 0.875, 4: 1.0}, "lag": {"lag_half": None}}
    assert topology_summary_line("hr", block) == "Topology hr TE: 0.2500 | within 2/4/8: 0.8750 / 1.0000 / - | lag_half: None"


def test_recon_scorer_without_topology_keeps_its_keys(monkeypatch):
    """ReconScorer(topology=False) -- the default -- returns the key set it always had and never touches the
    topology module (the device ops are replaced by torch stand-ins: this is about the host plumbing)."""
    import sys
    from qarig import ops, recon_eval

    def pair_error(a, b):
        d = (a.double() - b.double()).flatten(1)
        return torch.stack([(d * d).sum(1), d.abs().sum(1), d.abs().amax(1)], 1)

    monkeypatch.setattr(ops, "pair_error", pair_error)
    monkeypatch.setattr(ops, "ssim", lambda a, b, data_range: torch.ones(len(a), dtype=torch.float64))
    monkeypatch.setattr(ops, "index_histogram", lambda ids, counts: counts.add_(torch.bincount(ids.flatten(), minlength=len(counts))))
    monkeypatch.setattr(ops, "check_index_flag", lambda device, what: None)
    monkeypatch.setattr(ops, "bmu_top2", lambda *a: pytest.fail("top-2 search launched without the flag"))

    class Cb(torch.nn.Module):
        num_embeddings = 4

        def get_patches_bmu(self, x, reshape=False):
            return torch.arange(x.shape[0] * 4).reshape(x.shape[0], 4) % 4

        def get_quantized_image(self, ids):
            return torch.zeros(ids.shape[0], 2, 2, 2)

    sys.modules.pop("qarig.topology", None)
    s = recon_eval.ReconScorer(torch.nn.Identity(), {"cb": Cb()})
    s.add_batch(torch.ones(3, 2, 2, 2))
    r = s.result()
    assert "qarig.topology" not in sys.modules
    assert set(r) == {"images", "codebooks"} and set(r["codebooks"]["cb"]) == {"latent", "vs_decoder", "usage"}
    assert set(r["codebooks"]["cb"]["usage"]) == {"codes", "used", "dead", "perplexity", "entropy_bits", "max_share",
                                                  "counts"}
    assert set(recon_eval.without_per_image(r["codebooks"]["cb"])) == {"latent", "vs_decoder", "usage"}


def test_new_entries_refuse_bad_arguments_without_a_device():
    from qarig import _lib
    h = _lib.load()
    X = 4096   # a non-null pointer that is never dereferenced: every call below fails its argument checks
    top2 = lambda K, D=16: h.qarig_bmu_top2(X, 1, 4, 8, 8, 2, 2, X, K, D, X, X, X, X, None)   # noqa: E731
    assert top2(1) == -1 and "2 <= K" in _lib.last_error()
    assert top2(16385) == -1 and "2 <= K" in _lib.last_error()
    assert top2(64, 12) == -1 and "codebook width" in _lib.last_error()
    assert h.qarig_bmu_top2(X, 1, 4, 8, 8, 2, 2, X, 64, 16, X, None, X, X, None) == -1
    assert h.qarig_topology_rows(X, X, X, X, 0, 4, 8, X, X, X, X, None) == -1
    assert h.qarig_topology_rows(X, X, X, X, 1 << 20, 1 << 20, 8, X, X, X, X, None) == -1
    assert h.qarig_topology_rows(X, X, X, X, 2, 4, 1, X, X, X, X, None) == -1
    assert h.qarig_topology_rows(X, X, None, X, 2, 4, 8, X, X, X, X, None) == -1
    assert h.qarig_code_lag_profile(X, 1, 4, X, None) == -1 and h.qarig_code_lag_profile(None, 4, 4, X, None) == -1


def test_command_lines_take_the_new_flags(monkeypatch):
    import sys
    import evaluate_reconstruction as ER
    base = ["--dataset-path", "d.json", "--decoder-path", "m.pt"]
    assert ER.parse_args(base)["topology"] is False and ER.parse_args(base + ["--topology"])["topology"] is True
    import train_codebook as TC
    common = ["train_codebook.py", "--dataset-path", "d.json", "--decoder-path", "m.pt", "--config-path", "c.json",
              "--out-dir", "o"]
    monkeypatch.setattr(sys, "argv", common)
    assert TC.parse_args()["val_topology"] is False
    monkeypatch.setattr(sys, "argv", common + ["--val-dataset-path", "v.json", "--val-topology"])
    assert TC.parse_args()["val_topology"] is True
    monkeypatch.setattr(sys, "argv", common + ["--val-topology"])
    with pytest.raises(SystemExit):
        TC.parse_args()
