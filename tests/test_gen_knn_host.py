"""CPU half of the k-nearest-neighbour tests: the check families of tests/gen_knn_cases.py accept a NumPy emulation of
the definitions of qarig_knn_smallest / qarig_ball_count and reject eleven mutants of it (so that the GPU tests, which
run the same families on the kernels, can tell a wrong kernel); the reference alone leaves no index ambiguous and no
ball membership undecided on any of the real-valued cases; the brute-force metrics on closed forms; the C-ABI entries
refusing bad arguments without a device; the command line's arguments."""
import numpy as np
import pytest

import gen_knn_cases as K

E = K.EmulatedBackend


@pytest.mark.parametrize("dim", K.DIMS)
def test_the_reference_excuses_nothing_and_the_emulation_passes(dim):
    """Every (nq, nx, offset, self) of the value family at this D: zero ambiguous entries, zero undecided pairs."""
    amb = und = n = 0
    rel = 0.0
    for nq in K.NQS:
        for nx in K.NXS:
            for off in K.OFFSETS:
                for own in (False, True):
                    if own and nq > nx:
                        continue
                    c = K.case(nq, nx, dim, off, own)
                    a, u = K.ambiguities(c)
                    amb, und, n = amb + a, und + u, n + 1
                    rel = max(rel, float((c["bound"][c["cand"]] / c["ref"].astype(np.float64)[c["cand"]]).max()))
    print(f"D = {dim}: {n} cases, {amb} ambiguous entries, {und} undecided pairs, worst bound {rel:.2e} of the "
          f"distance")
    assert amb == 0 and und == 0
    worst = K.family_values(E(), dim)
    print(f"emulation, D = {dim}: worst fraction of the bound {worst:.3f}")
    assert worst < 1


def test_families_accept_the_emulation_rest():
    e = E()
    for k in K.KS:
        for nq, nx, D in ((17, 65, 33), (65, 257, 17), (2, 9, 5)):
            for own in (False, True):
                if nx >= k + 2:
                    assert K.ambiguities(K.case(nq, nx, D, 1000.0, own, k)) == (0, 0)
    b = K.BIG
    for off, own in ((0.0, False), (1000.0, True)):
        assert K.ambiguities(K.case(b["nq"], b["nx"], b["D"], off, own, b["k"])) == (0, 0)
    w = [K.family_other_k(e), K.family_big(e), K.family_exact(e), K.family_properties(e), K.family_nan(e),
         K.family_shift_matters(e)]
    print("emulation: worst fractions (other k, big, exact, properties, NaN, shift): " +
          ", ".join(f"{v:.3f}" for v in w))
    assert max(w) < 1


# which family has to catch which mutant, at the smallest shapes that can (the GPU tests run these families whole)
CATCHES = {
    "self_not_excluded": lambda b: K.family_values(b, 5, nqs=(2,), nxs=(9,), offsets=(0.0,)),
    "self_by_value": K.family_exact,
    "tie_high_index": K.family_exact,
    "ball_strict": K.family_exact,
    "query_radius": lambda b: K.family_values(b, 5, nqs=(15,), nxs=(17,), offsets=(0.0,)),
    "k_plus_1": lambda b: K.family_values(b, 5, nqs=(2,), nxs=(9,), offsets=(0.0,)),
    "partial_block_dropped": lambda b: K.family_values(b, 5, nqs=(17,), nxs=(65,), offsets=(0.0,)),
    "padded_rows_candidates": lambda b: K.family_values(b, 5, nqs=(17,), nxs=(65,), offsets=(0.0,)),
    "shift_ignored": lambda b: K.family_values(b, 17, nqs=(17,), nxs=(65,), offsets=(1000.0,)),
    "shift_on_padding": lambda b: K.family_values(b, 17, nqs=(17,), nxs=(65,), offsets=(0.0,)),
    "f32_row_map": lambda b: K.family_values(b, 16, nqs=(16,), nxs=(16,), offsets=(0.0,)),
}


@pytest.mark.parametrize("mutant", K.MUTANTS)
def test_families_reject_the_mutant(mutant):
    assert set(CATCHES) == set(K.MUTANTS)
    with pytest.raises(AssertionError) as e:
        CATCHES[mutant](E(mutant))
    print(f"{mutant}: {e.value}")


@pytest.mark.parametrize("mutant", ["self_not_excluded", "k_plus_1", "partial_block_dropped", "padded_rows_candidates",
                                    "shift_on_padding", "f32_row_map", "query_radius"])
def test_exact_family_rejects_it_too(mutant):
    """Bit equality on integers is the second net under every mutant that moves a value, an index or a count."""
    with pytest.raises(AssertionError):
        K.family_exact(E(mutant))


def test_shift_ignored_is_what_the_shift_family_looks_for():
    with pytest.raises(AssertionError) as e:
        K.family_shift_matters(type("NoShift", (), {
            "knn": staticmethod(lambda q, x, k, shift, so: K.emulate_knn(q, x, k, K.shift_of(x), so)),
            "ball": staticmethod(lambda q, x, r2, shift, so: K.emulate_ball(q, x, r2, K.shift_of(x), so))})())
    assert "WITHOUT its shift" in str(e.value)           # a backend that shifts anyway is told apart


# --- the metrics' definitions ----------------------------------------------------------------------------------
def test_brute_force_metrics_on_closed_forms():
    rng = np.random.default_rng(0)
    a = rng.standard_normal((40, 6))
    m = K.ref_metrics(a, a.copy(), 3)
    assert m["precision"] == m["recall"] == m["coverage"] == 1.0 and m["density"] > 1.0
    far = K.ref_metrics(a, a + 100.0, 3)
    assert far == {"precision": 0.0, "recall": 0.0, "density": 0.0, "coverage": 0.0}
    two = np.concatenate((a[:20], a[20:] + np.array([100.0, 0, 0, 0, 0, 0])))
    half = K.ref_metrics(two, two[:20].copy(), 3)                         # generated = one of the two real clusters
    assert half["precision"] == 1.0 and half["recall"] == 0.5 and half["coverage"] == 0.5


# --- the C ABI without a device ----------------------------------------------------------------------------------
def test_entries_refuse_bad_arguments_without_a_device():
    """Every call below is refused before any launch (X is a made-up address that is never dereferenced)."""
    from qarig import _lib
    h = _lib.load()
    X = 0x7f0000000000
    G = 1 << 30

    def ws_bytes(nq=16, nx=64, D=32, k=3):
        return h.qarig_knn_workspace_bytes(nq, nx, D, k)

    assert ws_bytes() >= (16 + 64) * 8 and ws_bytes(nx=1 << 20, k=8) > ws_bytes(nx=1 << 20, k=1)
    for kw in ({"D": 0}, {"D": 1025}, {"nq": 0}, {"nq": (1 << 20) + 1}, {"nx": 0}, {"nx": -5}, {"nx": (1 << 20) + 1},
               {"k": 0}, {"k": 9}, {"nq": 2 ** 31 - 1}):
        assert ws_bytes(**kw) == 0, kw

    def knn(nq=16, nx=64, D=32, k=3, so=-1, q=X, x=X + G, shift=X + 2 * G, d2=X + 3 * G, idx=X + 4 * G, ws=X + 5 * G,
            nws=None):
        nws = (ws_bytes(nq, nx, D, k) or 1 << 20) if nws is None else nws
        return h.qarig_knn_smallest(q, nq, x, nx, D, shift, k, so, d2, idx, ws, nws, None)

    def ball(nq=16, nx=64, D=32, so=-1, q=X, x=X + G, shift=X + 2 * G, r2=X + 3 * G, count=X + 4 * G, ws=X + 5 * G,
             nws=None):
        nws = (ws_bytes(nq, nx, D, 1) or 1 << 20) if nws is None else nws
        return h.qarig_ball_count(q, nq, x, nx, D, shift, r2, so, count, ws, nws, None)

    for kw in ({"q": None}, {"x": None}, {"d2": None}, {"idx": None}, {"ws": None}):
        assert knn(**kw) == -1 and "null" in _lib.last_error(), kw
    for kw in ({"q": None}, {"x": None}, {"r2": None}, {"count": None}, {"ws": None}):
        assert ball(**kw) == -1 and "null" in _lib.last_error(), kw
    for fn in (knn, ball):
        for D in (0, -1, 1025, 2 ** 30):
            assert fn(D=D) == -1 and "D =" in _lib.last_error(), D
        for n in (0, -1, 2 ** 20 + 1, 2 ** 31 - 1):
            assert fn(nq=n) == -1 and "nq =" in _lib.last_error(), n
            assert fn(nx=n) == -1 and "nx =" in _lib.last_error(), n
        for so in (-2, 49, 2 ** 31 - 1, -2 ** 31):                      # nx - nq = 48
            assert fn(so=so) == -1 and "self_offset" in _lib.last_error(), so
        assert fn(nq=65, nx=64, so=0) == -1 and "self_offset" in _lib.last_error()
        assert fn(nws=8) == -3 and "workspace" in _lib.last_error()
        assert fn(nws=ws_bytes(16, 64, 32, 1) - 1) == -3
        nbytes = 64 * 32 * 8
        for kw in ({"ws": X + G + nbytes - 8}, {"ws": X - 8}, {"ws": X + 2 * G + 8}):
            assert fn(**kw) == -1 and "workspace overlaps" in _lib.last_error(), kw
    for k in (0, -1, 9, 2 ** 31 - 1):
        assert knn(k=k) == -1 and "k =" in _lib.last_error(), k
    assert knn(nq=1, nx=3, k=3, so=0) == -1 and "candidates" in _lib.last_error()       # 2 candidates for k = 3
    assert knn(nq=1, nx=2, k=3) == -1 and "candidates" in _lib.last_error()
    assert ball(nq=1, nx=1, so=0) == -1 and "candidates" in _lib.last_error()
    for kw in ({"d2": X + 8}, {"idx": X + G + 64 * 32 * 8 - 4}, {"d2": X + 2 * G}, {"idx": X - 4}):
        assert knn(**kw) == -1 and "output overlaps" in _lib.last_error(), kw
    for kw in ({"count": X}, {"count": X + 3 * G + 8}, {"count": X + 2 * G + 32 * 8 - 4}):
        assert ball(**kw) == -1 and "output overlaps" in _lib.last_error(), kw
    # the queries MAY be rows of x (self), and the shift may be absent
    assert knn(q=X + G + 32 * 8, so=1, ws=None) == -1 and "null" in _lib.last_error()


def test_ops_and_metrics_refuse_cpu_tensors_and_bad_shapes():
    import torch
    from qarig import gen_eval, ops
    f = torch.zeros((5, 4), dtype=torch.float64)
    with pytest.raises(RuntimeError):
        ops.knn_smallest(f, f, 1)
    with pytest.raises(RuntimeError):
        ops.ball_count(f, f, torch.zeros(5, dtype=torch.float64))
    with pytest.raises(RuntimeError):
        gen_eval.FeatureBank(4, 8).add(f)
    with pytest.raises(ValueError):
        gen_eval.FeatureBank(4, 0)
    with pytest.raises(ValueError):
        gen_eval.FeatureBank(1025, 8)
    with pytest.raises(ValueError):
        gen_eval.FeatureBank(4, 8).rows()
    with pytest.raises(ValueError):
        gen_eval.manifold_metrics(f, f, 5)                               # needs k + 1 = 6 rows
    with pytest.raises(ValueError):
        gen_eval.manifold_metrics(f, f, 9)
    for kw in ({"knn": 9}, {"knn": -1}, {"knn": 3, "knn_max_samples": 0}):
        with pytest.raises(ValueError):
            gen_eval.GenerationScorer(1, **kw)
    s = gen_eval.GenerationScorer(1)
    assert s.knn == 0 and s._banks == {}
    assert "depend on k" in gen_eval.MANIFOLD_NOTE and "sample counts" in gen_eval.MANIFOLD_NOTE


def test_summary_line_appends_the_four_numbers_only_when_present():
    from qarig import gen_eval
    r = {"dim": 4, "counts": {"real": 8}, "fd_real_generated": {"fd": 1.5}}
    plain = gen_eval.summary_line("t", r)
    assert "precision" not in plain
    four = {"precision": 0.5, "recall": 0.25, "density": 0.75, "coverage": 1.0}
    line = gen_eval.summary_line("t", dict(r, manifold={"k": 3, "real_generated": four, "real_split": four}))
    assert line.startswith(plain) and "precision=0.5000" in line and "coverage=1.0000" in line and "k=3" in line


def test_evaluate_generation_knows_the_knn_options():
    import evaluate_generation as EG
    base = ["--real-dataset-path", "d.json", "--generated-latents", "g.npy"]
    a = EG.parse_args(base)
    assert a["knn"] == 0 and a["save_neighbours"] is None and a["knn_max_samples"] >= 1024
    a = EG.parse_args(base + ["--knn", "3", "--knn-max-samples", "500", "--save-neighbours", "o/nn.npz"])
    assert (a["knn"], a["knn_max_samples"], str(a["save_neighbours"])) == (3, 500, "o/nn.npz")
    for bad in (["--knn", "9"], ["--knn", "-1"], ["--knn", "3", "--knn-max-samples", "0"],
                ["--save-neighbours", "o/nn.npz"]):
        with pytest.raises(SystemExit):
            EG.parse_args(base + bad)
    EG.check_knn_counts(3, 8, 4)
    for n_real, n_gen, name in ((7, 4, "real_b (3)"), (8, 3, "generated (3)"), (1, 9, "real (1)")):
        with pytest.raises(SystemExit) as e:
            EG.check_knn_counts(3, n_real, n_gen)
        assert "--knn 3 needs at least 4 samples" in str(e.value) and name in str(e.value)
