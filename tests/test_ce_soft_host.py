"""tests/ce_soft_cases.py on the CPU: the fp64 reference is fp64 autograd of the mixed-target definition
-sum tau log softmax + zeta lse^2 (tau sums to 1 on every row), the tolerance table is what the emulation gives, the
emulation without a window is ce_reg_cases.reg_emulate bit for bit, every mutant is rejected by the GPU test's own
cells on the GPU test's own inputs, the +inf rows are the stated ones and no row escapes a verdict; the host-side
argument rules of qarig.ops.check_ce_soft and the weight table."""
import functools
import math

import pytest
import torch

import ce_reg_cases as G
import ce_soft_cases as S
import row_kernel_cases as R


@functools.lru_cache(maxsize=None)
def _emulation():
    return S.soft_verdicts(S.soft_emulate)


def _tau(c, gi):
    """The mixed target distribution of the definition, built column by column in plain Python (not by
    ce_soft_cases.window): (1 - eps - nu) onehot + eps / C + nu q on code rows, nu = 0 on special rows."""
    eps, _, nu = (G.f32(v) for v in S.SOFT_GRID[gi])
    tau = torch.full((c.M, c.C), eps / c.C, dtype=torch.float64)
    w = c.w.double()
    for r in range(c.M):
        t = int(c.t[r])
        if t >= c.K:
            tau[r, t] += 1.0 - eps
            continue
        lo, hi = max(0, t - c.R), min(c.K - 1, t + c.R)
        z = sum(float(w[abs(j - t)]) for j in range(lo, hi + 1))
        for j in range(lo, hi + 1):
            tau[r, j] += nu * float(w[abs(j - t)]) / z
        tau[r, t] += 1.0 - eps - nu
    return tau


def test_reference_is_autograd_of_the_mixed_target_definition():
    """Row objectives against -sum_c tau_c log softmax(x)_c + zeta lse^2 in fp64 (+inf rows: the same rows), tau sums
    to 1, the nll is F.cross_entropy, and M dlogits is autograd's gradient within 1e-12 on the finite rows."""
    cases = [c for c in S.soft_cases() if c.C <= 513]
    for c in cases:
        for gi, (eps, zeta, nu) in enumerate(S.SOFT_GRID):
            eps, zeta = G.f32(eps), G.f32(zeta)
            ref = S.soft_ref(c, gi)
            tau = _tau(c, gi)
            assert float((tau.sum(1) - 1.0).abs().max()) < 1e-14 and (tau >= 0).all()
            special = c.t >= c.K
            assert (tau[special].max(1).values >= 1.0 - eps - 1e-15).all()      # a special target keeps its whole mass
            assert (tau[:, c.K:][~special] == eps / c.C).all()                  # and is nobody's neighbour
            x = c.x.double().requires_grad_(True)
            logp = torch.log_softmax(x, 1)
            # a zero coefficient is not evaluated: 0 * -inf never forms
            rows = -torch.where(tau > 0, tau * logp, torch.zeros_like(logp)).sum(1) + zeta * torch.logsumexp(x, 1) ** 2
            inf = torch.isinf(rows.detach())
            assert torch.equal(inf, torch.isinf(ref["obj"])) and (ref["obj"][inf] > 0).all(), (c.C, c.K, c.R, gi)
            fin = ~inf
            torch.testing.assert_close(ref["obj"][fin], rows.detach()[fin], rtol=1e-12, atol=1e-12)
            plain = torch.nn.functional.cross_entropy(c.x.double(), c.t, reduction="none")
            torch.testing.assert_close(ref["nll"], plain, rtol=1e-12, atol=1e-12)
            assert torch.isfinite(ref["nll"]).all() and torch.isfinite(ref["dlogits"]).all()
            rows[fin].sum().backward()
            g = ref["dlogits"][fin] * c.M
            assert float((g - x.grad[fin]).abs().max()) <= 1e-12 * float(g.abs().max()), (c.C, c.K, c.R, gi)
            # a -inf logit inside a window: the gradient element is the finite -(eps / C + nu q) / M
            hit = torch.isinf(c.x) & (ref["q"] > 0)
            if hit.any():
                want = -(eps / c.C + ref["nur"][:, None] * ref["q"]) / c.M
                assert torch.equal(ref["dlogits"][hit], want[hit])


def test_tolerance_table_is_twice_the_emulation():
    worst, _, _ = _emulation()
    rows = {k: S.tolerance_of(w) for k, w in worst.items() if len(k) == 3 and k[0] != "dsum"}
    means = {k: S.tolerance_of(w) for k, w in worst.items() if len(k) == 2}
    assert rows == S.SOFT_TOL_U and means == S.SOFT_MEAN_TOL_U
    assert len(rows) == len(S.SOFT_ROW_OUTPUTS) * len(R.CE_FAMILIES) * len(S.SOFT_GRID)
    assert not S.soft_failures(worst)            # the gradient sums sit inside dlogits' tolerance
    assert max(S.SOFT_TOL_U.values()) <= max(G.REG_TOL_U.values())     # of the size the regularised kernel's are


def test_emulation_without_a_window_is_the_regularised_emulation_bit_for_bit():
    """K = 0 in the emulation makes every target special: nu = 0 by selects, reg_emulate's bits."""
    for c in S.soft_cases((41, 257)):
        for eps, zeta, nu in S.SOFT_GRID:
            got = S.soft_emulate(c.x, c.t, 0, c.R, c.w, eps, zeta, nu)
            want = G.reg_emulate(c.x, c.t, eps, zeta)
            for a, b in zip(got, want):
                assert torch.equal(a, b) or (torch.isnan(a) == torch.isnan(b)).all() and torch.equal(
                    torch.nan_to_num(a, nan=0.0), torch.nan_to_num(b, nan=0.0)), (c.C, eps, zeta)
            assert not any(torch.isnan(a).any() for a in got)


def test_cases_hold_the_targets_and_windows_they_claim():
    """Every forced target is in its case, special where it says; windows straddle the lane wrap and the four-trip
    boundary; R = 31 covers the whole axis at C = 3 and 41; the table is the package's."""
    from qarig import ops
    for c in S.soft_cases():
        assert [int(c.t[r]) for r in c.forced_rows] == c.forced and len(set(c.forced_rows)) == len(c.forced)
        assert all(c.family[r] in S.SOFT_FORCED_ROWS for r in c.forced_rows)
        assert torch.equal(c.w, ops.neighbour_table(c.R, c.R / 2.0)) and float(c.w[0]) == 1.0 and (c.w > 0).all()
        inside, _ = S.window(c.t, c.C, c.K, c.R, c.w)
        assert int(inside.sum(1).max()) <= 2 * c.R + 1 <= 63 and not inside[:, c.K:].any()
        assert (inside.sum(1) == 0).equal(c.t >= c.K)
        if c.K < c.C:
            assert c.K in c.forced
        if c.K > 64 + 1:
            r = c.forced_rows[c.forced.index(64)]
            assert inside[r, 63] and inside[r, 64]
        if c.K > 256 + 1:
            r = c.forced_rows[c.forced.index(256)]
            assert inside[r, 255] and inside[r, 256]
        if c.R == 31 and c.C in (3, 41):
            whole = inside[c.t < c.K].sum(1).eq(c.K)          # every target at C = 3, the middle ones at C = 41
            assert whole.all() if c.C == 3 else whole.any()
    assert len(S.soft_cases()) == 2 * len(S.SOFT_RANGES) * len(S.SOFT_CLASSES) + len(S.SOFT_MEAN_M)


# which cells must see each mutant: (outputs, grid points) of which at least one combination fails
EXPECT = {
    "no_clamp_end": ("obj", "dlogits"),
    "no_renorm": ("obj", "dlogits", "dsum"),
    "special_smoothed": ("obj", "dlogits"),
    "no_nu_hot": ("obj", "dlogits", "dsum"),
    "no_nuq_grad": ("dlogits", "dsum"),
    "short_window": ("obj", "dlogits"),
    "table_by_lo": ("obj", "dlogits"),
    "nu_multiplied": ("obj",),
}


@pytest.mark.parametrize("mutant", S.SOFT_MUTANTS)
def test_mutant_is_rejected(mutant):
    failed = S.mutant_failures(mutant)
    assert failed, mutant
    cells = [k for k in failed if len(k) == 3]
    print(f"MUTANT {mutant} rejected by {len(failed)} cells: {failed}")
    for out in EXPECT[mutant]:        # at every grid point: nu > 0 everywhere on the grid
        assert {k[2] for k in cells if k[0] == out} == set(range(len(S.SOFT_GRID))), (mutant, out, failed)
    if mutant == "nu_multiplied":     # NaN on the masked rows' objectives (and the means over them), nowhere else
        assert {k[:2] for k in cells} == {("obj", "masked")}
        assert all(k[0] == "mean_obj" for k in failed if len(k) == 2)
    if mutant == "no_nuq_grad":       # the objective is untouched
        assert not [k for k in failed if k[0] in ("obj", "nll", "mean_obj", "mean_nll")]
    assert not [k for k in failed if k[0] in ("nll", "mean_nll")]     # the plain nll never sees the feature


def test_inf_rows_are_the_stated_ones_and_every_row_enters_a_verdict():
    """Each (case, grid point, row) is judged on its four row outputs; the only entries without an error figure are
    the +inf row objectives: every masked row at eps > 0, and at eps = 0 the masked rows with a -inf logit inside
    their window -- counted by the definition of the window, not by any arithmetic."""
    worst, judged, excused = _emulation()
    rows = sum(c.M for c in S.soft_cases())
    assert judged == 4 * rows * len(S.SOFT_GRID)
    by_rule = sum(len(S.window_inf_rows(c)) for c in S.soft_cases())
    assert S.SOFT_INF_ROWS_NB == by_rule == 146 and S.SOFT_INF_ROWS_EPS == 270
    n_eps = sum(1 for e, _, _ in S.SOFT_GRID if e > 0)
    assert excused == n_eps * S.SOFT_INF_ROWS_EPS + (len(S.SOFT_GRID) - n_eps) * S.SOFT_INF_ROWS_NB
    assert all(w == w and w != float("inf") for w in worst.values())
    for c in S.soft_cases():
        for gi, (e, _, _) in enumerate(S.SOFT_GRID):
            want = c.rows("masked") if e > 0 else S.window_inf_rows(c)
            assert torch.nonzero(torch.isinf(S.soft_ref(c, gi)["obj"])).flatten().tolist() == want
            assert set(want) <= set(c.rows("masked"))


def test_host_argument_rules_and_weight_table():
    from qarig import ops
    w = ops.neighbour_table(4, 2.0)
    assert w.dtype == torch.float32 and w.shape == (5,) and float(w[0]) == 1.0
    assert torch.equal(w, torch.tensor([math.exp(-d * d / 8.0) for d in range(5)], dtype=torch.float64).float())
    assert ops.check_ce_soft() == (0.0, 0.0, 0.0, None, None)
    assert ops.check_ce_soft(0.1, 1e-4, 0.2, 4, None, 512, 513) == (0.1, 1e-4, 0.2, 4, 2.0)
    assert ops.check_ce_soft(0.1, 0.0, 0.2, 31, 0.5, 512) == (0.1, 0.0, 0.2, 31, 0.5)
    for bad in (dict(neighbour_smoothing=1.0), dict(neighbour_smoothing=-0.1), dict(neighbour_smoothing=float("nan")),
                dict(label_smoothing=0.5, neighbour_smoothing=0.5, neighbour_range=2, codes=8),
                dict(neighbour_smoothing=0.2, codes=8), dict(neighbour_range=2), dict(neighbour_sigma=1.0),
                dict(neighbour_smoothing=0.2, neighbour_range=0, codes=8),
                dict(neighbour_smoothing=0.2, neighbour_range=32, codes=8),
                dict(neighbour_smoothing=0.2, neighbour_range=1.5, codes=8),
                dict(neighbour_smoothing=0.2, neighbour_range=2, neighbour_sigma=0.0, codes=8),
                dict(neighbour_smoothing=0.2, neighbour_range=2, neighbour_sigma=float("inf"), codes=8),
                dict(neighbour_smoothing=0.2, neighbour_range=2, neighbour_sigma=float("nan"), codes=8),
                dict(neighbour_smoothing=0.2, neighbour_range=2), dict(neighbour_smoothing=0.2, neighbour_range=2, codes=0),
                dict(neighbour_smoothing=0.2, neighbour_range=2, codes=9, classes=8), dict(label_smoothing=1.0),
                dict(z_loss=-1.0)):
        with pytest.raises(ValueError):
            ops.check_ce_soft(**bad)
