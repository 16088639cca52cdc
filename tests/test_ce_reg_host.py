"""tests/ce_reg_cases.py on the CPU: the fp64 reference is torch's label-smoothed cross-entropy plus the z-loss, the
tolerance table is what the emulation gives, the emulation at (0, 0) is row_kernel_cases.ce_emulate bit for bit, every
mutant is rejected by the GPU test's own cells on the GPU test's own inputs, and no row escapes a verdict."""
import functools

import pytest
import torch

import ce_reg_cases as G
import row_kernel_cases as R


@functools.lru_cache(maxsize=None)
def _emulation():
    return G.reg_verdicts(G.reg_emulate)


def test_reference_is_torch_label_smoothing_plus_z_loss():
    """Row objectives against F.cross_entropy(label_smoothing) + zeta logsumexp^2 in fp64 (+inf where torch gives
    +inf), the plain nll against F.cross_entropy, and M dlogits against autograd within 1e-12 on the finite rows."""
    for c in G.reg_cases()[:len(G.REG_CLASSES)] + G.reg_cases()[-4:-1]:
        for gi, (eps, zeta) in enumerate(G.REG_GRID):
            eps, zeta = G.f32(eps), G.f32(zeta)
            ref = G.reg_ref(c, gi)
            x = c.x.double().requires_grad_(True)
            rows = torch.nn.functional.cross_entropy(x, c.t, label_smoothing=eps, reduction="none") + \
                zeta * torch.logsumexp(x, 1) ** 2
            inf = torch.isinf(rows.detach())
            assert torch.equal(inf, torch.isinf(ref["obj"])) and (ref["obj"][inf] > 0).all()
            assert int(inf.sum()) == (5 if eps > 0 and len(set(c.family)) > 1 else 0)
            fin = ~inf
            torch.testing.assert_close(ref["obj"][fin], rows.detach()[fin], rtol=1e-12, atol=1e-12)
            plain = torch.nn.functional.cross_entropy(c.x.double(), c.t, reduction="none")
            torch.testing.assert_close(ref["nll"], plain, rtol=1e-12, atol=1e-12)
            assert torch.isfinite(ref["nll"]).all() and torch.isfinite(ref["dlogits"]).all()
            rows[fin].sum().backward()
            g = ref["dlogits"][fin] * c.M
            assert float((g - x.grad[fin]).abs().max()) <= 1e-12 * float(g.abs().max()), (c.C, gi)
            if eps > 0 and inf.any():       # the -inf columns of the masked rows get -eps / (C M)
                masked = torch.isinf(c.x) & inf[:, None]
                assert masked.any() and (ref["dlogits"][masked] == -eps / c.C / c.M).all()


def test_tolerance_table_is_twice_the_emulation():
    worst, _, _ = _emulation()
    rows = {k: G.tolerance_of(w) for k, w in worst.items() if len(k) == 3 and k[0] != "dsum"}
    means = {k: G.tolerance_of(w) for k, w in worst.items() if len(k) == 2}
    assert rows == G.REG_TOL_U and means == G.REG_MEAN_TOL_U
    assert len(rows) == len(G.REG_ROW_OUTPUTS) * len(R.CE_FAMILIES) * len(G.REG_GRID)
    assert not G.reg_failures(worst)            # the gradient sums sit inside dlogits' tolerance as argued
    # of the size the plain kernel's are; the plain cells at (0, 0) on row_kernel_cases' own class counts ARE its table
    assert max(G.REG_TOL_U.values()) <= max(R.CE_TOL_U.values())
    plain = G.reg_verdicts(G.reg_emulate, cases=R.ce_cases(), grid=(0,))[0]
    for (k, fam), tol in R.CE_TOL_U.items():
        assert G.tolerance_of(plain[("nll" if k == "loss" else k, fam, 0)]) == tol


def test_emulation_at_zero_is_the_plain_emulation_bit_for_bit():
    for c in G.reg_cases():
        obj, nll, d, mobj, mnll = G.reg_emulate(c.x, c.t, 0.0, 0.0)
        loss, dl, mean = R.ce_emulate(c.x, c.t)
        assert torch.equal(obj, loss) and torch.equal(nll, loss) and torch.equal(d, dl)
        assert torch.equal(mobj, mean) and torch.equal(mnll, mean)


# which cells must see each mutant: (outputs, families, grid points) of which at least one combination fails
EXPECT = {
    "unshifted": (("obj",), ("offset",), (1, 3)),
    "no_eps_grad": (("dlogits", "dsum"), R.CE_FAMILIES, (1, 3, 4)),
    "no_one_minus_eps": (("dlogits", "dsum"), R.CE_FAMILIES, (1, 3, 4)),
    "single_zeta": (("dlogits", "dsum"), R.CE_FAMILIES, (2, 3, 4)),
    "eps_multiplied": (("obj",), ("masked",), (0, 2)),
    "drop_tail": (("obj", "nll", "dlogits"), R.CE_FAMILIES, range(len(G.REG_GRID))),
}


@pytest.mark.parametrize("mutant", G.REG_MUTANTS)
def test_mutant_is_rejected(mutant):
    failed = G.mutant_failures(mutant)
    assert failed, mutant
    if mutant == "mean_256":
        assert set(failed) == {(k, gi) for k in ("mean_obj", "mean_nll") for gi in range(len(G.REG_GRID))}
        return
    outs, fams, grid = EXPECT[mutant]
    hit = [k for k in failed if len(k) == 3 and k[0] in outs and k[1] in fams and k[2] in grid]
    assert hit, (mutant, failed)
    if mutant in ("no_eps_grad", "no_one_minus_eps", "single_zeta"):     # a wrong formula: every family sees it
        assert {k[1] for k in hit} == set(R.CE_FAMILIES)
        # and it is wrong only where its coefficient is on
        assert all(k[-1] in grid for k in failed), failed
    if mutant == "eps_multiplied":     # NaN on the masked rows at eps = 0, nowhere else
        assert all(k[-1] in grid for k in failed), failed


def test_every_row_enters_a_verdict():
    """Each (case, grid point, row) is judged on its four row outputs; the only entries without an error figure are
    the +inf row objectives of the masked rows at eps > 0 (5 rows x 9 class counts per such grid point), which must
    be equal; there is no NaN anywhere in the emulation's verdicts."""
    worst, judged, excused = _emulation()
    rows = sum(c.M for c in G.reg_cases())
    assert judged == 4 * rows * len(G.REG_GRID)
    n_eps = sum(1 for e, _ in G.REG_GRID if e > 0)
    assert G.REG_INF_ROWS == 45 and excused == n_eps * G.REG_INF_ROWS
    assert all(w == w and w != float("inf") for w in worst.values())
    for c in G.reg_cases()[:len(G.REG_CLASSES)]:
        assert sorted(set(c.family)) == sorted(R.CE_FAMILIES) and len(c.rows("masked")) == 5
        for gi, (e, _) in enumerate(G.REG_GRID):
            m = G.reg_measures(c, gi, *G.reg_emulate(c.x, c.t, *G.REG_GRID[gi]))
            assert m["inf_rows"] == (c.rows("masked") if e > 0 else [])
