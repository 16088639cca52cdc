"""CPU self-test of tests/row_kernel_cases.py: the row families are what they claim, every stored tolerance is twice
the recomputed worst error of the intended fp32 emulation on the GPU test's own inputs (rounded up to a whole u),
that emulation passes every assertion of tests/test_gpu_row_kernels.py, and each of the five mutants fails at least
one of them -- in the family named in REJECTED_BY.  So a failure of the GPU test is the kernel's."""
import math

import pytest
import torch

import row_kernel_cases as R

# mutant -> (table, key) it must fail; the families that catch it besides are printed
REJECTED_BY = {
    "one_pass": ("ln", ("rstd", "offset")),
    "lse": ("ce", ("loss", "offset")),
    "drop_tail": ("ln", ("mean", "unit")),
    "mean_256": ("ce", "mean"),
    "one_trip": ("mse", ("loss", "unit")),
}


def test_layernorm_rows_are_what_they_claim():
    cases = [c for c, _, _, _ in R.ln_runs()] + [R.ln_case(K, max(R.DEC_M), "decode") for K in R.DEC_K]
    for c in cases:
        D = c.D
        train = c.M == R.LN_M
        assert c.M % 4 != 0 or not train
        for fam in (R.LN_FAMILIES if train else R.DEC_FAMILIES):
            assert len(c.rows(fam)) >= 3, (D, fam)
        x = c.x.double()
        for r in c.rows("const"):
            assert (c.x[r] == c.x[r, 0]).all() and float(c.x[r, 0]) == int(c.x[r, 0]) and abs(int(c.x[r, 0])) <= 16
            assert float(x[r].mean()) == float(c.x[r, 0])                      # the mean is exact
            assert float(R.row_sum(c.x[r:r + 1])[0] / torch.tensor(float(D))) == float(c.x[r, 0])
        offs = sorted({c.param[r] for r in c.rows("offset")})
        exps = sorted({c.param[r] for r in c.rows("scaled")})
        assert {abs(o) for o in offs} == {10.0, 100.0, 1000.0} and min(offs) < 0 < max(offs)
        assert min(exps) == -20 and max(exps) == 20
        if D >= 32:
            for r in c.rows("offset"):
                assert abs(float(x[r].mean()) - c.param[r]) < 1.0 and 0.5 < float(x[r].std()) < 1.5
            for r in c.rows("scaled"):
                assert 0.5 < float(x[r].std()) / 2.0 ** c.param[r] < 1.5
            # small-scale rows put eps in play: the variance is far below it
            assert min(float(x[r].var()) for r in c.rows("scaled")) < 1e-3 * R.EPS
        if train:
            last = D - 1
            assert c.outlier_cols[:3] == (0, min(63, last), last) and c.outlier_cols[3] // 64 == last // 64
            assert {c.param[r] for r in c.rows("outlier")} == {0, 1, 2, 3}
            if D >= 32:
                for r in c.rows("outlier"):
                    col = c.outlier_cols[c.param[r]]
                    assert int(x[r].abs().argmax()) == col or float(x[r, col].abs()) > 50
            idx = c.mod_idx.tolist()
            assert 0 in idx and R.LN_TABLE_ROWS - 1 in idx and len(set(idx)) < len(idx) and idx != sorted(idx)
            assert set(idx) == set(range(R.LN_TABLE_ROWS))
            bad = c.nonfinite()
            changed = (bad != c.x) | torch.isnan(bad)
            assert int(changed.sum()) == 2 and torch.isnan(bad[R.LN_BAD_ROWS[0]]).sum() == 1
            assert torch.isinf(bad[R.LN_BAD_ROWS[1]]).sum() == 1
            assert ((c.dy["onehot"] != 0).sum(1) == 1).all() and (c.dy["full"] != 0).all()
    assert set(R.LN_FWD_VEC) | set(R.LN_BWD_VEC) <= set(R.LN_WIDTHS) and 768 in R.LN_WIDTHS
    assert all(D % 256 or D in R.LN_FWD_VEC or D == 768 for D in R.LN_WIDTHS)


def test_cross_entropy_rows_are_what_they_claim():
    for C in R.CE_CLASSES:
        c = R.ce_case(R.CE_M, C)
        last = C - 1
        places = {0, last, 64 * (last // 64) + (last % 64) // 2}
        assert ((c.t >= 0) & (c.t < C)).all()
        for fam in R.CE_FAMILIES:
            rows = c.rows(fam)
            assert len(rows) >= 3, (C, fam)
            assert {int(c.t[r]) for r in rows} >= places, (C, fam)             # every family meets every place
        loss, p, _, _ = R.ce_ref(c.x, c.t)
        assert torch.isfinite(loss).all()
        means = sorted(round(float(c.x[r].mean()), -1) for r in c.rows("offset"))
        assert means[0] == -100.0 and means[-1] == 1000.0 and 100.0 in means
        for r in c.rows("peak_target"):
            assert int(c.x[r].argmax()) == int(c.t[r]) and float(loss[r]) < 0.5
        for r in c.rows("peak_other"):
            assert int(c.x[r].argmax()) != int(c.t[r]) and 5.0 < float(loss[r]) < 40.0
        for r in c.rows("ties"):
            assert (c.x[r] == c.x[r, 0]).all() and abs(float(loss[r]) - math.log(C)) < 1e-12
            assert float((p[r] - 1.0 / C).abs().max()) < 1e-12          # (fp64 rounds at |x| = 1000)
        for r in c.rows("masked"):
            m = torch.isinf(c.x[r])
            assert 1 <= int(m.sum()) and (C < 9 or int(m.sum()) >= 3) and not m[c.t[r]] and (c.x[r][m] < 0).all()
            assert (p[r][m] == 0).all()
        t = c.bad_targets()
        assert int(t[R.CE_BAD_ROWS[0]]) == C and int(t[R.CE_BAD_ROWS[1]]) == -1 and int((t != c.t).sum()) == 2
    assert [M for M, _ in R.CE_MEAN_SHAPES] == [1, 255, 256, 257, 16385]


def test_mse_data_is_what_it_claims():
    assert R.MSE_GRID == 262144 and R.MSE_SIZES == (1, 255, 257, 262144, 262145, 2 * 262144 + 77)
    for n in R.MSE_SIZES:
        a, b = R.mse_case(n, "offset")
        assert (a - b).double().equal(a.double() - b.double()) and (a != b).all()      # the difference is exact
        assert float((a - 1000).abs().max()) <= 0.5 and float((b - 1000).abs().max()) <= 0.5 + 2.0 ** -10
        for fam in R.MSE_FAMILIES:
            a, b = R.mse_case(n, fam)
            assert a.shape == b.shape == (n,) and float(R.mse_ref(a, b)[0]) > 0
    a, _ = R.mse_case(R.MSE_SIZES[-1], "mixed")
    assert float(a.abs().max()) > 2.0 ** 9 and float(a.abs().median()) < 2.0 ** 2


def test_emulation_primitives():
    """The lane-order sums are sums, fma32 is a fused multiply-add, the tree mean is a mean."""
    g = torch.Generator().manual_seed(0)
    v = torch.randn((5, 512), generator=g)
    for vec in (False, True):
        assert float((R.row_sum(v, vec).double() - v.double().sum(1)).abs().max()) < 1e-4
        assert float((R.row_dot(v, v, vec).double() - (v.double() ** 2).sum(1)).abs().max()) < 1e-3
    w = torch.randn((3, 100), generator=g)
    assert float((R.row_sum(w).double() - w.double().sum(1)).abs().max()) < 1e-5
    a = torch.tensor([1.0 + 2.0 ** -12])
    assert float(R.fma32(a, a, -(a * a))) == float(a.double() ** 2 - (a * a).double()) != 0.0
    for n in (1, 255, 256, 257, 1000):
        x = torch.randn(n, generator=g)
        assert abs(float(R.mean_emulate(x, torch.tensor(1.0 / n))) - float(x.double().mean())) < 1e-6
        assert (n <= 256) == (float(R.mean_emulate(x, torch.tensor(1.0 / n), True)) ==
                              float(R.mean_emulate(x, torch.tensor(1.0 / n))))


@pytest.fixture(scope="module")
def worst():
    return {"ln": R.ln_emulation_worst(), "ce": R.ce_emulation_worst(), "mse": R.mse_emulation_worst()}


def test_tolerances_are_twice_the_emulation_on_the_gpu_tests_own_inputs(worst):
    stored = {"ln": dict(R.LN_TOL_U), "ce": dict(R.CE_TOL_U, mean=R.CE_MEAN_TOL_U), "mse": dict(R.MSE_TOL_U)}
    assert set(stored["ln"]) == {(o, f) for o in ("mean", "rstd", "y", "dx", "dy_xhat") for f in R.LN_FAMILIES}
    assert set(stored["ce"]) == {(o, f) for o in ("loss", "dlogits") for f in R.CE_FAMILIES} | {"mean"}
    assert set(stored["mse"]) == {("loss", f) for f in R.MSE_FAMILIES}
    for table, tols in stored.items():
        for key, tol in tols.items():
            w = worst[table][key]
            print(f"{table} {key}: emulation worst {w:.3f} u, tolerance {tol} u")
            assert tol == math.ceil(2 * w), (table, key, w)
    # exact where the family is exact; dpred inside the derived bound
    for key in (("mean", "const"), ("y", "const"), ("dy_xhat", "const")):
        assert R.LN_TOL_U[key] == 0
    for fam in R.MSE_FAMILIES:
        assert worst["mse"][("dpred", fam)] <= R.MSE_DPRED_TOL_U


def test_intended_emulation_passes_every_gpu_assertion(worst):
    assert R.ln_failures(worst["ln"]) == [] and R.ce_failures(worst["ce"]) == [] and R.mse_failures(worst["mse"]) == []
    # the bit-exact claims of the const family, at every width
    eps = torch.tensor(R.EPS, dtype=torch.float32)
    for c, fv, _, _ in R.ln_runs():
        rows = c.rows("const")
        for form in R.LN_FORMS:
            _, mul, add = c.operands(form)
            mean, rstd, y = R.ln_fwd_emulate(c.x, form, mul, add, fv)
            assert torch.equal(mean[rows], c.x[rows, 0]) and torch.equal(y[rows], add[rows])
            assert (rstd[rows] == 1.0 / torch.sqrt(eps)).all()
    # non-finite rows stay in their rows
    c = R.ln_case(100)
    _, mul, add = c.operands("affine")
    clean = R.ln_fwd_emulate(c.x, "affine", mul, add, False)
    dirty = R.ln_fwd_emulate(c.nonfinite(), "affine", mul, add, False)
    keep = [r for r in range(c.M) if r not in R.LN_BAD_ROWS]
    for a, b in zip(clean, dirty):
        assert torch.equal(a[keep], b[keep]) and not torch.isfinite(b[list(R.LN_BAD_ROWS)]).all(-1).any()


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_every_mutant_is_rejected(mutant):
    failed = R.mutant_verdicts(mutant)
    print(f"{mutant}: rejected by " + "; ".join(f"{t}: {', '.join(map(str, k))}" for t, k in failed.items() if k))
    table, key = REJECTED_BY[mutant]
    assert key in failed[table], (mutant, failed)
    assert any(failed.values())


def test_rejections_stand_far_above_the_tolerances():
    """One-pass variance on offset rows and the lse form on offset logits: not borderline."""
    one = R.ln_verdicts(lambda *a: R.ln_fwd_emulate(*a, mutant="one_pass"), R.ln_bwd_emulate, decode=False)
    assert one[("rstd", "offset")] > 1000 * R.LN_TOL_U[("rstd", "offset")]
    lse = R.ce_verdicts(lambda x, t: R.ce_emulate(x, t, "lse"), [R.ce_case(R.CE_M, C) for C in R.CE_CLASSES])
    assert lse[("loss", "offset")] > 10 * R.CE_TOL_U[("loss", "offset")]
    assert lse[("dlogits", "offset")] > 5 * R.CE_TOL_U[("dlogits", "offset")]


def test_measures_see_one_wrong_row():
    """A row wrong by 2^-15 of its own scale next to rows 2^20 times larger: a global maximum would not see it."""
    c = R.ln_case(512)
    _, mul, add = c.operands("affine")
    rm, rr, _, ry = R.ln_fwd_ref(c.x, mul, add)
    mean, rstd, y = R.ln_fwd_emulate(c.x, "affine", mul, add, True)
    r = next(r for r in c.rows("scaled") if c.param[r] == -20)
    y = y.clone()
    y[r, 7] += float(ry[r].abs().max()) * 2.0 ** -15
    e = R.ln_measures(c.x, {"mean": mean, "rstd": rstd, "y": y}, {"mean": rm, "rstd": rr, "y": ry})["y"]
    bad = [i for i in range(c.M) if not R.within(float(e[i]), R.LN_TOL_U[("y", c.family[i])])]
    assert bad == [r]
    # and a NaN is a failure, not a pass
    assert not R.within(float("nan"), 1e30) and R.worse(3.0, float("nan")) != R.worse(3.0, float("nan"))
    assert R.worse(float("nan"), 3.0) != 3.0
