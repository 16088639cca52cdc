"""qarig_cross_entropy_soft_fwd (ce_reg_rows_kernel<., ., true> + mean2_kernel, csrc/loss.hip) on an MI355X through the
C ABI, with its own row_ws, flag and weight table: every case of tests/ce_soft_cases.py at every (label_smoothing,
z_loss, neighbour_smoothing) of its grid against fp64 within the emulation-derived tolerances, +inf exactly where the
reference has it, the bits of qarig_cross_entropy_reg_fwd at neighbour_smoothing = 0 and on rows with a special
target, the same losses without dlogits, the flag on bad targets, the argument errors.  tests/test_ce_soft_host.py
shows on the CPU that these assertions reject the eight mutants.

Every figure is printed before it is asserted (`MEASURED ce_soft output family eps zeta nu worst tolerance`,
u = 2^-24): profiles/r32_ce_soft_tests.txt is made of those lines."""
import math

import pytest
import torch

import ce_soft_cases as S
import row_kernel_cases as R

pytestmark = pytest.mark.gpu

RUNS = [(c.C, c.K, c.R, c.M) for c in S.soft_cases()]
IDS = [f"C{C}-K{K}-R{r}-M{M}" for C, K, r, M in RUNS]


def _soft(x, t, K, rng, w, eps, zeta, nu, want_grad=True):
    """(row objectives, row nlls, dlogits, loss (2,), flag) of one call."""
    from qarig import _lib
    M, C = x.shape
    loss = torch.full((2,), -1.0, dtype=torch.float32, device="cuda")
    rows = torch.full((2 * M,), -1.0, dtype=torch.float32, device="cuda")
    dl = torch.empty((M, C), dtype=torch.float32, device="cuda") if want_grad else None
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    _lib.check(_lib.load().qarig_cross_entropy_soft_fwd(_lib.ptr(x), _lib.ptr(t), M, C, K, eps, zeta, nu, rng,
                                                        _lib.ptr(w), _lib.ptr(loss), _lib.ptr(dl), _lib.ptr(rows),
                                                        _lib.ptr(flag), _lib.stream()),
               "qarig_cross_entropy_soft_fwd")
    return rows[:M], rows[M:], dl, loss, int(flag.item())


def _reg(x, t, eps, zeta):
    from qarig import _lib
    M, C = x.shape
    loss = torch.full((2,), -1.0, dtype=torch.float32, device="cuda")
    rows = torch.full((2 * M,), -1.0, dtype=torch.float32, device="cuda")
    dl = torch.empty((M, C), dtype=torch.float32, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    _lib.check(_lib.load().qarig_cross_entropy_reg_fwd(_lib.ptr(x), _lib.ptr(t), M, C, eps, zeta, _lib.ptr(loss),
                                                       _lib.ptr(dl), _lib.ptr(rows), _lib.ptr(flag), _lib.stream()),
               "qarig_cross_entropy_reg_fwd")
    return rows[:M], rows[M:], dl, loss


def _same(a, b):
    """Bit for bit (+inf equals +inf; these outputs hold no NaN)."""
    return all(torch.equal(p, q) for p, q in zip(a, b))


@pytest.mark.parametrize("C,K,rng,M", RUNS, ids=IDS)
def test_rows_gradient_and_means(C, K, rng, M):
    """Row objective, row nll, every gradient element, the gradient's row sum and both means on their own scales at
    every grid point; +inf objectives exactly where the reference has them; the gradient finite everywhere and exact
    on -inf columns; NULL dlogits and a second launch the same bits; special rows the regularised entry's bits."""
    c = S.soft_case(C, K, rng, M)
    x, t, w = c.x.cuda(), c.t.cuda(), c.w.cuda()
    masked = torch.isinf(c.x)
    special = (c.t >= K).cuda()
    bad = []
    for gi, (eps, zeta, nu) in enumerate(S.SOFT_GRID):
        obj, nll, dl, loss, flag = _soft(x, t, K, rng, w, eps, zeta, nu)
        assert flag == 0
        m = S.soft_measures(c, gi, obj.cpu(), nll.cpu(), dl.cpu(), loss[0].cpu(), loss[1].cpu())
        for k in ("mean_obj", "mean_nll"):
            tol = S.soft_tol((k, gi))
            print(f"MEASURED ce_soft {k} all {eps} {zeta} {nu} {m[k]:.3f} {tol}")
            if not R.within(m[k], tol):
                bad.append((k, gi, m[k], tol))
        for k in ("obj", "nll", "dlogits", "dsum"):
            for fam in sorted(set(c.family)):
                wst, tol = float(m[k][c.rows(fam)].max()), S.soft_tol((k, fam, gi))
                print(f"MEASURED ce_soft {k} {fam} {eps} {zeta} {nu} {wst:.3f} {tol}")
                if not R.within(wst, tol):
                    bad.append((k, fam, gi, wst, tol, [r for r in c.rows(fam) if not R.within(float(m[k][r]), tol)]))
        # the +inf row objectives: the masked rows at eps > 0, those with a -inf logit in their window at eps = 0
        want_inf = (c.rows("masked") if eps > 0 else S.window_inf_rows(c)) if M == R.CE_M else []
        assert m["inf_rows"] == want_inf
        assert torch.nonzero(torch.isinf(obj.cpu())).flatten().tolist() == want_inf and (obj.cpu()[want_inf] > 0).all()
        assert math.isinf(float(loss[0])) == bool(want_inf)
        assert torch.isfinite(nll).all() and torch.isfinite(loss[1]) and torch.isfinite(dl).all()
        if masked.any():
            # p == 0 exactly, so the element is (-eps / C - nu q) / M with no exp or log in it: sums, one division
            # and products, all correctly rounded -- the emulation's bits
            emu = S.soft_emulate(c.x, c.t, K, rng, c.w, eps, zeta, nu)[2]
            assert torch.equal(dl.cpu()[masked], emu[masked]), (C, K, rng, gi)
            assert (emu[masked] < 0).all() or eps == 0
        assert _same((obj, nll, dl, loss), _soft(x, t, K, rng, w, eps, zeta, nu)[:4]), (C, gi, "two launches differ")
        obj3, nll3, none, loss3, flag3 = _soft(x, t, K, rng, w, eps, zeta, nu, want_grad=False)
        assert none is None and flag3 == 0 and _same((obj, nll, loss), (obj3, nll3, loss3)), (C, gi, "dlogits = NULL")
        if special.any():       # nu = 0 by selects: the regularised entry's row outputs, bit for bit
            objr, nllr, dlr, _ = _reg(x, t, eps, zeta)
            assert _same((obj[special], nll[special], dl[special]), (objr[special], nllr[special], dlr[special]))
    assert not bad, (C, K, rng, M, bad)


def test_inf_row_counts():
    """No more +inf rows than the module states, over all cases."""
    n_nb = n_eps = 0
    for c in S.soft_cases():
        x, t, w = c.x.cuda(), c.t.cuda(), c.w.cuda()
        n_nb += int(torch.isinf(_soft(x, t, c.K, c.R, w, *S.SOFT_GRID[0])[0]).sum())
        n_eps += int(torch.isinf(_soft(x, t, c.K, c.R, w, *S.SOFT_GRID[1])[0]).sum())
    assert (n_nb, n_eps) == (S.SOFT_INF_ROWS_NB, S.SOFT_INF_ROWS_EPS)


@pytest.mark.parametrize("C,K,rng,M", RUNS, ids=IDS)
def test_bits_of_the_regularised_entry_at_zero(C, K, rng, M):
    """neighbour_smoothing = 0: qarig_cross_entropy_reg_fwd's bits on every output, with the table or without."""
    c = S.soft_case(C, K, rng, M)
    x, t, w = c.x.cuda(), c.t.cuda(), c.w.cuda()
    eps, zeta, nu = S.SOFT_BITS_POINT
    assert nu == 0.0
    want = _reg(x, t, eps, zeta)
    assert _same(_soft(x, t, K, rng, w, eps, zeta, nu)[:4], want)
    assert _same(_soft(x, t, K, 0, None, eps, zeta, nu)[:4], want)
    assert _same(_soft(x, t, K, rng, w, 0.0, 0.0, 0.0)[:4], _reg(x, t, 0.0, 0.0))


@pytest.mark.parametrize("C", S.SOFT_CLASSES)
def test_row_independence_and_bad_targets(C):
    """A row permutation permutes the outputs bit for bit; bad targets set the flag, zero their own rows' losses and
    leave every other row's outputs untouched."""
    c = S.soft_case(C, C - 1, 2)
    x, t, w = c.x.cuda(), c.t.cuda(), c.w.cuda()
    perm = torch.randperm(c.M, generator=torch.Generator().manual_seed(C)).cuda()
    keep = [r for r in range(c.M) if r not in (3, 30)]
    for eps, zeta, nu in S.SOFT_GRID:
        obj, nll, dl, loss, _ = _soft(x, t, c.K, c.R, w, eps, zeta, nu)
        objp, nllp, dlp, _, _ = _soft(x[perm].contiguous(), t[perm].contiguous(), c.K, c.R, w, eps, zeta, nu)
        assert _same((objp, nllp, dlp), (obj[perm], nll[perm], dl[perm])), (C, eps, zeta, nu, "permutation")
        objb, nllb, dlb, lossb, flagb = _soft(x, c.bad_targets().cuda(), c.K, c.R, w, eps, zeta, nu)
        assert flagb == 1 and (objb[[3, 30]] == 0).all() and (nllb[[3, 30]] == 0).all()
        assert _same((objb[keep], nllb[keep], dlb[keep]), (obj[keep], nll[keep], dl[keep])), (C, eps, zeta, nu, "bad")
        assert torch.isfinite(lossb[1]) and torch.isfinite(dlb).all()


def test_argument_errors():
    from qarig import _lib
    lib = _lib.load()
    c = S.soft_case(41, 40, 2)
    x, t, w = c.x.cuda(), c.t.cuda(), c.w.cuda()
    M, C = x.shape
    loss = torch.zeros(2, device="cuda")
    rows = torch.zeros(2 * M, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    p = _lib.ptr

    def call(eps=0.1, zeta=1e-4, nu=0.2, rng=2, ws=w, k=40, xs=x, ts=t, ls=loss, rs=rows, fl=flag, m=M, cc=C):
        return lib.qarig_cross_entropy_soft_fwd(p(xs), p(ts), m, cc, k, eps, zeta, nu, rng, p(ws), p(ls), None, p(rs),
                                                p(fl), _lib.stream())

    for kw in (dict(eps=1.0), dict(eps=-0.1), dict(eps=float("nan")), dict(zeta=-1.0), dict(zeta=float("inf")),
               dict(zeta=float("nan")), dict(nu=1.0), dict(nu=-0.1), dict(nu=float("nan")), dict(eps=0.5, nu=0.5),
               dict(eps=0.9, nu=0.2), dict(k=0), dict(k=-1), dict(k=C + 1), dict(rng=0), dict(rng=32), dict(rng=-1),
               dict(ws=None), dict(xs=None), dict(ts=None), dict(ls=None), dict(rs=None), dict(fl=None), dict(m=0),
               dict(cc=0), dict(m=-3), dict(nu=0.0, k=0), dict(nu=0.0, eps=1.0)):
        assert call(**kw) == -1, kw
        assert "cross_entropy_soft" in _lib.last_error(), kw
    torch.cuda.synchronize()
    assert float(loss.abs().sum()) == 0 and int(flag.item()) == 0       # a refused call launches nothing
    assert call() == 0 and call(k=C) == 0 and call(rng=31, ws=S.soft_table(31, 15.5).cuda()) == 0
    assert call(nu=0.0, rng=0, ws=None) == 0            # off: range and table are not looked at
