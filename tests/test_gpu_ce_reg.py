"""qarig_cross_entropy_reg_fwd (ce_reg_rows_kernel + mean2_kernel, csrc/loss.hip) on an MI355X through the C ABI, with
its own row_ws and flag: every case of tests/ce_reg_cases.py at every (label_smoothing, z_loss) of its grid against
fp64 within the emulation-derived tolerances, the bits of qarig_cross_entropy_fwd at (0, 0), the same bits without
dlogits, under a row permutation, from a logits pointer 4 bytes off a 16-byte boundary, and next to bad targets; the
argument errors.  tests/test_ce_reg_host.py shows on the CPU that these assertions reject the seven mutants.

Every figure is printed before it is asserted (`MEASURED ce_reg output family eps zeta worst tolerance`, u = 2^-24):
profiles/r23_ce_reg_tests.txt is made of those lines."""
import math

import pytest
import torch

import ce_reg_cases as G
import row_kernel_cases as R

pytestmark = pytest.mark.gpu

RUNS = [(R.CE_M, C, True) for C in G.REG_CLASSES] + [(M, C, False) for M, C in R.CE_MEAN_SHAPES]
IDS = [f"M{M}-C{C}" for M, C, _ in RUNS]


def _reg(x, t, eps, zeta, want_grad=True):
    """(row objectives, row nlls, dlogits, loss (2,), flag) of one call."""
    from qarig import _lib
    M, C = x.shape
    loss = torch.full((2,), -1.0, dtype=torch.float32, device="cuda")
    rows = torch.full((2 * M,), -1.0, dtype=torch.float32, device="cuda")
    dl = torch.empty((M, C), dtype=torch.float32, device="cuda") if want_grad else None
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    _lib.check(_lib.load().qarig_cross_entropy_reg_fwd(_lib.ptr(x), _lib.ptr(t), M, C, eps, zeta, _lib.ptr(loss),
                                                       _lib.ptr(dl), _lib.ptr(rows), _lib.ptr(flag), _lib.stream()),
               "qarig_cross_entropy_reg_fwd")
    return rows[:M], rows[M:], dl, loss, int(flag.item())


def _plain(x, t):
    from qarig import _lib
    M, C = x.shape
    loss = torch.empty((), dtype=torch.float32, device="cuda")
    rows = torch.full((M,), -1.0, dtype=torch.float32, device="cuda")
    dl = torch.empty_like(x)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    _lib.check(_lib.load().qarig_cross_entropy_fwd(_lib.ptr(x), _lib.ptr(t), M, C, _lib.ptr(loss), _lib.ptr(dl),
                                                   _lib.ptr(rows), _lib.ptr(flag), _lib.stream()),
               "qarig_cross_entropy_fwd")
    return rows, dl, loss


def _same(a, b):
    """Bit for bit (+inf equals +inf; these outputs hold no NaN)."""
    return all(torch.equal(p, q) for p, q in zip(a, b))


@pytest.mark.parametrize("M,C,mixed", RUNS, ids=IDS)
def test_rows_gradient_and_means(M, C, mixed):
    """Row objective, row nll, every gradient element, the gradient's row sum and both means on their own scales at
    every grid point; +inf objectives exactly where the reference has them; masked columns exact; NULL dlogits and a
    second launch the same bits."""
    c = R.ce_case(M, C, mixed)
    x, t = c.x.cuda(), c.t.cuda()
    masked = torch.isinf(c.x)
    bad = []
    for gi, (eps, zeta) in enumerate(G.REG_GRID):
        obj, nll, dl, loss, flag = _reg(x, t, eps, zeta)
        assert flag == 0
        m = G.reg_measures(c, gi, obj.cpu(), nll.cpu(), dl.cpu(), loss[0].cpu(), loss[1].cpu())
        for k in ("mean_obj", "mean_nll"):
            tol = G.reg_tol((k, gi))
            print(f"MEASURED ce_reg {k} all {eps} {zeta} {m[k]:.3f} {tol}")
            if not R.within(m[k], tol):
                bad.append((k, gi, m[k], tol))
        for k in ("obj", "nll", "dlogits", "dsum"):
            for fam in sorted(set(c.family)):
                w, tol = float(m[k][c.rows(fam)].max()), G.reg_tol((k, fam, gi))
                print(f"MEASURED ce_reg {k} {fam} {eps} {zeta} {w:.3f} {tol}")
                if not R.within(w, tol):
                    bad.append((k, fam, gi, w, tol, [r for r in c.rows(fam) if not R.within(float(m[k][r]), tol)]))
        # the +inf row objectives: the masked rows at eps > 0 and no others; everything else finite
        want_inf = c.rows("masked") if (eps > 0 and mixed) else []
        assert m["inf_rows"] == want_inf
        assert torch.nonzero(torch.isinf(obj.cpu())).flatten().tolist() == want_inf and (obj.cpu()[want_inf] > 0).all()
        assert math.isinf(float(loss[0])) == bool(want_inf)
        assert torch.isfinite(nll).all() and torch.isfinite(loss[1]) and torch.isfinite(dl).all()
        if masked.any():        # p == 0 exactly: 0 at eps = 0, (-eps / C) / M in the kernel's own fp32 otherwise
            col = -(torch.tensor(eps, dtype=torch.float32) / torch.tensor(float(C))) * \
                (torch.tensor(1.0) / torch.tensor(float(M)))
            assert (dl.cpu()[masked] == (col if eps > 0 else 0.0)).all(), (C, gi)
        assert _same((obj, nll, dl, loss), _reg(x, t, eps, zeta)[:4]), (C, gi, "two launches differ")
        obj3, nll3, none, loss3, flag3 = _reg(x, t, eps, zeta, want_grad=False)
        assert none is None and flag3 == 0 and _same((obj, nll, loss), (obj3, nll3, loss3)), (C, gi, "dlogits = NULL")
    assert not bad, (M, C, bad)


@pytest.mark.parametrize("M,C,mixed", RUNS, ids=IDS)
def test_bits_of_the_plain_entry_at_zero(M, C, mixed):
    c = R.ce_case(M, C, mixed)
    x, t = c.x.cuda(), c.t.cuda()
    rows, dl, loss = _plain(x, t)
    obj, nll, dlr, pair, _ = _reg(x, t, 0.0, 0.0)
    assert torch.equal(obj, rows) and torch.equal(nll, rows) and torch.equal(dlr, dl)
    assert torch.equal(pair[0], loss) and torch.equal(pair[1], loss)


@pytest.mark.parametrize("C", G.REG_CLASSES)
def test_row_independence_alignment_and_bad_targets(C):
    """A row permutation permutes the outputs bit for bit; a logits base 4 bytes off a 16-byte boundary (C = 513 rows
    are that anyway) gives the aligned copy's bits; bad targets set the flag, zero their own rows' losses and leave
    every other row's outputs untouched."""
    c = R.ce_case(R.CE_M, C)
    x, t = c.x.cuda(), c.t.cuda()
    perm = torch.randperm(c.M, generator=torch.Generator().manual_seed(C)).cuda()
    buf = torch.empty(x.numel() + 8, dtype=torch.float32, device="cuda")
    assert x.data_ptr() % 16 == 0 and buf.data_ptr() % 16 == 0
    xo = buf[1:1 + x.numel()].view(x.shape)
    xo.copy_(x)
    assert xo.data_ptr() % 16 == 4 and xo.is_contiguous()
    keep = [r for r in range(c.M) if r not in R.CE_BAD_ROWS]
    for eps, zeta in G.REG_GRID:
        obj, nll, dl, loss, _ = _reg(x, t, eps, zeta)
        objp, nllp, dlp, _, _ = _reg(x[perm].contiguous(), t[perm].contiguous(), eps, zeta)
        assert _same((objp, nllp, dlp), (obj[perm], nll[perm], dl[perm])), (C, eps, zeta, "permutation")
        assert _same(_reg(xo, t, eps, zeta)[:4], (obj, nll, dl, loss)), (C, eps, zeta, "unaligned base")
        objb, nllb, dlb, lossb, flagb = _reg(x, c.bad_targets().cuda(), eps, zeta)
        bad = list(R.CE_BAD_ROWS)
        assert flagb == 1 and (objb[bad] == 0).all() and (nllb[bad] == 0).all()
        assert _same((objb[keep], nllb[keep], dlb[keep]), (obj[keep], nll[keep], dl[keep])), (C, eps, zeta, "bad")
        assert torch.isfinite(lossb[1]) and torch.isfinite(dlb).all()


def test_argument_errors():
    from qarig import _lib
    lib = _lib.load()
    x, t = R.ce_case(R.CE_M, 41).x.cuda(), R.ce_case(R.CE_M, 41).t.cuda()
    M, C = x.shape
    loss = torch.zeros(2, device="cuda")
    rows = torch.zeros(2 * M, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    p = _lib.ptr

    def call(eps=0.1, zeta=1e-4, xs=x, ts=t, ls=loss, rs=rows, fl=flag, m=M, cc=C):
        return lib.qarig_cross_entropy_reg_fwd(p(xs), p(ts), m, cc, eps, zeta, p(ls), None, p(rs), p(fl), _lib.stream())

    for kw in (dict(eps=1.0), dict(eps=-0.1), dict(eps=1.5), dict(eps=float("nan")), dict(zeta=-1.0),
               dict(zeta=float("inf")), dict(zeta=float("nan")), dict(xs=None), dict(ts=None), dict(ls=None),
               dict(rs=None), dict(fl=None), dict(m=0), dict(cc=0), dict(m=-3)):
        assert call(**kw) == -1, kw
        assert "cross_entropy_reg" in _lib.last_error(), kw
    torch.cuda.synchronize()
    assert float(loss.abs().sum()) == 0 and int(flag.item()) == 0       # a refused call launches nothing
    assert call() == 0 and call(eps=0.0, zeta=0.0) == 0
