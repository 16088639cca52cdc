"""The row-reduction kernels on an MI355X, row by row against fp64 on the constructed families of
tests/row_kernel_cases.py: LayerNorm forward and backward at every width the host switches on (NV = 1, 2, 4, 8, the
scalar form, the misaligned fallback), cross-entropy with its per-row losses read back from `row_ws`, MSE past one
grid trip, and the LayerNorm prologue of the decode step's Linear kernels through a selector weight.  The tolerances
are row_kernel_cases' emulation-derived constants; tests/test_row_kernels_host.py shows on the CPU that these very
assertions reject a one-pass variance, the lse - x[t] loss, a dropped tail chunk, a mean or an MSE of one trip.

Every figure is printed before it is asserted (`MEASURED kernel output family worst tolerance`, in u = 2^-24):
profiles/row_kernels_measured.txt is made of those lines."""
import pytest
import torch

import row_kernel_cases as R

pytestmark = pytest.mark.gpu


def _note(kernel, output, family, value, tol):
    print(f"MEASURED {kernel} {output} {family} {value:.3f} {tol}")
    return R.within(value, tol)


def _dev(t):
    return None if t is None else t.cuda()


def _check_families(kernel, c, errors, tols, where):
    """errors {output: (M,) u}: per family the worst row against tols[(output, family)]."""
    bad = []
    for k, e in errors.items():
        for fam in sorted(set(c.family)):
            w = float(e[c.rows(fam)].max())
            if not _note(kernel, k, fam, w, tols[(k, fam)]):
                rows = [r for r in c.rows(fam) if not R.within(float(e[r]), tols[(k, fam)])]
                bad.append((k, fam, w, tols[(k, fam)], rows))
    assert not bad, (where, bad)


# ==== LayerNorm ==================================================================================================

def _offset_view(t):
    """A dense (M, D) copy of t that starts 4 bytes past a 16-byte boundary, inside a buffer this test owns."""
    buf = torch.empty(t.numel() + 8, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def _ln_fwd(x, args, unaligned):
    """(y, mean, rstd) of qarig_layernorm_fwd; unaligned: x and y both sit 4 bytes off, through the C entry."""
    from qarig import ops, _lib
    gamma, beta, scale, shift, idx = args
    if not unaligned:
        assert x.data_ptr() % 16 == 0
        return ops.layernorm_fwd(x, gamma, beta, scale, shift, mod_idx=idx)
    M, D = x.shape
    y = _offset_view(torch.zeros_like(x))
    mean, rstd = torch.empty(M, device="cuda"), torch.empty(M, device="cuda")
    p = _lib.ptr
    _lib.check(_lib.load().qarig_layernorm_fwd(p(x), M, D, R.EPS, p(gamma), p(beta), p(scale), p(shift), p(idx), p(y),
                                               p(mean), p(rstd), _lib.stream()), "qarig_layernorm_fwd")
    return y, mean, rstd


LN_RUNS = [(D, False) for D in R.LN_WIDTHS] + [(R.LN_UNALIGNED_D, True)]


@pytest.mark.parametrize("D,unaligned", LN_RUNS, ids=[f"D{D}{'-unaligned' if u else ''}" for D, u in LN_RUNS])
def test_layernorm_rows(D, unaligned):
    """Forward (mean, rstd, y) and backward (dx, dy_xhat) of all four forms, both dy, with and without dx_add: every
    row within its family's tolerance on its own scale; const rows bit-exact; two launches the same bits; a NaN and an
    inf stay in their rows."""
    from qarig import ops
    c = R.ln_case(D)
    place = _offset_view if unaligned else (lambda t: t)
    tag = "unaligned" if unaligned else ("vec" if D in R.LN_FWD_VEC else "scalar")
    tagb = "unaligned" if unaligned else ("vec" if D in R.LN_BWD_VEC else "scalar")
    x, xbad = place(c.x.cuda()), place(c.nonfinite().cuda())
    const = c.rows("const")
    keep = [r for r in range(c.M) if r not in R.LN_BAD_ROWS]
    rstd0 = 1.0 / torch.sqrt(torch.tensor(R.EPS, dtype=torch.float32))
    for form in R.LN_FORMS:
        args, mul, add = c.operands(form)
        gargs = tuple(_dev(t) for t in args)
        y, mean, rstd = _ln_fwd(x, gargs, unaligned)
        again = _ln_fwd(x, gargs, unaligned)
        assert all(torch.equal(a, b) for a, b in zip((y, mean, rstd), again)), (form, "two launches differ")
        rm, rr, _, ry = R.ln_fwd_ref(c.x, mul, add)
        got = {"mean": mean.cpu(), "rstd": rstd.cpu(), "y": y.cpu()}
        _check_families(f"layernorm_fwd[{tag}]", c, R.ln_measures(c.x, got, {"mean": rm, "rstd": rr, "y": ry}),
                        R.LN_TOL_U, (D, form))
        # const rows: the mean is the integer, the variance 0, y the addend -- bit for bit
        assert torch.equal(got["mean"][const], c.x[const, 0]) and (got["rstd"][const] == rstd0).all(), (D, form)
        assert torch.equal(got["y"][const], add[const]), (D, form)
        gam, sc, idx = gargs[0], gargs[2], gargs[4]
        first = True
        for kind, with_add in R.BWD_ARMS:
            dy = c.dy[kind].cuda()
            a = c.dx_add.cuda() if with_add else None
            dx, dh = ops.layernorm_bwd(dy, x, mean, rstd, gamma=gam, scale=sc, want_dy_xhat=True, mod_idx=idx, dx_add=a)
            rdx, rdh = R.ln_bwd_ref(c.x, c.dy[kind], mul, c.dx_add if with_add else None)
            _check_families(f"layernorm_bwd[{tagb}]", c,
                            R.ln_measures(c.x, {"dx": dx.cpu(), "dy_xhat": dh.cpu()}, {"dx": rdx, "dy_xhat": rdh}),
                            R.LN_TOL_U, (D, form, kind, with_add))
            assert (dh.cpu()[const] == 0).all()
            if first:
                dx2, dh2 = ops.layernorm_bwd(dy, x, mean, rstd, gamma=gam, scale=sc, want_dy_xhat=True, mod_idx=idx,
                                             dx_add=a)
                assert torch.equal(dx, dx2) and torch.equal(dh, dh2), (form, "two launches differ")
                dx3, none = ops.layernorm_bwd(dy, x, mean, rstd, gamma=gam, scale=sc, mod_idx=idx, dx_add=a)
                assert none is None and torch.equal(dx, dx3)
                # nonfinite: the NaN row and the inf row are lost, every other row of every output keeps its bits
                yb, mb, rb = _ln_fwd(xbad, gargs, unaligned)
                dxb, dhb = ops.layernorm_bwd(dy, xbad, mb, rb, gamma=gam, scale=sc, want_dy_xhat=True, mod_idx=idx,
                                             dx_add=a)
                for clean, dirty in ((y, yb), (mean, mb), (rstd, rb), (dx, dxb), (dh, dhb)):
                    assert torch.equal(clean[keep], dirty[keep]), (D, form, "a non-finite row leaked")
                assert not torch.isfinite(yb[list(R.LN_BAD_ROWS)]).all(1).any()
                first = False


# ==== cross-entropy ==============================================================================================

def _ce(x, t, want_grad=True):
    """qarig_cross_entropy_fwd with its own row_ws and flag: (row losses, dlogits, mean loss, flag)."""
    from qarig import _lib
    M, C = x.shape
    loss = torch.empty((), dtype=torch.float32, device="cuda")
    rows = torch.full((M,), -1.0, dtype=torch.float32, device="cuda")
    dl = torch.empty_like(x) if want_grad else None
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    _lib.check(_lib.load().qarig_cross_entropy_fwd(_lib.ptr(x), _lib.ptr(t), M, C, _lib.ptr(loss), _lib.ptr(dl),
                                                   _lib.ptr(rows), _lib.ptr(flag), _lib.stream()),
               "qarig_cross_entropy_fwd")
    return rows, dl, loss, int(flag.item())


CE_RUNS = [(R.CE_M, C, True) for C in R.CE_CLASSES] + [(M, C, False) for M, C in R.CE_MEAN_SHAPES]


@pytest.mark.parametrize("M,C,mixed", CE_RUNS, ids=[f"M{M}-C{C}" for M, C, _ in CE_RUNS])
def test_cross_entropy_rows(M, C, mixed):
    """Row losses, every gradient element, the gradient's row sum and the mean loss on their own scales; masked
    entries exactly 0; the same bits without dlogits and on a second launch; bad targets flagged, their rows 0, every
    other row untouched."""
    c = R.ce_case(M, C, mixed)
    x, t = c.x.cuda(), c.t.cuda()
    rows, dl, loss, flag = _ce(x, t)
    assert flag == 0
    e_loss, e_d, e_sum, e_mean = R.ce_measures(c, rows.cpu(), dl.cpu(), loss.cpu())
    tols = dict(R.CE_TOL_U)
    tols.update({("dsum", f): R.CE_TOL_U[("dlogits", f)] for f in R.CE_FAMILIES})
    ok = _note("cross_entropy", "mean", "all", e_mean, R.CE_MEAN_TOL_U)
    _check_families("cross_entropy", c, {"loss": e_loss, "dlogits": e_d, "dsum": e_sum}, tols, (M, C))
    assert ok, (M, C, "mean loss", e_mean)
    masked = torch.isinf(c.x)
    assert (dl.cpu()[masked] == 0).all() and torch.isfinite(rows).all() and torch.isfinite(dl).all()
    rows2, dl2, loss2, _ = _ce(x, t)
    assert torch.equal(rows, rows2) and torch.equal(dl, dl2) and torch.equal(loss, loss2)
    rows3, none, loss3, flag3 = _ce(x, t, want_grad=False)
    assert none is None and flag3 == 0 and torch.equal(rows, rows3) and torch.equal(loss, loss3)
    if mixed:
        rowsb, dlb, lossb, flagb = _ce(x, c.bad_targets().cuda())
        assert flagb == 1
        bad = list(R.CE_BAD_ROWS)
        keep = [r for r in range(M) if r not in bad]
        assert (rowsb[bad] == 0).all()
        assert torch.equal(rowsb[keep], rows[keep]) and torch.equal(dlb[keep], dl[keep])
        assert torch.isfinite(lossb) and torch.isfinite(dlb).all()


# ==== MSE ========================================================================================================

@pytest.mark.parametrize("n", R.MSE_SIZES)
def test_mse(n):
    """The loss against fp64 within the emulation-derived tolerance, dpred within the derived 2 u of 2 (a - b) / n,
    at sizes below, at and past one grid trip of 1024 x 256 threads."""
    from qarig import ops
    bad = []
    for fam in R.MSE_FAMILIES:
        a, b = R.mse_case(n, fam)
        ga, gb = a.cuda(), b.cuda()
        loss, dp = ops.mse_fwd(ga, gb)
        e, ed = R.mse_measures(a, b, loss.cpu(), dp.cpu())
        if not _note("mse", "loss", fam, e, R.MSE_TOL_U[("loss", fam)]):
            bad.append(("loss", fam, e))
        if not _note("mse", "dpred", fam, ed, R.MSE_DPRED_TOL_U):
            bad.append(("dpred", fam, ed))
        loss2, none = ops.mse_fwd(ga, gb, want_grad=False)
        loss3, dp3 = ops.mse_fwd(ga, gb)
        assert none is None and torch.equal(loss, loss2) and torch.equal(loss, loss3) and torch.equal(dp, dp3)
    assert not bad, (n, bad)


# ==== the decode step's LayerNorm prologue =======================================================================

@pytest.mark.parametrize("K", R.DEC_K)
def test_decode_linear_layernorm_prologue(K):
    """y = LN(x) W^T with row n of W one-hot at kappa(n): every product but one is an exact zero, so y[m, n] is the
    normalised value LN(x)[m, kappa(n)] and the prologue of both kernels (all rows per lane: decode_rows = 0; rows
    split over the waves: decode_rows = 2), with fp32 weights and their bf16 image, is judged per row like the
    training kernel -- same measure, same tolerances; const rows give the addend bit for bit."""
    from qarig import ops, _lib
    c = R.ln_case(K, max(R.DEC_M), "decode")
    kappa = R.dec_kappa(K)
    W32 = R.dec_weight(K).cuda()
    assert torch.equal(W32.bfloat16().float(), W32)
    weights = {"f32": W32, "bf16": W32.bfloat16()}
    bad = []
    for opt, kernel in ((0, "all_rows"), (2, "row_split")):
        old = _lib.set_option("decode_rows", opt)
        try:
            for M in R.DEC_M:
                starts = range(len(R.DEC_FAMILIES)) if M == 1 else (0,)
                for r0 in starts:
                    rows = list(range(r0, r0 + M))
                    x = c.x[rows].contiguous().cuda()
                    for form in R.DEC_FORMS:
                        mul, add = R.dec_operands(c, form)
                        if form == "affine":
                            kw = dict(gamma=c.gamma.cuda(), beta=c.beta.cuda())
                        elif form == "rows":
                            kw = dict(scale=c.scale[rows].contiguous().cuda(), shift=c.shift[rows].contiguous().cuda())
                        else:
                            kw = dict(scale=c.scale[0].cuda(), shift=c.shift[0].cuda())
                        ref = R.ln_fwd_ref(c.x[rows], mul[rows], add[rows])[3][:, kappa]
                        for wname, W in weights.items():
                            if wname == "bf16" and opt == 0 and M > 4:
                                continue              # a bf16 image of more than 4 rows always takes the row split
                            assert ops.decode_linear_supported(M, K, K, ln=True)
                            y = ops.decode_linear(x, W, **kw).cpu()
                            assert torch.equal(y, ops.decode_linear(x, W, **kw).cpu())
                            e = R.worst_or_exact((y.double() - ref).abs().max(1).values, ref.abs().max(1).values)
                            for i, r in enumerate(rows):
                                fam = c.family[r]
                                tol = R.LN_TOL_U[("y", fam)]
                                if not _note(f"decode_linear[{kernel},{wname}]", "y", fam, float(e[i]), tol):
                                    bad.append((kernel, wname, M, r, form, fam, float(e[i]), tol))
                                if fam == "const":
                                    assert torch.equal(y[i], add[r][kappa]), (kernel, wname, M, r, form)
        finally:
            _lib.set_option("decode_rows", old)
    assert not bad, (K, bad)
