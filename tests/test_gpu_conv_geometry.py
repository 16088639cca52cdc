"""The conv entry points of csrc/conv.hip at every geometry and pointer alignment they accept, against fp64
(tests/conv_cases.py holds the cases and says what each is there for).

Two arms.  EXACT: small-integer operands, every partial sum an integer below 2^24 (tests/test_conv_cases_host.py
proves it per case), so y, preact, dx, dw and db must equal the fp64 reference bit for bit on every element,
whichever kernel family, tile shape or split count served the call.  FP64: the float operands and tolerances of
tests/test_gpu_conv.py (pre 2e-6, y 4e-6, every gradient 1e-5)."""
import pytest
import torch

from conftest import grad_err, rel_err
import conv_cases as cc

pytestmark = pytest.mark.gpu


def _ids(cases):
    return [c.name for c in cases]


class _options:
    def __init__(self, opts):
        self.opts = opts

    def __enter__(self):
        from qarig import _lib
        self.olds = []
        for name, v in self.opts:
            self.olds.append((name, _lib.set_option(name, v)))

    def __exit__(self, *exc):
        from qarig import _lib
        for name, old in reversed(self.olds):
            _lib.set_option(name, old)


def _forward(c, x, w, b, act):
    from qarig import functional as QF
    if c.kind == "convt":
        return QF.conv_transpose2d_act(x, w, b, act)
    return QF.conv2d_act(x, w, b, c.stride, c.pad, act)


def _forward_pre(c, x, w, b, act):
    from qarig import ops
    if c.kind == "convt":
        return ops.conv_transpose2d_fwd(x, w, b, act, want_preact=True)
    return ops.conv2d_fwd(x, w, b, c.stride, c.pad, act, want_preact=True)


def _exact_fwd_bwd(c, bias=True):
    """y, dx, dw, db of the autograd node at act 0 on integer operands: every element equal to fp64."""
    (x, w, b, dy), ref, ref_nb = cc.int_case(c)
    if not bias:
        b, ref = None, ref_nb
    g = [t.cuda().requires_grad_(True) if t is not None else None for t in (x, w, b)]
    y = _forward(c, g[0], g[1], g[2], 0)
    assert y.shape == ref.y.shape
    assert torch.equal(y.detach().double().cpu(), ref.y), c.name
    (y * dy.cuda()).sum().backward()
    for name, got, want in (("dx", g[0].grad, ref.dx), ("dw", g[1].grad, ref.dw),
                            ("db", g[2].grad if bias else None, ref.db)):
        if want is None:
            assert got is None
            continue
        assert got.shape == want.shape
        assert torch.equal(got.double().cpu(), want), (c.name, name, float((got.double().cpu() - want).abs().max()))


def _exact_pre_and_activations(c, acts, bias=True):
    """pre bit-exact and y within the project's 4e-6 through the forward entry with a saved pre-activation."""
    (x, w, b, dy), ref, ref_nb = cc.int_case(c)
    if not bias:
        b, ref = None, ref_nb
    xc, wc, bc = x.cuda(), w.cuda(), None if b is None else b.cuda()
    for act in acts:
        y, pre = _forward_pre(c, xc, wc, bc, act)
        assert torch.equal(pre.double().cpu(), ref.pre), (c.name, act)
        assert rel_err(y, cc.rm.activation(ref.pre, cc.ACT_NAMES[act])) < 4e-6, (c.name, act)


def _fp64_errors(c, act, bias=True):
    """rel_err / grad_err of pre, y and every gradient on float operands against fp64."""
    x, w, b, dy = cc.float_operands(c)
    if not bias:
        b = None
    ref = cc.reference(c, x, w, b, dy, act)
    g = [t.cuda().requires_grad_(True) if t is not None else None for t in (x, w, b)]
    y = _forward(c, g[0], g[1], g[2], act)
    (y * dy.cuda()).sum().backward()
    _, pre = _forward_pre(c, x.cuda(), w.cuda(), None if b is None else b.cuda(), act)
    errs = {"pre": rel_err(pre, ref.pre), "y": rel_err(y, ref.y), "dx": grad_err(g[0].grad, ref.dx),
            "dw": grad_err(g[1].grad, ref.dw)}
    if bias:
        errs["db"] = grad_err(g[2].grad, ref.db)
    return errs


@pytest.mark.parametrize("c", cc.GEOMETRY, ids=_ids(cc.GEOMETRY))
def test_geometry_exact(c):
    _exact_fwd_bwd(c)
    _exact_pre_and_activations(c, (1, 2, 3))


@pytest.mark.parametrize("i", range(len(cc.GEOMETRY)), ids=_ids(cc.GEOMETRY))
def test_geometry_fp64(i):
    c, act = cc.GEOMETRY[i], i % 4
    errs = _fp64_errors(c, act)
    print(c.name, act, errs)
    assert errs["pre"] < 2e-6 and errs["y"] < 4e-6, errs
    assert errs["dx"] < 1e-5 and errs["dw"] < 1e-5 and errs["db"] < 1e-5, errs


def test_forward_only_geometries_and_refusals():
    """stride 3..4 and pad >= k: the forward is exact (and meets the fp64 tolerances on float data); a backward
    that needs the input gradient is refused by qarig_conv2d_bwd_data before anything is launched, one that needs
    only the weight gradient is refused by qarig_conv_wgrad at stride 3..4 and exact where it accepts the geometry.
    An output without elements is refused by name."""
    from qarig import _lib
    for c in cc.FORWARD_ONLY:
        _exact_pre_and_activations(c, (0, 2))
        _exact_pre_and_activations(c, (0,), bias=False)
        x, w, b, dy = cc.float_operands(c)
        ref = cc.reference(c, x, w, b, dy, 1)
        y, pre = _forward_pre(c, x.cuda(), w.cuda(), b.cuda(), 1)
        assert rel_err(pre, ref.pre) < 2e-6 and rel_err(y, ref.y) < 4e-6, c.name
        # the backward
        (x, w, b, dy), ref, _ = cc.int_case(c)
        g = [t.cuda().requires_grad_(True) for t in (x, w, b)]
        loss = (_forward(c, g[0], g[1], g[2], 0) * dy.cuda()).sum()
        with pytest.raises(RuntimeError, match="conv2d_bwd_data: unsupported geometry"):
            loss.backward()
        assert g[0].grad is None and g[1].grad is None
        xg, wg = x.cuda(), w.cuda().requires_grad_(True)
        loss = (_forward(c, xg, wg, None, 0) * dy.cuda()).sum()
        if cc.wgrad_accepts(c):
            loss.backward()
            assert torch.equal(wg.grad.double().cpu(), ref.dw), c.name
        else:
            with pytest.raises(RuntimeError, match="conv_wgrad: unsupported geometry"):
                loss.backward()
            assert wg.grad is None
    lib = _lib.load()
    for N, Cin, H, W, k, s, p in cc.EMPTY_OUTPUTS:
        x = torch.zeros((N, Cin, H, W), device="cuda")
        w = torch.zeros((4, Cin, k, k), device="cuda")
        y = torch.zeros((N, 4, 8, 8), device="cuda")      # (an address, and room for what a wrong Ho == 1 would write)
        ws = torch.empty(lib.qarig_conv2d_fwd_workspace_bytes(Cin, 4, k) + 16, dtype=torch.uint8, device="cuda")
        rc = lib.qarig_conv2d_fwd_ws(x.data_ptr(), N, Cin, H, W, w.data_ptr(), None, 4, k, s, p, 0, y.data_ptr(), None,
                                     ws.data_ptr(), ws.numel(), 0, _lib.stream())
        with pytest.raises(RuntimeError, match="conv2d: empty output"):
            _lib.check(rc, "qarig_conv2d_fwd_ws")
        assert not bool(y.any())


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("path", cc.PATHS, ids=[p.case.name for p in cc.PATHS])
def test_every_conv_path_exact(path, bias):
    c = path.case
    with _options(path.opts):
        _exact_fwd_bwd(c, bias)
        _exact_pre_and_activations(c, (2, 3) if c.kind == "convt" else (1,), bias)
        if c.kind == "convt":       # the transposed layer through tanh and sigmoid, forward and backward
            for act in (2, 3):
                errs = _fp64_errors(c, act, bias)
                print(c.name, act, errs)
                assert errs["pre"] < 2e-6 and errs["y"] < 4e-6, errs
                assert all(errs[k] < 1e-5 for k in errs if k.startswith("d")), errs


# ---- alignment: the C entry points with one operand 4 or 8 bytes off a 16-byte boundary ---------------------------
def _aligned_nan(shape):
    t = torch.empty(shape, dtype=torch.float32, device="cuda")
    t.view(torch.int32).fill_(cc.NAN_PATTERN)
    return t


@pytest.mark.parametrize("a", cc.ALIGNMENT, ids=[f"{a.entry}-{a.path}-{a.operand}{a.off}" for a in cc.ALIGNMENT])
def test_offset_pointers_exact_and_guarded(a):
    from qarig import _lib
    path = cc.PATH[a.path]
    c = path.case
    (x, w, b, dy), ref, _ = cc.int_case(c)
    lib = _lib.load()
    N, Cin, H, W, Cout = c.N, c.Cin, c.H, c.W, c.Cout
    Ho, Wo = cc.out_hw(c)
    guards = []

    def inp(name, t):
        t = t.cuda()
        if name != a.operand:
            assert t.data_ptr() % 16 == 0
            return t
        v, buf, front, back = cc.offset_view(t, a.off)
        guards.extend((front, back))
        return v

    def out(name, shape):
        if name != a.operand:
            return _aligned_nan(shape)
        v, buf, front, back = cc.offset_view(torch.empty(shape, dtype=torch.float32, device="cuda"), a.off, copy=False)
        guards.extend((front, back))
        return v

    def scratch(nbytes):
        return inp("workspace", torch.zeros(max(16, nbytes) // 4 + 4)), max(16, nbytes)

    with _options(path.opts):
        sizes = cc.workspace_sizes(lib, c) if a.entry != "wgrad" else None
        st = _lib.stream()
        if a.entry == "fwd":
            ws, nb = scratch(sizes["fwd"][0])
            xs, wt, bs = inp("x", x), inp("w", w), b.cuda()
            y, pre = out("y", ref.y.shape), out("y", ref.y.shape)
            rc = lib.qarig_conv2d_fwd_ws(xs.data_ptr(), N, Cin, H, W, wt.data_ptr(), bs.data_ptr(), Cout, c.k, c.stride,
                                         c.pad, 0, y.data_ptr(), pre.data_ptr(), ws.data_ptr(), nb, 0, st)
            results = [(y, ref.y), (pre, ref.pre)]
        elif a.entry == "convt_fwd":
            ws, nb = scratch(sizes["convt_fwd"][0])
            xs, wt, bs = inp("x", x), w.cuda(), b.cuda()
            y, pre = out("y", ref.y.shape), out("y", ref.y.shape)
            rc = lib.qarig_conv_transpose2d_fwd(xs.data_ptr(), N, Cin, H, W, wt.data_ptr(), bs.data_ptr(), Cout, 0,
                                                y.data_ptr(), pre.data_ptr(), ws.data_ptr(), nb, 0, st)
            results = [(y, ref.y), (pre, ref.pre)]
        elif a.entry == "dgrad":
            ws, nb = scratch(sizes["dgrad"][0])
            dT, wt, dx = inp("dT", dy), w.cuda(), out("dx", ref.dx.shape)
            rc = lib.qarig_conv2d_bwd_data(dT.data_ptr(), N, Cout, Ho, Wo, wt.data_ptr(), Cin, c.k, c.stride, c.pad, H, W,
                                           dx.data_ptr(), ws.data_ptr(), nb, st)
            results = [(dx, ref.dx)]
        elif a.entry == "convt_dgrad":
            ws, nb = scratch(sizes["convt_dgrad"][0])
            dT, wt, dx = inp("dT", dy), w.cuda(), out("dx", ref.dx.shape)
            rc = lib.qarig_conv_transpose2d_bwd_data_ws(dT.data_ptr(), N, Cout, H, W, wt.data_ptr(), Cin, dx.data_ptr(),
                                                        ws.data_ptr(), nb, st)
            results = [(dx, ref.dx)]
        else:
            ws, nb = scratch(lib.qarig_conv_wgrad_workspace_bytes(Cout, Cin * 9, N * Ho * Wo))
            G, X, dw = inp("G", dy), inp("X", x), out("dw", ref.dw.shape)
            rc = lib.qarig_conv_wgrad(G.data_ptr(), N, Cout, Ho, Wo, X.data_ptr(), Cin, H, W, c.k, c.stride, c.pad,
                                      dw.data_ptr(), ws.data_ptr(), nb, st)
            results = [(dw, ref.dw)]
        torch.cuda.synchronize()
    assert rc == 0, _lib.last_error()
    assert len(guards) == (4 if a.operand == "y" else 2)
    for got, want in results:
        assert not bool(torch.isnan(got).any())
        assert torch.equal(got.double().cpu(), want), float((got.double().cpu() - want).abs().max())
    assert cc.guards_intact(*guards)
    for g in guards:
        assert g.dtype == torch.float32 and bool((g.view(torch.int32) == cc.NAN_PATTERN).all())


def test_conv1x1_stride2_layer_trains():
    """The shortcut of a residual downsampling block: ConvLayer(8, 16, kernel_size=1, stride=2, padding=0).  Three of
    the four parity classes of x.grad have no tap (qarig_conv2d_bwd_data, k < stride): they are written as zero."""
    from models.layers import ConvLayer
    c = cc.SHORTCUT
    torch.manual_seed(11)
    layer = ConvLayer(c.Cin, c.Cout, kernel_size=1, stride=2, padding=0)
    gen = torch.Generator().manual_seed(12)
    x = torch.randn((c.N, c.Cin, c.H, c.W), generator=gen)
    dy = torch.randn((c.N, c.Cout) + cc.out_hw(c), generator=gen)
    conv = layer.conv_layer[0]
    a = [t.detach().double().requires_grad_(True) for t in (x, conv.weight, conv.bias)]
    ya = cc.rm.activation(torch.nn.functional.conv2d(a[0], a[1], a[2], stride=2, padding=0), "silu")
    (ya * dy.double()).sum().backward()
    layer = layer.cuda()
    xg = x.cuda().requires_grad_(True)
    y = layer(xg)
    assert rel_err(y, ya) < 4e-6
    (y * dy.cuda()).sum().backward()
    conv = layer.conv_layer[0]
    for got, want in ((xg.grad, a[0].grad), (conv.weight.grad, a[1].grad), (conv.bias.grad, a[2].grad)):
        assert grad_err(got, want) < 1e-5
    assert not bool(xg.grad[:, :, 1::2, :].any()) and not bool(xg.grad[:, :, :, 1::2].any())
    assert bool(xg.grad[:, :, ::2, ::2].any())
    # integer data through the same layer shape: bit for bit, bias or not
    _exact_fwd_bwd(c)
    _exact_fwd_bwd(c, bias=False)
