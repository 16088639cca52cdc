"""Every GEMM-family kernel on sub-views of larger buffers, each argument with its own leading dimension.

The C ABI (include/qarig.h) gives every matrix argument a leading dimension of its own and qarig.ops passes
`t.stride(0)` straight through, but the rest of the suite hands the kernels contiguous tensors almost everywhere,
so a kernel that indexes the residual with ldc, the bf16 copy with ldp or the split-K reduce with N would pass it.
Here every matrix of a call is a view `parent[G:G+rows, off:off+cols]` of a parent filled with a sentinel
(`Call` below): all leading dimensions and column offsets of one call are pairwise different, input parents hold
NaN (a read outside the view poisons the result), output parents a fixed bit pattern, and after the call every
parent must still hold its sentinel outside the view, bit for bit -- "writes all of its output and nothing else".

Three kinds of comparison, none with a tolerance of its own:
 1. exact data: small-integer operands, bias and residual (as test_lp_fragment_maps_on_exact_integer_data and
    test_mx_scale_and_fragment_map_on_exact_data choose them) -- every product and partial sum is exact in fp32,
    so C, the saved pre-activation, the bf16 copies, split-K and accumulate results equal the fp64 contraction;
 2. contiguous twin: the same entry point under the same options on contiguous copies of random operands gives
    bit-identical results (only where the views keep the alignment class of contiguous tensors, so the
    dispatch cannot depend on the stride);
 3. SiLU / act' epilogues against fp64 at the bound the existing test of the same kernel uses (5e-6 as
    test_gemm_epilogues / test_lp_epilogue_bf16_copies; 4e-3 for a bf16-only output as
    test_mx_epilogue_options_on_exact_data)."""
import functools

import pytest
import torch

from conftest import rel_err

gpu = pytest.mark.gpu

F8 = torch.float8_e4m3fn
_INT = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.uint8: torch.uint8}
_ALIGN = {torch.float32: 4, torch.bfloat16: 8, torch.uint8: 16}     # elements: the 16-B class of a contiguous tensor
SENT_IN = {torch.float32: 0x7FC00000, torch.bfloat16: 0x7FC0, torch.uint8: 0xFF}    # NaN (fp32, bf16, e4m3, e8m0)
SENT_OUT = {torch.float32: 0x4B1DC0DE, torch.bfloat16: 0x4B1D, torch.uint8: 0xA5}   # finite, never a result here


class Call:
    """The matrix arguments of ONE call as views of sentinel-filled parents.

    add(name, t, kind[, align]) registers a logical (rows, cols) tensor `t` (a tensor whose values are copied
    into the view, or (rows, cols, dtype) for an output); kind "in" = NaN parent, checked unchanged as a whole
    afterwards; "out" = fixed-pattern parent, checked outside the view.  build() hands out pairwise different
    leading dimensions and column offsets (multiples of `align` elements: 4 fp32 / 8 bf16 / 16 bytes keep the
    alignment class of a contiguous tensor; `ragged` = odd offsets and odd leading dimensions, nothing 16-B
    aligned), allocates the parents and returns {name: view}.

    Guard rows: an access of R rows through the LARGEST leading dimension of the call, starting at the view,
    ends before (R ldmax) elements; every parent has enough rows below its view for that (R = the most rows of
    any argument), so exchanging two leading dimensions or row counts shows as a failed assertion, not a fault.
    `reach`: that product for a call whose arguments are spread over two Call objects."""

    def __init__(self, device, ragged=False, reach=0):
        self.device, self.ragged, self.reach, self.specs, self.items = device, ragged, reach, [], {}

    def add(self, name, t, kind, align=None):
        assert kind in ("in", "out") and name not in [s[0] for s in self.specs]
        if isinstance(t, tuple):
            rows, cols, dtype = t
            t = None
        else:
            (rows, cols), dtype = t.shape, t.dtype
        self.specs.append((name, t, rows, cols, dtype, kind, 1 if self.ragged else (align or _ALIGN[dtype])))
        return self

    def plan(self):
        """[(name, ld, off, guard rows)]: pairwise distinct ld and off."""
        used, offs, out = set(), set(), []
        for i, (name, _, rows, cols, dtype, kind, a) in enumerate(self.specs):
            off = 2 * i + 1 if self.ragged else a * (i + 1)
            while off in offs:
                off += a
            offs.add(off)
            ld = -(-(cols + off + a) // a) * a
            while ld in used or (self.ragged and ld % 2 == 0):
                ld += a
            used.add(ld)
            out.append([name, ld, off, 0])
        R = max(s[2] for s in self.specs)
        ldmax = max(p[1] for p in out)
        for p, s in zip(out, self.specs):
            p[3] = max(2, -(-max(R * ldmax, self.reach) // p[1]) - s[2] + 2)
        return [tuple(p) for p in out]

    def build(self):
        views = {}
        for (name, ld, off, G), (_, t, rows, cols, dtype, kind, _) in zip(self.plan(), self.specs):
            sent = (SENT_IN if kind == "in" else SENT_OUT)[dtype]
            parent = torch.full((rows + 2 * G, ld), sent, dtype=_INT[dtype], device=self.device).view(dtype)
            view = parent[G:G + rows, off:off + cols]
            if t is not None:
                view.copy_(t)
            self.items[name] = (parent, view, kind, sent, parent.view(_INT[dtype]).clone() if kind == "in" else None,
                                (G, rows, off, cols))
            views[name] = view
        return views

    def check(self):
        """Every parent outside its view still holds the sentinel bit for bit; input parents are unchanged."""
        for name, (parent, view, kind, sent, saved, (G, rows, off, cols)) in self.items.items():
            bits = parent.view(_INT[parent.dtype])
            if kind == "in":
                assert torch.equal(bits, saved), f"{name}: an input buffer was written"
                continue
            outside = torch.ones(bits.shape, dtype=torch.bool, device=bits.device)
            outside[G:G + rows, off:off + cols] = False
            bad = int((bits[outside] != sent).sum())
            assert bad == 0, f"{name}: {bad} element(s) outside the view were written"


def test_view_helper_self_test_on_cpu():
    """The helper itself, on CPU tensors: the check fires on one altered element outside the view (above, below,
    left and right of it, for fp32, bf16 and uint8 parents, inputs and outputs), not when only the view is
    written; leading dimensions and offsets of one call are pairwise distinct; guard rows cover the largest
    leading dimension of the call."""
    for ragged in (False, True):
        for dtype in (torch.float32, torch.bfloat16, torch.uint8):
            for kind in ("in", "out"):
                def fresh():
                    c = Call("cpu", ragged)
                    c.add("x", (5, 8, dtype), kind).add("y", torch.ones((3, 40), dtype=torch.float32), "in")
                    c.add("z", (7, 8, torch.bfloat16), "out").add("s", (5, 4, torch.uint8), "out", 4)
                    return c, c.build()
                c, v = fresh()
                plan = c.plan()
                assert len({p[1] for p in plan}) == len(plan) == len({p[2] for p in plan})
                assert all(v[p[0]].stride(0) == p[1] and v[p[0]].stride(1) == 1 for p in plan)
                if ragged:
                    assert all(p[1] % 2 == 1 and p[2] % 2 == 1 for p in plan)
                else:
                    assert all(v[n].data_ptr() % 16 == 0 for n in ("x", "y", "z")) and v["s"].data_ptr() % 4 == 0
                R, ldmax = 7, max(p[1] for p in plan)
                for name, ld, off, G in plan:
                    parent = c.items[name][0]
                    assert (G + v[name].shape[0]) * ld >= R * ldmax and parent.shape[0] == v[name].shape[0] + 2 * G
                c.check()
                if kind == "out":
                    v["x"].copy_(torch.arange(40).reshape(5, 8).to(dtype))      # the view alone: no alarm
                    v["z"].fill_(1.0)
                    c.check()
                parent, view, _, _, _, (G, rows, off, cols) = c.items["x"]
                for (r, col) in ((G - 1, off), (G + rows, off + cols - 1), (G, off - 1), (G + rows - 1, off + cols),
                                 (0, 0), (parent.shape[0] - 1, parent.shape[1] - 1)):
                    c, v = fresh()
                    p = c.items["x"][0]
                    p[r, col] = 3
                    with pytest.raises(AssertionError, match="x: "):
                        c.check()
                if kind == "in":
                    c, v = fresh()
                    v["x"][2, 3] = 3                                             # inputs: the view is guarded too
                    with pytest.raises(AssertionError, match="x: an input buffer was written"):
                        c.check()
    assert all(torch.full((1,), SENT_IN[d], dtype=_INT[d]).view(d).float().isnan().all()
               for d in (torch.float32, torch.bfloat16))
    assert torch.full((1,), 0xFF, dtype=torch.uint8).view(F8).float().isnan().all()
    assert all(torch.full((1,), SENT_OUT[d], dtype=_INT[d]).view(d).float().isfinite().all()
               for d in (torch.float32, torch.bfloat16))


@pytest.fixture
def option():
    from qarig import _lib
    saved = []

    def set_(name, value):
        saved.append((name, _lib.set_option(name, value)))

    yield set_
    for name, old in reversed(saved):
        _lib.set_option(name, old)


def _silu(t):
    return t * torch.sigmoid(t)


def _dsilu(z):
    sg = torch.sigmoid(z)
    return sg * (1 + z * (1 - sg))


def _ld(t):
    return t.stride(0) if t is not None else 0


def _ptr(t):
    return None if t is None else t.data_ptr()


# ---- fp32: qarig_gemm_f32 ----------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _ints(M, N, K):
    """Exact data for an (M, N, K) product and its fp64 contraction; never modified by the tests."""
    g = torch.Generator().manual_seed(M * 131 + N * 17 + K)
    d = dict(A=torch.randint(-4, 5, (M, K), generator=g).float(),
             B=torch.randint(-8, 9, (N, K), generator=g).float() + torch.arange(N)[:, None] % 5,
             bias=torch.randint(-3, 4, (1, N), generator=g).float(), R=torch.randint(-3, 4, (M, N), generator=g).float(),
             Z=torch.randn((M, N), generator=g), C0=torch.randint(-5, 6, (M, N), generator=g).float(),
             rs0=torch.randint(-5, 6, (1, M), generator=g).float())
    d["P"] = d["A"].double() @ d["B"].double().t()
    # every partial sum of every summation order, bias, residual and the accumulate target included, is an integer
    # below 2^24: exact in fp32
    assert float((d["A"].abs().double() @ d["B"].abs().double().t()).max()) + 3 + 3 + 5 < 2 ** 24
    assert float(d["P"].abs().max()) + 11 < 2 ** 24
    return d


@functools.lru_cache(maxsize=None)
def _rand(M, N, K):
    g = torch.Generator().manual_seed(M * 7 + N * 3 + K + 1)
    return dict(A=torch.randn((M, K), generator=g), B=torch.randn((N, K), generator=g) * 0.2,
                bias=torch.randn((1, N), generator=g), R=torch.randn((M, N), generator=g),
                Z=torch.randn((M, N), generator=g), C0=torch.randn((M, N), generator=g),
                rs0=torch.randn((1, M), generator=g))


def _gemm_f32(v, ak, bk, M, N, K, act=0, gact=0, splitk=1, accumulate=False):
    """qarig_gemm_f32 on the tensors of `v` with each one's own pointer and stride, as ops.gemm passes them."""
    from qarig import _lib
    lib = _lib.load()
    ws, nws = None, 0
    if splitk > 1 or "rs" in v:
        ws = _lib.workspace(lib.qarig_gemm_workspace_bytes(M, N, splitk), v["A"].device, "gemm")
        nws = ws.numel()
    g = v.get
    _lib.check(lib.qarig_gemm_f32(
        _ptr(v["A"]), _ld(v["A"]), int(ak), _ptr(v["B"]), _ld(v["B"]), int(bk), _ptr(v["C"]), _ld(v["C"]), M, N, K,
        _ptr(g("bias")), _ptr(g("R")), _ld(g("R")), _ptr(g("pre")), _ld(g("pre")), act, _ptr(g("Z")), _ld(g("Z")), gact,
        splitk, int(accumulate), _ptr(g("rs")), _ptr(ws), nws, _lib.stream()), "qarig_gemm_f32")


_EPI_INPUTS = {"plain": (), "split": (), "full": ("bias", "R"), "fullsplit": ("bias", "R"), "gradz": ("Z",),
               "gradzsplit": ("Z",), "acc1": (), "acc2": (), "rowsum": (), "rowsumacc": ()}


def _f32_views(d, ak, bk, M, N, epi, ragged, device="cuda"):
    c = Call(device, ragged)
    c.add("A", d["A"] if ak else d["A"].t(), "in").add("B", d["B"] if bk else d["B"].t(), "in")
    for n in _EPI_INPUTS[epi]:
        c.add(n, d[n], "in")
    c.add("C", d["C0"] if epi in ("acc1", "acc2", "rowsumacc") else (M, N, torch.float32), "out")
    if epi in ("full", "fullsplit"):
        c.add("pre", (M, N, torch.float32), "out")
    if epi in ("rowsum", "rowsumacc"):
        c.add("rs", d["rs0"] if epi == "rowsumacc" else (1, M, torch.float32), "out")
    return c, c.build()


def _f32_args(epi):
    return dict(act=1 if epi in ("full", "fullsplit") else 0, gact=1 if epi in ("gradz", "gradzsplit") else 0,
                splitk=2 if epi in ("split", "fullsplit", "gradzsplit", "acc2", "rowsumacc") else 1,
                accumulate=epi in ("acc1", "acc2", "rowsumacc"))


# kernel -> (options, (M, N, K), K of the split-K cases, ragged)
F32_KERNELS = {
    "ring": ({"gemm_tile64": 0, "gemm_pair": 0}, (256, 128, 64), 64, False),
    "pair": ({"gemm_pair": 1}, (256, 128, 64), 128, False),     # two-team kernel: >= 4 k-tiles per split, an even count
    "tile64": ({}, (128, 192, 64), 64, False),
    "ragged": ({}, (257, 130, 70), 70, True),
    "x3half": ({"gemm_x3": 1}, (256, 512, 64), 64, False),
    "x3half512": ({"gemm_x3": 1}, (512, 1024, 64), 64, False),
    "x3full": ({"gemm_x3": 2}, (512, 1024, 64), 64, False),
}
LAYOUTS = [(True, True), (True, False), (False, False)]
EPIS = ["plain", "full", "gradz", "acc1", "acc2", "split", "fullsplit", "gradzsplit", "rowsum", "rowsumacc"]


def _assert_route(lib, kernel, M, N, K, splitk):
    """The exported predicates (and, where none is exported, the dispatch arithmetic of csrc/gemm.hip gemm_dispatch)
    say that this (shape, split) under the options just set takes the kernel the case is named after."""
    t128 = -(-M // 128) * -(-N // 128)
    half = t128 * splitk < 192 and (M // 64) * (N // 64) * splitk >= 32 and M % 64 == 0 and N % 64 == 0 and K % 32 == 0
    if kernel == "ring":
        assert lib.qarig_gemm_tile64(M, N, K) == 0 and M % 128 == 0 and N % 128 == 0 and (K // splitk) % 16 == 0
    elif kernel == "pair":
        nk = K // splitk // 16
        assert M % 128 == 0 and N % 128 == 0 and nk % 2 == 0 and nk >= 4
    elif kernel == "tile64":
        assert lib.qarig_gemm_tile64(M, N, K) == 1 and (K // splitk) % 16 == 0
    elif kernel == "ragged":
        assert M % 64 and N % 64 and K % 16 and lib.qarig_gemm_tile64(M, N, K) == 0
    elif kernel in ("x3half", "x3half512"):
        assert half
    else:
        assert lib.qarig_gemm_x3_ok(M, N, K, splitk) == 1 and t128 >= 32 and (K // splitk) % 32 == 0


# (a_rowsum rides on the (xc, xc) weight-gradient layout only)
F32_CASES = [(k, ak, bk, e) for k in F32_KERNELS for ak, bk in LAYOUTS for e in EPIS
             if not e.startswith("rowsum") or not (ak or bk)]


@gpu
@pytest.mark.parametrize("kernel,ak,bk,epi", F32_CASES)
def test_gemm_f32_on_views(option, kernel, ak, bk, epi):
    """qarig_gemm_f32 through the C ABI, every matrix a view with its own leading dimension.  Kernels reached
    (csrc/gemm.hip gemm_dispatch; _assert_route states why):
      ring       gemm_dma_pf_kernel            gemm_tile64 = 0, gemm_pair = 0, 256 x 128 x 64
      pair       gemm_dma_pf2_kernel           gemm_pair = 1, 256 x 128 x 64 (x 128 when the reduction is split)
      tile64     gemm64_kernel                 default routing, 128 x 192 x 64
      ragged     gemm_kernel<.., false>        257 x 130 x 70, odd offsets and leading dimensions
      x3half     gemm_x3 half-tile kernel      gemm_x3 = 1, 256 x 512 x 64: the smallest shape with 32 tiles of 64 x 64
      x3half512  the same                      gemm_x3 = 1 at 512 x 1024 x 64 (under 192 tiles of 128 the option's
                                               value 1 still picks the half-tile form)
      x3full     gemm_x3 128 x 128 kernel      gemm_x3 = 2 (full form only), 512 x 1024 x 64 = 32 tiles
    plus slab_reduce_kernel (split, acc2), slab_reduce_epilogue_kernel (fullsplit, gradzsplit) and
    slab_reduce_rowsum_kernel (rowsumacc) behind each of them.
    Epilogues: plain; bias + residual + saved pre-activation + SiLU (`full`); gradz / gact; accumulate with one
    and two splits; a_rowsum on the (xc, xc) layout."""
    from qarig import _lib
    opts, (M, N, K), ksplit, ragged = F32_KERNELS[kernel]
    args = _f32_args(epi)
    if args["splitk"] > 1:
        K = ksplit
    for name, value in opts.items():
        option(name, value)
    _assert_route(_lib.load(), kernel, M, N, K, args["splitk"])
    d = _ints(M, N, K)
    c, v = _f32_views(d, ak, bk, M, N, epi, ragged)
    _gemm_f32(v, ak, bk, M, N, K, **args)
    c.check()
    P = d["P"]
    C = v["C"].double().cpu()
    if epi in ("plain", "split", "rowsum"):
        assert torch.equal(C, P)
    elif epi in ("acc1", "acc2", "rowsumacc"):
        assert torch.equal(C, P + d["C0"].double())
    elif epi in ("full", "fullsplit"):
        t = P + d["bias"].double() + d["R"].double()
        assert torch.equal(v["pre"].double().cpu(), t)
        assert rel_err(C, _silu(t)) < 5e-6
    else:
        assert rel_err(C, P * _dsilu(d["Z"].double())) < 5e-6
    if "rs" in v:
        want = d["A"].double().sum(1)[None] + (d["rs0"].double() if epi == "rowsumacc" else 0)
        assert torch.equal(v["rs"].double().cpu(), want)
    if ragged:
        return
    # contiguous twin on random data: same entry point, same options, bit-identical results
    r = _rand(M, N, K)
    c, v = _f32_views(r, ak, bk, M, N, epi, False)
    twin = {n: t.contiguous() for n, t in v.items()}
    assert all(t.data_ptr() % 16 == 0 and t.stride(0) % 4 == 0 for t in v.values())
    _gemm_f32(v, ak, bk, M, N, K, **args)
    _gemm_f32(twin, ak, bk, M, N, K, **args)
    c.check()
    for n in ("C", "pre", "rs"):
        if n in v:
            assert torch.equal(v[n], twin[n]), n


@gpu
@pytest.mark.parametrize("route,epi", [("skinny", "plain"), ("skinny", "full"), ("skinny", "gradz"),
                                       ("decode", "plain"), ("decode", "full")])
def test_gemm_f32_few_rows_on_views(option, route, epi):
    """skinny: gemm_skinny_kernel (csrc/gemm.hip), M = 17, N = 130, K = 256 with decode_stream = 0.
    decode: the same call under the default decode_stream at M = 16 (qarig_decode_linear_supported), which
    qarig_gemm_f32 hands to decode_linear_kernel (csrc/decode.hip) when neither a saved pre-activation nor gradz
    is asked for; A, B, C and the residual strided.  A and B keep 16-B alignment (the route requires it); the
    epilogue tensors have odd offsets and leading dimensions."""
    from qarig import _lib
    lib = _lib.load()
    M, N, K = (17 if route == "skinny" else 16), 130, 256
    if route == "skinny":
        option("decode_stream", 0)
        assert lib.qarig_decode_linear_supported(M, N, K, 0) == 0
    else:
        assert lib.qarig_decode_linear_supported(M, N, K, 0) == 1
    d = _ints(M, N, K)
    c = Call("cuda").add("A", d["A"], "in").add("B", d["B"], "in")
    e = Call("cuda", ragged=True, reach=N * max(p[1] for p in c.plan()))
    if epi == "full":
        e.add("bias", d["bias"], "in").add("R", d["R"], "in")
        if route == "skinny":
            e.add("pre", (M, N, torch.float32), "out")
    if epi == "gradz":
        e.add("Z", d["Z"], "in")
    e.add("C", (M, N, torch.float32), "out")
    v = {**c.build(), **e.build()}
    assert len({t.stride(0) for t in v.values()}) == len(v)
    _gemm_f32(v, True, True, M, N, K, act=int(epi == "full"), gact=int(epi == "gradz"))
    c.check()
    e.check()
    C, P = v["C"].double().cpu(), d["P"]
    if epi == "plain":
        assert torch.equal(C, P)
    elif epi == "full":
        t = P + d["bias"].double() + d["R"].double()
        if "pre" in v:
            assert torch.equal(v["pre"].double().cpu(), t)
        assert rel_err(C, _silu(t)) < 5e-6
    else:
        assert rel_err(C, P * _dsilu(d["Z"].double())) < 5e-6


@gpu
@pytest.mark.parametrize("epi", ["plain", "full", "gradz", "acc", "split", "fullsplit", "sum", "sumacc"])
@pytest.mark.parametrize("ak,bk", LAYOUTS)
def test_gemm_grouped_on_packed_views(ak, bk, epi):
    """gemm_dma_pf_grouped_kernel and slab_reduce_grouped_kernel (csrc/gemm.hip) through ops.gemm_grouped, G = 3
    products of 128 x 128 x 64: the groups are column blocks of ONE packed parent for A, B, C, the residual, the
    saved pre-activation and gradz (the layout of packed q / k / v), so each row stride is three blocks plus the
    parent's padding.  acc carries a_rowsum on the (xc, xc) layout."""
    from qarig import ops
    G, M, N, K = 3, 128, 128, 64
    splitk = 2 if epi in ("split", "fullsplit") else 1
    assert ops.gemm_grouped_supported(M, N, K, splitk, any_precision=True)
    ds = [_ints(M, N + 128 * i, K) for i in range(G)]       # three different data sets, cut to N columns
    ds = [dict(A=d["A"], B=d["B"][:N], bias=d["bias"][:, :N], R=d["R"][:, :N], Z=d["Z"][:, :N], C0=d["C0"][:, :N],
               rs0=d["rs0"]) for d in ds]
    Ps = [d["A"].double() @ d["B"].double().t() for d in ds]
    cat = lambda n, tr=False: torch.cat([d[n].t() if tr else d[n] for d in ds], 1)   # noqa: E731
    c = Call("cuda").add("A", cat("A", not ak), "in").add("B", cat("B", not bk), "in")
    full, summed = epi in ("full", "fullsplit"), epi in ("sum", "sumacc")
    if full:
        c.add("bias", cat("bias"), "in").add("R", cat("R"), "in").add("pre", (M, G * N, torch.float32), "out")
    if epi == "gradz":
        c.add("Z", cat("Z"), "in")
    if summed:
        c.add("C", ds[0]["C0"] if epi == "sumacc" else (M, N, torch.float32), "out")
    else:
        c.add("C", cat("C0") if epi == "acc" else (M, G * N, torch.float32), "out")
    rowsum = epi == "acc" and not ak
    if rowsum:
        c.add("rs", cat("rs0"), "out")
    v = c.build()
    blocks = lambda n, w: list(v[n].split(w, 1)) if n in v else None                 # noqa: E731
    bias = [b[0] for b in blocks("bias", N)] if full else None
    rs = [r[0] for r in blocks("rs", M)] if rowsum else None
    ops.gemm_grouped(blocks("A", K if ak else M), blocks("B", K if bk else N), blocks("C", N), M, N, K, ak, bk,
                     bias=bias, residual=blocks("R", N), preact=blocks("pre", N), act=int(full),
                     gradz=blocks("Z", N), gact=int(epi == "gradz"), splitk=splitk,
                     accumulate=epi in ("acc", "sumacc"), sum_groups=summed, a_rowsum=rs)
    c.check()
    C = v["C"].double().cpu()
    if summed:
        assert torch.equal(C, sum(Ps) + (ds[0]["C0"].double() if epi == "sumacc" else 0))
        return
    for i, (d, P) in enumerate(zip(ds, Ps)):
        Ci = C[:, i * N:(i + 1) * N]
        if epi in ("plain", "split"):
            assert torch.equal(Ci, P), i
        elif epi == "acc":
            assert torch.equal(Ci, P + d["C0"].double()), i
            if rowsum:
                assert torch.equal(v["rs"][0, i * M:(i + 1) * M].double().cpu(), d["A"].double().sum(1) + d["rs0"][0].double())
        elif full:
            t = P + d["bias"].double() + d["R"].double()
            assert torch.equal(v["pre"][:, i * N:(i + 1) * N].double().cpu(), t), i
            assert rel_err(Ci, _silu(t)) < 5e-6
        else:
            assert rel_err(Ci, P * _dsilu(d["Z"].double())) < 5e-6


# ---- bf16 / e4m3 / MX-e4m3: qarig_gemm_lp, qarig_gemm_f8, qarig_gemm_mx -----------------------------------

def _lp_operands(d, layout, dtype=torch.bfloat16):
    A = d["A"] if layout != 1 else d["A"].t()
    B = d["B"] if layout == 0 else d["B"].t()
    return A.to(dtype), B.to(dtype)


def _lp_outputs(c, M, N, fp32=("C", "pre"), bf16=("Cb", "Pb")):
    for n in fp32:
        c.add(n, (M, N, torch.float32), "out")
    for n in bf16:
        c.add(n, (M, N, torch.bfloat16), "out")
    return c


@gpu
@pytest.mark.parametrize("layout", [0, 1, 2])
@pytest.mark.parametrize("big", [0, 1])
@pytest.mark.parametrize("mfma16", [0, 1])
def test_gemm_lp_on_views(option, mfma16, big, layout):
    """The six lp_ring instantiations of csrc/gemm_lp.hip in their three layouts: gemm_lp_kernel / gemm_lp16_kernel
    (lp_big = 0, 128 x 256 x 128) and gemm_lp_big_kernel / gemm_lp_big16_kernel (lp_big = 1, 256 x 512 x 128, whole
    256-tiles), chosen by options lp_mfma16 and lp_big.  One call passes bias, residual, saved pre-activation, its
    bf16 copy Pb, a bf16 gradz, C and its bf16 copy Cb, all at different leading dimensions; then SiLU on the
    output, split-K = 2 and accumulate (qarig_slab_reduce_f32 with ldc) into a strided C."""
    from qarig import _lib, ops
    option("lp_mfma16", mfma16)
    option("lp_big", big)
    M, N, K = (256, 512, 128) if big else (128, 256, 128)
    assert _lib.load().qarig_gemm_lp_supported(M, N, K, 2) == 1 and (not big or (M % 256 == 0 and N % 256 == 0))
    d = _ints(M, N, K)
    Ab, Bb = _lp_operands(d, layout)
    P = d["P"]
    t = P + d["bias"].double() + d["R"].double()

    def everything(data, device="cuda"):
        A, B = _lp_operands(data, layout)
        c = Call(device).add("A", A, "in").add("B", B, "in").add("bias", data["bias"], "in").add("R", data["R"], "in")
        c.add("Z", data["Z"].bfloat16(), "in")
        return _lp_outputs(c, M, N)

    def run_everything(v):
        ops.gemm_lp(v["A"], v["B"], layout, M, N, K, C=v["C"], bias=v["bias"][0], residual=v["R"], preact=v["pre"],
                    gradz=v["Z"], gact=1, Cb=v["Cb"], Pb=v["Pb"])

    c = everything(d)
    v = c.build()
    assert len({x.stride(0) for x in v.values()}) == len(v) and v["A"].stride(0) % 8 == 0 and v["B"].stride(0) % 8 == 0
    run_everything(v)
    c.check()
    assert torch.equal(v["pre"].double().cpu(), t) and torch.equal(v["Pb"].cpu(), t.bfloat16())
    assert rel_err(v["C"], t * _dsilu(d["Z"].bfloat16().double())) < 5e-6
    assert torch.equal(v["Cb"], v["C"].bfloat16())
    # the same call on random data: bit-identical to its contiguous twin
    c = everything(_rand(M, N, K))
    v = c.build()
    twin = {n: x.contiguous() for n, x in v.items()}
    run_everything(v)
    run_everything(twin)
    c.check()
    for n in ("C", "pre", "Cb", "Pb"):
        assert torch.equal(v[n], twin[n]), n
    # SiLU on the output, fp32 and bf16 copies
    c = _lp_outputs(Call("cuda").add("A", Ab, "in").add("B", Bb, "in").add("bias", d["bias"], "in").add("R", d["R"], "in"),
                    M, N, fp32=("C",), bf16=("Cb",))
    v = c.build()
    ops.gemm_lp(v["A"], v["B"], layout, M, N, K, C=v["C"], bias=v["bias"][0], residual=v["R"], act=1, Cb=v["Cb"])
    c.check()
    assert rel_err(v["C"], _silu(t)) < 5e-6 and torch.equal(v["Cb"], v["C"].bfloat16())
    # plain with both outputs, split-K = 2, accumulate with one and two splits
    for splitk, acc in ((1, False), (2, False), (1, True), (2, True)):
        c = Call("cuda").add("A", Ab, "in").add("B", Bb, "in").add("C", d["C0"] if acc else (M, N, torch.float32), "out")
        if splitk == 1 and not acc:
            c.add("Cb", (M, N, torch.bfloat16), "out")
        v = c.build()
        ops.gemm_lp(v["A"], v["B"], layout, M, N, K, C=v["C"], splitk=splitk, accumulate=acc, Cb=v.get("Cb"))
        c.check()
        assert torch.equal(v["C"].double().cpu(), P + (d["C0"].double() if acc else 0)), (splitk, acc)
        if "Cb" in v:
            assert torch.equal(v["Cb"].cpu(), P.bfloat16())


@gpu
@pytest.mark.parametrize("big", [0, 1])
def test_gemm_f8_on_views(option, big):
    """gemm_f8_kernel<false> (lp_big = 0, 128 x 128 x 128) and gemm_f8_big_kernel<false> (lp_big = 1,
    256 x 256 x 128) of csrc/gemm_lp.hip: e4m3 operands in parents with ld % 16 == 0, integers exact in e4m3,
    inverse scales 1 and 1/4; the full epilogue (C, Cb, Pb, saved pre-activation, residual, bias), then SiLU."""
    from qarig import _lib, ops
    option("lp_big", big)
    M, N, K = (256, 256, 128) if big else (128, 128, 128)
    assert _lib.load().qarig_gemm_f8_supported(M, N, K) == 1
    d = _ints(M, N, K)
    A8, B8 = d["A"].to(F8).view(torch.uint8), d["B"].to(F8).view(torch.uint8)
    assert torch.equal(A8.view(F8).float(), d["A"]) and torch.equal(B8.view(F8).float(), d["B"])
    inv_a, inv_b = torch.ones(1, device="cuda"), torch.full((1,), 0.25, device="cuda")
    t = 0.25 * d["P"] + d["bias"].double() + d["R"].double()
    for act in (0, 1):
        c = Call("cuda").add("A", A8, "in").add("B", B8, "in").add("bias", d["bias"], "in").add("R", d["R"], "in")
        v = _lp_outputs(c, M, N).build()
        assert len({x.stride(0) for x in v.values()}) == len(v) and v["A"].stride(0) % 16 == 0 and v["B"].stride(0) % 16 == 0
        ops.gemm_f8(v["A"], inv_a, v["B"], inv_b, M, N, K, C=v["C"], bias=v["bias"][0], residual=v["R"],
                    preact=v["pre"], act=act, Cb=v["Cb"], Pb=v["Pb"])
        c.check()
        assert torch.equal(v["pre"].double().cpu(), t) and torch.equal(v["Pb"].cpu(), t.bfloat16())
        if act == 0:
            assert torch.equal(v["C"].double().cpu(), t) and torch.equal(v["Cb"].cpu(), t.bfloat16())
        else:
            assert rel_err(v["C"], _silu(t)) < 5e-6 and torch.equal(v["Cb"], v["C"].bfloat16())


@functools.lru_cache(maxsize=None)
def _mx_ints(rows, K, seed):
    """An exact MX operand as test_gpu_mxfp8._scaled_ints makes it: integers in [-4, 4] (exact in e4m3) with a
    random scale byte in 125..129 per row and 32-block; (bytes, scale bytes, fp64 values)."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randint(-4, 5, (rows, K), generator=g).float()
    s = torch.randint(125, 130, (rows, K // 32), generator=g).to(torch.uint8)
    val = (q.double().reshape(rows, -1, 32) * torch.pow(2.0, s.double() - 127.0)[..., None]).reshape(rows, K)
    return q.to(F8).view(torch.uint8), s, val


@gpu
@pytest.mark.parametrize("big", [0, 1])
def test_gemm_mx_on_views(option, big):
    """gemm_f8_kernel<true, MxScales> (lp_big = 0, 128 x 128) and gemm_f8_big_kernel<true, MxScales> (lp_big = 1,
    256 x 256) of csrc/gemm_lp.hip: element bytes AND scale bytes come from parents, lda != ldb (% 16, >= K),
    ldsa != ldsb (% 4, >= K / 32), random per-block scale bytes.  Products of integers in [-4, 4] times 2^(-4..4)
    over K <= 256 stay exact (test_mx_scale_and_fragment_map_on_exact_data).  Full epilogue, act' fused into a
    bf16-only output (4e-3, as test_mx_epilogue_options_on_exact_data), split-K = 2 at K = 256 and accumulate."""
    from qarig import _lib, ops
    option("lp_big", big)
    M = N = 256 if big else 128
    lib = _lib.load()
    d = _ints(M, N, 128)                                    # bias, residual, gradz, accumulate target
    for K, calls in ((128, ("full", "silu", "gradz", "gradzb", "acc")), (256, ("split", "accsplit"))):
        Aq, As, Av = _mx_ints(M, K, 1)
        Bq, Bs, Bv = _mx_ints(N, K, 2)
        P = Av @ Bv.t()
        t = P + d["bias"].double() + d["R"].double()
        for what in calls:
            splitk = 2 if what in ("split", "accsplit") else 1
            assert lib.qarig_gemm_mx_supported(M, N, K, splitk) == 1
            c = Call("cuda").add("A", Aq, "in").add("sA", As, "in", 4).add("B", Bq, "in").add("sB", Bs, "in", 4)
            kw = {}
            if what in ("full", "silu"):
                _lp_outputs(c.add("bias", d["bias"], "in").add("R", d["R"], "in"), M, N)
            elif what in ("gradz", "gradzb"):
                c.add("Z", d["Z"] if what == "gradz" else d["Z"].bfloat16(), "in").add("Cb", (M, N, torch.bfloat16), "out")
            else:
                c.add("C", d["C0"] if what.startswith("acc") else (M, N, torch.float32), "out")
            v = c.build()
            lds = [x.stride(0) for x in v.values()]
            assert len(set(lds)) == len(lds) and v["A"].stride(0) % 16 == 0 and v["B"].stride(0) % 16 == 0
            assert v["sA"].stride(0) % 4 == 0 and v["sB"].stride(0) % 4 == 0 and v["sA"].stride(0) >= K // 32
            if "bias" in v:
                kw = dict(bias=v["bias"][0], residual=v["R"], preact=v["pre"], Pb=v["Pb"], act=int(what == "silu"))
            if "Z" in v:
                kw = dict(gradz=v["Z"], gact=1)
            ops.gemm_mx(ops.MxOperand(v["A"], v["sA"]), ops.MxOperand(v["B"], v["sB"]), M, N, K, C=v.get("C"),
                        Cb=v.get("Cb"), splitk=splitk, accumulate=what.startswith("acc"), **kw)
            c.check()
            if what in ("full", "silu"):
                assert torch.equal(v["pre"].double().cpu(), t) and torch.equal(v["Pb"].cpu(), t.bfloat16())
                if what == "full":
                    assert torch.equal(v["C"].double().cpu(), t) and torch.equal(v["Cb"].cpu(), t.bfloat16())
                else:
                    assert rel_err(v["C"], _silu(t)) < 5e-6 and torch.equal(v["Cb"], v["C"].bfloat16())
            elif "Z" in v:
                assert rel_err(v["Cb"].float(), P * _dsilu(v["Z"].double().cpu())) < 4e-3
            else:
                assert torch.equal(v["C"].double().cpu(), P + (d["C0"].double() if what.startswith("acc") else 0)), what


# ---- casts and reductions with a strided source ---------------------------------------------------------------

@gpu
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_cast_colsum_strided_source(dtype, accumulate):
    """cast_colsum_kernel / colsum_bf16_kernel + colsum_reduce_kernel (csrc/gemm_lp.hip) through ops.cast_colsum:
    a source with a row stride of its own gives the bf16 copy and the column sums of its contiguous twin, bit
    for bit (200 x 264: ragged 16-row groups, a partial 512-column block)."""
    from qarig import ops
    g = torch.Generator().manual_seed(5)
    x = torch.randn((200, 264), generator=g).to(dtype)
    cs0 = torch.randn(264, generator=g).cuda()
    c = Call("cuda").add("pad", (1, 4, dtype), "out").add("x", x, "in")
    v = c.build()
    assert v["x"].stride(0) > 264 and not v["x"].is_contiguous()
    outs = []
    for src in (v["x"], v["x"].contiguous()):
        cs = cs0.clone()
        outs.append((ops.cast_colsum(src, cs, accumulate=accumulate, want_cast=dtype == torch.float32), cs))
    c.check()
    assert torch.equal(outs[0][1], outs[1][1])
    assert rel_err(outs[0][1], x.double().sum(0) + (cs0.double().cpu() if accumulate else 0)) < 2e-6
    if dtype == torch.float32:
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][0].cpu(), x.bfloat16())


@gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_mx_quant_strided_source(dtype):
    """mx_quant_kernel (csrc/gemm_lp.hip) through ops.mx_quant: row form, transposed form and column sums of a
    strided (200, 256) source equal those of its contiguous twin bit for bit."""
    from qarig import ops
    g = torch.Generator().manual_seed(6)
    x = (torch.randn((200, 256), generator=g) * torch.logspace(-3, 3, 200)[:, None]).to(dtype)
    c = Call("cuda").add("pad", (1, 4, dtype), "out").add("x", x, "in")
    v = c.build()
    assert v["x"].stride(0) > 256
    outs = []
    for src in (v["x"], v["x"].contiguous()):
        cs = torch.full((256,), 5.0, device="cuda")
        rf, tf = ops.mx_quant(src, row=True, transposed=True, colsum=cs)
        outs.append((rf.q, rf.s, tf.q, tf.s, cs))
    c.check()
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert rel_err(outs[0][4], x.double().sum(0)) < 1e-6          # (the colsum did run: not the 5.0 it held)


@gpu
def test_colsum_strided_source():
    """colsum_partial_kernel + slab_reduce_kernel (csrc/gemm.hip) through ops.colsum on a (301, 130) source with an
    odd offset and an odd row stride: the sums of the contiguous twin, bit for bit, with and without accumulate."""
    from qarig import ops
    g = torch.Generator().manual_seed(7)
    x = torch.randn((301, 130), generator=g)
    c = Call("cuda", ragged=True).add("x", x, "in")
    v = c.build()
    assert v["x"].stride(0) % 2 == 1
    a, b = ops.colsum(v["x"]), ops.colsum(v["x"].contiguous())
    assert torch.equal(a, b) and rel_err(a, x.double().sum(0)) < 2e-6
    o = Call("cuda").add("out", torch.ones((1, 130)), "out")
    ov = o.build()
    ops.colsum(v["x"], out=ov["out"][0], accumulate=True)
    c.check()
    o.check()
    assert torch.equal(ov["out"][0], ops.colsum(v["x"].contiguous(), out=torch.ones(130, device="cuda"), accumulate=True))


# ---- refusals ----------------------------------------------------------------------------------------------------

def _overlapping(rows, cols, ld, dtype, fill):
    """A (rows, cols) view whose row stride `ld` is SHORTER than its row (rows overlap), inside one buffer."""
    base = torch.full((rows * cols + 64,), fill, dtype=_INT[dtype], device="cuda").view(dtype)
    return base.as_strided((rows, cols), (ld, 1))


@gpu
def test_misaligned_views_are_refused_and_nothing_is_written():
    """One call per constraint include/qarig.h states for qarig_gemm_lp / _f8 / _mx and qarig_gemm_f32_grouped
    (operand leading dimensions: % 8 elements for bf16, % 16 bytes and >= K for e4m3; scale rows % 4 bytes and
    >= K / 32; fp32 epilogue tensors 16-B aligned; bf16 outputs 8-B aligned; grouped row strides % 4): each returns
    QARIG_ERR_ARG, which check() raises with the message of the constraint, and leaves every output parent at
    its sentinel."""
    from qarig import ops
    M = N = K = 128
    d = _ints(M, N, K)
    Ab, Bb = d["A"].bfloat16(), d["B"].bfloat16()
    A8, B8 = d["A"].to(F8).view(torch.uint8), d["B"].to(F8).view(torch.uint8)
    one = torch.ones(1, device="cuda")

    def padded(t, pad):
        """t as the first columns of a NaN-filled parent `pad` elements wider: aligned start, row stride + pad."""
        parent = torch.full((t.shape[0], t.shape[1] + pad), SENT_IN[t.dtype], dtype=_INT[t.dtype], device="cuda")
        view = parent.view(t.dtype)[:, :t.shape[1]]
        view.copy_(t)
        return view

    def views(A, B, extra=()):
        c = Call("cuda").add("A", A, "in").add("B", B, "in")
        for n, dtype, align in (("C", torch.float32, None), ("Cb", torch.bfloat16, None), *extra):
            c.add(n, (M, N, dtype), "out", align)
        return c, c.build()

    def refused(c, match, fn):
        with pytest.raises(RuntimeError, match=match):
            fn()
        torch.cuda.synchronize()
        c.check()
        for name, (parent, view, kind, sent, _, _) in c.items.items():      # ... the views included
            assert kind == "in" or bool((parent.view(_INT[parent.dtype]) == sent).all()), name

    # bf16 operand rows at 4 elements (8 bytes): lda % 8
    c, v = views(Ab, Bb)
    a4 = padded(Ab, 4)
    assert a4.stride(0) % 8 == 4 and a4.data_ptr() % 16 == 0
    refused(c, "gemm_lp: operands 16-B aligned, ld % 8", lambda: ops.gemm_lp(a4, v["B"], 0, M, N, K, C=v["C"]))
    refused(c, "gemm_lp: operands 16-B aligned, ld % 8", lambda: ops.gemm_lp(v["A"], a4, 0, M, N, K, C=v["C"]))
    # fp32 output at an 8-byte offset; bf16 output at a 4-byte offset; fp32 leading dimension % 4
    c, v = views(Ab, Bb, extra=(("C8", torch.float32, 2),))
    assert v["C8"].data_ptr() % 16 == 8
    refused(c, "fp32 epilogue tensors 16-B aligned", lambda: ops.gemm_lp(v["A"], v["B"], 0, M, N, K, C=v["C8"]))
    refused(c, "fp32 epilogue tensors 16-B aligned",
            lambda: ops.gemm_lp(v["A"], v["B"], 0, M, N, K, C=v["C"], preact=v["C8"]))
    c, v = views(Ab, Bb, extra=(("Cb4", torch.bfloat16, 2),))
    assert v["Cb4"].data_ptr() % 8 == 4
    refused(c, "bf16 outputs 8-B aligned", lambda: ops.gemm_lp(v["A"], v["B"], 0, M, N, K, C=v["C"], Cb=v["Cb4"]))
    refused(c, "bf16 outputs 8-B aligned", lambda: ops.gemm_lp(v["A"], v["B"], 0, M, N, K, C=v["C"], Pb=v["Cb4"]))
    # e4m3 operand rows at 8 bytes: ld % 16 (per-tensor scales and MX)
    c, v = views(A8, B8)
    a8 = padded(A8, 8)
    assert a8.stride(0) % 16 == 8 and a8.data_ptr() % 16 == 0
    refused(c, "gemm_f8: operands 16-B aligned, ld % 16",
            lambda: ops.gemm_f8(a8, one, v["B"], one, M, N, K, C=v["C"]))
    sA = torch.full((M, K // 32), 127, dtype=torch.uint8, device="cuda")
    mx = lambda q, s: ops.MxOperand(q, s)                                                   # noqa: E731
    refused(c, "gemm_mx: operands 16-B aligned, ld % 16",
            lambda: ops.gemm_mx(mx(v["A"], sA), mx(a8, sA), M, N, K, C=v["C"]))
    # MX: an operand row stride shorter than K; scale rows at ld % 4 != 0 and shorter than K / 32
    short = _overlapping(M, K, K - 16, torch.uint8, 0)
    refused(c, "gemm_mx: operands 16-B aligned, ld % 16",
            lambda: ops.gemm_mx(mx(short, sA), mx(v["B"], sA), M, N, K, C=v["C"]))
    s6 = torch.full((M, 6), 127, dtype=torch.uint8, device="cuda")[:, :4]
    refused(c, "gemm_mx: scales 4-B aligned, ld % 4",
            lambda: ops.gemm_mx(mx(v["A"], s6), mx(v["B"], sA), M, N, K, C=v["C"]))
    s0 = _overlapping(M, 4, 0, torch.uint8, 127)
    refused(c, "gemm_mx: scales 4-B aligned, ld % 4",
            lambda: ops.gemm_mx(mx(v["A"], sA), mx(v["B"], s0), M, N, K, C=v["C"]))
    # grouped launch: a residual whose row stride is not a multiple of 4 elements
    c = Call("cuda").add("A", d["A"], "in").add("B", d["B"], "in").add("C", (M, N, torch.float32), "out")
    v = c.build()
    r = padded(d["R"], 6)
    assert r.stride(0) % 4 and r.data_ptr() % 16 == 0
    refused(c, "gemm_grouped: row strides must be multiples of 4",
            lambda: ops.gemm_grouped([v["A"]], [v["B"]], [v["C"]], M, N, K, residual=[r]))
