"""Cases, operands, fp64 references and offset views shared by tests/test_gpu_conv_geometry.py (the conv entry points
of csrc/conv.hip on an MI355X) and tests/test_conv_cases_host.py (the same pieces on the CPU).

WHAT IS UNDER TEST.  qarig_conv2d_fwd[_ws], qarig_conv_transpose2d_fwd, qarig_conv2d_bwd_data,
qarig_conv_transpose2d_bwd_data_ws and qarig_conv_wgrad pick among six ring kinds, two gather loaders (each FAST and
guarded), two direct kernels, three weight-gradient kernels and a split reduction from the kernel size, stride,
padding, channel counts, row width and POINTER ALIGNMENT.  tests/test_gpu_conv.py runs the shapes of the README
autoencoder: 3x3 with padding 1 (and the 4/2/1 transpose), with a bias, on tensors as the allocator hands them out.
The tables below hold what the entry points accept beyond that.

THE EXACT ARM.  The conv kernels multiply in fp32 (v_mfma_f32_32x32x2f32, fmaf).  With small-integer operands
(`int_operands`) every product and every partial sum of every output is an integer below 2^24 (`exact_bound`, proved
per case by the host test), so the result is the same whatever the summation order, tile shape, split count or
kernel family, and the GPU test asks for torch.equal with the fp64 reference on every element of y, preact, dx, dw
and db.  A quarter of the weights are zero, so a tap that is read from the wrong place changes the answer.

Each row of a table says which host condition of conv.hip it is there for."""
import collections
import functools

import torch

from oracle import ref_models as rm

F = torch.nn.functional
ACT_NAMES = {0: None, 1: "silu", 2: "tanh", 3: "sigmoid"}

# kind "conv": nn.Conv2d(Cin, Cout, k, stride, pad) on (N, Cin, H, W); "convt": nn.ConvTranspose2d(Cin, Cout, 4, 2, 1)
Case = collections.namedtuple("Case", "name kind N Cin H W Cout k stride pad why")
Ref = collections.namedtuple("Ref", "pre y dx dw db")


def conv(name, N, Cin, H, W, Cout, k, stride, pad, why):
    return Case(name, "conv", N, Cin, H, W, Cout, k, stride, pad, why)


def convt(name, N, Cin, H, W, Cout, why):
    return Case(name, "convt", N, Cin, H, W, Cout, 4, 2, 1, why)


def out_hw(c):
    if c.kind == "convt":
        return 2 * c.H, 2 * c.W
    return (c.H + 2 * c.pad - c.k) // c.stride + 1, (c.W + 2 * c.pad - c.k) // c.stride + 1


def weight_shape(c):
    return (c.Cin, c.Cout, 4, 4) if c.kind == "convt" else (c.Cout, c.Cin, c.k, c.k)


# ---- operands ---------------------------------------------------------------------------------------------------
def _gen(c, seed):
    return torch.Generator().manual_seed(seed * 1000003 + c.N * 7919 + c.Cin * 131 + c.Cout * 17 + c.H * 5 + c.W
                                         + c.k * 977 + c.stride * 389 + c.pad * 61)


def int_operands(c, seed=0):
    """x, w, b, dy as fp32 tensors of integers: x, dy in [-4, 4], w in [-3, 3], b in [-8, 8]; the weight elements
    whose flat index i has (i + i // 4 + i // 16) % 4 == 0 -- one of every four consecutive elements, at a position
    that moves from group to group -- are zero."""
    g = _gen(c, seed)
    Ho, Wo = out_hw(c)
    x = torch.randint(-4, 5, (c.N, c.Cin, c.H, c.W), generator=g).float()
    w = torch.randint(-3, 4, weight_shape(c), generator=g).float()
    i = torch.arange(w.numel())
    w.view(-1)[(i + i // 4 + i // 16) % 4 == 0] = 0.0
    b = torch.randint(-8, 9, (c.Cout,), generator=g).float()
    dy = torch.randint(-4, 5, (c.N, c.Cout, Ho, Wo), generator=g).float()
    return x, w, b, dy


def float_operands(c, seed=0):
    """The scaling of tests/test_gpu_conv.py: x, b, dy standard normal, w = randn / (k sqrt(Cin))."""
    g = _gen(c, seed + 17)
    Ho, Wo = out_hw(c)
    x = torch.randn((c.N, c.Cin, c.H, c.W), generator=g)
    w = torch.randn(weight_shape(c), generator=g) / (c.k * c.Cin ** 0.5)
    b = torch.randn(c.Cout, generator=g)
    dy = torch.randn((c.N, c.Cout, Ho, Wo), generator=g)
    return x, w, b, dy


def reference(c, x, w, b, dy, act=0):
    """fp64 on the CPU: pre-activation, output and the gradients of sum(y * dy) (db is None without a bias)."""
    a = [t.double().requires_grad_(True) if t is not None else None for t in (x, w, b)]
    if c.kind == "convt":
        pre = F.conv_transpose2d(a[0], a[1], a[2], stride=2, padding=1)
    else:
        pre = F.conv2d(a[0], a[1], a[2], stride=c.stride, padding=c.pad)
    y = rm.activation(pre, ACT_NAMES[act])
    (y * dy.double()).sum().backward()
    return Ref(pre.detach(), y.detach(), a[0].grad, a[1].grad, None if b is None else a[2].grad)


def exact_bound(c, x, w, b, dy):
    """The largest magnitude any partial sum of any output element can reach, in any summation order: the same
    sums over the operands' absolute values (pre / y, dx, dw, db)."""
    r = reference(c, x.abs(), w.abs(), None if b is None else b.abs(), dy.abs(), 0)
    return max(float(t.abs().max()) for t in r if t is not None)


@functools.lru_cache(maxsize=None)
def int_case(c, seed=0):
    """(operands, reference with the bias at act 0, reference without it) of a case, computed once and shared:
    callers must not write to them."""
    ops = int_operands(c, seed)
    return ops, reference(c, *ops, 0), reference(c, ops[0], ops[1], None, ops[3], 0)


# ---- offset views -----------------------------------------------------------------------------------------------
NAN_PATTERN = 0x7FC0BEEF          # a quiet NaN with a recognisable payload, as int32


def offset_view(t, bytes_off, guard=64, copy=True):
    """A contiguous tensor of t's shape and values (copy=False: left at the NaN pattern -- an output) that starts
    `bytes_off` (4 or 8) bytes past a 16-byte boundary inside a fresh, larger fp32 buffer on t's device, filled with
    NAN_PATTERN.  Returns (view, buffer, front, back): the `guard` floats of the buffer directly in front of and
    behind the view."""
    assert bytes_off in (4, 8) and t.dtype == torch.float32
    n = t.numel()
    buf = torch.empty(n + 2 * guard + 8, dtype=torch.float32, device=t.device)
    buf.view(torch.int32).fill_(NAN_PATTERN)
    base = buf.data_ptr()
    start = guard
    while (base + 4 * start) % 16 != bytes_off:
        start += 1
    view = buf[start:start + n].view(t.shape)
    if copy:
        view.copy_(t)
    return view, buf, buf[start - guard:start], buf[start + n:start + n + guard]


def guards_intact(*guards):
    return all(bool((g.view(torch.int32) == NAN_PATTERN).all()) for g in guards)


# ---- GEOMETRY: every (k, stride, pad) both gradients accept, in three channel / extent regimes --------------------
GEOMETRIES = tuple((k, s, p) for k in (1, 2, 3, 4) for s in (1, 2) for p in range(k))      # 20
REGIMES = ("direct", "gather", "gather-row")


def _geometry_cases():
    out = []
    for k, s, p in GEOMETRIES:
        tag = f"k{k}s{s}p{p}"
        # launch_conv `o.Cout <= 8` both ways (the input gradient's output channels are Cin): conv_direct_kernel with
        # general taps; 9 x 11 is odd, so H != 2 Ho at stride 2, and (9 - k) is odd for even k: without padding a
        # trailing input row that no output reads
        out.append(conv(f"direct-{tag}", 2, 5, 9, 11, 3, k, s, p, "launch_conv: o.Cout <= 8, not plain3x3"))
        out.append(conv(f"direct-mirror-{tag}", 2, 3, 9, 11, 5, k, s, p,
                        "launch_conv: o.Cout <= 8 for the input gradient's 3 channels"))
        # conv_mma_kernel guarded in Cout, K and P; Wo % 4 != 0 for most geometries: SrcIm2col; (10 - k) is odd for
        # odd k: the uncovered trailing row of the odd kernel sizes (pad 0), and (13 - k) the column of the even ones
        out.append(conv(f"gather-{tag}", 2, 20, 10, 13, 24, k, s, p, "launch_conv: !fast, !rowvec (SrcIm2col)"))
        # Wo == 8: rowvec (SrcIm2colRow) at stride 1, `row` in qarig_conv_wgrad (SrcGradPixRow / SrcIm2colPixRow);
        # 136 channels hang over one 128 tile; at stride 2 one more row than the windows cover (an input row at pad 0)
        H = 5 * s + k - 2 * p + (1 if s == 2 else 0)
        W = 7 * s + k - 2 * p
        out.append(conv(f"gather-row-{tag}", 1, 16, H, W, 136, k, s, p,
                        "launch_conv: rowvec; qarig_conv_wgrad: row; Cout over one 128 tile"))
    # the 1x1 / stride-2 shortcut at a channel count the ring kinds would take for 3x3: conv2d_ring_plan says no,
    # class (0, 0) runs conv_mma_kernel over whole tiles, the other three classes have no taps
    out.append(conv("ringlike-k1s2p0", 1, 128, 16, 16, 16, 1, 2, 0, "qarig_conv2d_bwd_data: k < stride, empty classes"))
    return tuple(out)


GEOMETRY = _geometry_cases()


def regime(c):
    return c.name.rsplit("-k", 1)[0].replace("direct-mirror", "direct")


def uncovered_rows(c):
    """Trailing rows of the input itself that no output window reads: what (H + 2 pad - k) % stride leaves over,
    less the padding rows among them."""
    return max(0, (c.H + 2 * c.pad - c.k) % c.stride - c.pad) if c.kind == "conv" else 0


# ---- FORWARD_ONLY: geometries only qarig_conv2d_fwd accepts (stride 3..4, pad >= k) -------------------------------
FORWARD_ONLY_GEOMETRIES = ((1, 1, 1), (1, 2, 2), (2, 1, 3), (2, 2, 2), (3, 1, 4), (3, 3, 0), (3, 4, 4), (4, 3, 2),
                           (1, 3, 0), (4, 4, 1))
FORWARD_ONLY = tuple(
    cs for k, s, p in FORWARD_ONLY_GEOMETRIES for cs in (
        conv(f"direct-k{k}s{s}p{p}", 2, 5, 9, 11, 3, k, s, p, "conv2d_fwd_impl: stride 3..4 / pad >= k, direct"),
        conv(f"gather-k{k}s{s}p{p}", 2, 20, 10, 13, 24, k, s, p, "conv2d_fwd_impl: stride 3..4 / pad >= k, gather")))


def bwd_data_accepts(c):
    return c.stride <= 2 and c.pad < c.k


def wgrad_accepts(c):
    return c.stride <= 2 and c.pad <= 4


# (N, Cin, H, W, k, stride, pad): H + 2 pad < k (at stride 2 the truncating division alone would say Ho == 1)
EMPTY_OUTPUTS = ((1, 4, 3, 8, 4, 1, 0), (1, 4, 3, 8, 4, 2, 0), (1, 4, 8, 1, 2, 2, 0), (2, 4, 1, 1, 4, 3, 1))

# ---- PATHS: one case per kernel family at its smallest whole-tile shape -------------------------------------------
# opts: options set around the calls (qarig._lib.set_option); splits: which of the scratch-size functions promise
# slabs for this shape ("fwd", "dgrad": qarig_conv2d_{fwd,bwd_data}_workspace_bytes_n; "convt_fwd", "convt_dgrad":
# qarig_conv_transpose2d_{,bwd_data_}workspace_bytes_n)
Path = collections.namedtuple("Path", "case opts splits")
RING_OFF = (("conv_ring", 0),)
FOUR_LAUNCH = (("conv_ring", 0), ("convt_pair", 0))


def _paths():
    c3 = lambda name, N, Cin, H, W, Cout, s, why: conv(name, N, Cin, H, W, Cout, 3, s, 1, why)
    return (
        Path(c3("ring_s1_fwd", 1, 16, 8, 16, 128, 1, "conv_ring_plan RING_S1_FWD: C 16, M 128, P 128"), (), ()),
        Path(c3("ring_s1_dgrad", 1, 128, 8, 16, 16, 1, "conv_ring_plan RING_S1_DGRAD: C = Cout 16, M = Cin 128"), (), ()),
        Path(c3("ring_s2_fwd", 1, 16, 16, 32, 128, 2, "conv_ring_plan RING_S2_FWD: grid 8 x 16"), (), ()),
        Path(c3("ring_s2_dgrad", 1, 128, 16, 32, 16, 2, "conv_ring_plan RING_S2_DGRAD: mode 1, classes of 1/2/2/4 taps"), (), ()),
        Path(convt("ring_convt_fwd", 1, 16, 8, 16, 128, "conv_ring_plan RING_CONVT_FWD: pair stores"), (), ()),
        Path(convt("ring_convt_dgrad", 1, 128, 8, 16, 16, "conv_ring_plan RING_CONVT_DGRAD: 16 taps, strided"), (), ()),
        # conv_ring_splits: the smallest reduction that splits has K / 16 >= 32 k-tiles (two parts of >= 16)
        Path(c3("split_s1_fwd", 1, 64, 8, 16, 128, 1, "conv_ring_splits: 36 k-tiles -> 2 parts, conv_split_reduce_kernel"),
             (), ("fwd",)),
        Path(c3("split_s1_dgrad", 1, 128, 8, 16, 64, 1, "conv_ring_splits on RING_S1_DGRAD"), (), ("dgrad",)),
        Path(c3("split_s2_fwd", 1, 64, 16, 32, 128, 2, "conv_ring_splits on RING_S2_FWD"), (), ("fwd",)),
        Path(convt("split_convt_fwd", 1, 128, 8, 16, 128, "conv_ring_splits on RING_CONVT_FWD: 32 k-tiles per class"),
             (), ("convt_fwd", "convt_dgrad")),
        Path(convt("split_convt_dgrad", 1, 128, 8, 16, 32, "conv_ring_splits on RING_CONVT_DGRAD: 32 k-tiles"),
             (), ("convt_dgrad",)),
        Path(c3("direct4_cs8", 1, 64, 8, 16, 3, 1, "launch_conv plain3x3, cs8: C % 8 == 0 && C >= 64"), (), ()),
        Path(c3("direct4_plain", 2, 12, 8, 12, 4, 1, "launch_conv plain3x3, !cs8"), (), ()),
        Path(c3("direct4_flip_cs8", 1, 3, 8, 16, 64, 1, "launch_conv flip_taps: input gradient to 3 channels"), (), ()),
        Path(c3("wgrad_direct", 2, 8, 8, 12, 3, 1, "wgrad_direct_ok: Cg 3"), (), ()),
        Path(c3("wgrad_ring", 2, 128, 16, 16, 128, 1, "qarig_conv_wgrad: conv3x3_wgrad_ring_kernel"), (),
             ("fwd", "dgrad")),
        Path(c3("wgrad_mma_fast", 2, 128, 16, 16, 128, 1, "qarig_conv_wgrad: conv_wgrad_kernel<true, true>"), RING_OFF, ()),
        Path(convt("convt_pair", 1, 16, 8, 16, 128, "qarig_conv_transpose2d_fwd: pair, rowvec, fast"), RING_OFF, ()),
        Path(convt("convt_pair_guarded", 2, 20, 5, 6, 12, "qarig_conv_transpose2d_fwd: pair, !rowvec, !fast"), RING_OFF, ()),
        Path(convt("convt_four_launch", 1, 16, 8, 16, 128, "qarig_conv_transpose2d_fwd: convt_pair = 0"), FOUR_LAUNCH, ()),
        Path(convt("convt_four_launch_guarded", 2, 20, 5, 6, 12, "one class per launch, guarded tiles"), FOUR_LAUNCH, ()),
        Path(convt("convt_direct", 2, 20, 5, 6, 3, "qarig_conv_transpose2d_fwd: Cout <= 8, conv_direct_kernel per class"),
             (), ()),
    )


PATHS = _paths()
PATH = {p.case.name: p for p in PATHS}


def workspace_sizes(h, c):
    """{which: (bytes the _n function asks for, bytes of the re-ordered weights alone)} of a case's entry points;
    h = the loaded library."""
    if c.kind == "convt":
        base = h.qarig_conv_transpose2d_workspace_bytes(c.Cin, c.Cout)
        return {"convt_fwd": (h.qarig_conv_transpose2d_workspace_bytes_n(c.N, c.Cin, c.H, c.W, c.Cout), base),
                "convt_dgrad": (h.qarig_conv_transpose2d_bwd_data_workspace_bytes_n(c.N, c.Cin, c.H, c.W, c.Cout), base)}
    return {"fwd": (h.qarig_conv2d_fwd_workspace_bytes_n(c.N, c.Cin, c.H, c.W, c.Cout, c.k, c.stride),
                    h.qarig_conv2d_fwd_workspace_bytes(c.Cin, c.Cout, c.k)),
            "dgrad": (h.qarig_conv2d_bwd_data_workspace_bytes_n(c.N, c.Cin, c.H, c.W, c.Cout, c.k, c.stride),
                      h.qarig_conv2d_bwd_data_workspace_bytes(c.Cin, c.Cout, c.k))}


# ---- ALIGNMENT: one operand of one entry point moved 4 or 8 bytes off a 16-byte boundary --------------------------
# entry: "fwd" qarig_conv2d_fwd_ws | "convt_fwd" qarig_conv_transpose2d_fwd | "dgrad" qarig_conv2d_bwd_data |
# "convt_dgrad" qarig_conv_transpose2d_bwd_data_ws | "wgrad" qarig_conv_wgrad; operand: the argument that moves
# ("y" moves y and preact together); path: the PATHS row whose shape and options the call uses
Align = collections.namedtuple("Align", "entry path operand off why")


def _alignment():
    rows = []
    add = lambda *a: rows.append(Align(*a))
    for path in ("ring_s1_fwd", "split_s1_fwd", "ring_s2_fwd"):
        add("fwd", path, "x", 4, "conv_ring_usable: (x | workspace) & 15 -> gather kernels, F4u loads")
        add("fwd", path, "y", 8, "run_conv_ring: align_split 15 -> unsplit ring launch, 4-B stores")
        add("fwd", path, "y", 4, "the same at 4 B")
        add("fwd", path, "w", 4, "conv_pack_tap_kernel reads w element-wise")
        add("fwd", path, "workspace", 4, "conv_ring_usable: workspace & 15 -> gather kernels")
    for path in ("direct4_cs8", "direct4_plain"):
        add("fwd", path, "x", 4, "plain3x3: (x | y | preact) & 15 -> conv_direct_kernel")
        add("fwd", path, "y", 8, "plain3x3: 16-B stores of conv_direct4_kernel need y & 15 == 0")
        add("fwd", path, "y", 4, "the same at 4 B")
    add("fwd", "wgrad_mma_fast", "w", 4, "launch_conv sa.vec4: weights & 15 -> element loads, !fast")
    add("fwd", "wgrad_mma_fast", "x", 4, "SrcIm2colRow: 16-B loads from 4-B aligned rows")
    for path in ("ring_convt_fwd", "split_convt_fwd"):
        add("convt_fwd", path, "x", 4, "conv_ring_usable -> convt_pair_kernel")
        add("convt_fwd", path, "y", 8, "align 7 holds (pair stores), align_split 15 does not")
        add("convt_fwd", path, "y", 4, "align 7: ring and pair both refuse -> four launches")
        add("convt_fwd", path, "workspace", 4, "conv_ring_usable; convt_pair_kernel with sa.vec4 false")
    add("convt_fwd", "convt_pair", "y", 8, "pair: (y | preact) & 7 == 0 -> 8-B stores")
    add("convt_fwd", "convt_pair", "y", 4, "pair refused -> four launches")
    add("convt_fwd", "convt_pair", "x", 4, "SrcIm2colRow in convt_pair_kernel")
    for path in ("ring_s1_dgrad", "split_s1_dgrad", "ring_s2_dgrad", "direct4_flip_cs8"):
        add("dgrad", path, "dT", 4, "conv_ring_usable / plain3x3 on the gradient -> gather / conv_direct_kernel")
        add("dgrad", path, "dx", 8, "align_split 15 (stride 1), align 7 holds (stride 2), plain3x3 refuses")
        add("dgrad", path, "dx", 4, "align 7 (stride 2): the class loop; plain3x3 refuses")
    for path in ("ring_convt_dgrad", "split_convt_dgrad"):
        add("convt_dgrad", path, "dT", 4, "conv_ring_usable -> conv_mma_kernel<SrcIm2col> at stride 2")
        add("convt_dgrad", path, "dx", 8, "align_split 15 -> unsplit")
        add("convt_dgrad", path, "dx", 4, "the same at 4 B")
    for path in ("wgrad_direct", "wgrad_ring", "wgrad_mma_fast"):
        add("wgrad", path, "G", 4, "wgrad_direct_ok / ring / row: G & 15 -> conv_wgrad_kernel<false, false>")
        add("wgrad", path, "X", 4, "wgrad_direct_ok / ring: X & 15 -> conv_wgrad_kernel row forms")
        add("wgrad", path, "dw", 4, "launch_slab_reduce: out & 15 -> slab_reduce_kernel")
    return tuple(rows)


ALIGNMENT = _alignment()

# the layer of the issue's defect: models.layers.ConvLayer(8, 16, kernel_size=1, stride=2, padding=0) on 2 x 8 x 10 x 12
SHORTCUT = conv("shortcut-k1s2p0", 2, 8, 10, 12, 16, 1, 2, 0, "qarig_conv2d_bwd_data: k < stride")


def exact_cases():
    """Every case the GPU test runs with integer operands."""
    seen = {}
    for c in GEOMETRY + FORWARD_ONLY + tuple(p.case for p in PATHS):
        seen[c] = None
    return tuple(seen)
