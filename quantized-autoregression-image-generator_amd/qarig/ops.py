"""Raw (non-autograd) wrappers: one Python function per C-ABI entry point.

Shapes/dtypes/contiguity are validated here, before the call, so the C side only
sees well-formed arguments (SURVEY.md 8b "Errors").
"""
import ctypes
import math
import os

import torch

from . import _lib
from ._lib import check, f32c, ptr, require_cuda, stream, workspace
from .dropout import ATTN_DROPOUT_SITES      # attention sites the mask numbers (one definition)

ACT_IDS = {None: 0, "none": 0, "silu": 1, "tanh": 2, "sigmoid": 3}


def act_id(name):
    if name not in ACT_IDS:
        raise KeyError(name)  # same failure mode as the reference's ModuleDict lookup
    return ACT_IDS[name]


# --------------------------------------------------------------------------- BMU
_bmu_images = {}
_bmu_seen = {}               # id(codebook) -> state key of the last search (bmu_image only_if_stable)
BMU_IMAGE_MIN_ROWS = 24576   # the dispatch takes the coarse-pass kernel (the image's consumer) from here up
# K > 1024 (the chunked coarse pass): the row count from which the dispatch takes it by itself -- nowhere so far
# (csrc/bmu.hip BMU_CHUNKED_AUTO_ROWS, profiles/r08_bmu_large_k.log); under option bmu_coarse = 1 it runs at every
# row count, and the image is built for it there.
BMU_IMAGE_MIN_ROWS_LARGE_K = 2 ** 31 - 1


def bmu_invalidate():
    """Forget every prepared codebook image (after a write into parameters that neither torch's version counter
    nor FlatAdam's step count sees, e.g. parallel.broadcast_params)."""
    _bmu_images.clear()
    _bmu_seen.clear()


def _bmu_key(codebook):
    owner = getattr(codebook, "_qarig_owner", None)
    K, D = codebook.shape
    return (codebook.data_ptr(), K, D, codebook._version, owner.step_count if owner is not None else -1)


def bmu_image(codebook, only_if_stable=False):
    """Prepared image of a codebook for the coarse-pass search (include/qarig.h qarig_bmu_prepare), or
    None where that form does not apply.  Cached per codebook tensor until it changes: torch's version
    counter, and -- for a parameter FlatAdam owns, whose updates bypass that counter -- the optimiser's
    step count.  only_if_stable: build the image only for a codebook that an earlier call already saw in
    this state (a codebook under training changes between searches: preparing it every time would cost a
    launch for nothing)."""
    K, D = codebook.shape
    lib = _lib.load()
    nb = lib.qarig_bmu_prepare_bytes(K, D)
    if nb == 0 or codebook.data_ptr() % 16:
        return None
    key = _bmu_key(codebook)
    hit = _bmu_images.get(id(codebook))
    if hit is not None and hit[0] == key and hit[1]() is codebook:
        return hit[2]
    if torch.cuda.is_current_stream_capturing():
        return None                       # no allocation / caching inside a capture: the kernel stages by itself
    if only_if_stable:
        seen = _bmu_seen.get(id(codebook))
        _bmu_seen[id(codebook)] = key
        if len(_bmu_seen) > 256:
            _bmu_seen.clear()
        if seen != key:
            return None
    import weakref
    img = torch.empty(nb, dtype=torch.uint8, device=codebook.device)
    check(lib.qarig_bmu_prepare(ptr(codebook), K, D, ptr(img), stream()), "qarig_bmu_prepare")
    if len(_bmu_images) > 64:
        _bmu_images.clear()
    _bmu_images[id(codebook)] = (key, weakref.ref(codebook), img)
    return img


def bmu(x, codebook, patch_dim):
    """int64 (N*Seq,) best-matching-unit indices of every patch of x (N,C,H,W).

    Replaces patchify + torch.cdist + torch.argmin in Codebook.get_patches_bmu
    (reference models/Codebook.py:77-99)."""
    require_cuda(x, codebook)
    x = f32c(x)
    cb = codebook if (codebook.dtype == torch.float32 and codebook.is_contiguous()) else f32c(codebook)
    N, C, H, W = x.shape
    pH, pW = patch_dim
    K, D = cb.shape
    rows = N * (H // pH) * (W // pW)
    out = torch.empty(rows, dtype=torch.int64, device=x.device)
    lib = _lib.load()
    # Large launches take the coarse-pass kernel inside qarig_bmu_fwd.  A codebook that an earlier search saw in
    # its present state (frozen: tokenising a dataset, the Transformer training loop) goes in as its prepared
    # image, which the workgroups DMA into LDS instead of each converting the codebook (65,536 x 512 x 16:
    # 14.3 -> 13.x us).  Never inside a graph capture: a replay would search the image of the codebook as it was
    # when the graph was captured.
    # Only for an nn.Parameter: its identity is stable, torch's version counter sees every in-place update
    # through torch, FlatAdam's step count (p._qarig_owner) those made through the flat buffer.
    img = None
    if K <= 1024:
        wants_image = rows >= BMU_IMAGE_MIN_ROWS
    else:
        wants_image = rows >= BMU_IMAGE_MIN_ROWS_LARGE_K or _lib.option_value("bmu_coarse") == 1
    if wants_image and cb is codebook and isinstance(codebook, torch.nn.Parameter) and \
            not torch.cuda.is_current_stream_capturing():
        img = bmu_image(cb, only_if_stable=True)
    nb = lib.qarig_bmu_workspace_bytes(rows, K)
    ws = workspace(nb, x.device)
    check(lib.qarig_bmu_fwd_prepared(ptr(x), N, C, H, W, pH, pW, ptr(cb), K, D, ptr(out), ptr(ws),
                                     ws.numel(), ptr(img), stream()), "qarig_bmu_fwd_prepared")
    return out


def bmu_coarse(x, codebook, patch_dim, prepared=False):
    """(indices, rows that needed the exact re-scan): the coarse-pass form of `bmu` forced
    (include/qarig.h qarig_bmu_fwd_coarse; beyond 1,024 codes its chunked form, qarig_bmu_fwd_coarse_ws); raises
    where it does not apply.  prepared: through the cached codebook image (bmu_image) instead of staging the
    codebook in every workgroup."""
    require_cuda(x, codebook)
    x = f32c(x)
    codebook = f32c(codebook)
    N, C, H, W = x.shape
    pH, pW = patch_dim
    K, D = codebook.shape
    out = torch.empty(N * (H // pH) * (W // pW), dtype=torch.int64, device=x.device)
    cnt = torch.zeros(8, dtype=torch.int32, device=x.device)    # [0] re-scanned rows, [1..4] phase clocks
    img = bmu_image(codebook) if prepared else None
    lib = _lib.load()
    if K > 1024:
        ws = workspace(lib.qarig_bmu_coarse_workspace_bytes(out.numel(), K), x.device)
        check(lib.qarig_bmu_fwd_coarse_ws(ptr(x), N, C, H, W, pH, pW, ptr(codebook), K, D, ptr(out), ptr(cnt),
                                          ptr(img), ptr(ws), ws.numel(), stream()), "qarig_bmu_fwd_coarse_ws")
    else:
        check(lib.qarig_bmu_fwd_coarse(ptr(x), N, C, H, W, pH, pW, ptr(codebook), K, D, ptr(out), ptr(cnt),
                                       ptr(img), stream()), "qarig_bmu_fwd_coarse")
    return out, cnt[:1] if not BMU_COARSE_PHASES else cnt


BMU_COARSE_PHASES = False      # tools: return all eight counters


# ------------------------------------------------------------- SOM topology
def bmu_top2(x, codebook, patch_dim):
    """(idx1, idx2, d1, d2) of every patch of x (N,C,H,W): the two best-matching units under the (d, k) order of
    include/qarig.h qarig_bmu_top2 (int64, int64, fp32, fp32; N*Seq each).  idx1 equals `bmu` (beyond the 25 rows
    x 25 codes up to which `bmu` takes torch.cdist's direct form); 2 <= K <= 16384."""
    require_cuda(x, codebook)
    x = f32c(x)
    cb = f32c(codebook)
    N, C, H, W = x.shape
    pH, pW = patch_dim
    K, D = cb.shape
    rows = N * (H // pH) * (W // pW)
    idx = torch.empty((2, rows), dtype=torch.int64, device=x.device)
    d = torch.empty((2, rows), dtype=torch.float32, device=x.device)
    check(_lib.load().qarig_bmu_top2(ptr(x), N, C, H, W, pH, pW, ptr(cb), K, D, ptr(idx[0]), ptr(idx[1]), ptr(d[0]),
                                     ptr(d[1]), stream()), "qarig_bmu_top2")
    return idx[0], idx[1], d[0], d[1]


def topology_rows(idx1, idx2, d1, d2, images, gap_hist, ratio_hist, img_sums=None):
    """Reduces one bmu_top2 call of `images` images: returns img_sums (images,3) fp64 = per-image {sum d1, sum d2,
    sum d1^2} (written into `img_sums` when given) and adds the histograms of |idx1 - idx2| and of
    min(31, floor(32 d1 / d2)) to gap_hist (int64 [K]) and ratio_hist (int64 [32]), all on the device
    (include/qarig.h qarig_topology_rows).  Every tensor must be contiguous."""
    require_cuda(idx1, idx2, d1, d2, gap_hist, ratio_hist, img_sums)
    rows = idx1.numel()
    if images < 1 or rows % images or not (idx2.numel() == d1.numel() == d2.numel() == rows):
        raise ValueError(f"topology_rows: {rows} rows do not make {images} images of equal length")
    if img_sums is None:
        img_sums = torch.empty((images, 3), dtype=torch.float64, device=idx1.device)
    for name, t, dt in (("idx1", idx1, torch.int64), ("idx2", idx2, torch.int64), ("d1", d1, torch.float32),
                        ("d2", d2, torch.float32), ("gap_hist", gap_hist, torch.int64),
                        ("ratio_hist", ratio_hist, torch.int64), ("img_sums", img_sums, torch.float64)):
        if t.dtype != dt or not t.is_contiguous():
            raise ValueError(f"topology_rows: {name} must be a contiguous {dt} tensor")
    if ratio_hist.numel() != 32 or img_sums.numel() != images * 3:
        raise ValueError("topology_rows: ratio_hist has 32 bins, img_sums is (images, 3)")
    check(_lib.load().qarig_topology_rows(ptr(idx1), ptr(idx2), ptr(d1), ptr(d2), images, rows // images,
                                          gap_hist.numel(), ptr(img_sums), ptr(gap_hist), ptr(ratio_hist),
                                          ptr(_bad_flag(idx1.device)), stream()), "qarig_topology_rows")
    return img_sums


def code_lag_profile(codebook):
    """fp64 [K]: [r] = sum_t |w_t - w_{t+r}| over the codebook's index axis, r = 1 ... K-1; [0] = 0
    (include/qarig.h qarig_code_lag_profile)."""
    require_cuda(codebook)
    cb = f32c(codebook)
    K, D = cb.shape
    out = torch.zeros(K, dtype=torch.float64, device=cb.device)
    check(_lib.load().qarig_code_lag_profile(ptr(cb), K, D, ptr(out), stream()), "qarig_code_lag_profile")
    return out


# -------------------------------------------------------------------------- GEMM
# bench.py sets this to a list to bracket every GEMM launch with HIP events on the
# launch stream: entries are (flops, start_event, end_event).
GEMM_EVENTS = None

# "f32" (default; the parity mode: exact fp32 fma chains on the fp32 MFMA) or "bf16"
# (opt-in: Linear-layer contractions on the bf16 MFMA with fp32 accumulation and fp32
# tensors; BASELINE config 5 direction, tolerance stated in tests/test_gpu_bf16.py).
# QARIG_PRECISION in the environment sets the default.
# "fp8" adds per-tensor e4m3 forward products to "bf16"; "mxfp8" runs every product of the Linear
# nodes (forward and both gradients) on block-scaled MX-e4m3 operands (include/qarig.h).
PRECISION = os.environ.get("QARIG_PRECISION", "f32")
PRECISIONS = ("f32", "bf16", "fp8", "mxfp8")


def lp_mode():
    """bf16 storage / bf16-MFMA nodes active ("bf16"; "fp8" and "mxfp8" build on it)."""
    return PRECISION in ("bf16", "fp8", "mxfp8")


def set_precision(name):
    """Selects the contraction precision of the Linear / attention products for the process."""
    global PRECISION
    if name not in PRECISIONS:
        raise ValueError(f"qarig.ops precision must be one of {PRECISIONS}, not {name!r}")
    PRECISION = name


def gemm(A, B, a_kcontig=True, b_kcontig=True, bias=None, residual=None, want_preact=False,
         act=0, gradz=None, gact=0, splitk=None, out=None, accumulate=False, a_rowsum=None,
         flop_frac=1.0):
    """C[M,N] = epilogue(sum_k A(m,k) B(n,k)); see include/qarig.h qarig_gemm_f32.
    flop_frac: fraction of the 2MNK products that are algorithmic work (zero-padded operands
    of the ragged classifier): only bench.py's FLOP accounting reads it.

    A is (M,K) if a_kcontig else (K,M); B is (N,K) if b_kcontig else (K,N).
    Returns C, or (C, preact) when want_preact."""
    require_cuda(A, B, bias, residual, gradz)
    assert A.dim() == 2 and B.dim() == 2 and A.dtype == torch.float32 and B.dtype == torch.float32
    assert A.stride(1) == 1 and B.stride(1) == 1, "operands must be row-contiguous"
    M, K = (A.shape if a_kcontig else (A.shape[1], A.shape[0]))
    N, K2 = (B.shape if b_kcontig else (B.shape[1], B.shape[0]))
    assert K == K2, f"reduction mismatch {K} vs {K2}"
    C = out if out is not None else torch.empty((M, N), dtype=torch.float32, device=A.device)
    assert C.shape == (M, N) and C.stride(1) == 1
    pre = torch.empty((M, N), dtype=torch.float32, device=A.device) if want_preact else None
    if bias is not None:
        assert bias.shape == (N,) and bias.is_contiguous()
    for t in (residual, gradz):
        if t is not None:
            assert t.shape == (M, N) and t.stride(1) == 1
    if splitk is None:
        splitk = auto_splitk(M, N, K)
    lib = _lib.load()
    ws = None
    nws = 0
    if a_rowsum is not None:
        assert a_rowsum.shape == (M,) and a_rowsum.is_contiguous() and a_rowsum.dtype == torch.float32
    # (the ragged weight-gradient route keeps its tail partials in the workspace at any split)
    if splitk > 1 or a_rowsum is not None or (not a_kcontig and not b_kcontig and lib.qarig_gemm_ragged_tn(M, N, K)):
        nws = lib.qarig_gemm_workspace_bytes(M, N, splitk)
        ws = workspace(nws, A.device, "gemm")
        nws = ws.numel()
    if lp_mode():
        done = _gemm_lp(lib, A, B, a_kcontig, b_kcontig, C, pre, M, N, K, bias, residual, act, gradz,
                        gact, splitk, accumulate, a_rowsum)
        if done:
            return (C, pre) if want_preact else C
    elif PRECISION != "f32":
        raise ValueError(f"qarig.ops.PRECISION must be one of {PRECISIONS}, not {PRECISION!r}")
    fn, fn_name = lib.qarig_gemm_f32, "qarig_gemm_f32"
    if GEMM_EVENTS is not None:
        ev0 = torch.cuda.Event(enable_timing=True)
        ev0.record()
    check(fn(
        ptr(A), A.stride(0), int(a_kcontig), ptr(B), B.stride(0), int(b_kcontig),
        ptr(C), C.stride(0), M, N, K, ptr(bias),
        ptr(residual), residual.stride(0) if residual is not None else 0,
        ptr(pre), pre.stride(0) if pre is not None else 0, act,
        ptr(gradz), gradz.stride(0) if gradz is not None else 0, gact,
        splitk, int(accumulate), ptr(a_rowsum), ptr(ws), nws, stream()), fn_name)
    if GEMM_EVENTS is not None:
        ev1 = torch.cuda.Event(enable_timing=True)
        ev1.record()
        outs = "+".join(n for n, t in (("C", C), ("P", pre)) if t is not None)
        ins = "".join(n for n, t in (("b", bias), ("r", residual), ("z", gradz), ("s", a_rowsum)) if t is not None)
        hbm = 4.0 * (M * K + N * K + M * N * ((2 if accumulate and splitk == 1 else 1) + (pre is not None) +
                                              (residual is not None) + (gradz is not None)))
        GEMM_EVENTS.append((2.0 * M * N * K * flop_frac, ev0, ev1, "",
                            f"f32 {'N' if a_kcontig else 'T'}{'T' if b_kcontig else 'N'} {M}x{N}x{K} sk{splitk} "
                            f"out {outs} in {ins or '-'} act{act}{' acc' if accumulate else ''}", hbm))
    return (C, pre) if want_preact else C


# ---- reduced precision (BASELINE config 5): bf16 operands in HBM -------------------------------
# bf16 shadows of tensors that several GEMMs read (weights, in both layouts): keyed by storage,
# shape, torch's in-place version counter and LP_EPOCH, which qarig.optim bumps whenever its
# Adam kernel rewrites the parameters behind torch's back.
LP_EPOCH = 0
_lp_cache = {}


def lp_invalidate():
    """Every key carries LP_EPOCH, so all entries are dead after the bump: drop them (and the device
    memory they hold) right away."""
    global LP_EPOCH
    LP_EPOCH += 1
    _lp_cache.clear()


def _lp_get(key, src):
    """Cached shadow of `src` under `key`, or None.  Keys name a tensor by address / shape / version
    only, and an address can be handed to another tensor of the same shape once its owner is freed
    (a second model built in the same process): an entry therefore also holds a weak reference to
    the tensor it was made from and only serves that very tensor."""
    hit = _lp_cache.get(key)
    if hit is None:
        return None
    if hit[0]() is not src:
        del _lp_cache[key]
        return None
    return hit[1]


_LP_CACHE_MAX = 1024     # entries; a process that keeps meeting new weights / geometries starts over


def _lp_put(key, src, value):
    import weakref
    if len(_lp_cache) >= _LP_CACHE_MAX:
        _lp_cache.clear()
    _lp_cache[key] = (weakref.ref(src), value)


def _lp_image(head, x, build, extras=(), tail=()):
    """The cached image of weight x under the key (head, address, shape, *extras, version, LP_EPOCH, *tail):
    build() makes it on a miss, and it is kept for -- and only served to -- the tensor x stands for (x._qarig_src
    when x is a detached alias of a parameter, else x).  Under stream capture there is no lookup and no store:
    the image is rebuilt, so that a replayed graph reads the weights the optimiser has just written and holds no
    address that an invalidation can free."""
    if torch.cuda.is_current_stream_capturing():
        return build()
    src = getattr(x, "_qarig_src", x)
    key = (head, x.data_ptr(), tuple(x.shape), *extras, x._version, LP_EPOCH, *tail)
    hit = _lp_get(key, src)
    if hit is None:
        hit = build()
        _lp_put(key, src, hit)
    return hit


def cast_bf16(x, cache=False):
    """bf16 copy (torch.bfloat16, same shape) of a dense fp32 tensor, rounded to nearest even."""
    assert x.dtype == torch.float32 and x.is_contiguous()
    if cache:
        return _lp_image("n", x, lambda: cast_bf16(x))
    out = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    check(_lib.load().qarig_cast_bf16(ptr(x), ptr(out), x.numel(), stream()), "qarig_cast_bf16")
    return out


def cast_fp8(x, cache=False, want_bf16=False):
    """(e4m3 bytes as torch.uint8 of x's shape, dequantisation factor as a 1-element fp32 tensor
    [, bf16 copy of x from the same pass]) of a dense fp32 tensor: one scale for the tensor, 448 / max|x| (include/qarig.h
    qarig_cast_fp8).  The factor stays on the device; the GEMM epilogue multiplies by it."""
    assert x.dtype == torch.float32 and x.is_contiguous() and x.numel() % 4 == 0
    if cache:
        return _lp_image("f8", x, lambda: cast_fp8(x, want_bf16=want_bf16))
    out = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    aux = torch.empty(2, dtype=torch.float32, device=x.device)     # [0] inv_scale, [1] amax bits
    xb = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device) if want_bf16 else None
    check(_lib.load().qarig_cast_fp8(ptr(x), x.numel(), ptr(out), ptr(aux), aux.data_ptr() + 4, ptr(xb),
                                     stream()), "qarig_cast_fp8")
    return (out, aux[:1], xb) if want_bf16 else (out, aux[:1])


def f8_supported(M, N, K):
    return bool(_lib.load().qarig_gemm_f8_supported(M, N, K))


def _ld(t):
    return t.stride(0) if t is not None else 0


def _epilogue_args(C, M, N, K, bias, residual, preact, act, Cb, Pb, grad=()):
    """The epilogue arguments that qarig_gemm_lp / _f8 / _mx share, in their order: C, the extents, bias,
    residual, pre-activation, act, [`grad`: gradz, gact, splitk, accumulate -- not for _f8], Cb, Pb."""
    if grad:
        gradz, gact, splitk, accumulate = grad
        grad = (ptr(gradz), _ld(gradz), int(gradz is not None and gradz.dtype == torch.bfloat16), gact, splitk,
                int(accumulate))
    return (ptr(C), _ld(C), M, N, K, ptr(bias), ptr(residual), _ld(residual), ptr(preact), _ld(preact), act,
            *grad, ptr(Cb), _ld(Cb), ptr(Pb), _ld(Pb))


def _splitk_workspace(nbytes_fn, M, N, splitk, device):
    """(workspace, its size) for the fp32 slabs of a split-K product; (None, 0) without split-K."""
    if splitk <= 1:
        return None, 0
    ws = workspace(nbytes_fn(M, N, splitk), device, "gemm")
    return ws, ws.numel()


def _event_begin():
    """Start event of a GEMM_EVENTS record (None when nothing is recorded)."""
    if GEMM_EVENTS is None:
        return None
    ev0 = torch.cuda.Event(enable_timing=True)
    ev0.record()
    return ev0


def _event_end(ev0, M, N, K, tail):
    """Appends (flops, start, end, *tail()) to GEMM_EVENTS."""
    if ev0 is None or GEMM_EVENTS is None:
        return
    ev1 = torch.cuda.Event(enable_timing=True)
    ev1.record()
    GEMM_EVENTS.append((2.0 * M * N * K, ev0, ev1, *tail()))


def _lp_event_tail(what, operand_bytes, M, N, K, C, bias, residual, preact, act, gradz, splitk, accumulate, Cb, Pb):
    """("", description, HBM bytes) of a reduced-precision product for its GEMM_EVENTS record."""
    outs = "+".join(n for n, t in (("C", C), ("P", preact), ("Cb", Cb), ("Pb", Pb)) if t is not None)
    ins = "".join(n for n, t in (("b", bias), ("r", residual), ("z", gradz)) if t is not None)
    hbm = operand_bytes * (M * K + N * K) + M * N * (4.0 * (C is not None) * (2 if accumulate and splitk == 1 else 1) +
                                                     4.0 * (preact is not None) + 2.0 * (Cb is not None) +
                                                     2.0 * (Pb is not None) + 4.0 * (residual is not None) +
                                                     (0 if gradz is None else gradz.element_size()))
    return "", f"{what} {M}x{N}x{K} sk{splitk} out {outs} in {ins or '-'} act{act}", hbm


def gemm_f8(A8, inv_a, B8, inv_b, M, N, K, C=None, bias=None, residual=None, preact=None, act=0,
            Cb=None, Pb=None):
    """Forward product on e4m3 operands (include/qarig.h qarig_gemm_f8): C = epilogue(inv_a * inv_b *
    A8 B8^T), A8 (M,K) and B8 (N,K) uint8 from cast_fp8."""
    ev0 = _event_begin()
    check(_lib.load().qarig_gemm_f8(
        ptr(A8), A8.stride(0), ptr(B8), B8.stride(0), ptr(inv_a), ptr(inv_b),
        *_epilogue_args(C, M, N, K, bias, residual, preact, act, Cb, Pb), stream()), "qarig_gemm_f8")
    _event_end(ev0, M, N, K, lambda: ("f8",))


class MxOperand:
    """An MX-e4m3 operand (include/qarig.h): q (rows, K) e4m3 bytes as torch.uint8, s (rows, K/32) e8m0
    scale bytes.  `rows` is the logical row count of the product operand."""
    __slots__ = ("q", "s")

    def __init__(self, q, s):
        self.q, self.s = q, s


def mx_quant(x, row=True, transposed=False, colsum=None, accumulate=False):
    """One pass over x (R, C) (fp32 or bf16, row-contiguous, C % 128 == 0): (row form or None,
    transposed form or None) as MxOperand; with `colsum` (fp32 (C,)) the column sums of x are
    written into it (added with `accumulate`)."""
    assert x.dim() == 2 and x.stride(1) == 1 and x.dtype in (torch.float32, torch.bfloat16)
    R, C = x.shape
    Rp = (R + 127) // 128 * 128
    dev = x.device
    rf = MxOperand(torch.empty((R, C), dtype=torch.uint8, device=dev),
                   torch.empty((R, C // 32), dtype=torch.uint8, device=dev)) if row else None
    tf = MxOperand(torch.empty((C, Rp), dtype=torch.uint8, device=dev),
                   torch.empty((C, Rp // 32), dtype=torch.uint8, device=dev)) if transposed else None
    lib = _lib.load()
    ws, nws = None, 0
    if colsum is not None:
        assert colsum.shape == (C,) and colsum.is_contiguous() and colsum.dtype == torch.float32
        ws = workspace(lib.qarig_mx_quant_workspace_bytes(R, C), dev, "colsum")
        nws = ws.numel()
    check(lib.qarig_mx_quant(ptr(x), x.stride(0), int(x.dtype == torch.bfloat16), R, C,
                             ptr(rf.q if rf else None), ptr(rf.s if rf else None),
                             ptr(tf.q if tf else None), ptr(tf.s if tf else None), ptr(colsum), int(accumulate),
                             ptr(ws), nws, stream()), "qarig_mx_quant")
    return rf, tf


def mx_supported(M, N, K, splitk=1):
    return bool(_lib.load().qarig_gemm_mx_supported(int(M), int(N), int(K), int(splitk)))


def gemm_mx(A, B, M, N, K, C=None, bias=None, residual=None, preact=None, act=0, gradz=None, gact=0, splitk=1,
            accumulate=False, Cb=None, Pb=None):
    """C = epilogue(A B^T) on MX-e4m3 operands (include/qarig.h qarig_gemm_mx): A, B MxOperand with
    (M, K) and (N, K) bytes; epilogue options as gemm_lp."""
    lib = _lib.load()
    ws, nws = _splitk_workspace(lib.qarig_gemm_mx_workspace_bytes, M, N, splitk, A.q.device)
    ev0 = _event_begin()
    check(lib.qarig_gemm_mx(
        ptr(A.q), A.q.stride(0), ptr(A.s), A.s.stride(0), ptr(B.q), B.q.stride(0), ptr(B.s), B.s.stride(0),
        *_epilogue_args(C, M, N, K, bias, residual, preact, act, Cb, Pb, (gradz, gact, splitk, accumulate)),
        ptr(ws), nws, stream()), "qarig_gemm_mx")
    _event_end(ev0, M, N, K, lambda: _lp_event_tail("mx NT", 1.03, M, N, K, C, bias, residual, preact, act, gradz,
                                                    splitk, accumulate, Cb, Pb))


def mx_weight(w, pad_rows=0):
    """(row form, transposed form) of a weight (N, K) -- zero-padded to pad_rows output rows when
    given -- cached until the next optimiser step under the keys of the bf16 shadows (address,
    shape, version, LP_EPOCH); rebuilt on every call under stream capture, so that a replayed
    graph quantises the weights the optimiser has just written."""
    Np = pad_rows or w.shape[0]

    def quantised():
        wd = w.detach()
        if Np != w.shape[0]:
            wp = torch.zeros((Np, w.shape[1]), dtype=torch.float32, device=w.device)
            wp[:w.shape[0]].copy_(wd)
            wd = wp
        return mx_quant(wd if wd.is_contiguous() else wd.contiguous(), row=True, transposed=True)

    return _lp_image("mx", w, quantised, extras=(Np,))


def cast_transpose_bf16(x, cache=False):
    """bf16 (C, R) transpose of a row-contiguous fp32 (R, C) matrix."""
    assert x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1
    if cache:
        return _lp_image("t", x, lambda: cast_transpose_bf16(x), extras=(x.stride(0),))
    R, Cc = x.shape
    out = torch.empty((Cc, R), dtype=torch.bfloat16, device=x.device)
    check(_lib.load().qarig_cast_transpose_bf16(ptr(x), x.stride(0), R, Cc, ptr(out), stream()),
          "qarig_cast_transpose_bf16")
    return out


def cast_colsum(x, colsum_out, accumulate=False, want_cast=True):
    """One pass over x (M,N) (fp32, or bf16 with want_cast False): column sums (+)= into
    colsum_out (fp32 (N,)) -- the bias gradient -- and, for fp32 input, the bf16 copy of x."""
    M, N = x.shape
    assert x.stride(1) == 1 and colsum_out.shape == (N,) and colsum_out.is_contiguous()
    is_bf = x.dtype == torch.bfloat16
    out = torch.empty((M, N), dtype=torch.bfloat16, device=x.device) if (want_cast and not is_bf) else None
    lib = _lib.load()
    ws = workspace(lib.qarig_cast_colsum_workspace_bytes(M, N), x.device, "colsum")
    check(lib.qarig_cast_colsum(ptr(x), x.stride(0), int(is_bf), M, N, ptr(out), ptr(colsum_out),
                                int(accumulate), ptr(ws), ws.numel(), stream()), "qarig_cast_colsum")
    return out


def _is_param_like(t):
    """Weights (cached shadows) vs activations (cast per call)."""
    return isinstance(t, torch.nn.Parameter) or getattr(t, "_qarig_weight", False)


def gemm_lp(A_bf, B_bf, layout, M, N, K, C=None, bias=None, residual=None, preact=None, act=0, gradz=None,
            gact=0, splitk=1, accumulate=False, Cb=None, Pb=None):
    """Raw reduced-precision GEMM on bf16 operands (include/qarig.h qarig_gemm_lp)."""
    lib = _lib.load()
    ws, nws = _splitk_workspace(lib.qarig_gemm_lp_workspace_bytes, M, N, splitk, A_bf.device)
    ev0 = _event_begin()
    check(lib.qarig_gemm_lp(
        ptr(A_bf), A_bf.stride(0), ptr(B_bf), B_bf.stride(0), layout,
        *_epilogue_args(C, M, N, K, bias, residual, preact, act, Cb, Pb, (gradz, gact, splitk, accumulate)),
        ptr(ws), nws, stream()), "qarig_gemm_lp")
    _event_end(ev0, M, N, K, lambda: _lp_event_tail(f"lp {('NT', 'TN', 'NN')[layout]}", 2.0, M, N, K, C, bias,
                                                    residual, preact, act, gradz, splitk, accumulate, Cb, Pb))


def _gemm_lp(lib, A, B, a_kcontig, b_kcontig, C, pre, M, N, K, bias, residual, act, gradz, gact, splitk,
             accumulate, a_rowsum):
    """The fp32-tensor GEMM contract on the bf16 MFMA: operands are cast to bf16 in HBM (weights
    once per optimiser step, in the layout the product needs; activations per call) and
    multiplied by qarig_gemm_lp.  Returns False when the shape is not an interior one (the
    caller then runs the fp32 kernels).  The three Linear products map to
        forward   (kc, kc): NT on  x_bf (M,K)    and W_bf (N,K)
        d-input   (kc, xc): NN on  dT_bf (M,N')  and the weight shadow as stored (N',K')
        d-weight  (xc, xc): TN on  dT_bf, x_bf as they lie (row-major, reduction-major)."""
    if a_kcontig == (not b_kcontig) and not a_kcontig:
        return False                       # (xc, kc) never occurs on the hot path
    if splitk > 1 and (K % splitk or (K // splitk) % 64):
        s = splitk
        while s > 1 and (K % s or (K // s) % 64):
            s -= 1
        splitk = s
    plain = bias is None and residual is None and pre is None and gradz is None and act == 0
    if splitk > 1 and not plain:
        splitk = 1
    if not lib.qarig_gemm_lp_supported(M, N, K, splitk):
        return False
    for t in (A, B):
        if t.data_ptr() % 16 or t.stride(0) % 8:
            return False
    if a_rowsum is not None:
        if a_kcontig:
            return False
        colsum(A, out=a_rowsum, accumulate=accumulate)      # bias gradient: its own fp32 pass
    if a_kcontig and b_kcontig:            # forward
        A_bf = cast_bf16(A if A.is_contiguous() else A.contiguous())
        B_bf = cast_bf16(B if B.is_contiguous() else B.contiguous(), cache=_is_param_like(B))
        layout = 0
    elif a_kcontig:                        # d-input: B is (K_red, N_out) = the weight as stored
        if B.stride(0) % 8 or not B.is_contiguous():
            return False
        A_bf = cast_bf16(A if A.is_contiguous() else A.contiguous())
        B_bf = cast_bf16(B, cache=_is_param_like(B))
        layout = 2
    else:                                  # d-weight
        A_bf = cast_bf16(A if A.is_contiguous() else A.contiguous())
        B_bf = cast_bf16(B if B.is_contiguous() else B.contiguous())
        layout = 1
    gemm_lp(A_bf, B_bf, layout, M, N, K, C=C, bias=bias, residual=residual, preact=pre, act=act,
            gradz=gradz, gact=gact, splitk=splitk, accumulate=accumulate)
    return True


def gemm_grouped_skinny(A, W, bias=None, act=0, shared_a=False):
    """out[g] = act(A[g] @ W[g].T + bias[g]).  A: (G, M, K) or (M, K) with shared_a;
    W: (G, N, K); bias: (G, N) or None.  M <= 512, K % 256 == 0.  Returns (G, M, N)."""
    require_cuda(A, W, bias)
    G, N, K = W.shape
    assert W.is_contiguous() and A.is_contiguous() and A.dtype == W.dtype == torch.float32
    if shared_a:
        M, Ka = A.shape
        a_gs = 0
    else:
        Ga, M, Ka = A.shape
        assert Ga == G
        a_gs = M * K
    assert Ka == K
    if bias is not None:
        assert bias.shape == (G, N) and bias.is_contiguous()
    C = torch.empty((G, M, N), dtype=torch.float32, device=A.device)
    check(_lib.load().qarig_gemm_grouped_skinny_f32(
        ptr(A), K, a_gs, ptr(W), K, N * K, ptr(C), N, M * N, ptr(bias), N, G, M, N, K, act,
        stream()), "qarig_gemm_grouped_skinny_f32")
    return C


# launches of the strided-groups ring product, counted per call (tests assert the training forward of a
# position table took it)
STRIDED_CALLS = {"gemm_strided": 0}
# ragged-width routes taken by the Linear and loss nodes, counted per call: the classifier forward on its true width,
# its weight gradient on the true rows, the cross-entropy launch on logits left in their padded buffer
RAGGED_CALLS = {"forward": 0, "wgrad": 0, "ce_ld": 0}


def gemm_strided_supported(M, N, K):
    """Shapes gemm_strided takes: whole 128 x 128 tiles and 16-deep k-tiles (include/qarig.h)."""
    return bool(_lib.load().qarig_gemm_grouped_supported(int(M), int(N), int(K), 1))


def table_forward_ring(G, P, D):
    """The training forward of G (D, D) projections of a (P, D) position table goes to gemm_strided when the
    shape is one of its own and the launch gives every one of the 256 CUs a workgroup (BASELINE config 2: 42
    projections of 384 positions, 504 tiles); a smaller launch leaves CUs idle behind lone waves, and the
    skinny launch is kept (config 4's 256 encoder positions: 240 tiles)."""
    return gemm_strided_supported(P, D, D) and G * (P // 128) * (D // 128) >= 256


def gemm_strided(A, W, bias=None, act=0):
    """out[g] = act(A @ W[g].T + bias[g]) for any number of groups that share A, as one launch of
    G * (M/128) * (N/128) tiles on the fp32 ring (include/qarig.h qarig_gemm_f32_strided).
    A: (M, K); W: (G, N, K); bias: (G, N) or None.  Returns (G, M, N)."""
    require_cuda(A, W, bias)
    G, N, K = W.shape
    M, Ka = A.shape
    assert Ka == K and W.is_contiguous() and A.is_contiguous() and A.dtype == W.dtype == torch.float32
    if bias is not None:
        assert bias.shape == (G, N) and bias.is_contiguous() and bias.dtype == torch.float32
    C = torch.empty((G, M, N), dtype=torch.float32, device=A.device)
    ev0 = _event_begin()
    check(_lib.load().qarig_gemm_f32_strided(
        ptr(A), K, ptr(W), K, N * K, ptr(C), N, M * N, ptr(bias), N, G, M, N, K, act, stream()),
        "qarig_gemm_f32_strided")
    STRIDED_CALLS["gemm_strided"] += 1
    _event_end(ev0, M, G * N, K, lambda: (
        "f32g" if lp_mode() else "",
        f"f32 NT strided {G}x {M}x{N}x{K} out C in {'b' if bias is not None else '-'} act{act}",
        4.0 * (M * K + G * N * K + G * M * N)))
    return C


def gemm_skinny_ln(x, W, bias=None, act=0, gamma=None, beta=None, scale=None, shift=None, eps=1e-5, mul=None):
    """out[g] = act(LN(x) @ W[g].T + bias[g]) [* mul]: the decode step's Linear with the LayerNorm in
    front of it (affine gamma/beta (K,) or AdaLN scale/shift (M, K); neither: none) and the gate
    multiply behind it (mul (M, N)) inside the same launch.  x: (M, K); W: (G, N, K) or (N, K);
    bias: like W without K.  Returns (G, M, N), or (M, N) for a 2-D W."""
    require_cuda(x, W, bias, gamma, beta, scale, shift, mul)
    single = W.dim() == 2
    G, (N, K) = (1 if single else W.shape[0]), W.shape[-2:]
    M = x.shape[0]
    assert x.shape == (M, K) and x.is_contiguous() and W.is_contiguous() and x.dtype == W.dtype == torch.float32
    if bias is not None:
        assert bias.numel() == G * N and bias.is_contiguous()
    for t in (gamma, beta):
        assert t is None or (t.shape == (K,) and t.is_contiguous())
    for t in (scale, shift):
        assert t is None or (t.shape == (M, K) and t.is_contiguous())
    assert mul is None or (mul.shape == (M, N) and mul.is_contiguous() and G == 1)
    C = torch.empty((G, M, N), dtype=torch.float32, device=x.device)
    check(_lib.load().qarig_gemm_skinny_ln_f32(
        ptr(x), K, float(eps), ptr(gamma), ptr(beta), ptr(scale), ptr(shift), K, ptr(W), K, N * K, ptr(C), N,
        M * N, ptr(bias), N, ptr(mul), N, G, M, N, K, act, stream()), "qarig_gemm_skinny_ln_f32")
    return C[0] if single else C


def decode_linear_supported(M, N, K, ln=False):
    return bool(_lib.load().qarig_decode_linear_supported(int(M), int(N), int(K), int(bool(ln))))


def decode_linear(x, W, bias=None, act=0, gamma=None, beta=None, scale=None, shift=None, eps=1e-5,
                  residual=None, mul=None, out=None):
    """out[g] = act(LN(x[g]) @ W[g].T + bias[g] + residual) * mul -- the Linear of a single-token decode
    step on the weight-streaming kernel (csrc/decode.hip; M <= 16 rows).  x: (M, K) shared by the
    groups, or (G, M, K); W: (G, N, K) or (N, K); bias like W without K.  LN: gamma/beta (K,), or
    scale/shift (M, K) rows or ONE (K,) row for every activation row.  residual (M, N) (one group);
    mul (M, N) or (N,).  Returns (G, M, N), or (M, N) for a 2-D W.
    W fp32, or torch.bfloat16 -- a bf16 image of the weight (cast_bf16), streamed at half the bytes and widened
    exactly in the kernel (qarig_decode_linear_bf16w): everything else stays fp32."""
    require_cuda(x, W, bias, gamma, beta, scale, shift, residual, mul)
    single = W.dim() == 2
    G, (N, K) = (1 if single else W.shape[0]), W.shape[-2:]
    if x.dim() == 3:
        assert x.shape[0] == G
        M, x_gs = x.shape[1], x.shape[1] * K
    else:
        M, x_gs = x.shape[0], 0
    assert x.shape[-1] == K and x.is_contiguous() and W.is_contiguous() and x.dtype == torch.float32
    assert W.dtype in (torch.float32, torch.bfloat16)
    lp = W.dtype == torch.bfloat16
    if bias is not None:
        assert bias.numel() == G * N and bias.is_contiguous()
    for t in (gamma, beta):
        assert t is None or (t.shape == (K,) and t.is_contiguous())
    ldmod = 0
    for t in (scale, shift):
        assert t is None or (t.shape in ((M, K), (K,)) and t.is_contiguous())
    if scale is not None:
        assert scale.shape == shift.shape
        ldmod = K if scale.dim() == 2 else 0
    assert residual is None or (residual.shape == (M, N) and residual.is_contiguous() and G == 1)
    ldmul = 0
    if mul is not None:
        assert mul.shape in ((M, N), (N,)) and mul.is_contiguous()
        ldmul = N if mul.dim() == 2 else 0
    C = out if out is not None else torch.empty((G, M, N), dtype=torch.float32, device=x.device)
    assert C.numel() == G * M * N and C.is_contiguous() and C.dtype == torch.float32
    entry = "qarig_decode_linear_bf16w" if lp else "qarig_decode_linear_f32"
    check(getattr(_lib.load(), entry)(
        ptr(x), K, x_gs, float(eps), ptr(gamma), ptr(beta), ptr(scale), ptr(shift), ldmod, ptr(W), K, N * K,
        ptr(bias), N, ptr(residual), N, ptr(mul), ldmul, ptr(C), N, M * N, G, M, N, K, act, stream()), entry)
    return C.view(M, N) if single else C.view(G, M, N)


GEMM_MAX_GROUPS = 16          # csrc/gemm.hip GEMM_MAX_GROUPS


def grouped_splitk(groups, M, N, K):
    """Reduction split of a grouped launch of `groups` (M, N, K) products: 1 when the groups alone
    fill the chip twice over, else the smallest split whose workgroup count is at least 512 and a
    (near) multiple of the 256 CUs -- co-resident workgroups share a CU's matrix pipes, so the
    launch lasts as long as its busiest CU."""
    tiles = groups * ((M + 127) // 128) * ((N + 127) // 128)
    if tiles >= 512:
        return 1
    best, best_eff = 1, 0.0
    for s in (1, 2, 3, 4, 6, 8, 12, 16):
        if K % (16 * s) or K // s < 128:
            continue
        wg = tiles * s
        eff = wg / (-(-wg // 256) * 256)
        if wg >= 512 and eff >= 0.95:
            return s
        if eff > best_eff + 1e-9:
            best, best_eff = s, eff
    return best


def gemm_grouped_supported(M, N, K, splitk=1, any_precision=False):
    """any_precision: callers whose products stay on the fp32 grouped kernel in the reduced-precision mode
    too (the conditioning projections of a position table: a few thousand rows, where 63 separate bf16
    nodes -- a cast, a product, two gradient products, a reduce and an accumulation add each -- cost twice
    what the twelve fp32 grouped launches do)."""
    return (any_precision or not lp_mode()) and bool(_lib.load().qarig_gemm_grouped_supported(M, N, K, splitk))


def _ptr_table(tensors, G):
    if tensors is None:
        return None
    assert len(tensors) == G
    return (_lib.P * G)(*[t.data_ptr() if t is not None else None for t in tensors])


def gemm_grouped(A, B, C, M, N, K, a_kcontig=True, b_kcontig=True, bias=None, residual=None, preact=None,
                 act=0, gradz=None, gact=0, splitk=1, accumulate=False, sum_groups=False, a_rowsum=None):
    """`len(A)` products of one shape in one launch (include/qarig.h qarig_gemm_f32_grouped): lists
    of fp32 tensors per group (A / B entries may repeat), outputs in the tensors of C (one tensor
    when sum_groups).  Operands must be dense row-major with a common row stride."""
    G = len(A)
    assert 1 <= G <= GEMM_MAX_GROUPS and len(B) == G
    require_cuda(*A, *B, *C)
    lda, ldb, ldc = A[0].stride(0), B[0].stride(0), C[0].stride(0)
    for t in (*A, *B, *C, *(bias or ()), *(residual or ()), *(preact or ()), *(gradz or ()), *(a_rowsum or ())):
        assert t.dtype == torch.float32 and t.stride(-1) == 1
    assert all(t.stride(0) == lda for t in A) and all(t.stride(0) == ldb for t in B)
    assert all(t.stride(0) == ldc and t.shape == (M, N) for t in C) and len(C) == (1 if sum_groups else G)
    ld = lambda ts: ts[0].stride(0) if ts else 0   # noqa: E731
    for ts in (residual, preact, gradz):
        if ts:
            assert all(t.stride(0) == ts[0].stride(0) and t.shape == (M, N) for t in ts)
    lib = _lib.load()
    ws, nws = None, 0
    if splitk > 1 or sum_groups or a_rowsum is not None:
        nws = lib.qarig_gemm_grouped_workspace_bytes(G, M, N, splitk, int(sum_groups))
        ws = workspace(nws, A[0].device, "gemm")
        nws = ws.numel()
    if GEMM_EVENTS is not None:
        ev0 = torch.cuda.Event(enable_timing=True)
        ev0.record()
    Ct = list(C) + [C[0]] * (G - len(C))
    check(lib.qarig_gemm_f32_grouped(
        G, _ptr_table(A, G), lda, int(a_kcontig), _ptr_table(B, G), ldb, int(b_kcontig), _ptr_table(Ct, G), ldc,
        M, N, K, _ptr_table(bias, G), _ptr_table(residual, G), ld(residual), _ptr_table(preact, G), ld(preact),
        act, _ptr_table(gradz, G), ld(gradz), gact, splitk, int(accumulate), int(sum_groups),
        _ptr_table(a_rowsum, G), ptr(ws), nws, stream()), "qarig_gemm_f32_grouped")
    if GEMM_EVENTS is not None:
        ev1 = torch.cuda.Event(enable_timing=True)
        ev1.record()
        GEMM_EVENTS.append((2.0 * G * M * N * K, ev0, ev1, "f32g" if lp_mode() else ""))


def colsum(X, out=None, accumulate=False):
    """(N,) column sums of X (M,N) in a fixed order (optionally added into `out`)."""
    require_cuda(X)
    assert X.dim() == 2 and X.stride(1) == 1 and X.dtype == torch.float32
    M, N = X.shape
    if out is None:
        assert not accumulate
        out = torch.empty(N, dtype=torch.float32, device=X.device)
    lib = _lib.load()
    nb = lib.qarig_colsum_workspace_bytes(M, N)
    ws = workspace(nb, X.device, "colsum")
    check(lib.qarig_colsum_f32(ptr(X), X.stride(0), M, N, ptr(out), int(accumulate), ptr(ws),
                               ws.numel(), stream()), "qarig_colsum_f32")
    return out


def auto_splitk(M, N, K):
    """GEMMs with fewer output tiles than CUs (the M = batch*beams rows of autoregressive
    decode, small per-GPU batches) spread their reduction over the chip; the epilogue then
    runs in the reduce pass."""
    tiles = ((M + 127) // 128) * ((N + 127) // 128)
    if tiles >= 192 or K < 256 or K % 64:
        return 1
    s64 = _tile64_splitk(M, N, K)
    if s64:
        return s64
    if tiles < 64:
        return max(1, min(256 // tiles, K // 64))
    return max(1, min(512 // tiles, K // 128))


def _tile64_splitk(M, N, K):
    """Reduction split of a product the library runs on 64 x 64 tiles (qarig_gemm_tile64): none when the tiles
    fill the chip, else the smallest split of whole 16-deep k-tiles, at least 128 deep, that gives >= 256
    workgroups.  0: not a 64-tile shape."""
    if not _lib.load().qarig_gemm_tile64(int(M), int(N), int(K)):
        return 0
    tiles = (M // 64) * (N // 64)
    s = 1
    while tiles * s < 256 and K % (2 * s) == 0 and (K // (2 * s)) % 16 == 0 and K // (2 * s) >= 128:
        s *= 2
    return s


def wgrad_ring_rows(M, N, K):
    """Output rows of a weight gradient (M x N over a reduction of K rows) that run on the 128-tile ring:
    M, or M - M % 128 where the GEMM entry takes its ragged route (qarig_gemm_ragged_tn: the last 1..8
    rows go to the tail kernels) -- the row count a caller picks the reduction split for."""
    if not lp_mode() and _lib.load().qarig_gemm_ragged_tn(int(M), int(N), int(K)):
        return M - M % 128
    return M


def ragged_output_native(M, N, K):
    """A Linear with N = 128 q + r output columns (1 <= r <= 8) over M rows of K features whose forward
    product and weight gradient both take the GEMM entry's ragged routes (include/qarig.h): callers then
    pass the true width instead of zero-padded copies."""
    lib = _lib.load()
    return (not lp_mode() and bool(lib.qarig_gemm_ragged_nt(int(M), int(N), int(K)))
            and bool(lib.qarig_gemm_ragged_tn(int(N), int(K), int(M))))


def pick_splitk(M, N, K):
    """Reduction split for weight-gradient shaped GEMMs (small M x N, long K)."""
    tiles = ((M + 127) // 128) * ((N + 127) // 128)
    if tiles >= 256:
        return 1
    s64 = _tile64_splitk(M, N, K)
    if s64:
        return s64
    if K < 2048:
        # short reductions over few tiles (weight gradients of the position-table layers,
        # K = a few hundred positions): a handful of workgroups would each walk the whole
        # reduction at DMA latency; spread it in 64-deep slices that divide K exactly
        if tiles > 64 or K % 64:
            return 1
        s = K // 64
        while s > 1 and (K % s or (K // s) % 16 or s * tiles > 512):
            s -= 1
        return max(1, s)
    # (a 512 x 512 gradient over 2,048 rows -- 16 tiles -- measured 40 us in 4 slices of 512 rows and
    # 29 us in 8 of 256: with few tiles the slices may be as short as 16 k-tiles; over 16,384 rows the same
    # gradient comes here -- qarig_gemm_tile64 stops at K = 2048 -- and runs 32 slices of 512 in 79 us)
    s = max(1, min(max(1, 512 // tiles), K // (256 if tiles <= 32 else 512), 32))
    # slices that divide K into whole 16-deep tiles keep the launch on the interior kernels
    # (the padded classifier's 640 x 2048 output over K = 16384 asked for 6: 2736-deep slices
    # sent it to the guarded kernel at half the rate)
    while s > 1 and (K % s or (K // s) % 16):
        s -= 1
    return s


# ------------------------------------------------------------ shared small helpers
_flag_cache = {}


def _bad_flag(device):
    """Device int the kernels set when they meet an out-of-range index."""
    key = device.index if device.index is not None else torch.cuda.current_device()
    f = _flag_cache.get(key)
    if f is None:
        f = torch.zeros(1, dtype=torch.int32, device=device)
        _flag_cache[key] = f
    return f


def check_index_flag(device, what):
    """Raises IndexError (what torch's embedding / nll_loss would do) if a kernel
    flagged an out-of-range index.  Synchronises; callers use it where the reference
    already synchronises (loss.item()) or in tests/debug mode."""
    f = _bad_flag(device)
    if int(f.item()) != 0:
        f.zero_()
        raise IndexError(f"{what}: index out of range")


def _i64c(t):
    if t.dtype != torch.int64:
        t = t.long()
    return t if t.is_contiguous() else t.contiguous()


# ---------------------------------------------------------------------- codebook
def patchify(image, patch_dim):
    """(N,C,H,W) -> (N,Seq,D).  reference models/layers.py:8-34"""
    require_cuda(image)
    image = f32c(image)
    N, C, H, W = image.shape
    pH, pW = patch_dim
    if H % pH or W % pW:  # the reference truncates silently (`//`)
        image = image[:, :, :H // pH * pH, :W // pW * pW].contiguous()
        N, C, H, W = image.shape
    out = torch.empty((N, (H // pH) * (W // pW), C * pH * pW), dtype=torch.float32,
                      device=image.device)
    check(_lib.load().qarig_patchify_fwd(ptr(image), N, C, H, W, pH, pW, ptr(out), stream()),
          "qarig_patchify_fwd")
    return out


def unpatchify(patches, image_dim, patch_dim):
    """(N,Seq,D) -> (N,C,H,W).  reference models/layers.py:37-71"""
    require_cuda(patches)
    patches = f32c(patches)
    H, W = image_dim
    pH, pW = patch_dim
    N, Seq, D = patches.shape
    C = D // (pH * pW)
    assert Seq == (H // pH) * (W // pW) and H % pH == 0 and W % pW == 0
    out = torch.empty((N, C, H, W), dtype=torch.float32, device=patches.device)
    check(_lib.load().qarig_unpatchify_fwd(ptr(patches), N, C, H, W, pH, pW, ptr(out), stream()),
          "qarig_unpatchify_fwd")
    return out


def codebook_gather_image(ids, codebook, image_dim, patch_dim):
    """unpatchify(codebook[ids]).  reference models/Codebook.py:138-154"""
    require_cuda(ids, codebook)
    ids = _i64c(ids)
    codebook = f32c(codebook)
    N, Seq = ids.shape
    H, W = image_dim
    pH, pW = patch_dim
    K, D = codebook.shape
    C = D // (pH * pW)
    assert Seq == (H // pH) * (W // pW)
    out = torch.empty((N, C, H, W), dtype=torch.float32, device=ids.device)
    check(_lib.load().qarig_codebook_gather_image(ptr(ids), N, C, H, W, pH, pW, ptr(codebook), K,
                                                  ptr(out), ptr(_bad_flag(ids.device)), stream()),
          "qarig_codebook_gather_image")
    return out


def gather_rows(ids, table):
    require_cuda(ids, table)
    ids = _i64c(ids).reshape(-1)
    table = f32c(table)
    K, D = table.shape
    out = torch.empty((ids.numel(), D), dtype=torch.float32, device=table.device)
    check(_lib.load().qarig_gather_rows(ptr(ids), ids.numel(), D, K, ptr(table), ptr(out),
                                        ptr(_bad_flag(table.device)), stream()), "qarig_gather_rows")
    return out


def som_weights(bmu_idx, K, two_var):
    require_cuda(bmu_idx)
    bmu_idx = _i64c(bmu_idx).reshape(-1)
    g = torch.empty((bmu_idx.numel(), K), dtype=torch.float32, device=bmu_idx.device)
    check(_lib.load().qarig_som_weights_fwd(ptr(bmu_idx), bmu_idx.numel(), K, float(two_var), ptr(g),
                                            stream()), "qarig_som_weights_fwd")
    return g


def som_reach(two_var):
    """Index distance beyond which exp(-d^2 / two_var) < 2^-40: what som_band drops."""
    import math
    return int(math.ceil(math.sqrt(40.0 * math.log(2.0) * float(two_var))))


def som_band(table, two_var, reach=None):
    """out[j] = sum_{|j-b| <= reach} exp(-(j-b)^2 / two_var) table[b] (reference Codebook.py:112-130
    folded onto the code axis: see csrc/codebook.hip som_band_kernel)."""
    require_cuda(table)
    table = f32c(table)
    K, D = table.shape
    out = torch.empty_like(table)
    reach = som_reach(two_var) if reach is None else int(reach)
    check(_lib.load().qarig_som_band(ptr(table), K, D, float(two_var), min(reach, K), ptr(out), stream()),
          "qarig_som_band")
    return out


# ------------------------------------------------------------------- transformer
_freq_cache = {}


def pos_frequencies(D, device):
    """exp(arange(D/2) * -ln(1e4)/(D/2-1)) computed on the host with the same torch
    ops as the reference (layers.py:84-91), cached per (D, device)."""
    import math
    key = (D, str(device))
    f = _freq_cache.get(key)
    if f is None:
        half = D // 2
        c = math.log(10_000) / (half - 1)
        f = torch.exp(torch.arange(half, dtype=torch.float32) * -c).to(device)
        _freq_cache[key] = f
    return f


def posemb(pos, D):
    """get_positional_embeddings(D, pos) -> (len(pos), D).  pos: int or float tensor."""
    require_cuda(pos)
    pos = pos.reshape(-1).to(torch.float32).contiguous()
    out = torch.empty((pos.numel(), D), dtype=torch.float32, device=pos.device)
    check(_lib.load().qarig_posemb_fwd(ptr(pos), pos.numel(), D, ptr(pos_frequencies(D, pos.device)),
                                       ptr(out), stream()), "qarig_posemb_fwd")
    return out


TOKEN_NOISE_STREAMS = 2        # 0: the decoder's hr tokens, 1: the encoder's lr tokens (csrc/dropout_philox.h)


def _token_noise_args(threshold, neighbour_range, key, what):
    threshold, neighbour_range = int(threshold), int(neighbour_range)
    if not 1 <= threshold <= DROPOUT_MAX_THRESHOLD:
        raise ValueError(f"{what}: threshold must lie in [1, {DROPOUT_MAX_THRESHOLD}], got {threshold}")
    if neighbour_range < 0:
        raise ValueError(f"{what}: the neighbour range must be >= 0 (0 = the whole codebook), got {neighbour_range}")
    if key.dtype != torch.int32 or key.numel() != 4 or not key.is_contiguous():
        raise TypeError(f"{what}: key is a contiguous int32 tensor of 4 words {{seed_lo, seed_hi, step, rank}}")
    return threshold, neighbour_range


def token_noise(ids, k, threshold, neighbour_range, stream_id, key, out=None):
    """Token noise over a whole (N,S) int64 tensor (include/qarig.h qarig_token_noise): token (n, j) is replaced with
    probability threshold / 65536 by a draw from the whole codebook [0, k) (neighbour_range 0) or from the ids within
    neighbour_range of its own, a pure function of (key = device int32[4] {seed_lo, seed_hi, step, rank}, stream_id,
    n, j).  out: None (a new tensor) or ids itself (in place)."""
    require_cuda(ids, key, out)
    if ids.dtype != torch.int64 or ids.dim() != 2 or not ids.is_contiguous():
        raise TypeError("token_noise: ids must be a contiguous int64 (N,S) tensor")
    threshold, neighbour_range = _token_noise_args(threshold, neighbour_range, key, "token_noise")
    y = torch.empty_like(ids) if out is None else out
    if y.dtype != torch.int64 or y.shape != ids.shape or not y.is_contiguous():
        raise TypeError("token_noise: out must be a contiguous int64 tensor of ids' shape")
    N, S = ids.shape
    check(_lib.load().qarig_token_noise(ptr(ids), ptr(y), N, S, int(k), threshold, neighbour_range, int(stream_id),
                                        ptr(key), stream()), "qarig_token_noise")
    return y


def assemble_tokens(lr_idx, hr_idx, base, k_lr, k_hr, offs=None, window=None, noise=None):
    """(hr_in, hr_tg, pos) int64 (N,W) from the BMU indices: token assembly + window slicing of
    the training loop (reference train_quantized_transformer.py:423-484) in one launch.
    offs: int64 (N,) window starts on the device, or None for the whole sequence (pos None).
    noise: None, or (threshold, neighbour_range, key) -- the hr tokens of hr_in pass through the token noise of
    stream 0 (qarig_assemble_tokens_noise replaces the plain entry; hr_tg and pos are unchanged)."""
    require_cuda(hr_idx, lr_idx, offs)
    hr_idx = _i64c(hr_idx)
    N, S_hr = hr_idx.shape
    S_lr = 0
    if base:
        lr_idx = _i64c(lr_idx)
        S_lr = lr_idx.shape[1]
    s_in = (S_lr if base else 1) + S_hr
    W = s_in if offs is None else int(window)
    dev = hr_idx.device
    hr_in = torch.empty((N, W), dtype=torch.int64, device=dev)
    hr_tg = torch.empty((N, W), dtype=torch.int64, device=dev)
    pos = torch.empty((N, W), dtype=torch.int64, device=dev) if offs is not None else None
    if offs is not None:
        offs = _i64c(offs)
        assert offs.shape == (N,)
    if noise is not None:
        require_cuda(noise[2])
        threshold, neighbour_range = _token_noise_args(noise[0], noise[1], noise[2], "assemble_tokens")
        check(_lib.load().qarig_assemble_tokens_noise(ptr(lr_idx) if base else None, S_lr, ptr(hr_idx), S_hr, N,
                                                      int(base), int(k_lr), int(k_hr), ptr(offs), W, ptr(hr_in),
                                                      ptr(hr_tg), ptr(pos), ptr(_bad_flag(dev)), threshold,
                                                      neighbour_range, ptr(noise[2]), stream()),
              "qarig_assemble_tokens_noise")
        return hr_in, hr_tg, pos
    check(_lib.load().qarig_assemble_tokens(ptr(lr_idx) if base else None, S_lr, ptr(hr_idx), S_hr, N,
                                            int(base), int(k_lr), int(k_hr), ptr(offs), W, ptr(hr_in),
                                            ptr(hr_tg), ptr(pos), ptr(_bad_flag(dev)), stream()),
          "qarig_assemble_tokens")
    return hr_in, hr_tg, pos


def embedding_fwd(ids, table, pe=None):
    """table[ids] (+ pe[s]) -> (N,S,D)."""
    require_cuda(ids, table, pe)
    ids = _i64c(ids)
    N, S = ids.shape
    V, D = table.shape
    out = torch.empty((N, S, D), dtype=torch.float32, device=table.device)
    check(_lib.load().qarig_embedding_fwd(ptr(ids), N * S, S, D, V, ptr(table), ptr(pe), ptr(out),
                                          ptr(_bad_flag(table.device)), stream()),
          "qarig_embedding_fwd")
    return out


def embedding_bwd(ids, dy, V):
    ids = _i64c(ids).reshape(-1)
    dy = f32c(dy).reshape(ids.numel(), -1)
    D = dy.shape[1]
    out = torch.empty((V, D), dtype=torch.float32, device=dy.device)
    check(_lib.load().qarig_embedding_bwd(ptr(ids), ids.numel(), D, V, ptr(dy), ptr(out), stream()),
          "qarig_embedding_bwd")
    return out


def layernorm_fwd(x2d, gamma=None, beta=None, scale=None, shift=None, eps=1e-5, mod_idx=None):
    """mod_idx (int32 (M,)): scale/shift are (P,D) position tables read at row mod_idx[token]."""
    M, D = x2d.shape
    y = torch.empty_like(x2d)
    mean = torch.empty(M, dtype=torch.float32, device=x2d.device)
    rstd = torch.empty(M, dtype=torch.float32, device=x2d.device)
    if mod_idx is not None:
        assert mod_idx.dtype == torch.int32 and mod_idx.shape == (M,) and mod_idx.is_contiguous()
    check(_lib.load().qarig_layernorm_fwd(ptr(x2d), M, D, eps, ptr(gamma), ptr(beta), ptr(scale),
                                          ptr(shift), ptr(mod_idx), ptr(y), ptr(mean), ptr(rstd),
                                          stream()), "qarig_layernorm_fwd")
    return y, mean, rstd


def layernorm_bwd(dy, x2d, mean, rstd, gamma=None, scale=None, want_dy_xhat=False, mod_idx=None,
                  dx_add=None):
    """dx_add (M,D): the skip connection's gradient of the same x, added into dx by the kernel."""
    M, D = x2d.shape
    dx = torch.empty_like(x2d)
    dyx = torch.empty_like(x2d) if want_dy_xhat else None
    if dx_add is not None:
        assert dx_add.shape == x2d.shape and dx_add.dtype == torch.float32 and dx_add.is_contiguous()
    check(_lib.load().qarig_layernorm_bwd(ptr(dy), ptr(x2d), ptr(mean), ptr(rstd), ptr(gamma),
                                          ptr(scale), ptr(mod_idx), M, D, ptr(dx), ptr(dyx), ptr(dx_add),
                                          stream()), "qarig_layernorm_bwd")
    return dx, dyx


def rowmap_build(idx, P):
    """(offsets (P+1,), rows (M,)) int32: rows[offsets[p]:offsets[p+1]] = ascending tokens with
    idx == p.  Out-of-range indices set the device index flag (see check_index_flag)."""
    require_cuda(idx)
    assert idx.dtype == torch.int32 and idx.dim() == 1 and idx.is_contiguous()
    M = idx.numel()
    counts = torch.empty(P, dtype=torch.int32, device=idx.device)
    offsets = torch.empty(P + 1, dtype=torch.int32, device=idx.device)
    rows = torch.empty(M, dtype=torch.int32, device=idx.device)
    check(_lib.load().qarig_rowmap_build(ptr(idx), M, P, ptr(counts), ptr(offsets), ptr(rows),
                                         ptr(_bad_flag(idx.device)), stream()), "qarig_rowmap_build")
    return offsets, rows


def segment_sum(src, offsets, rows):
    """(P,D) sums of the rows of src (M,D) that the row map assigns to each table row."""
    P = offsets.numel() - 1
    M, D = src.shape
    assert src.is_contiguous() and rows.numel() == M
    out = torch.empty((P, D), dtype=torch.float32, device=src.device)
    check(_lib.load().qarig_segment_sum(ptr(src), ptr(offsets), ptr(rows), P, D, ptr(out), stream()),
          "qarig_segment_sum")
    return out


def mul_rows_fwd(a, tab, idx):
    M, D = a.shape
    y = torch.empty_like(a)
    check(_lib.load().qarig_mul_rows_fwd(ptr(a), ptr(tab), ptr(idx), ptr(y), M, D, stream()),
          "qarig_mul_rows_fwd")
    return y


def mul_rows_bwd(dy, a, tab, idx):
    M, D = a.shape
    da = torch.empty_like(a)
    db = torch.empty_like(a)
    check(_lib.load().qarig_mul_rows_bwd(ptr(dy), ptr(a), ptr(tab), ptr(idx), ptr(da), ptr(db), M, D,
                                         stream()), "qarig_mul_rows_bwd")
    return da, db


# Backward of the table consumers with the table sums inside (csrc/condtable.hip): one workgroup per table
# position.  Taken when the tokens per table row, M / P (known on the host; the used rows are at most P, so the
# mean per used row is no smaller), reach this value: measured faster than the two-step path at every M / P from
# 1.8 (2,048 tokens over 1,152 rows) to 42.7, never measured on sparser row maps, where most of a workgroup's 8
# waves find no token (profiles/r18_table_bwd_bench.txt).
TABLE_BWD_MIN_TOKENS_PER_ROW = 2
TABLE_BWD_WIDTHS = (256, 512, 1024)


def table_bwd_fused(M, P, D, *tensors):
    """Whether a table backward of M tokens over P positions takes the fused kernel (else: the per-token
    kernel and segment_sum)."""
    return (D in TABLE_BWD_WIDTHS and M >= TABLE_BWD_MIN_TOKENS_PER_ROW * P
            and all(t is None or t.data_ptr() % 16 == 0 for t in tensors))


def layernorm_bwd_table(dy, x2d, mean, rstd, scale_tab, offsets, rows, dx_add=None):
    """(dx, dscale, dshift): layernorm_bwd(scale=scale_tab, mod_idx=idx, want_dy_xhat=True) and the two
    segment_sum launches over its results in one kernel, bit-identical to them."""
    M, D = x2d.shape
    P = offsets.numel() - 1
    assert dy.shape == x2d.shape and dy.is_contiguous() and x2d.is_contiguous() and rows.numel() == M
    assert scale_tab.shape == (P, D) and scale_tab.is_contiguous()
    if dx_add is not None:
        assert dx_add.shape == x2d.shape and dx_add.dtype == torch.float32 and dx_add.is_contiguous()
    dx = torch.empty_like(x2d)
    dscale = torch.empty((P, D), dtype=torch.float32, device=x2d.device)
    dshift = torch.empty((P, D), dtype=torch.float32, device=x2d.device)
    check(_lib.load().qarig_layernorm_bwd_table(ptr(dy), ptr(x2d), ptr(mean), ptr(rstd), ptr(scale_tab),
                                                ptr(offsets), ptr(rows), M, P, D, ptr(dx), ptr(dx_add),
                                                ptr(dscale), ptr(dshift), stream()), "qarig_layernorm_bwd_table")
    return dx, dscale, dshift


def mul_rows_bwd_table(dy, a, tab, offsets, rows):
    """(da, dg): mul_rows_bwd and the segment_sum of its per-token products in one kernel, bit-identical."""
    M, D = a.shape
    P = offsets.numel() - 1
    assert dy.shape == a.shape and dy.is_contiguous() and a.is_contiguous() and rows.numel() == M
    assert tab.shape == (P, D) and tab.is_contiguous()
    da = torch.empty_like(a)
    dg = torch.empty((P, D), dtype=torch.float32, device=a.device)
    check(_lib.load().qarig_mul_rows_bwd_table(ptr(dy), ptr(a), ptr(tab), ptr(offsets), ptr(rows), M, P, D,
                                               ptr(da), ptr(dg), stream()), "qarig_mul_rows_bwd_table")
    return da, dg


def slab_reduce(slabs, out, M, N, accumulate=False, rs_part=None, rs_out=None):
    """out[:M, :N] (+)= slabs (nslab, M, N) summed over the slabs in ascending order; with rs_part (nslab, M):
    rs_out[:M] (+)= its sum too, in the same launch -- the reductions behind a split-K gemm()."""
    nslab = slabs.shape[0]
    assert slabs.is_contiguous() and slabs.dtype == torch.float32 and slabs.shape[1:] == (M, N)
    assert out.dtype == torch.float32 and out.stride(1) == 1 and out.shape[0] >= M and out.shape[1] >= N
    if rs_part is not None:
        assert rs_part.is_contiguous() and rs_part.shape == (nslab, M) and rs_out.is_contiguous()
    check(_lib.load().qarig_slab_reduce_rowsum_f32(ptr(slabs), ptr(out), out.stride(0), M, N, nslab,
                                                   int(accumulate), ptr(rs_part), ptr(rs_out), stream()),
          "qarig_slab_reduce_rowsum_f32")
    return out


ATTENTION_HEAD_DIMS = (4, 8, 16, 32, 64, 128)   # csrc/attention.hip instantiations; 128: csrc/attention_wide.hip
# Head dims cached generation takes by default: decode_attention_kernel's instantiations and 128 (the grouped kernel's
# full bucket).  The other multiples of 4 up to 124 run on the grouped kernel too, opt-in (DECODE_PADDED_HEAD_DIMS:
# the dims the training path zero-pads; sampling.CACHE_PADDED_HEADS).
DECODE_HEAD_DIMS = (4, 8, 16, 32, 64, 128)
DECODE_PADDED_HEAD_DIMS = tuple(d for d in range(4, 128, 4) if d not in DECODE_HEAD_DIMS)


def attention_head_dim(d):
    """The kernel head dim that serves a model head dim d: d itself, or the next instantiated one (the
    caller zero-pads every head: extra zero columns add nothing to q.k and yield zero output columns),
    or None above the widest."""
    for hd in ATTENTION_HEAD_DIMS:
        if hd >= d:
            return hd
    return None


def _attention_dropout_args(dropout):
    """(threshold, scale, site, key pointer) of attention_fwd / attention_bwd's dropout = (T, s, site, key buffer):
    the checks that need the tensor; the entry point refuses the rest."""
    threshold, scale, site, key = dropout
    require_cuda(key)
    if key.dtype != torch.int32 or key.numel() != 4 or not key.is_contiguous():
        raise TypeError("attention dropout: key is a contiguous int32 tensor of 4 words {seed_lo, seed_hi, step, rank}")
    threshold, site = int(threshold), int(site)
    if not 0 <= threshold < 2 ** 32 or not 0 <= site < 2 ** 32:
        raise ValueError(f"attention dropout: threshold and site must fit 32 bits, got {threshold}, {site}")
    return threshold, float(scale), site, ptr(key)


def attention_fwd(q, k, v, heads, causal, scale_dim=None, dropout=None):
    """scale_dim: the model's head dim when the tensors carry zero-padded heads (softmax scale 1/sqrt(scale_dim)).
    dropout: None, or (T, s, site, key buffer) -- attention-probability dropout, include/qarig.h
    qarig_attention_dropout_fwd."""
    N, Sq, D = q.shape
    Sk = k.shape[1]
    d = D // heads
    o = torch.empty_like(q)
    lse = torch.empty((N, heads, Sq), dtype=torch.float32, device=q.device)
    lib = _lib.load()
    if dropout is not None:
        fn = lib.qarig_attention_dropout_lp_fwd if lp_mode() else lib.qarig_attention_dropout_fwd
        check(fn(ptr(q), ptr(k), ptr(v), N, Sq, Sk, heads, d, int(causal), float((scale_dim or d) ** 0.5), ptr(o),
                 ptr(lse), stream(), *_attention_dropout_args(dropout)), "qarig_attention_dropout_fwd")
        return o, lse
    fn = lib.qarig_attention_lp_fwd if lp_mode() else lib.qarig_attention_fwd
    check(fn(ptr(q), ptr(k), ptr(v), N, Sq, Sk, heads, d, int(causal), float((scale_dim or d) ** 0.5), ptr(o),
             ptr(lse), stream()), "qarig_attention_fwd")
    return o, lse


def attention_decode(q, k_new, v_new, kcache, vcache, length, heads, len_dev=None, o_mul=None, out=None):
    """One decode step: q (B,D) against cache rows [0,length) (+ the appended new row).
    kcache/vcache: row-major (B, max_len, D) views with unit row stride D (batch stride free), or
    head-major (B, H, max_len, d) -- DecodeCache's layout.  o_mul: (B, D), or one (D,) row for every sequence.
    out: optional contiguous (B, D) buffer for the result."""
    B, D = q.shape
    d = D // heads
    assert kcache.shape == vcache.shape and kcache.shape[0] == B and vcache.stride() == kcache.stride()
    if kcache.dim() == 4:
        assert kcache.shape[1] == heads and kcache.shape[3] == d and kcache.stride(3) == 1 and kcache.stride(2) == d
        max_len, hstride, rstride = kcache.shape[2], kcache.stride(1), d
    else:
        assert kcache.shape[2] == D and kcache.stride(2) == 1 and kcache.stride(1) == D
        max_len, hstride, rstride = kcache.shape[1], d, D
    assert q.is_contiguous()
    o = out if out is not None else torch.empty_like(q)
    assert o.shape == q.shape and o.is_contiguous() and o.dtype == q.dtype
    ldmul = 0
    if o_mul is not None:
        assert o_mul.shape in (q.shape, (D,)) and o_mul.is_contiguous()
        ldmul = D if o_mul.dim() == 2 else 0
    check(_lib.load().qarig_decode_attention(
        ptr(q), ptr(k_new) if k_new is not None else None,
        ptr(v_new) if v_new is not None else None, ptr(kcache), ptr(vcache), B, heads, d,
        int(length), ptr(len_dev) if len_dev is not None else None, max_len,
        kcache.stride(0), hstride, rstride, float(d ** 0.5), ptr(o_mul), ldmul, ptr(o), stream()),
        "qarig_decode_attention")
    return o


def decode_attention_keys_per_pass(d):
    """Keys a wave of the cache attention kernel covers per pass of its loop at head dim d; 0: d unsupported."""
    return int(_lib.load().qarig_decode_attention_keys_per_pass(int(d)))


DECODE_CTL_WORDS = 8          # include/qarig.h QARIG_DECODE_CTL_WORDS: [0] len, [1] chunk start, [2] draws, [3] candidate


def decode_embed(ids, table, pe, ctl=None, length=0, proj_table=None, proj_row=None):
    """x[b] = table[ids[b]] + pe[len] (len = ctl[0], or `length` without ctl) and proj_row <- row len of
    proj_table (max_len, PD), the stage's per-position projections of `cond`.  Returns x (B, D)."""
    require_cuda(ids, table, pe, ctl, proj_table, proj_row)
    ids = _i64c(ids).reshape(-1)
    B, (V, D) = ids.numel(), table.shape
    assert table.is_contiguous() and table.dtype == torch.float32
    max_len = pe.shape[0] if pe is not None else (proj_table.shape[0] if proj_table is not None else int(length) + 1)
    assert pe is None or (pe.shape == (max_len, D) and pe.is_contiguous())
    pd = 0
    if proj_table is not None:
        assert proj_table.dim() == 2 and proj_table.shape[0] == max_len and proj_table.is_contiguous()
        pd = proj_table.shape[1]
        assert proj_row is not None and proj_row.numel() == pd and proj_row.is_contiguous()
    assert ctl is None or (ctl.dtype == torch.int32 and ctl.numel() >= DECODE_CTL_WORDS)
    x = torch.empty((B, D), dtype=torch.float32, device=table.device)
    check(_lib.load().qarig_decode_embed(ptr(ids), B, D, V, ptr(table), ptr(pe), ptr(ctl), int(length), max_len,
                                         ptr(proj_table), pd, ptr(x), ptr(proj_row), ptr(_bad_flag(table.device)),
                                         stream()), "qarig_decode_embed")
    return x


def check_sample_filter(top_k, top_p):
    """(top_k, top_p) as (int, float), or ValueError: top_k an integer >= 0 (0: off), top_p in (0, 1] (1: off)."""
    import operator
    try:
        k = operator.index(top_k)
    except TypeError:
        raise ValueError(f"top_k must be an integer >= 0 (0: off), got {top_k!r}") from None
    p = float(top_p)
    if k < 0:
        raise ValueError(f"top_k must be an integer >= 0 (0: off), got {top_k!r}")
    if not (0.0 < p <= 1.0):        # NaN fails both comparisons
        raise ValueError(f"top_p must be in (0, 1] (1: off), got {top_p!r}")
    return min(k, 2 ** 31 - 1), p


def decode_sample(logits, temperature, end_token, generate_mode, shift, uniforms, ctl, slot, beam_width, ids,
                  chunk, comb, forced=None, probs_log=None, inc_len=False, beams=0, top_k=0, top_p=1.0):
    """One draw per row of logits (B, V): see include/qarig.h qarig_decode_sample.  beams > 0: candidate-major
    draw numbering, uniforms / forced / probs_log have B // beams columns.  top_k > 0 or top_p < 1: the row is
    filtered first (qarig_decode_sample_filtered); both off: the unfiltered kernel, as without the keywords."""
    top_k, top_p = check_sample_filter(top_k, top_p)
    require_cuda(logits, uniforms, ctl, ids, chunk, comb, forced, probs_log)
    B, V = logits.shape
    max_draws = uniforms.shape[0]
    cols = B // beams if beams else B
    assert logits.stride(1) == 1 and uniforms.shape == (max_draws, cols) and uniforms.is_contiguous()
    assert ids.dtype == chunk.dtype == torch.int64 and ids.numel() == B and chunk.shape == (B, beam_width)
    assert comb.shape == (B,) and comb.dtype == torch.float32 and ctl.dtype == torch.int32
    assert forced is None or (forced.shape == (max_draws, cols) and forced.dtype == torch.int64 and forced.is_contiguous())
    assert probs_log is None or (probs_log.shape == (max_draws, cols, V) and probs_log.is_contiguous())
    if top_k > 0 or top_p < 1.0:
        check(_lib.load().qarig_decode_sample_filtered(
            ptr(logits), logits.stride(0), B, V, float(temperature), int(end_token), int(bool(generate_mode)),
            int(shift), ptr(uniforms), ptr(forced), ptr(ctl), int(slot), int(beam_width), max_draws,
            int(bool(inc_len)), int(beams), ptr(ids), ptr(chunk), ptr(comb), ptr(probs_log), top_k, top_p, stream()),
            "qarig_decode_sample_filtered")
        return
    check(_lib.load().qarig_decode_sample(ptr(logits), logits.stride(0), B, V, float(temperature), int(end_token),
                                          int(bool(generate_mode)), int(shift), ptr(uniforms), ptr(forced), ptr(ctl),
                                          int(slot), int(beam_width), max_draws, int(bool(inc_len)), int(beams),
                                          ptr(ids), ptr(chunk), ptr(comb), ptr(probs_log), stream()),
          "qarig_decode_sample")


def decode_decide(ctl, N, NB, beam_width, comb, chunk, best_p, best_chunk, take, draws=None):
    """draws: draw rows the candidate set consumed (default beam_width: one candidate chunk per row)."""
    require_cuda(ctl, comb, chunk, best_p, best_chunk, take)
    assert comb.numel() == N * NB and chunk.shape == (N * NB, beam_width) and best_chunk.shape == (N, beam_width)
    assert best_p.numel() == N and take.numel() == N and take.dtype == torch.int32
    check(_lib.load().qarig_decode_decide(ptr(ctl), N, NB, beam_width, int(beam_width if draws is None else draws),
                                          ptr(comb), ptr(chunk), ptr(best_p), ptr(best_chunk), ptr(take), stream()),
          "qarig_decode_decide")


def decode_rows(ctl, kv, staged, take, N, NB, restore):
    """kv (layers, 2, N * NB, H, max_len, d) <-> staged (layers, 2, N, H, R, d) at rows [ctl[1], ctl[1] + R)."""
    require_cuda(ctl, kv, staged, take)
    layers, two, B, H, max_len, d = kv.shape
    R = staged.shape[4]
    assert two == 2 and B == N * NB and staged.shape == (layers, 2, N, H, R, d)
    assert kv.is_contiguous() and staged.is_contiguous()
    check(_lib.load().qarig_decode_rows(ptr(ctl), ptr(kv), ptr(staged), ptr(take), layers * 2, N, NB, H, R, d,
                                        max_len, int(bool(restore)), stream()), "qarig_decode_rows")


def decode_cache_fill(k, v, kv_layer, beams):
    """Rows [0, P1) of one layer of the head-major cache, kv_layer (2, images * beams, H, max_len, d), from
    token-major k / v (images, P1, H * d) with a row and an image stride of their own (unit channel stride):
    every candidate row of an image gets the image's rows.  One launch for both halves."""
    require_cuda(k, v, kv_layer)
    two, B, H, max_len, d = kv_layer.shape
    images, P1, D = k.shape
    beams = int(beams)
    assert two == 2 and B == images * beams and D == H * d and kv_layer.is_contiguous()
    assert k.dtype == v.dtype == kv_layer.dtype == torch.float32
    assert v.shape == k.shape and v.stride() == k.stride() and k.stride(2) == 1
    if P1 > max_len:
        raise IndexError(f"decode_cache_fill: {P1} prefix rows for a cache of {max_len}")
    check(_lib.load().qarig_decode_cache_fill(ptr(k), ptr(v), k.stride(1), k.stride(0), ptr(kv_layer), images, beams,
                                              H, d, P1, max_len, stream()), "qarig_decode_cache_fill")


def decode_commit(ctl, N, NB, beam_width, best_chunk, tokens, ids):
    require_cuda(ctl, best_chunk, tokens, ids)
    assert tokens.dtype == torch.int64 and tokens.dim() == 2 and tokens.shape[0] == N and tokens.stride(1) == 1
    assert ids.numel() == N * NB and best_chunk.shape == (N, beam_width)
    check(_lib.load().qarig_decode_commit(ptr(ctl), N, NB, beam_width, ptr(best_chunk), ptr(tokens),
                                          tokens.stride(0), ptr(ids), stream()), "qarig_decode_commit")


def decode_advance(ctl, beam_width):
    require_cuda(ctl)
    check(_lib.load().qarig_decode_advance(ptr(ctl), int(beam_width), stream()), "qarig_decode_advance")


CTL_RING = 5                  # include/qarig.h: ctl[5], tokens in the window step's token ring


def window_step_supported(R, window, D, heads):
    return bool(_lib.load().qarig_window_step_supported(int(R), int(window), int(D), int(heads)))


def window_assemble(ring, ctl, table, pe, W1, pad, x, rowmap=None, last_map=None, P=0, pos_off=0):
    """The slid window in front of ring length ctl[5] into x (R, W1 + pad, D) (+ the rows of the conditioning
    table into rowmap (R * (W1 + pad),) and that of each last real token into last_map (R,)); see
    include/qarig.h qarig_window_assemble."""
    require_cuda(ring, ctl, table, pe, x, rowmap, last_map)
    R, ldr = ring.shape
    Wp = int(W1) + int(bool(pad))
    V, D = table.shape
    assert ring.dtype == torch.int64 and ring.stride(1) == 1 and ctl.dtype == torch.int32 and ctl.numel() > CTL_RING
    assert table.is_contiguous() and pe.is_contiguous() and pe.shape[0] >= Wp and pe.shape[1] == D
    assert x.shape == (R, Wp, D) and x.is_contiguous() and x.dtype == torch.float32
    for t, n in ((rowmap, R * Wp), (last_map, R)):
        assert t is None or (t.dtype == torch.int32 and t.numel() == n and t.is_contiguous())
    check(_lib.load().qarig_window_assemble(ptr(ring), ring.stride(0), ptr(ctl), R, int(W1), Wp, D, V, ptr(table),
                                            ptr(pe), int(P), int(pos_off), ptr(x), ptr(rowmap), ptr(last_map),
                                            ptr(_bad_flag(table.device)), stream()), "qarig_window_assemble")


def window_attention(q, k, v, n_keys, heads, o_mul=None, out=None):
    """q (R, D): the last real token of each window; k / v (R, rows, D) token-major (rows >= n_keys; rows past
    n_keys -- the pad row -- are not attended).  Returns o (R, D)."""
    require_cuda(q, k, v, o_mul, out)
    R, D = q.shape
    rows = k.shape[1]
    assert k.shape == v.shape and k.shape[0] == R and k.shape[2] == D and k.stride() == v.stride()
    assert k.stride(2) == 1 and k.stride(1) == D and q.is_contiguous()
    o = out if out is not None else torch.empty_like(q)
    assert o.shape == q.shape and o.is_contiguous()
    ldmul = 0
    if o_mul is not None:
        assert o_mul.shape in (q.shape, (D,)) and o_mul.is_contiguous()
        ldmul = D if o_mul.dim() == 2 else 0
    check(_lib.load().qarig_window_attention(ptr(q), ptr(k), ptr(v), R, int(heads), D // int(heads), int(n_keys),
                                             rows, k.stride(0), ptr(o_mul), ldmul, ptr(o), stream()),
          "qarig_window_attention")
    return o


def window_append(ctl, ring, ids):
    """ring[b][ctl[5]] = ids[b], ctl[5] += 1."""
    require_cuda(ctl, ring, ids)
    B, ldr = ring.shape
    assert ring.dtype == torch.int64 and ring.stride(1) == 1 and ctl.dtype == torch.int32 and ctl.numel() > CTL_RING
    assert ids.dtype == torch.int64 and ids.numel() == B and ids.is_contiguous()
    check(_lib.load().qarig_window_append(ptr(ctl), ptr(ids), ptr(ring), B, ring.stride(0),
                                          ptr(_bad_flag(ring.device)), stream()), "qarig_window_append")


def attention_bwd(q, k, v, o, dO, lse, heads, causal, scale_dim=None, dropout=None):
    """dropout: what attention_fwd took for the same (q, k, v): the backward passes regenerate its mask."""
    N, Sq, D = q.shape
    Sk = k.shape[1]
    d = D // heads
    dq = torch.empty_like(q)
    dk = torch.empty_like(k)
    dv = torch.empty_like(v)
    delta = torch.empty_like(lse)
    lib = _lib.load()
    if dropout is not None:
        fn = lib.qarig_attention_dropout_lp_bwd if lp_mode() else lib.qarig_attention_dropout_bwd
        check(fn(ptr(q), ptr(k), ptr(v), ptr(o), ptr(dO), ptr(lse), N, Sq, Sk, heads, d, int(causal),
                 float((scale_dim or d) ** 0.5), ptr(dq), ptr(dk), ptr(dv), ptr(delta), stream(),
                 *_attention_dropout_args(dropout)), "qarig_attention_dropout_bwd")
        return dq, dk, dv
    fn = lib.qarig_attention_lp_bwd if lp_mode() else lib.qarig_attention_bwd
    check(fn(ptr(q), ptr(k), ptr(v), ptr(o), ptr(dO), ptr(lse), N, Sq, Sk, heads, d, int(causal),
             float((scale_dim or d) ** 0.5), ptr(dq), ptr(dk), ptr(dv), ptr(delta), stream()), "qarig_attention_bwd")
    return dq, dk, dv


def check_ce_regularisers(label_smoothing, z_loss):
    """(label_smoothing, z_loss) as floats, or ValueError: what the cross-entropy entries accept."""
    eps, zeta = float(label_smoothing), float(z_loss)
    if not 0.0 <= eps < 1.0:
        raise ValueError(f"label_smoothing must lie in [0, 1), got {label_smoothing}")
    if not (0.0 <= zeta < float("inf")):
        raise ValueError(f"z_loss must be finite and >= 0, got {z_loss}")
    return eps, zeta


NEIGHBOUR_RANGE_MAX = 31        # a window of 2 R + 1 <= 63 columns: one per lane of the row's wave
_NEIGHBOUR_WEIGHTS = {}


def _f32(v):
    """The fp32 value a float argument of the C entry arrives as."""
    import struct
    return struct.unpack("f", struct.pack("f", v))[0]


def neighbour_table(R, sigma):
    """w[d] = exp(-d^2 / (2 sigma^2)), d = 0 .. R, of the INDEX distance on the SOM axis (not of a distance between
    the codes' latents): computed in fp64, rounded once to fp32; w[0] = 1.  A host tensor."""
    d = torch.arange(int(R) + 1, dtype=torch.float64)
    return torch.exp(-(d * d) / (2.0 * float(sigma) ** 2)).to(torch.float32)


def neighbour_weights(R, sigma, device):
    """neighbour_table(R, sigma) on `device`, made once per (device, R, sigma): a captured step holds its address."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (device, int(R), float(sigma))
    w = _NEIGHBOUR_WEIGHTS.get(key)
    if w is None:
        w = _NEIGHBOUR_WEIGHTS[key] = neighbour_table(R, sigma).to(device)
    return w


def check_ce_soft(label_smoothing=0.0, z_loss=0.0, neighbour_smoothing=0.0, neighbour_range=None,
                  neighbour_sigma=None, codes=None, classes=None):
    """(label_smoothing, z_loss, neighbour_smoothing, range, sigma) as qarig_cross_entropy_fused_fwd accepts them, or
    ValueError.  neighbour_smoothing = 0 gives (eps, zeta, 0.0, None, None) and refuses a range or a sigma: they
    would do nothing.  neighbour_smoothing > 0 needs a range in 1 .. 31; sigma defaults to range / 2.  codes (the
    classes on the SOM axis) and classes are checked against each other when both are given."""
    eps, zeta = check_ce_regularisers(label_smoothing, z_loss)
    nu = float(neighbour_smoothing)
    if not 0.0 <= nu < 1.0:
        raise ValueError(f"neighbour_smoothing must lie in [0, 1), got {neighbour_smoothing}")
    if not _f32(_f32(eps) + _f32(nu)) < 1.0:
        raise ValueError(f"label_smoothing + neighbour_smoothing must stay below 1, got {eps} + {nu}")
    if nu == 0.0:
        if neighbour_range is not None or neighbour_sigma is not None:
            raise ValueError("neighbour_range / neighbour_sigma do nothing without neighbour_smoothing > 0")
        return eps, zeta, 0.0, None, None
    if neighbour_range is None:
        raise ValueError("neighbour_smoothing > 0 needs neighbour_range")
    if isinstance(neighbour_range, bool) or int(neighbour_range) != neighbour_range or \
            not 1 <= neighbour_range <= NEIGHBOUR_RANGE_MAX:
        raise ValueError(f"neighbour_range must be an integer in 1 .. {NEIGHBOUR_RANGE_MAX}, got {neighbour_range}")
    R = int(neighbour_range)
    sigma = R / 2.0 if neighbour_sigma is None else float(neighbour_sigma)
    if not 0.0 < sigma < float("inf"):
        raise ValueError(f"neighbour_sigma must be finite and > 0, got {neighbour_sigma}")
    if codes is None:
        raise ValueError("neighbour_smoothing > 0 needs codes, the number of classes on the SOM axis")
    if isinstance(codes, bool) or int(codes) != codes or codes < 1 or (classes is not None and codes > classes):
        raise ValueError(f"codes must be an integer in 1 .. C = {classes}, got {codes}")
    return eps, zeta, nu, R, sigma


def cross_entropy_fwd(logits2d, target, label_smoothing=0.0, z_loss=0.0, neighbour_smoothing=0.0,
                      neighbour_range=None, neighbour_sigma=None, codes=None, ld_grad=None, want_grad=True):
    """Mean cross-entropy of logits (M, C) against int64 targets in the fused launch (include/qarig.h
    qarig_cross_entropy_fused_fwd): F.cross_entropy(logits2d, target, label_smoothing=...) + z_loss *
    mean(logsumexp(logits2d)^2), and with neighbour_smoothing > 0 that much of the target mass on the codes within
    neighbour_range of the target among the leading `codes` classes, by a Gaussian of the index distance with width
    neighbour_sigma (default range / 2), clamped at the ends of the axis and renormalised (check_ce_soft).
    logits2d: dense, or a column slice of a wider buffer (unit column stride, row stride >= C; the columns behind the
    slice are never read).  Returns (pair, dlogits): pair = {mean objective, mean plain nll} as one (2,) tensor, the
    plain loss twice with all three numbers 0; dlogits an (M, ld_grad) buffer (ld_grad >= C, default the logits' row
    stride) holding the gradient of the objective, its columns C .. ld_grad - 1 exact zeros (None unless want_grad)."""
    require_cuda(logits2d, target)
    assert logits2d.dtype == torch.float32 and logits2d.dim() == 2 and logits2d.stride(1) == 1
    assert target.dtype == torch.int64 and target.is_contiguous() and target.numel() == logits2d.shape[0]
    M, C = logits2d.shape
    ld = logits2d.stride(0) if M > 1 else max(C, logits2d.stride(0))
    ld_grad = ld if ld_grad is None else int(ld_grad)
    assert ld >= C and ld_grad >= C
    eps, zeta, nu, R, sigma = check_ce_soft(label_smoothing, z_loss, neighbour_smoothing, neighbour_range,
                                            neighbour_sigma, codes, C)
    w = neighbour_weights(R, sigma, logits2d.device) if nu > 0 else None
    pair = torch.empty(2, dtype=torch.float32, device=logits2d.device)
    dl = torch.empty((M, ld_grad), dtype=torch.float32, device=logits2d.device) if want_grad else None
    rows = torch.empty(2 * M, dtype=torch.float32, device=logits2d.device)
    check(_lib.load().qarig_cross_entropy_fused_fwd(ptr(logits2d), ld, ptr(target), M, C,
                                                    C if codes is None else int(codes), eps, zeta, nu, R or 0, ptr(w),
                                                    ptr(pair), ptr(dl), ld_grad, ptr(rows),
                                                    ptr(_bad_flag(logits2d.device)), stream()),
          "qarig_cross_entropy_fused_fwd")
    return pair, dl


def token_score(logits2d, target, ignore_index=-100):
    """(row_nll fp32 (M,), row_rank int32 (M,)) of logits (M,C) against int64 targets: the negative
    log-likelihood in nats and the number of classes ranked before the target (0: arg-max, ties to the smaller
    index).  Rows whose target is ignore_index give (0, -1); other targets outside [0,C) give the same and set
    the device index flag (check_index_flag)."""
    require_cuda(logits2d, target)
    assert logits2d.dtype == torch.float32 and logits2d.dim() == 2 and logits2d.is_contiguous()
    M, C = logits2d.shape
    target = _i64c(target).reshape(-1)
    assert target.numel() == M
    nll = torch.empty(M, dtype=torch.float32, device=logits2d.device)
    rank = torch.empty(M, dtype=torch.int32, device=logits2d.device)
    check(_lib.load().qarig_token_score(ptr(logits2d), ptr(target), M, C, int(ignore_index), ptr(nll), ptr(rank),
                                        ptr(_bad_flag(logits2d.device)), stream()), "qarig_token_score")
    return nll, rank


def score_reduce(row_nll, row_rank, N, S, pos0, topk, img_nll, pos_nll, pos_cnt, totals):
    """Adds the (N,S) rows of one token_score call into the accumulators of an evaluation: img_nll fp64 (N,),
    pos_nll fp64 (P,) and pos_cnt int64 (P,) at positions pos0 ... pos0 + S - 1, totals int64 (3,) = {rows
    counted, rank == 0, rank < topk}.  Fixed-order fp64 sums, no atomics: deterministic."""
    require_cuda(row_nll, row_rank, img_nll, pos_nll, pos_cnt, totals)
    assert row_nll.dtype == torch.float32 and row_rank.dtype == torch.int32
    assert row_nll.is_contiguous() and row_rank.is_contiguous() and row_nll.numel() == row_rank.numel() == N * S
    assert img_nll.dtype == pos_nll.dtype == torch.float64 and pos_cnt.dtype == totals.dtype == torch.int64
    for t in (img_nll, pos_nll, pos_cnt, totals):
        assert t.dim() == 1 and t.is_contiguous()
    P = pos_nll.numel()
    assert img_nll.numel() == N and pos_cnt.numel() == P and totals.numel() == 3
    check(_lib.load().qarig_score_reduce(ptr(row_nll), ptr(row_rank), N, S, int(pos0), P, int(topk), ptr(img_nll),
                                         ptr(pos_nll), ptr(pos_cnt), ptr(totals), stream()), "qarig_score_reduce")


def pair_error(a, b):
    """(N,3) fp64 = {sum (a-b)^2, sum |a-b|, max |a-b|} per image of two equally shaped fp32 batches (the first
    axis counts the images).  fp64 throughout, one fixed summation order, independent of the batch an image is in."""
    require_cuda(a, b)
    if a.shape != b.shape or a.dim() < 1 or a.numel() == 0:
        raise ValueError(f"pair_error: shapes {tuple(a.shape)} and {tuple(b.shape)}")
    a, b = f32c(a), f32c(b)
    N = a.shape[0]
    E = a.numel() // N
    lib = _lib.load()
    out = torch.empty((N, 3), dtype=torch.float64, device=a.device)
    ws = _lib.workspace(lib.qarig_pair_error_workspace_bytes(N, E), a.device, tag="recon")
    check(lib.qarig_pair_error(ptr(a), ptr(b), N, E, ptr(out), ptr(ws), ws.numel(), stream()), "qarig_pair_error")
    return out


def gaussian_window(taps, sigma):
    """1-D Gaussian weights exp(-(i - taps // 2)^2 / 2 sigma^2), normalised to sum 1, as Python floats."""
    w = [math.exp(-((i - taps // 2) ** 2) / (2.0 * sigma * sigma)) for i in range(taps)]
    s = math.fsum(w)
    return [v / s for v in w]


def _ssim_args(what, a, b, data_range, sigma, taps, k1, k2, window):
    """The arguments the SSIM entries share: (a, b) fp32 contiguous, the window as a ctypes array of doubles (kept
    alive by the caller until the call returns), taps, c1, c2."""
    require_cuda(a, b)
    if a.shape != b.shape or a.dim() != 4:
        raise ValueError(f"{what}: need two (N,C,H,W) batches, got {tuple(a.shape)} and {tuple(b.shape)}")
    w = [float(v) for v in window] if window is not None else gaussian_window(int(taps), float(sigma))
    taps = len(w)
    win = (ctypes.c_double * max(taps, 1))(*w)
    return f32c(a), f32c(b), win, taps, (k1 * data_range) ** 2, (k2 * data_range) ** 2


def ssim(a, b, data_range=2.0, sigma=1.5, taps=11, k1=0.01, k2=0.03, window=None):
    """(N,) fp64 mean structural similarity of two (N,C,H,W) fp32 batches, per channel over the valid positions
    of a separable window: Gaussian (sigma, taps) unless `window` gives the 1-D weights themselves.  Window
    moments in fp64; c1 = (k1 data_range)^2, c2 = (k2 data_range)^2."""
    a, b, win, taps, c1, c2 = _ssim_args("ssim", a, b, data_range, sigma, taps, k1, k2, window)
    N, C, H, W = a.shape
    lib = _lib.load()
    out = torch.empty(N, dtype=torch.float64, device=a.device)
    ws = _lib.workspace(lib.qarig_ssim_workspace_bytes(N, C, H, W, taps), a.device, tag="recon")
    check(lib.qarig_ssim(ptr(a), ptr(b), N, C, H, W, ctypes.cast(win, ctypes.c_void_p), taps, c1, c2, ptr(out),
                         ptr(ws), ws.numel(), stream()), "qarig_ssim")
    return out


def ssim_fwd_maps(a, b, data_range=2.0, sigma=1.5, taps=11, k1=0.01, k2=0.03, window=None):
    """(out, maps): ops.ssim(a, b, ...) bit for bit, and maps (3,N,C,oh,ow) fp64, the derivatives of every valid
    position's score with respect to the window moments sum w a, sum w a^2 and sum w a b -- what ssim_bwd needs."""
    a, b, win, taps, c1, c2 = _ssim_args("ssim_fwd_maps", a, b, data_range, sigma, taps, k1, k2, window)
    N, C, H, W = a.shape
    lib = _lib.load()
    out = torch.empty(N, dtype=torch.float64, device=a.device)
    # (0 bytes for arguments the entry refuses: it is called all the same, and names what is wrong)
    maps = torch.empty(lib.qarig_ssim_maps_bytes(N, C, H, W, taps) // 8, dtype=torch.float64, device=a.device)
    ws = _lib.workspace(lib.qarig_ssim_workspace_bytes(N, C, H, W, taps), a.device, tag="recon")
    check(lib.qarig_ssim_fwd_maps(ptr(a), ptr(b), N, C, H, W, ctypes.cast(win, ctypes.c_void_p), taps, c1, c2,
                                  ptr(out), ptr(maps), ptr(ws), ws.numel(), stream()), "qarig_ssim_fwd_maps")
    return out, maps.view(3, N, C, H - taps + 1, W - taps + 1)


def ssim_bwd(a, b, maps, g, data_range=2.0, sigma=1.5, taps=11, k1=0.01, k2=0.03, window=None):
    """da (N,C,H,W) fp32: the gradient of sum_n g[n] ssim(a, b)[n] with respect to a, from the maps of
    ssim_fwd_maps on the same arguments; g (N,) fp64 on the device.  Deterministic, image by image."""
    a, b, win, taps, _, _ = _ssim_args("ssim_bwd", a, b, data_range, sigma, taps, k1, k2, window)
    require_cuda(maps, g)
    N, C, H, W = a.shape
    lib = _lib.load()
    if maps.dtype != torch.float64 or not maps.is_contiguous() or maps.numel() * 8 != lib.qarig_ssim_maps_bytes(
            N, C, H, W, taps) or maps.numel() == 0:
        raise ValueError(f"ssim_bwd: maps of {tuple(maps.shape)} {maps.dtype} do not belong to images of "
                         f"{tuple(a.shape)} and a window of {taps} taps")
    if g.dtype != torch.float64 or g.numel() != N:
        raise ValueError(f"ssim_bwd: g must hold {N} fp64 weights, got {tuple(g.shape)} {g.dtype}")
    g = g.contiguous()
    da = torch.empty_like(a)
    check(lib.qarig_ssim_bwd(ptr(a), ptr(b), ptr(maps), ptr(g), N, C, H, W, ctypes.cast(win, ctypes.c_void_p), taps,
                             ptr(da), stream()), "qarig_ssim_bwd")
    return da


def pool_features(z, pool):
    """(N, D) fp64 features of an (N,C,H,W) fp32 batch, D = C (H/pool) (W/pool): the mean of every pool x pool
    block, summed in fp64 in raster order (pool 1: a conversion).  D is at most 1024."""
    require_cuda(z)
    if z.dim() != 4 or z.numel() == 0:
        raise ValueError(f"pool_features: need a non-empty (N,C,H,W) batch, got {tuple(z.shape)}")
    z = f32c(z)
    N, C, H, W = z.shape
    pool = int(pool)
    D = C * (H // pool) * (W // pool) if pool >= 1 else 0
    f = torch.empty((N, max(D, 1)), dtype=torch.float64, device=z.device)
    check(_lib.load().qarig_pool_features(ptr(z), N, C, H, W, pool, ptr(f), stream()), "qarig_pool_features")
    return f


def moments_add(f, state, shift=None):
    """Adds the rows of f (n, D) fp64 into state = (count int64 (1,), sum fp64 (D,), gram fp64 (D,D)), which the
    caller zeroed once: count += n, sum += sum_r a_r, gram += sum_r a_r a_r^T on the upper triangle of 16 x 16
    tiles (diagonal tiles whole; the rest of gram is left alone), a_r = f_r - shift.  fp64 MFMA, one fixed order,
    no atomics: deterministic."""
    count, total, gram = state
    require_cuda(f, count, total, gram, shift)
    if f.dim() != 2 or f.dtype != torch.float64 or f.numel() == 0:
        raise ValueError(f"moments_add: need non-empty (n, D) fp64 features, got {tuple(f.shape)} {f.dtype}")
    f = f.contiguous()
    n, D = f.shape
    assert count.dtype == torch.int64 and count.numel() == 1
    assert total.dtype == gram.dtype == torch.float64 and total.is_contiguous() and gram.is_contiguous()
    assert total.shape == (D,) and gram.shape == (D, D), (tuple(total.shape), tuple(gram.shape), D)
    if shift is not None:
        assert shift.dtype == torch.float64 and shift.shape == (D,) and shift.is_contiguous()
    check(_lib.load().qarig_moments_add(ptr(f), n, D, ptr(shift), ptr(count), ptr(total), ptr(gram), stream()),
          "qarig_moments_add")


def _knn_args(what, q, x, shift, self_offset, k):
    """The checks knn_smallest and ball_count share; returns (q, x, shift, nq, nx, D, workspace)."""
    require_cuda(q, x, shift)
    for name, f in (("q", q), ("x", x)):
        if f.dim() != 2 or f.dtype != torch.float64 or f.numel() == 0:
            raise ValueError(f"{what}: need non-empty (n, D) fp64 rows for {name}, got {tuple(f.shape)} {f.dtype}")
    if q.shape[1] != x.shape[1]:
        raise ValueError(f"{what}: q has {q.shape[1]} features per row, x has {x.shape[1]}")
    q, x = q.contiguous(), x.contiguous()
    (nq, D), nx = q.shape, x.shape[0]
    if shift is not None:
        if shift.dtype != torch.float64 or tuple(shift.shape) != (D,):
            raise ValueError(f"{what}: shift must be ({D},) fp64, got {tuple(shift.shape)} {shift.dtype}")
        shift = shift.contiguous()
    self_offset = int(self_offset)
    if self_offset != -1 and not 0 <= self_offset <= nx - nq:
        raise ValueError(f"{what}: self_offset {self_offset} is neither -1 nor in 0 ... nx - nq = {nx - nq}")
    if nx - (self_offset >= 0) < k:
        raise ValueError(f"{what}: {nx - (self_offset >= 0)} candidates per query, fewer than k = {k}")
    nb = _lib.load().qarig_knn_workspace_bytes(nq, nx, D, k)
    if nb == 0:
        raise ValueError(f"{what}: nq = {nq}, nx = {nx}, D = {D}, k = {k} outside what the kernel supports")
    return q, x, shift, nq, nx, D, torch.empty(nb, dtype=torch.uint8, device=q.device)


def knn_smallest(q, x, k, shift=None, self_offset=-1):
    """(d2 (nq, k) fp64, idx (nq, k) int32): for every row of q (nq, D) fp64 the k smallest squared distances to the
    rows of x (nx, D) fp64, ascending, ties to the lower index, and their x indices.  Distances are taken about
    `shift` ((D,) fp64 or None) in the Gram form on fp64 MFMA (include/qarig.h).  self_offset >= 0: query i is x row
    self_offset + i, which is no candidate.  1 <= k <= 8.  Deterministic; nothing is read back."""
    k = int(k)
    if not 1 <= k <= 8:
        raise ValueError(f"knn_smallest: k = {k}, need 1 ... 8")
    q, x, shift, nq, nx, D, ws = _knn_args("knn_smallest", q, x, shift, self_offset, k)
    d2 = torch.empty((nq, k), dtype=torch.float64, device=q.device)
    idx = torch.empty((nq, k), dtype=torch.int32, device=q.device)
    check(_lib.load().qarig_knn_smallest(ptr(q), nq, ptr(x), nx, D, ptr(shift), k, int(self_offset), ptr(d2),
                                         ptr(idx), ptr(ws), ws.numel(), stream()), "qarig_knn_smallest")
    return d2, idx


def ball_count(q, x, r2, shift=None, self_offset=-1):
    """count (nq,) int32: the number of rows j of x (row self_offset + i excluded when self_offset >= 0) with
    d2(q_i, x_j) <= r2[j], r2 (nx,) fp64 -- the radius belongs to the x row; d2 as in knn_smallest, bit for bit."""
    q, x, shift, nq, nx, D, ws = _knn_args("ball_count", q, x, shift, self_offset, 1)
    require_cuda(r2)
    if r2.dtype != torch.float64 or tuple(r2.shape) != (nx,):
        raise ValueError(f"ball_count: r2 must be ({nx},) fp64, got {tuple(r2.shape)} {r2.dtype}")
    r2 = r2.contiguous()
    count = torch.empty(nq, dtype=torch.int32, device=q.device)
    check(_lib.load().qarig_ball_count(ptr(q), nq, ptr(x), nx, D, ptr(shift), ptr(r2), int(self_offset), ptr(count),
                                       ptr(ws), ws.numel(), stream()), "qarig_ball_count")
    return count


def _adam_asserts(p, shadow, ema=None, decay_mask=None, dev_step=None, dev_floats=None, clip_state=None):
    """What the four Adam wrappers ask of their optional tensors.  dev_floats: the (least, most) floats dev_step may
    hold."""
    n = p.numel()
    assert shadow is None or (shadow.dtype == torch.bfloat16 and shadow.numel() == n)
    assert ema is None or (ema.dtype == torch.float32 and ema.numel() == n and ema.is_contiguous())
    assert decay_mask is None or (decay_mask.dtype == torch.uint8 and decay_mask.is_contiguous()
                                  and decay_mask.is_cuda and decay_mask.numel() == (n + 7) // 8)
    assert dev_step is None or dev_floats is None or dev_floats[0] <= dev_step.numel() <= dev_floats[1]
    assert clip_state is None or (clip_state.dtype == torch.float64 and clip_state.is_cuda
                                  and clip_state.numel() == 4)


def adam_step(p, g, m, v, beta1, beta2, eps, step_size, bc2_sqrt, grad_scale=1.0, dev_step=None, shadow=None):
    """shadow: optional bf16 tensor of p's numel that receives the updated parameters (reduced precision)."""
    _adam_asserts(p, shadow)
    check(_lib.load().qarig_adam_step(ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), beta1, beta2, eps,
                                      step_size, bc2_sqrt, grad_scale, ptr(dev_step), ptr(shadow), stream()),
          "qarig_adam_step")


def adam_ema_step(p, g, m, v, ema, beta1, beta2, eps, step_size, bc2_sqrt, ema_w, grad_scale=1.0, dev_step=None,
                  shadow=None):
    """adam_step that also moves `ema` (fp32, p's numel) towards the updated parameters by weight ema_w.
    dev_step, when given, holds three floats: {step_size, bc2_sqrt, ema_w}."""
    assert ema is not None
    _adam_asserts(p, shadow, ema, dev_step=dev_step, dev_floats=(3, math.inf))
    check(_lib.load().qarig_adam_ema_step(ptr(p), ptr(g), ptr(m), ptr(v), ptr(ema), p.numel(), beta1, beta2, eps,
                                          step_size, bc2_sqrt, ema_w, grad_scale, ptr(dev_step), ptr(shadow),
                                          stream()),
          "qarig_adam_ema_step")


def adamw_step(p, g, m, v, ema, decay_mask, beta1, beta2, eps, step_size, bc2_sqrt, ema_w, decay, grad_scale=1.0,
               dev_step=None, shadow=None):
    """adam_step / adam_ema_step (ema may be None) behind a decoupled weight decay: the elements of the groups of 8
    whose byte in `decay_mask` (uint8, ceil(numel / 8) entries) is non-zero are first moved to fma(-decay, p, p),
    decay = fp32(lr * lambda).  dev_step, when given, holds four floats: {step_size, bc2_sqrt, ema_w, decay}."""
    assert decay_mask is not None
    _adam_asserts(p, shadow, ema, decay_mask, dev_step, (4, 4))
    check(_lib.load().qarig_adamw_step(ptr(p), ptr(g), ptr(m), ptr(v), ptr(ema), ptr(decay_mask), p.numel(), beta1,
                                       beta2, eps, step_size, bc2_sqrt, ema_w, decay, grad_scale, ptr(dev_step),
                                       ptr(shadow), stream()),
          "qarig_adamw_step")


GRAD_NORM_PARTIALS = 2048       # include/qarig.h QARIG_GRAD_NORM_PARTIALS: doubles in grad_clip_coef's scratch buffer


def grad_clip_coef(g, grad_scale, max_norm, partials, state):
    """Global norm of fp32(g * grad_scale) and the clip coefficient fp32(min(1, max_norm / (norm + 1e-6))), left
    on the device: state (4 doubles) receives {norm, coef} and counts skipped (non-finite norm) and clipped steps
    in state[2] and state[3].  partials: GRAD_NORM_PARTIALS doubles of scratch.  Two launches, no read-back."""
    require_cuda(g, partials, state)
    assert g.dtype == torch.float32 and g.is_contiguous()
    assert partials.dtype == torch.float64 and partials.is_contiguous() and partials.numel() >= GRAD_NORM_PARTIALS
    assert state.dtype == torch.float64 and state.is_contiguous() and state.numel() == 4
    check(_lib.load().qarig_grad_clip_coef(ptr(g), g.numel(), grad_scale, max_norm, ptr(partials), ptr(state),
                                           stream()),
          "qarig_grad_clip_coef")


def adam_clip_step(p, g, m, v, ema, decay_mask, beta1, beta2, eps, step_size, bc2_sqrt, ema_w, decay, clip_state,
                   grad_scale=1.0, dev_step=None, shadow=None):
    """adamw_step with the gradient also scaled by clip_state[1], skipped on the device when clip_state[0] is not
    finite (clip_state: the four doubles grad_clip_coef leaves).  ema and decay_mask may be None.  dev_step, when
    given, holds four floats: {step_size, bc2_sqrt, ema_w, decay}."""
    assert clip_state is not None
    _adam_asserts(p, shadow, ema, decay_mask, dev_step, (4, 4), clip_state)
    check(_lib.load().qarig_adam_clip_step(ptr(p), ptr(g), ptr(m), ptr(v), ptr(ema), ptr(decay_mask), p.numel(),
                                           beta1, beta2, eps, step_size, bc2_sqrt, ema_w, decay, grad_scale,
                                           ptr(dev_step), ptr(shadow), ptr(clip_state), stream()),
          "qarig_adam_clip_step")


def swap_(a, b):
    """Exchanges the contents of two fp32 tensors of equal size in place, bit for bit.  They must not overlap."""
    require_cuda(a, b)
    if a.dtype != torch.float32 or b.dtype != torch.float32 or a.numel() != b.numel() \
            or not (a.is_contiguous() and b.is_contiguous()):
        raise ValueError("swap_: two contiguous fp32 tensors of the same size")
    check(_lib.load().qarig_swap_f32(ptr(a), ptr(b), a.numel(), stream()), "qarig_swap_f32")


def mul_fwd(a, b):
    y = torch.empty_like(a)
    check(_lib.load().qarig_mul_fwd(ptr(a), ptr(b), ptr(y), a.numel(), stream()), "qarig_mul_fwd")
    return y


def mul_bwd(dy, a, b):
    da = torch.empty_like(a)
    db = torch.empty_like(a)
    check(_lib.load().qarig_mul_bwd(ptr(dy), ptr(a), ptr(b), ptr(da), ptr(db), a.numel(), stream()),
          "qarig_mul_bwd")
    return da, db


def act_fwd(x, act):
    y = torch.empty_like(x)
    check(_lib.load().qarig_act_fwd(ptr(x), ptr(y), x.numel(), act, stream()), "qarig_act_fwd")
    return y


def act_bwd(dy, z, act):
    dz = torch.empty_like(z)
    check(_lib.load().qarig_act_bwd(ptr(dy), ptr(z), ptr(dz), z.numel(), act, stream()),
          "qarig_act_bwd")
    return dz


def scale_by(x, s):
    y = torch.empty_like(x)
    check(_lib.load().qarig_scale_by(ptr(x), ptr(s), ptr(y), x.numel(), stream()), "qarig_scale_by")
    return y


# Launch geometry of qarig_dropout (csrc/dropout_philox.h): 256 threads, eight elements per thread-iteration, at
# most 8192 workgroups -- a launch of more than DROPOUT_SWEEP elements wraps the grid-stride loop.
DROPOUT_MAX_THRESHOLD = 58982
DROPOUT_SWEEP = 8192 * 256 * 8


def dropout(x, threshold, scale, site, key, out=None):
    """y = x * scale where kept, +0 where dropped; the keep-bit of flat element e is a pure function of
    (key = device int32[4] {seed_lo, seed_hi, step, rank}, site, e) -- include/qarig.h qarig_dropout.
    threshold: 1 ... 58982, drop rate threshold / 65536; scale: 65536 / (65536 - threshold) as fp32
    (qarig.dropout.threshold_and_scale gives both).  out: None (a new tensor), x itself (in place) or a
    contiguous fp32 tensor of x's size that does not overlap x."""
    require_cuda(x, key, out)
    if x.dtype != torch.float32 or not x.is_contiguous():
        raise TypeError(f"dropout: a contiguous fp32 tensor, got {x.dtype}"
                        f"{'' if x.is_contiguous() else ' (not contiguous)'}; nothing is cast or copied here")
    if key.dtype != torch.int32 or key.numel() != 4 or not key.is_contiguous():
        raise TypeError("dropout: key is a contiguous int32 tensor of 4 words {seed_lo, seed_hi, step, rank}")
    y = torch.empty_like(x) if out is None else out
    if y.dtype != torch.float32 or not y.is_contiguous() or y.numel() != x.numel():
        raise TypeError("dropout: out must be a contiguous fp32 tensor of x's size")
    threshold, site = int(threshold), int(site)
    if not 1 <= threshold <= DROPOUT_MAX_THRESHOLD:
        raise ValueError(f"dropout: threshold must lie in [1, {DROPOUT_MAX_THRESHOLD}], got {threshold}")
    if not 0 <= site < 2 ** 32:
        raise ValueError(f"dropout: site must fit 32 bits, got {site}")
    check(_lib.load().qarig_dropout(ptr(x), ptr(y), x.numel(), threshold, float(scale), site, ptr(key), stream()),
          "qarig_dropout")
    return y


# -------------------------------------------------------------------------- conv
def _conv_workspace(weight, nbytes, geom, tag, inference):
    """(scratch tensor, flags) of a conv forward.  Training (`inference` False -- the caller decides, outside
    its autograd node: torch.is_grad_enabled() is always False inside an autograd.Function.forward, and
    functional.conv2d_act samples it before .apply): the shared scratch, weights re-ordered in every call.  Inference (the
    weights are constants between optimiser steps): one scratch per weight and geometry, kept while the
    weight is unchanged (address / version / LP_EPOCH, as the bf16 shadows), so the re-ordering launch runs
    once (QARIG_CONV_PACKED_VALID).  Inside a stream capture always the shared scratch: a captured launch
    must not hold the address of a cache entry that an invalidation can free."""
    if not inference or torch.cuda.is_current_stream_capturing():
        return workspace(nbytes, weight.device, tag), 0
    fresh = []

    def scratch():
        fresh.append(torch.empty(max(16, nbytes), dtype=torch.uint8, device=weight.device))
        return fresh[0]

    ws = _lp_image(tag, weight, scratch, tail=(_lib.OPTION_EPOCH, geom))
    return ws, int(not fresh)


def conv2d_fwd(x, weight, bias, stride, pad, act, want_preact=False, inference=False):
    """nn.Conv2d + bias + activation (reference models/layers.py:157-184, 211-230).
    inference: no gradient will be asked of this call (cached re-ordered weights, _conv_workspace)."""
    require_cuda(x, weight, bias)
    x = f32c(x)
    N, Cin, H, W = x.shape
    Cout, Cin2, k, k2 = weight.shape
    assert Cin == Cin2 and k == k2
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    y = torch.empty((N, Cout, Ho, Wo), dtype=torch.float32, device=x.device)
    pre = torch.empty_like(y) if want_preact else None
    lib = _lib.load()
    ws, flags = _conv_workspace(weight, lib.qarig_conv2d_fwd_workspace_bytes_n(N, Cin, H, W, Cout, k, stride),
                                (N, H, W, stride, pad, x.data_ptr() % 16), "convfwd", inference)   # (alignment picks the kernel family)
    check(lib.qarig_conv2d_fwd_ws(ptr(x), N, Cin, H, W, ptr(weight), ptr(bias), Cout, k, stride,
                                  pad, act, ptr(y), ptr(pre), ptr(ws), ws.numel(), flags, stream()),
          "qarig_conv2d_fwd_ws")
    return (y, pre) if want_preact else y


def conv_transpose2d_fwd(x, weight, bias, act, want_preact=False, inference=False):
    """nn.ConvTranspose2d(4, 2, 1) + bias + activation (reference layers.py:188-207)."""
    require_cuda(x, weight, bias)
    x = f32c(x)
    N, Cin, H, W = x.shape
    Cin2, Cout, k, k2 = weight.shape
    assert Cin == Cin2 and k == 4 and k2 == 4
    y = torch.empty((N, Cout, 2 * H, 2 * W), dtype=torch.float32, device=x.device)
    pre = torch.empty_like(y) if want_preact else None
    lib = _lib.load()
    ws, flags = _conv_workspace(weight, lib.qarig_conv_transpose2d_workspace_bytes_n(N, Cin, H, W, Cout),
                                (N, H, W, bool(want_preact), x.data_ptr() % 16), "convt", inference)
    check(lib.qarig_conv_transpose2d_fwd(ptr(x), N, Cin, H, W, ptr(weight), ptr(bias), Cout, act,
                                         ptr(y), ptr(pre), ptr(ws), ws.numel(), flags, stream()),
          "qarig_conv_transpose2d_fwd")
    return (y, pre) if want_preact else y


def mse_fwd(pred, target, want_grad=True):
    """mean((pred-target)^2) and its gradient w.r.t. pred."""
    require_cuda(pred, target)
    assert pred.shape == target.shape
    loss = torch.empty((), dtype=torch.float32, device=pred.device)
    dp = torch.empty_like(pred) if want_grad else None
    lib = _lib.load()
    part = torch.empty(lib.qarig_mse_workspace_bytes() // 4, dtype=torch.float32, device=pred.device)
    check(lib.qarig_mse_fwd(ptr(pred), ptr(target), pred.numel(), ptr(loss), ptr(dp), ptr(part),
                            stream()), "qarig_mse_fwd")
    return loss, dp


def index_histogram(ids, counts):
    """counts (int64 [K], on the device) += histogram of ids."""
    require_cuda(ids, counts)
    ids = _i64c(ids).reshape(-1)
    assert counts.dtype == torch.int64 and counts.is_contiguous()
    check(_lib.load().qarig_index_histogram(ptr(ids), ids.numel(), counts.numel(), ptr(counts),
                                            ptr(_bad_flag(ids.device)), stream()),
          "qarig_index_histogram")
    return counts
