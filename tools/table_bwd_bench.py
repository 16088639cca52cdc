"""Backward of the position-table consumers with the table sums inside, and the 16-B split-K slab reduce, against the
launches they replace -- both forms alternating in one process, device events, medians.

Part 1, one decoder-block boundary: layernorm_bwd (table form, dx_add, dy_xhat) + segment_sum x 2 + mul_rows_bwd +
segment_sum (five launches) against layernorm_bwd_table + mul_rows_bwd_table (two), D = 512, at M = 16,384 / 8,192 /
2,048 token rows over tables of P = 384 and 1,152 rows.  The row map is a training batch's: M / 256 sequences, each a
window of 256 consecutive positions with a random start inside 257 (P = 384: config 2) or 1,025 (P = 1,152: config
4) positions.  The operands rotate through SETS buffer sets so that a launch does not find its inputs in the
last-level cache from the launch before.  The M / P sweep is what ops.TABLE_BWD_MIN_TOKENS_PER_ROW is read from.

Part 2, the slab reduce at 2048 x 512 x 8 slabs and 512 x 512 x 32 slabs (accumulate, as the weight gradients run
it), with the row sums where this build exposes them; --other-lib PATH adds the plain reduce of another build of the
library (the parent commit's scalar kernel) to the alternation.

    python tools/table_bwd_bench.py --out profiles/r18_table_bwd_bench.txt [--other-lib PATH]
"""
import argparse
import ctypes
import os
import statistics
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
for p in (ROOT, os.path.join(ROOT, "quantized-autoregression-image-generator_amd")):
    sys.path.insert(0, os.path.abspath(p))

from qarig import _lib, ops  # noqa: E402

REPS = 25
SETS = 4
D = 512


def timed(fn, launches):
    """Microseconds per call: device events around `launches` back-to-back calls fn(i)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(launches):
        fn(i)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / launches


def alternate(forms, launches):
    for fn in forms.values():
        for i in range(SETS):
            fn(i)
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for _ in range(REPS):
        for k, fn in forms.items():
            times[k].append(timed(fn, launches))
    return {k: (statistics.median(t), min(t), max(t)) for k, t in times.items()}


def row_index(M, positions, gen):
    n = M // 256
    start = torch.randint(0, positions - 256 + 1, (n, 1), generator=gen)
    return (start + torch.arange(256)[None]).reshape(-1).to(torch.int32)


def boundary(M, P, positions, lines):
    gen = torch.Generator().manual_seed(M + P)
    idx = row_index(M, positions, gen).cuda()
    offsets, rows = ops.rowmap_build(idx, P)
    st = (torch.randn((P, D), generator=gen) * 0.5 + 1.0).cuda()
    sh = torch.randn((P, D), generator=gen).cuda()
    gt = (torch.randn((P, D), generator=gen) * 0.5 + 1.0).cuda()
    sets = []
    for _ in range(SETS):
        x, dy, add, a = (torch.randn((M, D), device="cuda") for _ in range(4))
        _, mean, rstd = ops.layernorm_fwd(x, scale=st, shift=sh, mod_idx=idx)
        sets.append((x, dy, add, a, mean, rstd))

    def ln_two_step(i):
        x, dy, add, _, mean, rstd = sets[i % SETS]
        _, dyx = ops.layernorm_bwd(dy, x, mean, rstd, scale=st, want_dy_xhat=True, mod_idx=idx, dx_add=add)
        ops.segment_sum(dyx, offsets, rows)
        ops.segment_sum(dy, offsets, rows)

    def ln_fused(i):
        x, dy, add, _, mean, rstd = sets[i % SETS]
        ops.layernorm_bwd_table(dy, x, mean, rstd, st, offsets, rows, dx_add=add)

    def mul_two_step(i):
        _, dy, _, a, _, _ = sets[i % SETS]
        _, tok = ops.mul_rows_bwd(dy, a, gt, idx)
        ops.segment_sum(tok, offsets, rows)

    def mul_fused(i):
        _, dy, _, a, _, _ = sets[i % SETS]
        ops.mul_rows_bwd_table(dy, a, gt, offsets, rows)

    # the fused kernels give the two-step bits on this very row map
    x, dy, add, a, mean, rstd = sets[0]
    dx0, dyx = ops.layernorm_bwd(dy, x, mean, rstd, scale=st, want_dy_xhat=True, mod_idx=idx, dx_add=add)
    got = ops.layernorm_bwd_table(dy, x, mean, rstd, st, offsets, rows, dx_add=add)
    assert torch.equal(got[0], dx0) and torch.equal(got[1], ops.segment_sum(dyx, offsets, rows))
    assert torch.equal(got[2], ops.segment_sum(dy, offsets, rows))
    da0, tok = ops.mul_rows_bwd(dy, a, gt, idx)
    got = ops.mul_rows_bwd_table(dy, a, gt, offsets, rows)
    assert torch.equal(got[0], da0) and torch.equal(got[1], ops.segment_sum(tok, offsets, rows))

    res = alternate({"ln_two_step": ln_two_step, "ln_fused": ln_fused, "mul_two_step": mul_two_step,
                     "mul_fused": mul_fused}, launches=8)
    used = int((offsets[1:] > offsets[:-1]).sum())
    two = res["ln_two_step"][0] + res["mul_two_step"][0]
    one = res["ln_fused"][0] + res["mul_fused"][0]
    lines.append(f"boundary M={M} P={P} used_positions={used} M/P={M / P:.1f} D={D}: "
                 f"five launches {two:.1f} us, two launches {one:.1f} us, ratio {one / two:.3f}")
    for k, (med, lo, hi) in res.items():
        lines.append(f"    {k:13s} median {med:7.2f} us  min {lo:7.2f}  max {hi:7.2f}  ({REPS} samples of 8 launches)")
    print("\n".join(lines[-5:]), flush=True)


def slab(M, N, nslab, other, lines):
    P, L, I = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    lib, s = _lib.load(), _lib.stream()
    lib.qarig_slab_reduce_f32.restype = I
    lib.qarig_slab_reduce_f32.argtypes = [P, P, L, I, I, I, I, P]
    sets = [(torch.randn((nslab, M, N), device="cuda"), torch.randn((M, N), device="cuda"),
             torch.randn((nslab, M), device="cuda"), torch.randn(M, device="cuda")) for _ in range(SETS)]

    def plain(h):
        def fn(i):
            sl, out, _, _ = sets[i % SETS]
            assert h.qarig_slab_reduce_f32(sl.data_ptr(), out.data_ptr(), N, M, N, nslab, 1, s) == 0
        return fn

    def rowsum(i):
        sl, out, part, rs = sets[i % SETS]
        ops.slab_reduce(sl, out, M, N, accumulate=True, rs_part=part, rs_out=rs)

    forms = {"vec_plain": plain(lib), "vec_rowsum": rowsum}
    if other:
        other.qarig_slab_reduce_f32.restype = I
        other.qarig_slab_reduce_f32.argtypes = [P, P, L, I, I, I, I, P]
        forms["other_lib_plain"] = plain(other)
    res = alternate(forms, launches=16)
    mb = 4.0 * M * N * (nslab + 2) * 1e-6
    lines.append(f"slab reduce {M} x {N} x {nslab} slabs, accumulate ({mb:.1f} MB moved)")
    for k, (med, lo, hi) in res.items():
        lines.append(f"    {k:16s} median {med:7.2f} us  min {lo:7.2f}  max {hi:7.2f}  {mb / med * 1e3:.0f} GB/s"
                     f"  ({REPS} samples of 16 launches)")
    print("\n".join(lines[-1 - len(res):]), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    ap.add_argument("--other-lib", default=None, help="another build of the library (the parent commit's)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    torch.cuda.set_device(0)
    lines = [f"device {torch.cuda.get_device_name(0)}; TABLE_BWD_MIN_TOKENS_PER_ROW = "
             f"{ops.TABLE_BWD_MIN_TOKENS_PER_ROW}"]
    for P, positions in ((384, 257), (1152, 1025)):
        for M in (16384, 8192, 2048):
            boundary(M, P, positions, lines)
    other = ctypes.CDLL(os.path.abspath(args.other_lib)) if args.other_lib else None
    slab(2048, 512, 8, other, lines)
    slab(512, 512, 32, other, lines)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
