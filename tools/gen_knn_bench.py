"""Cost of the k-nearest-neighbour launches of the generation evaluation (csrc/knn.hip) and of manifold_metrics as a
whole, beside what a user would otherwise reach for: torch.cdist in fp64 plus topk on the same data.

Shapes: (n = m = 4,096, D = 256) and (16,384, D = 1,024), rows 0.7 N(0,1) + 0.3, shift = the mean of the first 64 rows.
Arms per shape, alternating in one process, device events around back-to-back calls, medians of 7 after warm-up:
  knn_smallest      ops.knn_smallest(x, x, 3, shift, 0)           (self excluded)
  ball_count        ops.ball_count(g, x, r2, shift)
  manifold_metrics  gen_eval.manifold_metrics(x, g, 3, shift)     (five launches of the above and one read-back)
  cdist_topk        torch.cdist(x, x) (fp64) and topk(4, largest=False) -- the yardstick, not a reference: it returns
                    distances, not squared ones, and does not exclude self by index
For the two kernels the achieved fp64 rate (2 n m D per launch, the useful terms) is stated against the 78.6 TFLOP/s
that AMD publishes as the MI355X's fp64 matrix peak -- a data-sheet figure, not measured here.  No counter pass was
made, so no limiter is named.  Nothing is gated: the numbers are recorded as measured.

    python tools/gen_knn_bench.py --out profiles/r35_gen_knn.json
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
for p in (ROOT, os.path.join(ROOT, "quantized-autoregression-image-generator_amd")):
    sys.path.insert(0, os.path.abspath(p))

from qarig import gen_eval, ops  # noqa: E402

REPS = 7
FP64_MATRIX_PEAK_TFLOPS = 78.6      # AMD's published MI355X figure
K = 3


def timed(fn, launches):
    """Milliseconds per call of fn: device events around `launches` back-to-back calls."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / launches


def shape_part(n, D, launches, with_cdist=True):
    g = torch.Generator(device="cuda").manual_seed(n + D)
    x = torch.randn((n, D), device="cuda", dtype=torch.float64, generator=g) * 0.7 + 0.3
    gen = torch.randn((n, D), device="cuda", dtype=torch.float64, generator=g) * 0.75 + 0.3
    shift = x[:64].mean(dim=0)
    r2 = ops.knn_smallest(x, x, K, shift, 0)[0][:, K - 1].contiguous()
    arms = {"knn_smallest": lambda: ops.knn_smallest(x, x, K, shift, 0),
            "ball_count": lambda: ops.ball_count(gen, x, r2, shift),
            "manifold_metrics": lambda: gen_eval.manifold_metrics(x, gen, K, shift)}
    if with_cdist:
        arms["cdist_topk"] = lambda: torch.cdist(x, x).topk(K + 1, dim=1, largest=False)
    for fn in arms.values():
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    for _ in range(REPS):
        for k, fn in arms.items():
            times[k].append(timed(fn, launches))
    out = {"n": n, "m": n, "D": D, "k": K, "launches_per_sample": launches, "samples": REPS}
    for k, ts in times.items():
        out[k] = {"ms_median": round(statistics.median(ts), 4), "ms_min": round(min(ts), 4),
                  "ms_max": round(max(ts), 4)}
    for k in ("knn_smallest", "ball_count"):
        tf = 2.0 * n * n * D / (out[k]["ms_median"] * 1e-3) * 1e-12
        out[k]["useful_fp64_TFLOPs"] = round(tf, 3)
        out[k]["share_of_fp64_matrix_peak"] = round(tf / FP64_MATRIX_PEAK_TFLOPS, 4)
    # the same neighbours?  (cdist takes differences: its nearest rows are the reference's on this data)
    if with_cdist:
        ours = ops.knn_smallest(x, x, K, shift, 0)[1]
        theirs = torch.cdist(x, x).topk(K + 1, dim=1, largest=False).indices[:, 1:]
        out["neighbours_equal_to_cdist_topk"] = bool((ours == theirs.int()).all())
    out["metrics"] = gen_eval.manifold_metrics(x, gen, K, shift)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="write the JSON result here as well as to stdout")
    ap.add_argument("--small-only", action="store_true", help="the (4,096, 256) shape only")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    torch.cuda.set_device(0)
    shapes = [shape_part(4096, 256, 5)]
    if not args.small_only:
        shapes.append(shape_part(16384, 1024, 1))
    res = {"device": torch.cuda.get_device_name(0), "fp64_matrix_peak_TFLOPs": FP64_MATRIX_PEAK_TFLOPS,
           "limiter": "not measured (no counter pass was made)", "shapes": shapes}
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
