"""Cost of the generation-evaluation launches (csrc/moments.hip) and their share of one GenerationScorer.add.

Kernel part: ops.pool_features (pool 1: the fp32 -> fp64 conversion) and ops.moments_add at (n = 64, D = 256) --
64 latents of 4 x 8 x 8 -- and at (n = 256, D = 1024) -- 256 latents of 4 x 16 x 16; device events around back-to-back
calls, medians of 7 after warm-up.  For moments_add the achieved fp64 rate is stated twice: over the products the
maintained triangle needs (2 n per maintained element) and over the MFMAs issued (whole 16 x 16 x 4 steps, four tiles
per wave, padding included), against the 78.6 TFLOP/s that AMD publishes as the MI355X's fp64 matrix peak.

Scorer part: one GenerationScorer.add of a generated batch in image space at config-1 shapes (batch 4, latents
4 x 16 x 16, the 2-layer 256 ... 512-channel decoder giving 3 x 64 x 64, pool 8: D = 192) against the decoder call it
contains.  The two arms alternate in one process; medians of 7.  Nothing is gated: the numbers are recorded as measured.

    python tools/gen_eval_bench.py --out profiles/r34_gen_eval.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
for p in (ROOT, os.path.join(ROOT, "quantized-autoregression-image-generator_amd")):
    sys.path.insert(0, os.path.abspath(p))

from models.FC_Decoder import FC_Decoder  # noqa: E402
from qarig import gen_eval, ops  # noqa: E402

REPS = 7
FP64_MATRIX_PEAK_TFLOPS = 78.6      # AMD's published MI355X figure


def timed(fn, launches):
    """Microseconds per call of fn: device events around `launches` back-to-back calls."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / launches


def summary(ts, unit="us"):
    return {f"{unit}_median": round(statistics.median(ts), 2), f"{unit}_min": round(min(ts), 2),
            f"{unit}_max": round(max(ts), 2)}


def kernel_part(N, C, H, W):
    g = torch.Generator(device="cuda").manual_seed(0)
    z = torch.tanh(torch.randn((N, C, H, W), device="cuda", generator=g))
    f = ops.pool_features(z, 1)
    D = f.shape[1]
    shift = f.mean(dim=0)
    state = (torch.zeros(1, dtype=torch.int64, device="cuda"), torch.zeros(D, dtype=torch.float64, device="cuda"),
             torch.zeros((D, D), dtype=torch.float64, device="cuda"))
    forms = {"pool_features": lambda: ops.pool_features(z, 1), "moments_add": lambda: ops.moments_add(f, state, shift)}
    for fn in forms.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for _ in range(REPS):
        for k, fn in forms.items():
            times[k].append(timed(fn, 20))
    out = {"n": N, "D": D, "launches_per_sample": 20, "samples": REPS}
    for k, ts in times.items():
        out[k] = summary(ts)
    T = -(-D // 16)
    maintained = sum(min(16, D - 16 * i) * (D - 16 * i) for i in range(T))
    issued = sum(-(-(T - i) // 4) * 4 for i in range(T)) * 256 * (-(-N // 4) * 4)
    us = out["moments_add"]["us_median"]
    out["moments_add"]["useful_fp64_TFLOPs"] = round(2 * N * maintained / us * 1e-6, 3)
    out["moments_add"]["issued_fp64_TFLOPs"] = round(2 * issued / us * 1e-6, 3)
    out["moments_add"]["issued_share_of_fp64_matrix_peak"] = round(2 * issued / us * 1e-6 / FP64_MATRIX_PEAK_TFLOPS, 4)
    out["pool_features"]["GBps"] = round((4 + 8) * z.numel() / out["pool_features"]["us_median"] * 1e-3, 1)
    return out


def scorer_part(calls_per_sample):
    torch.manual_seed(0)
    dev = torch.device("cuda", torch.cuda.current_device())
    dec = FC_Decoder(num_layers=2, image_channel=3, min_channel=256, max_channel=512, latent_channel=4).to(dev).eval()
    z = torch.tanh(torch.randn((4, 4, 16, 16), generator=torch.Generator().manual_seed(1))).to(dev)
    scorer = gen_eval.GenerationScorer(8, space="image", decoder=dec)
    scorer.add(z, "real")

    @torch.no_grad()
    def decoder_only():
        return dec(z)

    arms = {"add": lambda: scorer.add(z, "generated"), "decoder_only": decoder_only}
    for fn in arms.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    for _ in range(REPS):
        for k, fn in arms.items():
            t0 = time.perf_counter()
            for _ in range(calls_per_sample):
                fn()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) / calls_per_sample * 1e6)
    out = {"shapes": "config 1: batch 4, latent 4x16x16, decoder 2 layers 256..512 channels -> 3x64x64, pool 8, D=192",
           "calls_per_sample": calls_per_sample, "samples": REPS, "timing": "host wall clock around synchronised calls"}
    for k, ts in times.items():
        out[k] = summary(ts)
    out["moments_us"] = round(out["add"]["us_median"] - out["decoder_only"]["us_median"], 2)
    out["moments_share_of_add"] = round(out["moments_us"] / out["add"]["us_median"], 4)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="write the JSON result here as well as to stdout")
    ap.add_argument("--calls-per-sample", type=int, default=10)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    torch.cuda.set_device(0)
    res = {"device": torch.cuda.get_device_name(0), "fp64_matrix_peak_TFLOPs": FP64_MATRIX_PEAK_TFLOPS,
           "kernel": [kernel_part(64, 4, 8, 8), kernel_part(256, 4, 16, 16)],
           "scorer": scorer_part(args.calls_per_sample)}
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
