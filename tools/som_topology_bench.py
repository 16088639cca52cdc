"""Cost of the SOM topology evaluation (csrc/bmu.hip qarig_bmu_top2, csrc/topology.hip) -- recorded, nothing gated.

Search: ops.bmu_top2 against ops.bmu on the same inputs at 65,536 rows x 512 codes x 16 (config 2) and at 8,192 and
32,768 rows x 8,192 codes x 4 (config 5); device events around back-to-back calls, the two arms alternating in one
process, medians of 7 after warm-up, and the ratio of the medians.  ops.bmu is the project's most-tuned kernel (a
branch-free scan on the fp32 / bf16 MFMA); the top-2 search evaluates the literal distance per candidate on the
vector ALU, so a ratio of several is what the form costs.

Reductions: ops.topology_rows on the search's outputs and ops.code_lag_profile at K = 512, D = 16 and K = 8,192,
D = 4, in microseconds.

Scorer: ReconScorer.add_batch with and without topology=True at the config-1 shapes of tools/recon_bench.py, host
wall clock around synchronised calls, arms alternating.

    python tools/som_topology_bench.py --out profiles/r36_som_topology.json
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

from models.Codebook import Codebook  # noqa: E402
from models.FC_Decoder import FC_Decoder  # noqa: E402
from qarig import ops, recon_eval  # noqa: E402

REPS = 7


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


def alternate(arms, launches):
    for fn in arms.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    for _ in range(REPS):
        for k, fn in arms.items():
            times[k].append(timed(fn, launches))
    return {k: summary(ts) for k, ts in times.items()}


def search_part(N, C, H, W, patch, K, launches):
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.tanh(torch.randn((N, C, H, W), device="cuda", generator=g))
    w = torch.tanh(torch.randn((K, C * patch * patch), device="cuda", generator=g))
    rows = N * (H // patch) * (W // patch)
    out = alternate({"bmu": lambda: ops.bmu(x, w, (patch, patch)),
                     "bmu_top2": lambda: ops.bmu_top2(x, w, (patch, patch))}, launches)
    i1, i2, d1, d2 = ops.bmu_top2(x, w, (patch, patch))
    assert torch.equal(i1, ops.bmu(x, w, (patch, patch))), "idx1 differs from ops.bmu"
    gap = torch.zeros(K, dtype=torch.int64, device="cuda")
    ratio = torch.zeros(32, dtype=torch.int64, device="cuda")
    sums = torch.empty((N, 3), dtype=torch.float64, device="cuda")
    out.update(alternate({"topology_rows": lambda: ops.topology_rows(i1, i2, d1, d2, N, gap, ratio, sums),
                          "code_lag_profile": lambda: ops.code_lag_profile(w)}, launches))
    out.update(rows=rows, K=K, D=C * patch * patch, images=N, launches_per_sample=launches, samples=REPS,
               top2_over_bmu=round(out["bmu_top2"]["us_median"] / out["bmu"]["us_median"], 2),
               top2_candidates_per_us=round(rows * K / out["bmu_top2"]["us_median"], 1))
    return out


def scorer_part(calls_per_sample):
    torch.manual_seed(0)
    dev = torch.device("cuda", torch.cuda.current_device())
    dec = FC_Decoder(num_layers=2, image_channel=3, min_channel=256, max_channel=512, latent_channel=4).to(dev).eval()
    cb = Codebook(patch_dim=(2, 2), image_dim=(16, 16), image_channel=4, num_embeddings=512).to(dev).eval()
    with torch.no_grad():
        cb.codebook.weight.copy_(torch.tanh(torch.randn(cb.codebook.weight.shape)))
    z = torch.tanh(torch.randn((4, 4, 16, 16), generator=torch.Generator().manual_seed(1))).to(dev)
    scorers = {"add_batch": recon_eval.ReconScorer(dec, {"hr": cb}),
               "add_batch_topology": recon_eval.ReconScorer(dec, {"hr": cb}, topology=True)}

    def arm(scorer):
        def run():
            scorer.add_batch(z)
            for entry in scorer._err.values():        # keep the lists from growing over the run
                entry[1].clear()
                if entry[2] is not None:
                    entry[2].clear()
            if scorer._topology is not None:
                for st in scorer._topology._state.values():
                    st[2].clear()
        return run

    arms = {k: arm(s) for k, s in scorers.items()}
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
    out = {"shapes": "config 1: batch 4, latent 4x16x16, decoder 2 layers 256..512 channels -> 3x64x64, K=512 patch 2x2",
           "calls_per_sample": calls_per_sample, "samples": REPS, "timing": "host wall clock around synchronised calls"}
    for k, ts in times.items():
        out[k] = summary(ts)
    out["topology_us"] = round(out["add_batch_topology"]["us_median"] - out["add_batch"]["us_median"], 2)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="write the JSON result here as well as to stdout")
    ap.add_argument("--calls-per-sample", type=int, default=10)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    torch.cuda.set_device(0)
    res = {"device": torch.cuda.get_device_name(0),
           "search": [search_part(64, 4, 64, 64, 2, 512, 20),         # config 2: 65,536 x 512 x 16
                      search_part(8, 4, 32, 32, 1, 8192, 10),         # config 5:  8,192 x 8,192 x 4
                      search_part(32, 4, 32, 32, 1, 8192, 5)],        #           32,768 x 8,192 x 4
           "scorer": scorer_part(args.calls_per_sample),
           "limiters": "not measured (no counter run): the search is expected to be bound by vector-ALU issue"}
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
