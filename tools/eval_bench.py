"""Cost of the held-out evaluation (csrc/score.hip, qarig/evaluate.py); two comparisons, each with its arms
alternating in one process, medians of 7 after warm-up.

(a) kernels: qarig_token_score + qarig_score_reduce against the existing pair behind
    qarig_cross_entropy_fwd(dlogits = NULL) (ce_reg_rows_kernel<false, false, false> + mean2_kernel, whose two sweeps
    are token_score_kernel's: csrc/row_sweep.h) on the same logits and targets, at
    16,384 x 513 (config 2: 64 windows of 256 tokens) and 32,768 x 8,193 (config 5's vocabulary: 8 x 4,096).  Both
    arms sweep the logits twice; achieved GB/s counts one read of the logits (the second sweep may hit in cache).
(b) pipeline: TokenScorer.add_batch against pipeline.train_step at config 2's shapes (bench.py's model builder), in
    tokens/s -- tokens scored (64 x 257, two windows) against tokens trained on (64 x 256, one window).

    python tools/eval_bench.py --out profiles/r19_token_score.json
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

import bench  # noqa: E402
from qarig import _lib, evaluate, ops, pipeline  # noqa: E402
from qarig.optim import FlatAdam  # noqa: E402

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


def kernel_part(N, S, C):
    M = N * S
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randn((M, C), device="cuda", generator=g) * 3.0
    t = torch.randint(0, C, (M,), device="cuda", generator=g)
    lib, s, P = _lib.load(), _lib.stream(), _lib.ptr
    loss = torch.empty((), dtype=torch.float32, device="cuda")
    rows = torch.empty(M, dtype=torch.float32, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    nll = torch.empty(M, dtype=torch.float32, device="cuda")
    rank = torch.empty(M, dtype=torch.int32, device="cuda")
    img = torch.zeros(N, dtype=torch.float64, device="cuda")
    pos = torch.zeros(S + 1, dtype=torch.float64, device="cuda")
    cnt = torch.zeros(S + 1, dtype=torch.int64, device="cuda")
    tot = torch.zeros(3, dtype=torch.int64, device="cuda")

    def old():
        return lib.qarig_cross_entropy_fwd(P(x), P(t), M, C, P(loss), None, P(rows), P(flag), s)

    def new():
        return lib.qarig_token_score(P(x), P(t), M, C, -100, P(nll), P(rank), P(flag), s) or \
            lib.qarig_score_reduce(P(nll), P(rank), N, S, 0, S + 1, 5, P(img), P(pos), P(cnt), P(tot), s)

    def new_rows_only():
        return lib.qarig_token_score(P(x), P(t), M, C, -100, P(nll), P(rank), P(flag), s)

    forms = {"cross_entropy_fwd_pair": old, "token_score_pair": new, "token_score_alone": new_rows_only}
    launches = max(5, min(50, (1 << 31) // (4 * M * C)))
    for fn in forms.values():
        for _ in range(3):
            assert fn() == 0
    torch.cuda.synchronize()
    assert torch.equal(nll, rows), "the two row kernels share their arithmetic"
    times = {k: [] for k in forms}
    for _ in range(REPS):
        for k, fn in forms.items():
            times[k].append(timed(fn, launches))
    out = {"rows": M, "classes": C, "N": N, "S": S, "launches_per_sample": launches, "samples": REPS,
           "logits_MB": round(4 * M * C * 1e-6, 1)}
    for k, ts in times.items():
        med = statistics.median(ts)
        out[k] = {"us_median": round(med, 2), "us_min": round(min(ts), 2), "us_max": round(max(ts), 2),
                  "us_samples": [round(v, 2) for v in ts], "logits_GBps": round(4 * M * C / med * 1e-3, 1)}
    o, n = out["cross_entropy_fwd_pair"], out["token_score_pair"]
    out["new_over_old"] = round(n["us_median"] / o["us_median"], 4)
    out["new_slower_beyond_old_spread"] = bool(n["us_median"] > o["us_max"])
    return out


def pipeline_part(steps_per_sample):
    cfg = dict(bench.CFG)
    dev = torch.device("cuda", torch.cuda.current_device())
    C, H, W = cfg["latent"]
    z = torch.tanh(torch.randn((cfg["batch"], C, H, W), generator=torch.Generator().manual_seed(1))).to(dev)
    seq = (H // cfg["hr_patch"]) * (W // cfg["hr_patch"]) + 1
    nwin = pipeline.num_windows(seq, cfg["window"])
    rng = torch.Generator().manual_seed(4)
    lr_cb, hr_cb, model = bench.build_models(dev, cfg)
    opt = FlatAdam(model.parameters(), lr=cfg["lr"], betas=(0.5, 0.999))
    scorer = evaluate.TokenScorer(model, lr_cb, hr_cb, cfg["base"], cfg["window"])

    def train():
        rand = torch.randint(0, nwin, (cfg["batch"],), generator=rng)
        hr_in, lr_in, hr_tg, pos = pipeline.tokenize_window(z, lr_cb, hr_cb, cfg["base"], cfg["window"], rand)
        pipeline.train_step(model, opt, hr_in, lr_in, hr_tg, pos, dp=False, pos_bound=seq)

    arms = {"train_step": (train, cfg["batch"] * cfg["window"]),
            "add_batch": (lambda: scorer.add_batch(z), cfg["batch"] * seq)}
    for fn, _ in arms.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    for _ in range(REPS):
        for k, (fn, _) in arms.items():
            t0 = time.perf_counter()
            for _ in range(steps_per_sample):
                fn()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) / steps_per_sample * 1e3)
    r = scorer.result()
    out = {"workload": cfg["name"], "steps_per_sample": steps_per_sample, "samples": REPS,
           "eval_windows": pipeline.eval_windows(seq, cfg["window"]), "scored_tokens_total": r["tokens"]}
    for k, ts in times.items():
        med = statistics.median(ts)
        out[k] = {"ms_median": round(med, 3), "ms_min": round(min(ts), 3), "ms_max": round(max(ts), 3),
                  "tokens_per_call": arms[k][1], "tokens_per_s": round(arms[k][1] / med * 1e3, 1)}
    out["add_batch_over_train_step_tokens_per_s"] = round(out["add_batch"]["tokens_per_s"] /
                                                          out["train_step"]["tokens_per_s"], 4)
    out["add_batch_faster"] = bool(out["add_batch"]["tokens_per_s"] > out["train_step"]["tokens_per_s"])
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="write the JSON result here as well as to stdout")
    ap.add_argument("--no-pipeline", action="store_true", help="kernel part only")
    ap.add_argument("--steps-per-sample", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    torch.cuda.set_device(0)
    res = {"device": torch.cuda.get_device_name(0)}
    res["kernels"] = [kernel_part(64, 256, 513), kernel_part(8, 4096, 8193)]
    torch.cuda.empty_cache()
    if not args.no_pipeline:
        res["config2"] = pipeline_part(args.steps_per_sample)
        ops.check_index_flag(torch.device("cuda", 0), "eval_bench")
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    assert args.no_pipeline or res["config2"]["add_batch_faster"], \
        "the forward alone must score tokens faster than the step trains on them"


if __name__ == "__main__":
    main()
