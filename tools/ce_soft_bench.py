"""Cost of SOM-neighbour soft targets in the fused cross-entropy launch (csrc/loss.hip); two comparisons,
each with its arms alternating in one process, medians of 7 after warm-up, device events around the kernels.  Nothing
is gated: the numbers are recorded as measured.

(a) kernels, with dlogits as the training step calls them, at 16,384 x 513 (config 2: 64 windows of 256 tokens) and
    32,768 x 8,193 (config 5's vocabulary: 8 x 4,096): qarig_cross_entropy_reg_fwd at (0.1, 1e-4) against
    qarig_cross_entropy_soft_fwd at (0.1, 1e-4, 0.2), R = 4, sigma = 2, codes = C - 1, and the soft entry at
    neighbour_smoothing = 0, which must write the regularised entry's bits (checked here; since DESIGN 9.41 both
    entries fill the same launcher's arguments, so that arm compares a launch with itself).  Achieved GB/s counts one
    read of the logits and one write of dlogits (the second and third sweep may hit in cache).
(b) the config-2 step (bench.py's model builder), pipeline.train_step with the soft targets off and on (no other
    regulariser in either arm: off is the default step).
(c) with --parent-root DIR (a built checkout of the parent commit): bench.py --gpus 1 as a child process, this
    tree's and the parent's alternating, three runs each -- the default step makes the parent's calls, so the two
    should agree within the run-to-run spread.

    python tools/ce_soft_bench.py --parent-root ../parent --out profiles/r32_ce_soft.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
for p in (ROOT, os.path.join(ROOT, "quantized-autoregression-image-generator_amd")):
    sys.path.insert(0, os.path.abspath(p))

import bench  # noqa: E402
from qarig import _lib, ops, pipeline  # noqa: E402
from qarig.optim import FlatAdam  # noqa: E402

REPS = 7
EPS, ZETA, NU, RANGE = 0.1, 1e-4, 0.2, 4


def timed(fn, launches):
    """Microseconds per call of fn: device events around `launches` back-to-back calls."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / launches


def kernel_part(M, C):
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randn((M, C), device="cuda", generator=g) * 3.0
    t = torch.randint(0, C, (M,), device="cuda", generator=g)
    lib, s, P = _lib.load(), _lib.stream(), _lib.ptr
    w = ops.neighbour_weights(RANGE, RANGE / 2.0, x.device)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    pair = torch.empty(2, dtype=torch.float32, device="cuda")
    rows = torch.empty(2 * M, dtype=torch.float32, device="cuda")
    dl = torch.empty_like(x)
    pair2 = torch.empty(2, dtype=torch.float32, device="cuda")
    rows2 = torch.empty(2 * M, dtype=torch.float32, device="cuda")
    dl2 = torch.empty_like(x)

    def reg():
        return lib.qarig_cross_entropy_reg_fwd(P(x), P(t), M, C, EPS, ZETA, P(pair), P(dl), P(rows), P(flag), s)

    def soft(nu):
        return lambda: lib.qarig_cross_entropy_soft_fwd(P(x), P(t), M, C, C - 1, EPS, ZETA, nu, RANGE, P(w), P(pair2),
                                                        P(dl2), P(rows2), P(flag), s)

    forms = {"reg_0.1_1e-4": reg, "soft_nu_0": soft(0.0), "soft_nu_0.2_R4": soft(NU)}
    launches = max(5, min(50, (1 << 31) // (8 * M * C)))
    for _ in range(3):
        assert forms["soft_nu_0.2_R4"]() == 0 and reg() == 0 and forms["soft_nu_0"]() == 0
    torch.cuda.synchronize()
    same = bool(torch.equal(dl, dl2) and torch.equal(rows, rows2) and torch.equal(pair, pair2))
    assert same, "the new entry at neighbour_smoothing = 0 must write the regularised entry's bits"
    times = {k: [] for k in forms}
    for _ in range(REPS):
        for k, fn in forms.items():
            times[k].append(timed(fn, launches))
    out = {"rows": M, "classes": C, "codes": C - 1, "launches_per_sample": launches, "samples": REPS,
           "logits_MB": round(4 * M * C * 1e-6, 1), "soft_nu_0_bits_equal_reg": same}
    for k, ts in times.items():
        med = statistics.median(ts)
        out[k] = {"us_median": round(med, 2), "us_min": round(min(ts), 2), "us_max": round(max(ts), 2),
                  "us_samples": [round(v, 2) for v in ts], "read_plus_write_GBps": round(8 * M * C / med * 1e-3, 1)}
    base = out["reg_0.1_1e-4"]
    for k in ("soft_nu_0", "soft_nu_0.2_R4"):
        out[k + "_over_reg"] = round(out[k]["us_median"] / base["us_median"], 4)
        out[k + "_slower_beyond_reg_spread"] = bool(out[k]["us_median"] > base["us_max"])
    return out


def step_part(steps_per_sample):
    cfg = dict(bench.CFG)
    dev = torch.device("cuda", torch.cuda.current_device())
    C, H, W = cfg["latent"]
    z = torch.tanh(torch.randn((cfg["batch"], C, H, W), generator=torch.Generator().manual_seed(1))).to(dev)
    seq = (H // cfg["hr_patch"]) * (W // cfg["hr_patch"]) + 1
    nwin = pipeline.num_windows(seq, cfg["window"])
    rng = torch.Generator().manual_seed(4)
    lr_cb, hr_cb, model = bench.build_models(dev, cfg)
    opt = FlatAdam(model.parameters(), lr=cfg["lr"], betas=(0.5, 0.999))

    def step(**soft):
        def fn():
            rand = torch.randint(0, nwin, (cfg["batch"],), generator=rng)
            hr_in, lr_in, hr_tg, pos = pipeline.tokenize_window(z, lr_cb, hr_cb, cfg["base"], cfg["window"], rand)
            return pipeline.train_step(model, opt, hr_in, lr_in, hr_tg, pos, dp=False, pos_bound=seq, **soft)
        return fn

    arms = {"off": step(), "on": step(neighbour_smoothing=NU, neighbour_range=RANGE, codes=hr_cb.num_embeddings)}
    last = {}
    for k, fn in arms.items():
        for _ in range(2):
            last[k] = fn()
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    for _ in range(REPS):
        for k, fn in arms.items():
            t0 = time.perf_counter()
            for _ in range(steps_per_sample):
                last[k] = fn()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) / steps_per_sample * 1e3)
    out = {"workload": cfg["name"], "steps_per_sample": steps_per_sample, "samples": REPS,
           "neighbour_smoothing": NU, "neighbour_range": RANGE, "neighbour_sigma": RANGE / 2.0,
           "codes": hr_cb.num_embeddings, "tokens_per_step": cfg["batch"] * cfg["window"],
           "last_pair_on": pipeline.loss_pair(last["on"]).tolist(), "last_loss_off": float(last["off"].detach())}
    for k, ts in times.items():
        med = statistics.median(ts)
        out[k] = {"ms_median": round(med, 3), "ms_min": round(min(ts), 3), "ms_max": round(max(ts), 3),
                  "ms_samples": [round(v, 3) for v in ts]}
    out["on_over_off"] = round(out["on"]["ms_median"] / out["off"]["ms_median"], 4)
    out["on_slower_beyond_off_spread"] = bool(out["on"]["ms_median"] > out["off"]["ms_max"])
    return out


def bench_part(parent_root, steps, warmup, runs=3):
    """bench.py as a child process (a fresh process per run), this tree's and the parent checkout's alternating."""
    arms = {"this": os.path.abspath(ROOT), "parent": os.path.abspath(parent_root)}
    vals, losses = {k: [] for k in arms}, {k: [] for k in arms}
    for _ in range(runs):
        for k, root in arms.items():
            r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", str(steps),
                                "--warmup", str(warmup)], cwd=root, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                raise RuntimeError(f"bench.py ({k}) failed:\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
            line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
            vals[k].append(line["ms_per_step"])
            losses[k].append(line.get("config", {}).get("loss"))
    out = {"steps": steps, "warmup": warmup, "runs_each": runs}
    for k, v in vals.items():
        out[k] = {"ms_per_step": v, "median": statistics.median(v), "min": min(v), "max": max(v), "loss": losses[k]}
    out["this_over_parent"] = round(out["this"]["median"] / out["parent"]["median"], 4)
    out["this_outside_parent_spread"] = bool(not out["parent"]["min"] <= out["this"]["median"] <= out["parent"]["max"])
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="write the JSON result here as well as to stdout")
    ap.add_argument("--no-step", action="store_true", help="kernel part only")
    ap.add_argument("--steps-per-sample", type=int, default=3)
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit, for comparison (c)")
    ap.add_argument("--bench-steps", type=int, default=20)
    ap.add_argument("--bench-warmup", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    torch.cuda.set_device(0)
    res = {"device": torch.cuda.get_device_name(0)}
    res["kernels"] = [kernel_part(16384, 513), kernel_part(32768, 8193)]
    torch.cuda.empty_cache()
    if not args.no_step:
        res["config2_step"] = step_part(args.steps_per_sample)
        ops.check_index_flag(torch.device("cuda", 0), "ce_soft_bench")
    if args.parent_root:
        torch.cuda.empty_cache()
        res["bench_py"] = bench_part(args.parent_root, args.bench_steps, args.bench_warmup)
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
