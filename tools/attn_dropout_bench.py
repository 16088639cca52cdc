"""Cost of attention-probability dropout in the fused attention kernels (csrc/attention.hip, DROP = true).
Three comparisons, each with its arms alternating in one process, medians of 7 after warm-up.  Nothing is gated: the
numbers are recorded as measured.

(a) the launches at config 2's attention shape (64 sequences of 256 tokens, 64 heads of 8, causal), plain against
    dropout at p = 0.1: the forward launch, and the backward call (its dQ launch followed by its dK/dV launch) between
    device events.  The C ABI issues the two backward launches from one call, so events see their sum; --loop N runs N
    plain and N dropout calls of each and nothing else, for a kernel-trace profiler to split the two launches by name
    (the recorded split: profiles/r28_attn_dropout_kernel_stats.csv).
(b) the config-2 step (bench.py's model builder), pipeline.train_step on two copies of the model, attention dropout
    off (p = 0: the default path) and p = 0.1.
(c) with --parent-root DIR (a built checkout of the parent commit): bench.py --gpus 1 as a child process, this
    tree's and the parent's alternating, three runs each.  The default step runs the same kernel instantiations in
    both, so a difference beyond the parent's own spread is a finding.

    python tools/attn_dropout_bench.py --parent-root ../parent --out profiles/r28_attn_dropout.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
for p in (ROOT, os.path.join(ROOT, "quantized-autoregression-image-generator_amd")):
    sys.path.insert(0, os.path.abspath(p))

import bench  # noqa: E402
from qarig import ops, pipeline  # noqa: E402
from qarig.dropout import DropoutKey, threshold_and_scale  # noqa: E402
from qarig.optim import FlatAdam  # noqa: E402

REPS = 7
P = 0.1
SHAPE = dict(N=64, S=256, H=64, d=8)


def timed(fn, launches):
    """Microseconds per call of fn: device events around `launches` back-to-back calls."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / launches


def _forms():
    N, S, H, d = (SHAPE[k] for k in ("N", "S", "H", "d"))
    g = torch.Generator(device="cuda").manual_seed(0)
    q, k, v, do = (torch.randn((N, S, H * d), device="cuda", generator=g) for _ in range(4))
    key = DropoutKey(0x5EED, 0, q.device)
    key.set_step(1)
    drop = (*threshold_and_scale(P), 0, key.buffer)
    o, lse = ops.attention_fwd(q, k, v, H, True)
    od, lsed = ops.attention_fwd(q, k, v, H, True, dropout=drop)
    return {"fwd_plain": lambda: ops.attention_fwd(q, k, v, H, True),
            "fwd_dropout": lambda: ops.attention_fwd(q, k, v, H, True, dropout=drop),
            "bwd_plain": lambda: ops.attention_bwd(q, k, v, o, do, lse, H, True),
            "bwd_dropout": lambda: ops.attention_bwd(q, k, v, od, do, lsed, H, True, dropout=drop)}


def kernel_part(launches=20):
    forms = _forms()
    for fn in forms.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for _ in range(REPS):
        for k, fn in forms.items():
            times[k].append(timed(fn, launches))
    out = dict(SHAPE, causal=True, p=P, launches_per_sample=launches, samples=REPS,
               note="bwd = the dQ launch followed by the dK/dV launch (one C-ABI call)")
    for k, ts in times.items():
        out[k] = {"us_median": round(statistics.median(ts), 2), "us_min": round(min(ts), 2),
                  "us_max": round(max(ts), 2), "us_samples": [round(v, 2) for v in ts]}
    for part in ("fwd", "bwd"):
        out[f"{part}_dropout_over_plain"] = round(out[f"{part}_dropout"]["us_median"] /
                                                  out[f"{part}_plain"]["us_median"], 4)
    return out


def loop_part(n):
    """n calls of each form and nothing else: run under a kernel-trace profiler to time the launches by name."""
    forms = _forms()
    for _ in range(n):
        for fn in forms.values():
            fn()
    torch.cuda.synchronize()


def step_part(steps_per_sample):
    cfg = dict(bench.CFG)
    dev = torch.device("cuda", torch.cuda.current_device())
    C, H, W = cfg["latent"]
    z = torch.tanh(torch.randn((cfg["batch"], C, H, W), generator=torch.Generator().manual_seed(1))).to(dev)
    seq = (H // cfg["hr_patch"]) * (W // cfg["hr_patch"]) + 1
    nwin = pipeline.num_windows(seq, cfg["window"])
    rng = torch.Generator().manual_seed(4)
    arms, sites = {}, 0
    for name, p in (("off", 0.0), ("on", P)):
        lr_cb, hr_cb, model = bench.build_models(dev, cfg)
        model.train()
        opt = FlatAdam(model.parameters(), lr=cfg["lr"], betas=(0.5, 0.999))
        model.enable_attention_dropout(p, 0x5EED)
        if p:
            sites = len(model._attention_layers())

        def fn(lr_cb=lr_cb, hr_cb=hr_cb, model=model, opt=opt):
            rand = torch.randint(0, nwin, (cfg["batch"],), generator=rng)
            hr_in, lr_in, hr_tg, pos = pipeline.tokenize_window(z, lr_cb, hr_cb, cfg["base"], cfg["window"], rand)
            return pipeline.train_step(model, opt, hr_in, lr_in, hr_tg, pos, dp=False, pos_bound=seq)
        arms[name] = fn
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
    out = {"workload": cfg["name"], "steps_per_sample": steps_per_sample, "samples": REPS, "p": P,
           "tokens_per_step": cfg["batch"] * cfg["window"], "attention_sites": sites,
           "last_loss_off": float(last["off"].detach()), "last_loss_on": float(last["on"].detach())}
    for k, ts in times.items():
        med = statistics.median(ts)
        out[k] = {"ms_median": round(med, 3), "ms_min": round(min(ts), 3), "ms_max": round(max(ts), 3),
                  "ms_samples": [round(v, 3) for v in ts]}
    out["on_minus_off_ms"] = round(out["on"]["ms_median"] - out["off"]["ms_median"], 3)
    out["on_over_off"] = round(out["on"]["ms_median"] / out["off"]["ms_median"], 4)
    return out


def bench_part(parent_root, steps, warmup, runs=3):
    """bench.py as a child process (a fresh process per run), this tree's and the parent checkout's alternating."""
    arms = {"this": ROOT, "parent": os.path.abspath(parent_root)}
    vals = {k: [] for k in arms}
    for _ in range(runs):
        for k, root in arms.items():
            r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", str(steps),
                                "--warmup", str(warmup)], cwd=root, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                raise RuntimeError(f"bench.py ({k}) failed:\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
            vals[k].append(json.loads(line)["ms_per_step"])
    out = {"steps": steps, "warmup": warmup, "runs_each": runs}
    for k, v in vals.items():
        out[k] = {"ms_per_step": v, "median": statistics.median(v), "min": min(v), "max": max(v)}
    out["this_over_parent"] = round(out["this"]["median"] / out["parent"]["median"], 4)
    out["this_outside_parent_spread"] = bool(not out["parent"]["min"] <= out["this"]["median"] <= out["parent"]["max"])
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="write the JSON result here as well as to stdout")
    ap.add_argument("--no-step", action="store_true", help="skip the config-2 step comparison")
    ap.add_argument("--steps-per-sample", type=int, default=3)
    ap.add_argument("--loop", type=int, default=0, help="only run this many calls of each form (for a profiler)")
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit, for comparison (c)")
    ap.add_argument("--bench-steps", type=int, default=10)
    ap.add_argument("--bench-warmup", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    torch.cuda.set_device(0)
    if args.loop:
        loop_part(args.loop)
        return
    res = {"device": torch.cuda.get_device_name(0), "kernels": kernel_part()}
    torch.cuda.empty_cache()
    if not args.no_step:
        res["config2_step"] = step_part(args.steps_per_sample)
        ops.check_index_flag(torch.device("cuda", 0), "attn_dropout_bench")
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
