"""Cost of token noise (csrc/embed.hip assemble_tokens_noise_kernel / token_noise_kernel).  Comparisons
with their arms alternating in one process, medians of 7 after warm-up.  Nothing is gated: the numbers are recorded
as measured.

(a) the assembling launch at config 2's shape (64 samples, one lr token and 256 hr tokens, base model, windows of 256),
    plain against noise at p = 0.1 with neighbour range 0 and 4, and the whole-tensor launch on 64 x 256 lr-like
    tokens, between device events.
(b) the config-2 step (bench.py's model builder: a base stage, so the input stream alone), pipeline.train_step on two
    copies of the model, token noise off (the default path) and p = 0.1.
(c) with --parent-root DIR (a built checkout of the parent commit): bench.py --gpus 1 as a child process, this
    tree's and the parent's alternating, three runs each.  The default step makes the same calls in both, so a
    difference beyond the parent's own spread is a finding.

    python tools/token_noise_bench.py --parent-root ../parent --out profiles/r31_token_noise.json
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
RANGE = 4


def timed(fn, launches):
    """Microseconds per call of fn: device events around `launches` back-to-back calls."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / launches


def kernel_part(launches=50):
    cfg = bench.CFG
    N, W, k_lr, k_hr = cfg["batch"], cfg["window"], cfg["k_lr"], cfg["k_hr"]
    S_hr = (cfg["latent"][1] // cfg["hr_patch"]) * (cfg["latent"][2] // cfg["hr_patch"])
    g = torch.Generator().manual_seed(0)
    lr = torch.randint(0, k_lr, (N, 1), generator=g).cuda()
    hr = torch.randint(0, k_hr, (N, S_hr), generator=g).cuda()
    offs = torch.randint(0, 1 + S_hr - W + 1, (N,), generator=g).cuda()
    key = DropoutKey(0x5EED, 0, hr.device)
    key.set_step(1)
    t = threshold_and_scale(P)[0]
    forms = {"assemble_plain": lambda: ops.assemble_tokens(lr, hr, True, k_lr, k_hr, offs, W),
             "assemble_noise": lambda: ops.assemble_tokens(lr, hr, True, k_lr, k_hr, offs, W, noise=(t, 0, key.buffer)),
             "assemble_noise_range": lambda: ops.assemble_tokens(lr, hr, True, k_lr, k_hr, offs, W,
                                                                 noise=(t, RANGE, key.buffer)),
             "token_noise": lambda: ops.token_noise(hr, k_hr, t, 0, 1, key.buffer)}
    for fn in forms.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for _ in range(REPS):
        for k, fn in forms.items():
            times[k].append(timed(fn, launches))
    out = dict(N=N, S_lr=1, S_hr=S_hr, window=W, base=True, p=P, range=RANGE, tokens_per_launch=N * W,
               token_noise_tokens=N * S_hr, launches_per_sample=launches, samples=REPS,
               note="each call allocates its outputs through the caching allocator, plain and noise alike")
    for k, ts in times.items():
        out[k] = {"us_median": round(statistics.median(ts), 2), "us_min": round(min(ts), 2),
                  "us_max": round(max(ts), 2), "us_samples": [round(v, 2) for v in ts]}
    out["noise_minus_plain_us"] = round(out["assemble_noise"]["us_median"] - out["assemble_plain"]["us_median"], 2)
    ops.check_index_flag(hr.device, "token_noise_bench")
    return out


def step_part(steps_per_sample):
    cfg = dict(bench.CFG)
    dev = torch.device("cuda", torch.cuda.current_device())
    C, H, W = cfg["latent"]
    z = torch.tanh(torch.randn((cfg["batch"], C, H, W), generator=torch.Generator().manual_seed(1))).to(dev)
    seq = (H // cfg["hr_patch"]) * (W // cfg["hr_patch"]) + 1
    nwin = pipeline.num_windows(seq, cfg["window"])
    rng = torch.Generator().manual_seed(4)
    arms = {}
    for name, p in (("off", 0.0), ("on", P)):
        lr_cb, hr_cb, model = bench.build_models(dev, cfg)
        model.train()
        opt = FlatAdam(model.parameters(), lr=cfg["lr"], betas=(0.5, 0.999))
        model.enable_token_noise(p, 0.0, 0x5EED, neighbour_range=RANGE)

        def fn(lr_cb=lr_cb, hr_cb=hr_cb, model=model, opt=opt):
            rand = torch.randint(0, nwin, (cfg["batch"],), generator=rng)
            if model.token_noise is not None:
                pipeline.set_dropout_step(model, opt)
            hr_in, lr_in, hr_tg, pos = pipeline.tokenize_window(z, lr_cb, hr_cb, cfg["base"], cfg["window"], rand,
                                                                token_noise=model.token_noise)
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
    out = {"workload": cfg["name"], "steps_per_sample": steps_per_sample, "samples": REPS, "p_input": P,
           "range": RANGE, "tokens_per_step": cfg["batch"] * cfg["window"],
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
    ap.add_argument("--no-step", action="store_true", help="skip the config-2 step comparison")
    ap.add_argument("--steps-per-sample", type=int, default=3)
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit, for comparison (c)")
    ap.add_argument("--bench-steps", type=int, default=10)
    ap.add_argument("--bench-warmup", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    torch.cuda.set_device(0)
    res = {"device": torch.cuda.get_device_name(0), "kernels": kernel_part()}
    torch.cuda.empty_cache()
    if not args.no_step:
        res["config2_step"] = step_part(args.steps_per_sample)
        ops.check_index_flag(torch.device("cuda", 0), "token_noise_bench")
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
