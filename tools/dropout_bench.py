"""Cost of the counter-based dropout (csrc/dropout.hip); two comparisons, each with its arms alternating in one
process, medians of 7 after warm-up, device events around the kernel launches.  Nothing is gated: the numbers are
recorded as measured.

(a) the launch at 16,384 x 512 = 8 Mi elements (one site of config 2: 64 windows of 256 tokens, width 512; 32 MiB
    per tensor, so input and output can live in the 256 MiB last-level cache between back-to-back launches) and at
    64 Mi elements (256 MiB per tensor: input and output together are twice that cache), against ops.mul_fwd
    (csrc/elementwise.hip, y = a * b) of the same size.  GB/s counts the compulsory traffic:
    dropout reads x and writes y (8 bytes per element), mul_fwd reads a and b and writes y (12 bytes).  Dropout also
    runs one Philox4x32-10 call (20 32-bit multiplies giving high and low halves) per 8 elements; if its GB/s
    stays at mul_fwd's the launch is bandwidth-bound, if it falls clearly below, the integer multiplies show.
    Also timed: the launch on a base 4 bytes off 16 (the element-by-element path) and in place.
(b) the config-2 step (bench.py's model builder), pipeline.train_step on two copies of the model, dropout off
    (p = 0: the default path) and p = 0.1.

    python tools/dropout_bench.py --out profiles/r24_dropout.json
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
from qarig import ops, pipeline  # noqa: E402
from qarig.dropout import DropoutKey, threshold_and_scale  # noqa: E402
from qarig.optim import FlatAdam  # noqa: E402

REPS = 7
P = 0.1


def timed(fn, launches):
    """Microseconds per call of fn: device events around `launches` back-to-back calls."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / launches


def kernel_part(n):
    g = torch.Generator(device="cuda").manual_seed(0)
    buf = torch.randn(n + 4, device="cuda", generator=g)
    x, x_off = buf[:n], buf[1:n + 1]
    b = torch.randn(n, device="cuda", generator=g)
    y = torch.empty(n + 4, device="cuda")
    inplace = x.clone()
    key = DropoutKey(0x5EED, 0, x.device)
    key.set_step(1)
    t, s = threshold_and_scale(P)
    forms = {"mul_fwd": (lambda: ops.mul_fwd(x, b), 12),
             "dropout": (lambda: ops.dropout(x, t, s, 0, key.buffer, out=y[:n]), 8),
             "dropout_unaligned": (lambda: ops.dropout(x_off, t, s, 0, key.buffer, out=y[1:n + 1]), 8),
             "dropout_in_place": (lambda: ops.dropout(inplace, t, s, 0, key.buffer, out=inplace), 8)}
    launches = max(10, min(200, (1 << 30) // (8 * n)))
    for fn, _ in forms.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for _ in range(REPS):
        for k, (fn, _) in forms.items():
            times[k].append(timed(fn, launches))
    out = {"elements": n, "MB_per_tensor": round(4 * n * 1e-6, 1), "launches_per_sample": launches, "samples": REPS,
           "p": P, "threshold": t}
    for k, ts in times.items():
        med = statistics.median(ts)
        out[k] = {"us_median": round(med, 2), "us_min": round(min(ts), 2), "us_max": round(max(ts), 2),
                  "us_samples": [round(v, 2) for v in ts], "bytes_per_element": forms[k][1],
                  "GBps": round(forms[k][1] * n / med * 1e-3, 1)}
    out["dropout_over_mul_fwd_time"] = round(out["dropout"]["us_median"] / out["mul_fwd"]["us_median"], 4)
    out["dropout_over_mul_fwd_GBps"] = round(out["dropout"]["GBps"] / out["mul_fwd"]["GBps"], 4)
    return out


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
        model.enable_dropout(p, 0x5EED)
        if p:
            sites = 2 + len(model._residual_layers()) - (0 if model.use_encoder else 1)

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
           "tokens_per_step": cfg["batch"] * cfg["window"], "dropout_sites": sites,
           "dropout_launches_per_step": 2 * sites,
           "last_loss_off": float(last["off"].detach()), "last_loss_on": float(last["on"].detach())}
    for k, ts in times.items():
        med = statistics.median(ts)
        out[k] = {"ms_median": round(med, 3), "ms_min": round(min(ts), 3), "ms_max": round(max(ts), 3),
                  "ms_samples": [round(v, 3) for v in ts]}
    out["on_minus_off_ms"] = round(out["on"]["ms_median"] - out["off"]["ms_median"], 3)
    out["on_over_off"] = round(out["on"]["ms_median"] / out["off"]["ms_median"], 4)
    out["on_slower_beyond_off_spread"] = bool(out["on"]["ms_median"] > out["off"]["ms_max"])
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="write the JSON result here as well as to stdout")
    ap.add_argument("--no-step", action="store_true", help="kernel part only")
    ap.add_argument("--steps-per-sample", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    torch.cuda.set_device(0)
    res = {"device": torch.cuda.get_device_name(0)}
    res["kernels"] = [kernel_part(16384 * 512), kernel_part(64 * 1024 * 1024)]
    torch.cuda.empty_cache()
    if not args.no_step:
        res["config2_step"] = step_part(args.steps_per_sample)
        ops.check_index_flag(torch.device("cuda", 0), "dropout_bench")
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
