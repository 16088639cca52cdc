"""Cost of the AdamW launch (csrc/optim.hip qarig_adamw_step: groups of 8 elements, 16-byte accesses, one mask byte
per group) against the plain launches (qarig_adam_step / qarig_adam_ema_step: 4 bytes per access), and of a
config-2 train step with weight decay on against off.  Nothing is gated: the figures are recorded.

Kernel part: all eight launches alternate in one process on the same buffers -- plain Adam and AdamW with a mask
of zeros, a mask of ones and the config-2 model's real mask (the `weight` of every nn.Linear), each without and
with the EMA -- at the config-2 model's parameter count and at 8 Mi elements (there the real mask is the model's,
cut to size); medians of 7 after warm-up; achieved GB/s from the bytes each form has to move (7 streams of 4 n
bytes, 9 with the EMA, plus n / 8 mask bytes for AdamW).

Step part: bench.py's own model builder and pipeline.train_step, two optimizers (weight decay on / off) over two
copies of the config-2 model, alternating.

    python tools/adamw_bench.py --out profiles/r25_adamw.json
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
from qarig import _lib, pipeline  # noqa: E402
from qarig.optim import FlatAdam, decay_parameters  # noqa: E402

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


def kernel_part(n, real_mask):
    g = torch.Generator(device="cuda").manual_seed(0)
    p, grad, ema = (torch.randn(n, device="cuda", generator=g) * 0.05 for _ in range(3))
    m = torch.zeros(n, device="cuda")
    v = torch.zeros(n, device="cuda")
    groups = (n + 7) // 8
    masks = {"mask0": torch.zeros(groups, dtype=torch.uint8, device="cuda"),
             "mask1": torch.ones(groups, dtype=torch.uint8, device="cuda"),
             "real": real_mask[:groups].contiguous()}
    assert masks["real"].numel() == groups
    lib, s = _lib.load(), _lib.stream()
    common = (0.5, 0.999, 1e-8, 1e-4, 0.0316)
    ptrs = (p.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr())

    def adamw(mask, e):
        return lambda: lib.qarig_adamw_step(*ptrs, e, mask.data_ptr(), n, *common, 0.001, 1e-6, 1.0, None, None, s)

    forms = {"adam": lambda: lib.qarig_adam_step(*ptrs, n, *common, 1.0, None, None, s),
             "adam_ema": lambda: lib.qarig_adam_ema_step(*ptrs, ema.data_ptr(), n, *common, 0.001, 1.0, None, None, s)}
    for name, mask in masks.items():
        forms["adamw_" + name] = adamw(mask, None)
        forms["adamw_ema_" + name] = adamw(mask, ema.data_ptr())
    launches = max(3, min(50, (1 << 29) // n))
    for fn in forms.values():
        for _ in range(3):
            assert fn() == 0
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for _ in range(REPS):
        for k, fn in forms.items():
            times[k].append(timed(fn, launches))
    out = {"n": n, "launches_per_sample": launches, "samples": REPS,
           "real_mask_decayed_fraction": round(float((masks["real"] != 0).float().mean()), 4)}
    for k, ts in times.items():
        nbytes = (9 if "ema" in k else 7) * 4 * n + (groups if k.startswith("adamw") else 0)
        med = statistics.median(ts)
        out[k] = {"us_median": round(med, 2), "us_min": round(min(ts), 2), "us_max": round(max(ts), 2),
                  "bytes": nbytes, "GBps": round(nbytes / med * 1e-3, 1)}
    for k in list(times):
        if k.startswith("adamw"):
            base = "adam_ema" if "ema" in k else "adam"
            out[k]["over_" + base] = round(out[k]["us_median"] / out[base]["us_median"], 4)
    return out


def step_part(steps_per_sample):
    cfg = dict(bench.CFG)
    dev = torch.device("cuda", torch.cuda.current_device())
    C, H, W = cfg["latent"]
    z = torch.tanh(torch.randn((cfg["batch"], C, H, W), generator=torch.Generator().manual_seed(1))).to(dev)
    seq = (H // cfg["hr_patch"]) * (W // cfg["hr_patch"]) + 1
    nwin = pipeline.num_windows(seq, cfg["window"])
    rng = torch.Generator().manual_seed(4)
    runs = {}
    for name in ("off", "on"):
        lr_cb, hr_cb, model = bench.build_models(dev, cfg)
        opt = FlatAdam(model.parameters(), lr=cfg["lr"], betas=(0.5, 0.999))
        if name == "on":
            opt.enable_weight_decay(0.01, decay_parameters(model))
        runs[name] = (lr_cb, hr_cb, model, opt)

    def step(name):
        lr_cb, hr_cb, model, opt = runs[name]
        rand = torch.randint(0, nwin, (cfg["batch"],), generator=rng)
        hr_in, lr_in, hr_tg, pos = pipeline.tokenize_window(z, lr_cb, hr_cb, cfg["base"], cfg["window"], rand)
        return pipeline.train_step(model, opt, hr_in, lr_in, hr_tg, pos, dp=False, pos_bound=seq)

    for name in runs:
        for _ in range(2):
            step(name)
    torch.cuda.synchronize()
    times = {k: [] for k in runs}
    for _ in range(REPS):
        for name in runs:
            t0 = time.perf_counter()
            for _ in range(steps_per_sample):
                step(name)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / steps_per_sample * 1e3)
    opt = runs["on"][3]
    out = {"workload": cfg["name"], "parameters": opt.total, "steps_per_sample": steps_per_sample, "samples": REPS}
    for k, ts in times.items():
        out["decay_" + k] = {"ms_median": round(statistics.median(ts), 3), "ms_min": round(min(ts), 3),
                             "ms_max": round(max(ts), 3)}
    out["on_minus_off_ms"] = round(out["decay_on"]["ms_median"] - out["decay_off"]["ms_median"], 3)
    out["extra_bytes_per_step_MB"] = round(opt.total / 8 * 1e-6, 2)
    return out, opt.total, opt.decay_mask.clone()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="write the JSON result here as well as to stdout")
    ap.add_argument("--steps-per-sample", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    torch.cuda.set_device(0)
    res = {"device": torch.cuda.get_device_name(0)}
    res["config2_step"], n_model, mask = step_part(args.steps_per_sample)
    torch.cuda.empty_cache()
    res["kernel"] = [kernel_part(n, mask) for n in (n_model, 8 * 1024 * 1024)]
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
