"""Cost of global-norm gradient clipping (csrc/optim.hip): qarig_grad_clip_coef (the streaming fp64 sum of squares
and the one-workgroup second stage) against the bytes it reads, qarig_adam_clip_step against qarig_adamw_step and
qarig_adam_step / qarig_adam_ema_step, and a config-2 train step with the clip on against off.  Nothing is gated:
the figures are recorded.

Kernel part: all launches alternate in one process on the same buffers, at the config-2 model's parameter count and
at 8 Mi elements; medians of 7 after warm-up, device events around back-to-back launches.  grad_clip_coef moves
4 n bytes (its partials are kilobytes); the Adam forms 7 streams of 4 n bytes, 9 with the EMA, plus n / 8 mask
bytes where a mask is given.  clip_state holds a finite norm and coef = 1 for the Adam arms (the arithmetic of a
clipped step is the same instructions).

Step part: bench.py's own model builder and pipeline.train_step, two optimizers (clip on / off) over two copies of
the config-2 model, alternating.

    python tools/grad_clip_bench.py --out profiles/r27_grad_clip.json
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
from qarig import _lib, ops, pipeline  # noqa: E402
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


def kernel_part(n):
    g = torch.Generator(device="cuda").manual_seed(0)
    p, grad, ema = (torch.randn(n, device="cuda", generator=g) * 0.05 for _ in range(3))
    m = torch.zeros(n, device="cuda")
    v = torch.zeros(n, device="cuda")
    groups = (n + 7) // 8
    mask = torch.zeros(groups, dtype=torch.uint8, device="cuda")
    mask[::2] = 1
    partials = torch.zeros(ops.GRAD_NORM_PARTIALS, dtype=torch.float64, device="cuda")
    state = torch.zeros(4, dtype=torch.float64, device="cuda")
    fixed = torch.tensor([1.0, 1.0, 0.0, 0.0], dtype=torch.float64, device="cuda")
    lib, s = _lib.load(), _lib.stream()
    common = (0.5, 0.999, 1e-8, 1e-4, 0.0316)
    ptrs = (p.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr())

    def clip(e, mk):
        return lambda: lib.qarig_adam_clip_step(*ptrs, e, mk, n, *common, 0.001, 1e-6, 1.0, None, None,
                                                fixed.data_ptr(), s)

    forms = {"grad_clip_coef": lambda: lib.qarig_grad_clip_coef(grad.data_ptr(), n, 1.0, 1.0, partials.data_ptr(),
                                                                state.data_ptr(), s),
             "adam": lambda: lib.qarig_adam_step(*ptrs, n, *common, 1.0, None, None, s),
             "adam_ema": lambda: lib.qarig_adam_ema_step(*ptrs, ema.data_ptr(), n, *common, 0.001, 1.0, None, None, s),
             "adamw": lambda: lib.qarig_adamw_step(*ptrs, None, mask.data_ptr(), n, *common, 0.001, 1e-6, 1.0, None,
                                                   None, s),
             "adamw_ema": lambda: lib.qarig_adamw_step(*ptrs, ema.data_ptr(), mask.data_ptr(), n, *common, 0.001,
                                                       1e-6, 1.0, None, None, s),
             "adam_clip": clip(None, None), "adam_clip_ema": clip(ema.data_ptr(), None),
             "adam_clip_mask": clip(None, mask.data_ptr()), "adam_clip_ema_mask": clip(ema.data_ptr(), mask.data_ptr())}
    launches = max(3, min(50, (1 << 29) // n))
    for fn in forms.values():
        for _ in range(3):
            assert fn() == 0
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for _ in range(REPS):
        for k, fn in forms.items():
            times[k].append(timed(fn, launches))
    out = {"n": n, "launches_per_sample": launches, "samples": REPS, "norm": state.tolist()[0]}
    for k, ts in times.items():
        if k == "grad_clip_coef":
            nbytes = 4 * n
        else:
            nbytes = (9 if "ema" in k else 7) * 4 * n + (groups if ("mask" in k or k.startswith("adamw")) else 0)
        med = statistics.median(ts)
        out[k] = {"us_median": round(med, 2), "us_min": round(min(ts), 2), "us_max": round(max(ts), 2),
                  "bytes": nbytes, "GBps": round(nbytes / med * 1e-3, 1)}
    for k, base in (("adam_clip", "adam"), ("adam_clip_ema", "adam_ema"), ("adam_clip_mask", "adamw"),
                    ("adam_clip_ema_mask", "adamw_ema")):
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
            opt.enable_grad_clip(1.0)
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
    out = {"workload": cfg["name"], "parameters": opt.total, "steps_per_sample": steps_per_sample, "samples": REPS,
           "clip_stats_after": opt.clip_stats()}
    for k, ts in times.items():
        out["clip_" + k] = {"ms_median": round(statistics.median(ts), 3), "ms_min": round(min(ts), 3),
                            "ms_max": round(max(ts), 3)}
    out["on_minus_off_ms"] = round(out["clip_on"]["ms_median"] - out["clip_off"]["ms_median"], 3)
    out["extra_bytes_per_step_MB"] = round(opt.total * 4 * 1e-6, 2)
    return out, opt.total


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="write the JSON result here as well as to stdout")
    ap.add_argument("--steps-per-sample", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    torch.cuda.set_device(0)
    res = {"device": torch.cuda.get_device_name(0)}
    res["config2_step"], n_model = step_part(args.steps_per_sample)
    torch.cuda.empty_cache()
    res["kernel"] = [kernel_part(n) for n in (n_model, 8 * 1024 * 1024)]
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
