"""Cost of the EMA fused into the Adam launch (csrc/optim.hip qarig_adam_ema_step) against the plain launch
(qarig_adam_step), and of a config-2 train step with the EMA on against off.

Kernel part: both launches alternate in one process on the same buffers, at the config-2 model's parameter count
and at 8 Mi elements; medians of 7 after warm-up; achieved GB/s from the bytes each form has to move (plain:
read p g m v, write p m v = 7 streams; EMA: + read and write ema = 9 streams of 4 n bytes).  --other-lib PATH adds
the plain launch of another build of the library (the parent commit's) to the same alternation.

Step part: bench.py's own model builder and pipeline.train_step, two optimizers (EMA on / off) over two copies of
the config-2 model, alternating.

    python tools/adam_ema_bench.py --out profiles/r17_adam_ema.json
"""
import argparse
import ctypes
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


def kernel_part(n, other_lib):
    g = torch.Generator(device="cuda").manual_seed(0)
    p, grad, ema = (torch.randn(n, device="cuda", generator=g) * 0.05 for _ in range(3))
    m = torch.zeros(n, device="cuda")
    v = torch.zeros(n, device="cuda")
    lib, s = _lib.load(), _lib.stream()
    P = ctypes.c_void_p
    common = (0.5, 0.999, 1e-8, 1e-4, 0.0316)

    def plain(h):
        return lambda: h.qarig_adam_step(p.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(), n, *common, 1.0,
                                         None, None, s)

    forms = {"plain": plain(lib),
             "ema": lambda: lib.qarig_adam_ema_step(p.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(),
                                                    ema.data_ptr(), n, *common, 0.001, 1.0, None, None, s)}
    if other_lib:
        h = ctypes.CDLL(os.path.abspath(other_lib))
        F = ctypes.c_float
        h.qarig_adam_step.restype = ctypes.c_int
        h.qarig_adam_step.argtypes = [P, P, P, P, ctypes.c_int64, F, F, F, F, F, F, P, P, P]
        forms["plain_other_lib"] = plain(h)
    launches = max(3, min(50, (1 << 29) // n))
    for fn in forms.values():
        for _ in range(3):
            assert fn() == 0
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for _ in range(REPS):
        for k, fn in forms.items():
            times[k].append(timed(fn, launches))
    out = {"n": n, "launches_per_sample": launches, "samples": REPS}
    for k, ts in times.items():
        streams = 9 if k == "ema" else 7
        med = statistics.median(ts)
        out[k] = {"us_median": round(med, 2), "us_min": round(min(ts), 2), "us_max": round(max(ts), 2),
                  "streams": streams, "GBps": round(streams * 4 * n / med * 1e-3, 1)}
    out["ema_over_plain"] = round(out["ema"]["us_median"] / out["plain"]["us_median"], 4)
    out["predicted_from_bytes"] = round(9 / 7, 4)
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
            opt.enable_ema(0.999)
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
    n = runs["on"][3].total
    out = {"workload": cfg["name"], "parameters": n, "steps_per_sample": steps_per_sample, "samples": REPS}
    for k, ts in times.items():
        out["ema_" + k] = {"ms_median": round(statistics.median(ts), 3), "ms_min": round(min(ts), 3),
                           "ms_max": round(max(ts), 3)}
    out["on_minus_off_ms"] = round(out["ema_on"]["ms_median"] - out["ema_off"]["ms_median"], 3)
    out["extra_bytes_per_step_GB"] = round(2 * 4 * n * 1e-9, 3)
    return out, n


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="write the JSON result here as well as to stdout")
    ap.add_argument("--other-lib", default=None, help="another build of the library: its plain launch joins the alternation")
    ap.add_argument("--no-step", action="store_true", help="kernel part only (at 78.2 M and 8 Mi elements)")
    ap.add_argument("--steps-per-sample", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    torch.cuda.set_device(0)
    res = {"device": torch.cuda.get_device_name(0)}
    n_model = 78_200_000
    if not args.no_step:
        res["config2_step"], n_model = step_part(args.steps_per_sample)
        torch.cuda.empty_cache()
    res["kernel"] = [kernel_part(n, args.other_lib) for n in (n_model, 8 * 1024 * 1024)]
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
