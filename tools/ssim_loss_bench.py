"""Cost of training against SSIM (csrc/recon.hip ssim_tile_maps_kernel, ssim_bwd_kernel; QF.ssim_loss).

Kernel part: ops.ssim (tile launch + finishing launch) against ops.ssim_fwd_maps (the same two launches, the tile
launch also writing three fp64 maps) against ops.ssim_bwd (one launch), at 64 images of 3 x 64 x 64 and at 16 of
3 x 256 x 256; device events around back-to-back calls, the three arms alternating, medians of 7 after warm-up.
For the backward the bytes its maps make it read are given too: 3 x 8 B per valid position, once, and with the
halo every workgroup re-reads ((16 + taps - 1)^2 entries per map for 16 x 16 pixels).

Step part: the config-1 training step (tools/c1_autoencoder.py: README autoencoder, batch 4 of 3 x 64 x 64, MSE +
backward + Adam) with the loss of --ssim-weight 0 against --ssim-weight 0.5; host wall clock around synchronised
steps, the two arms alternating in one process, medians of 7.  Nothing is gated: the numbers are recorded.

    python tools/ssim_loss_bench.py --out profiles/r22_ssim_loss.json
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

from models.Autoencoder import Autoencoder  # noqa: E402
from qarig import functional as QF  # noqa: E402
from qarig import ops  # noqa: E402
from qarig.optim import FlatAdam  # noqa: E402

REPS = 7
TAPS = 11


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
    a = torch.tanh(torch.randn((N, C, H, W), device="cuda", generator=g))
    b = (a + 0.1 * torch.randn((N, C, H, W), device="cuda", generator=g)).clamp_(-1, 1)
    up = torch.full((N,), -1.0 / N, dtype=torch.float64, device="cuda")
    _, maps = ops.ssim_fwd_maps(a, b)
    forms = {"ssim": lambda: ops.ssim(a, b), "ssim_fwd_maps": lambda: ops.ssim_fwd_maps(a, b),
             "ssim_bwd": lambda: ops.ssim_bwd(a, b, maps, up)}
    for fn in forms.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for _ in range(REPS):
        for k, fn in forms.items():
            times[k].append(timed(fn, 20))
    oh, ow = H - TAPS + 1, W - TAPS + 1
    tiles = N * C * ((H + 15) // 16) * ((W + 15) // 16)
    out = {"images": N, "shape": [C, H, W], "launches_per_sample": 20, "samples": REPS,
           "maps_bytes": maps.numel() * 8, "bwd_halo_read_bytes": tiles * 3 * 8 * (16 + TAPS - 1) ** 2}
    for k, ts in times.items():
        out[k] = summary(ts)
    out["ssim_fwd_maps"]["over_ssim_us"] = round(out["ssim_fwd_maps"]["us_median"] - out["ssim"]["us_median"], 2)
    out["ssim_fwd_maps"]["maps_write_GBps"] = round(maps.numel() * 8 / out["ssim_fwd_maps"]["us_median"] * 1e-3, 1)
    # the halo entries past the valid region are not read: an upper bound on the bytes requested, most of them L2 hits
    out["ssim_bwd"]["maps_once_GBps"] = round(maps.numel() * 8 / out["ssim_bwd"]["us_median"] * 1e-3, 1)
    out["ssim_bwd"]["halo_GBps_upper"] = round(out["bwd_halo_read_bytes"] / out["ssim_bwd"]["us_median"] * 1e-3, 1)
    return out


def step_part(steps_per_sample):
    torch.manual_seed(3)
    m = Autoencoder(num_layers=2, image_channel=3, min_channel=256, max_channel=512, latent_channel=4).cuda()
    x = (torch.rand((4, 3, 64, 64), generator=torch.Generator().manual_seed(0)) * 2 - 1).cuda()
    opt = FlatAdam(m.parameters(), lr=1e-4, betas=(0.5, 0.999))

    def step(weight):
        opt.zero_grad()
        recon = m(x)
        if weight > 0:
            loss = QF.mse_loss(recon, x) + weight * QF.ssim_loss(recon, x)
        else:
            loss = QF.mse_loss(recon, x)
        loss.backward()
        opt.step()
        return loss

    arms = {"ssim_weight_0": lambda: step(0.0), "ssim_weight_0.5": lambda: step(0.5)}
    for fn in arms.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    for _ in range(REPS):
        for k, fn in arms.items():
            t0 = time.perf_counter()
            for _ in range(steps_per_sample):
                fn()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) / steps_per_sample * 1e6)
    out = {"shapes": "config 1: README autoencoder 256..512 channels, batch 4 of 3x64x64, MSE (+ 0.5 ssim_loss) + backward + Adam",
           "steps_per_sample": steps_per_sample, "samples": REPS, "timing": "host wall clock around synchronised steps"}
    for k, ts in times.items():
        out[k] = summary(ts)
    out["added_us"] = round(out["ssim_weight_0.5"]["us_median"] - out["ssim_weight_0"]["us_median"], 2)
    out["added_share_of_step"] = round(out["added_us"] / out["ssim_weight_0"]["us_median"], 4)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="write the JSON result here as well as to stdout")
    ap.add_argument("--steps-per-sample", type=int, default=10)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    torch.cuda.set_device(0)
    res = {"device": torch.cuda.get_device_name(0),
           "kernel": [kernel_part(64, 3, 64, 64), kernel_part(16, 3, 256, 256)],
           "step": step_part(args.steps_per_sample)}
    # the four SSIM launches of a step, back to back at its shape (device time; the step's figure is host time)
    res["step"]["ssim_launches_at_step_shape"] = kernel_part(4, 3, 64, 64)
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
