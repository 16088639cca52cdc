#!/usr/bin/env python3
"""The "mxfp8" mode against "bf16" (and "fp8") on BASELINE config 5 (run on the GPU box).

1. Per product, at the config-5 shapes of profiles/r03_c5_gemm_by_shape.txt (M = 32,768 tokens): the
   bf16 kernel (qarig_gemm_lp, operands already bf16) against the MX form -- the quantise pass(es) of the
   activation operand(s) from fp32 plus qarig_gemm_mx (weights quantised once per optimiser step, not
   counted) -- alternating in one process.  TF against the dense peaks of MI355X_MICROARCH.md.
2. The config-5 shard train step (bench.build_models, bench.CFG_C5, eager) in "bf16", "fp8" and
   "mxfp8", alternating on one model: ms/step and loss.

Prints one line per measurement; --json writes them to a file as well.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "quantized-autoregression-image-generator_amd")):
    sys.path.insert(0, p)
import torch  # noqa: E402

PEAK_BF16, PEAK_F8 = 2500.0, 5000.0      # dense TF, MI355X_MICROARCH.md (bench.py uses the same bf16 figure)
M = 32768
# name, bf16 layout (0 NT fwd, 2 NN dgrad, 1 TN wgrad), product M, N, K, bf16 splitk, and whether the node holds
# the activation operand(s) the MX form quantises in bf16 (h and dT1 come from GEMM epilogues) or fp32
PRODUCTS = [
    ("fwd 512->2048", 0, M, 2048, 512, 1, ("f32",)),
    ("fwd 2048->512", 0, M, 512, 2048, 1, ("bf16",)),
    ("dgrad 2048<-512", 2, M, 2048, 512, 1, ("f32",)),
    ("dgrad 512<-2048", 2, M, 512, 2048, 1, ("bf16",)),
    ("wgrad 2048x512", 1, 2048, 512, M, 16, ("bf16", "f32")),
    ("wgrad 512x2048", 1, 512, 2048, M, 16, ("f32", "bf16")),
    ("classifier fwd", 0, M, 8320, 2048, 1, ("bf16",)),
]


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3      # us


def products(out, reps, rounds):
    from qarig import functional_lp as FL
    from qarig import ops
    g = torch.Generator(device="cuda").manual_seed(0)
    for name, layout, m, n, k, sk, srcs in PRODUCTS:
        if layout == 1:       # dW (m, n) = dT^T x over k tokens: the activations lie (k, m) and (k, n)
            a32 = torch.randn((k, m), device="cuda", generator=g)
            b32 = torch.randn((k, n), device="cuda", generator=g)
        else:
            a32 = torch.randn((m, k), device="cuda", generator=g)
            b32 = torch.randn((n, k) if layout == 0 else (k, n), device="cuda", generator=g)
        ab, bb = ops.cast_bf16(a32), ops.cast_bf16(b32)
        C = torch.empty((m, n), device="cuda")
        if layout == 0:
            mx_b, _ = ops.mx_quant(b32)
        elif layout == 2:
            _, mx_b = ops.mx_quant(b32, row=False, transposed=True)      # the weight's transposed form
        mx_sk = FL._mx_splitk((m // 128) * (n // 128), k) if layout == 1 else 1
        a_src = ab if srcs[0] == "bf16" else a32
        if layout == 1:
            b_src = bb if srcs[1] == "bf16" else b32

            def quant():
                return (ops.mx_quant(a_src, row=False, transposed=True)[1],
                        ops.mx_quant(b_src, row=False, transposed=True)[1])
        else:
            def quant():
                return ops.mx_quant(a_src)[0], mx_b
        qa, qb = quant()

        def bf16():
            ops.gemm_lp(ab, bb, layout, m, n, k, C=C, splitk=sk)

        def mx():
            ops.gemm_mx(qa, qb, m, n, k, C=C, splitk=mx_sk)

        bf16(), mx(), quant()
        torch.cuda.synchronize()
        best = {"bf16": 1e30, "mx": 1e30, "quant": 1e30}
        for _ in range(rounds):
            best["bf16"] = min(best["bf16"], timed(bf16, reps))
            best["mx"] = min(best["mx"], timed(mx, reps))
            best["quant"] = min(best["quant"], timed(quant, reps))
        fl = 2.0 * m * n * k
        rec = dict(kind="product", name=name, M=m, N=n, K=k, quant_from=list(srcs), bf16_splitk=sk, mx_splitk=mx_sk,
                   bf16_us=round(best["bf16"], 1), mx_gemm_us=round(best["mx"], 1),
                   mx_quant_us=round(best["quant"], 1), mx_total_us=round(best["mx"] + best["quant"], 1),
                   bf16_tf=round(fl / best["bf16"] / 1e6, 1), mx_gemm_tf=round(fl / best["mx"] / 1e6, 1),
                   bf16_of_peak=round(fl / best["bf16"] / 1e6 / PEAK_BF16, 3),
                   mx_of_peak=round(fl / best["mx"] / 1e6 / PEAK_F8, 3),
                   speedup_gemm=round(best["bf16"] / best["mx"], 3),
                   speedup_with_quant=round(best["bf16"] / (best["mx"] + best["quant"]), 3))
        print(json.dumps(rec), flush=True)
        out.append(rec)
        del a32, b32, ab, bb, C, qa, qb, a_src
        torch.cuda.empty_cache()


def train_steps(out, steps, rounds, modes=("bf16", "fp8", "mxfp8")):
    import bench
    from qarig import ops, pipeline
    from qarig.optim import FlatAdam
    cfg = bench.CFG_C5
    device = torch.device("cuda", 0)
    lr_cb, hr_cb, model = bench.build_models(device, cfg)
    optim = FlatAdam(model.parameters(), lr=cfg["lr"], betas=(0.5, 0.999))
    C, H, W = cfg["latent"]
    g = torch.Generator().manual_seed(1)
    z = torch.tanh(torch.randn((cfg["batch"], C, H, W), generator=g)).to(device)
    seq = (H // cfg["hr_patch"]) * (W // cfg["hr_patch"]) + 1
    nwin = pipeline.num_windows(seq, cfg["window"])
    rng = torch.Generator().manual_seed(4)

    def step():
        rand = torch.randint(0, nwin, (cfg["batch"],), generator=rng)
        hr_in, lr_in, hr_tg, pos = pipeline.tokenize_window(z, lr_cb, hr_cb, cfg["base"], cfg["window"], rand)
        return pipeline.train_step(model, optim, hr_in, lr_in, hr_tg, pos, pos_bound=seq)

    old = ops.PRECISION
    res = {m: [] for m in modes}
    try:
        for m in modes:                   # warm-up: workspaces, caches
            ops.set_precision(m)
            step(), step()
        torch.cuda.synchronize()
        for _ in range(rounds):
            for m in modes:
                ops.set_precision(m)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(steps):
                    loss = step()
                torch.cuda.synchronize()
                res[m].append(((time.perf_counter() - t0) / steps * 1e3, float(loss)))
    finally:
        ops.set_precision(old)
    for m in modes:
        rec = dict(kind="train_step", config="c5", precision=m, steps_per_round=steps,
                   ms_per_step=[round(t, 2) for t, _ in res[m]], loss=[round(lv, 5) for _, lv in res[m]])
        print(json.dumps(rec), flush=True)
        out.append(rec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--skip-products", action="store_true")
    ap.add_argument("--skip-train", action="store_true")
    ap.add_argument("--modes", default="bf16,fp8,mxfp8", help="precisions of the train-step part, alternating")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    out = []
    if not args.skip_products:
        products(out, args.reps, args.rounds)
    if not args.skip_train:
        train_steps(out, args.steps, args.rounds, tuple(args.modes.split(",")))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
