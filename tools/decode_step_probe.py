#!/usr/bin/env python3
"""Single-token decode step of a README-size encoder-decoder stage (config 3, stage 3) in isolation:
ms per captured-graph replay (the device chain alone), per DecodeCache.step (with the host feeds) and
C-ABI launches per step: "table" = the per-position table of the cond projections + fused norms (what
generation runs), "fused" = per-token cond path + fused norms, "separate" = every norm its own launch.
    python tools/decode_step_probe.py [--rows 4] [--steps 200]
With --top-k / --top-p also the sampling draw of a step in isolation: microseconds per launch of the draw
kernel, unfiltered against filtered, in alternating blocks of back-to-back launches (--draw-vocab: V;
--draw-only skips the step measurements).
--decode-weights bf16 runs the step measurements with the weight-only bf16 step (kvcache.DECODE_WEIGHTS);
--weights-ab instead times the "table" step's graph replay with fp32 and bf16 weights alternating in one process
(7 rounds of --steps replays each: median, min, max) and reports the weight bytes a step streams in each mode,
counted from the shapes of its Linear layers.
--width / --heads choose the stage's shape (512 / 64, head dim 8, by default; 512 / 4 is head dim 128, 768 / 8 head
dim 96); --heads-ab H times the "table" step's graph replay at --heads against H heads of the same width, alternating
in one process (7 rounds of --steps replays each): the weight bytes of a step are the same, the attention launch
differs."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "quantized-autoregression-image-generator_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402
from bench_generate import build_stage_model  # noqa: E402
from qarig import kvcache, _lib  # noqa: E402


def probe_draw(rows, V, top_k, top_p, dev, launches=400, rounds=7):
    """us per launch of ops.decode_sample on (rows, V) logits: both filters off against (top_k, top_p), `rounds`
    alternating blocks of `launches` back-to-back launches each, timed with device events."""
    import statistics
    from qarig import ops
    g = torch.Generator().manual_seed(V)
    logits = (torch.randn((rows, V), generator=g) * 3).to(dev)
    uniforms = torch.rand((launches, rows), generator=g).to(dev)
    ctl = torch.zeros(ops.DECODE_CTL_WORDS, dtype=torch.int32, device=dev)
    ids = torch.zeros(rows, dtype=torch.int64, device=dev)
    chunk = torch.zeros((rows, 1), dtype=torch.int64, device=dev)
    comb = torch.ones(rows, device=dev)

    def block(k, p):
        comb.fill_(1.0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            ops.decode_sample(logits, 1.0, V - 1, True, 0, uniforms, ctl, 0, 1, ids, chunk, comb, top_k=k, top_p=p)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / launches * 1e3

    block(0, 1.0), block(top_k, top_p)              # code-object loads
    t = {"off": [], "filtered": []}
    for _ in range(rounds):
        t["off"].append(round(block(0, 1.0), 3))
        t["filtered"].append(round(block(top_k, top_p), 3))
    med = {k: statistics.median(v) for k, v in t.items()}
    return {"rows": rows, "V": V, "top_k": top_k, "top_p": top_p, "launches_per_block": launches,
            "us_per_launch": t, "median_us": med, "min_us": {k: min(v) for k, v in t.items()},
            "filtered_over_off": round(med["filtered"] / med["off"], 3)}


def streamed_weight_elements(cache):
    """Weight elements one step of `cache` streams: every Linear it evaluates per token (stacked q/k/v MLPs, the
    other two-layer MLPs, residual layers, classifier), from their shapes."""
    from models.layers import _lin_params
    mlps, res, classifier = cache._step_linears()
    n = sum(_lin_params(lin)[0].numel() for seq in mlps + [classifier] for lin in (seq[0], seq[1]))
    n += sum(_lin_params(r.linear)[0].numel() for r in res)
    for layer in cache.model.decoder_layers:
        at = layer.self_attn_block.self_attn
        n += sum(_lin_params(lin)[0].numel() for blk in (at.q_block, at.k_block, at.v_block) for lin in (blk[0], blk[1]))
    return n


def weights_ab(model, enc, B, S, positions, steps, rounds=7):
    """ms per graph replay of the "table" step, fp32 weights against bf16 weights: both caches captured first, then
    `rounds` alternating blocks of `steps` replays each."""
    import statistics
    caches = {w: kvcache.DecodeCache(model, enc, B, S, graph=True, positions=positions, weights=w)
              for w in kvcache.DECODE_WEIGHTS}
    ids = torch.zeros(B, dtype=torch.int64, device=caches["f32"].kv.device)
    for c in caches.values():
        for t in range(8):
            c.step(ids, None, t)
        c.ctl[0:1].fill_(S - 1)
    t = {w: [] for w in caches}
    for _ in range(rounds):
        for w, c in caches.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                c._graph.replay()
            torch.cuda.synchronize()
            t[w].append(round((time.perf_counter() - t0) / steps * 1e3, 4))
    n = streamed_weight_elements(caches["f32"])
    lp = caches["bf16"]._img is not None
    med = {w: statistics.median(v) for w, v in t.items()}
    return {"graph_replay_ms": t, "median_ms": med, "min_ms": {w: min(v) for w, v in t.items()},
            "max_ms": {w: max(v) for w, v in t.items()}, "bf16_over_f32": round(med["bf16"] / med["f32"], 4),
            "bf16_images_in_use": lp,
            "streamed_weight_bytes_per_step": {"f32": 4 * n, "bf16": (2 if lp else 4) * n}}


def heads_ab(models, encs, B, S, positions, steps, weights, rounds=7):
    """ms per graph replay of the "table" step for each of `models` (name -> model): all captured first, then
    `rounds` alternating blocks of `steps` replays each, the cache full (the longest attention)."""
    import statistics
    caches = {n: kvcache.DecodeCache(m, encs[n], B, S, graph=True, positions=positions, weights=weights)
              for n, m in models.items()}
    for c in caches.values():
        ids = torch.zeros(B, dtype=torch.int64, device=c.kv.device)
        for t in range(8):
            c.step(ids, None, t)
        c.ctl[0:1].fill_(S - 1)
    t = {n: [] for n in caches}
    for _ in range(rounds):
        for n, c in caches.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                c._graph.replay()
            torch.cuda.synchronize()
            t[n].append(round((time.perf_counter() - t0) / steps * 1e3, 4))
    med = {n: statistics.median(v) for n, v in t.items()}
    return {"graph_replay_ms": t, "median_ms": med, "min_ms": {n: min(v) for n, v in t.items()},
            "max_ms": {n: max(v) for n, v in t.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--base", action="store_true", help="decoder-only base stage")
    ap.add_argument("--opt", action="append", default=[], help="name=value kernel-selection option (qarig_set_option)")
    ap.add_argument("--top-k", type=int, default=0, help="draw probe: top-k filter (0: off)")
    ap.add_argument("--top-p", type=float, default=1.0, help="draw probe: nucleus filter (1: off)")
    ap.add_argument("--draw-vocab", type=int, action="append", default=[], help="draw probe: V (default 513); repeatable")
    ap.add_argument("--draw-only", action="store_true", help="only the draw probe")
    ap.add_argument("--decode-weights", choices=list(kvcache.DECODE_WEIGHTS), default="f32",
                    help="weights the step streams (bf16: weight-only, everything else fp32)")
    ap.add_argument("--weights-ab", action="store_true",
                    help="only the fp32 / bf16 weights A/B of the table step's graph replay")
    ap.add_argument("--width", type=int, default=512, help="model width (README: 512)")
    ap.add_argument("--heads", type=int, default=64, help="attention heads (README: 64, head dim 8)")
    ap.add_argument("--heads-ab", type=int, default=0, metavar="H",
                    help="only the A/B of the table step's graph replay at --heads against H heads, same width")
    args = ap.parse_args()
    if args.draw_only or args.top_k > 0 or args.top_p < 1.0:
        dev = torch.device("cuda", 0)
        draws = [probe_draw(args.rows, V, args.top_k, args.top_p, dev) for V in (args.draw_vocab or [513])]
        if args.draw_only:
            print(json.dumps({"draw": draws}))
            return
    else:
        draws = None
    for o in args.opt:
        k, v = o.split("=")
        _lib.load().qarig_set_option(k.encode(), int(v))
    dev = torch.device("cuda", 0)
    torch.manual_seed(1)
    K, B, S = 512, args.rows, 256
    model = build_stage_model(0 if args.base else 2, K, dev, args.width, args.heads)
    out = {"width": args.width, "heads": args.heads, "head_dim": args.width // args.heads, "rows": B, "window": S, "options": args.opt, "stage": "base" if args.base else "encoder-decoder", "steps": args.steps,
           "decode_weights": args.decode_weights}
    with torch.no_grad():
        enc = None if args.base else model.encode(torch.randint(0, K, (B, 64), device=dev))
        ids = torch.randint(0, K, (B,), device=dev)
        pos = torch.rand(B, device=dev) * 100
        positions = [0.0] + [float(i + 1) for i in range(1, S)]
        if args.heads_ab:
            other = build_stage_model(0 if args.base else 2, K, dev, args.width, args.heads_ab)
            names = {f"heads_{args.heads}_d{args.width // args.heads}": model,
                     f"heads_{args.heads_ab}_d{args.width // args.heads_ab}": other}
            lr = torch.randint(0, K, (B, 64), device=dev)
            encs = {n: None if args.base else m.encode(lr) for n, m in names.items()}
            out["heads_ab"] = heads_ab(names, encs, B, S, positions, args.steps, args.decode_weights)
            print(json.dumps(out))
            return
        if args.weights_ab:
            del out["decode_weights"]
            out["weights_ab"] = weights_ab(model, enc, B, S, positions, args.steps)
            print(json.dumps(out))
            return
        for name, fused, table in (("table", True, True), ("fused", True, False), ("separate", False, False)):
            kvcache.FUSE_NORMS = fused
            eager = kvcache.DecodeCache(model, enc, B, S, graph=False, positions=positions if table else None,
                                        weights=args.decode_weights)
            n0 = _lib.N_CALLS
            eager.step(ids, pos, 0)
            launches = _lib.N_CALLS - n0
            cache = kvcache.DecodeCache(model, enc, B, S, graph=True, positions=positions if table else None,
                                        weights=args.decode_weights)
            for t in range(8):
                cache.step(ids, pos, t)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for t in range(args.steps):
                cache.step(ids, pos, 8 + t % (S - 8))
            torch.cuda.synchronize()
            step_ms = (time.perf_counter() - t0) / args.steps * 1e3
            cache.ctl[0:1].fill_(S - 1)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for t in range(args.steps):
                cache._graph.replay()
            torch.cuda.synchronize()
            replay_ms = (time.perf_counter() - t0) / args.steps * 1e3
            out[name] = {"qarig_launches_per_step": launches, "step_ms": round(step_ms, 4),
                         "graph_replay_ms": round(replay_ms, 4)}
        kvcache.FUSE_NORMS = True
    if draws is not None:
        out["draw"] = draws
    print(json.dumps(out))


if __name__ == "__main__":
    main()
