#!/usr/bin/env python3
"""The slid part of a configs[3]-type stage: 64 x 64 x 4 latents at HR patch 2 (1,024 tokens), window 256,
4 images, beam 4 x 4 (16 rows), README model sizes (encoder-decoder stage: 5 + 7 layers, width 512, hidden 2048,
64 heads), random weights, 1 MI355X.  Once the window slides every token is a full evaluation of 16 x 255 rows:
the eager tail (model.decode of the window) against the window graph (kvcache.WindowStep, one replay), in one
process.  One JSON line: ms per slid evaluation and accepted tokens/s of the stage for both, the step graph's
kernel count, and the GFLOP of one evaluation counted from the model's shapes with the fraction of the fp32
MFMA peak (157.3 TF) and of the fp32 GEMM family's
measured 122 TF that implies.
    python tools/bench_window_generate.py [--evals 50] [--window-graph-only]"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "quantized-autoregression-image-generator_amd"))
import torch  # noqa: E402
from models.Transformer import Transformer  # noqa: E402
from qarig import sampling  # noqa: E402

FP32_GEMM_TF = 122.0      # measured fp32 MFMA GEMM family (README)
FP32_MFMA_PEAK_TF = 157.3  # MI355X fp32 MFMA peak


def stage_model(K, dev):
    return Transformer(use_encoder=True, use_pos_cond=True, num_enc_layers=5, num_dec_layers=7,
                       num_enc_embedding=K, num_dec_embedding=K + 1, self_attn_heads=64, cross_attn_heads=64,
                       transformer_in_dim=512, transformer_out_dim=K + 1, transformer_hidden_dim=2048).to(dev).eval()


def eval_gflop(model, R, W1, S_enc):
    """Multiply-adds x 2 of one window evaluation as WindowStep runs it (cross k / v and the conditioning table
    are built once per stage and not counted): per layer but the last, on all R x W1 tokens, the q / k / v MLPs
    (D -> H -> D each), the causal attention (q.k and p.v: W1 / 2 keys on average), the cross-attention q MLP and
    its attention over S_enc keys, the three residual Linears (D x D) and the FFN (D -> H -> D); the last layer's
    k / v MLPs on all tokens and everything else on R rows; the classifier (D -> H -> V) on R rows."""
    D = model.dec_embedding.weight.shape[1]
    Hd = model.decoder_layers[0].feedforward_block.feedforward[0].linear_layer[0].weight.shape[0]
    V = model.classifier[1].linear_layer[0].weight.shape[0]
    Hc = model.classifier[0].linear_layer[0].weight.shape[0]
    cross = model.decoder_layers[0].use_cross_attn
    mlp = 2 * D * Hd                        # one D -> H -> D MLP per token
    per_tok = 3 * mlp + 2 * D * W1 / 2 + (mlp + 2 * D * S_enc + D * D if cross else 0) + 2 * D * D + mlp
    T = R * W1
    L = len(model.decoder_layers)
    macs = (L - 1) * T * per_tok + T * 2 * mlp + R * (mlp + 2 * D * W1 + D * D
                                                      + ((mlp + 2 * D * S_enc + D * D) if cross else 0)
                                                      + D * D + mlp) + R * (D * Hc + Hc * V)
    return 2 * macs / 1e9


def graph_kernels(step):
    """(kernel nodes, all nodes) of the window step's graph: the same evaluation captured once more into a graph
    that keeps its hipGraph_t, counted with hipGraphGetNodes / hipGraphNodeGetType (never replayed)."""
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(graph), torch.no_grad():
        step._forward()
    hip = ctypes.CDLL("libamdhip64.so")
    g = ctypes.c_void_p(graph.raw_cuda_graph())
    n = ctypes.c_size_t(0)
    if hip.hipGraphGetNodes(g, None, ctypes.byref(n)) != 0:
        return None
    nodes = (ctypes.c_void_p * n.value)()
    hip.hipGraphGetNodes(g, nodes, ctypes.byref(n))
    kinds = []
    for i in range(n.value):
        t = ctypes.c_int(-1)
        hip.hipGraphNodeGetType(ctypes.c_void_p(nodes[i]), ctypes.byref(t))
        kinds.append(t.value)
    return sum(1 for k in kinds if k == 0), len(kinds)       # hipGraphNodeTypeKernel == 0


def timed(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--evals", type=int, default=50, help="timed evaluations of each form")
    ap.add_argument("--tokens", type=int, default=1024)
    ap.add_argument("--window-graph-only", action="store_true",
                    help="only the window graph (evaluations, then one stage): for a profiler pass")
    ap.add_argument("--no-stage", action="store_true", help="per-evaluation times only")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    K, N, NB, W, S_enc = 512, 4, 4, 256, 256
    R, W1 = N * NB, W - 1
    model = stage_model(K, dev)
    lr_in = torch.randint(0, K, (N, S_enc), device=dev)
    first = torch.full((N, 1), K, dtype=torch.int64, device=dev)
    total = args.tokens
    pos_off, bw = 1, 4
    pos_bound = total + bw + pos_off + 1
    out = {"stage": f"{total} tokens, window {W}, {N} images, beam {NB} x {bw}", "rows": R, "window_tokens": W1}
    with torch.no_grad():
        enc = model.encode(lr_in).repeat_interleave(NB, dim=0)
        seq = torch.randint(0, K, (R, 600), device=dev)
        step = sampling.window_step(model, enc, R, W, total + bw, pos_bound, pos_off)
        step.load(seq)
        step.evaluate()
        out["window_graph_ms_per_eval"] = round(timed(step.evaluate, args.evals), 3)
        out["pad_row"] = bool(step.pad)
        kn = graph_kernels(step)
        if kn is not None:
            out["step_graph_kernels"], out["step_graph_nodes"] = kn
        if not args.window_graph_only:
            win = torch.cat((seq[:, -W1:], seq[:, -1:]), dim=1).contiguous()     # the eager tail's padded window
            j = torch.arange(600 - W1, 600, device=dev)
            pos = torch.cat((j, j[-1:])).add(pos_off).expand(R, -1).contiguous()

            def eager():
                return model.decode(win, enc, pos, pos_bound=pos_bound)[:, -2]
            eager()
            out["eager_ms_per_eval"] = round(timed(eager, max(5, args.evals // 5)), 3)
            out["speedup_per_eval"] = round(out["eager_ms_per_eval"] / out["window_graph_ms_per_eval"], 2)
    gf = eval_gflop(model, R, W1, S_enc)
    out["gflop_per_eval"] = round(gf, 2)
    tf = gf / (out["window_graph_ms_per_eval"] * 1e-3) / 1e3
    out["window_graph_tflops"] = round(tf, 1)
    out["fraction_of_fp32_mfma_peak"] = round(tf / FP32_MFMA_PEAK_TF, 3)
    out["fraction_of_fp32_gemm_family"] = round(tf / FP32_GEMM_TF, 3)
    out["floor_ms_at_122tf"] = round(gf / (FP32_GEMM_TF * 1e3) * 1e3, 3)
    if not args.no_stage:
        modes = [True] if args.window_graph_only else [False, True]
        for wg in modes:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            toks = sampling.generate_tokens(model, first, lr_in, total, 1.0, True, W, end_token=K, num_beam=NB,
                                            beam_width=bw, mode="generate", sampler="fused", window_graph=wg)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            assert toks.shape[1] >= total
            out[("window_graph" if wg else "eager") + "_stage_accepted_tokens_per_s"] = round(N * total / dt, 1)
            out[("window_graph" if wg else "eager") + "_stage_seconds"] = round(dt, 3)
        if not args.window_graph_only:
            out["stage_tokens_per_s_ratio"] = round(out["window_graph_stage_accepted_tokens_per_s"]
                                                    / out["eager_stage_accepted_tokens_per_s"], 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
