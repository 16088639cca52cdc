#!/usr/bin/env python3
"""Cascade image generation on MI355X: same command line, stage-config JSON and output
files as the reference's generate_images.py (base stage "0" + encoder-decoder stages,
best-of-`num_beam` chunks of `beam_width` tokens, sliding window).

Under torchrun (one process per GPU) the images are sharded across the ranks -- they are independent, no
collective on the data path -- and every stage's token ids are gathered (a few KB) so that rank 0 decodes and
writes the same image grids a single process writes; rank r seeds its generator with --seed + r."""
import argparse
import os
import pathlib

import numpy as np
import torch

from models.Transformer import Transformer
from qarig import cli_common as cc
from qarig import ops, parallel, sampling
from utils.image_utils import save_images
from utils.model_utils import load_model


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Generate Images.")
    p.add_argument("--device", choices=["cpu", "cuda"], type=str, default="cpu",
                   help="Which hardware device will model run on.")
    p.add_argument("--decoder-path", required=True, type=pathlib.Path,
                   help="File path to pre-trained decoder model.")
    p.add_argument("--num-images", type=int, default=25, help="Num of images to generate.")
    p.add_argument("--seed", type=int, default=None,
                   help="Seed value.  Reproduces a run of this program; only --sampler torch keeps the reference's "
                        "generator stream (the default fused sampler draws the same distribution from a stream of "
                        "its own).")
    p.add_argument("--config-path", required=True, type=pathlib.Path,
                   help="File path to load json config file.")
    p.add_argument("--out-dir", required=True, type=pathlib.Path, help="File path to output directory.")
    p.add_argument("--batch-beams", action="store_true",
                   help="(additive) number the draws of the num_beam candidate chunks by batch row instead of "
                        "candidate after candidate as the reference loop does (the candidates are evaluated as one "
                        "batch either way when images x num_beam <= 16; with --sampler torch this is what batches them).")
    p.add_argument("--sampler", choices=["fused", "torch"], default=None,
                   help="(additive) cached decoding: 'fused' (default) draws inside the decode loop's own kernel from "
                        "uniforms of the device generator -- the whole chunk search stays on the GPU; 'torch' makes one "
                        "torch.multinomial call per token like the reference (its generator stream for a given --seed).")
    p.add_argument("--no-kv-cache", action="store_true",
                   help="re-run the whole window for every token like the reference instead of "
                        "decoding one token per step from a key/value cache")
    p.add_argument("--window-graph", action="store_true",
                   help="(additive) once the sliding window slides, evaluate each token as one replay of a captured "
                        "graph on the GPU instead of an eager pass over the window.  Applies only to the fused "
                        "sampler, images x num_beam <= 16 and models that generate from the key/value cache "
                        "(head dim 4 ... 64 or 128; the other multiples of 4 up to 124 with --cache-padded-heads); "
                        "elsewhere it is ignored.")
    p.add_argument("--cache-padded-heads", action="store_true",
                   help="(additive) generate from the key/value cache also when a head dim (width / heads) is a "
                        "multiple of 4 up to 124 other than 4, 8, 16, 32, 64 -- the head dims that train zero-padded; "
                        "without it such a model re-runs the whole window for every token.  Head dims that are no "
                        "multiple of 4 (the cache's 16-byte row loads and row copies need it) keep that loop either way.")
    p.add_argument("--top-k", type=int, default=None,
                   help="(additive) sample from the top-k most probable tokens only (ties at the cut: lower index "
                        "first); 0: off.  Overrides the config's per-stage \"top_k\" for all stages.")
    p.add_argument("--top-p", type=float, default=None,
                   help="(additive) nucleus sampling: of the tokens in descending probability, keep those with "
                        "less than this share of the mass in front of them (in (0, 1]; 1: off); applied after "
                        "--top-k.  Kept probabilities are not renormalised: best-of-num_beam still ranks chunks by "
                        "the model's own likelihood.  Overrides the config's per-stage \"top_p\" for all stages.")
    p.add_argument("--decode-weights", choices=["f32", "bf16"], default="f32",
                   help="(additive) weights of the cached single-token decode steps: 'bf16' streams every Linear weight "
                        "of a step as a bf16 image (rounded once, to nearest even; half the bytes per token) when "
                        "images x num_beam <= 16 and the model fits the streaming kernel.  Weight-only: activations, "
                        "accumulation, LayerNorm, attention, the key/value cache and sampling stay fp32.  Not the "
                        "fp32 parity mode.")
    p.add_argument("--prompt-fmaps", type=pathlib.Path, default=None,
                   help="(additive) image completion: a feature-map dataset index (generate_fmap_dataset.py's JSON); "
                        "its first --num-images latents are the prompts.  Every stage tokenises them with its own "
                        "codebooks, keeps the top rows of its token grid (--prompt-fraction) and generates the rest; "
                        "stage 0 takes its condition token from the latent's LR code instead of a random one.  The "
                        "decode of the real tokens is saved as prompt_model_{index}.jpg.  Needs --prompt-fraction.")
    p.add_argument("--prompt-fraction", type=float, default=None,
                   help="(additive) share of the token rows each stage keeps from the prompt, inside (0, 1): "
                        "floor(fraction x rows) rows.  The kept token count must be a multiple of the stage's "
                        "beam_width and, for a stage with a sliding window, stay below the window.")
    # (absent from the parsed arguments unless given: a run without the flag parses to what it always did)
    p.add_argument("--use-ema", action="store_true", default=argparse.SUPPRESS,
                   help="(additive) every Transformer stage loads the exponential moving average of its weights "
                        "(the checkpoint's 'model_ema', written by train_quantized_transformer.py --ema-decay) "
                        "instead of the last-step weights; a stage file without one is an error.")
    p.add_argument("--save-latents", type=pathlib.Path, default=argparse.SUPPRESS,
                   help="(additive) rank 0 writes the last stage's quantised latents -- the tensors the decoder turns "
                        "into recon_model_<last> -- for all --num-images as one fp32 (N,C,H,W) .npy file: the input of "
                        "evaluate_generation.py.")
    return vars(p.parse_args(argv))


def main():
    args = parse_args()
    device, world, rank = cc.require_gpu(args["device"])
    num_images, out_dir = args["num_images"], args["out_dir"]
    lo, hi = parallel.shard_range(num_images)
    n_local = hi - lo                                    # this rank's images
    log = print if rank == 0 else (lambda *a, **k: None)
    os.makedirs(out_dir, exist_ok=True)
    if args["seed"] is not None:
        torch.manual_seed(args["seed"] + rank)
    config = cc.read_config(args["config_path"])
    decoder_model, _ = cc.load_decoder(args["decoder_path"], device)
    decoder_model.eval()
    prompted = cc.check_prompt_args(args["prompt_fmaps"], args["prompt_fraction"])
    prompt_z = cc.load_prompt_latents(args["prompt_fmaps"], lo, hi, device) if prompted else None

    hr_input = None
    for index, data in config.items():          # stages "0", "1", "2" in file order
        log(f"Model: {int(index):,}")
        lr_codebook = None
        if data["lr_codebook_path"] is not None:
            lr_codebook, lr_d = cc.load_codebook(data["lr_codebook_path"], device)
        hr_codebook, hr_d = cc.load_codebook(data["hr_codebook_path"], device)
        k_hr = hr_d["num_embeddings"]
        img_H, img_W = hr_d["image_dim"]
        pH, pW = hr_d["patch_dim"]
        total_Seq = (img_H // pH) * (img_W // pW)
        if total_Seq % data["beam_width"] != 0:
            raise Exception("Invalid value for beam_width!")

        ok, md = load_model(data["model_path"])
        if not ok:
            raise Exception("An error occured while loading model checkpoint!")
        model = Transformer(
            use_encoder=not md["train_base_model"], use_pos_cond=md["use_sliding_window"],
            num_enc_layers=md["num_enc_layers"], num_dec_layers=md["num_dec_layers"],
            num_enc_embedding=md["num_enc_embedding"], num_dec_embedding=md["num_dec_embedding"],
            self_attn_heads=md["self_attn_heads"], cross_attn_heads=md["cross_attn_heads"],
            transformer_in_dim=md["transformer_in_dim"], transformer_out_dim=md["transformer_out_dim"],
            transformer_hidden_dim=md["transformer_hidden_dim"],
            hidden_activation=md["hidden_activation"])
        use_ema = args.get("use_ema", False)
        if use_ema and "model_ema" not in md:
            raise Exception(f"--use-ema: {data['model_path']} holds no 'model_ema' (train with --ema-decay)!")
        model.custom_load_state_dict(md["model_ema" if use_ema else "model"])
        model = model.to(device).eval()

        with torch.no_grad():
            shift = 0
            if index == "0":
                # base stage: a random LR-codebook token is the image-level condition
                k_lr = lr_d["num_embeddings"]
                lr_input = None
                if prompted:    # the image-level condition of the real latent: its LR code (as training assembles it)
                    hr_input = torch.zeros((n_local, 1), dtype=torch.int64, device=device)
                    if n_local:
                        hr_input = lr_codebook.get_patches_bmu(prompt_z, reshape=True)
                        if hr_input.shape[1] != 1:
                            raise Exception("Invalid LR codebook for a prompt: the base stage takes one LR token!")
                else:
                    hr_input = torch.randint(low=0, high=k_lr, size=(n_local, 1), device=device)
                all_cond = parallel.gather_rows(hr_input, num_images)
                if rank == 0:
                    cond = decoder_model(lr_codebook.get_quantized_image(indices=all_cond, unpatchify_input=True))
                    save_images(images=cond, file_name="recon_model_Cond", dest_path=out_dir, logging=print)
                shift = k_lr
            else:
                lr_input = hr_input                                   # previous stage's tokens
                hr_input = torch.full((n_local, 1), k_hr, dtype=torch.int64, device=device)

            # optional per-stage keys (the reference's config files have neither: off)
            top_k = data.get("top_k", 0) if args["top_k"] is None else args["top_k"]
            top_p = data.get("top_p", 1.0) if args["top_p"] is None else args["top_p"]
            kept = 0
            if prompted:
                # the stage's own tokens of the real latents (train_quantized_transformer.py tokenises the same
                # way); the top rows of the grid, in the numbering the loop appends (+ shift), follow the start token
                kept = cc.prompt_tokens(args["prompt_fraction"], hr_d["image_dim"], hr_d["patch_dim"],
                                        data["beam_width"], md["sliding_window"] if md["use_sliding_window"] else None)
                real = torch.zeros((0, total_Seq), dtype=torch.int64, device=device)
                if n_local:
                    real = hr_codebook.get_patches_bmu(prompt_z, reshape=True)
                    hr_input = torch.cat((hr_input, real[:, :kept] + shift), dim=1)
                all_real = parallel.gather_rows(real, num_images)
                if rank == 0:
                    truth = decoder_model(hr_codebook.get_quantized_image(indices=all_real, unpatchify_input=True))
                    save_images(images=truth, file_name=f"prompt_model_{index}", dest_path=out_dir, logging=print)
                log(f"Prompt: {kept:,} / {total_Seq:,} tokens kept")
            if n_local:
                hr_input = sampling.generate_tokens(
                    model, hr_input, lr_input, total_Seq, data["temperature"], md["use_sliding_window"],
                    md["sliding_window"], end_token=k_hr, shift=shift, num_beam=data["num_beam"],
                    beam_width=data["beam_width"], mode="generate",
                    progress=lambda i, t: log(f"{i:,} / {t:,}"), batch_beams=args["batch_beams"],
                    use_kv_cache=not args["no_kv_cache"], sampler=args["sampler"],
                    window_graph=args["window_graph"], top_k=top_k, top_p=top_p,
                    decode_weights=args["decode_weights"],
                    cache_padded_heads=args["cache_padded_heads"] or None)
                hr_input = hr_input[:, 1:] - shift
                if prompted and not torch.equal(hr_input[:, :kept], real[:, :kept]):
                    raise Exception("The completion does not keep the prompt's tokens!")
            else:                                       # more ranks than images: nothing to generate here
                hr_input = torch.zeros((0, total_Seq), dtype=torch.int64, device=device)
            ops.check_index_flag(device, f"stage {index} tokens")
            all_tokens = parallel.gather_rows(hr_input, num_images)
            if prompted and rank == 0:
                same = torch.equal(all_tokens[:, :kept], all_real[:, :kept])
                log(f"Prompt: completions {'keep' if same else 'DO NOT keep'} the {kept:,} prompt tokens of "
                    f"{num_images:,} images")
            if rank == 0:
                latents = hr_codebook.get_quantized_image(indices=all_tokens, unpatchify_input=True)
                recon = decoder_model(latents)
                ops.check_index_flag(device, f"stage {index} tokens")
                if args.get("save_latents") is not None and index == list(config)[-1]:
                    args["save_latents"].parent.mkdir(parents=True, exist_ok=True)
                    with open(args["save_latents"], "wb") as f:      # (a file object: np.save appends no ".npy")
                        np.save(f, latents.detach().float().cpu().numpy())
                save_images(images=recon, file_name=f"recon_model_{index}", dest_path=out_dir, logging=print)
        sampling.decode_cache_clear()        # (the stage's decode caches hold its model: let both go, as the reference does)
        del model
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
