#!/usr/bin/env python3
"""Train the quantized (cascaded) Transformer on MI355X.  Same command line, JSON config
keys, log lines, checkpoint dict and output tree as the reference's
train_quantized_transformer.py; the compute is the HIP path (models/, qarig/).

New, additive: run under `python -m torch.distributed.run --nproc-per-node N ...` for
data parallelism (--batch-size is then per GPU; one RCCL all-reduce of the flat gradient
buffer per step; rank 0 logs, checkpoints and samples)."""
import argparse
import logging
import math
import pathlib

import torch

from models.Transformer import Transformer
from qarig import cli_common as cc
from qarig import ops, parallel, pipeline, sampling
from qarig.optim import FlatAdam, LRSchedule, decay_parameters
from utils.image_utils import save_images
from utils.model_utils import load_model, save_model
from dataset_loader.feature_map_dataset import FeatureMapDataset


def restricted_float(x):
    try:
        x = float(x)
    except ValueError:
        raise argparse.ArgumentTypeError("%r not a floating-point literal" % (x,))
    if x < 0.1:
        raise argparse.ArgumentTypeError("%r not in range > 0.1" % (x,))
    return x


def parse_args():
    p = argparse.ArgumentParser(description="Train Quantized Transformer models.")
    p.add_argument("--device", choices=["cpu", "cuda"], type=str, default="cpu",
                   help="Which hardware device will model run on.")
    p.add_argument("--dataset-path", required=True, type=pathlib.Path,
                   help="File path to feature map dataset json file.")
    p.add_argument("--train-base-model", action="store_true", help="Train Base Model, Decoder-only.")
    p.add_argument("--decoder-path", required=True, type=pathlib.Path,
                   help="File path to pre-trained decoder model.")
    p.add_argument("--lr-codebook-path", required=True, type=pathlib.Path,
                   help="File path to saved Low-Res codebook.")
    p.add_argument("--hr-codebook-path", required=True, type=pathlib.Path,
                   help="File path to saved High-Res codebook.")
    p.add_argument("--model-path", default=None, required=False, type=pathlib.Path,
                   help="File path to saved model checkpoint.")
    p.add_argument("--test-num-sample", type=int, default=25, help="Num samples for testing dataset.")
    p.add_argument("--load-optim", action="store_true", help="Load saved optim parameters with model.")
    p.add_argument("--batch-size", type=int, default=8, help="Batch size for dataset.")
    p.add_argument("--temperature", type=restricted_float, default=1.0,
                   help="Temperature for softmax sampling.")
    p.add_argument("--checkpoint-step", type=int, default=1_000,
                   help="Steps at which checkpoint takes place.")
    p.add_argument("--lr-step", type=int, default=50_000, help="Steps before halving learning rate.")
    p.add_argument("--max-epoch", type=int, default=1_000, help="Maximum epoch for training model.")
    p.add_argument("--use-activation-checkpoint", action="store_true",
                   help="Use Activation Checkpointing; trade-off memory footprint and compute.")
    p.add_argument("--config-path", required=True, type=pathlib.Path,
                   help="File path to load json config file.")
    p.add_argument("--out-dir", required=True, type=pathlib.Path, help="File path to output directory.")
    p.add_argument("--graph-step", action="store_true",
                   help="(additive) replay the training step from captured HIP graphs: removes the Python "
                        "launch overhead for small per-GPU batches; full batches only.  Under torchrun the "
                        "capture is a chain of segments cut at the gradient buckets, the bucket all-reduces "
                        "issued between them")
    p.add_argument("--gemm-x3", action="store_true",
                   help="(additive) run the eligible fp32 Linear products on the bf16 matrix pipe from exact three-way "
                        "bf16 splits of the fp32 operands (library option gemm_x3, csrc/gemm_x3.hip): fp32 operands, "
                        "results and tolerances, about 1.2 x the step throughput at README sizes")
    p.add_argument("--packed-dataset", default=None,
                   help="(additive) one (N,C,H,W) float32 .npy holding every latent of --dataset-path "
                        "(dataset_loader.prefetch.pack_feature_maps): read through one mmap instead of "
                        "one file per item; same items, same order")
    p.add_argument("--max-steps", type=int, default=None,
                   help="(additive) stop after this many optimiser steps.")
    p.add_argument("--ema-decay", type=float, default=0.0,
                   help="(additive; the reference keeps no such average) keep an exponential moving average of "
                        "the weights with this decay (0 < D < 1, e.g. 0.999; 0 = off), updated by the optimiser's "
                        "own launch with the usual warm-up min(D, (1 + n) / (10 + n)).  Checkpoints then also "
                        "carry 'model_ema' / 'model_ema_meta' (generate_images.py --use-ema samples from it) and "
                        "every checkpoint writes a second sample grid, high_res_recon_ema_<steps>")
    p.add_argument("--val-dataset-path", type=pathlib.Path, default=None,
                   help="(additive; the reference never evaluates) feature map dataset json file of held-out latents: "
                        "every --val-step steps rank 0 scores it (qarig/evaluate.py: the training objective on "
                        "deterministic windows, every token once), logs Val Loss | bits/token | top-1 and appends "
                        "one JSON line to <out-dir>/val_log.jsonl; with --ema-decay the averaged weights are "
                        "scored too")
    p.add_argument("--val-step", type=int, default=None,
                   help="(additive) steps between two evaluations of --val-dataset-path (default: --checkpoint-step).")
    p.add_argument("--val-batches", type=int, default=None,
                   help="(additive) score only the first batches of --val-dataset-path.")
    cc.add_regulariser_args(p)
    cc.add_neighbour_args(p)
    cc.add_dropout_args(p)
    cc.add_attn_dropout_args(p)
    cc.add_token_noise_args(p)
    cc.add_optimizer_args(p)
    cc.add_grad_clip_args(p)
    args = vars(p.parse_args())
    try:        # what holds only between the flags (cosine needs --lr-decay-steps, at or past the warm-up)
        cc.check_optimizer_args(args["weight_decay"], args["lr_schedule"], args["lr_warmup_steps"],
                                args["lr_decay_steps"], args["lr_min_ratio"])
        cc.check_grad_clip_args(args["clip_grad_norm"], args["max_skipped_steps"])
        cc.check_neighbour_args(args["label_smoothing"], args["z_loss"], args["neighbour_smoothing"],
                                args["neighbour_range"], args["neighbour_sigma"])
        cc.check_token_noise_args(args["input_noise"], args["cond_noise"], args["noise_range"], args["dropout_seed"],
                                  train_base_model=args["train_base_model"])
    except ValueError as e:
        p.error(str(e))
    return args


def main():
    project_name = "Quantized Transformer"
    args = parse_args()
    cfg = cc.read_config(args["config_path"])
    device, world, rank = cc.require_gpu(args["device"])
    if args["gemm_x3"]:
        from qarig import _lib
        _lib.set_option("gemm_x3", 1)
    out_dir = args["out_dir"]
    cc.setup_logging(out_dir, project_name, rank)
    temperature = args["temperature"]
    train_base_model = args["train_base_model"]
    test_num_sample = args["test_num_sample"]

    decoder_model, dec_d = cc.load_decoder(args["decoder_path"], device)
    lr_codebook, lr_d = cc.load_codebook(args["lr_codebook_path"], device, "Low-Resolution codebook")
    hr_codebook, hr_d = cc.load_codebook(args["hr_codebook_path"], device, "Low-Resolution codebook")
    lr_num_embeddings, hr_num_embeddings = lr_d["num_embeddings"], hr_d["num_embeddings"]
    img_H, img_W = hr_d["image_dim"]
    hr_pH, hr_pW = hr_d["patch_dim"]
    total_hr_Seq = (img_H // hr_pH) * (img_W // hr_pW)

    # vocabularies (reference :258-296)
    if train_base_model:
        num_enc_layers = num_enc_embedding = cross_attn_heads = None
        num_dec_embedding = lr_num_embeddings + hr_num_embeddings
    else:
        num_enc_embedding = lr_num_embeddings
        num_enc_layers = cfg["num_enc_layers"]
        cross_attn_heads = cfg["cross_attn_heads"]
        num_dec_embedding = hr_num_embeddings + 1          # + <start>
    use_sliding_window = cfg["use_sliding_window"]
    sliding_window = cfg["sliding_window"] if use_sliding_window else None
    hp = dict(num_dec_layers=cfg["num_dec_layers"], self_attn_heads=cfg["self_attn_heads"],
              transformer_in_dim=cfg["in_dim"], transformer_out_dim=hr_num_embeddings + 1,
              transformer_hidden_dim=cfg["hidden_dim"], hidden_activation=cfg["hidden_activation"])

    model = Transformer(use_encoder=not train_base_model, use_pos_cond=use_sliding_window,
                        num_enc_layers=num_enc_layers, num_enc_embedding=num_enc_embedding,
                        num_dec_embedding=num_dec_embedding, cross_attn_heads=cross_attn_heads,
                        use_activation_checkpoint=args["use_activation_checkpoint"], **hp).to(device)
    model_lr = cfg["model_lr"]
    if args["model_path"] is not None:
        ok, saved = load_model(args["model_path"])
        if not ok:
            raise Exception("An error occured while loading model checkpoint!")
        model.custom_load_state_dict(saved["model"])
    optim = FlatAdam(model.parameters(), lr=model_lr, betas=(0.5, 0.999))
    if args["model_path"] is not None:
        if args["load_optim"]:
            optim.load_state_dict(saved["model_optimizer"])
        else:
            for g in optim.param_groups:
                g["lr"] = model_lr
    parallel.broadcast_params(optim)
    ema_decay = args["ema_decay"]
    if ema_decay:
        # after the broadcast and the optimizer state: the average starts from the parameters every rank holds
        resumed = args["model_path"] is not None and args["load_optim"] and "model_ema" in saved
        meta = saved.get("model_ema_meta", {}) if resumed else {}
        optim.enable_ema(ema_decay, warmup=meta.get("warmup", True))
        if resumed:
            optim.load_ema(saved["model_ema"], model, meta.get("count", 0))
    optim.enable_allreduce_overlap()     # no-op at world 1
    weight_decay, lr_schedule, lr_warmup_steps, lr_decay_steps, lr_min_ratio = cc.check_optimizer_args(
        args["weight_decay"], args["lr_schedule"], args["lr_warmup_steps"], args["lr_decay_steps"],
        args["lr_min_ratio"])
    schedule = None         # the reference's loop: halve_lr every --lr-step
    if not cc.optimizer_args_are_default(weight_decay, lr_schedule, lr_warmup_steps, lr_decay_steps, lr_min_ratio):
        # a function of the optimizer's step count: with --load-optim the schedule continues where it was
        schedule = LRSchedule(model_lr, lr_schedule, lr_step=args["lr_step"], warmup_steps=lr_warmup_steps,
                              decay_steps=lr_decay_steps, min_ratio=lr_min_ratio)
    if weight_decay > 0:
        optim.enable_weight_decay(weight_decay, decay_parameters(model))
    clip_grad_norm, max_skipped_steps = cc.check_grad_clip_args(args["clip_grad_norm"], args["max_skipped_steps"])
    if clip_grad_norm is not None:
        # the norm is taken in optim.step(), behind the gradient exchange: the same bits on every rank
        optim.enable_grad_clip(clip_grad_norm)
    # argparse has checked both; once more before anything is launched with them
    label_smoothing, z_loss = ops.check_ce_regularisers(args["label_smoothing"], args["z_loss"])
    # the HR codes are the classes on the SOM axis; <end>, the class behind them, is nobody's neighbour
    neighbour_smoothing, neighbour_range, neighbour_sigma = cc.check_neighbour_args(
        label_smoothing, z_loss, args["neighbour_smoothing"], args["neighbour_range"], args["neighbour_sigma"],
        codes=hr_codebook.num_embeddings)
    soft = dict(neighbour_smoothing=neighbour_smoothing, neighbour_range=neighbour_range,
                neighbour_sigma=neighbour_sigma, codes=hr_codebook.num_embeddings if neighbour_smoothing > 0 else None)
    regularised = label_smoothing > 0 or z_loss > 0 or neighbour_smoothing > 0
    dropout, dropout_seed = cc.check_dropout_args(args["dropout"], args["dropout_seed"])
    if dropout > 0:
        # the step word of the mask key follows optim.step_count: with --load-optim the sequence continues
        model.enable_dropout(dropout, dropout_seed, rank=parallel.rank())
    # the longest query and key extents an attention layer of this run can meet: the window (or the whole
    # sequence: LR tokens, <start>, HR tokens), and the LR tokens for cross-attention
    lr_seq = (lr_d["image_dim"][0] // lr_d["patch_dim"][0]) * (lr_d["image_dim"][1] // lr_d["patch_dim"][1])
    longest = lr_seq + total_hr_Seq + 1
    if use_sliding_window:
        longest = min(longest, sliding_window)
    attn_dropout, _ = cc.check_attn_dropout_args(
        args["attn_dropout"], dropout_seed, sites=len(model._attention_layers()), batch=args["batch_size"],
        heads=max(hp["self_attn_heads"], cross_attn_heads or 1), seq_q=longest, seq_k=max(longest, lr_seq))
    if attn_dropout > 0:
        # the same key (seed, rank, step word) as --dropout; the attention sites are a namespace of their own
        model.enable_attention_dropout(attn_dropout, dropout_seed, rank=parallel.rank())
    try:        # (the codebook sizes are known only here)
        input_noise, cond_noise, noise_range, _ = cc.check_token_noise_args(
            args["input_noise"], args["cond_noise"], args["noise_range"], dropout_seed,
            train_base_model=train_base_model, k_lr=lr_num_embeddings, k_hr=hr_num_embeddings)
    except ValueError as e:
        raise SystemExit(str(e))
    token_noise = input_noise > 0 or cond_noise > 0
    if token_noise:
        # the same key once more; the tokens are corrupted where they are assembled (pipeline.tokenize_window)
        model.enable_token_noise(input_noise, cond_noise, dropout_seed, rank=parallel.rank(),
                                 neighbour_range=noise_range)

    dataset = FeatureMapDataset(dataset_path=args["dataset_path"], load_image=False,
                                return_filepaths=False)
    train_set = dataset
    if args["packed_dataset"]:
        from dataset_loader.prefetch import PackedFeatureMapDataset
        train_set = PackedFeatureMapDataset(args["packed_dataset"])
        assert len(train_set) == len(dataset), "--packed-dataset does not match --dataset-path"
    # batches are copied to the device from pinned memory on a side stream, two ahead of the
    # step that consumes them (the reference copies each batch synchronously, :407)
    from dataset_loader.prefetch import DevicePrefetcher
    loader = DevicePrefetcher(cc.ShardedLoader(train_set, args["batch_size"], num_workers=4, shuffle=True),
                              device, depth=2)
    test_loader = torch.utils.data.DataLoader(dataset, batch_size=test_num_sample, num_workers=2,
                                              shuffle=True)

    info = logging.info
    info(f"{project_name}")
    info(f"Output Dir: {out_dir}")
    info(f"Model size: {sum(p.numel() for p in model.parameters()):,}")
    info("#" * 100)
    info("Decoder Parameters.")
    for k in ("num_layers", "image_channel", "min_channel", "max_channel", "latent_channel"):
        info(f"{k.replace('_', ' ').title()}: {dec_d[k]:,}")
    info(f"Hidden activation type: {dec_d['hidden_activation_type']}")
    info(f"Decoder activation type: {dec_d['decoder_activation_type']}")
    info("#" * 100)
    info("Codebook Parameters.")
    info(f"Low Res Patch size: {lr_d['patch_dim']}")
    info(f"Low Res Num Embeddings: {lr_num_embeddings:,}")
    info(f"High Res Patch size: {hr_d['patch_dim']}")
    info(f"High Res Num Embeddings: {hr_num_embeddings:,}")
    info("#" * 100)
    info("Transformer Parameters.")
    if use_sliding_window:
        info(f"Sliding Window: {sliding_window:,}")
    info(f"Num Encoder Embedding: {num_enc_embedding}")
    info(f"Num Encoder Layers: {num_enc_layers}")
    info(f"Num Decoder Embedding: {num_dec_embedding:,}")
    info(f"Num Decoder Layers: {hp['num_dec_layers']:,}")
    info(f"Self Attention Heads: {hp['self_attn_heads']:,}")
    info(f"Cross Attention Heads: {cross_attn_heads}")
    info(f"In Dim: {hp['transformer_in_dim']:,}")
    info(f"Out Dim: {hp['transformer_out_dim']:,}")
    info(f"Hidden Dim: {hp['transformer_hidden_dim']:,}")
    info(f"Hidden activation: {hp['hidden_activation']}")
    info("#" * 100)
    info("Training Parameters.")
    info(f"Max Epoch: {args['max_epoch']:,}")
    info(f"Batch Size: {args['batch_size']:,}" + (f" x {world} GPUs" if world > 1 else ""))
    info(f"Model LR Update size: {args['lr_step']:,}")
    info(f"Model Checkpoint step: {args['checkpoint_step']:,}")
    if ema_decay:
        info(f"EMA decay: {ema_decay}")
    if regularised:
        info(f"Label Smoothing: {label_smoothing}")
        info(f"Z-Loss: {z_loss}")
    if neighbour_smoothing > 0:
        info(f"Neighbour Smoothing: {neighbour_smoothing}")
        info(f"Neighbour Range: {neighbour_range}")
        info(f"Neighbour Sigma: {neighbour_sigma}")
    if dropout > 0:
        info(f"Dropout: {dropout}")
        info(f"Dropout Seed: {dropout_seed}")
    if attn_dropout > 0:
        info(f"Attention Dropout: {attn_dropout}")
        if not dropout > 0:
            info(f"Dropout Seed: {dropout_seed}")
    if token_noise:
        info(f"Input Noise: {input_noise}")
        info(f"Cond Noise: {cond_noise}")
        info(f"Noise Range: {noise_range}")
        if not (dropout > 0 or attn_dropout > 0):
            info(f"Dropout Seed: {dropout_seed}")
    if weight_decay > 0:
        info(f"Weight Decay: {weight_decay}")
    if schedule is not None:
        info(f"LR Schedule: {lr_schedule}")
        info(f"LR Warmup Steps: {lr_warmup_steps:,}")
        if lr_decay_steps is not None:
            info(f"LR Decay Steps: {lr_decay_steps:,}")
        info(f"LR Min Ratio: {lr_min_ratio}")
    if clip_grad_norm is not None:
        info(f"Clip Grad Norm: {clip_grad_norm}")
        info(f"Max Skipped Steps: {max_skipped_steps:,}")
    info("#" * 100)
    info("Sampling Parameters.")
    info(f"Temperature: {temperature:,}")
    info("#" * 100)

    def checkpoint(global_steps):
        model_dict = {"train_base_model": train_base_model, "use_sliding_window": use_sliding_window,
                      "sliding_window": sliding_window, "num_enc_embedding": num_enc_embedding,
                      "num_dec_embedding": num_dec_embedding, "num_enc_layers": num_enc_layers,
                      "num_dec_layers": hp["num_dec_layers"], "self_attn_heads": hp["self_attn_heads"],
                      "cross_attn_heads": cross_attn_heads,
                      "transformer_in_dim": hp["transformer_in_dim"],
                      "transformer_out_dim": hp["transformer_out_dim"],
                      "transformer_hidden_dim": hp["transformer_hidden_dim"],
                      "hidden_activation": hp["hidden_activation"],
                      "model": {k: v.detach().clone() for k, v in model.state_dict().items()},
                      "model_optimizer": optim.state_dict()}
        if ema_decay:
            model_dict["model_ema"] = optim.ema_state_dict(model)
            model_dict["model_ema_meta"] = optim.ema_meta()
        if label_smoothing > 0:     # informational: a resumed run takes its values from its own command line
            model_dict["label_smoothing"] = label_smoothing
        if z_loss > 0:
            model_dict["z_loss"] = z_loss
        if neighbour_smoothing > 0:     # informational likewise
            model_dict["neighbour_smoothing"] = neighbour_smoothing
            model_dict["neighbour_range"] = neighbour_range
            model_dict["neighbour_sigma"] = neighbour_sigma
        if dropout > 0:             # informational likewise
            model_dict["dropout"] = dropout
            model_dict["dropout_seed"] = dropout_seed
        if attn_dropout > 0:        # informational likewise
            model_dict["attn_dropout"] = attn_dropout
            model_dict["dropout_seed"] = dropout_seed
        if token_noise:             # informational likewise: the non-zero values
            if input_noise > 0:
                model_dict["input_noise"] = input_noise
            if cond_noise > 0:
                model_dict["cond_noise"] = cond_noise
            if noise_range > 0:
                model_dict["noise_range"] = noise_range
            model_dict["dropout_seed"] = dropout_seed
        if weight_decay > 0:        # informational likewise
            model_dict["weight_decay"] = weight_decay
        if schedule is not None:
            model_dict["lr_schedule"] = lr_schedule
            model_dict["lr_warmup_steps"] = lr_warmup_steps
            model_dict["lr_decay_steps"] = lr_decay_steps
            model_dict["lr_min_ratio"] = lr_min_ratio
        if clip_grad_norm is not None:      # informational likewise
            model_dict["clip_grad_norm"] = clip_grad_norm
        ok = save_model(model_dict=model_dict, dest_path=out_dir, file_name=f"model_{global_steps}.pt",
                        logging=info)
        info("Successfully saved model." if ok else "Error occured saving model.")
        # one full autoregressive sample per checkpoint (reference :536-677)
        model.eval()
        with torch.no_grad():
            fm = next(iter(test_loader)).to(device)
            n = fm.shape[0]
            save_images(decoder_model(fm), f"ground_truth_{global_steps}", out_dir, logging=info)
            save_images(decoder_model(lr_codebook(fm)), f"low_res_cond_{global_steps}", out_dir,
                        logging=info)
            save_images(decoder_model(hr_codebook(fm)), f"high_res_example_{global_steps}", out_dir,
                        logging=info)
            lr_idx = lr_codebook.get_patches_bmu(fm, reshape=True)
            if train_base_model:
                first, lr_in, shift = lr_idx, None, lr_num_embeddings
            else:
                first = torch.full((n, 1), hr_num_embeddings, dtype=torch.int64, device=device)
                lr_in, shift = lr_idx, 0

            def sample_grid(name):
                toks = sampling.generate_tokens(
                    model, first, lr_in, total_hr_Seq, temperature, use_sliding_window, sliding_window,
                    end_token=hr_num_embeddings, shift=shift, mode="train",
                    progress=lambda i, t: print(f"{i:,} / {t:,}"))
                toks = toks[:, first.shape[1]:] if train_base_model else toks[:, 1:]
                if train_base_model:
                    toks = toks - lr_num_embeddings
                    toks[toks == hr_num_embeddings] = lr_num_embeddings
                else:
                    toks[toks == hr_num_embeddings] = 0
                save_images(decoder_model(hr_codebook.get_quantized_image(toks, unpatchify_input=True)),
                            f"{name}_{global_steps}", out_dir, logging=info)

            sample_grid("high_res_recon")
            if ema_decay:
                with optim.ema_weights():       # the same conditioning, from the averaged weights
                    sample_grid("high_res_recon_ema")
        model.train()
        torch.cuda.empty_cache()

    val_loader, val_step = cc.build_validation(args, rank, info)     # (None, None) without the flag or off rank 0
    if val_loader is not None:
        from qarig import evaluate

    def validate(global_steps):
        """Rank 0 alone, like checkpoint(): the other ranks wait at their next exchange."""
        def score():
            scorer = evaluate.TokenScorer(model, lr_codebook, hr_codebook, train_base_model,
                                          sliding_window if use_sliding_window else None)
            evaluate.score_loader(scorer, val_loader, device, args["val_batches"])
            r = scorer.result()
            del r["per_image_nll"]          # (evaluate_transformer.py reports it; the log keeps one line per evaluation)
            return r

        entry = {"step": global_steps, "model": score()}
        info(evaluate.summary_line("Val", entry["model"]))
        if ema_decay:
            with optim.ema_weights():
                entry["model_ema"] = score()
            info(evaluate.summary_line("Val EMA", entry["model_ema"]))
        cc.validate(out_dir, entry, (), info)

    graphed = None
    batch_size = args["batch_size"]
    lr_pH, lr_pW = lr_d["patch_dim"]
    # tokens per sequence before windowing: the LR tokens (base model) or <start>, then the HR tokens
    graphed_seq = total_hr_Seq + ((img_H // lr_pH) * (img_W // lr_pW) if train_base_model else 1)
    if args["graph_step"]:
        graphed = pipeline.GraphedTrainStep(model, optim, lr_codebook, hr_codebook, train_base_model,
                                            sliding_window if use_sliding_window else None,
                                            label_smoothing=label_smoothing, z_loss=z_loss, **soft)
    global_steps = 0
    done = False
    skipped_before, skipped_run = 0, 0      # --clip-grad-norm: the device's count so far, consecutive skips
    for epoch in range(0, args["max_epoch"]):
        total_loss, total_nll, iteration_count = 0.0, 0.0, 0      # total_nll: with a regulariser only
        averaged = 0            # --clip-grad-norm: the steps in the two running sums (skipped ones are left out)
        for index, feature_map in enumerate(loader):
            iteration_count += 1
            feature_map = feature_map.to(device)
            N = feature_map.shape[0]
            model.train()
            if schedule is not None:     # before every step, eager or replayed (advance_captured reads the group)
                optim.param_groups[0]["lr"] = schedule.lr(optim.step_count + 1)
            if graphed is not None and N == batch_size:
                rand = None
                if use_sliding_window:
                    rand = torch.randint(low=0, high=pipeline.num_windows(graphed_seq, sliding_window),
                                         size=(N * world,))             # CPU global RNG, drawn globally
                    rand = parallel.shard(parallel.broadcast_host_tensor(rand))
                loss = graphed(feature_map, rand)
            else:
                seq_total = graphed_seq
                rand = None
                if use_sliding_window:
                    nwin = pipeline.num_windows(seq_total, sliding_window)
                    rand = torch.randint(low=0, high=nwin, size=(N * world,))   # CPU global RNG
                    rand = parallel.shard(parallel.broadcast_host_tensor(rand))
                if token_noise:      # the assembling launch reads the step word (train_step writes it again)
                    pipeline.set_dropout_step(model, optim)
                hr_in, lr_in, hr_tg, pos_idx = pipeline.tokenize_window(
                    feature_map, lr_codebook, hr_codebook, train_base_model,
                    sliding_window if use_sliding_window else None, rand, token_noise=model.token_noise)
                loss = pipeline.train_step(model, optim, hr_in, lr_in, hr_tg, pos_idx,
                                           pos_bound=seq_total, label_smoothing=label_smoothing,
                                           z_loss=z_loss, **soft)
            nll_val = 0.0
            if regularised:                                          # one read-back for the two numbers
                loss_val, nll_val = pipeline.loss_pair(loss).tolist()
            else:
                loss_val = loss.item()                               # the reference's per-step sync
            ops.check_index_flag(device, "training batch")
            clip = None
            if clip_grad_norm is None:
                if loss_val != loss_val:
                    raise Exception("NaN encountered during training.")
                total_loss += loss_val
                total_nll += nll_val
            else:
                # the device has already decided: a step with a non-finite gradient changed nothing
                clip = optim.clip_stats()
                skipped_run = skipped_run + 1 if clip["skipped"] > skipped_before else 0
                skipped_before = clip["skipped"]
                if skipped_run > max_skipped_steps:
                    raise Exception(f"{skipped_run} consecutive steps skipped for non-finite gradients "
                                    f"(--max-skipped-steps {max_skipped_steps}).")
                if math.isfinite(loss_val) and math.isfinite(clip["norm"]) and math.isfinite(nll_val):
                    total_loss += loss_val
                    total_nll += nll_val
                    averaged += 1
            if schedule is None and global_steps % args["lr_step"] == 0 and global_steps > 0:
                cc.halve_lr(optim)
            if global_steps % args["checkpoint_step"] == 0 and global_steps >= 0 and rank == 0:
                checkpoint(global_steps)
            if val_loader is not None and global_steps % val_step == 0:
                validate(global_steps)
            info("Cum. Steps: {:,} | Steps: {:,} / {:,} | L.R.: {:.8f} | Recon Loss: {:.5f}".format(
                global_steps + 1, index + 1, len(loader), optim.param_groups[0]["lr"],
                total_loss / (iteration_count if clip is None else max(averaged, 1))) +
                (" | NLL: {:.5f}".format(total_nll / (iteration_count if clip is None else max(averaged, 1)))
                 if regularised else "") +
                ("" if clip is None else " | Grad Norm: {:.5f} | Clipped: {:,} | Skipped: {:,}".format(
                    clip["norm"], clip["clipped"], clip["skipped"])))
            global_steps += 1
            if args["max_steps"] is not None and global_steps >= args["max_steps"]:
                done = True
                break
        if done:
            break


if __name__ == "__main__":
    main()
