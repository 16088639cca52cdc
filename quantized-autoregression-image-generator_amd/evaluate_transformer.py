#!/usr/bin/env python3
"""Score a Transformer-stage checkpoint on a feature-map dataset without training (additive; the reference has
no evaluation): held-out loss in nats and bits per token, perplexity, top-1 / top-k accuracy, and the loss per
sequence position and per image.  The objective is the training one -- a token sees at most the checkpoint's
sliding window -- on deterministic windows that count every token once (qarig/evaluate.py)."""
import argparse
import json
import logging
import pathlib

import torch

from models.Transformer import Transformer
from qarig import cli_common as cc
from qarig import evaluate
from utils.model_utils import load_model
from dataset_loader.feature_map_dataset import FeatureMapDataset


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Evaluate a Quantized Transformer checkpoint.")
    p.add_argument("--device", choices=["cpu", "cuda"], type=str, default="cpu",
                   help="Which hardware device will model run on.")
    p.add_argument("--dataset-path", required=True, type=pathlib.Path,
                   help="File path to feature map dataset json file (read in order).")
    p.add_argument("--lr-codebook-path", required=True, type=pathlib.Path,
                   help="File path to saved Low-Res codebook.")
    p.add_argument("--hr-codebook-path", required=True, type=pathlib.Path,
                   help="File path to saved High-Res codebook.")
    p.add_argument("--model-path", required=True, type=pathlib.Path,
                   help="File path to saved model checkpoint (train_quantized_transformer.py).")
    p.add_argument("--batch-size", type=int, default=8, help="Batch size for dataset.")
    p.add_argument("--max-batches", type=int, default=None, help="Score the first batches only.")
    p.add_argument("--use-ema", action="store_true",
                   help="Score the exponential moving average of the weights (the checkpoint's 'model_ema', "
                        "written with --ema-decay) instead of the last-step weights.")
    p.add_argument("--topk", type=int, default=5, help="k of the top-k accuracy.")
    p.add_argument("--input-noise", type=cc.input_noise_arg, default=0.0,
                   help="Score under the token noise of training (train_quantized_transformer.py --input-noise): each HR "
                        "token the decoder reads is replaced with probability P in (0, 0.9]; the targets stay clean.  "
                        "0 = off.")
    p.add_argument("--cond-noise", type=cc.cond_noise_arg, default=0.0,
                   help="The same for the LR tokens an encoder-decoder stage conditions on.  0 = off.")
    p.add_argument("--noise-range", type=int, default=0,
                   help="Replacements are drawn from the codes within R of the token's own; 0 = the whole codebook.")
    p.add_argument("--noise-seed", type=cc.dropout_seed_arg, default=0,
                   help="64-bit seed of the noise; the step word is the batch number, so the result is a function of "
                        "the dataset order.")
    p.add_argument("--out-json", type=pathlib.Path, default=None, help="Where the result is written as JSON.")
    return vars(p.parse_args(argv))


def main():
    args = parse_args()
    device, _, _ = cc.require_gpu(args["device"])
    logging.basicConfig(format="%(asctime)s %(message)s", level=logging.INFO, force=True)
    lr_codebook, _ = cc.load_codebook(args["lr_codebook_path"], device, "Low-Resolution codebook")
    hr_codebook, _ = cc.load_codebook(args["hr_codebook_path"], device, "High-Resolution codebook")
    ok, md = load_model(args["model_path"])
    if not ok:
        raise Exception("An error occured while loading model checkpoint!")
    if args["use_ema"] and "model_ema" not in md:
        raise SystemExit(f"--use-ema: {args['model_path']} holds no 'model_ema' (train with --ema-decay)!")
    model = Transformer(
        use_encoder=not md["train_base_model"], use_pos_cond=md["use_sliding_window"],
        num_enc_layers=md["num_enc_layers"], num_dec_layers=md["num_dec_layers"],
        num_enc_embedding=md["num_enc_embedding"], num_dec_embedding=md["num_dec_embedding"],
        self_attn_heads=md["self_attn_heads"], cross_attn_heads=md["cross_attn_heads"],
        transformer_in_dim=md["transformer_in_dim"], transformer_out_dim=md["transformer_out_dim"],
        transformer_hidden_dim=md["transformer_hidden_dim"], hidden_activation=md["hidden_activation"])
    model.custom_load_state_dict(md["model_ema" if args["use_ema"] else "model"])
    model = model.to(device).eval()
    try:
        input_noise, cond_noise, noise_range, noise_seed = cc.check_token_noise_args(
            args["input_noise"], args["cond_noise"], args["noise_range"], args["noise_seed"],
            train_base_model=md["train_base_model"], k_lr=lr_codebook.num_embeddings, k_hr=hr_codebook.num_embeddings)
    except ValueError as e:
        raise SystemExit(str(e))

    dataset = FeatureMapDataset(dataset_path=args["dataset_path"], load_image=False, return_filepaths=False)
    loader = torch.utils.data.DataLoader(dataset, batch_size=args["batch_size"], num_workers=2, shuffle=False)
    scorer = evaluate.TokenScorer(model, lr_codebook, hr_codebook, md["train_base_model"],
                                  md["sliding_window"] if md["use_sliding_window"] else None, topk=args["topk"],
                                  input_noise=input_noise, cond_noise=cond_noise,
                                  noise_range=noise_range if input_noise or cond_noise else 0,
                                  noise_seed=noise_seed if input_noise or cond_noise else 0)
    evaluate.score_loader(scorer, loader, device, args["max_batches"])
    result = scorer.result()
    result["weights"] = "model_ema" if args["use_ema"] else "model"
    for k, v in (("input_noise", input_noise), ("cond_noise", cond_noise), ("noise_range", noise_range),
                 ("noise_seed", noise_seed)):
        result.setdefault(k, v)         # the four values are recorded with and without noise
    logging.info(evaluate.summary_line("Eval", result) + f" | images: {result['images']:,}")
    if args["out_json"] is not None:
        args["out_json"].parent.mkdir(parents=True, exist_ok=True)
        with open(args["out_json"], "w") as f:
            json.dump(result, f)


if __name__ == "__main__":
    main()
