#!/usr/bin/env python3
"""Train a SOM-style codebook on latent patches on MI355X: same command line, JSON keys,
checkpoint dict and log lines as the reference's train_codebook.py."""
import argparse
import logging
import pathlib

import torch

from models.Codebook import Codebook
from qarig import cli_common as cc
from qarig import functional as QF
from qarig import parallel
from qarig.optim import FlatAdam
from utils.image_utils import save_images
from utils.model_utils import load_model, save_model
from dataset_loader.feature_map_dataset import FeatureMapDataset


def parse_args():
    p = argparse.ArgumentParser(description="Train Codebook models.")
    p.add_argument("--device", choices=["cpu", "cuda"], type=str, default="cpu")
    p.add_argument("--dataset-path", required=True, type=pathlib.Path)
    p.add_argument("--decoder-path", required=True, type=pathlib.Path)
    p.add_argument("--codebook-path", default=None, required=False, type=pathlib.Path)
    p.add_argument("--batch-size", type=int, default=64)
    p.add_argument("--checkpoint-step", type=int, default=1_000)
    p.add_argument("--lr-step", type=int, default=50_000)
    p.add_argument("--max-epoch", type=int, default=1_000)
    p.add_argument("--config-path", required=True, type=pathlib.Path)
    p.add_argument("--out-dir", required=True, type=pathlib.Path)
    p.add_argument("--max-steps", type=int, default=None, help="(additive) stop after N steps.")
    p.add_argument("--val-dataset-path", type=pathlib.Path, default=None,
                   help="(additive; the reference never evaluates) feature map dataset json file of held-out latents: "
                        "every --val-step steps rank 0 scores the codebook on it (qarig/recon_eval.py: hard "
                        "quantisation, the decoded image against the autoencoder's own), logs Val Latent MSE | PSNR | "
                        "SSIM | used | perplexity and appends one JSON line to <out-dir>/val_log.jsonl")
    p.add_argument("--val-step", type=int, default=None, help="Steps between evaluations (default: --checkpoint-step).")
    p.add_argument("--val-batches", type=int, default=None, help="Score the first batches of the held-out set only.")
    p.add_argument("--val-topology", action="store_true",
                   help="(additive, not in the reference) the validation pass also measures the codebook's SOM topology "
                        "(qarig/topology.py): a \"topology\" block in val_log.jsonl and ' | TE: <topographic error>' on "
                        "the Val line.  Needs --val-dataset-path.")
    args = p.parse_args()
    if args.val_topology and args.val_dataset_path is None:
        p.error("--val-topology needs --val-dataset-path")
    return vars(args)


def main():
    project_name = "Codebook"
    args = parse_args()
    cfg = cc.read_config(args["config_path"])
    device, world, rank = cc.require_gpu(args["device"])
    out_dir = args["out_dir"]
    cc.setup_logging(out_dir, project_name, rank)
    info = logging.info
    decoder_model, _ = cc.load_decoder(args["decoder_path"], device)
    decoder_model.eval()
    model_lr, neighbourhood_step = cfg["model_lr"], cfg["neighbourhood_step"]
    global_steps = 0
    if args["codebook_path"] is not None:
        ok, d = load_model(args["codebook_path"])
        if not ok:
            raise Exception("An error occured while loading codebook checkpoint!")
        patch_dim, image_dim, image_C = d["patch_dim"], d["image_dim"], d["image_C"]
        codebook = Codebook(patch_dim=patch_dim, image_dim=image_dim, image_channel=image_C,
                            num_embeddings=d["num_embeddings"],
                            init_neighbour_range=d["neighbourhood_range"])
        codebook.custom_load_state_dict(d["checkpoint"])
        global_steps = d["global_steps"]
    else:
        image_dim = (cfg["image_H"], cfg["image_W"])
        image_C = cfg["image_C"]
        patch_dim = (cfg["patch_H"], cfg["patch_W"])
        codebook = Codebook(patch_dim=patch_dim, image_dim=image_dim, image_channel=image_C,
                            num_embeddings=cfg["num_embeddings"],
                            init_neighbour_range=cfg["num_embeddings"] // 2)
    codebook = codebook.to(device)
    optim = FlatAdam(codebook.parameters(), lr=model_lr, betas=(0.5, 0.999))
    parallel.broadcast_params(optim)
    dataset = FeatureMapDataset(dataset_path=args["dataset_path"], load_image=False,
                                return_filepaths=False)
    loader = cc.ShardedLoader(dataset, args["batch_size"], num_workers=4, shuffle=True)
    val_loader, val_step = cc.build_validation(args, rank, info)

    def validate(global_steps):
        """Rank 0 alone, like the checkpoint: the other ranks wait at their next exchange."""
        from qarig import recon_eval
        scorer = recon_eval.ReconScorer(decoder_model, {"codebook": codebook}, topology=args["val_topology"])
        recon_eval.score_loader(scorer, val_loader, device, args["val_batches"])
        block = recon_eval.without_per_image(scorer.result()["codebooks"]["codebook"])
        line = recon_eval.recon_summary_line("Val", block)
        if args["val_topology"]:
            line += " | TE: {:.4f}".format(block["topology"]["topographic_error"])
        cc.validate(out_dir, {"step": global_steps, "codebook": block}, [line], info)

    info(f"{project_name}")
    info(f"Output Dir: {out_dir}")
    info(f"Patch dim: {patch_dim} | Image dim: {image_dim} | Num Embeddings: {codebook.num_embeddings:,}")
    info("#" * 100)

    done = False
    for epoch in range(0, args["max_epoch"]):
        iteration_count, total = 0, 0.0
        for index, fm in enumerate(loader):
            iteration_count += 1
            fm = fm.to(device)
            codebook.train()
            optim.zero_grad()
            quant = codebook(fm, use_gaussian=True)
            loss = QF.mse_loss(quant, fm)
            loss.backward()
            if world > 1:
                parallel.allreduce_flat(optim.flat_grad)
            optim.step(grad_scale=1.0 / world)
            lv = loss.item()
            if lv != lv:
                raise Exception("NaN encountered during training")
            total += lv
            if global_steps % args["lr_step"] == 0 and global_steps > 0:
                cc.halve_lr(optim)
            if global_steps % args["checkpoint_step"] == 0 and rank == 0:
                with torch.no_grad():
                    save_images(decoder_model(fm), f"image_plot_{global_steps}", out_dir, logging=info)
                    save_images(decoder_model(quant.detach()), f"quant_image_plot_{global_steps}",
                                out_dir, logging=info)
                d = {"patch_dim": patch_dim, "image_dim": image_dim, "image_C": image_C,
                     "num_embeddings": codebook.num_embeddings,
                     "neighbourhood_range": codebook.neighbourhood_range,
                     "global_steps": global_steps,
                     "checkpoint": {k: v.detach().clone() for k, v in codebook.state_dict().items()}}
                ok = save_model(model_dict=d, dest_path=out_dir, file_name=f"codebook_{global_steps}.pt",
                                logging=info)
                info("Successfully saved model." if ok else "Error occured saving model.")
            if val_loader is not None and global_steps % val_step == 0:
                validate(global_steps)
            info("Cum. Steps: {:,} | Steps: {:,} / {:,} | L.R.: {:.8f} | Recon Loss: {:.5f} | "
                 "Neighbourhood Range: {}".format(global_steps + 1, index + 1, len(loader),
                                                  optim.param_groups[0]["lr"], total / iteration_count,
                                                  codebook.neighbourhood_range))
            global_steps += 1
            if global_steps % neighbourhood_step == 0:
                codebook.decrease_neighbourhood(steps=1)
            if args["max_steps"] is not None and iteration_count >= args["max_steps"]:
                done = True
                break
        if done:
            break


if __name__ == "__main__":
    main()
