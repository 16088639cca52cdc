#!/usr/bin/env python3
"""Score a decoder and any number of codebooks on a feature-map dataset without training (additive; the reference
has no evaluation): per codebook the hard-quantisation error in latent space, PSNR / SSIM of the decoded
quantised latent against the autoencoder's own reconstruction, and the usage of the codes (dead codes,
perplexity); with --with-images the same against the source images, and the autoencoder's reconstruction error
itself (qarig/recon_eval.py).  Single-process only."""
import argparse
import json
import logging
import pathlib

import torch

from qarig import cli_common as cc
from qarig import recon_eval
from dataset_loader.feature_map_dataset import FeatureMapDataset


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Evaluate the reconstruction of a decoder and codebooks "
                                            "(single-process only: it is not launched with several ranks).")
    p.add_argument("--device", choices=["cpu", "cuda"], type=str, default="cpu",
                   help="Which hardware device will model run on.")
    p.add_argument("--dataset-path", required=True, type=pathlib.Path,
                   help="File path to feature map dataset json file (read in order).")
    p.add_argument("--decoder-path", required=True, type=pathlib.Path,
                   help="File path to saved decoder / autoencoder checkpoint.")
    p.add_argument("--codebook-path", action="append", default=[], type=pathlib.Path,
                   help="File path to a saved codebook; may be given any number of times (results are keyed by "
                        "the file stem, a repeated stem gets a numeric suffix).")
    p.add_argument("--with-images", action="store_true",
                   help="Load the index's image_path files and score the reconstructions against them too.")
    p.add_argument("--batch-size", type=int, default=8, help="Batch size for dataset.")
    p.add_argument("--max-batches", type=int, default=None, help="Score the first batches only.")
    p.add_argument("--data-range", type=float, default=2.0,
                   help="Peak-to-peak range of the images for PSNR and SSIM (pixels in [-1, 1]: 2).")
    p.add_argument("--topology", action="store_true",
                   help="(additive, not in the reference) also measure every codebook's SOM topology "
                        "(qarig/topology.py): topographic error, index-gap shares and the lag profile, as a "
                        "\"topology\" block per codebook and one Topology line each.")
    p.add_argument("--out-json", type=pathlib.Path, default=None, help="Where the result is written as JSON.")
    return vars(p.parse_args(argv))


def codebook_names(paths):
    """Result keys of the codebook files: the stem, de-duplicated as stem, stem_2, stem_3, ..."""
    names = []
    for path in paths:
        stem, name, k = pathlib.Path(path).stem, pathlib.Path(path).stem, 1
        while name in names:
            k += 1
            name = f"{stem}_{k}"
        names.append(name)
    return names


def main():
    args = parse_args()
    device, world, _ = cc.require_gpu(args["device"])
    if world != 1:
        raise SystemExit("evaluate_reconstruction.py is single-process only")
    logging.basicConfig(format="%(asctime)s %(message)s", level=logging.INFO, force=True)
    decoder, _ = cc.load_decoder(args["decoder_path"], device)
    codebooks = {}
    for name, path in zip(codebook_names(args["codebook_path"]), args["codebook_path"]):
        codebooks[name], _ = cc.load_codebook(path, device, f"codebook {name}")
    dataset = FeatureMapDataset(dataset_path=args["dataset_path"], load_image=args["with_images"],
                                return_filepaths=False)
    loader = torch.utils.data.DataLoader(dataset, batch_size=args["batch_size"], num_workers=2, shuffle=False)
    scorer = recon_eval.ReconScorer(decoder, codebooks, data_range=args["data_range"], topology=args["topology"])
    recon_eval.score_loader(scorer, loader, device, args["max_batches"])
    result = scorer.result()
    if "autoencoder" in result:
        logging.info(recon_eval.recon_summary_line("Eval autoencoder", result["autoencoder"]) +
                     f" | images: {result['images']:,}")
    for name, block in result["codebooks"].items():
        logging.info(recon_eval.recon_summary_line(f"Eval {name}", block) + f" | images: {result['images']:,}")
        if "topology" in block:
            from qarig.topology import topology_summary_line
            logging.info(topology_summary_line(name, block["topology"]))
    if args["out_json"] is not None:
        args["out_json"].parent.mkdir(parents=True, exist_ok=True)
        with open(args["out_json"], "w") as f:
            json.dump(result, f)


if __name__ == "__main__":
    main()
