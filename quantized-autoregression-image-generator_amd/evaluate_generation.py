#!/usr/bin/env python3
"""Score generated samples against a feature-map dataset without an Inception network (additive; the reference has
no evaluation): the Frechet distance between the pooled latents of the dataset and the latents that
generate_images.py --save-latents wrote -- or between their decoded images with --space image -- next to two floors:
what hard quantisation with the HR codebook alone costs, and the distance between two halves of the real set (the
sampling noise of this many samples) (qarig/gen_eval.py).  The number is NOT FID: it is comparable only between
runs that share the autoencoder, --feature-pool and --space.  --knn K adds k-nearest-neighbour precision, recall,
density and coverage and the generated samples' distances to their nearest real sample, beside the same statistics of
the two real halves; --save-neighbours writes every generated sample's nearest real sample.  Single-process only."""
import argparse
import json
import logging
import pathlib

import numpy as np
import torch

from qarig import cli_common as cc
from qarig import gen_eval
from dataset_loader.feature_map_dataset import FeatureMapDataset


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Evaluate generated latents against a feature-map dataset: Frechet "
                                            "distance in latent (or decoded-image) space, not FID "
                                            "(single-process only: it is not launched with several ranks).")
    p.add_argument("--device", choices=["cpu", "cuda"], type=str, default="cpu",
                   help="Which hardware device will model run on.")
    p.add_argument("--real-dataset-path", required=True, type=pathlib.Path,
                   help="File path to feature map dataset json file: the real latents (read in order).")
    p.add_argument("--generated-latents", required=True, type=pathlib.Path,
                   help="fp32 (N,C,H,W) .npy file written by generate_images.py --save-latents.")
    p.add_argument("--hr-codebook-path", type=pathlib.Path, default=None,
                   help="File path to the last stage's HR codebook: adds the hard-quantised real latents as a set "
                        "(the floor the codebook alone sets).")
    p.add_argument("--decoder-path", type=pathlib.Path, default=None,
                   help="File path to saved decoder / autoencoder checkpoint (required with --space image).")
    p.add_argument("--space", choices=["latent", "image"], default="latent",
                   help="Features from the latents themselves or from their decoded images.")
    p.add_argument("--feature-pool", type=int, default=1,
                   help="Mean-pool P x P blocks before taking moments; P must divide the height and width, and "
                        "channels x (H/P) x (W/P) may be at most 1024.")
    p.add_argument("--batch-size", type=int, default=64, help="Batch size for both sets.")
    p.add_argument("--max-batches", type=int, default=None, help="Score the first batches of the real set only.")
    p.add_argument("--out-json", type=pathlib.Path, default=None, help="Where the result is written as JSON.")
    p.add_argument("--knn", type=int, default=0,
                   help="k of the k-nearest-neighbour precision / recall / density / coverage (0 = off; 3 and 5 are "
                        "the usual values, at most 8).  The values depend on k and on both sample counts.")
    p.add_argument("--knn-max-samples", type=int, default=gen_eval.KNN_MAX_SAMPLES,
                   help="With --knn: the first N samples of each set are kept for the neighbour statistics.")
    p.add_argument("--save-neighbours", type=pathlib.Path, default=None,
                   help="With --knn: write an .npz with, per generated sample, the index (dataset order) of its "
                        "nearest real sample and the distance to it.")
    args = vars(p.parse_args(argv))
    if args["space"] == "image" and args["decoder_path"] is None:
        p.error("--space image needs --decoder-path")
    if args["feature_pool"] < 1 or args["batch_size"] < 1:
        p.error("--feature-pool and --batch-size must be positive")
    if not 0 <= args["knn"] <= gen_eval.MAX_KNN:
        p.error(f"--knn must be 0 (off) ... {gen_eval.MAX_KNN}")
    if args["knn_max_samples"] < 1:
        p.error("--knn-max-samples must be positive")
    if args["save_neighbours"] is not None and args["knn"] == 0:
        p.error("--save-neighbours needs --knn")
    return args


def feature_dim(shape, pool):
    """D of samples of shape (C,H,W) pooled by `pool`; SystemExit when the pool does not fit or D exceeds the limit."""
    C, H, W = shape
    if H % pool or W % pool:
        raise SystemExit(f"--feature-pool {pool} does not divide the {H} x {W} samples")
    D = C * (H // pool) * (W // pool)
    if D > gen_eval.MAX_DIM:
        raise SystemExit(f"{C} x {H // pool} x {W // pool} = {D:,} features per sample exceed {gen_eval.MAX_DIM:,}: "
                         f"pass a larger --feature-pool")
    return D


def check_knn_counts(k, n_real, n_generated):
    """SystemExit unless real, its two halves and the generated set all hold at least k + 1 samples."""
    sets = {"real": n_real, "real_a": (n_real + 1) // 2, "real_b": n_real // 2, "generated": n_generated}
    small = [f"{name} ({n})" for name, n in sets.items() if n < k + 1]
    if small:
        raise SystemExit(f"--knn {k} needs at least {k + 1} samples in every set (the real set is also split into "
                         f"halves): too few in {', '.join(small)}")


def main():
    args = parse_args()
    device, world, _ = cc.require_gpu(args["device"])
    if world != 1:
        raise SystemExit("evaluate_generation.py is single-process only")
    logging.basicConfig(format="%(asctime)s %(message)s", level=logging.INFO, force=True)
    dataset = FeatureMapDataset(dataset_path=args["real_dataset_path"], load_image=False, return_filepaths=False)
    generated = np.load(args["generated_latents"])
    real_shape = tuple(dataset[0].shape)
    if generated.ndim != 4 or generated.dtype != np.float32 or tuple(generated.shape[1:]) != real_shape:
        raise SystemExit(f"--generated-latents holds {generated.dtype} {tuple(generated.shape)}, the dataset's latents "
                         f"are float32 (N, {', '.join(map(str, real_shape))}): the two do not share an autoencoder")
    decoder = hr_codebook = None
    if args["decoder_path"] is not None:
        decoder, _ = cc.load_decoder(args["decoder_path"], device)
    if args["hr_codebook_path"] is not None:
        hr_codebook, _ = cc.load_codebook(args["hr_codebook_path"], device, "HR codebook")
    pool = args["feature_pool"]
    if args["space"] == "image":
        with torch.no_grad():
            shape = tuple(decoder.eval()(torch.from_numpy(generated[:1]).to(device)).shape[1:])
    else:
        shape = real_shape
    D = feature_dim(shape, pool)

    if args["knn"]:
        n_real = len(dataset)
        if args["max_batches"] is not None:
            n_real = min(n_real, args["max_batches"] * args["batch_size"])
        check_knn_counts(args["knn"], min(n_real, args["knn_max_samples"]),
                         min(generated.shape[0], args["knn_max_samples"]))
    scorer = gen_eval.GenerationScorer(pool, space=args["space"], decoder=decoder, hr_codebook=hr_codebook,
                                       knn=args["knn"], knn_max_samples=args["knn_max_samples"])
    loader = torch.utils.data.DataLoader(dataset, batch_size=args["batch_size"], num_workers=2, shuffle=False)
    for i, batch in enumerate(loader):
        if args["max_batches"] is not None and i >= args["max_batches"]:
            break
        scorer.add(batch.to(device), "real")
    for lo in range(0, generated.shape[0], args["batch_size"]):
        scorer.add(torch.from_numpy(generated[lo:lo + args["batch_size"]]).to(device), "generated")
    result = scorer.result()
    for name, n in result["counts"].items():
        if n < 2 * D:
            logging.warning(f"Warning: set '{name}' has {n:,} samples for D = {D:,} features (fewer than 2 D): its "
                            f"covariance is rank-deficient or poorly estimated and the distance is biased upward")
    logging.info(gen_eval.summary_line("Eval generation", result))
    if args["knn"]:
        m = result["manifold"]
        for name, n in m["dropped"].items():
            if n:
                logging.warning(f"Warning: --knn-max-samples {args['knn_max_samples']:,} dropped {n:,} samples of set "
                                f"'{name}' from the neighbour statistics (the Frechet distance uses all of them)")
        for key in ("nn_generated_real", "nn_real_split"):
            logging.info(f"Eval generation nearest-neighbour distance {key[3:]} | " +
                         " ".join(f"{q}={v:.6g}" for q, v in m[key].items()))
    if args["save_neighbours"] is not None:
        idx, d2 = gen_eval.nearest_real(scorer.bank("generated"), scorer.bank("real"), scorer.shift)
        args["save_neighbours"].parent.mkdir(parents=True, exist_ok=True)
        with open(args["save_neighbours"], "wb") as f:      # a file object: np.savez would append .npz to a path
            np.savez(f, index=idx.cpu().numpy(), distance=np.sqrt(np.maximum(d2.cpu().numpy(), 0.0)))
    if args["out_json"] is not None:
        args["out_json"].parent.mkdir(parents=True, exist_ok=True)
        with open(args["out_json"], "w") as f:
            json.dump(result, f)


if __name__ == "__main__":
    main()
