"""Reconstruction evaluation of the stages upstream of the Transformers (additive; the reference has none): what the
decoder makes of a codebook's hard-quantised latent -- the ceiling of everything the cascade can generate --
against the autoencoder's own reconstruction and, optionally, the source image; the quantisation error in latent
space; and how the codebook's codes are used.

Built like evaluate.TokenScorer: per-image fp64 sums (ops.pair_error, ops.ssim) and int64 usage counts
(ops.index_histogram) stay on the device for a whole dataset and are read back once, in result().  The kernels sum
in one fixed order and an image's value does not depend on its batch, so the same model and data give the same
bits at any batch size (as far as the decoder and the BMU search do)."""
import math

import torch

from . import ops


def error_block(sums, elements, data_range, ssim=None):
    """One comparison's numbers from per-image {sum d^2, sum |d|, max |d|} triples (rows of ops.pair_error, as
    Python floats), `elements` per image and, for images, the per-image SSIM values.  Host arithmetic only."""
    n = len(sums)
    total = n * elements
    finite = all(math.isfinite(v) for s in sums for v in s)      # (a NaN or inf in an image reaches the totals)
    mse = math.fsum(s[0] for s in sums) / total if finite else sum(s[0] for s in sums) / total
    if mse == 0.0:
        psnr = None
    elif math.isfinite(mse):
        psnr = 10.0 * math.log10(data_range * data_range / mse)
    else:
        psnr = math.nan if mse != mse else -math.inf
    worst = [s[2] for s in sums]
    block = {"mse": mse, "mae": (math.fsum(s[1] for s in sums) if finite else sum(s[1] for s in sums)) / total,
             "max_abs": math.nan if any(v != v for v in worst) else max(worst), "psnr": psnr,
             "per_image_mse": [s[0] / elements for s in sums]}
    if ssim is not None:
        block["ssim"] = math.fsum(ssim) / n
        block["per_image_ssim"] = list(ssim)
    return block


def usage_block(counts):
    """Codebook usage from integer counts per code: perplexity = exp(-sum p ln p) over the codes with p > 0."""
    counts = [int(c) for c in counts]
    total = sum(counts)
    used = sum(1 for c in counts if c > 0)
    entropy = -math.fsum((c / total) * math.log(c / total) for c in counts if c > 0) if total else 0.0
    return {"codes": len(counts), "used": used, "dead": len(counts) - used, "perplexity": math.exp(entropy),
            "entropy_bits": entropy / math.log(2.0), "max_share": max(counts) / total if total else 0.0,
            "counts": counts}


class ReconScorer:
    def __init__(self, decoder, codebooks, data_range=2.0, topology=False):
        """topology: also measure every codebook's SOM topology on the same latents (qarig.topology) and add a
        "topology" key to its block."""
        if not float(data_range) > 0.0:
            raise ValueError(f"data_range must be positive, got {data_range}")
        self.decoder = decoder
        self.codebooks = dict(codebooks)
        self.data_range = float(data_range)
        self.device = None
        self._err = {}       # (block, comparison) -> [elements per image, [pair_error (N,3)], [ssim (N,)] or None]
        self._counts = {}    # codebook name -> int64 (K,) on the device
        self._images = 0
        self._topology = None
        if topology:
            from .topology import TopologyScorer
            self._topology = TopologyScorer(self.codebooks)

    def _score(self, block, comparison, got, want, with_ssim):
        entry = self._err.get((block, comparison))
        if entry is None:
            entry = self._err[(block, comparison)] = [got[0].numel(), [], [] if with_ssim else None]
        elif entry[0] != got[0].numel():
            raise ValueError(f"ReconScorer: {comparison} of {got[0].numel()} elements after {entry[0]}")
        entry[1].append(ops.pair_error(got, want))
        if with_ssim:
            entry[2].append(ops.ssim(got, want, data_range=self.data_range))

    @torch.no_grad()
    def add_batch(self, latent, image=None):
        """Scores one batch of latents (N,C,H,W), optionally against their source images (N,H,W,C) in [-1, 1]
        with the decoder's channel order, on the device; nothing is read back."""
        modules = [self.decoder, *self.codebooks.values()]
        modes = [m.training for m in modules]
        for m in modules:
            m.eval()
        try:
            self.device = latent.device
            ref = self.decoder(latent)
            if image is not None:
                image = image.permute(0, 3, 1, 2)
                if image.shape != ref.shape:
                    raise ValueError(f"ReconScorer: images of shape {tuple(image.shape)} (N,C,H,W) against decoder "
                                     f"outputs of shape {tuple(ref.shape)}")
                image = image.float().contiguous()
                self._score("autoencoder", "vs_image", ref, image, True)
            for name, cb in self.codebooks.items():
                ids = cb.get_patches_bmu(latent, reshape=True)
                zq = cb.get_quantized_image(ids)          # hard quantisation: what generation decodes
                img = self.decoder(zq)
                self._score(name, "latent", zq, latent, False)
                self._score(name, "vs_decoder", img, ref, True)
                if image is not None:
                    self._score(name, "vs_image", img, image, True)
                counts = self._counts.get(name)
                if counts is None:
                    counts = self._counts[name] = torch.zeros(cb.num_embeddings, dtype=torch.int64,
                                                              device=latent.device)
                ops.index_histogram(ids, counts)
            if self._topology is not None:
                self._topology.add_batch(latent)
            self._images += latent.shape[0]
        finally:
            for m, mode in zip(modules, modes):
                m.train(mode)

    def _block(self, name):
        out = {}
        for (block, comparison), (elements, errs, ssims) in self._err.items():
            if block == name:
                sums = torch.cat(errs).cpu().tolist()
                out[comparison] = error_block(sums, elements, self.data_range,
                                              torch.cat(ssims).cpu().tolist() if ssims is not None else None)
        return out

    def result(self):
        """The one read-back: {"images", "autoencoder" (when images were given), "codebooks": {name: block}}."""
        if self.device is None:
            raise RuntimeError("ReconScorer.result: no batch was scored")
        ops.check_index_flag(self.device, "reconstruction evaluation")
        r = {"images": self._images}
        if ("autoencoder", "vs_image") in self._err:
            r["autoencoder"] = self._block("autoencoder")
        r["codebooks"] = {}
        topology = self._topology.result() if self._topology is not None else {}
        for name in self.codebooks:
            block = self._block(name)
            block["usage"] = usage_block(self._counts[name].cpu().tolist())
            if name in topology:
                block["topology"] = topology[name]
            r["codebooks"][name] = block
        return r


def score_loader(scorer, batches, device, max_batches=None):
    """Feeds an iterable of latent batches, or of (latent, image) pairs, in order; returns the number scored."""
    n = 0
    for batch in batches:
        if max_batches is not None and n >= max_batches:
            break
        if isinstance(batch, (tuple, list)):
            scorer.add_batch(batch[0].to(device), batch[1].to(device))
        else:
            scorer.add_batch(batch.to(device))
        n += 1
    return n


def without_per_image(block):
    """A copy of a result block without its per-image lists (one log line per evaluation stays short)."""
    return {k: ({c: v for c, v in b.items() if not c.startswith("per_image_")} if k != "usage" else b)
            for k, b in block.items()}


def _psnr(v):
    return "inf" if v is None else "{:.3f}".format(v)


def recon_summary_line(tag, block):
    """One log line for a codebook block (latent error, the decoded image against the autoencoder's, usage) or for
    the autoencoder block (the reconstruction against the source image)."""
    if "latent" not in block:
        e = block["vs_image"]
        return "{} Image MSE: {:.6f} | PSNR: {} | SSIM: {:.5f}".format(tag, e["mse"], _psnr(e["psnr"]), e["ssim"])
    d, u = block["vs_decoder"], block["usage"]
    line = "{} Latent MSE: {:.6f} | PSNR: {} | SSIM: {:.5f} | used: {:,} / {:,} | perplexity: {:.2f}".format(
        tag, block["latent"]["mse"], _psnr(d["psnr"]), d["ssim"], u["used"], u["codes"], u["perplexity"])
    if "vs_image" in block:
        e = block["vs_image"]
        line += " | vs image PSNR: {} | SSIM: {:.5f}".format(_psnr(e["psnr"]), e["ssim"])
    return line
