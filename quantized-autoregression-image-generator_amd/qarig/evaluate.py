"""Held-out evaluation of a Transformer stage (additive; the reference has none): the training objective --
next-token cross-entropy, a token seeing at most its sliding window -- on the deterministic windows of
pipeline.eval_windows, every target position of every sequence scored exactly once.

The forward pass is the training one under torch.no_grad(); the per-row scores (ops.token_score) are reduced per
image, per position and in total into fp64 / int64 accumulators on the device (ops.score_reduce), so a whole
dataset is scored with one read-back, in result().  All sums are deterministic: the same model, data and batch
size give the same bits."""
import math

import torch

from . import ops, pipeline

IGNORE_INDEX = -100


class TokenScorer:
    def __init__(self, model, lr_codebook, hr_codebook, train_base_model, window, topk=5, input_noise=0,
                 cond_noise=0, noise_range=0, noise_seed=0):
        """input_noise / cond_noise / noise_range / noise_seed: the held-out nll under the token noise of training
         -- the decoder's hr tokens and the encoder's lr tokens corrupted, the targets clean -- from a
        key of the scorer's own (rank 0) whose step word is the number of the batch, counted from 0: a
        deterministic function of the dataset order.  All four 0 (the default): no key, today's calls and bits."""
        if int(topk) < 1:
            raise ValueError(f"topk must be at least 1, got {topk}")
        self.noise = None
        self.noise_seed = int(noise_seed)
        self._noise_args = (input_noise, cond_noise, noise_range)
        if input_noise != 0 or cond_noise != 0:
            from .dropout import TokenNoise
            if cond_noise != 0 and train_base_model:
                raise ValueError("TokenScorer: cond_noise needs an encoder-decoder stage")
            self.noise = TokenNoise.probabilities(input_noise, cond_noise, noise_range)     # the key: at the first batch
        elif noise_range != 0 or self.noise_seed != 0:
            raise ValueError("TokenScorer: noise_range / noise_seed without input_noise or cond_noise")
        self._batches = 0
        self.model = model
        self.lr_cb, self.hr_cb = lr_codebook, hr_codebook
        self.base, self.window, self.topk = bool(train_base_model), window, int(topk)
        self.seq_len = None
        self.device = None
        self._img = []            # one fp64 (N,) tensor per batch, in dataset order
        self._offs = {}

    def _starts(self, N, start):
        key = (N, start)
        t = self._offs.get(key)
        if t is None:
            t = self._offs[key] = torch.full((N,), start, dtype=torch.int64, device=self.device)
        return t

    @torch.no_grad()
    def add_batch(self, feature_map):
        """Scores one batch of latents (N,C,H,W) on the device; nothing is read back."""
        model = self.model
        dev = feature_map.device
        N = feature_map.shape[0]
        lr_idx = self.lr_cb.get_patches_bmu(feature_map, reshape=True)
        hr_idx = self.hr_cb.get_patches_bmu(feature_map, reshape=True)
        seq = (lr_idx.shape[1] if self.base else 1) + hr_idx.shape[1]
        if self.seq_len is None:
            self.seq_len, self.device = seq, dev
            self._pos_nll = torch.zeros(seq, dtype=torch.float64, device=dev)
            self._pos_cnt = torch.zeros(seq, dtype=torch.int64, device=dev)
            self._totals = torch.zeros(3, dtype=torch.int64, device=dev)
            if self.noise is not None:
                from .dropout import DropoutKey
                self.noise = self.noise.with_key(DropoutKey(self.noise_seed, 0, dev))
        elif seq != self.seq_len:
            raise ValueError(f"TokenScorer: sequences of {seq} tokens after sequences of {self.seq_len}")
        noise_args = None
        if self.noise is not None:
            self.noise.key.set_step(self._batches)
            noise_args = self.noise.input_args()
            lr_idx = self.noise.corrupt_cond(lr_idx, self.lr_cb.num_embeddings)     # before model.encode
        self._batches += 1
        was_training = model.training
        model.eval()
        try:
            enc = model.encode(lr_idx) if model.use_encoder else None       # once per batch, not per window
            img = torch.zeros(N, dtype=torch.float64, device=dev)
            for start, skip in pipeline.eval_windows(seq, self.window):
                if start is None and model.use_pos_cond:
                    start = 0                    # a window as long as the sequence still carries its positions
                W = seq if start is None or self.window is None else min(int(self.window), seq)
                offs = None if start is None else self._starts(N, start)
                hr_in, hr_tg, pos = ops.assemble_tokens(lr_idx, hr_idx, self.base, self.lr_cb.num_embeddings,
                                                        self.hr_cb.num_embeddings, offs, W, noise=noise_args)
                if skip:
                    hr_tg[:, :skip] = IGNORE_INDEX      # counted by the window before
                logits = model.decode(hr_in, enc, pos, seq)
                nll, rank = ops.token_score(logits.view(-1, logits.shape[-1]), hr_tg.flatten(), IGNORE_INDEX)
                ops.score_reduce(nll, rank, N, W, start or 0, self.topk, img, self._pos_nll, self._pos_cnt,
                                 self._totals)
        finally:
            model.train(was_training)
        self._img.append(img)

    def result(self):
        """The one read-back.  nll_mean in nats per token; per_position_nll / per_image_nll are SUMS of nats (over
        the images at a position, over the tokens of an image: the image's negative log-likelihood), so both add
        up to tokens x nll_mean; per_position_count is the number of tokens behind each position's sum."""
        if self.seq_len is None:
            raise RuntimeError("TokenScorer.result: no batch was scored")
        ops.check_index_flag(self.device, "evaluation tokens")
        totals = [int(v) for v in self._totals.cpu()]
        pos = self._pos_nll.cpu()
        img = torch.cat(self._img).cpu()
        tokens = totals[0]
        mean = float(pos.sum()) / max(tokens, 1)
        return {"tokens": tokens, "images": int(img.numel()), "nll_mean": mean,
                "bits_per_token": mean / math.log(2.0),
                "perplexity": math.exp(mean) if mean < 700.0 else math.inf,
                "top1": totals[1] / max(tokens, 1), "topk": totals[2] / max(tokens, 1), "k": self.topk,
                "per_position_nll": pos.tolist(), "per_position_count": self._pos_cnt.cpu().tolist(),
                "per_image_nll": img.tolist(),
                **({} if self.noise is None else
                   {"input_noise": self.noise.p_input, "cond_noise": self.noise.p_cond,
                    "noise_range": self.noise.neighbour_range, "noise_seed": self.noise_seed})}


def score_loader(scorer, batches, device, max_batches=None):
    """Feeds an iterable of latent batches (in order) to `scorer`; returns the number of batches scored."""
    n = 0
    for feature_map in batches:
        if max_batches is not None and n >= max_batches:
            break
        scorer.add_batch(feature_map.to(device))
        n += 1
    return n


def summary_line(tag, r):
    return "{} Loss: {:.5f} | bits/token: {:.5f} | top-1: {:.4f} | top-{}: {:.4f} | tokens: {:,}".format(
        tag, r["nll_mean"], r["bits_per_token"], r["top1"], r["k"], r["topk"], r["tokens"])
