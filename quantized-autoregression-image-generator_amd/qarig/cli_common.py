"""Shared plumbing of the re-hosted command lines (same flags, JSON keys, log lines,
checkpoint dicts and output tree as the reference's scripts)."""
import json
import logging
import os

import torch

from . import parallel


def require_gpu(device):
    if device != "cuda":
        raise SystemExit("this build runs on MI355X only: pass --device cuda "
                         "(PyTorch-ROCm names the HIP device 'cuda'); there is no CPU path")
    if not torch.cuda.is_available():
        raise SystemExit("--device cuda requested but no GPU is visible")
    world, rank, local = parallel.init()
    local %= torch.cuda.device_count()      # (more ranks than GPUs: gloo tests on a one-GPU box share the device)
    torch.cuda.set_device(local)
    return torch.device("cuda", local), world, rank


def read_config(path):
    with open(path, "r") as f:
        return json.loads(f.read())


def setup_logging(out_dir, project_name, rank=0):
    os.makedirs(out_dir, exist_ok=True)
    handlers = [logging.StreamHandler()]
    if rank == 0:
        handlers.insert(0, logging.FileHandler(os.path.join(out_dir, f"{project_name}.log")))
    logging.basicConfig(format="%(asctime)s %(message)s", encoding="utf-8", handlers=handlers,
                        level=logging.DEBUG if rank == 0 else logging.WARNING, force=True)


def load_decoder(path, device):
    """FC_Decoder rebuilt from an autoencoder/decoder checkpoint dict
    (reference train_quantized_transformer.py:186-208)."""
    from models.FC_Decoder import FC_Decoder
    from utils.model_utils import load_model
    ok, d = load_model(path)
    if not ok:
        raise Exception("An error occured while loading decoder model checkpoint!")
    dec = FC_Decoder(num_layers=d["num_layers"], image_channel=d["image_channel"],
                     min_channel=d["min_channel"], max_channel=d["max_channel"],
                     latent_channel=d["latent_channel"],
                     hidden_activation_type=d["hidden_activation_type"],
                     use_final_activation=d["use_final_dec_activation"],
                     final_activation_type=d["decoder_activation_type"]).to(device)
    dec.custom_load_state_dict(d["model"])
    return dec, d


def load_codebook(path, device, what="codebook"):
    """Codebook rebuilt from its checkpoint dict (reference :211-255)."""
    from models.Codebook import Codebook
    from utils.model_utils import load_model
    ok, d = load_model(path)
    if not ok:
        raise Exception(f"An error occured while loading {what} checkpoint!")
    cb = Codebook(patch_dim=d["patch_dim"], image_dim=d["image_dim"], image_channel=d["image_C"],
                  num_embeddings=d["num_embeddings"],
                  init_neighbour_range=d["neighbourhood_range"]).to(device)
    cb.custom_load_state_dict(d["checkpoint"])
    return cb, d


class ShardedLoader:
    """Batches of a Dataset with a shuffle drawn ONCE per epoch from the global CPU
    generator and sliced per rank (same permutation on every rank), so that a DP run on
    identical inputs reproduces the single-process order.  At world 1 it is
    torch's own DataLoader(shuffle=True), i.e. the reference's loader."""

    def __init__(self, dataset, batch_size, num_workers=4, shuffle=True, drop_last=False):
        self.dataset, self.batch_size = dataset, batch_size
        self.world, self.rank = parallel.world_size(), parallel.rank()
        self.num_workers, self.shuffle = num_workers, shuffle
        self._plain = None
        if self.world == 1:
            self._plain = torch.utils.data.DataLoader(dataset, batch_size=batch_size,
                                                      num_workers=num_workers, shuffle=shuffle,
                                                      drop_last=drop_last)

    def __len__(self):
        if self._plain is not None:
            return len(self._plain)
        return len(self.dataset) // (self.batch_size * self.world)

    def __iter__(self):
        if self._plain is not None:
            yield from self._plain
            return
        n = len(self.dataset)
        order = torch.randperm(n) if self.shuffle else torch.arange(n)
        order = parallel.broadcast_host_tensor(order)   # rank 0's draw, on every rank
        per = self.batch_size * self.world
        for b in range(n // per):
            idx = order[b * per + self.rank * self.batch_size:
                        b * per + (self.rank + 1) * self.batch_size].tolist()
            yield torch.utils.data.default_collate([self.dataset[i] for i in idx])


def build_validation(args, rank, info):
    """--val-dataset-path / --val-step of a training command line: (loader, step) on rank 0 when the flag is given,
    (None, None) otherwise.  The held-out latents are read in order, with a generator of the loader's own, so that
    the training run draws what it draws without validation."""
    if args.get("val_dataset_path") is None or rank != 0:
        return None, None
    from dataset_loader.feature_map_dataset import FeatureMapDataset
    step = args["val_step"] if args.get("val_step") is not None else args["checkpoint_step"]
    val_set = FeatureMapDataset(dataset_path=args["val_dataset_path"], load_image=False, return_filepaths=False)
    loader = torch.utils.data.DataLoader(val_set, batch_size=args["batch_size"], num_workers=2, shuffle=False,
                                         generator=torch.Generator())
    info(f"Validation: {len(val_set):,} latents every {step:,} steps")
    return loader, step


def validate(out_dir, entry, lines, info):
    """One evaluation of a training run: its log lines, and `entry` appended to <out-dir>/val_log.jsonl."""
    for line in lines:
        info(line)
    with open(os.path.join(out_dir, "val_log.jsonl"), "a") as f:
        f.write(json.dumps(entry) + "\n")


def label_smoothing_arg(text):
    """argparse type of --label-smoothing: a float in [0, 1)."""
    import argparse
    try:
        v = float(text)
    except ValueError:
        v = float("nan")
    if not 0.0 <= v < 1.0:
        raise argparse.ArgumentTypeError(f"--label-smoothing must lie in [0, 1), got {text}")
    return v


def z_loss_arg(text):
    """argparse type of --z-loss: a finite float >= 0."""
    import argparse
    try:
        v = float(text)
    except ValueError:
        v = float("nan")
    if not 0.0 <= v < float("inf"):
        raise argparse.ArgumentTypeError(f"--z-loss must be finite and >= 0, got {text}")
    return v


def add_regulariser_args(p):
    """--label-smoothing / --z-loss of a Transformer training command line (both additive, both 0 by default)."""
    p.add_argument("--label-smoothing", type=label_smoothing_arg, default=0.0,
                   help="(additive; the reference trains with plain cross-entropy) epsilon in [0, 1): train against "
                        "torch.nn.CrossEntropyLoss(label_smoothing=epsilon); 0 = off.  Costs the step nothing: the "
                        "term lives in the fused cross-entropy launch.  The step line then shows the objective as "
                        "Recon Loss and the plain loss as NLL; validation and evaluate_transformer.py always report "
                        "the plain nll, so their numbers stay comparable across regularisation settings")
    p.add_argument("--z-loss", type=z_loss_arg, default=0.0,
                   help="(additive) zeta >= 0: add zeta * mean(logsumexp(logits)^2) to the training loss (keeps the "
                        "classifier's log-partition from drifting, e.g. 1e-4; 0 = off), inside the same fused launch.  "
                        "Logged and evaluated as --label-smoothing describes")


def neighbour_smoothing_arg(text):
    """argparse type of --neighbour-smoothing: a float in [0, 1)."""
    import argparse
    try:
        v = float(text)
    except ValueError:
        v = float("nan")
    if not 0.0 <= v < 1.0:
        raise argparse.ArgumentTypeError(f"--neighbour-smoothing must lie in [0, 1), got {text}")
    return v


def neighbour_range_arg(text):
    """argparse type of --neighbour-range: an integer in 1 .. 31."""
    import argparse
    try:
        v = int(text)
    except ValueError:
        v = 0
    if not 1 <= v <= 31:
        raise argparse.ArgumentTypeError(f"--neighbour-range must be an integer in 1 .. 31, got {text}")
    return v


def neighbour_sigma_arg(text):
    """argparse type of --neighbour-sigma: a finite float > 0."""
    import argparse
    try:
        v = float(text)
    except ValueError:
        v = float("nan")
    if not 0.0 < v < float("inf"):
        raise argparse.ArgumentTypeError(f"--neighbour-sigma must be finite and > 0, got {text}")
    return v


def add_neighbour_args(p):
    """--neighbour-smoothing / --neighbour-range / --neighbour-sigma of a Transformer training command line (additive,
    off by default)."""
    p.add_argument("--neighbour-smoothing", type=neighbour_smoothing_arg, default=0.0,
                   help="(additive) nu in [0, 1), nu + --label-smoothing < 1: that much of the target's mass goes to "
                        "the HR codes within --neighbour-range of the target's index -- the codebooks are SOMs, "
                        "neighbouring indices decode to similar patches -- by a Gaussian of the index distance, clamped "
                        "at the ends of the axis and renormalised; <end> is nobody's neighbour and an <end> target is "
                        "not smoothed.  0 = off.  One more term of the fused cross-entropy launch.  Logged and "
                        "evaluated as --label-smoothing describes")
    p.add_argument("--neighbour-range", type=neighbour_range_arg, default=None,
                   help="(additive) R in 1 .. 31: the codes either side of the target that share "
                        "--neighbour-smoothing; required with it, refused without it")
    p.add_argument("--neighbour-sigma", type=neighbour_sigma_arg, default=None,
                   help="(additive) width > 0 of the Gaussian of the index distance (default R / 2)")


def check_neighbour_args(label_smoothing, z_loss, neighbour_smoothing, neighbour_range, neighbour_sigma, codes=None):
    """(nu, R, sigma) once more before anything is launched with them, or ValueError, worded by flag: what holds
    between the flags (nu + --label-smoothing < 1, nu > 0 needs R, R or sigma need nu > 0).  Off: (0.0, None, None)."""
    from . import ops
    try:
        _, _, nu, R, sigma = ops.check_ce_soft(label_smoothing, z_loss, neighbour_smoothing, neighbour_range,
                                               neighbour_sigma, 1 if codes is None else codes)
    except ValueError as e:
        text = str(e)
        for name in ("label_smoothing", "neighbour_smoothing", "neighbour_range", "neighbour_sigma", "z_loss"):
            text = text.replace(name, "--" + name.replace("_", "-"))
        raise ValueError(text)
    return nu, R, sigma


def dropout_arg(text):
    """argparse type of --dropout: 0 (off) or a probability qarig.dropout.threshold_and_scale accepts."""
    import argparse
    from .dropout import threshold_and_scale
    try:
        v = float(text)
        if v != 0.0:
            threshold_and_scale(v)
    except ValueError:
        raise argparse.ArgumentTypeError(f"--dropout must be 0 or lie in (0, 0.9], got {text}")
    return v


def dropout_seed_arg(text):
    """argparse type of --dropout-seed: an unsigned 64-bit integer (decimal, or 0x... hexadecimal)."""
    import argparse
    try:
        v = int(text, 0)
    except ValueError:
        v = -1
    if not 0 <= v < 1 << 64:
        raise argparse.ArgumentTypeError(f"--dropout-seed must be an integer in [0, 2^64), got {text}")
    return v


def add_dropout_args(p):
    """--dropout / --dropout-seed of a Transformer training command line (both additive, both 0 by default)."""
    p.add_argument("--dropout", type=dropout_arg, default=0.0,
                   help="(additive; the reference has no dropout) drop probability P in (0, 0.9] of the residual and "
                        "embedding dropout (0 = off, nothing is launched): applied to the two embedding outputs and "
                        "to every sublayer output entering its residual layer, in training steps only (sampling, "
                        "validation and generation never see it).  The mask is a counter-based function of "
                        "(--dropout-seed, rank, optimizer step, site, element): no generator state, the same masks "
                        "with --graph-step and --use-activation-checkpoint, and a run resumed with --load-optim "
                        "continues the sequence")
    p.add_argument("--dropout-seed", type=dropout_seed_arg, default=0,
                   help="(additive) 64-bit seed of the --dropout masks (default 0).")


def check_dropout_args(dropout, dropout_seed):
    """(p, seed) once more before anything is launched with them (argparse has checked both), or ValueError."""
    from .dropout import threshold_and_scale
    p, seed = float(dropout), int(dropout_seed)
    if p != 0.0:
        threshold_and_scale(p)
    if not 0 <= seed < 1 << 64:
        raise ValueError(f"--dropout-seed must be an integer in [0, 2^64), got {dropout_seed}")
    return p, seed


def attn_dropout_arg(text):
    """argparse type of --attn-dropout: 0 (off) or a probability qarig.dropout.threshold_and_scale accepts."""
    import argparse
    from .dropout import threshold_and_scale
    try:
        v = float(text)
        if v != 0.0:
            threshold_and_scale(v)
    except ValueError:
        raise argparse.ArgumentTypeError(f"--attn-dropout must be 0 or lie in (0, 0.9], got {text}")
    return v


def add_attn_dropout_args(p):
    """--attn-dropout of a Transformer training command line (additive, 0 by default; shares --dropout-seed)."""
    p.add_argument("--attn-dropout", type=attn_dropout_arg, default=0.0,
                   help="(additive; the reference has no dropout) drop probability P in (0, 0.9] of the attention "
                        "probabilities (0 = off: the plain attention kernels, nothing else is launched or allocated): "
                        "every softmax row of every attention layer loses each entry with probability P and the kept "
                        "ones are scaled by 1 / (1 - P), in training steps only.  The mask is generated inside the fused "
                        "attention kernels from (--dropout-seed, rank, optimizer step, layer, sequence, head, query, "
                        "key) and never stored; it is independent of the --dropout masks under the same seed.  Not "
                        "available for models whose head dim runs on the head-dim-128 kernel")


def check_attn_dropout_args(attn_dropout, dropout_seed, sites=1, batch=1, heads=1, seq_q=1, seq_k=1):
    """(p, seed) once more before anything is launched with them, or ValueError.  With p > 0 also what the
    attention entry points would refuse at the first step (include/qarig.h qarig_attention_dropout_fwd): more
    than 256 attention layers (the site is eight bits of a counter word), more than 2^26 keys, and
    batch * heads * queries not below 2^32 (one counter word)."""
    from .dropout import ATTN_DROPOUT_MAX_KEYS, ATTN_DROPOUT_SITES, MAX_THRESHOLD, threshold_and_scale
    p, seed = float(attn_dropout), int(dropout_seed)
    if not 0 <= seed < 1 << 64:
        raise ValueError(f"--dropout-seed must be an integer in [0, 2^64), got {dropout_seed}")
    if p == 0.0:
        return p, seed
    t, _ = threshold_and_scale(p)
    assert 1 <= t <= MAX_THRESHOLD
    if not 1 <= int(sites) <= ATTN_DROPOUT_SITES:
        raise ValueError(f"--attn-dropout: {sites} attention layers; the mask numbers at most {ATTN_DROPOUT_SITES}")
    if int(seq_k) > ATTN_DROPOUT_MAX_KEYS:
        raise ValueError(f"--attn-dropout: {seq_k} keys per sequence, at most 2^26")
    if int(batch) * int(heads) * int(seq_q) >= 1 << 32:
        raise ValueError(f"--attn-dropout: batch * heads * queries = {int(batch) * int(heads) * int(seq_q)} must stay "
                         "below 2^32")
    return p, seed


def _noise_arg(flag):
    def parse(text):
        import argparse
        from .dropout import threshold_and_scale
        try:
            v = float(text)
            if v != 0.0:
                threshold_and_scale(v)
        except ValueError:
            raise argparse.ArgumentTypeError(f"{flag} must be 0 or lie in (0, 0.9], got {text}")
        return v
    return parse


input_noise_arg = _noise_arg("--input-noise")
cond_noise_arg = _noise_arg("--cond-noise")


def add_token_noise_args(p):
    """--input-noise / --cond-noise / --noise-range of a Transformer training command line (additive, all 0 by
    default; they share --dropout-seed)."""
    p.add_argument("--input-noise", type=input_noise_arg, default=0.0,
                   help="(additive; the reference trains on clean tokens) probability P in (0, 0.9] with which each "
                        "teacher-forced HR token the decoder reads is replaced in training steps (0 = off: the plain "
                        "token-assembly launch, nothing else is launched or allocated); the targets stay clean.  "
                        "Models the sampling mistakes a stage meets in generation, where every token it reads was "
                        "drawn by the model.  The decision is a counter-based function of (--dropout-seed, rank, "
                        "optimizer step, sample, absolute token position), made inside the token-assembly kernel: "
                        "the same tokens with --graph-step, and --load-optim continues the sequence.  Sampling, "
                        "validation and generation never see it")
    p.add_argument("--cond-noise", type=cond_noise_arg, default=0.0,
                   help="(additive) the same for the LR tokens an encoder-decoder stage conditions on (in generation: "
                        "the previous stage's samples): one small launch per step.  Not with --train-base-model, "
                        "whose LR tokens are its start tokens and are drawn at random in generation")
    p.add_argument("--noise-range", type=_steps_arg("--noise-range", 0), default=0,
                   help="(additive) R >= 0: a replaced token is drawn from the codes within R of its own index -- the "
                        "codebooks are SOMs, neighbouring indices are similar codes -- clamped at the ends of the "
                        "axis; 0 (default) draws from the whole codebook.  The draw may return the token itself: the "
                        "effective change rate is P (1 - 1 / span)")


def check_token_noise_args(input_noise, cond_noise, noise_range, dropout_seed, train_base_model=False, k_lr=None,
                           k_hr=None):
    """(p_input, p_cond, range, seed) once more before anything is launched with them, or ValueError: either
    probability outside (0, 0.9], a negative range, --cond-noise for a base model, and a range that reaches across
    the smaller codebook (k_lr, k_hr: the vocabulary sizes, when known)."""
    from .dropout import TokenNoise
    seed = int(dropout_seed)
    if not 0 <= seed < 1 << 64:
        raise ValueError(f"--dropout-seed must be an integer in [0, 2^64), got {dropout_seed}")
    for flag, p in (("--input-noise", input_noise), ("--cond-noise", cond_noise)):
        try:
            TokenNoise.probabilities(p, 0.0)
        except ValueError:
            raise ValueError(f"{flag} must be 0 or lie in (0, 0.9], got {p}")
    if isinstance(noise_range, bool) or int(noise_range) != noise_range or noise_range < 0:
        raise ValueError(f"--noise-range must be an integer >= 0, got {noise_range}")
    p_input, p_cond, r = float(input_noise), float(cond_noise), int(noise_range)
    if p_cond > 0 and train_base_model:
        raise ValueError("--cond-noise does not go with --train-base-model: the base stage's LR tokens are its start "
                         "tokens, and its generation draws them at random")
    sizes = [int(k) for k in (k_lr, k_hr) if k is not None]
    if r > 0 and sizes and r >= min(sizes):
        raise ValueError(f"--noise-range {r} reaches across the smaller codebook ({min(sizes)} codes): use 0 to draw "
                         "from the whole codebook")
    return p_input, p_cond, r, seed


def weight_decay_arg(text):
    """argparse type of --weight-decay: 0 (off) or a float in (0, 1]."""
    import argparse
    try:
        v = float(text)
    except ValueError:
        v = float("nan")
    if not 0.0 <= v <= 1.0:
        raise argparse.ArgumentTypeError(f"--weight-decay must lie in [0, 1], got {text}")
    return v


def lr_min_ratio_arg(text):
    """argparse type of --lr-min-ratio: a float in [0, 1]."""
    import argparse
    try:
        v = float(text)
    except ValueError:
        v = float("nan")
    if not 0.0 <= v <= 1.0:
        raise argparse.ArgumentTypeError(f"--lr-min-ratio must lie in [0, 1], got {text}")
    return v


def _steps_arg(flag, least):
    def parse(text):
        import argparse
        try:
            v = int(text)
        except ValueError:
            v = least - 1
        if v < least:
            raise argparse.ArgumentTypeError(f"{flag} must be an integer >= {least}, got {text}")
        return v
    return parse


def add_optimizer_args(p):
    """--weight-decay and the --lr-* schedule flags of a Transformer training command line (all additive; at their
    defaults the loop is the reference's: plain Adam, the learning rate halved every --lr-step)."""
    p.add_argument("--weight-decay", type=weight_decay_arg, default=0.0,
                   help="(additive; the reference trains without) decoupled weight decay lambda in (0, 1], as "
                        "torch.optim.AdamW (0 = off, the plain Adam launch): every step shrinks the decayed "
                        "parameters by lr x lambda, at that step's learning rate, inside the optimiser's one launch.  "
                        "Decayed: the `weight` of every nn.Linear module.  Not decayed: every bias, every "
                        "nn.LayerNorm affine, every nn.Embedding table, every bare nn.Parameter.  A checkpoint's "
                        "own value is ignored on --load-optim: the command line governs")
    p.add_argument("--lr-schedule", choices=["step", "cosine"], default="step",
                   help="(additive) 'step' (default): the learning rate halves every --lr-step steps, the "
                        "reference's rule.  'cosine': base x (r + (1 - r)(1 + cos(pi u)) / 2) with u running from 0 "
                        "at the end of the warm-up to 1 at --lr-decay-steps, r = --lr-min-ratio; constant base x r "
                        "afterwards.  The schedule is a function of the optimizer's step count: a run resumed with "
                        "--load-optim continues it")
    p.add_argument("--lr-warmup-steps", type=_steps_arg("--lr-warmup-steps", 0), default=0,
                   help="(additive) linear warm-up, with either schedule: step t <= W runs at t / W of the "
                        "schedule's rate (default 0 = none).")
    p.add_argument("--lr-decay-steps", type=_steps_arg("--lr-decay-steps", 1), default=None,
                   help="(additive) the step at which --lr-schedule cosine reaches its floor (required with it, "
                        "not before the end of the warm-up).")
    p.add_argument("--lr-min-ratio", type=lr_min_ratio_arg, default=0.0,
                   help="(additive) floor of --lr-schedule cosine as a fraction of the base rate, in [0, 1] "
                        "(default 0).")


def check_optimizer_args(weight_decay, lr_schedule, lr_warmup_steps, lr_decay_steps, lr_min_ratio):
    """The five values once more before anything is launched with them (argparse has checked each on its own;
    what only holds between them -- cosine needs --lr-decay-steps, at or past the warm-up -- is checked here), or
    ValueError.  Returns them: (weight_decay, lr_schedule, lr_warmup_steps, lr_decay_steps, lr_min_ratio)."""
    wd, ratio = float(weight_decay), float(lr_min_ratio)
    if not 0.0 <= wd <= 1.0:                 # (NaN fails both comparisons)
        raise ValueError(f"--weight-decay must lie in [0, 1], got {weight_decay}")
    if lr_schedule not in ("step", "cosine"):
        raise ValueError(f"--lr-schedule must be 'step' or 'cosine', got {lr_schedule!r}")
    if int(lr_warmup_steps) != lr_warmup_steps or lr_warmup_steps < 0:
        raise ValueError(f"--lr-warmup-steps must be an integer >= 0, got {lr_warmup_steps}")
    if not 0.0 <= ratio <= 1.0:
        raise ValueError(f"--lr-min-ratio must lie in [0, 1], got {lr_min_ratio}")
    if lr_decay_steps is not None and (int(lr_decay_steps) != lr_decay_steps or lr_decay_steps < 1):
        raise ValueError(f"--lr-decay-steps must be an integer >= 1, got {lr_decay_steps}")
    if lr_schedule == "cosine":
        if lr_decay_steps is None:
            raise ValueError("--lr-schedule cosine needs --lr-decay-steps")
        if lr_decay_steps < lr_warmup_steps:
            raise ValueError(f"--lr-decay-steps ({lr_decay_steps}) lies before the end of --lr-warmup-steps "
                             f"({lr_warmup_steps})")
    return wd, lr_schedule, int(lr_warmup_steps), None if lr_decay_steps is None else int(lr_decay_steps), ratio


def optimizer_args_are_default(weight_decay, lr_schedule, lr_warmup_steps, lr_decay_steps, lr_min_ratio):
    """True when the training loop is the reference's: no decay, the halving rule, no warm-up."""
    return weight_decay == 0 and lr_schedule == "step" and lr_warmup_steps == 0 and lr_decay_steps is None \
        and lr_min_ratio == 0


def clip_grad_norm_arg(text):
    """argparse type of --clip-grad-norm: a float > 0, or inf (the non-finite guard alone)."""
    import argparse
    try:
        v = float(text)
    except ValueError:
        v = float("nan")
    if not v > 0.0:
        raise argparse.ArgumentTypeError(f"--clip-grad-norm must be > 0 (or inf), got {text}")
    return v


def add_grad_clip_args(p):
    """--clip-grad-norm and --max-skipped-steps of a Transformer training command line (additive; without the first
    the loop is the reference's)."""
    p.add_argument("--clip-grad-norm", type=clip_grad_norm_arg, default=None,
                   help="(additive; the reference trains without) clip the global L2 norm of all gradients to C > 0 "
                        "before the optimiser step, torch.nn.utils.clip_grad_norm_'s rule, measured and applied on "
                        "the device; `inf` clips nothing.  With the flag a step whose gradients are not all finite "
                        "is skipped on the device (parameters, moments and EMA keep their bits) instead of ending "
                        "the run, and the log line carries Grad Norm | Clipped | Skipped")
    p.add_argument("--max-skipped-steps", type=_steps_arg("--max-skipped-steps", 0), default=10,
                   help="(additive; with --clip-grad-norm) end the run once more than this many consecutive steps "
                        "were skipped (default 10).")


def check_grad_clip_args(clip_grad_norm, max_skipped_steps):
    """The two values once more before anything is launched with them, or ValueError.  Returns them:
    (clip_grad_norm or None, max_skipped_steps)."""
    if clip_grad_norm is not None and not float(clip_grad_norm) > 0.0:       # (NaN fails the comparison)
        raise ValueError(f"--clip-grad-norm must be > 0 (or inf), got {clip_grad_norm}")
    if isinstance(max_skipped_steps, bool) or int(max_skipped_steps) != max_skipped_steps or max_skipped_steps < 0:
        raise ValueError(f"--max-skipped-steps must be an integer >= 0, got {max_skipped_steps}")
    return None if clip_grad_norm is None else float(clip_grad_norm), int(max_skipped_steps)


def check_prompt_args(prompt_fmaps, prompt_fraction):
    """generate_images.py --prompt-fmaps / --prompt-fraction: both or neither, the fraction inside (0, 1).
    Returns whether the run is prompted."""
    if prompt_fmaps is None and prompt_fraction is None:
        return False
    if prompt_fmaps is None or prompt_fraction is None:
        raise SystemExit("--prompt-fmaps and --prompt-fraction go together")
    if not 0.0 < float(prompt_fraction) < 1.0:       # NaN fails both comparisons
        raise SystemExit(f"--prompt-fraction must be inside (0, 1), got {prompt_fraction!r}")
    return True


def prompt_tokens(fraction, image_dim, patch_dim, beam_width, sliding_window=None):
    """Tokens of a stage's own token grid that a prompted run keeps: the top floor(fraction x patch_rows) rows.
    The generation loop appends whole chunks, so a kept count that is no multiple of `beam_width` is refused
    like a beam_width that does not divide the sequence; sliding_window (a stage that slides): the start token
    and the kept tokens must leave the window room (a prefix at or past the window is out of scope)."""
    rows, cols = image_dim[0] // patch_dim[0], image_dim[1] // patch_dim[1]
    kept = int(float(fraction) * rows + 1e-9) * cols      # (0.29 x 100 is 28.999...6 in binary: still 29 rows)
    if kept % beam_width != 0:
        raise Exception("Invalid value for beam_width!")
    if sliding_window is not None and 1 + kept >= sliding_window:
        raise Exception(f"Invalid value for prompt-fraction: {kept} prompt tokens reach the sliding window "
                        f"({sliding_window})!")
    return kept


def load_prompt_latents(path, lo, hi, device):
    """Latents lo .. hi-1 of a feature-map dataset index (generate_fmap_dataset.py's output) as one batch."""
    from dataset_loader.feature_map_dataset import FeatureMapDataset
    data = FeatureMapDataset(dataset_path=path)
    if len(data) < hi:
        raise Exception(f"--prompt-fmaps holds {len(data)} latents, {hi} images asked for!")
    if hi <= lo:
        return None
    return torch.stack([data[i] for i in range(lo, hi)]).to(device)


def halve_lr(optim):
    for g in optim.param_groups:
        g["lr"] = g["lr"] * 0.5
