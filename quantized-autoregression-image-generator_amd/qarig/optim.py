"""Adam over ONE flat fp32 buffer.

All parameters are re-pointed (as views) into a single allocation, and so are their
gradients and both moments: the optimiser step is one kernel launch, zero_grad is one
memset, and the flat gradient buffer is exactly what the data-parallel all-reduce
moves over RCCL (qarig.parallel).  Semantics and state_dict layout follow
torch.optim.Adam as the reference uses it (betas=(0.5, 0.999), eps 1e-8, no weight
decay; train_quantized_transformer.py:317-334), so "model_optimizer" entries of
reference checkpoints load and save unchanged.

Additive: enable_weight_decay (AdamW: decoupled decay of selected parameters from the same launch, through a
mask of one byte per 8 elements), LRSchedule (linear warm-up; the reference's halving rule or a cosine decay) and
enable_grad_clip (global-norm gradient clipping and a guard that skips a step with non-finite gradients, both decided
on the device: two launches in the place of the one).
"""
import contextlib
import math
import struct

import torch
import torch.distributed as dist

from . import ops

# Gradient buckets for the overlapped data-parallel all-reduce: 16 Mi floats = 64 MiB keeps
# each xGMI link busy with few, large messages (ring collectives are per-link bound).
BUCKET_ELEMS = 16 * 1024 * 1024


def ema_weight(count, decay, warmup=True):
    """Weight of the new parameters in EMA update number `count` (0-based): 1 - decay, or with warm-up
    1 - min(decay, (1 + count) / (10 + count)), so that an average started from the initial weights forgets
    them within tens of steps instead of 1 / (1 - decay).  Computed in double, rounded to fp32 once (the
    value the kernel receives)."""
    d = float(decay)
    if warmup:
        d = min(d, (1.0 + count) / (10.0 + count))
    return struct.unpack("f", struct.pack("f", 1.0 - d))[0]


def fp32(x):
    """The double `x` rounded to fp32 once (the value a kernel receives for it)."""
    return struct.unpack("f", struct.pack("f", float(x)))[0]


def decay_group_mask(sizes, offsets, total, decayed):
    """The decay mask of qarig_adamw_step for a flat buffer of `total` floats whose parameter k occupies
    [offsets[k], offsets[k] + sizes[k]): a uint8 CPU tensor with one entry per group of 8 elements, 1 on the groups
    of the parameters flagged in `decayed`, 0 elsewhere (the padding groups between slices included).  Slices
    start on multiples of 8, so no group belongs to two parameters; anything else is refused."""
    sizes, offsets, decayed = list(sizes), list(offsets), list(decayed)
    if not (len(sizes) == len(offsets) == len(decayed)):
        raise ValueError("decay_group_mask: sizes, offsets and decayed must have one entry per parameter")
    if total < 0 or total % 8:
        raise ValueError(f"decay_group_mask: total must be a non-negative multiple of 8, got {total}")
    mask = torch.zeros(total // 8, dtype=torch.uint8)
    for s, o, d in zip(sizes, offsets, decayed):
        if o % 8:
            raise ValueError(f"decay_group_mask: offset {o} is not a multiple of 8")
        if s < 0 or o < 0 or o + s > total:
            raise ValueError(f"decay_group_mask: slice [{o}, {o + s}) outside a buffer of {total}")
        if d:
            mask[o // 8:(o + s + 7) // 8] = 1
    return mask


def decay_parameters(model):
    """The parameters --weight-decay decays: the `weight` of every nn.Linear module of `model`, and nothing else
    (no bias, no nn.LayerNorm affine, no nn.Embedding table, no bare nn.Parameter)."""
    out, seen = [], set()
    for mod in model.modules():
        if isinstance(mod, torch.nn.Linear) and id(mod.weight) not in seen:
            seen.add(id(mod.weight))
            out.append(mod.weight)
    return out


class LRSchedule:
    """Learning rate of the 1-based optimizer step t, a pure function computed in double.

    warm(t) = min(1, t / warmup_steps), or 1 when warmup_steps == 0.
    kind "step":   base * warm(t) * 0.5 ** h(t), h(1) = 0 and h(t) = floor((t - 2) / lr_step): the halvings the
                   training loop's `--lr-step` rule has applied before step t.
    kind "cosine": u = clamp((t - 1 - warmup_steps) / max(1, decay_steps - warmup_steps), 0, 1) and
                   base * warm(t) * (min_ratio + (1 - min_ratio) * (1 + cos(pi u)) / 2)."""

    def __init__(self, base_lr, kind="step", lr_step=None, warmup_steps=0, decay_steps=None, min_ratio=0.0):
        base_lr = float(base_lr)
        if not (0.0 < base_lr < float("inf")):
            raise ValueError(f"LRSchedule: base_lr must be finite and positive, got {base_lr}")
        if kind not in ("step", "cosine"):
            raise ValueError(f"LRSchedule: kind must be 'step' or 'cosine', got {kind!r}")
        if int(warmup_steps) != warmup_steps or warmup_steps < 0:
            raise ValueError(f"LRSchedule: warmup_steps must be an integer >= 0, got {warmup_steps}")
        min_ratio = float(min_ratio)
        if not (0.0 <= min_ratio <= 1.0):
            raise ValueError(f"LRSchedule: min_ratio must lie in [0, 1], got {min_ratio}")
        if kind == "step":
            if lr_step is None or int(lr_step) != lr_step or lr_step < 1:
                raise ValueError(f"LRSchedule: kind 'step' needs an integer lr_step >= 1, got {lr_step}")
        else:
            if decay_steps is None or int(decay_steps) != decay_steps or decay_steps < 1:
                raise ValueError(f"LRSchedule: kind 'cosine' needs an integer decay_steps >= 1, got {decay_steps}")
            if decay_steps < warmup_steps:
                raise ValueError(f"LRSchedule: decay_steps ({decay_steps}) ends before the warm-up "
                                 f"({warmup_steps})")
        self.base_lr, self.kind, self.min_ratio = base_lr, kind, min_ratio
        self.lr_step = None if lr_step is None else int(lr_step)
        self.warmup_steps = int(warmup_steps)
        self.decay_steps = None if decay_steps is None else int(decay_steps)

    def lr(self, t):
        if int(t) != t or t < 1:
            raise ValueError(f"LRSchedule.lr: the optimizer step is 1-based, got {t}")
        t = int(t)
        warm = min(1.0, t / self.warmup_steps) if self.warmup_steps else 1.0
        if self.kind == "step":
            h = 0 if t == 1 else (t - 2) // self.lr_step
            return self.base_lr * warm * 0.5 ** h
        u = (t - 1 - self.warmup_steps) / max(1, self.decay_steps - self.warmup_steps)
        u = min(1.0, max(0.0, u))
        return self.base_lr * warm * (self.min_ratio + (1.0 - self.min_ratio) * 0.5 * (1.0 + math.cos(math.pi * u)))


class FlatAdam:
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
        self.params = [p for p in params]
        if not self.params:
            raise ValueError("optimizer got an empty parameter list")
        dev = self.params[0].device
        if dev.type != "cuda":
            raise RuntimeError("FlatAdam needs the parameters on the GPU (call model.to(device) first)")
        self.defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=0, amsgrad=False)
        self.param_groups = [dict(self.defaults, params=list(range(len(self.params))))]
        sizes = [p.numel() for p in self.params]
        # 32-B aligned slices: every fp32 view can be read with float4 loads, and the same offsets are 16-B
        # aligned in the bf16 image of the buffer (flat_shadow: LDS-DMA rows of the reduced-precision GEMMs)
        offs, total = [], 0
        for s in sizes:
            offs.append(total)
            total += (s + 7) // 8 * 8
        self.offsets, self.total = offs, total
        self.flat_param = torch.zeros(total, dtype=torch.float32, device=dev)
        self.flat_grad = torch.zeros(total, dtype=torch.float32, device=dev)
        self.exp_avg = torch.zeros(total, dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros(total, dtype=torch.float32, device=dev)
        self.step_count = 0
        self._overlap = False
        self._works = []
        self._capture_cut = None    # set by pipeline._SegmentedCapture while it records a step
        self.flat_ema = None        # enable_ema
        self._ema_swapped = False   # inside ema_weights()
        self.decay_mask = None      # enable_weight_decay
        self.clip_max_norm = None   # enable_grad_clip
        with torch.no_grad():
            for p, o, s in zip(self.params, offs, sizes):
                view = self.flat_param[o:o + s].view(p.shape)
                view.copy_(p.data)
                p.data = view
                p.grad = self.flat_grad[o:o + s].view(p.shape)
                p._qarig_owner = self      # caches of derived data (ops.bmu_image) follow step_count

    # -- data-parallel overlap ----------------------------------------------------------
    def enable_allreduce_overlap(self, force=False):
        """Launch the RCCL sum all-reduce of each gradient bucket as soon as the backward
        pass has written every gradient in it (buckets are contiguous runs of the flat
        buffer in parameter order, i.e. whole layers; backward completes them last layer
        first), so the exchange overlaps the rest of backward.  Completion is tracked
        exactly: the fused weight/bias-gradient kernels report each parameter they finish
        (qarig.functional), every other parameter through a post-accumulate-grad hook.
        Assumes each parameter receives its gradient once per step (true for the models
        of this repository)."""
        if self._overlap or not (dist.is_available() and dist.is_initialized()) \
                or (dist.get_world_size() == 1 and not force):
            return
        self._overlap = True
        self._bucket_of, self._bucket_range, self._pending0 = {}, [], []
        lo, count, start_i = 0, 0, 0
        for i, (p, o) in enumerate(zip(self.params, self.offsets)):
            end = o + (p.numel() + 3) // 4 * 4
            self._bucket_of[id(p)] = len(self._bucket_range)
            count += 1
            last = i == len(self.params) - 1
            if end - lo >= BUCKET_ELEMS or last:
                self._bucket_range.append((lo, end))
                self._pending0.append(count)
                lo, count = end, 0
        self._pending = list(self._pending0)
        self._done = set()
        self._launched = 0
        for p in self.params:
            p._qarig_grad_done = self._grad_done
            p.register_post_accumulate_grad_hook(self._grad_done)

    def _grad_done(self, p):
        # idempotent per step: a parameter may be reported both by the fused gradient
        # kernel path and by autograd's post-accumulate hook
        if id(p) in self._done:
            return
        if self._capture_cut is not None:
            self._capture_cut(None, len(self.params) - len(self._done))
        self._done.add(id(p))
        b = self._bucket_of[id(p)]
        self._pending[b] -= 1
        if self._pending[b] == 0:
            if self._capture_cut is not None:
                # a step is being recorded into graph segments: the bucket's all-reduce is not part
                # of the recording, the segment ends here and replay issues the collective behind it
                self._capture_cut(b, 0)
            else:
                self.launch_bucket(b)

    def launch_bucket(self, b):
        lo, hi = self._bucket_range[b]
        self._works.append(dist.all_reduce(self.flat_grad[lo:hi], op=dist.ReduceOp.SUM, async_op=True))
        self._launched += 1

    def reset_overlap_bookkeeping(self):
        """After a recording pass (no collective was issued, every parameter reported)."""
        self._pending = list(self._pending0)
        self._done = set()
        self._launched = 0

    def finish_allreduce(self):
        """Waits for the overlapped bucket all-reduces (no-op without overlap).  Returns
        True if this step's gradients have been reduced by the overlapped path."""
        if not self._overlap:
            return False
        # a replayed step (pipeline._SegmentedCapture) runs no hooks: its buckets were launched by
        # the replay loop, one per recorded cut
        replayed = not self._done and self._launched == len(self._bucket_range)
        if not replayed and any(n != 0 for n in self._pending):
            raise RuntimeError("overlapped all-reduce: some parameters never reported a gradient "
                               f"(pending per bucket: {self._pending})")
        if self._launched != len(self._bucket_range):
            raise RuntimeError(f"overlapped all-reduce: {self._launched} of {len(self._bucket_range)} "
                               "gradient buckets were exchanged")
        for w in self._works:
            w.wait()
        self._works = []
        self.reset_overlap_bookkeeping()
        return True

    # -- torch.optim API subset the reference's training loops use ------------------
    def zero_grad(self, set_to_none=False):
        self.flat_grad.zero_()
        for p, o in zip(self.params, self.offsets):
            if p.grad is None or p.grad.data_ptr() != self.flat_grad.data_ptr() + 4 * o:
                p.grad = self.flat_grad[o:o + p.numel()].view(p.shape)

    @torch.no_grad()
    def _step_scalars(self, step):
        g = self.param_groups[0]
        b1, b2 = g["betas"]
        return g["lr"] / (1 - b1 ** step), math.sqrt(1 - b2 ** step)

    # -- reduced precision: the bf16 copies of the weights come out of the Adam pass --------------------
    def _shadow_buffer(self):
        """Flat bf16 image of flat_param, written by the Adam kernel of every step while a reduced-precision
        mode is on (173 per-weight cast launches per step of the config-5 model otherwise)."""
        if not ops.lp_mode():
            return None
        if getattr(self, "flat_shadow", None) is None:
            self.flat_shadow = torch.empty(self.total, dtype=torch.bfloat16, device=self.flat_param.device)
            self._shadow_views = {}
            if self.clip_max_norm is not None:
                # a skipped step leaves the image as it is: it must hold the parameters before the first step
                self.flat_shadow.copy_(self.flat_param)
        return self.flat_shadow

    def _shadow_written(self):
        # the kernel writes through raw pointers: torch's version counters stay where they are, so a later
        # in-place change of a parameter by anyone else (load_state_dict, a test) shows as a version mismatch
        self._shadow_versions = [p._version for p in self.params]

    def shadow_of(self, p):
        """bf16 view of parameter p out of the last Adam pass, or None (no pass yet in this mode, or p was
        modified since)."""
        if getattr(self, "_shadow_versions", None) is None or not ops.lp_mode():
            return None
        i = self._index.get(id(p)) if hasattr(self, "_index") else None
        if i is None:
            self._index = {id(q): k for k, q in enumerate(self.params)}
            i = self._index.get(id(p))
        if i is None or self._shadow_versions[i] != p._version:
            return None
        v = self._shadow_views.get(i)
        if v is None:
            o = self.offsets[i]
            v = self._shadow_views[i] = self.flat_shadow[o:o + p.numel()].view(p.shape)
        return v

    def _adam(self, b1, b2, eps, step_size, bc2_sqrt, ema_w, grad_scale, dev_step, shadow):
        if self.clip_max_norm is not None:
            # the norm of the gradients as they stand now (behind any all-reduce: identical bits on every rank),
            # then the step that reads its verdict from the device
            ops.grad_clip_coef(self.flat_grad, grad_scale, self.clip_max_norm, self._clip_partials, self.clip_state)
            decay = 0.0 if dev_step is not None or self.decay_mask is None else self._decay()
            ops.adam_clip_step(self.flat_param, self.flat_grad, self.exp_avg, self.exp_avg_sq, self.flat_ema,
                               self.decay_mask, b1, b2, eps, step_size, bc2_sqrt, ema_w, decay, self.clip_state,
                               grad_scale, dev_step=dev_step, shadow=shadow)
        elif self.decay_mask is not None:
            ops.adamw_step(self.flat_param, self.flat_grad, self.exp_avg, self.exp_avg_sq, self.flat_ema,
                           self.decay_mask, b1, b2, eps, step_size, bc2_sqrt, ema_w,
                           0.0 if dev_step is not None else self._decay(), grad_scale, dev_step=dev_step,
                           shadow=shadow)
        elif self.flat_ema is None:
            ops.adam_step(self.flat_param, self.flat_grad, self.exp_avg, self.exp_avg_sq, b1, b2,
                          eps, step_size, bc2_sqrt, grad_scale, dev_step=dev_step, shadow=shadow)
        else:
            ops.adam_ema_step(self.flat_param, self.flat_grad, self.exp_avg, self.exp_avg_sq, self.flat_ema,
                              b1, b2, eps, step_size, bc2_sqrt, ema_w, grad_scale, dev_step=dev_step,
                              shadow=shadow)

    def _refuse_swapped(self):
        if self._ema_swapped:
            raise RuntimeError("FlatAdam: no optimizer step inside ema_weights() (the parameters hold the EMA)")

    def step(self, grad_scale=1.0):
        self._refuse_swapped()
        self.step_count += 1
        g = self.param_groups[0]
        b1, b2 = g["betas"]
        step_size, bc2_sqrt = self._step_scalars(self.step_count)
        shadow = self._shadow_buffer()
        ema_w = 0.0
        if self.flat_ema is not None:
            ema_w = ema_weight(self.ema_count, self.ema_decay, self.ema_warmup)
            self.ema_count += 1
        self._adam(b1, b2, g["eps"], step_size, bc2_sqrt, ema_w, grad_scale, None, shadow)
        ops.lp_invalidate()      # cached bf16 / e4m3 copies made from the old weights are stale now
        if shadow is not None:
            self._shadow_written()
        else:
            self._shadow_versions = None     # (a step outside the mode leaves the bf16 image behind)

    # -- graph replay (qarig.pipeline.GraphedTrainStep) -----------------------------------
    def _dev_step_buffer(self):
        if not hasattr(self, "_dev_step"):
            # {step_size, bc2_sqrt} and, with the EMA on, its weight; with weight decay or the gradient clip always
            # four, {step_size, bc2_sqrt, ema_w, decay}
            four = self.decay_mask is not None or self.clip_max_norm is not None
            size = 4 if four else 2 if self.flat_ema is None else 3
            self._dev_step = torch.zeros(size, dtype=torch.float32, device=self.flat_param.device)
        return self._dev_step

    def step_captured(self, grad_scale=1.0):
        """The Adam launch as it is recorded into a captured training-step graph: step size and
        bias correction are read from a device buffer that `advance_captured` refreshes on the
        host before every replay (learning-rate changes included)."""
        self._refuse_swapped()
        g = self.param_groups[0]
        b1, b2 = g["betas"]
        shadow = self._shadow_buffer()
        self._adam(b1, b2, g["eps"], 0.0, 1.0, 0.0, grad_scale, self._dev_step_buffer(), shadow)
        ops.lp_invalidate()
        if shadow is not None:
            self._shadow_written()
        else:
            self._shadow_versions = None

    def advance_captured(self):
        """Called before every replay of a captured step: the replayed Adam kernel rewrites the
        parameters without touching torch's version counters, so the reduced-precision weight
        shadows an eager forward may have cached (per-checkpoint sampling between replays) are stale
        from here on."""
        self._refuse_swapped()
        self.step_count += 1
        scalars = list(self._step_scalars(self.step_count))
        if self.flat_ema is not None:
            scalars.append(ema_weight(self.ema_count, self.ema_decay, self.ema_warmup))
            self.ema_count += 1
        if self.decay_mask is not None or self.clip_max_norm is not None:
            if len(scalars) == 2:
                scalars.append(0.0)         # (the EMA weight's slot: ignored without an EMA)
            scalars.append(self._decay() if self.decay_mask is not None else 0.0)
        if not hasattr(self, "_dev_step_feed"):
            from .pipeline import PinnedFeed
            self._dev_step_feed = PinnedFeed(self._dev_step_buffer())
        self._dev_step_feed.push(torch.tensor(scalars, dtype=torch.float32))
        ops.lp_invalidate()

    # -- decoupled weight decay (AdamW; additive: the reference trains without) --------------------------
    def _decay(self):
        """lr * weight_decay of this step, in double, rounded to fp32 once."""
        g = self.param_groups[0]
        return fp32(float(g["lr"]) * float(g["weight_decay"]))

    def enable_weight_decay(self, weight_decay, params):
        """Decoupled weight decay from here on: every step first shrinks the parameters listed in `params` by
        lr * weight_decay (p <- fma(-lr * weight_decay, p, p), the learning rate of that step), then applies
        Adam's update to the result -- torch.optim.AdamW with two groups, from one launch (qarig_adamw_step).
        The mask has one byte per 8 elements of the flat buffer.  Must be called before a step is captured: the
        captured launch reads four scalars from a device buffer that has to exist, at its final size, before the
        capture."""
        wd = float(weight_decay)
        if not (0.0 < wd <= 1.0):            # (NaN fails both comparisons)
            raise ValueError(f"weight decay must be finite and lie in (0, 1], got {weight_decay}")
        params = list(params)
        index = {id(p): i for i, p in enumerate(self.params)}
        for p in params:
            if id(p) not in index:
                raise ValueError("FlatAdam.enable_weight_decay: a parameter this optimizer does not own")
        if hasattr(self, "_dev_step"):
            raise RuntimeError("FlatAdam.enable_weight_decay: a captured step was already recorded (its launch "
                               "reads a scalar buffer without the decay and has no mask); enable weight decay "
                               "before the first captured step")
        if self._ema_swapped:
            raise RuntimeError("FlatAdam.enable_weight_decay inside ema_weights()")
        flags = [False] * len(self.params)
        for p in params:
            flags[index[id(p)]] = True
        mask = decay_group_mask([p.numel() for p in self.params], self.offsets, self.total, flags)
        self.decay_mask = mask.to(self.flat_param.device)
        self.param_groups[0]["weight_decay"] = wd

    # -- global-norm gradient clipping and the non-finite guard (additive: the reference trains without) ---------
    def enable_grad_clip(self, max_norm):
        """From here on every step first measures the global norm of the scaled gradients (qarig_grad_clip_coef:
        fp64, one fixed summation order) and then runs qarig_adam_clip_step in the place of the plain launch: the
        gradients enter Adam times coef = min(1, max_norm / (norm + 1e-6)), torch.nn.utils.clip_grad_norm_'s rule,
        and a step whose norm is not finite changes nothing on the device.  max_norm = inf keeps the guard alone.
        Norm, coefficient and both counts stay on the device (clip_state; clip_stats() reads them back).  A skipped
        step still advances step_count, the EMA's update count and whatever else the host counts: the host does
        not learn of the skip.  Must be called before a step is captured: the captured launches are different
        ones and read a four-float scalar buffer."""
        c = float(max_norm)
        if not c > 0.0:                          # (NaN fails the comparison)
            raise ValueError(f"gradient clipping: max_norm must be > 0 (inf: guard only), got {max_norm}")
        if hasattr(self, "_dev_step"):
            raise RuntimeError("FlatAdam.enable_grad_clip: a captured step was already recorded (its launch has "
                               "no clip and reads a scalar buffer of another size); enable the clip before the "
                               "first captured step")
        if self._ema_swapped:
            raise RuntimeError("FlatAdam.enable_grad_clip inside ema_weights()")
        dev = self.flat_param.device
        if self.clip_max_norm is None:
            self.clip_state = torch.zeros(4, dtype=torch.float64, device=dev)
            self._clip_partials = torch.zeros(ops.GRAD_NORM_PARTIALS, dtype=torch.float64, device=dev)
            if getattr(self, "flat_shadow", None) is not None:
                self.flat_shadow.copy_(self.flat_param)
        self.clip_max_norm = c

    def clip_stats(self):
        """One read-back of clip_state: the last step's norm and coefficient, and how many steps were skipped
        (non-finite norm) and clipped (coef < 1) so far."""
        if self.clip_max_norm is None:
            raise RuntimeError("FlatAdam: no gradient clip (call enable_grad_clip first)")
        norm, coef, skipped, clipped = self.clip_state.tolist()
        return {"norm": norm, "coef": coef, "skipped": int(skipped), "clipped": int(clipped)}

    # -- exponential moving average of the parameters (additive: the reference keeps none) ----------------
    def enable_ema(self, decay, warmup=True):
        """Keeps flat_ema, an EMA of flat_param, from here on: the Adam launch of every step moves it by
        ema_weight(ema_count, decay, warmup) towards the parameters it has just computed.  Starts as a copy of
        the present parameters.  Must be called before a step is captured: the captured launch reads its three
        scalars from a device buffer that has to exist, at its final size, before the capture."""
        if not (0.0 < float(decay) < 1.0):       # (NaN fails both comparisons)
            raise ValueError(f"EMA decay must lie in (0, 1), got {decay}")
        if hasattr(self, "_dev_step"):
            raise RuntimeError("FlatAdam.enable_ema: a captured step was already recorded (its launch reads a "
                               "two-float scalar buffer and has no EMA); enable the EMA before the first "
                               "captured step")
        if self._ema_swapped:
            raise RuntimeError("FlatAdam.enable_ema inside ema_weights()")
        self.ema_decay, self.ema_warmup = float(decay), bool(warmup)
        self.flat_ema = self.flat_param.clone()
        self.ema_count = 0

    def _need_ema(self):
        if self.flat_ema is None:
            raise RuntimeError("FlatAdam: no EMA (call enable_ema first)")

    def ema_views(self):
        """Per-parameter views of flat_ema, in parameter order."""
        self._need_ema()
        return [self.flat_ema[o:o + p.numel()].view(p.shape) for p, o in zip(self.params, self.offsets)]

    def _ema_index(self, model):
        index = {id(p): i for i, p in enumerate(self.params)}
        return [(name, index[id(p)]) for name, p in model.named_parameters(remove_duplicate=False)
                if id(p) in index]

    def ema_meta(self):
        """Plain numbers and a bool (loads under the weights-only unpickler)."""
        self._need_ema()
        return {"decay": self.ema_decay, "count": int(self.ema_count), "warmup": self.ema_warmup}

    @torch.no_grad()
    def ema_state_dict(self, model):
        """model.state_dict() with every parameter this optimizer owns replaced by a clone of its EMA; buffers
        (and parameters it does not own) as the model holds them."""
        self._need_ema()
        if self._ema_swapped:
            raise RuntimeError("FlatAdam.ema_state_dict inside ema_weights()")
        sd = model.state_dict()
        views = self.ema_views()
        for name, i in self._ema_index(model):
            if name in sd:
                sd[name] = views[i].clone()
        return sd

    @torch.no_grad()
    def load_ema(self, state_dict_like, model, count):
        """Resume: the EMA from the entries of `state_dict_like` (keys as model.state_dict()), its update
        count from `count`."""
        self._need_ema()
        if self._ema_swapped:
            raise RuntimeError("FlatAdam.load_ema inside ema_weights()")
        views = self.ema_views()
        for name, i in self._ema_index(model):
            if name not in state_dict_like:
                raise KeyError(f"EMA state has no entry {name!r}")
            views[i].copy_(state_dict_like[name].reshape(views[i].shape))
        self.ema_count = int(count)

    def _exchange_with_ema(self):
        ops.swap_(self.flat_param, self.flat_ema)
        # the swap writes the flat buffer behind torch's version counters and the step count: every copy derived
        # from the old contents is declared stale here
        ops.lp_invalidate()
        ops.bmu_invalidate()
        self._shadow_versions = None
        from . import sampling
        sampling.decode_cache_clear()

    @contextlib.contextmanager
    def ema_weights(self):
        """Inside the context the model's parameters hold the EMA (sampling, evaluation); on exit they hold the
        raw weights again, bit for bit.  Contents are exchanged, never pointers: a captured step holds the
        addresses.  Not re-entrant; no optimizer step inside."""
        self._need_ema()
        if self._ema_swapped:
            raise RuntimeError("FlatAdam.ema_weights is not re-entrant")
        if self._works or (self._overlap and (self._done or self._launched)):
            raise RuntimeError("FlatAdam.ema_weights: an overlapped gradient all-reduce is pending")
        self._exchange_with_ema()
        self._ema_swapped = True
        try:
            yield self
        finally:
            self._exchange_with_ema()
            self._ema_swapped = False

    def state_dict(self):
        state = {}
        if self.step_count > 0:
            for i, (p, o) in enumerate(zip(self.params, self.offsets)):
                n = p.numel()
                state[i] = {"step": torch.tensor(float(self.step_count)),
                            "exp_avg": self.exp_avg[o:o + n].view(p.shape).clone(),
                            "exp_avg_sq": self.exp_avg_sq[o:o + n].view(p.shape).clone()}
        groups = [{k: v for k, v in g.items()} for g in self.param_groups]
        return {"state": state, "param_groups": groups}

    @torch.no_grad()
    def load_state_dict(self, sd):
        for k in ("lr", "betas", "eps"):
            if k in sd["param_groups"][0]:
                self.param_groups[0][k] = sd["param_groups"][0][k]
        for i, st in sd["state"].items():
            i = int(i)
            o, n = self.offsets[i], self.params[i].numel()
            self.exp_avg[o:o + n].copy_(st["exp_avg"].reshape(-1))
            self.exp_avg_sq[o:o + n].copy_(st["exp_avg_sq"].reshape(-1))
            self.step_count = int(float(st["step"]))
        ops.lp_invalidate()
