"""Adam over ONE flat fp32 buffer.

All parameters are re-pointed (as views) into a single allocation, and so are their
gradients and both moments: the optimiser step is one kernel launch, zero_grad is one
memset, and the flat gradient buffer is exactly what the data-parallel all-reduce
moves over RCCL (qarig.parallel).  Semantics and state_dict layout follow
torch.optim.Adam as the reference uses it (betas=(0.5, 0.999), eps 1e-8, no weight
decay; train_quantized_transformer.py:317-334), so "model_optimizer" entries of
reference checkpoints load and save unchanged.
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
        if self.flat_ema is None:
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
            # {step_size, bc2_sqrt} and, with the EMA on, its weight
            self._dev_step = torch.zeros(2 if self.flat_ema is None else 3, dtype=torch.float32,
                                         device=self.flat_param.device)
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
        if not hasattr(self, "_dev_step_feed"):
            from .pipeline import PinnedFeed
            self._dev_step_feed = PinnedFeed(self._dev_step_buffer())
        self._dev_step_feed.push(torch.tensor(scalars, dtype=torch.float32))
        ops.lp_invalidate()

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
