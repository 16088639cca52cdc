"""Key/value cache for autoregressive decoding, and the device-resident sampling loop on top of it.

The reference samples every token by re-running the decoder over the whole window
(generate_images.py:283-307; train_quantized_transformer.py:600-640).  While the window has
not started to slide, the keys and values of tokens already in it never change: the
self-attention is causal, the sequence position of a token is its index in the window and
its `pos_cond` value is fixed when it is appended.  `DecodeCache.step` therefore evaluates
ONLY the new token: per decoder layer it runs the q/k/v MLPs on one row per sequence,
appends k/v to the cache and attends with `qarig_decode_attention`; cross-attention keys and
values of the (constant) encoder output are computed once.  The logits equal the last row
of `Transformer.decode` on the full window up to fp32 summation order.

The step is ~80 dependent launches whose time is memory LATENCY, not bytes (csrc/decode.hip), so:
  * every Linear runs on `decode_linear_kernel` (all loads issued before the first wait) with the
    LayerNorm in front of it, the residual layer's skip-add / activation and gate inside the launch;
  * `cond` depends on a token's position alone and the positions of a stage are known before its loop:
    with `positions` given the cache evaluates `pos_cond_layer` and EVERY ScaleLayer / ShiftLayer projection
    (models/layers.py:100-153, 258-304: 63 Linear layers, 66 MB of weights at README size) once per window
    position at construction; a step's first launch copies the current position's row;
  * the step is captured into a HIP graph; what changes between tokens (ids, cache length) lives in device
    buffers -- `ctl` (int32 control words, csrc/decode.hip DecCtl) -- that the kernels read.

`DecodeCache.begin_search / run_chunk / finish_search` keep the whole best-of-`num_beam` chunk search of
generate_images.py:256-345 on the device: sampling (`qarig_decode_sample`) and candidate bookkeeping
(`qarig_decode_decide` / `_rows` / `_commit` / `_advance`) are single launches between replays of the step's
graph, all reading and writing device state; the host enqueues them without reading anything back until the
stage is finished.

The cache stops being valid when the window slides (every token's window index shifts);
`sampling.generate_tokens` falls back to the full-window evaluation from there on.  `WindowStep` keeps that
evaluation on the device too (opt-in, `generate_tokens(window_graph=True)`): it cannot reuse keys and values
either -- a slide changes the window-relative positional embedding of every token -- but everything around the
recomputation is built once per stage and the evaluation itself is one graph replay.
"""
import os
from types import SimpleNamespace

import torch

from models.layers import _lin_params, _mlp2_forward, _norm_forward
from . import functional as QF
from . import functional_lp as QL
from . import ops

# LayerNorm (affine or AdaLN form) inside the launch of the Linear that reads it, the feed-forward
# gate multiply inside the launch of the Linear that produces its operand: 15 -> 11 dependent launches
# per encoder-decoder layer and token.  False: the separate launches (the tests compare both).
FUSE_NORMS = True

_WARM_SHAPES = set()        # step shapes that have run eagerly once in this process (begin_search)

# Weight-only bf16 for the <= 16-row Linear layers of a step (`weights="bf16"`): each weight is streamed as its bf16
# image (rounded once, to nearest even: ops.cast_bf16) by qarig_decode_linear_bf16w, half the bytes per token.
# Activations, accumulation, LayerNorm, attention, the key/value cache, the conditioning path and sampling stay
# fp32 -- it is neither the fp32 parity path nor ops.PRECISION's bf16 mode (which rounds activations too).
DECODE_WEIGHTS = ("f32", "bf16")
_WEIGHTS_WARNED = False


# Generation from a token prefix (`DecodeCache.prefill`): the cache rows of the prefix but its last token come from
# ONE batched pass over all of them (the model's full-window kernels, one row per image and not per candidate,
# qarig_decode_cache_fill writing each layer's keys / values into every candidate row) when the prefix has at least
# this many such rows; shorter ones replay the step graph once per token.
# Measured (profiles/r16_prefill_ab.json: tools/bench_generate.py --prefill-ab 7 at config 3's three stages, 4 and 16
# cache rows): the batched pass is ~150 eager launches on a few rows, 1.8 - 2.9 ms whether it covers 4 tokens or 128;
# a replay is 0.21 - 0.44 ms per token.  At 4 rows 8 tokens are a tie (batched / replays 0.93 - 1.07), at 16 rows
# the batched pass wins there in two stages (0.72 - 0.78; the third cell's batched arm was noisy: 1.19); from 12
# tokens up it wins in every cell (0.48 - 0.79 at 12, 0.07 at 128 tokens); at 4 tokens the replays win everywhere
# (1.4 - 2.0).  The batched arm is host-bound (eager launches) and scatters more than the replayed graph.
PREFILL_MIN_TOKENS = 12


def check_decode_weights(weights):
    if weights not in DECODE_WEIGHTS:
        raise ValueError(f"decode weights {weights!r}: expected one of {DECODE_WEIGHTS}")
    return weights


def _warn_weights_fallback(what):
    """Once per process: a bf16 request the streaming kernel cannot serve keeps the fp32 path."""
    global _WEIGHTS_WARNED
    if not _WEIGHTS_WARNED:
        import warnings
        warnings.warn(f'{what}: weights="bf16" needs every per-token Linear on the weight-streaming kernel '
                      "(<= 16 rows, K in {256, 512, 1024}, or 2048 / 4096 without LayerNorm); keeping fp32 weights")
        _WEIGHTS_WARNED = True


def _rows(t, B):
    """A (D,) row of the per-position table as the (B, D) operand the general kernels take."""
    return t if t.dim() == 2 else t.expand(B, t.shape[0]).contiguous()


def window_pad(rows, tokens):
    """Whether a full-window evaluation of `rows` sequences of `tokens` tokens takes one duplicate of the last
    token behind it.  A slid window is window - 1 tokens: rows x 255 is no whole number of 128-row GEMM tiles and
    runs the guarded kernels.  One more token behind the last makes it one (16 x 256 = 4,096 rows) and changes
    nothing before it -- self-attention is causal, everything else is per token -- so the logits wanted are those
    of the last token but one."""
    return (rows * tokens) % 128 != 0 and (rows * (tokens + 1)) % 128 == 0


def _warm_capture(dev, forward):
    """`forward()` as a captured graph: one eager run on a side stream first (kernel loads and the growth of the
    GEMM workspaces cannot happen inside a capture), then the capture.  Returns (graph, what forward returned
    inside the capture)."""
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side), torch.no_grad():
        forward()
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        out = forward()
    return graph, out


@torch.no_grad()
def _cross_kv(model, enc):
    """Per decoder layer: the encoder memory's (k, v) of its cross-attention, token-major (N, S, D), or None."""
    out = []
    for layer in model.decoder_layers:
        at = layer.cross_attn_block.cross_attn if layer.use_cross_attn else None
        out.append(None if at is None else (_mlp2_forward(at.k_block, enc), _mlp2_forward(at.v_block, enc)))
    return out


def _copy_cross_kv(kept, new):
    """The k / v of another encoder memory into the tensors the captured graphs read."""
    for old, kv in zip(kept, new):
        if old is not None:
            old[0].copy_(kv[0])
            old[1].copy_(kv[1])


class DecodeCache:
    def __init__(self, model, enc, batch, max_len, graph=None, positions=None, weights="f32"):
        """positions: optional sequence of max_len floats, the `pos_cond` value of the token at each
        window index (known before the loop: generate_images.py:306-322 numbers them cur + tok + 1);
        given, the conditioning path is evaluated once per position here and `step` ignores `pos`.
        weights: "f32", or "bf16" -- every Linear the step evaluates per token streams the bf16 image of its
        weight (DECODE_WEIGHTS above); a model the streaming kernel does not take keeps fp32 and warns once."""
        self.weights = check_decode_weights(weights)
        if not all(layer.self_attn_block.self_attn.use_masked_attn for layer in model.decoder_layers):
            raise ValueError("a KV cache needs causal decoder self-attention")
        self.model = model
        self.batch = batch
        self.max_len = max_len
        table = model.dec_embedding.weight
        self.dim = table.shape[1]
        dev = table.device
        n_layers = len(model.decoder_layers)
        heads = {layer.self_attn_block.self_attn.heads for layer in model.decoder_layers}
        if len(heads) != 1:
            raise ValueError("a KV cache needs one self-attention head count for all decoder layers")
        self.heads = heads.pop()
        # (layer, k|v, sequence, head, row, head channel): one tensor so that beam bookkeeping can save or
        # restore a chunk of rows for every layer with one copy; head-major, so that the keys of a head are
        # contiguous (the attention kernel's lane-per-key loads then read 2-KB runs instead of 32 B per 2 KB).
        self.kv = torch.zeros((n_layers, 2, batch, self.heads, max_len, self.dim // self.heads),
                              dtype=torch.float32, device=dev)
        self.pe = model._sequence_pe(max_len, self.dim, dev)
        self.ctl = torch.zeros(ops.DECODE_CTL_WORDS, dtype=torch.int32, device=dev)
        self.cross = self._cross_kv(enc)
        self._enc_shape = None if enc is None else tuple(enc.shape)
        self._stack_weights()
        self._img = None            # bf16 mode: id(weight) -> bf16 image, all built here (none inside a capture)
        if weights == "bf16":
            self._build_images()
        self._table = None
        self._cross_tm = self._prefill_cond = None      # prefill's operands, built by the first batched prefill
        if positions is not None and model.use_pos_cond and self._proj_lin and self.dim % 4 == 0:
            self._build_table(positions)
        self._graph = None
        self._search = None
        if graph is None:
            graph = os.environ.get("QARIG_DECODE_GRAPH", "1") != "0"
        if graph:
            self._capture()

    def _cross_kv(self, enc):
        """Per decoder layer: the encoder memory's (k, v) of its cross-attention, head-major, or None."""
        out = []
        for layer, kv in zip(self.model.decoder_layers, _cross_kv(self.model, enc)):
            if kv is not None:
                heads = layer.cross_attn_block.cross_attn.heads
                kv = tuple(t.reshape(t.shape[0], t.shape[1], heads, -1).permute(0, 2, 1, 3).contiguous() for t in kv)
            out.append(kv)
        return out

    @torch.no_grad()
    def rebind(self, enc):
        """The cache for another generation with the SAME model weights, batch and window: the encoder memory's
        keys / values are recomputed into the tensors the captured graphs read, the sequence starts over.  What
        stays: the per-position table of conditioning projections, the stacked weights, the captured step graph
        and the search's buffers (sampling keeps such caches per model: `sampling.decode_cache`).  False when
        the encoder memory's shape differs (the caller builds a new cache)."""
        if (None if enc is None else tuple(enc.shape)) != self._enc_shape:
            return False
        _copy_cross_kv(self.cross, self._cross_kv(enc))
        self._cross_tm = None
        self.ctl.zero_()
        return True

    def _capture(self):
        """Static input buffers, one eager warm-up (sizes the GEMM workspaces outside the
        capture; it only touches cache row 0, which the first real step rewrites), capture."""
        dev = self.kv.device
        self._ids = torch.zeros(self.batch, dtype=torch.int64, device=dev)
        self._pos = torch.zeros(self.batch, dtype=torch.float32, device=dev)
        self.ctl.zero_()
        self._graph, self._out = _warm_capture(dev, lambda: self._forward(self._ids, self._pos, 0, self.ctl))

    @torch.no_grad()
    def step(self, ids, pos, length):
        """ids (B,) int64: the token at window index `length`; pos (B,) fp32 `pos_cond` of
        that token or None (ignored when the cache was built with `positions`).  Appends the
        token's keys/values and returns logits (B, V)."""
        if not 0 <= length < self.max_len:
            raise IndexError(f"cache position {length} outside [0, {self.max_len})")
        if self._graph is None and self._search is not None:      # the search's captured step serves single steps too
            s = self._search
            s.ids.copy_(ids.reshape(self.batch))
            self.ctl[0:1].fill_(length)
            s.g_step.replay()
            return s.logits.clone()
        if self._graph is None:
            return self._forward(ids.reshape(self.batch), pos, length, None)
        self._ids.copy_(ids.reshape(self.batch))
        if pos is not None and self._table is None:
            self._pos.copy_(pos.reshape(self.batch))
        self.ctl[0:1].fill_(length)
        self._graph.replay()
        return self._out.clone()

    # -- launch-count reduction ----------------------------------------------------------------
    # The step time is the number of launches on its dependent chain.  Two groups of small GEMMs are
    # issued as one grouped launch each from weights stacked once at construction: every projection of
    # `cond` (AdaLN scale/shift and residual scale layers of ALL decoder layers: 9 per enc-dec layer;
    # with `positions` they leave the step altogether) and the q/k/v MLPs of a self-attention layer
    # (2 launches instead of 6); the residual layer's x * scale(cond) rides in the attention kernel's output.
    # (Issuing the independent work on side streams as parallel graph branches was measured
    # slower than the serial chain: cross-branch dependencies cost more than they hide.)
    def _stack_weights(self):
        model, D = self.model, self.dim
        ws, bs, self._proj_idx, self._proj_lin = [], [], [], []

        def add(lin):
            ws.append(lin.weight)
            bs.append(lin.bias)
            self._proj_lin.append(lin)
            return len(ws) - 1

        ok = True
        for blocks in model._decoder_blocks():
            idx = {}
            for name, blk, norm, res in blocks:
                if blk.use_adaln0:
                    idx[name + "_norm"] = (add(norm.scale_layer.scale), add(norm.shift_layer.shift))
                if res.use_scale_layer:
                    idx[name + "_scale"] = add(res.scale_layer.scale)
            self._proj_idx.append(idx)
        ok = ok and all(w.shape == (D, D) for w in ws) and D % 256 == 0 and self.batch <= 512
        self._qkv = []
        for layer in model.decoder_layers:
            at = layer.self_attn_block.self_attn
            blocks = (at.q_block, at.k_block, at.v_block)
            w1 = [_lin_params(b[0])[0] for b in blocks]
            ok = ok and all(w.shape == w1[0].shape for w in w1) and w1[0].shape[0] % 256 == 0 \
                and len({b[0]._act for b in blocks}) == 1 and len({b[1]._act for b in blocks}) == 1
            self._qkv.append(blocks)
        self._stacked = bool(ok)
        if not self._stacked:
            return
        with torch.no_grad():
            if ws:
                self._proj_w = torch.stack([w.detach() for w in ws]).contiguous()
                self._proj_b = torch.stack([b.detach() for b in bs]).contiguous()
            packed = []
            for blocks in self._qkv:
                packed.append((
                    torch.stack([_lin_params(b[0])[0].detach() for b in blocks]).contiguous(),
                    torch.stack([_lin_params(b[0])[1].detach() for b in blocks]).contiguous(),
                    torch.stack([_lin_params(b[1])[0].detach() for b in blocks]).contiguous(),
                    torch.stack([_lin_params(b[1])[1].detach() for b in blocks]).contiguous(),
                    blocks[0][0]._act, blocks[0][1]._act))
            self._qkv = packed

    def _step_linears(self):
        """The Linear layers a step evaluates per token besides the stacked q/k/v MLPs: the two-layer MLPs that sit
        behind a LayerNorm, the residual layers, the classifier."""
        mlps, res = [], []
        for layer in self.model.decoder_layers:
            res.append(layer.self_attn_block.self_attn_res)
            if layer.use_cross_attn:
                mlps.append(layer.cross_attn_block.cross_attn.q_block)
                res.append(layer.cross_attn_block.cross_attn_res)
            mlps.append(layer.feedforward_block.feedforward)
            res.append(layer.feedforward_block.feedforward_res)
        return mlps, res, self.model.classifier

    @torch.no_grad()
    def _build_images(self):
        """bf16 mode: the image of every weight `_forward` streams -- the stacked q/k/v weights cast here, single
        weights through functional_lp._shadow (the optimiser's own bf16 copy, or a cast cached until the weights
        change) -- or, when some Linear of the step does not fit the streaming kernel, none and the fp32 path."""
        B, D = self.batch, self.dim
        fits = lambda w, ln: ops.decode_linear_supported(B, w.shape[-2], w.shape[-1], ln)
        mlps, res, classifier = self._step_linears()
        ok = self._stacked and FUSE_NORMS and B <= 16 and D % 4 == 0
        singles = []
        for seq, ln in [(q, True) for q in mlps] + [(classifier, False)]:
            (w1, b1), (w2, b2) = _lin_params(seq[0]), _lin_params(seq[1])
            ok = ok and b1 is not None and b2 is not None and w1.shape[1] == D and fits(w1, ln) and fits(w2, False)
            singles += [w1, w2]
        for r in res:
            w = _lin_params(r.linear)[0]
            ok = ok and isinstance(r.skip_linear, torch.nn.Identity) and w.shape[1] == D and fits(w, False)
            singles.append(w)
        ok = ok and all(fits(q[0], True) and fits(q[2], False) for q in self._qkv)
        if not ok:
            _warn_weights_fallback("DecodeCache")
            return
        self._img = {id(w): QL._shadow(w) for w in singles}
        self._qkv_lp = [(ops.cast_bf16(w1), b1, ops.cast_bf16(w2), b2, a1, a2) for w1, b1, w2, b2, a1, a2 in self._qkv]

    def _w(self, w):
        """The operand a step's Linear streams for weight `w`: its bf16 image in bf16 mode, `w` itself otherwise."""
        return w if self._img is None else self._img[id(w)]

    @torch.no_grad()
    def _build_table(self, positions):
        """(max_len, P * D): row L holds every projection of cond(positions[L]); the views of `_proj_row`
        (the row of the step in flight) are what the launches of a step read."""
        dev, D, L = self.kv.device, self.dim, self.max_len
        pos = torch.as_tensor(list(positions), dtype=torch.float32, device=dev)
        if pos.shape != (L,):
            raise ValueError(f"positions: {tuple(pos.shape)} values for {L} cache rows")
        cond = _mlp2_forward(self.model.pos_cond_layer, ops.posemb(pos, D).reshape(1, L, D)).reshape(L, D)
        P = len(self._proj_lin)
        if self._stacked and L <= 512:
            allp = ops.gemm_grouped_skinny(cond.contiguous(), self._proj_w, self._proj_b, shared_a=True)   # (P, L, D)
        else:
            allp = torch.stack([QF.linear_act(cond.reshape(1, L, D), lin.weight, lin.bias).reshape(L, D)
                                for lin in self._proj_lin])
        self._table = allp.permute(1, 0, 2).reshape(L, P * D).contiguous()
        self._proj_row = torch.zeros((P, D), dtype=torch.float32, device=dev)
        pick = lambda v: (self._proj_row[v[0]], self._proj_row[v[1]]) if isinstance(v, tuple) else self._proj_row[v]
        self._row_proj = [{k: pick(v) for k, v in idx.items()} for idx in self._proj_idx]

    def _cond_projections(self, cond):
        """Per decoder layer: dict key -> tensor(s) (B,1,D) that depend on `cond` alone."""
        layers = self.model.decoder_layers
        if cond is None:
            return [{} for _ in layers]
        B, D = self.batch, self.dim
        if self._stacked and self._proj_idx and any(self._proj_idx):
            allp = ops.gemm_grouped_skinny(cond.reshape(B, D), self._proj_w, self._proj_b,
                                           shared_a=True)                       # (P, B, D)
            pick = lambda v: (allp[v[0]], allp[v[1]]) if isinstance(v, tuple) else allp[v]
            return [{k: pick(v) for k, v in idx.items()} for idx in self._proj_idx]
        out = []
        for blocks in self.model._decoder_blocks():
            proj = {}
            for name, blk, norm, res in blocks:
                if blk.use_adaln0:
                    proj[name + "_norm"] = (norm.scale_layer(cond).reshape(B, D), norm.shift_layer(cond).reshape(B, D))
                if res.use_scale_layer:
                    proj[name + "_scale"] = res.scale_layer(cond).reshape(B, D)
            out.append(proj)
        return out

    def _norm(self, norm, x, proj, key, use_adaln0):
        if use_adaln0:
            scale, shift = proj[key]
            B = self.batch
            return QF.layernorm_mod(x, _rows(scale, B).reshape(x.shape), _rows(shift, B).reshape(x.shape),
                                    norm.norm.eps)
        return QF.layernorm_affine(x, norm.weight, norm.bias, norm.eps)

    def _ln_mlp(self, norm, x, proj, key, use_adaln0, seq, mul=None, stacked=None):
        """The block's two-layer MLP on LayerNorm(x): the norm rides in the first Linear's launch and `mul`
        -- the residual layer's scale(cond) -- in the second's.  stacked: (w1, b1, w2, b2, act1, act2) with a
        leading group dimension (the q/k/v MLPs).  Returns (B, D), or (G, B, D) for a stacked MLP; None when the
        shapes do not fit the fused launches."""
        B, D = self.batch, self.dim
        if stacked is not None:
            w1, b1, w2, b2, act1, act2 = stacked
        else:
            (w1, b1), (w2, b2) = _lin_params(seq[0]), _lin_params(seq[1])
            act1, act2 = seq[0]._act, seq[1]._act
        if D % 256 or B > 512 or w1.shape[-1] != D or w2.shape[-1] % 256 or b1 is None or b2 is None:
            return None
        x2 = x.reshape(B, D)
        H = w1.shape[-2]
        if B <= 16 and ops.decode_linear_supported(B, H, D, True) and ops.decode_linear_supported(B, D, H, False):
            if stacked is None:
                w1, w2 = self._w(w1), self._w(w2)
            if use_adaln0:
                scale, shift = proj[key]
                hid = ops.decode_linear(x2, w1, b1, act1, scale=scale, shift=shift, eps=norm.norm.eps)
            else:
                hid = ops.decode_linear(x2, w1, b1, act1, gamma=norm.weight, beta=norm.bias, eps=norm.eps)
            return ops.decode_linear(hid, w2, b2, act2, mul=mul)
        if use_adaln0:
            scale, shift = proj[key]
            hid = ops.gemm_skinny_ln(x2, w1, b1, act1, scale=_rows(scale, B), shift=_rows(shift, B),
                                     eps=norm.norm.eps)
        else:
            hid = ops.gemm_skinny_ln(x2, w1, b1, act1, gamma=norm.weight, beta=norm.bias, eps=norm.eps)
        if stacked is not None:
            return ops.gemm_grouped_skinny(hid, w2, b2, act=act2)
        return ops.gemm_skinny_ln(hid, w2, b2, act2, mul=None if mul is None else _rows(mul, B))

    def _residual(self, res, x, x_skip, proj, key, scaled=False):
        """ResidualLinearLayer.forward with the scale projection supplied (`scaled`: the
        producer of x already applied it)."""
        if res.use_scale_layer and not scaled:
            x = QF.mul(x, _rows(proj[key], self.batch).reshape(x.shape))
        w, b = _lin_params(res.linear)
        if self._img is not None:       # bf16 mode: straight to the streaming kernel (skip_linear is the identity)
            B = self.batch
            y = ops.decode_linear(x.reshape(B, -1), self._w(w), b, res._act, residual=x_skip.reshape(B, -1))
            return y.reshape(B, 1, -1)
        return QF.linear_act(x, w, b, residual=res.skip_linear(x_skip), act=res._act)

    def _forward(self, ids, pos, length, len_dev, out=None):
        """One decoder step on one new row per sequence.  len_dev: the control words (graph replay:
        the kernels read the cache length from ctl[0]) or None (the host value `length`).
        out: optional (B, V) buffer for the logits."""
        model, B, D = self.model, self.batch, self.dim
        if D % 4 == 0:
            tab = self._table
            x = ops.decode_embed(ids, model.dec_embedding.weight, self.pe, ctl=len_dev, length=length,
                                 proj_table=tab, proj_row=self._proj_row if tab is not None else None)
            x = x.reshape(B, 1, D)
        else:
            x = QF.embedding_pos(ids.reshape(B, 1), model.dec_embedding.weight, self.pe[length:length + 1])
            assert len_dev is None, "graph replay needs a model width that is a multiple of 4"
        if self._table is not None:
            projections = self._row_proj
        else:
            cond = None
            if model.use_pos_cond:
                cond = ops.posemb(pos.reshape(B), D).reshape(B, 1, D)
                cond = _mlp2_forward(model.pos_cond_layer, cond)
            projections = self._cond_projections(cond)
        for li, layer in enumerate(model.decoder_layers):
            proj = projections[li]
            sab = layer.self_attn_block
            at = sab.self_attn
            qkv = self._ln_mlp(sab.self_attn_norm, x, proj, "self_norm", sab.use_adaln0, None,
                               stacked=self._qkv[li] if self._img is None else self._qkv_lp[li]) \
                if self._stacked and FUSE_NORMS else None
            if qkv is not None:
                q, k, v = qkv
            else:
                h = self._norm(sab.self_attn_norm, x, proj, "self_norm", sab.use_adaln0)
                if self._stacked:
                    w1, b1, w2, b2, act1, act2 = self._qkv[li]
                    hid = ops.gemm_grouped_skinny(h.reshape(B, D), w1, b1, act=act1, shared_a=True)
                    q, k, v = ops.gemm_grouped_skinny(hid, w2, b2, act=act2)
                else:
                    q = _mlp2_forward(at.q_block, h).reshape(B, D)
                    k = _mlp2_forward(at.k_block, h).reshape(B, D)
                    v = _mlp2_forward(at.v_block, h).reshape(B, D)
            o_mul = proj["self_scale"] if "self_scale" in proj else None
            o = ops.attention_decode(q, k, v, self.kv[li, 0], self.kv[li, 1], length, at.heads,
                                     len_dev=len_dev, o_mul=o_mul)
            x = self._residual(sab.self_attn_res, o.reshape(B, 1, D), x, proj, "self_scale", scaled=True)
            if layer.use_cross_attn:
                cab = layer.cross_attn_block
                at = cab.cross_attn
                ck, cv = self.cross[li]
                q = self._ln_mlp(cab.cross_attn_norm, x, proj, "cross_norm", cab.use_adaln0, at.q_block) \
                    if FUSE_NORMS else None
                if q is None:
                    h = self._norm(cab.cross_attn_norm, x, proj, "cross_norm", cab.use_adaln0)
                    q = _mlp2_forward(at.q_block, h).reshape(B, D)
                o_mul = proj["cross_scale"] if "cross_scale" in proj else None
                o = ops.attention_decode(q, None, None, ck, cv, ck.shape[2], at.heads, o_mul=o_mul)
                x = self._residual(cab.cross_attn_res, o.reshape(B, 1, D), x, proj, "cross_scale",
                                   scaled=True)
            fb = layer.feedforward_block
            gate = proj["ffn_scale"] if fb.feedforward_res.use_scale_layer else None
            h = self._ln_mlp(fb.feedforward_norm, x, proj, "ffn_norm", fb.use_adaln0, fb.feedforward, mul=gate) \
                if FUSE_NORMS else None
            if h is not None:
                x = self._residual(fb.feedforward_res, h.reshape(B, 1, D), x, proj, "ffn_scale", scaled=True)
            else:
                h = self._norm(fb.feedforward_norm, x, proj, "ffn_norm", fb.use_adaln0)
                h = _mlp2_forward(fb.feedforward, h)
                x = self._residual(fb.feedforward_res, h, x, proj, "ffn_scale")
        (w1, b1), (w2, b2) = _lin_params(model.classifier[0]), _lin_params(model.classifier[1])
        if self._img is not None:
            hid = ops.decode_linear(x.reshape(B, D), self._w(w1), b1, model.classifier[0]._act)
            return ops.decode_linear(hid, self._w(w2), b2, model.classifier[1]._act, out=out)
        if out is not None and B <= 16 and b1 is not None and b2 is not None and \
                ops.decode_linear_supported(B, w1.shape[0], D, False) and \
                ops.decode_linear_supported(B, w2.shape[0], w2.shape[1], False):
            hid = ops.decode_linear(x.reshape(B, D), w1, b1, model.classifier[0]._act)
            ops.decode_linear(hid, w2, b2, model.classifier[1]._act, out=out)      # straight into the caller's buffer
            return out
        logits = _mlp2_forward(model.classifier, x).reshape(B, -1)
        if out is not None:
            out.copy_(logits)
            return out
        return logits

    def rows(self, lo, hi):
        """View of cache rows [lo, hi) of every layer: (layer, 2, B, H, hi-lo, d)."""
        return self.kv[:, :, :, :, lo:hi]

    # -- generation from a token prefix ---------------------------------------------------------
    def prefill_batched(self, P1):
        """Whether `prefill` evaluates P1 prefix rows as one batched pass (else: P1 replays of the step).
        The replays serve bf16 step weights (every Linear of the cache then keeps that mode's rounded weights),
        a position-conditioned model whose cache has no per-position table, a model width that is no multiple
        of 4 (the fill kernel's 16-B rows), and prefixes below PREFILL_MIN_TOKENS."""
        return P1 >= max(1, PREFILL_MIN_TOKENS) and self.weights == "f32" and self.dim % 4 == 0 and \
            (self.dim // self.heads) % 4 == 0 and not (self.model.use_pos_cond and self._table is None)

    @torch.no_grad()
    def prefill(self, tokens, pos=None):
        """Cache rows [0, P1) of every layer from `tokens` (images, P1) int64 -- a prefix without its last token,
        one row per image: every candidate row of an image (batch = images x beams, beams of an image adjacent)
        receives the image's keys and values.  The logits of these tokens are not evaluated; the caller runs the
        prefix's last token through `step` (or the search's graph) like any other.  A run that continues from here
        is a from-scratch run interrupted at this point, up to fp32 summation order.
        pos: the `pos_cond` value of each of the P1 window indices, needed only by a cache built without
        `positions` for a position-conditioned model (the step replays then take it)."""
        tokens = tokens.to(torch.int64)
        images, P1 = tokens.shape
        if images < 1 or self.batch % images:
            raise ValueError(f"prefill: {images} images do not divide the cache's {self.batch} rows")
        if P1 > self.max_len:
            raise IndexError(f"prefill: {P1} prefix rows for a cache of {self.max_len}")
        if P1 == 0:
            return
        beams = self.batch // images
        if not self.prefill_batched(P1):
            B, dev = self.batch, self.kv.device
            for t in range(P1):
                p = None
                if self.model.use_pos_cond and self._table is None:
                    p = torch.full((B,), float(pos[t]), device=dev)
                self.step(tokens[:, t].repeat_interleave(beams) if beams > 1 else tokens[:, t], p, t)
            return
        self._prefill_forward(tokens.contiguous(), beams)

    def _prefill_operands(self, images, P1):
        """(cond, cross): the CondTable that reads the cache's own per-position projections at window indices
        0 .. P1-1 of every image (None without position conditioning), and per layer the encoder memory's
        token-major (k, v) of one row per image (None without cross-attention).  Both are built from what the
        cache holds: the projections per Linear once per cache, the k / v once per encoder memory."""
        dev, D, L = self.kv.device, self.dim, self.max_len
        cond = None
        if self._table is not None:
            if self._prefill_cond is None:
                P = len(self._proj_lin)
                self._prefill_cond = self._table.view(L, P, D).permute(1, 0, 2).contiguous()       # (P, L, D)
            tabs = self._prefill_cond
            idx = torch.arange(P1, dtype=torch.int32, device=dev).repeat(images)
            cond = QF.CondTable(tabs[0], idx, (images, P1))
            for j, lin in enumerate(self._proj_lin):
                cond._proj[id(lin)] = tabs[j]
        if self._cross_tm is None or self._cross_tm[0] != images:
            beams = self.batch // images
            tm = lambda t: t[::beams].permute(0, 2, 1, 3).reshape(images, t.shape[2], -1).contiguous()
            self._cross_tm = (images, [None if c is None else (tm(c[0]), tm(c[1])) for c in self.cross])
        return cond, self._cross_tm[1]

    def _prefill_forward(self, tokens, beams):
        """The batched pass: window assembly as QF.embedding_pos does it, then per layer what WindowStep._forward
        spells out for its last layer, on all rows -- norm, q / k / v MLPs, causal attention, residual,
        cross-attention block on the cache's cross k / v, feed-forward -- with the layer's k and v written into
        the cache by one qarig_decode_cache_fill launch.  The last layer stops behind its k / v: nothing reads
        the rows' outputs (the logits are discarded)."""
        model = self.model
        images, P1 = tokens.shape
        cond, cross = self._prefill_operands(images, P1)
        x = QF.embedding_pos(tokens, model.dec_embedding.weight, self.pe[:P1])
        layers = model.decoder_layers
        for li, layer in enumerate(layers):
            sab = layer.self_attn_block
            at = sab.self_attn
            h, _ = _norm_forward(sab.self_attn_norm, x, cond, sab.use_adaln0)
            final = li == len(layers) - 1
            k = _mlp2_forward(at.k_block, h)
            v = _mlp2_forward(at.v_block, h)
            ops.decode_cache_fill(k, v, self.kv[li], beams)
            if final:
                break
            q = _mlp2_forward(at.q_block, h)
            o = QF.attention(q, k, v, at.heads, True)
            x = sab.self_attn_res(x=o, x_skip=x, cond=cond)
            if layer.use_cross_attn:
                x = layer.cross_attn_block(x, cross_cond=None, cond=cond, kv=cross[li])
            x = layer.feedforward_block(x, cond=cond)

    # -- device-resident chunk search ----------------------------------------------------------
    @torch.no_grad()
    def begin_search(self, first_ids, images, beams, beam_width, temperature, end_token, shift, generate_mode,
                     max_chunks, candidates, forced=None, log_probs=False, generator=None, reference_order=False,
                     top_k=0, top_p=1.0):
        """Prepares the search of generate_images.py:256-345 on `images` x `beams` cache rows (beams > 1:
        the candidate chunks of an image as rows of one batch; beams == 1: `candidates` chunks one after the
        other): evaluates the first token (window index 0), captures the step's graph, draws the uniforms of
        every draw the stage can make (ONE call of the device generator).  first_ids: (N,) or (N, 1) ids, or an
        (N, P) prefix: its first P - 1 tokens are prefilled (`prefill`), the step is replayed for token P - 1 and
        the chunk search starts at window index P.  forced: optional (draws, columns)
        int64, entries >= 0 replace the draw (tests); log_probs: keep every probability row sampled from.
        top_k / top_p: every draw of the search is made from the filtered row (ops.decode_sample; 0 / 1.0: off).
        The draws are launches of their own between the replays of the step graph, so the graph does not change.

        reference_order (beams > 1): the candidates of a chunk are independent given the kept prefix, so they
        run as rows of one batch, but every draw keeps the number the reference's candidate-after-candidate
        loop gives it -- draw (chunk * beams + candidate) * beam_width + slot, one column per image -- and the
        first best candidate wins as in the reference's `>` comparison: the same tokens from the same draws as
        beams == 1 with `candidates` = beams, at the cost of the batched search."""
        N, NB, bw = int(images), int(beams), int(beam_width)
        B, D, dev = self.batch, self.dim, self.kv.device
        top_k, top_p = ops.check_sample_filter(top_k, top_p)
        if N * NB != B or self.dim % 4:
            raise ValueError("begin_search: images * beams must equal the cache's batch (and the width be 4-aligned)")
        if self.model.use_pos_cond and self._table is None:
            raise ValueError("begin_search: a position-conditioned model needs the cache built with `positions`")
        V = _lin_params(self.model.classifier[1])[0].shape[0]
        ordered = bool(reference_order) and NB > 1
        if ordered and int(candidates) != 1:
            raise ValueError("begin_search: reference_order runs every candidate as a row (candidates must be 1)")
        per_chunk = (NB if ordered else int(candidates)) * bw       # draw rows one chunk position consumes
        cols = N if ordered else B
        draws = max(1, int(max_chunks) * per_chunk)
        # The buffers the captured step graph reads and writes, and the graph itself, are kept across searches of
        # the same geometry (a cache that sampling.decode_cache handed out again): no capture, no eager warm-up.
        s = self._search
        fresh = s is None or (s.N, s.NB, s.bw, s.V) != (N, NB, bw, V)
        if fresh:
            s = SimpleNamespace(N=N, NB=NB, bw=bw, V=V)
            s.ids = torch.zeros(B, dtype=torch.int64, device=dev)
            s.comb = torch.ones(B, dtype=torch.float32, device=dev)
            s.chunk = torch.zeros((B, bw), dtype=torch.int64, device=dev)
            s.best_p = torch.zeros(N, dtype=torch.float32, device=dev)
            s.best_chunk = torch.zeros((N, bw), dtype=torch.int64, device=dev)
            s.take = torch.zeros(N, dtype=torch.int32, device=dev)
            R = max(bw - 1, 1)
            s.staged = torch.zeros((self.kv.shape[0], 2, N, self.heads, R, D // self.heads), dtype=torch.float32,
                                   device=dev)
            s.tokens = torch.zeros((N, self.max_len + bw), dtype=torch.int64, device=dev)
            s.last = torch.zeros((B, V), dtype=torch.float32, device=dev)
            s.logits = torch.zeros((B, V), dtype=torch.float32, device=dev)
            s.g_step = None
        else:
            s.comb.fill_(1.0)
            s.tokens.zero_()
        s.draws, s.used, s.chunks, s.candidates = draws, 0, 0, int(candidates)
        s.beams, s.per_set = (NB if ordered else 0), (NB * bw if ordered else bw)
        s.uniforms = torch.rand((draws, cols), device=dev, generator=generator)
        s.forced = None
        if forced is not None:
            s.forced = torch.full((draws, cols), -1, dtype=torch.int64, device=dev)
            f = torch.as_tensor(forced, dtype=torch.int64, device=dev).reshape(-1, cols)[:draws]
            s.forced[:f.shape[0]] = f
        s.probs = torch.zeros((draws, cols, V), dtype=torch.float32, device=dev) if log_probs else None
        first = first_ids.to(torch.int64)
        prefix = first.reshape(N, 1) if first.dim() < 2 else first.reshape(N, -1)
        P = prefix.shape[1]
        if not 1 <= P <= self.max_len:
            raise ValueError(f"begin_search: a prefix of {P} tokens for a cache of {self.max_len} rows")
        s.P = P
        s.tokens[:, :P] = prefix
        s.ids.copy_(prefix[:, 0].repeat_interleave(NB))
        self.ctl.zero_()
        s.gen, s.T, s.end, s.shift = bool(generate_mode), float(temperature), int(end_token), int(shift)
        s.top_k, s.top_p = top_k, top_p
        if s.g_step is None:
            # A capture records launches without running them, and the first launch of a kernel in a process (code
            # object load) or a workspace that has to grow cannot happen inside one: the first step of a given
            # shape in this process runs eagerly once; later stages of that shape go straight to the capture and
            # evaluate their first token by replaying it.
            sig = (B, D, V, self.heads, len(self.model.decoder_layers), tuple(c is not None for c in self.cross),
                   self._table is not None, self._stacked, FUSE_NORMS, self._img is not None,
                   tuple(k.shape[2] for c in self.cross if c is not None for k in c[:1]))
            if sig not in _WARM_SHAPES:
                self._forward(s.ids, None, 0, self.ctl, out=s.logits)
                self.ctl.zero_()
                _WARM_SHAPES.add(sig)
            s.g_step = torch.cuda.CUDAGraph()
            with torch.cuda.graph(s.g_step):
                self._forward(s.ids, None, 0, self.ctl, out=s.logits)
        self._search = s
        if P > 1:
            # the prefix but its last token fills cache rows [0, P - 1); the last one goes through the captured
            # step like every token after it, so s.last comes from the same kernels as always
            self.prefill(prefix[:, :P - 1])
            s.ids.copy_(prefix[:, P - 1].repeat_interleave(NB))
            self.ctl[0:1].fill_(P - 1)
        s.g_step.replay()                      # the prefix's last token, window index P - 1 (from scratch: 0)
        s.last.copy_(s.logits)
        # chunk search starts behind the prefix: window index P (from scratch: 1)
        self.ctl.zero_()
        self.ctl[0:2].fill_(P)
        return s

    def _draw(self, slot, src, inc):
        s = self._search
        ops.decode_sample(src, s.T, s.end, s.gen, s.shift, s.uniforms, self.ctl, slot, s.bw, s.ids, s.chunk, s.comb,
                          forced=s.forced, probs_log=s.probs, inc_len=inc, beams=s.beams, top_k=s.top_k, top_p=s.top_p)

    @torch.no_grad()
    def run_chunk(self, last=False):
        """One chunk position: `candidates` candidate chunks, then the kept one joins the sequence (and, unless
        `last`, its final token is evaluated for the next chunk's first draw).  Enqueues only -- the decoder step
        as one graph replay, sampling and bookkeeping as single launches -- and never synchronises."""
        s = self._search
        N, NB, bw = s.N, s.NB, s.bw
        for _ in range(s.candidates):
            self._draw(0, s.last, False)                    # every candidate's first draw: the kept prefix's logits
            for _ in range(1, bw):
                s.g_step.replay()                           # the token just drawn, at window index ctl[0]
                self._draw(-1, s.logits, True)              # slot = steps since the candidate began (ctl[4])
            ops.decode_decide(self.ctl, N, NB, bw, s.comb, s.chunk, s.best_p, s.best_chunk, s.take, draws=s.per_set)
            if bw > 1:
                ops.decode_rows(self.ctl, self.kv, s.staged, s.take, N, NB, restore=False)
        if bw > 1:
            ops.decode_rows(self.ctl, self.kv, s.staged, s.take, N, NB, restore=True)
        ops.decode_commit(self.ctl, N, NB, bw, s.best_chunk, s.tokens, s.ids)
        if not last:
            s.g_step.replay()
            s.last.copy_(s.logits)
        ops.decode_advance(self.ctl, bw)
        s.used += s.candidates * s.per_set
        s.chunks += 1

    def finish_search(self):
        """(N, P + chunks * beam_width) tokens of the sequences, the P tokens of the prefix (from scratch: the
        first token) included."""
        s = self._search
        return s.tokens[:, :s.P + s.chunks * s.bw].clone()


def _mlp2_fits(seq, R):
    (w1, b1), (w2, b2) = _lin_params(seq[0]), _lin_params(seq[1])
    return b1 is not None and b2 is not None and ops.decode_linear_supported(R, w1.shape[0], w1.shape[1], False) and \
        ops.decode_linear_supported(R, w2.shape[0], w2.shape[1], False)


def _mlp2_rows(seq, x, out=None, weights="f32", images=None):
    """The two-layer MLP `seq` on R <= 16 rows x (R, K): the weight-streaming decode kernel when the shapes
    fit it, the general kernels otherwise.  Returns (R, N) (written into `out` when given).
    weights "bf16": the streaming kernel reads the weights' bf16 images (DECODE_WEIGHTS) -- from `images`
    (id(weight) -> image; a caller that captures a graph builds them first) or functional_lp._shadow; shapes the
    kernel does not take run in fp32 as before."""
    check_decode_weights(weights)
    (w1, b1), (w2, b2) = _lin_params(seq[0]), _lin_params(seq[1])
    R, K = x.shape
    if _mlp2_fits(seq, R) and w1.shape[1] == K:
        if weights == "bf16":
            w1, w2 = ((images[id(w)] if images is not None and id(w) in images else QL._shadow(w)) for w in (w1, w2))
        hid = ops.decode_linear(x, w1, b1, seq[0]._act)
        return ops.decode_linear(hid, w2, b2, seq[1]._act, out=out)
    y = _mlp2_forward(seq, x.reshape(R, 1, K)).reshape(R, -1)
    if out is not None:
        out.copy_(y)
        return out
    return y


class WindowStep:
    """One evaluation of the slid window (generate_images.py:275-290): the last `window - 1` tokens of each of
    `rows` sequences through `model.decode` with window-relative positional embeddings, logits of the last token.

    The tokens live in a device ring (rows, capacity) whose length is the control word ctl[5]
    (`ops.window_append` adds the sampled ids); the evaluation reads nothing from the host, so it is captured
    once and replayed:
      window assembly (embedding + sinusoid, the row of every token in the conditioning table) ->
      decoder layers 0 .. L-2 on all rows (the model's own layer forwards) ->
      last layer: norm and the k / v MLPs on all rows, then q, attention, residual, cross-attention and
      feed-forward on the last real row of each sequence alone -> classifier on those rows.
    Built once: the conditioning table of positions 0 .. pos_bound with every ScaleLayer / ShiftLayer
    projection of it (models/layers.py:100-153, 258-304), and the cross-attention k / v of the encoder output
    for every layer (`rebind` recomputes them for another stage's encoder output).
    pos_off: the loop's position numbering (1: generate_images.py:306-322, cur + tok + 1; 0: training's)."""

    def __init__(self, model, enc, rows, window, capacity, pos_bound, pos_off, graph=True, weights="f32"):
        """weights "bf16": the two <= 16-row MLPs of the evaluation (last layer's q, classifier) stream bf16
        images of their weights (DECODE_WEIGHTS); everything on all rows of the window stays as it is."""
        self.weights = check_decode_weights(weights)
        table = model.dec_embedding.weight
        self.model, self.rows, self.window = model, int(rows), int(window)
        self.dim, dev = table.shape[1], table.device
        heads = model.decoder_layers[-1].self_attn_block.self_attn.heads
        if not ops.window_step_supported(self.rows, self.window, self.dim, heads):
            raise ValueError(f"WindowStep: {rows} rows, window {window}, width {self.dim}, {heads} heads do not fit "
                             "the window kernels (<= 16 rows, head dim a multiple of 4 from 4 to 128)")
        if not all(l.self_attn_block.self_attn.use_masked_attn for l in model.decoder_layers):
            raise ValueError("WindowStep: needs causal decoder self-attention")
        R, D = self.rows, self.dim
        self.W1 = self.window - 1
        self.pad = window_pad(R, self.W1)
        self.Wp = self.W1 + int(self.pad)
        self.pos_off = int(pos_off)
        self.ring = torch.zeros((R, int(capacity)), dtype=torch.int64, device=dev)
        self.ctl = torch.zeros(ops.DECODE_CTL_WORDS, dtype=torch.int32, device=dev)
        self.pe = model._sequence_pe(self.Wp, D, dev)
        self.x = torch.empty((R, self.Wp, D), dtype=torch.float32, device=dev)
        self.logits = torch.empty((R, _lin_params(model.classifier[1])[0].shape[0]), dtype=torch.float32, device=dev)
        self.cond = self.cond_last = self.rowmap = self.last_map = None
        self.P = 0
        with torch.no_grad():
            if model.use_pos_cond:
                self._build_table(pos_bound)
            self.cross = _cross_kv(model, enc)
            self._enc_shape = None if enc is None else tuple(enc.shape)
            self._img = None        # bf16 mode: the images exist before the capture
            if weights == "bf16":
                seqs = (model.decoder_layers[-1].self_attn_block.self_attn.q_block, model.classifier)
                if all(_mlp2_fits(seq, self.rows) for seq in seqs):
                    self._img = {id(w): QL._shadow(w) for seq in seqs for w in (_lin_params(seq[0])[0],
                                                                                 _lin_params(seq[1])[0])}
                else:
                    _warn_weights_fallback("WindowStep")
        self._graph = None
        if graph:
            self._capture()

    def _build_table(self, pos_bound):
        """cond of positions 0 .. P-1 (P: pos_bound in whole 128-row tiles, as Transformer._cond sizes it) and
        every projection of it, evaluated here once; the graph only gathers rows of them."""
        model, D, dev = self.model, self.dim, self.ring.device
        P = (int(pos_bound) + 127) // 128 * 128
        tab = _mlp2_forward(model.pos_cond_layer, ops.posemb(torch.arange(P, device=dev), D))
        R, Wp = self.rows, self.Wp
        self.rowmap = torch.zeros(R * Wp, dtype=torch.int32, device=dev)
        self.last_map = torch.zeros(R, dtype=torch.int32, device=dev)
        groups = model._cond_linear_groups()
        self.cond = QF.CondTable(tab, self.rowmap, (R, Wp), groups=groups)
        self.cond_last = QF.CondTable(tab, self.last_map, (R, 1), groups=groups)
        for lin in (l for per in model._cond_linears_per_layer() for l in per):
            self.cond._proj[id(lin)] = self.cond.projection(lin)
        self.cond_last._proj = self.cond._proj
        # the assembly kernel writes in-range rows (clamped, flagged) straight into the maps the consumers read
        self.cond.idx, self.cond_last.idx = self.rowmap, self.last_map
        self.P = P

    def rebind(self, enc):
        """The step for another stage with the same weights and shapes: the encoder output's cross-attention
        k / v are recomputed into the tensors the graph reads.  False when its shape differs."""
        if (None if enc is None else tuple(enc.shape)) != self._enc_shape:
            return False
        _copy_cross_kv(self.cross, _cross_kv(self.model, enc))
        return True

    @torch.no_grad()
    def load(self, tokens):
        """tokens (rows, n) int64: the sequences so far; the ring holds them and its length becomes n."""
        n = tokens.shape[1]
        if not 0 < n <= self.ring.shape[1]:
            raise ValueError(f"WindowStep.load: {n} tokens for a ring of {self.ring.shape[1]}")
        self.ring[:, :n].copy_(tokens)
        self.ctl[ops.CTL_RING:ops.CTL_RING + 1].fill_(n)

    def append(self, ids):
        """ids (rows,) int64 join the ring (device-side length)."""
        ops.window_append(self.ctl, self.ring, ids)

    def rewind(self, n):
        """The ring's length back to n (a candidate chunk starts over at the chunk position)."""
        self.ctl[ops.CTL_RING:ops.CTL_RING + 1].fill_(int(n))

    def _capture(self):
        dev = self.ring.device
        saved = self.ctl.clone()
        self.ctl[ops.CTL_RING:ops.CTL_RING + 1].fill_(self.W1)     # a valid window for the warm-up
        graph, _ = _warm_capture(dev, self._forward)
        self.ctl.copy_(saved)
        self._graph = graph

    @torch.no_grad()
    def evaluate(self):
        """Logits (rows, V) of the last token of the window in front of the ring's length (a buffer that the
        next evaluation overwrites)."""
        if self._graph is not None:
            self._graph.replay()
        else:
            self._forward()
        return self.logits

    def _forward(self):
        model, R, D = self.model, self.rows, self.dim
        ops.window_assemble(self.ring, self.ctl, model.dec_embedding.weight, self.pe, self.W1, self.pad, self.x,
                            self.rowmap, self.last_map, self.P, self.pos_off)
        x, cond = self.x, self.cond
        layers = model.decoder_layers
        for li, layer in enumerate(layers[:-1]):
            x = layer(x=x, cross_cond=None, pos_cond=cond, cross_kv=self.cross[li])
        layer, last = layers[-1], self.W1 - 1
        sab = layer.self_attn_block
        at = sab.self_attn
        h, _ = _norm_forward(sab.self_attn_norm, x, cond, sab.use_adaln0)
        k = _mlp2_forward(at.k_block, h)
        v = _mlp2_forward(at.v_block, h)
        lp = dict(weights="bf16", images=self._img) if self._img is not None else {}
        q = _mlp2_rows(at.q_block, h[:, last].contiguous(), **lp)
        o = ops.window_attention(q, k, v, self.W1, at.heads)
        # from here on only the last real token of each sequence is read (logits[:, -1])
        x = sab.self_attn_res(x=o.reshape(R, 1, D), x_skip=x[:, last:last + 1].contiguous(), cond=self.cond_last)
        if layer.use_cross_attn:
            x = layer.cross_attn_block(x, cross_cond=None, cond=self.cond_last, kv=self.cross[-1])
        x = layer.feedforward_block(x, cond=self.cond_last)
        _mlp2_rows(model.classifier, x.reshape(R, D), out=self.logits, **lp)
