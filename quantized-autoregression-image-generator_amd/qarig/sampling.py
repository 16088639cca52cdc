"""Autoregressive token sampling as the reference does it, on the device:
 - best-of-`num_beam` chunks of `beam_width` tokens with temperature sampling and the
   <end> probability zeroed (generate_images.py:256-345)           -> mode "generate";
 - plain ancestral sampling with the <end> -> 0 hack (the periodic sample inside
   train_quantized_transformer.py:581-656)                          -> mode "train".
The encoder half runs ONCE per stage (its input is constant across decode steps; the
reference recomputes it on every call).  Two samplers: the default, "fused", draws inside
the sampling kernel by inverse CDF from uniforms of the device generator -- the reference's
distribution, NOT its generator stream: a given --seed does not reproduce the reference's
tokens; sampler="torch" calls torch.multinomial on the device generator exactly like the
reference on --device cuda, so there a given --seed reproduces the reference's draw
sequence as long as the logits agree.

Which models generate from the key/value cache (`_cacheable`): those whose head dims all have a cache
kernel -- 4, 8, 16, 32, 64 and 128 by default; the other multiples of 4 up to 124 (the head dims the
training path zero-pads) with `cache_padded_heads` (opt-in); any other head dim re-evaluates the
window for every token like the reference.

top_k / top_p (off by default; the reference has neither) filter the probabilities of
every draw, on every path by the one definition of `filter_probs`: zeroing only, kept
entries keep their values.

Reference quirks kept on purpose (drop-in behaviour):
 - "generate" numbers the appended window positions cur_len + tok + 1 (position 1 is
   never used: 0, 2, 3, ...), "train" numbers them 0, 1, 2, ...;
 - "generate" loops while len < total_seq, so beam_width must divide total_seq."""
import dataclasses
import os
import weakref

import torch

from . import ops
from .kvcache import DecodeCache, WindowStep, check_decode_weights, window_pad


def filter_probs(probs, top_k=0, top_p=1.0):
    """Top-k and nucleus (top-p) filtering of probability rows (..., V), non-negative entries, on any device.
    Only zeroes entries:
      top_k (int, 0 = off): the top_k largest non-zero entries stay, ties at the cut going to the lower index;
        top_k >= the number of non-zero entries changes nothing;
      top_p (float in (0, 1], 1.0 = off), on what top_k left: with q = probs / sum(probs) in descending order
        (ties: lower index first), an entry stays iff the q-mass strictly in front of it is < top_p; at least
        one entry stays.
    Kept entries keep their values -- no renormalisation: torch.multinomial and the sampling kernel's
    inverse-CDF draw normalise by the row total themselves, and the probability product of a chunk keeps the
    model's own likelihood.  Both off: returns `probs` itself."""
    top_k, top_p = ops.check_sample_filter(top_k, top_p)
    if top_k == 0 and top_p == 1.0:
        return probs
    V = probs.shape[-1]
    out = probs
    if 0 < top_k < V:
        # a stable sort keeps equal entries in index order
        srt, idx = torch.sort(out, dim=-1, descending=True, stable=True)
        keep = (torch.arange(V, device=probs.device) < top_k) & (srt > 0)
        keep = torch.zeros_like(keep).scatter_(-1, idx, keep)
        out = torch.where(keep, out, torch.zeros_like(out))
    if top_p < 1.0:
        srt, idx = torch.sort(out, dim=-1, descending=True, stable=True)
        q = srt / srt.sum(dim=-1, keepdim=True)
        before = torch.cumsum(q, dim=-1) - q
        keep = (before < top_p) & (srt > 0)
        keep[..., 0] = srt[..., 0] > 0
        keep = torch.zeros_like(keep).scatter_(-1, idx, keep)
        out = torch.where(keep, out, torch.zeros_like(out))
    return out


@dataclasses.dataclass(frozen=True)
class _Stage:
    """What is constant over one generate_tokens call (built there once): its arguments and what follows from them.
    stop_len: the loops run while the sequence is shorter; pos_off: the position numbering (`_positions`);
    pos_bound: exclusive bound of the positions the loops can reach; limit: the decode cache's rows (`_cache_limit`)."""
    temperature: float
    end_token: int
    shift: int
    num_beam: int
    beam_width: int
    mode: str
    use_sliding_window: bool
    sliding_window: int
    total_seq: int
    stop_len: int
    pos_off: int
    pos_bound: int
    limit: int
    top_k: int
    top_p: float
    decode_weights: str
    progress: object
    batch_beams: bool

    def prefix_pos(self, tokens):
        """The `pos_cond` values (N, S) of the sequences `tokens` (N, S); None for a stage without a sliding window
        (its model is not position-conditioned)."""
        if not self.use_sliding_window:
            return None
        return _prefix_pos(tokens.shape[0], tokens.shape[1], self.pos_off, tokens.device)


def _sample(logits, st, rows, comb):
    """One sampling draw as the reference makes it; returns (next ids (B,1), comb)."""
    probs = torch.softmax(logits / st.temperature, dim=1)
    if st.mode == "generate":
        probs[:, st.end_token] = 0.0           # <end> removed from consideration
    if st.top_k > 0 or st.top_p < 1.0:
        probs = filter_probs(probs, st.top_k, st.top_p)
    nxt = torch.multinomial(probs, 1)
    comb = comb * probs[rows, nxt.squeeze(1)]
    if st.mode == "train":
        nxt[nxt == st.end_token] = 0           # reference HACK: <end> -> index 0
    return nxt, comb


def _repeat(t, B):
    """Each row of `t` B times, the copies adjacent (the candidates of an image as rows of one batch); None stays."""
    return t if t is None or B == 1 else t.repeat_interleave(B, dim=0)


# Head dims the training path zero-pads (the multiples of 4 up to 124 other than 4 ... 64: ops.DECODE_PADDED_HEAD_DIMS)
# have a cache kernel too, but keep the full-window loop unless asked for: generate_tokens(cache_padded_heads=True),
# generate_images.py --cache-padded-heads, or this module default.
CACHE_PADDED_HEADS = False


def _positions(lo, hi, pos_off):
    """The `pos_cond` values of sequence indices lo .. hi - 1: index 0 gets 0, index L >= 1 gets L + pos_off -- the
    reference appends cur_len + tok + 1 in "generate" (generate_images.py:306-322: position 1 is never used) and
    0, 1, 2, ... in training's sampler.  Every numbering of this module comes from here: a prefix, the decode
    cache's per-position table, the prefill, the value appended behind each drawn token."""
    return [float(L + pos_off) if L else 0.0 for L in range(lo, hi)]


def _prefix_pos(N, S0, pos_off, device):
    """`pos_cond` values (N, S0) of a prefix as the loop would have numbered them had it produced the tokens
    itself (`_positions`)."""
    return torch.tensor(_positions(0, S0, pos_off), device=device)[None].expand(N, -1).contiguous()


def _reach(stop_len, beam_width):
    """Exclusive bound of the tokens a sequence reaches: the loops overshoot stop_len by up to beam_width - 1
    tokens (the reference's `while len < total`)."""
    return stop_len + beam_width


def _cache_limit(hr_input, total_seq, use_sliding_window, sliding_window, beam_width, mode):
    """Rows of the decode cache of a stage (_generate_fused / _generate_cached: the tokens the loop reaches,
    overshoot included, or the window)."""
    # with the overshoot in, the last chunk of a sequence shorter than the window is cached like the others,
    # instead of falling to the full-window loop (whose ragged row counts run the guarded GEMM kernels: 14 % of a
    # 3-stage cascade)
    cap = _reach(total_seq if mode == "generate" else hr_input.shape[1] + total_seq, beam_width)
    return min(cap, sliding_window) if use_sliding_window else cap


def _cacheable(model, hr_input, use_sliding_window, cache_padded_heads=None, beam_width=None, limit=None):
    """limit, beam_width: the cache's rows and the chunk length -- a prefix of S0 > 1 tokens generates from the
    cache when at least one cached chunk fits behind it (S0 + beam_width <= limit); without them only S0 == 1."""
    S0 = hr_input.shape[1]
    if S0 > 1 and (limit is None or beam_width is None or S0 + beam_width > limit):
        return False
    if not (S0 >= 1 and hasattr(model, "decoder_layers")
            and bool(model.use_pos_cond) == bool(use_sliding_window)
            and all(l.self_attn_block.self_attn.use_masked_attn for l in model.decoder_layers)):
        return False
    # every attention of the model, cross-attention included, needs a cache kernel: ops.DECODE_HEAD_DIMS by default
    # (4 ... 64 and 128); the head dims that run zero-padded in QF.attention (the other multiples of 4 up to 124) only
    # with cache_padded_heads; anything else (d % 4 != 0: decode_rows and the kernels' 16-B row loads need the multiple
    # of 4; d > 128) keeps the full-window loop
    if cache_padded_heads is None:
        cache_padded_heads = CACHE_PADDED_HEADS
    dims = ops.DECODE_HEAD_DIMS + (ops.DECODE_PADDED_HEAD_DIMS if cache_padded_heads else ())
    return all(m.head_dim in dims for m in model.modules() if hasattr(m, "head_dim"))


# Which sampler the cached loop uses: "fused" (default) draws inside the captured graphs
# (csrc/decode.hip qarig_decode_sample: inverse CDF from uniforms of the device generator, ONE generator call
# per stage; the whole chunk search stays on the device), "torch" makes one torch.multinomial call per token as
# the reference does on --device cuda (same generator stream as the reference for a given seed, ~8 extra
# launches and a graph boundary per token).  QARIG_SAMPLER overrides the default.
DEFAULT_SAMPLER = "fused"
ORDERED_ROWS = 512       # images x candidates the reference-order search runs as rows of one batch (0: one by one)
DECODE_ROWS = 16         # rows the single-token kernels take (csrc/decode.hip); more rows run the general kernels
GROUP_BELOW_ROWS = 64    # fused sampler: 16 < images x candidates < 64 is generated in groups of 16 rows (measured:
                         # 16 images x 4 candidates in groups 0.47 s per 256-token stage, 25 x 4 = 100 rows as one
                         # batch on the general kernels 0.51 s -- from about 64 rows up one batch is the faster form)
GROUP_IMAGES = True

# Test hook of the fused sampler: {"forced": (draws, rows) int64 tensor or None, "log": bool}; after a stage
# "probs" holds the (draws, rows, V) probability rows it sampled from and "draws" their number.
FUSED_DEBUG = None


class _Timer:
    """QARIG_GEN_TIMING=1: wall time of the phases of a stage on stderr (synchronises; diagnosis only)."""

    def __init__(self):
        self.on = os.environ.get("QARIG_GEN_TIMING") == "1"
        self.marks = []
        if self.on:
            import time
            torch.cuda.synchronize()
            self.clock, self.t = time.perf_counter, time.perf_counter()

    def mark(self, name):
        if self.on:
            torch.cuda.synchronize()
            t = self.clock()
            self.marks.append(f"{name} {(t - self.t) * 1e3:.2f} ms")
            self.t = t

    def report(self):
        if self.on:
            import sys
            print("[qarig generate] " + ", ".join(self.marks), file=sys.stderr)


# Decode caches kept per model between generations (a process that generates more than once with the same
# weights: a server, a CLI run over several batches): what a cache holds beyond the sequence itself -- the
# per-position table of the conditioning projections, the stacked weights, the captured step graph, the search's
# buffers -- depends on the weights, the batch and the window only.  Keyed by the model object and the state of
# every parameter (data pointer, torch's version counter, the owning FlatAdam's step count) plus ops.LP_EPOCH,
# which every write into a flat parameter buffer bumps; a write into the weights that none of those sees
# (p.data arithmetic) needs decode_cache_clear().
# Window steps (kvcache.WindowStep: the slid window's evaluation as one captured graph, generate_tokens(
# window_graph=True)) are kept the same way: the step holds projections of the weights too (conditioning table,
# cross-attention k / v).
_DECODE_CACHES = {}
DECODE_CACHE_SLOTS = 8
_WINDOW_STEPS = {}
WINDOW_STEP_SLOTS = 4


def decode_cache_clear():
    _DECODE_CACHES.clear()
    _WINDOW_STEPS.clear()


def _weights_key(model):
    # ops.LP_EPOCH: every write into a flat parameter buffer that none of the per-parameter entries sees
    # (parallel.broadcast_params, FlatAdam.ema_weights' swap) bumps it
    key = [ops.LP_EPOCH]
    for p in model.parameters():
        owner = getattr(p, "_qarig_owner", None)
        key.append((p.data_ptr(), p._version, owner.step_count if owner is not None else -1))
    return tuple(key)


def _kept(store, slots, model, enc, shape, build):
    """The object `store` keeps for `model` and `shape` (plus the encoder memory's shape), re-bound to `enc`, when
    the model's weights have not changed since it was built; `build()` otherwise.  Either way it becomes the
    store's youngest entry (model weakref, weights' state, object); the oldest leaves beyond `slots` entries."""
    slot = (id(model), None if enc is None else tuple(enc.shape)) + shape
    wkey = _weights_key(model)
    hit = store.pop(slot, None)
    if hit is not None and hit[0]() is model and hit[1] == wkey and hit[2].rebind(enc):
        kept = hit[2]
    else:
        kept = build()
    if len(store) >= slots:
        store.pop(next(iter(store)))
    store[slot] = (weakref.ref(model), wkey, kept)
    return kept


def decode_cache(model, enc, batch, limit, positions, weights="f32"):
    """A DecodeCache(model, enc, batch, limit, positions=positions, weights=weights) -- a kept one re-bound to
    `enc` when the model's weights have not changed since it was built, a new one otherwise."""
    return _kept(_DECODE_CACHES, DECODE_CACHE_SLOTS, model, enc,
                 (batch, limit, None if positions is None else tuple(positions), weights),
                 lambda: DecodeCache(model, enc, batch, limit, graph=False, positions=positions, weights=weights))


def window_step(model, enc, rows, window, capacity, pos_bound, pos_off, weights="f32"):
    """A WindowStep for these shapes -- a kept one re-bound to `enc` when the weights have not changed since it
    was built, a new one otherwise."""
    return _kept(_WINDOW_STEPS, WINDOW_STEP_SLOTS, model, enc, (rows, window, capacity, pos_bound, pos_off, weights),
                 lambda: WindowStep(model, enc, rows, window, capacity, pos_bound, pos_off, weights=weights))


def _window_graph_fits(model, cache, hr_input, st):
    """The window step applies to this tail: a Transformer whose evaluation rows (images x candidates) and
    self-attention heads fit the window kernels, and an evaluation of the tail slides the window."""
    s = cache._search
    if s is None or not hasattr(model, "_cond"):
        return False
    heads = model.decoder_layers[-1].self_attn_block.self_attn.heads
    if s.N * s.NB > DECODE_ROWS or not ops.window_step_supported(s.N * s.NB, st.sliding_window, cache.dim, heads):
        return False
    cur = hr_input.shape[1]
    chunks = max(0, -(-(st.stop_len - cur) // st.beam_width))
    return chunks > 0 and cur + chunks * st.beam_width - 1 >= st.sliding_window


def _replay_step(cache, ids, index):
    """Logits of the token `ids` at window index `index`, which the decode cache still holds the rows in front of:
    a replay of the search's step graph (the tails' evaluations that come before the window slides)."""
    s = cache._search
    s.ids.copy_(ids)
    cache.ctl[0:1].fill_(index)
    s.g_step.replay()
    return s.logits


def _replays_below(cache, st):
    """Sequences shorter than this draw their next token from a replay of the cache's step graph (`_replay_step`):
    the last token's row fits the cache, and with a sliding window the evaluation does not slide it yet."""
    return min(cache.max_len + 1, st.sliding_window) if st.use_sliding_window else cache.max_len + 1


def _decide(cache, last):
    """Behind a candidate chunk of a tail: the decide kernel keeps it if it beats the kept one; behind the `last`
    candidate the search moves on to the next chunk position."""
    s = cache._search
    ops.decode_decide(cache.ctl, s.N, s.NB, s.bw, s.comb, s.chunk, s.best_p, s.best_chunk, s.take, draws=s.per_set)
    if last:
        ops.decode_advance(cache.ctl, s.bw)
        s.used += s.candidates * s.per_set


def _window_tail(model, cache, hr_input, enc, st):
    """_fused_tail with the slid evaluations replayed from a WindowStep's graph: the same draws, decisions and
    draw numbers (every launch of the search is the one _fused_tail enqueues), the tokens in the step's device
    ring instead of host-side torch.cat.  Evaluations that still fit the window replay the cache's step graph as
    there.  Enqueues only; nothing is read back."""
    s = cache._search
    N, NB, bw = s.N, s.NB, s.bw
    step = window_step(model, _repeat(enc, NB), N * NB, st.sliding_window, _reach(st.stop_len, bw), st.pos_bound,
                       st.pos_off, weights=cache.weights)
    step.load(_repeat(hr_input, NB))
    cur, replays = hr_input.shape[1], _replays_below(cache, st)
    while cur < st.stop_len:
        for c in range(s.candidates):
            step.rewind(cur)
            for tok in range(bw):
                n = cur + tok                    # tokens in the sequence; the next one is drawn from the last's logits
                if n < replays:
                    logits = _replay_step(cache, step.ring[:, n - 1], n - 1)
                else:
                    logits = step.evaluate()
                cache._draw(tok, logits, False)
                step.append(s.ids)
            _decide(cache, c == s.candidates - 1)
        step.ring.view(N, NB, -1)[:, :, cur:cur + bw].copy_(s.best_chunk[:, None, :])     # the kept chunk
        cur += bw
        if st.progress is not None:
            st.progress(cur - 1, st.total_seq)
    return step.ring[::NB, :cur].clone()


def _generate_fused(model, hr_input, enc, st):
    """The cached search with sampling, candidate bookkeeping and the decoder steps replayed from
    captured graphs (kvcache.DecodeCache.begin_search); nothing is read back before the stage ends.
    Returns (hr_input, pos, cache), or None when the model does not fit the fused kernels; the cache (rows of
    the kept tokens but the last) serves the evaluations of the next chunk that come before the window slides.
    top_k / top_p go to the search state (begin_search): _fused_tail and _window_tail draw with them too.
    st.decode_weights: the cache's `weights` mode (kvcache.DECODE_WEIGHTS)."""
    N, bw = hr_input.shape[0], st.beam_width
    # The candidate chunks of a position are independent given the kept prefix: they run as rows of one batch
    # either way.  Without --batch-beams every draw keeps the number the reference's candidate loop gives it
    # (begin_search reference_order: same draws -> same tokens as one candidate after the other); ORDERED_ROWS = 0
    # runs the candidates literally one after the other (tests, A/B).
    ordered = not st.batch_beams and st.num_beam > 1 and N * st.num_beam <= ORDERED_ROWS
    B = st.num_beam if (st.batch_beams or ordered) and st.num_beam > 1 else 1
    cur = hr_input.shape[1]
    chunks = 0
    while cur + chunks * bw < st.stop_len and cur + (chunks + 1) * bw <= st.limit:
        chunks += 1
    if chunks == 0:
        return hr_input, st.prefix_pos(hr_input), None
    positions = _positions(0, st.limit, st.pos_off) if st.use_sliding_window else None
    tm = _Timer()
    cache = decode_cache(model, _repeat(enc, B), N * B, st.limit, positions, st.decode_weights)
    if cache.dim % 4 or (model.use_pos_cond and cache._table is None):
        return None
    tm.mark("cache")
    dbg = FUSED_DEBUG or {}
    after = cur + chunks * bw                              # tokens (first included) once the cached chunks are in
    tail_chunks = max(0, -(-(st.stop_len - after) // bw))               # chunks _fused_tail draws for
    # a prefix of cur > 1 tokens: its first cur - 1 rows are prefilled, the search starts at window index cur
    cache.begin_search(hr_input[:, 0] if cur == 1 else hr_input, N, B, bw, st.temperature, st.end_token, st.shift,
                       st.mode == "generate", chunks + tail_chunks, 1 if B > 1 else st.num_beam,
                       forced=dbg.get("forced"), log_probs=bool(dbg.get("log")), reference_order=ordered,
                       top_k=st.top_k, top_p=st.top_p)
    tm.mark("capture")
    for c in range(chunks):
        cache.run_chunk(last=c == chunks - 1)
        if st.progress is not None:
            st.progress(cur + (c + 1) * bw - 1, st.total_seq)
    hr_input = cache.finish_search()
    tm.mark(f"{chunks} chunks")
    tm.report()
    return hr_input, st.prefix_pos(hr_input), cache


class _Window:
    """The sequences of one candidate in a loop that evaluates the whole window: tokens (rows, n), the `pos_cond`
    value of every token still in the window (None for a stage without a sliding window) and the index the
    window starts at."""

    __slots__ = ("tokens", "pos", "start", "window", "pos_off")

    def __init__(self, st, tokens, pos, start):
        self.tokens, self.pos, self.start, self.pos_off = tokens, pos, start, st.pos_off
        self.window = st.sliding_window if st.use_sliding_window else None

    def slide(self):
        """In front of an evaluation: a full window drops its oldest token (generate_images.py:275-286)."""
        if self.window is not None and self.tokens.shape[1] >= self.window:
            self.start += 1
            self.pos = self.pos[:, 1:]

    def view(self):
        """(tokens, positions) of the window as the model evaluates it."""
        return self.tokens[:, self.start:], self.pos

    def append(self, ids):
        """ids (rows, 1) join the sequences under the loop's position numbering (`_positions`)."""
        n = self.tokens.shape[1]
        self.tokens = torch.cat((self.tokens, ids), dim=1)
        if self.window is not None:
            value = _positions(n, n + 1, self.pos_off)[0]
            self.pos = torch.cat((self.pos, torch.full((ids.shape[0], 1), value, device=ids.device)), dim=1)


def _decode_window(model, tokens, pos, enc, st):
    """Logits (rows, S, V) of a window: the reference's full-window evaluation."""
    # the loop's positions are whole numbers (cur + tok + pos_off): as int64 the model evaluates the
    # conditioning path once per POSITION instead of once per token (Transformer._cond; same values)
    if pos is None or not hasattr(model, "_cond"):
        return model.decode(tokens.contiguous(), enc, pos)
    return model.decode(tokens.contiguous(), enc, pos.long(), pos_bound=st.pos_bound)


def _fused_tail(model, cache, hr_input, pos, enc, st):
    """The chunks behind the cached ones (the window slides inside them: every evaluation from there on is the
    reference's full-window evaluation, generate_images.py:275-286) on the state of the fused search: the candidates
    stay rows of one batch, every draw is made by the sampling kernel from the search's uniforms under the
    reference's draw numbers, the kept chunk is chosen by the decide kernel.  Evaluations that still fit the
    window (the chunk in which it starts to slide: all but its last) are replays of the cache's step graph.
    Enqueues only; nothing is read back."""
    s = cache._search
    NB = s.NB
    enc_eval = _repeat(enc, NB)
    start, replays = 0, _replays_below(cache, st)
    while hr_input.shape[1] < st.stop_len:
        for c in range(s.candidates):
            w = _Window(st, _repeat(hr_input, NB), _repeat(pos, NB), start)
            for tok in range(s.bw):
                w.slide()
                n = w.tokens.shape[1]
                if n < replays:
                    logits = _replay_step(cache, w.tokens[:, -1], n - 1)
                else:
                    win, wpos = w.view()
                    pad = window_pad(win.shape[0], win.shape[1])
                    if pad:             # the logits wanted are then those of the last token but one
                        win = torch.cat((win, win[:, -1:]), dim=1)
                        wpos = None if wpos is None else torch.cat((wpos, wpos[:, -1:]), dim=1)
                    logits = _decode_window(model, win, wpos, enc_eval, st)[:, -2 if pad else -1, :]
                cache._draw(tok, logits, False)
                w.append(s.ids[:, None])
            _decide(cache, c == s.candidates - 1)
        hr_input = torch.cat((hr_input, s.best_chunk), dim=1)
        start, pos = w.start, w.pos if w.pos is None else w.pos[::NB]
        if st.progress is not None:
            st.progress(hr_input.shape[1] - 1, st.total_seq)
    return hr_input


def _generate_cached(model, hr_input, enc, st):
    """The same search as `_generate_window`, evaluating one token per model call from a
    `DecodeCache` for as long as no evaluation of the next chunk would slide the window.
    Sampling draws are made in the reference's order (same shapes, same generator), so the
    sequential variant reproduces the full-window loop whenever the logits round alike.
    Returns (hr_input, pos) for the windowed loops to continue from."""
    device = hr_input.device
    N, bw = hr_input.shape[0], st.beam_width
    B = st.num_beam if st.batch_beams and st.num_beam > 1 else 1
    cur = hr_input.shape[1]
    if cur + bw > st.limit:
        return hr_input, st.prefix_pos(hr_input)
    cache = DecodeCache(model, _repeat(enc, B), N * B, st.limit, weights=st.decode_weights)
    rows = torch.arange(N * B, device=device)

    def position(index):
        """(N * B,) `pos_cond` of the token at sequence index `index`."""
        if not st.use_sliding_window:
            return None
        return torch.full((N * B,), _positions(index, index + 1, st.pos_off)[0], device=device)

    # a prefix: rows [0, cur - 1) are prefilled, its last token is the first step (from scratch: token 0 at index 0)
    if cur > 1:
        cache.prefill(hr_input[:, :cur - 1], pos=_positions(0, cur - 1, st.pos_off))
    last = cache.step(hr_input[:, cur - 1].repeat_interleave(B), position(cur - 1), cur - 1)
    while cur < st.stop_len and cur + bw <= st.limit:
        best_chunk = best_p = best_rows = None
        for _ in range(1 if B > 1 else st.num_beam):
            comb = torch.ones(N * B, device=device)
            logits, new = last, []
            for tok in range(bw):
                nxt, comb = _sample(logits, st, rows, comb)
                new.append(nxt + st.shift)
                if tok < bw - 1:
                    logits = cache.step(new[-1].squeeze(1), position(cur + tok), cur + tok)
            chunk = torch.cat(new, dim=1)
            if B > 1 or st.num_beam == 1:
                best_chunk, best_p = chunk, comb
                continue
            saved = cache.rows(cur, cur + bw - 1).clone() if bw > 1 else None
            if best_p is None:
                best_chunk, best_p, best_rows = chunk, comb, saved
            else:   # per sample, keep the candidate chunk with the larger probability product
                keep = best_p >= comb
                best_p = torch.where(keep, best_p, comb)
                best_chunk = torch.where(keep[:, None], best_chunk, chunk)
                if saved is not None:
                    best_rows = torch.where(keep[None, None, :, None, None, None], best_rows, saved)
        if B > 1:       # first beam with the maximal product wins, as in _generate_window
            pick = torch.arange(N, device=device) * B + best_p.view(N, B).argmax(dim=1)
            best_chunk = best_chunk[pick]
            if bw > 1:
                r = cache.rows(cur, cur + bw - 1)
                r.copy_(r[:, :, pick].repeat_interleave(B, dim=2))
        elif best_rows is not None:
            cache.rows(cur, cur + bw - 1).copy_(best_rows)
        hr_input = torch.cat((hr_input, best_chunk.long()), dim=1)
        cur += bw
        if st.progress is not None:
            st.progress(cur - 1, st.total_seq)
        if cur < st.stop_len and cur + bw <= st.limit:     # another cached chunk follows
            last = cache.step(best_chunk[:, -1].repeat_interleave(B), position(cur - 1), cur - 1)
    return hr_input, st.prefix_pos(hr_input)


def _generate_window(model, hr_input, pos, enc, st):
    """The search with every token drawn from an evaluation of the whole window, as the reference runs it
    (generate_images.py:256-345).  Without --batch-beams the `num_beam` candidate chunks of a position run one
    after the other, each drawing on its own N rows.  With it (additive option) they are ONE batch of N*num_beam
    sequences per model call, the beams of an image adjacent: 1/num_beam of the model calls; the device generator
    is consumed in a different order, so samples differ from the sequential candidates for a given seed."""
    device = hr_input.device
    N = hr_input.shape[0]
    B = st.num_beam if st.batch_beams and st.num_beam > 1 else 1
    enc_eval = _repeat(enc, B)
    rows = torch.arange(N * B, device=device)
    start = 0
    while hr_input.shape[1] < st.stop_len:
        best_in = best_p = None
        for _ in range(1 if B > 1 else st.num_beam):
            comb = torch.ones(N * B, device=device)
            w = _Window(st, _repeat(hr_input, B), _repeat(pos, B), start)
            for tok in range(st.beam_width):
                w.slide()
                logits = _decode_window(model, *w.view(), enc_eval, st)[:, -1, :]
                nxt, comb = _sample(logits, st, rows, comb)
                w.append(nxt + st.shift)
            if best_p is None:
                best_in, best_p = w.tokens, comb
            else:  # keep, per sample, the candidate chunk with the larger probability product
                keep = best_p >= comb
                best_p = torch.where(keep, best_p, comb)
                best_in = torch.where(keep[:, None], best_in, w.tokens)
        if B > 1:   # first beam with the maximal product wins (sequential candidates keep the earlier one on ties)
            best_in = best_in[torch.arange(N, device=device) * B + best_p.view(N, B).argmax(dim=1)]
        hr_input = best_in.long()
        start, pos = w.start, w.pos if w.pos is None else w.pos[::B]
        if st.progress is not None:
            st.progress(hr_input.shape[1] - 1, st.total_seq)
    return hr_input


@torch.no_grad()
def generate_tokens(model, hr_input, lr_input, total_seq, temperature, use_sliding_window,
                    sliding_window, end_token, shift=0, num_beam=1, beam_width=1, mode="generate",
                    progress=None, batch_beams=False, use_kv_cache=True, sampler=None, window_graph=False,
                    top_k=0, top_p=1.0, decode_weights="f32", cache_padded_heads=None):
    """hr_input: (N, S0) int64 conditioning/start tokens, S0 >= 1.  Returns the extended (N, S) tensor
    (first tokens included; callers strip them and undo `shift`).
    S0 > 1 is a prefix (the start token and S0 - 1 tokens already in the `shift`ed numbering the loop appends):
    the run behaves as a from-scratch run interrupted behind it -- the token at index L >= 1 has position
    L + pos_off (1 in "generate", 0 in "train"), index 0 has position 0.  It generates from the key/value cache
    when one cached chunk fits behind it (S0 + beam_width <= the cache's rows: kvcache.DecodeCache.prefill
    fills the prefix's rows); a longer prefix keeps the full-window loop.  A prefix at or past the sliding
    window (S0 >= sliding_window with use_sliding_window) is out of scope: the loop slides by one token per
    draw and would evaluate a window longer than the model was trained on.
    use_kv_cache: evaluate one
    token per step from a key/value cache until the window starts to slide (same logits up
    to fp32 summation order); False re-runs the window for every token like the reference.
    sampler: "fused" / "torch" for the cached loop (DEFAULT_SAMPLER).
    window_graph (opt-in): with the fused sampler, up to DECODE_ROWS rows (images x candidates) and a model the
    window kernels take, every evaluation after the window slides is a replay of one captured graph
    (kvcache.WindowStep) instead of an eager model.decode of the window; other cases ignore it.
    top_k / top_p: every draw is made from filter_probs(probs, top_k, top_p) -- inside the sampling kernel with
    the fused sampler, in front of torch.multinomial elsewhere; 0 / 1.0 (default): off, the code of a call
    without them.
    decode_weights: "f32" (default), or "bf16": the cached single-token steps stream bf16 images of their Linear
    weights (kvcache.DECODE_WEIGHTS: weight-only, everything else fp32; the full-window evaluations are not
    affected).
    cache_padded_heads: True lets a model whose head dims are multiples of 4 up to 124 other than 4 ... 64 (the ones
    the training path zero-pads) generate from the key/value cache like the others, window_graph included; False
    keeps the full-window loop for them; None (default): CACHE_PADDED_HEADS, which is False.  Head dims that are no
    multiple of 4 keep the full-window loop either way."""
    assert mode in ("generate", "train")
    check_decode_weights(decode_weights)
    top_k, top_p = ops.check_sample_filter(top_k, top_p)
    N = hr_input.shape[0]
    fused = (sampler or os.environ.get("QARIG_SAMPLER", DEFAULT_SAMPLER)) == "fused"
    # The single-token kernels behind the fused search take up to 16 rows (images x candidates).  A somewhat
    # larger batch is generated in groups of that many, one after the other through the model's kept decode
    # cache -- each group at the step time of 16 rows; from GROUP_BELOW_ROWS rows up the whole batch on the general
    # kernels is faster (the weights stream once per step for all rows).  The images are independent
    # (generate_images.py:256-345 loops over them only through the batch dimension).
    group = max(1, DECODE_ROWS // max(1, num_beam))
    rows_all = N * max(1, num_beam)
    limit = _cache_limit(hr_input, total_seq, use_sliding_window, sliding_window, beam_width, mode)
    cacheable = use_kv_cache and _cacheable(model, hr_input, use_sliding_window, cache_padded_heads, beam_width, limit)
    if fused and GROUP_IMAGES and N > group and DECODE_ROWS < rows_all < GROUP_BELOW_ROWS and cacheable:
        outs = []
        for g0 in range(0, N, group):
            sub = slice(g0, min(N, g0 + group))
            sub_progress = progress if g0 + group >= N else None
            outs.append(generate_tokens(model, hr_input[sub], None if lr_input is None else lr_input[sub], total_seq,
                                        temperature, use_sliding_window, sliding_window, end_token, shift, num_beam,
                                        beam_width, mode, sub_progress, batch_beams, use_kv_cache, sampler,
                                        window_graph=window_graph, top_k=top_k, top_p=top_p,
                                        decode_weights=decode_weights, cache_padded_heads=cache_padded_heads))
        return torch.cat(outs, dim=0)
    enc = model.encode(lr_input) if model.use_encoder else None
    pos_off = 1 if mode == "generate" else 0
    stop_len = total_seq if mode == "generate" else hr_input.shape[1] + total_seq
    st = _Stage(temperature=temperature, end_token=end_token, shift=shift, num_beam=num_beam, beam_width=beam_width,
                mode=mode, use_sliding_window=use_sliding_window, sliding_window=sliding_window, total_seq=total_seq,
                stop_len=stop_len, pos_off=pos_off, pos_bound=_reach(stop_len, beam_width) + pos_off + 1, limit=limit,
                top_k=top_k, top_p=top_p, decode_weights=decode_weights, progress=progress, batch_beams=batch_beams)
    pos, cache = st.prefix_pos(hr_input), None
    if cacheable:
        done = _generate_fused(model, hr_input, enc, st) if fused else None
        if done is not None:
            hr_input, pos, cache = done
        else:
            hr_input, pos = _generate_cached(model, hr_input, enc, st)

    tail = _Timer()
    if cache is not None and cache._search is not None:
        if window_graph and use_sliding_window and _window_graph_fits(model, cache, hr_input, st):
            hr_input = _window_tail(model, cache, hr_input, enc, st)
            tail.mark("windowed tail (window graph)")
        else:
            hr_input = _fused_tail(model, cache, hr_input, pos, enc, st)
            tail.mark("windowed tail (fused draws)")
        tail.report()
        if FUSED_DEBUG is not None:
            FUSED_DEBUG["probs"] = cache._search.probs
            FUSED_DEBUG["draws"] = cache._search.used
        return hr_input
    hr_input = _generate_window(model, hr_input, pos, enc, st)
    tail.mark("windowed tail (batched beams)" if batch_beams and num_beam > 1 else "windowed tail")
    tail.report()
    return hr_input

