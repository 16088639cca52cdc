"""Cached generation for head dim 128 (by default) and for the head dims that train zero-padded (opt-in,
generate_tokens(cache_padded_heads=True)): the checks of test_gpu_kvcache.py, test_gpu_window_graph.py and
test_gpu_decode_bf16w.py on three models whose attention runs on decode_attention_grouped_kernel --
2 heads x 128 (256 wide: the stacked, fused step), 5 heads x 96 (480 wide, opt-in) and 4 heads x 12 (48 wide, opt-in)."""
import warnings

import pytest
import torch

from conftest import rel_err

# name -> (heads, width, hidden, needs cache_padded_heads)
MODELS = {"d128": (2, 256, 512, False), "d96": (5, 480, 128, True), "d12": (4, 48, 96, True)}


def _model(use_encoder, heads, dim, hidden, layers=2, vocab=41, pos_cond=True, device="cuda"):
    from models.Transformer import Transformer
    torch.manual_seed(3)
    kw = dict(use_encoder=use_encoder, use_pos_cond=pos_cond, num_enc_layers=2 if use_encoder else None,
              num_dec_layers=layers, num_enc_embedding=vocab if use_encoder else None,
              num_dec_embedding=vocab, self_attn_heads=heads,
              cross_attn_heads=heads if use_encoder else None, transformer_in_dim=dim,
              transformer_out_dim=vocab, transformer_hidden_dim=hidden)
    m = Transformer(**kw).to(device).eval()
    with torch.no_grad():       # AdaLN-zero style zero inits would hide the conditioning path
        for p in m.parameters():
            if p.abs().max() == 0:
                p.normal_(0, 0.05)
    return m


def _named(name, use_encoder):
    heads, dim, hidden, opt_in = MODELS[name]
    return _model(use_encoder, heads, dim, hidden), opt_in


@pytest.mark.parametrize("use_encoder", [False, True])
def test_which_head_dims_are_cacheable(use_encoder):
    """No device needed: _cacheable looks at the modules' head dims (cross-attention included) alone."""
    from qarig import ops, sampling
    first = torch.zeros((2, 1), dtype=torch.int64)
    cpu = lambda heads, dim: _model(use_encoder, heads, dim, 2 * dim, device="cpu")
    assert 128 in ops.DECODE_HEAD_DIMS and sampling.CACHE_PADDED_HEADS is False
    assert sampling._cacheable(cpu(2, 256), first, True)                         # d = 128: by default
    assert sampling._cacheable(cpu(4, 64), first, True)                          # d = 16: as before
    m12 = cpu(4, 48)
    assert not sampling._cacheable(m12, first, True)                             # d = 12: opt-in
    assert not sampling._cacheable(m12, first, True, cache_padded_heads=False)
    assert sampling._cacheable(m12, first, True, cache_padded_heads=True)
    m96 = cpu(5, 480)
    assert not sampling._cacheable(m96, first, True)
    assert sampling._cacheable(m96, first, True, cache_padded_heads=True)
    assert not sampling._cacheable(cpu(4, 40), first, True, cache_padded_heads=True)     # d = 10: never


@pytest.mark.gpu
@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("use_encoder", [False, True])
@pytest.mark.parametrize("name", list(MODELS))
def test_decode_cache_step_matches_full_window(name, use_encoder, graph):
    """test_gpu_kvcache.py::test_decode_cache_step_matches_full_window, its bound."""
    from qarig.kvcache import DecodeCache
    m, _ = _named(name, use_encoder)
    B, S = 3, 12
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(0, 41, (B, S), generator=g).cuda()
    pos = torch.rand(B, S, generator=g).cuda() * 20
    with torch.no_grad():
        enc = m.encode(torch.randint(0, 41, (B, 7), generator=g).cuda()) if use_encoder else None
        cache = DecodeCache(m, enc, B, S, graph=graph)
        worst = 0.0
        for t in range(S):
            got = cache.step(ids[:, t], pos[:, t], t)
            want = m.decode(ids[:, :t + 1].contiguous(), enc, pos[:, :t + 1].contiguous())[:, -1]
            worst = max(worst, rel_err(got, want))
            assert rel_err(got, want) < 1e-5, t
        print(f"{name}: step against the full window {worst:.2e}")


# test_gpu_kvcache.py::test_cached_generation_matches_full_window_loop's cases (its `wide` pair is the d128 model
# here); "fused-one-by-one" only where it is a path of its own (unbatched beams, more than one candidate)
_SEARCHES = [(False, 1, 1, False), (False, 3, 4, False), (True, 2, 4, False), (True, 3, 2, True), (False, 2, 4, True),
             (True, 4, 4, False)]
_GENERATION_CASES = [(*s, sampler) for s in _SEARCHES for sampler in ("torch", "fused", "fused-one-by-one")
                     if sampler != "fused-one-by-one" or not (s[3] or s[1] == 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("use_encoder,num_beam,bw,batch_beams,sampler", _GENERATION_CASES)
@pytest.mark.parametrize("name", list(MODELS))
def test_cached_generation_matches_full_window_loop(name, use_encoder, num_beam, bw, batch_beams, sampler, monkeypatch):
    """The cached loop (then its windowed continuation once the window slides) must emit the tokens of the
    reference-style full-window loop.  sampler "torch": same seed, same torch.multinomial call order; "fused": the
    full-window run's draws are recorded and forced into the in-graph sampler, whose probability row must equal the
    recorded one at every draw; "fused-one-by-one": the candidates one after the other."""
    from conftest import DrawTape
    from qarig import sampling
    if sampler == "fused-one-by-one":
        monkeypatch.setattr(sampling, "ORDERED_ROWS", 0)
        sampler = "fused"
    m, opt_in = _named(name, use_encoder)
    with torch.no_grad():
        m.classifier[1].linear_layer[0].bias[40] -= 20.0     # <end> out of the way
    N, total, sw = 3, 24, 16
    g = torch.Generator().manual_seed(4)
    lr_in = torch.randint(0, 40, (N, 6), generator=g).cuda() if use_encoder else None
    first = torch.randint(0, 40, (N, 1), generator=g).cuda()
    assert sampling._cacheable(m, first, True, cache_padded_heads=opt_in)
    built = []
    real = sampling.DecodeCache.__init__

    def spy(self, *a, **k):
        built.append(1)
        real(self, *a, **k)
    monkeypatch.setattr(sampling.DecodeCache, "__init__", spy)
    sampling.decode_cache_clear()

    def run(cached):
        torch.manual_seed(11)
        return sampling.generate_tokens(m, first, lr_in, total, 0.05, True, sw, end_token=40,
                                        num_beam=num_beam, beam_width=bw, mode="generate",
                                        batch_beams=batch_beams, use_kv_cache=cached, sampler=sampler,
                                        cache_padded_heads=opt_in)
    if sampler == "torch":
        outs = [run(False), run(True)]
    else:
        tape = DrawTape(monkeypatch, tol=2e-5)
        outs = [tape.record(lambda: run(False)), tape.replay(0, lambda: run(True))]
        assert tape.fused_draws > 0
    assert built, "the cached run built no key/value cache"
    assert outs[0].shape[1] >= total       # the loop overshoots to 1 + k*beam_width
    assert torch.equal(outs[0], outs[1])
    sampling.decode_cache_clear()


def _count_window_evals(monkeypatch):
    from qarig.kvcache import WindowStep
    calls = {"n": 0}
    real = WindowStep.evaluate

    def counted(self):
        calls["n"] += 1
        return real(self)
    monkeypatch.setattr(WindowStep, "evaluate", counted)
    return calls


@pytest.mark.gpu
@pytest.mark.parametrize("use_encoder", [False, True])
@pytest.mark.parametrize("name", ["d128", "d12"])
def test_window_graph_generation_equals_the_eager_tail(name, use_encoder, monkeypatch):
    """~4 windows of 16 tokens, beam 2 x 4: the slid evaluations replayed from the window graph give the tokens of
    window_graph=False, and at least one evaluation was a replay."""
    from qarig import sampling
    m, opt_in = _named(name, use_encoder)
    with torch.no_grad():
        m.classifier[1].linear_layer[0].bias[40] -= 20.0
    N, total, sw = 3, 60, 16
    g = torch.Generator().manual_seed(4)
    lr_in = torch.randint(0, 40, (N, 6), generator=g).cuda() if use_encoder else None
    first = torch.randint(0, 40, (N, 1), generator=g).cuda()
    forced = torch.randint(0, 40, (512, N), generator=g)
    sampling.decode_cache_clear()

    def run(window_graph):
        sampling.FUSED_DEBUG = {"forced": forced}
        try:
            torch.manual_seed(11)
            return sampling.generate_tokens(m, first, lr_in, total, 0.05, True, sw, end_token=40, num_beam=2,
                                            beam_width=4, mode="generate", sampler="fused",
                                            window_graph=window_graph, cache_padded_heads=opt_in)
        finally:
            sampling.FUSED_DEBUG = None
    want = run(False)
    assert not sampling._WINDOW_STEPS
    calls = _count_window_evals(monkeypatch)
    got = run(True)
    assert calls["n"] > 0 and sampling._WINDOW_STEPS
    assert want.shape[1] >= total
    assert torch.equal(want, got)
    sampling.decode_cache_clear()


def _round_weights(m):
    """Every >= 2-D parameter to its bf16 value, in place (test_gpu_decode_bf16w.py)."""
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() >= 2:
                p.copy_(p.to(torch.bfloat16).float())
    return m


@pytest.mark.gpu
@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("use_encoder", [False, True])
def test_bf16_step_weights_at_head_dim_128(use_encoder, graph, monkeypatch):
    """decode_weights="bf16" at 2 heads x 128: the step runs on the streaming kernels (no fallback warning) and its
    logits are those of the fp64 evaluation on the rounded weights -- and of the model's own full-window decode --
    within test_gpu_decode_bf16w.py's bound for the step."""
    from oracle import ref_models as rm
    from qarig import kvcache
    from qarig.kvcache import DecodeCache
    m = _round_weights(_named("d128", use_encoder)[0])
    B, S = 3, 12
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(0, 41, (B, S), generator=g)
    pos = torch.rand(B, S, generator=g) * 20
    lr = torch.randint(0, 41, (B, 7), generator=g)
    sd = {k: v.detach().double().cpu() for k, v in m.state_dict().items()}
    cfg = dict(use_encoder=use_encoder, use_pos_cond=True, num_enc_layers=2, num_dec_layers=2, self_attn_heads=2,
               cross_attn_heads=2, hidden_activation="silu")
    want64 = rm.transformer_forward(sd, cfg, ids, lr if use_encoder else None, pos.double())       # (B, S, V)
    monkeypatch.setattr(kvcache, "_WEIGHTS_WARNED", False)
    ids, pos = ids.cuda(), pos.cuda()
    with torch.no_grad(), warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*keeping fp32 weights.*")
        enc = m.encode(lr.cuda()) if use_encoder else None
        cache = DecodeCache(m, enc, B, S, graph=graph, weights="bf16")
        assert cache._img is not None and cache.weights == "bf16"
        worst = worst64 = 0.0
        for t in range(S):
            got = cache.step(ids[:, t], pos[:, t], t)
            want = m.decode(ids[:, :t + 1].contiguous(), enc, pos[:, :t + 1].contiguous())[:, -1]
            e, e64 = rel_err(got, want), rel_err(got, want64[:, t])
            worst, worst64 = max(worst, e), max(worst64, e64)
            assert e < 1e-5 and e64 < 1e-5, (t, e, e64)
        print(f"bf16 step at d = 128: {worst:.2e} against the full window, {worst64:.2e} against fp64")
