"""Weight-only bf16 for the cached decode step: qarig_decode_linear_bf16w (csrc/decode.hip) streams a row-major
(N, K) bf16 image of the weight and widens it exactly, so it computes the fp32 kernel's function on
Wr = W.to(torch.bfloat16).float() -- the tolerances are the fp32 kernel's own (tests/test_gpu_decode.py,
tests/test_gpu_kvcache.py).  Kernel alone first (fp64, the fp32 kernel, the layout bit for bit, rejections), then
the decode step and generation through it (DecodeCache(weights="bf16"), generate_tokens(decode_weights="bf16"))."""
import warnings

import pytest
import torch

from conftest import rel_err
from test_gpu_decode import _ref
from test_gpu_kvcache import _model

pytestmark = pytest.mark.gpu

# one shape per launcher branch (rows <= 4: the all-rows kernel, else the row-split kernel; K = 256 on 8-B loads;
# 1 / 2 / 4 / 8 chunks per lane; 4 / 2 / 1 load passes by workgroup count; ragged N; groups).  K > 1024 has no
# LayerNorm form (qarig_decode_linear_supported): only "none" runs there.
_SHAPES = [(4, 1, 8, 256), (3, 1, 513, 256), (12, 1, 600, 256), (4, 3, 2048, 512), (9, 1, 512, 512), (2, 2, 77, 1024),
           (13, 1, 1030, 1024), (1, 1, 513, 2048), (16, 3, 512, 2048), (16, 1, 40, 2048), (5, 2, 40, 4096)]
_FORMS = ["none", "affine", "adaln", "adaln_row"]
_CASES = [(*s, f) for s in _SHAPES for f in (_FORMS if s[3] <= 1024 else _FORMS[:1])]


def _data(M, G, N, K, form, seed):
    """tests/test_gpu_decode.py's operands, drawn in its order."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn((M, K), generator=g) * 1.5 + 0.3).cuda()
    W = (torch.randn((G, N, K), generator=g) * 0.05).cuda()
    b = torch.randn((G, N), generator=g).cuda()
    gam, bet = torch.randn(K, generator=g).cuda(), torch.randn(K, generator=g).cuda()
    rows = (K,) if form == "adaln_row" else (M, K)
    sc, sh = torch.randn(rows, generator=g).cuda(), torch.randn(rows, generator=g).cuda()
    kw = {"none": {}, "affine": dict(gamma=gam, beta=bet), "adaln": dict(scale=sc, shift=sh),
          "adaln_row": dict(scale=sc, shift=sh)}[form]
    return g, x, W, b, gam, bet, sc, sh, kw


@pytest.mark.parametrize("M,G,N,K,form", _CASES)
def test_bf16w_linear_vs_fp64_on_rounded_weights(M, G, N, K, form):
    from qarig import ops
    assert ops.decode_linear_supported(M, N, K, form != "none")
    g, x, W, b, gam, bet, sc, sh, kw = _data(M, G, N, K, form, M * 131 + N + K)
    Wr = W.to(torch.bfloat16)
    Wf = Wr.float()
    f = "adaln" if form == "adaln_row" else form
    got = ops.decode_linear(x, Wr, b, act=1, **kw)
    assert got.shape == (G, M, N) and got.dtype == torch.float32
    err = rel_err(got, _ref(x, Wf, b, f, gam, bet, sc, sh, None, None, 1))
    print(f"fp64 on rounded weights: {err:.2e}")
    assert err < 5e-6
    if form == "none":      # the bf16 image was read, not the fp32 weight: the rounding is in the result
        gap = rel_err(got, _ref(x, W, b, f, gam, bet, sc, sh, None, None, 1))
        print(f"fp64 on unrounded weights: {gap:.2e}")
        assert gap > 1e-4
    if G == 1:
        res = torch.randn((M, N), generator=g).cuda()
        for mul in (torch.randn((M, N), generator=g).cuda(), torch.randn(N, generator=g).cuda()):
            got = ops.decode_linear(x, Wr[0], b[0], act=1, residual=res, mul=mul, **kw)
            assert got.shape == (M, N)
            assert rel_err(got, _ref(x, Wf, b, f, gam, bet, sc, sh, res, mul, 1)[0]) < 5e-6
        got = ops.decode_linear(x, Wr[0], None, act=0, **kw)
        assert rel_err(got, _ref(x, Wf, None, f, gam, bet, sc, sh, None, None, 0)[0]) < 5e-6
    else:
        xg = torch.randn((G, M, K), generator=g).cuda()
        if form == "none":
            got = ops.decode_linear(xg, Wr, b, act=1)
            assert rel_err(got, _ref(xg, Wf, b, "none", None, None, None, None, None, None, 1)) < 5e-6
    a = ops.decode_linear(x, Wr, b, act=1, **kw)
    assert torch.equal(a, ops.decode_linear(x, Wr, b, act=1, **kw)), "not run-to-run reproducible"


@pytest.mark.parametrize("M,G,N,K", [(16, 3, 2048, 512), (4, 1, 512, 2048), (9, 1, 512, 512)])
def test_bf16w_linear_vs_f32_kernel_on_rounded_weights(M, G, N, K):
    """Same function as the fp32 kernel fed Wr.float(), to the project's kernel-against-kernel bound (the two
    split K over the lanes differently: summation order)."""
    from qarig import ops
    g, x, W, b, gam, bet, sc, sh, _ = _data(M, G, N, K, "adaln_row", M + N + K)
    Wr = W.to(torch.bfloat16)
    Wf = Wr.float()
    pairs = [(ops.decode_linear(x, Wr, b, act=1), ops.decode_linear(x, Wf, b, act=1))]
    if K <= 1024:
        pairs.append((ops.decode_linear(x, Wr, b, act=1, scale=sc, shift=sh),
                      ops.decode_linear(x, Wf, b, act=1, scale=sc, shift=sh)))
        pairs.append((ops.decode_linear(x, Wr, b, act=1, gamma=gam, beta=bet),
                      ops.decode_linear(x, Wf, b, act=1, gamma=gam, beta=bet)))
    if G == 1:
        res, mul = torch.randn((M, N), generator=g).cuda(), torch.randn(N, generator=g).cuda()
        pairs.append((ops.decode_linear(x, Wr[0], b[0], act=1, residual=res, mul=mul),
                      ops.decode_linear(x, Wf[0], b[0], act=1, residual=res, mul=mul)))
    for got, want in pairs:
        err = rel_err(got, want)
        print(f"against the fp32 kernel: {err:.2e}")
        assert err < 2e-6


def _bit_pattern_weight(N, K, seed):
    """(N, K) bf16 from random 16-bit patterns, Inf / NaN patterns made finite, rows 0-3 cycling through
    +-largest finite, +-smallest subnormal, +-0 and 1.0."""
    g = torch.Generator().manual_seed(seed)
    bits = torch.randint(0, 65536, (N, K), generator=g, dtype=torch.int32)
    bits = torch.where((bits & 0x7F80) == 0x7F80, bits & ~0x0080, bits)
    special = torch.tensor([0x7F7F, 0xFF7F, 0x0001, 0x8001, 0x0000, 0x8000, 0x3F80], dtype=torch.int32)
    for r in range(4):
        bits[r] = special[(torch.arange(K) + r) % len(special)]
    bits = torch.where(bits >= 32768, bits - 65536, bits).to(torch.int16)
    return bits.view(torch.bfloat16).cuda()


@pytest.mark.parametrize("M", [16, 4])
@pytest.mark.parametrize("K", [256, 512, 1024, 2048, 4096])
def test_bf16w_layout_is_exact(M, K):
    """Every weight of the image lands on its own k: one-hot activation rows walk all k, and the outputs must be
    the image's values as numbers -- extreme finite values, subnormals and signed zeros included (the widening is a
    shift / a mask; products with 0 and 1 and sums with 0 are exact).  M = 16: the row-split kernel; 4: all rows."""
    from qarig import ops
    N = 24
    Wr = _bit_pattern_weight(N, K, K + M)
    assert torch.isfinite(Wr.float()).all()
    eye = torch.eye(K, device="cuda")
    out = torch.full((K, N), float("nan"), device="cuda")
    for k0 in range(0, K, M):
        ops.decode_linear(eye[k0:k0 + M], Wr, out=out[k0:k0 + M])
    assert torch.equal(out, Wr.float().T)


def test_bf16w_rejects_what_it_cannot_run():
    from qarig import ops, _lib
    W = torch.randn(8, 512).cuda().to(torch.bfloat16)
    with pytest.raises(RuntimeError, match="M <= 16"):
        ops.decode_linear(torch.randn(17, 512).cuda(), W)
    with pytest.raises(RuntimeError, match="M <= 16"):
        ops.decode_linear(torch.randn(4, 768).cuda(), torch.randn(8, 768).cuda().to(torch.bfloat16))
    with pytest.raises(RuntimeError, match="M <= 16"):
        ops.decode_linear(torch.randn(4, 2048).cuda(), torch.randn(8, 2048).cuda().to(torch.bfloat16),
                          gamma=torch.ones(2048).cuda(), beta=torch.ones(2048).cuda())
    x = torch.randn(4, 512).cuda()
    C = torch.empty(4, 8).cuda()
    lib = _lib.load()

    def call(Wp, ldw):
        ops.check(lib.qarig_decode_linear_bf16w(x.data_ptr(), 512, 0, 1e-5, None, None, None, None, 0, Wp, ldw, 0, None,
                                                0, None, 0, None, 0, C.data_ptr(), 8, 0, 1, 4, 8, 512, 0, ops.stream()),
                  "qarig_decode_linear_bf16w")
    big = torch.zeros(8, 516).cuda().to(torch.bfloat16)
    call(W.data_ptr(), 512)                                     # the call itself is fine
    with pytest.raises(RuntimeError, match="16-B aligned"):
        call(big.data_ptr(), 516)                               # a view whose row stride is no multiple of 8
    with pytest.raises(RuntimeError, match="16-B aligned"):
        call(big.data_ptr() + 2, 520)                           # W offset by one element
    torch.cuda.synchronize()


def _round_weights(m):
    """Every >= 2-D parameter to its bf16 value, in place: the fp32 model then computes on the weights the bf16
    step streams (embedding rows and conditioning weights are read in fp32 by both)."""
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() >= 2:
                p.copy_(p.to(torch.bfloat16).float())
    return m


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("use_encoder", [False, True])
def test_bf16w_step_matches_full_window_on_rounded_weights(use_encoder, graph):
    from qarig.kvcache import DecodeCache
    m = _round_weights(_model(use_encoder, heads=32, dim=256, hidden=512))
    B, S = 3, 12
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(0, 41, (B, S), generator=g).cuda()
    pos = torch.rand(B, S, generator=g).cuda() * 20
    with torch.no_grad():
        enc = m.encode(torch.randint(0, 41, (B, 7), generator=g).cuda()) if use_encoder else None
        cache = DecodeCache(m, enc, B, S, graph=graph, weights="bf16")
        assert cache._img is not None and cache.weights == "bf16"
        worst = 0.0
        for t in range(S):
            got = cache.step(ids[:, t], pos[:, t], t)
            want = m.decode(ids[:, :t + 1].contiguous(), enc, pos[:, :t + 1].contiguous())[:, -1]
            worst = max(worst, rel_err(got, want))
            assert rel_err(got, want) < 1e-5, t
        print(f"step against the full window: {worst:.2e}")


@pytest.mark.parametrize("use_encoder", [False, True])
def test_bf16w_step_routes_every_linear_to_the_bf16_kernel(use_encoder, monkeypatch):
    """After construction nothing of a step may reach a GEMM entry or a cast: every Linear group of the step --
    stacked q/k/v MLPs, cross-attention q MLP, FFN, the residual Linears, classifier -- calls ops.decode_linear
    with a bf16 image that existed before the step."""
    from models.layers import _lin_params
    from qarig import ops
    from qarig.kvcache import DecodeCache
    m = _round_weights(_model(use_encoder, heads=32, dim=256, hidden=512))
    B, S = 3, 12
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(0, 41, (B, S), generator=g).cuda()
    with torch.no_grad():
        enc = m.encode(torch.randint(0, 41, (B, 7), generator=g).cuda()) if use_encoder else None
        cache = DecodeCache(m, enc, B, S, graph=False, positions=[float(i) for i in range(S)], weights="bf16")
        assert cache._img is not None and cache._table is not None
        group = {}
        for li, layer in enumerate(m.decoder_layers):
            group[cache._qkv_lp[li][0].data_ptr()] = group[cache._qkv_lp[li][2].data_ptr()] = "qkv"
            named = [("ffn", layer.feedforward_block.feedforward)]
            res = [layer.self_attn_block.self_attn_res, layer.feedforward_block.feedforward_res]
            if layer.use_cross_attn:
                named.append(("cross_q", layer.cross_attn_block.cross_attn.q_block))
                res.append(layer.cross_attn_block.cross_attn_res)
            for name, seq in named:
                for lin in (seq[0], seq[1]):
                    group[cache._img[id(_lin_params(lin)[0])].data_ptr()] = name
            for r in res:
                group[cache._img[id(_lin_params(r.linear)[0])].data_ptr()] = "residual"
        for lin in (m.classifier[0], m.classifier[1]):
            group[cache._img[id(_lin_params(lin)[0])].data_ptr()] = "classifier"

        def refuse(name):
            def f(*a, **k):
                raise AssertionError(f"ops.{name} called inside a bf16-weight step")
            return f
        for name in ("gemm", "gemm_grouped_skinny", "gemm_skinny_ln", "cast_bf16", "cast_transpose_bf16"):
            monkeypatch.setattr(ops, name, refuse(name))
        real, seen = ops.decode_linear, []

        def spy(x, W, *a, **k):
            seen.append((W.dtype, group.get(W.data_ptr())))
            return real(x, W, *a, **k)
        monkeypatch.setattr(ops, "decode_linear", spy)
        logits = cache.step(ids[:, 0], None, 0)
        assert logits.shape == (B, 41) and torch.isfinite(logits).all()
    assert seen and all(dt == torch.bfloat16 for dt, _ in seen)
    want = {"qkv", "ffn", "residual", "classifier"} | ({"cross_q"} if use_encoder else set())
    assert {name for _, name in seen} == want
    layers = len(m.decoder_layers)
    assert sum(name == "residual" for _, name in seen) == (3 if use_encoder else 2) * layers


def test_bf16w_generation_emits_the_full_window_tokens(monkeypatch):
    """test_cached_generation_matches_full_window_loop's case (True, 2, 4, False, True), fused sampler: the
    full-window fp32 run's draws forced into the cached run with bf16 step weights; on pre-rounded weights every
    probability row must equal the recorded one within the tape's tolerance and the tokens must be the same."""
    from conftest import DrawTape
    from qarig import sampling
    m = _round_weights(_model(True, heads=32, dim=256, hidden=512))
    with torch.no_grad():
        m.classifier[1].linear_layer[0].bias[40] -= 20.0
    N, total, sw = 3, 24, 16
    g = torch.Generator().manual_seed(4)
    lr_in = torch.randint(0, 40, (N, 6), generator=g).cuda()
    first = torch.randint(0, 40, (N, 1), generator=g).cuda()

    def run(cached):
        torch.manual_seed(11)
        return sampling.generate_tokens(m, first, lr_in, total, 0.05, True, sw, end_token=40, num_beam=2, beam_width=4,
                                        mode="generate", batch_beams=False, use_kv_cache=cached, sampler="fused",
                                        decode_weights="bf16" if cached else "f32")
    sampling.decode_cache_clear()
    tape = DrawTape(monkeypatch, tol=2e-5)
    outs = [tape.record(lambda: run(False)), tape.replay(0, lambda: run(True))]
    print(f"worst probability difference: {tape.worst:.2e}")
    assert tape.fused_draws > 0
    caches = [hit[2] for hit in sampling._DECODE_CACHES.values()]
    assert len(caches) == 1 and caches[0].weights == "bf16" and caches[0]._img is not None
    assert outs[0].shape[1] >= total
    assert torch.equal(outs[0], outs[1])
    sampling.decode_cache_clear()


def test_f32_default_is_untouched_and_kept_caches_are_keyed_by_mode():
    from qarig import sampling
    from qarig.kvcache import DecodeCache
    m = _model(True, heads=32, dim=256, hidden=512)
    with torch.no_grad():
        m.classifier[1].linear_layer[0].bias[40] -= 20.0
    B, S = 3, 6
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(0, 40, (B, S), generator=g).cuda()
    pos = torch.rand(B, S, generator=g).cuda() * 20
    lr_in = torch.randint(0, 40, (B, 6), generator=g).cuda()
    with torch.no_grad():
        enc = m.encode(lr_in)
        plain = DecodeCache(m, enc, B, S, graph=False)
        named = DecodeCache(m, enc, B, S, graph=False, weights="f32")
        lp = DecodeCache(m, enc, B, S, graph=False, weights="bf16")
        assert plain.weights == "f32" and plain._img is None and named._img is None and lp._img is not None
        differs = False
        for t in range(S):
            a = plain.step(ids[:, t], pos[:, t], t)
            assert torch.equal(a, named.step(ids[:, t], pos[:, t], t))
            differs = differs or not torch.equal(a, lp.step(ids[:, t], pos[:, t], t))
        assert differs                       # unrounded weights: the bf16 step is a different computation
    first = ids[:, :1].contiguous()

    def run(mode):
        torch.manual_seed(5)
        return sampling.generate_tokens(m, first, lr_in, 24, 0.7, True, 16, end_token=40, num_beam=2, beam_width=4,
                                        mode="generate", use_kv_cache=True, sampler="fused", decode_weights=mode)
    sampling.decode_cache_clear()
    a, _, c = run("f32"), run("bf16"), run("f32")
    assert torch.equal(a, c)
    modes = sorted(hit[2].weights for hit in sampling._DECODE_CACHES.values())
    assert modes == ["bf16", "f32"]
    torch.manual_seed(5)
    assert torch.equal(a, sampling.generate_tokens(m, first, lr_in, 24, 0.7, True, 16, end_token=40, num_beam=2,
                                                   beam_width=4, mode="generate", use_kv_cache=True, sampler="fused"))
    sampling.decode_cache_clear()


def test_bf16w_request_on_a_model_the_kernel_does_not_take_warns_once_and_stays_fp32(monkeypatch):
    from qarig import kvcache
    m = _model(False)                        # width 64: no streaming kernel
    B, S = 3, 4
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(0, 41, (B, S), generator=g).cuda()
    pos = torch.rand(B, S, generator=g).cuda() * 20
    monkeypatch.setattr(kvcache, "_WEIGHTS_WARNED", False)
    with torch.no_grad():
        plain = kvcache.DecodeCache(m, None, B, S, graph=False)
        with pytest.warns(UserWarning, match="keeping fp32 weights"):
            lp = kvcache.DecodeCache(m, None, B, S, graph=False, weights="bf16")
        with warnings.catch_warnings():
            warnings.filterwarnings("error", message=".*keeping fp32 weights.*")       # once per process
            kvcache.DecodeCache(m, None, B, S, graph=False, weights="bf16")
        assert lp._img is None
        for t in range(S):
            assert torch.equal(plain.step(ids[:, t], pos[:, t], t), lp.step(ids[:, t], pos[:, t], t))
    with pytest.raises(ValueError, match="decode weights"):
        kvcache.DecodeCache(m, None, B, S, graph=False, weights="fp16")


@pytest.mark.parametrize("graph", [False, True])
def test_bf16w_window_step_matches_eager_decode_on_rounded_weights(graph):
    """WindowStep(weights="bf16"): the last layer's q MLP and the classifier on the bf16 kernel; on pre-rounded
    weights the logits are the eager decoder's within test_window_step_matches_eager_decode's bound."""
    from qarig.kvcache import WindowStep
    m = _round_weights(_model(True, heads=32, dim=256, hidden=512))
    R, W, n, pos_off = 3, 16, 30, 1
    g = torch.Generator(device="cuda").manual_seed(R)
    tokens = torch.randint(0, 41, (R, n), device="cuda", generator=g)
    with torch.no_grad():
        enc = m.encode(torch.randint(0, 41, (R, 7), device="cuda", generator=g))
        step = WindowStep(m, enc, R, W, 40, pos_bound=44, pos_off=pos_off, graph=graph, weights="bf16")
        assert step._img is not None
        for cur in (W - 1, n):
            step.load(tokens[:, :cur])
            win = tokens[:, cur - (W - 1):cur].contiguous()
            j = torch.arange(cur - (W - 1), cur, device="cuda")
            pos = torch.where(j == 0, torch.zeros_like(j), j + pos_off).expand(R, W - 1).contiguous()
            want = m.decode(win, enc, pos, pos_bound=44)[:, -1]
            assert rel_err(step.evaluate(), want) < 1e-5, cur
