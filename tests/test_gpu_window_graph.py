"""Device-resident evaluation of the slid window (qarig.kvcache.WindowStep, generate_tokens(window_graph=True)):
the window assembly and last-query attention kernels against torch, one evaluation against the eager
`model.decode(window)[:, -1]` (reference generate_images.py:275-290), and whole generations against the
full-window loop under the same draws."""
import pytest
import torch
from conftest import rel_err

pytestmark = pytest.mark.gpu


def _model(use_encoder, heads=8, dim=64, hidden=128, layers=2, vocab=41, pos_cond=True, enc_layers=2):
    from models.Transformer import Transformer
    torch.manual_seed(3)
    m = Transformer(use_encoder=use_encoder, use_pos_cond=pos_cond, num_enc_layers=enc_layers if use_encoder else None,
                    num_dec_layers=layers, num_enc_embedding=vocab if use_encoder else None,
                    num_dec_embedding=vocab, self_attn_heads=heads, cross_attn_heads=heads if use_encoder else None,
                    transformer_in_dim=dim, transformer_out_dim=vocab, transformer_hidden_dim=hidden).cuda().eval()
    with torch.no_grad():       # AdaLN-zero style zero inits would hide the conditioning path
        for p in m.parameters():
            if p.abs().max() == 0:
                p.normal_(0, 0.05)
    return m


def _positions(n, W1, R, pos_off):
    j = torch.arange(n - W1, n, device="cuda")
    return torch.where(j == 0, torch.zeros_like(j), j + pos_off).expand(R, W1)


@pytest.mark.parametrize("R,W1,pad", [(1, 15, False), (4, 31, True), (16, 255, False), (16, 255, True), (3, 7, True)])
def test_window_assembly_matches_torch(R, W1, pad):
    from qarig import ops
    V, D, cap, P = 37, 32, 300, 384
    Wp = W1 + int(pad)
    g = torch.Generator(device="cuda").manual_seed(R * 1000 + W1)
    table = torch.randn(V, D, device="cuda", generator=g)
    pe = torch.randn(Wp, D, device="cuda", generator=g)
    ring = torch.randint(0, V, (R, cap), device="cuda", generator=g)
    ctl = torch.zeros(ops.DECODE_CTL_WORDS, dtype=torch.int32, device="cuda")
    guard = 4096
    xbuf = torch.full((R * Wp * D + guard,), float("nan"), device="cuda")
    x = xbuf[:R * Wp * D].view(R, Wp, D)
    rowmap = torch.empty(R * Wp, dtype=torch.int32, device="cuda")
    last = torch.empty(R, dtype=torch.int32, device="cuda")
    ops._bad_flag(table.device).zero_()
    for n, pos_off in ((W1, 1), (W1 + 1, 0), (cap - 3, 1), (cap, 1)):
        ctl[ops.CTL_RING] = n
        ops.window_assemble(ring, ctl, table, pe, W1, pad, x, rowmap, last, P, pos_off)
        ids = ring[:, n - W1:n]
        pos = _positions(n, W1, R, pos_off)
        if pad:
            ids = torch.cat((ids, ids[:, -1:]), dim=1)
            pos = torch.cat((pos, pos[:, -1:]), dim=1)
        assert torch.equal(x, table[ids] + pe[None])
        assert torch.equal(rowmap.view(R, Wp).long(), pos)
        assert torch.equal(last.long(), pos[:, W1 - 1])
        assert torch.isnan(xbuf[R * Wp * D:]).all()
    ops.check_index_flag(table.device, "window assembly")          # nothing flagged so far

    # an id outside the vocabulary: flagged, zero row, nothing written outside x
    ring[0, cap - 2] = V
    ctl[ops.CTL_RING] = cap
    ops.window_assemble(ring, ctl, table, pe, W1, pad, x, rowmap, last, P, 1)
    with pytest.raises(IndexError):
        ops.check_index_flag(table.device, "window assembly")
    assert not x[0, W1 - 2].any()
    assert torch.isnan(xbuf[R * Wp * D:]).all()
    ring[0, cap - 2] = 0
    # positions past the table, a window start in front of the ring: flagged and clamped
    for n, P_ in ((cap, cap - 10), (W1 - 1, P)):
        ctl[ops.CTL_RING] = n
        ops.window_assemble(ring, ctl, table, pe, W1, pad, x, rowmap, last, P_, 1)
        with pytest.raises(IndexError):
            ops.check_index_flag(table.device, "window assembly")
        assert int(rowmap.max()) < P_ and int(rowmap.min()) >= 0
        assert torch.isnan(xbuf[R * Wp * D:]).all()


@pytest.mark.parametrize("d", [8, 16, 64])
@pytest.mark.parametrize("W", [15, 255, 256])
@pytest.mark.parametrize("R", [1, 4, 16])
def test_window_attention_matches_fp64(d, W, R):
    from qarig import ops
    H = 4
    D = H * d
    g = torch.Generator(device="cuda").manual_seed(d * 7 + W + R)
    n_keys = W - 1 if W % 2 == 0 else W        # even windows: a pad row behind the keys
    rows = W
    q = torch.randn(R, D, device="cuda", generator=g)
    k = torch.randn(R, rows, D, device="cuda", generator=g)
    v = torch.randn(R, rows, D, device="cuda", generator=g)
    got = ops.window_attention(q, k, v, n_keys, H)
    qh = q.double().view(R, H, 1, d)
    kh = k[:, :n_keys].double().view(R, n_keys, H, d).transpose(1, 2)
    vh = v[:, :n_keys].double().view(R, n_keys, H, d).transpose(1, 2)
    want = torch.softmax(qh @ kh.transpose(-1, -2) / d ** 0.5, dim=-1) @ vh
    assert rel_err(got, want.reshape(R, D).float()) < 1e-5
    if n_keys < rows:                           # the pad row does not take part
        k[:, n_keys:] = 1e4
        v[:, n_keys:] = float("nan")
        assert torch.equal(ops.window_attention(q, k, v, n_keys, H), got)
    mul = torch.randn(R, D, device="cuda", generator=g)
    assert rel_err(ops.window_attention(q, k, v, n_keys, H, o_mul=mul), got * mul) < 1e-5


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("pos_cond", [False, True])
@pytest.mark.parametrize("use_encoder", [False, True])
@pytest.mark.parametrize("R", [3, 8])
def test_window_step_matches_eager_decode(use_encoder, pos_cond, wide, graph, R):
    from qarig.kvcache import WindowStep
    m = _model(use_encoder, heads=32, dim=256, hidden=512, pos_cond=pos_cond) if wide else \
        _model(use_encoder, pos_cond=pos_cond)
    W, n, pos_off = 16, 30, 1
    g = torch.Generator(device="cuda").manual_seed(R)
    tokens = torch.randint(0, 41, (R, n), device="cuda", generator=g)
    with torch.no_grad():
        enc = m.encode(torch.randint(0, 41, (R, 7), device="cuda", generator=g)) if use_encoder else None
        step = WindowStep(m, enc, R, W, 40, pos_bound=44, pos_off=pos_off, graph=graph)
        assert step.pad == (R == 8)             # 8 x 15 rows + 8 pad rows = one 128-row tile
        for cur in (W - 1, 22, n):
            step.load(tokens[:, :cur])
            win = tokens[:, cur - (W - 1):cur].contiguous()
            pos = _positions(cur, W - 1, R, pos_off).contiguous() if pos_cond else None
            want = m.decode(win, enc, pos, pos_bound=44)[:, -1]
            got = step.evaluate()
            assert rel_err(got, want) < 1e-5, cur
        # the ring grows on the device: append + evaluate again
        step.load(tokens[:, :n - 1])
        step.append(tokens[:, n - 1].contiguous())
        assert rel_err(step.evaluate(), want) < 1e-5


def _count_window_evals(monkeypatch):
    from qarig.kvcache import WindowStep
    calls = {"n": 0}
    real = WindowStep.evaluate

    def counted(self):
        calls["n"] += 1
        return real(self)
    monkeypatch.setattr(WindowStep, "evaluate", counted)
    return calls


@pytest.mark.parametrize("use_encoder,num_beam,bw,batch_beams,wide", [
    (False, 1, 1, False, False), (False, 3, 4, False, False), (True, 2, 4, False, False),
    (True, 3, 2, True, False), (False, 2, 4, True, False), (True, 2, 4, False, True),
    (True, 3, 2, True, True)])
def test_window_graph_generation_matches_full_window_loop(use_encoder, num_beam, bw, batch_beams, wide, monkeypatch):
    """Sequences of ~4 windows: the full-window loop's draws are forced into the fused sampler running on the
    window graph; the probability row of every draw and the tokens must agree."""
    from conftest import DrawTape
    from qarig import sampling
    m = _model(use_encoder, heads=32, dim=256, hidden=512) if wide else _model(use_encoder)
    with torch.no_grad():
        m.classifier[1].linear_layer[0].bias[40] -= 20.0     # <end> out of the way
    N, total, sw = 3, 60, 16
    g = torch.Generator().manual_seed(4)
    lr_in = torch.randint(0, 40, (N, 6), generator=g).cuda() if use_encoder else None
    first = torch.randint(0, 40, (N, 1), generator=g).cuda()

    def run(cached):
        torch.manual_seed(11)
        return sampling.generate_tokens(m, first, lr_in, total, 0.05, True, sw, end_token=40, num_beam=num_beam,
                                        beam_width=bw, mode="generate", batch_beams=batch_beams,
                                        use_kv_cache=cached, sampler="fused", window_graph=cached)
    tape = DrawTape(monkeypatch, tol=2e-5)
    want = tape.record(lambda: run(False))
    calls = _count_window_evals(monkeypatch)
    got = tape.replay(0, lambda: run(True))
    assert tape.fused_draws > 0 and calls["n"] > 0
    assert want.shape[1] >= total
    assert torch.equal(want, got)


def test_readme_dim_stage_window_graph_matches_fused_tail(monkeypatch):
    """A configs[3]-type stage at README width that slides: window 256, 320 tokens, 4 images, beam 4 x 4 --
    16 rows of 255 tokens, the pad row included -- window graph against the eager tail, the same forced draws."""
    from qarig import sampling
    K = 512
    m = _model(True, heads=64, dim=512, hidden=2048, layers=7, vocab=K + 1, enc_layers=5)
    N, total = 4, 320
    g = torch.Generator().manual_seed(9)
    lr_in = torch.randint(0, K, (N, 64), generator=g).cuda()
    first = torch.full((N, 1), K, dtype=torch.int64, device="cuda")
    forced = torch.randint(0, K, (2048, N), generator=g)

    def run(window_graph):
        sampling.FUSED_DEBUG = {"forced": forced}
        try:
            torch.manual_seed(2)
            return sampling.generate_tokens(m, first, lr_in, total, 1.0, True, 256, end_token=K, num_beam=4,
                                            beam_width=4, mode="generate", sampler="fused", window_graph=window_graph)
        finally:
            sampling.FUSED_DEBUG = None
    want = run(False)
    calls = _count_window_evals(monkeypatch)
    got = run(True)
    assert calls["n"] > 0
    assert torch.equal(want, got)


@pytest.mark.parametrize("case", ["head_dim_12", "rows_68"])
def test_window_graph_falls_back_outside_its_scope(case):
    from qarig import sampling
    if case == "head_dim_12":
        m, N = _model(False, heads=4, dim=48), 3
    else:
        m, N = _model(False), 17                 # 17 images x 4 candidates: one batch on the general kernels
    sampling.decode_cache_clear()
    g = torch.Generator().manual_seed(6)
    first = torch.randint(0, 40, (N, 1), generator=g).cuda()

    def run(window_graph):
        torch.manual_seed(8)
        return sampling.generate_tokens(m, first, None, 40, 0.7, True, 16, end_token=40, num_beam=4, beam_width=4,
                                        mode="generate", sampler="fused", window_graph=window_graph)
    want = run(False)
    got = run(True)
    assert torch.equal(want, got)
    assert not sampling._WINDOW_STEPS


@pytest.mark.parametrize("write", ["optimiser", "broadcast"])
def test_kept_window_step_follows_the_weights(write):
    from qarig import parallel, sampling
    m = _model(True)
    R, W, n = 4, 16, 25
    g = torch.Generator(device="cuda").manual_seed(12)
    tokens = torch.randint(0, 41, (R, n), device="cuda", generator=g)
    lr = torch.randint(0, 41, (R, 6), device="cuda", generator=g)
    pos = _positions(n, W - 1, R, 1).contiguous()
    sampling.decode_cache_clear()

    def both():
        with torch.no_grad():
            enc = m.encode(lr)
            step = sampling.window_step(m, enc, R, W, 40, 44, 1)
            step.load(tokens)
            return step, step.evaluate().clone(), m.decode(tokens[:, n - W + 1:].contiguous(), enc, pos,
                                                           pos_bound=44)[:, -1]
    step0, got, want = both()
    assert rel_err(got, want) < 1e-5
    assert both()[0] is step0                    # same weights: the kept step is handed out again
    if write == "optimiser":
        opt = torch.optim.SGD(m.parameters(), lr=0.5)
        for p in m.parameters():
            p.grad = torch.randn_like(p) * 0.05
        opt.step()
    else:   # a write behind torch's version counters, declared by the broadcast of the parameters
        with torch.no_grad():
            for p in m.parameters():
                p.data.add_(torch.randn_like(p) * 0.05)
        parallel.broadcast_params(torch.zeros(1, device="cuda"))
    step1, got1, want1 = both()
    assert step1 is not step0
    assert rel_err(want1, want) > 1e-3           # the weights did change the logits
    assert rel_err(got1, want1) < 1e-5
    sampling.decode_cache_clear()
