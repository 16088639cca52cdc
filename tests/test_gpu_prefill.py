"""Generation from a token prefix: `qarig_decode_cache_fill` writes exactly the rows it is given, `DecodeCache.prefill`
(one batched pass over the prefix) leaves the cache a from-scratch run would have built token by token, and a
generation that starts from a prefix is a from-scratch generation interrupted at that point."""
import pytest
import torch

from conftest import rel_err

pytestmark = pytest.mark.gpu


def _model(use_encoder, heads=8, dim=64, hidden=128, layers=2, vocab=41, pos_cond=True):
    """The models of tests/test_gpu_kvcache.py: narrow (per-module launches) by default; heads=32, dim=256,
    hidden=512 is the wide one on which the step stacks its projections."""
    from models.Transformer import Transformer
    torch.manual_seed(3)
    kw = dict(use_encoder=use_encoder, use_pos_cond=pos_cond, num_enc_layers=2 if use_encoder else None,
              num_dec_layers=layers, num_enc_embedding=vocab if use_encoder else None,
              num_dec_embedding=vocab, self_attn_heads=heads,
              cross_attn_heads=heads if use_encoder else None, transformer_in_dim=dim,
              transformer_out_dim=vocab, transformer_hidden_dim=hidden)
    m = Transformer(**kw).cuda().eval()
    with torch.no_grad():       # AdaLN-zero style zero inits would hide the conditioning path
        for p in m.parameters():
            if p.abs().max() == 0:
                p.normal_(0, 0.05)
    return m


@pytest.fixture
def batched(monkeypatch):
    """The batched pass for every prefix length (the constant is a speed threshold, not a correctness one)."""
    from qarig import kvcache
    monkeypatch.setattr(kvcache, "PREFILL_MIN_TOKENS", 0)


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,d", [(3, 4), (3, 8), (2, 64), (2, 128), (5, 96)])       # 5 x 96: the padded-head cache's rows
def test_cache_fill_writes_the_addressed_rows_bit_exactly_and_nothing_else(H, d):
    from qarig import ops
    D, max_len, layers = H * d, 20, 2
    g = torch.Generator().manual_seed(H * 1000 + d)
    for images in (1, 3):
        for beams in (1, 3, 4):
            for P1 in (1, 2, 5, 15, 16, 17, max_len - 1):
                kv = torch.full((layers, 2, images * beams, H, max_len, d), float("nan"), device="cuda")
                # k and v are column sub-views of one wider buffer: row stride 2 * D + 8, not D
                wide = torch.randn((images, P1, 2 * D + 8), generator=g).cuda()
                k, v = wide[:, :, 4:4 + D], wide[:, :, D + 4:2 * D + 4]
                assert k.stride(1) == 2 * D + 8 and k.stride() == v.stride()
                ops.decode_cache_fill(k, v, kv[1], beams)
                what = (images, beams, P1)
                for half, src in ((0, k), (1, v)):
                    want = src.reshape(images, P1, H, d).permute(0, 2, 1, 3).repeat_interleave(beams, dim=0)
                    assert torch.equal(kv[1, half, :, :, :P1], want), what        # every candidate row, bit for bit
                assert torch.isnan(kv[1, :, :, :, P1:]).all(), what               # rows behind the prefix
                assert torch.isnan(kv[0]).all(), what                             # the other layer
    with pytest.raises(IndexError):
        big = torch.zeros((1, max_len + 1, D), device="cuda")
        ops.decode_cache_fill(big, big, torch.zeros((2, 1, H, max_len, d), device="cuda"), 1)


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pos_cond", [True, False])
@pytest.mark.parametrize("use_encoder", [False, True])
@pytest.mark.parametrize("wide", [False, True])
def test_prefill_matches_step_replays_and_the_full_window_model(wide, use_encoder, pos_cond, monkeypatch):
    """Cache rows of one batched pass against the rows P - 1 step replays leave (the replay path is the oracle:
    tests/test_gpu_kvcache.py holds it to the model), then every later step's logits against the full-window
    decoder.  Both bounds are test_decode_cache_step_matches_full_window's.  wide: the stacked, graph-captured step."""
    from qarig import kvcache
    m = _model(use_encoder, heads=32, dim=256, hidden=512, pos_cond=pos_cond) if wide else \
        _model(use_encoder, pos_cond=pos_cond)
    images, beams, S, P = 2, 2, 12, 7
    B = images * beams
    g = torch.Generator().manual_seed(6)
    ids = torch.randint(0, 41, (images, S), generator=g).cuda()
    values = [0.0] + [float(L + 1) for L in range(1, S)]           # "generate" numbering: 0, 2, 3, ...
    pos = torch.tensor(values).cuda()[None].expand(images, -1).contiguous() if pos_cond else None
    with torch.no_grad():
        enc = m.encode(torch.randint(0, 41, (images, 7), generator=g).cuda()) if use_encoder else None
        enc_b = enc.repeat_interleave(beams, dim=0) if use_encoder else None
        caches = {}
        for name, floor in (("batched", 0), ("replayed", 1 << 20)):
            monkeypatch.setattr(kvcache, "PREFILL_MIN_TOKENS", floor)
            c = kvcache.DecodeCache(m, enc_b, B, S, graph=wide, positions=values if pos_cond else None)
            assert c.prefill_batched(P - 1) == (name == "batched")
            c.prefill(ids[:, :P - 1])
            caches[name] = c
        got, want = caches["batched"].kv, caches["replayed"].kv
        err = rel_err(got[:, :, :, :, :P - 1], want[:, :, :, :, :P - 1])
        print(f"cache rows, batched pass against replays: rel_err {err:.2e}")
        assert err < 1e-5
        assert not got[:, :, :, :, P - 1:].any()                    # nothing behind the prefix was written
        assert torch.equal(got[:, :, 0::beams], got[:, :, 1::beams])      # every candidate row holds the image's rows
        cache = caches["batched"]
        for t in range(P - 1, S):
            logits = cache.step(ids[:, t].repeat_interleave(beams), None, t)
            ref = m.decode(ids[:, :t + 1].contiguous(), enc, None if pos is None else pos[:, :t + 1].contiguous())[:, -1]
            err = rel_err(logits, ref.repeat_interleave(beams, dim=0))
            print(f"step {t}: logits against the full window rel_err {err:.2e}")
            assert err < 1e-5, t


def test_prefill_falls_back_to_step_replays(batched):
    """bf16 step weights, a position-conditioned cache without its table and a prefix below the threshold keep the
    replays; the replays of a table-less cache take the positions they are given."""
    from qarig import kvcache
    m = _model(False)
    ids = torch.randint(0, 41, (2, 6), generator=torch.Generator().manual_seed(1)).cuda()
    values = [0.0] + [float(L + 1) for L in range(1, 8)]
    with torch.no_grad():
        tabled = kvcache.DecodeCache(m, None, 2, 8, graph=False, positions=values)
        bare = kvcache.DecodeCache(m, None, 2, 8, graph=False)
        assert tabled.prefill_batched(5) and not bare.prefill_batched(5) and not tabled.prefill_batched(0)
        assert not kvcache.DecodeCache(m, None, 2, 8, graph=False, positions=values, weights="bf16").prefill_batched(5)
        tabled.prefill(ids[:, :5])
        bare.prefill(ids[:, :5], pos=values)
        assert rel_err(bare.kv, tabled.kv) < 1e-5
        with pytest.raises(IndexError):
            tabled.prefill(torch.zeros((2, 9), dtype=torch.int64, device="cuda"))
        with pytest.raises(ValueError):
            tabled.prefill(torch.zeros((3, 2), dtype=torch.int64, device="cuda"))


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampler", ["torch", "fused"])
@pytest.mark.parametrize("P", [2, 5, "sw - bw"])
@pytest.mark.parametrize("use_encoder,num_beam,bw,batch_beams,wide", [
    (False, 3, 4, False, False), (True, 2, 4, True, False), (True, 3, 2, False, True)])
def test_cached_generation_from_a_prefix_matches_full_window_loop(use_encoder, num_beam, bw, batch_beams, wide, P,
                                                                  sampler, monkeypatch, batched):
    """tests/test_gpu_kvcache.py::test_cached_generation_matches_full_window_loop with `first` of shape (N, P): the
    full-window loop numbers the prefix's positions 0, 2, 3, ...; the cached loop prefills P - 1 rows and must emit
    that loop's tokens -- sampler "torch" under the same seed, "fused" with the full-window run's draws forced and
    its probability row matched at every draw."""
    from conftest import DrawTape
    from qarig import sampling
    m = _model(use_encoder, heads=32, dim=256, hidden=512) if wide else _model(use_encoder)
    with torch.no_grad():
        m.classifier[1].linear_layer[0].bias[40] -= 20.0     # <end> out of the way
    N, total, sw = 3, 24, 16
    P = sw - bw if P == "sw - bw" else P
    g = torch.Generator().manual_seed(4)
    lr_in = torch.randint(0, 40, (N, 6), generator=g).cuda() if use_encoder else None
    first = torch.randint(0, 40, (N, P), generator=g).cuda()

    def run(cached):
        torch.manual_seed(11)
        return sampling.generate_tokens(m, first, lr_in, total, 0.05, True, sw, end_token=40,
                                        num_beam=num_beam, beam_width=bw, mode="generate",
                                        batch_beams=batch_beams, use_kv_cache=cached, sampler=sampler)
    try:
        if sampler == "torch":
            outs = [run(False), run(True)]
        else:
            tape = DrawTape(monkeypatch, tol=2e-5)
            outs = [tape.record(lambda: run(False)), tape.replay(0, lambda: run(True))]
            assert tape.fused_draws > 0
    finally:
        sampling.decode_cache_clear()
    assert outs[0].shape[1] >= total and torch.equal(outs[0][:, :P], first)
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("use_encoder", [False, True])
def test_cached_generation_from_a_prefix_without_position_conditioning(use_encoder, batched):
    """No sliding window: the whole stage is cached, and the torch sampler's cache (built without a position table)
    prefills in one batched pass."""
    from qarig import sampling
    m = _model(use_encoder, pos_cond=False)
    with torch.no_grad():
        m.classifier[1].linear_layer[0].bias[40] -= 20.0
    g = torch.Generator().manual_seed(14)
    lr_in = torch.randint(0, 40, (3, 6), generator=g).cuda() if use_encoder else None
    first = torch.randint(0, 40, (3, 6), generator=g).cuda()
    outs = []
    for cached in (False, True):
        torch.manual_seed(2)
        outs.append(sampling.generate_tokens(m, first, lr_in, 20, 0.05, False, None, end_token=40, num_beam=2,
                                             beam_width=4, mode="generate", use_kv_cache=cached, sampler="torch"))
    assert outs[0].shape == (3, 22) and torch.equal(outs[0], outs[1])


# ---------------------------------------------------------------------------------------------------------------------
def _fused_run(m, first, lr_in, forced, sw, num_beam, bw, batch_beams):
    """(tokens, probability row of every draw made) of a fused run whose draws are `forced`."""
    from qarig import sampling
    sampling.FUSED_DEBUG = {"forced": forced, "log": True}
    try:
        torch.manual_seed(3)
        toks = sampling.generate_tokens(m, first, lr_in, 24, 0.7, True, sw, end_token=40, num_beam=num_beam,
                                        beam_width=bw, mode="generate", batch_beams=batch_beams, sampler="fused")
        dbg = sampling.FUSED_DEBUG
        return toks, dbg["probs"][:dbg["draws"]].clone()
    finally:
        sampling.FUSED_DEBUG = None


@pytest.mark.parametrize("num_beam,batch_beams,sw", [(2, False, 32), (3, True, 32), (2, True, 16), (3, False, 16)])
def test_run_from_a_prefix_continues_an_interrupted_run(num_beam, batch_beams, sw, batched):
    """A fused run from one token with forced draws gives T and its probability rows; a second run from
    T[:, :1 + c * bw] with the remaining draws must emit the rest of T exactly and sample from the same rows
    (DrawTape's tolerance).  sw = 16: the tail of both runs slides the window (24 tokens)."""
    from qarig import sampling
    m = _model(True)
    with torch.no_grad():
        m.classifier[1].linear_layer[0].bias[40] -= 20.0
    N, bw, c = 3, 4, 2
    g = torch.Generator().manual_seed(17)
    lr_in = torch.randint(0, 40, (N, 6), generator=g).cuda()
    first = torch.randint(0, 40, (N, 1), generator=g).cuda()
    cols = N * num_beam if batch_beams else N               # draw rows: one column per cache row / per image
    per_chunk = bw if batch_beams else num_beam * bw        # draw rows one chunk position consumes
    forced = torch.randint(0, 40, (7 * per_chunk, cols), generator=g)
    try:
        T, rows = _fused_run(m, first, lr_in, forced, sw, num_beam, bw, batch_beams)
        assert T.shape == (N, 25) and rows.shape[0] == 6 * per_chunk
        T2, rows2 = _fused_run(m, T[:, :1 + c * bw].contiguous(), lr_in, forced[c * per_chunk:], sw, num_beam, bw,
                               batch_beams)
    finally:
        sampling.decode_cache_clear()
    assert torch.equal(T2, T)
    assert rows2.shape[0] == (6 - c) * per_chunk
    err = float((rows2 - rows[c * per_chunk:]).abs().max())
    print(f"probability rows of the resumed run against the uninterrupted one: max abs err {err:.2e}")
    assert err < 2e-5


def test_one_token_prefix_is_todays_start():
    """begin_search with (N,) ids and with an (N, 1) prefix: identical tokens and probability rows."""
    from qarig import sampling
    m = _model(True)
    N, NB, bw, limit = 3, 2, 4, 13
    g = torch.Generator().manual_seed(23)
    first = torch.randint(0, 40, (N, 1), generator=g).cuda()
    positions = [0.0] + [float(L + 1) for L in range(1, limit)]
    outs = []
    try:
        with torch.no_grad():
            enc = m.encode(torch.randint(0, 40, (N, 6), generator=g).cuda()).repeat_interleave(NB, dim=0)
            for ids in (first[:, 0], first):
                cache = sampling.decode_cache(m, enc, N * NB, limit, positions)
                gen = torch.Generator(device="cuda").manual_seed(5)
                s = cache.begin_search(ids, N, NB, bw, 0.7, 40, 0, True, 3, 1, log_probs=True, generator=gen)
                for ch in range(3):
                    cache.run_chunk(last=ch == 2)
                outs.append((cache.finish_search(), s.probs.clone()))
    finally:
        sampling.decode_cache_clear()
    assert outs[0][0].shape == (N, 1 + 3 * bw)
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
