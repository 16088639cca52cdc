"""Top-k / nucleus (top-p) filtering inside the device-resident sampler (csrc/decode.hip
decode_sample_filtered_kernel, qarig_decode_sample_filtered) and through every sampling path of
qarig.sampling.generate_tokens.  The reference is qarig.sampling.filter_probs on the fp64 softmax
(tests/test_sampling_filter_host.py checks that function against a numpy restatement).

Where a comparison of zero patterns could hinge on rounding, the test first asserts a CONDITION ON ITS INPUTS,
in fp64: the cut is at least 1e-4 away from a tie.  The kernel's sums are a thread's <= 65 entries (V <= 16,385)
in index order, a 6-level butterfly over the wave and 4 wave totals: at most 75 roundings of 2^-24 each, 5e-6
of a unit total -- below the 2e-5 of a 257 + 64 term shape, so 1e-4 holds for it as well."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

MARGIN = 1e-4


def _reference(logits, T, end, gen):
    want = torch.softmax(logits.double() / T, dim=1)
    if gen:
        want[:, end] = 0
    return want


def _margins(want, top_k, top_p):
    """fp64, per row: (relative gap between the k-th and the (k + 1)-th largest probability,
    distance of top_p from the mass in front of the last kept / the first dropped token); inf where there is no
    cut (top_k >= the number of non-zero entries; nothing dropped)."""
    from qarig.sampling import filter_probs
    B = want.shape[0]
    inf = torch.full((B,), math.inf, dtype=torch.float64)
    gap_k, gap_p = inf.clone(), inf.clone()
    want = want.cpu()
    for r in range(B):
        row = want[r]
        if top_k > 0:
            s = torch.sort(row, descending=True, stable=True).values
            if top_k < int((s > 0).sum()):
                gap_k[r] = (s[top_k - 1] - s[top_k]) / s[top_k - 1]
            row = filter_probs(row[None], top_k, 1.0)[0]
        if top_p < 1.0:
            s = torch.sort(row, descending=True, stable=True).values
            s = s[s > 0]
            q = s / s.sum()
            before = torch.cumsum(q, 0) - q
            kept = int((before < top_p).sum())
            gap_p[r] = top_p - before[kept - 1]
            if kept < len(s):
                gap_p[r] = min(gap_p[r], before[kept] - top_p)
    return gap_k, gap_p


def _draw(logits, T, end, gen, shift, uniforms, ctl, slot, bw, top_k, top_p, forced=None, inc=False, beams=0,
          comb0=0.5):
    from qarig import ops
    B, V = logits.shape
    cols = B // beams if beams else B
    ids = torch.zeros(B, dtype=torch.int64, device="cuda")
    chunk = torch.full((B, bw), -7, dtype=torch.int64, device="cuda")
    comb = torch.full((B,), comb0, device="cuda")
    probs = torch.zeros((uniforms.shape[0], cols, V), device="cuda")
    ops.decode_sample(logits, T, end, gen, shift, uniforms, ctl, slot, bw, ids, chunk, comb, forced=forced,
                      probs_log=probs, inc_len=inc, beams=beams, top_k=top_k, top_p=top_p)
    return ids, chunk, comb, probs


CASES = [(1, 1.0), (5, 1.0), (64, 1.0), (0, 0.9), (0, 0.5), (50, 0.9), (3, 0.3)]
CASES_16385 = [(1, 1.0), (5, 1.0), (64, 1.0), (0, 0.5), (3, 0.3)]
_INPUTS = {}


def _inputs(V):
    """The inputs of tests/test_gpu_decode.py::test_decode_sample_is_the_references_draw and their fp64
    probabilities, computed once per V."""
    if V not in _INPUTS:
        g = torch.Generator().manual_seed(V)
        B, draws, end, T = 6, 5, V - 1, 0.7
        logits = (torch.randn((B, V), generator=g) * 3).cuda()
        uniforms = torch.rand((draws, B), generator=g).cuda()
        _INPUTS[V] = (logits, uniforms, _reference(logits, T, end, True))
    return _INPUTS[V]


@pytest.mark.parametrize("V,top_k,top_p", [(V, k, p) for V in (3, 41, 513, 8193) for k, p in CASES] +
                         [(16385, k, p) for k, p in CASES_16385])
def test_filtered_draw_against_the_fp64_reference(V, top_k, top_p):
    from qarig import ops
    from qarig.sampling import filter_probs
    logits, uniforms, want = _inputs(V)
    B, bw, end, T, d, slot = 6, 4, V - 1, 0.7, 1, 1
    gap_k, gap_p = _margins(want, top_k, top_p)
    print(f"V={V} top_k={top_k} top_p={top_p}: min margins {float(gap_k.min()):.3e} {float(gap_p.min()):.3e}")
    assert float(gap_k.min()) >= MARGIN and float(gap_p.min()) >= MARGIN, "inputs too close to a tie at the cut"
    ref = filter_probs(want, top_k, top_p)
    ctl = torch.zeros(ops.DECODE_CTL_WORDS, dtype=torch.int32, device="cuda")
    runs = []
    for _ in range(2):
        ctl.zero_()
        ctl[2], ctl[0] = d - slot, 10
        runs.append(_draw(logits, T, end, True, 100, uniforms, ctl, slot, bw, top_k, top_p, inc=True))
        assert int(ctl[0]) == 11 and int(ctl[2]) == d - slot
    ids, chunk, comb, probs = runs[0]
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b), "two launches on the same input differ"
    err = float((probs[d].double() - ref).abs().max())
    print(f"  logged row: max |err| {err:.3e}")
    assert err < 1e-6
    assert torch.equal(probs[d] > 0, ref > 0), "zero pattern differs from filter_probs"
    assert not probs[[i for i in range(probs.shape[0]) if i != d]].any()
    tok = ids - 100
    assert int(tok.min()) >= 0 and int(tok.max()) < V
    assert torch.equal(chunk[:, slot], ids) and (chunk[:, [s for s in range(bw) if s != slot]] == -7).all()
    rows = torch.arange(B, device="cuda")
    assert (ref[rows, tok] > 0).all(), "a filtered-out token was drawn"
    cdf = torch.cumsum(ref, dim=1)
    target = uniforms[d].double() * cdf[:, -1]
    hi = cdf[rows, tok]
    lo = hi - ref[rows, tok]
    assert ((lo - 1e-6 <= target) & (target < hi + 1e-6)).all(), "token outside its CDF interval"
    assert float((comb.double() - 0.5 * want[rows, tok]).abs().max()) < 1e-6       # the UNFILTERED probability


@pytest.mark.parametrize("gen", [True, False])
@pytest.mark.parametrize("V,top_k,top_p", [(41, 5, 1.0), (41, 0, 0.49), (41, 5, 0.49), (600, 400, 1.0),
                                           (600, 0, 0.7007), (1700, 900, 0.5003), (8193, 7000, 0.80007)])
def test_equal_entries_stay_in_index_order(V, top_k, top_p, gen):
    """All-equal rows (the rows of the host test; larger ones whose cut falls in another thread and wave of
    the prefix count): every kept entry is decided by the tie rule alone.  Train mode: <end> is one of them.
    top_p is chosen so that top_p * (entries) is at least 0.09 away from a whole number in both modes (19.6 and
    20.09; 419.7 and 420.4; 450.27; 5600.49): 9e-5 of the total at worst, against 5e-6 of rounding in the kernel's sums."""
    from qarig import ops
    from qarig.sampling import filter_probs
    B, bw, end = 3, 1, V - 1
    logits = torch.zeros((B, V), device="cuda")
    uniforms = torch.tensor([[0.0, 0.5, 0.99999994]], device="cuda")
    ctl = torch.zeros(ops.DECODE_CTL_WORDS, dtype=torch.int32, device="cuda")
    want = _reference(logits, 1.0, end, gen)
    ref = filter_probs(want, top_k, top_p)
    ids, _, comb, probs = _draw(logits, 1.0, end, gen, 0, uniforms, ctl, 0, bw, top_k, top_p)
    kept = int((ref[0] > 0).sum())
    if V == 41:                                   # the host test's figures
        n = V - 1 if gen else V
        expect = {(5, 1.0): 5, (0, 0.49): math.ceil(0.49 * n), (5, 0.49): 3}[(top_k, top_p)]
        assert kept == expect
    assert torch.equal(ref[0] > 0, torch.arange(V, device="cuda") < kept)          # the lowest indices
    assert torch.equal(probs[0] > 0, ref > 0)
    assert float((probs[0].double() - ref).abs().max()) < 1e-6
    # u = 0 draws the first kept entry, u -> 1 the last one
    assert int(ids[0]) == 0 and int(ids[2]) == kept - 1 and 0 <= int(ids[1]) < kept
    assert float((comb.double() - 0.5 * want[0, 0]).abs().max()) < 1e-6


def test_candidate_major_draw_numbers_and_forced_tokens():
    """tests/test_gpu_decode.py::test_decode_sample_candidate_major_draw_numbers with top_k = 5; a forced token
    outside the kept set is taken, and the product takes its filtered probability: 0."""
    from qarig import ops
    from qarig.sampling import filter_probs
    g = torch.Generator().manual_seed(5)
    N, NB, bw, V, end, T, top_k = 3, 4, 4, 41, 40, 0.9, 5
    B, draws = N * NB, 2 * NB * bw
    logits = (torch.randn((B, V), generator=g) * 2).cuda()
    uniforms = torch.rand((draws, N), generator=g).cuda()
    ctl = torch.zeros(ops.DECODE_CTL_WORDS, dtype=torch.int32, device="cuda")
    base, slot = NB * bw, 2
    ctl[2] = base
    want = _reference(logits, T, end, True)
    gap_k, _ = _margins(want, top_k, 1.0)
    print(f"min margin {float(gap_k.min()):.3e}")
    assert float(gap_k.min()) >= MARGIN
    ref = filter_probs(want, top_k, 1.0)
    ids, chunk, comb, probs = _draw(logits, T, end, True, 0, uniforms, ctl, slot, bw, top_k, 1.0, beams=NB, comb0=1.0)
    cdf = torch.cumsum(ref, dim=1)
    used = torch.zeros(draws, dtype=torch.bool)
    for n in range(N):
        for c in range(NB):
            r, d = n * NB + c, base + c * bw + slot
            used[d] = True
            assert float((probs[d, n].double() - ref[r]).abs().max()) < 1e-6
            assert torch.equal(probs[d, n] > 0, ref[r] > 0) and int((probs[d, n] > 0).sum()) == top_k
            target = float(uniforms[d, n].double() * cdf[r, -1])
            tok = int(ids[r])
            assert float(ref[r, tok]) > 0
            assert float(cdf[r, tok] - ref[r, tok]) - 1e-6 <= target < float(cdf[r, tok]) + 1e-6
            assert abs(float(comb[r]) - float(want[r, tok])) < 1e-6
    assert not probs[~used].any()
    # forced entries follow the same numbering; the least probable token of a row is not among its top 5
    low = want.clone()
    low[:, end] = 2.0
    outside = low.argmin(dim=1)
    forced = torch.full((draws, N), -1, dtype=torch.int64, device="cuda")
    for n in range(N):
        for c in range(NB):
            # candidates 0 and 1 are forced out of the kept set, 2 into it, 3 draws
            r = n * NB + c
            forced[base + c * bw + slot, n] = outside[r] if c < 2 else (ref[r].argmax() if c == 2 else -1)
    ids2, _, comb2, _ = _draw(logits, T, end, True, 0, uniforms, ctl, slot, bw, top_k, 1.0, forced=forced, beams=NB,
                              comb0=1.0)
    for n in range(N):
        for c in range(NB):
            r = n * NB + c
            if c < 2:
                assert int(ids2[r]) == int(outside[r]) and float(ref[r, outside[r]]) == 0 and float(comb2[r]) == 0.0
            elif c == 2:
                assert int(ids2[r]) == int(ref[r].argmax()) and abs(float(comb2[r]) - float(want[r].max())) < 1e-6
            else:
                assert int(ids2[r]) == int(ids[r]) and float(comb2[r]) == float(comb[r])


def test_filters_off_is_the_unfiltered_call_and_bad_values_are_refused():
    from qarig import _lib, ops
    V = 513
    logits, uniforms, _ = _inputs(V)
    B, bw, end, T = 6, 4, V - 1, 0.7
    ctl = torch.zeros(ops.DECODE_CTL_WORDS, dtype=torch.int32, device="cuda")
    ctl[2] = 1

    def call(**kw):
        ids = torch.zeros(B, dtype=torch.int64, device="cuda")
        chunk = torch.full((B, bw), -7, dtype=torch.int64, device="cuda")
        comb = torch.full((B,), 0.5, device="cuda")
        probs = torch.zeros((uniforms.shape[0], B, V), device="cuda")
        ops.decode_sample(logits, T, end, True, 3, uniforms, ctl, 2, bw, ids, chunk, comb, probs_log=probs, **kw)
        return ids, chunk, comb, probs
    plain, off = call(), call(top_k=0, top_p=1.0)
    for a, b in zip(plain, off):
        assert torch.equal(a, b)
    for kw in (dict(top_k=-1), dict(top_p=0.0), dict(top_p=1.5), dict(top_p=math.nan), dict(top_k=-1, top_p=0.5)):
        with pytest.raises(ValueError):
            call(**kw)
    # the C entry refuses them itself: status -1 and a message
    fn = _lib.load().qarig_decode_sample_filtered
    ids = torch.zeros(B, dtype=torch.int64, device="cuda")
    chunk = torch.zeros((B, bw), dtype=torch.int64, device="cuda")
    comb = torch.ones(B, device="cuda")

    def raw(lg, ld, rows, cols, k, p):
        return fn(_lib.ptr(lg), ld, rows, cols, T, end, 1, 0, _lib.ptr(uniforms), None, _lib.ptr(ctl), 0, bw,
                  uniforms.shape[0], 0, 0, _lib.ptr(ids), _lib.ptr(chunk), _lib.ptr(comb), None, k, p,
                  _lib.stream())
    for k, p, word in ((-1, 1.0, "top_k"), (0, 0.0, "top_p"), (0, 1.5, "top_p"), (0, math.nan, "top_p")):
        assert raw(logits, V, B, V, k, p) == -1 and word in _lib.last_error()
    assert raw(logits, V, B, V, 4, 0.5) == 0
    # the documented bound: the row is staged in LDS, V <= 32768; the largest V runs, one more is refused
    big = torch.randn((1, 32769), generator=torch.Generator().manual_seed(1)).cuda()
    assert raw(big, 32769, 1, 32769, 1, 1.0) == -1 and "32768" in _lib.last_error()
    with pytest.raises(RuntimeError, match="32768"):
        ops.decode_sample(big, 1.0, 5, True, 0, uniforms[:, :1].contiguous(), ctl, 0, bw, ids[:1], chunk[:1], comb[:1],
                          top_k=1)
    ops.decode_sample(big[:, :32768], 1.0, 5, True, 0, uniforms[:, :1].contiguous(), ctl, 0, bw, ids[:1], chunk[:1],
                      comb[:1], top_k=1)
    want = big[0, :32768].clone()
    want[5] = -math.inf
    assert int(ids[0]) == int(want.argmax())


def _model(use_encoder, seed, dec_vocab=None, heads=8, dim=64, hidden=128, layers=2, vocab=41):
    """The small model of tests/test_gpu_kvcache.py (dim 64, 2 layers, vocab 41, pos_cond)."""
    from models.Transformer import Transformer
    torch.manual_seed(seed)
    kw = dict(use_encoder=use_encoder, use_pos_cond=True, num_enc_layers=2 if use_encoder else None,
              num_dec_layers=layers, num_enc_embedding=vocab if use_encoder else None,
              num_dec_embedding=dec_vocab or vocab, self_attn_heads=heads,
              cross_attn_heads=heads if use_encoder else None, transformer_in_dim=dim,
              transformer_out_dim=vocab, transformer_hidden_dim=hidden)
    m = Transformer(**kw).cuda().eval()
    with torch.no_grad():
        for p in m.parameters():
            if p.abs().max() == 0:
                p.normal_(0, 0.05)
    return m


GREEDY_SEED = 3          # model seed for which the top-2 gap below holds at every step (chosen on the GPU: smallest
                         # gap 4.6e-3 with the encoder, 6.6e-3 without; seed 4, for one, has a step at 3.7e-4)
GREEDY_T = 0.05          # the temperature of the cached-vs-full-window parity tests (test_gpu_kvcache.py)


def greedy_runs(use_encoder, total, seed=GREEDY_SEED, variants=True):
    """Tokens of every sampling path with top_k = 1 and the smallest top-2 probability gap the full-window loop
    saw.  {name: tokens}, gap."""
    from qarig import sampling
    m = _model(use_encoder, seed)
    N, sw = 3, 16
    g = torch.Generator().manual_seed(4)
    lr_in = torch.randint(0, 40, (N, 6), generator=g).cuda() if use_encoder else None
    first = torch.randint(0, 40, (N, 1), generator=g).cuda()

    def run(**kw):
        torch.manual_seed(11)
        return sampling.generate_tokens(m, first, lr_in, total, GREEDY_T, True, sw, end_token=40, num_beam=2,
                                        beam_width=4, mode="generate", top_k=1, **kw)
    gaps = []
    real = sampling.filter_probs

    def spy(probs, top_k=0, top_p=1.0):
        top2 = torch.topk(probs, 2, dim=-1).values
        gaps.append(float((top2[..., 0] - top2[..., 1]).min()))
        return real(probs, top_k, top_p)
    sampling.filter_probs = spy
    try:
        outs = {"full window": run(use_kv_cache=False, sampler="torch")}
    finally:
        sampling.filter_probs = real
    if variants:
        outs["fused"] = run(sampler="fused")
        outs["fused, window graph"] = run(sampler="fused", window_graph=True)
        outs["torch"] = run(sampler="torch")
        outs["batch beams, fused"] = run(sampler="fused", batch_beams=True)
        outs["batch beams, torch"] = run(sampler="torch", batch_beams=True)
        outs["batch beams, full window"] = run(use_kv_cache=False, batch_beams=True)
    sampling.decode_cache_clear()
    return outs, min(gaps)


@pytest.mark.parametrize("use_encoder", [False, True])
@pytest.mark.parametrize("total", [12, 24])
def test_greedy_generation_is_the_same_on_every_path(use_encoder, total):
    """top_k = 1 makes every path deterministic: the fused sampler (its tail past the window eager and as the
    window graph), sampler="torch", the full-window loop and the batched-beams forms must emit the same tokens
    (window 16: 12 tokens stay inside it, 24 slide it).  The paths' probabilities agree to 2e-5 (the tolerance of
    the parity tests in test_gpu_kvcache.py); the top-2 gap is required to be 50 times that at every step."""
    outs, gap = greedy_runs(use_encoder, total)
    print(f"use_encoder={use_encoder} total={total}: smallest top-2 gap {gap:.3e}")
    assert gap >= 1e-3, "a near-tie: an argmax flip from summation order would not be a bug"
    ref = outs["full window"]
    assert ref.shape[1] >= total
    for name, toks in outs.items():
        assert torch.equal(toks, ref), f"{name} differs from the full-window loop"


@pytest.mark.parametrize("num_beam,batch_beams", [(1, False), (2, False), (2, True)])
def test_filtered_generation_draws_only_kept_tokens(num_beam, batch_beams):
    """The fused sampler, base-stage form (shift = 41), top_k = 5 and top_p = 0.9, past the window: every logged
    row has 1..5 non-zero entries and every emitted token is non-zero in the row it was drawn from."""
    from qarig import sampling
    V, shift, N, bw, total, sw = 41, 41, 3, 4, 24, 16
    m = _model(False, 3, dec_vocab=2 * V)
    first = torch.randint(0, V, (N, 1), generator=torch.Generator().manual_seed(4)).cuda()
    sampling.FUSED_DEBUG = {"log": True}
    try:
        torch.manual_seed(11)
        toks = sampling.generate_tokens(m, first, None, total, 0.7, True, sw, end_token=V - 1, shift=shift,
                                        num_beam=num_beam, beam_width=bw, mode="generate", sampler="fused",
                                        batch_beams=batch_beams, top_k=5, top_p=0.9)
        dbg = sampling.FUSED_DEBUG
    finally:
        sampling.FUSED_DEBUG = None
        sampling.decode_cache_clear()
    draws = int(dbg["draws"])
    chunks = (toks.shape[1] - 1) // bw
    assert toks.shape[1] >= total and draws == chunks * bw * (1 if batch_beams else num_beam)
    probs = dbg["probs"][:draws]
    nnz = (probs > 0).sum(dim=-1)
    assert int(nnz.min()) >= 1 and int(nnz.max()) <= 5
    assert not dbg["probs"][draws:].any()
    tok = toks[:, 1:] - shift
    assert int(tok.min()) >= 0 and int(tok.max()) < V - 1
    # draw rows of chunk c: candidate k, slot j.  Reference order (one column per image): (c * NB + k) * bw + j;
    # --batch-beams (one column per image and beam): c * bw + j, column n * NB + k.  The kept chunk is one
    # candidate's: all of its tokens are non-zero in that candidate's rows.
    for c in range(chunks):
        for n in range(N):
            ok = False
            for k in range(num_beam):
                if batch_beams:
                    rows = [probs[c * bw + j, n * num_beam + k] for j in range(bw)]
                else:
                    rows = [probs[(c * num_beam + k) * bw + j, n] for j in range(bw)]
                ok = ok or all(float(rows[j][tok[n, c * bw + j]]) > 0 for j in range(bw))
            assert ok, f"chunk {c} of image {n}: a token outside the kept set"


@pytest.mark.parametrize("sampler", ["fused", "torch"])
def test_default_keywords_change_nothing(sampler):
    """A stage without the keys: the same tokens as a call without the keywords, for a fixed seed."""
    from qarig import sampling
    m = _model(True, 3)
    N, total, sw = 3, 24, 16
    g = torch.Generator().manual_seed(4)
    lr_in = torch.randint(0, 40, (N, 6), generator=g).cuda()
    first = torch.randint(0, 40, (N, 1), generator=g).cuda()

    def run(**kw):
        torch.manual_seed(11)
        return sampling.generate_tokens(m, first, lr_in, total, 0.7, True, sw, end_token=40, num_beam=2,
                                        beam_width=4, mode="generate", sampler=sampler, **kw)
    a, b, c = run(), run(top_k=0, top_p=1.0), run(top_k=5, top_p=0.9)
    sampling.decode_cache_clear()
    assert torch.equal(a, b)
    assert not torch.equal(a, c)           # (and the filter does reach this path)
