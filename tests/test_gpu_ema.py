"""EMA of the weights out of the Adam launch (csrc/optim.hip qarig_adam_ema_step), the in-place buffer exchange
(qarig_swap_f32) and what FlatAdam builds on them: enable_ema / ema_weights() / state round trip, eager, captured
and data parallel.  The kernel's bound is derived in tests/test_ema_host.py, which checks it on an fp32 emulation."""
import os
import socket
import sys

import pytest
import torch
import torch.multiprocessing as mp

from test_ema_host import STEPS, U, ema_w_sets

pytestmark = pytest.mark.gpu

WRAP = 8192 * 256 + 3        # one element past the capped grid: the grid-stride loop wraps
B1, B2, EPS = 0.5, 0.999, 1e-8


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _state(n, scale, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    p = torch.randn(n, device="cuda", generator=g) * scale
    e = torch.randn(n, device="cuda", generator=g) * scale       # independent of p: mixed signs on both
    return p, e, torch.zeros_like(p), torch.zeros_like(p), g


# ---------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("scale", [1e-3, 1.0, 1e3])
@pytest.mark.parametrize("wset", ["warmup", "mixed"])
@pytest.mark.parametrize("n", [1, 255, 257, WRAP])
def test_ema_matches_fp64_recurrence(n, wset, scale):
    """T = 5 steps with a weight that changes per step.  The fp64 recurrence is fed the kernel's own fp32
    parameters after each step, so Adam's error does not enter; per element
    |e - ref| <= 4 T 2^-24 M, M the largest max(|e|, |p|) the element saw (tests/test_ema_host.py)."""
    from qarig import ops
    ws = ema_w_sets()[wset]
    p, e, m, v, g = _state(n, scale, 7)
    ref = e.double()
    M = ref.abs()
    for t, w in enumerate(ws, 1):
        grad = torch.randn(n, device="cuda", generator=g) * scale
        ops.adam_ema_step(p, grad, m, v, e, B1, B2, EPS, 1e-2 * scale / (1 - B1 ** t), (1 - B2 ** t) ** 0.5, w)
        p64 = p.double()
        ref = ref + float(w) * (p64 - ref)
        M = torch.maximum(M, torch.maximum(torch.maximum(ref.abs(), p64.abs()), e.double().abs()))
    err = (e.double() - ref).abs() / (U * M.clamp_min(1e-37))
    worst = float(err.max())
    print(f"adam_ema n={n} {wset} scale={scale:g}: worst {worst:.3f} x 2^-24 M (bound {4 * STEPS})")
    assert torch.isfinite(e).all() and worst <= 4 * STEPS


@pytest.mark.parametrize("n", [257, WRAP])
def test_ema_exact_cases_bitwise(n):
    from qarig import ops
    p, e, m, v, g = _state(n, 1.0, 3)
    grad = torch.randn(n, device="cuda", generator=g)
    e0 = e.clone()
    ops.adam_ema_step(p, grad, m, v, e, B1, B2, EPS, 1e-2, 0.03, 1.0)          # w = 1: e' is p'
    assert _same_bits(e, p) and not _same_bits(e, e0)
    ops.adam_ema_step(p, grad, m, v, e, B1, B2, EPS, 1e-2, 0.03, 0.0)          # w = 0: e stays
    assert not _same_bits(e, p)
    e1 = e.clone()
    ops.adam_ema_step(p, grad, m, v, e, B1, B2, EPS, 1e-2, 0.03, 0.0)
    assert _same_bits(e, e1)
    # e == p, zero gradient, zero moments: p does not move and neither does e, at any weight
    for w in (0.0, 0.3, 0.5, 0.9, 1.0):
        q = p.clone()
        e = q.clone()
        z = torch.zeros_like(q)
        ops.adam_ema_step(q, z, z.clone(), z.clone(), e, B1, B2, EPS, 1e-2, 0.03, w)
        assert _same_bits(q, p) and _same_bits(e, p)


@pytest.mark.parametrize("with_shadow", [False, True])
@pytest.mark.parametrize("with_dev_step", [False, True])
@pytest.mark.parametrize("n", [257, WRAP])
def test_ema_launch_leaves_adam_bit_identical(n, with_dev_step, with_shadow):
    from qarig import ops
    p, e, m, v, g = _state(n, 1.0, 5)
    grad = torch.randn(n, device="cuda", generator=g)
    m.copy_(torch.randn(n, device="cuda", generator=g) * 0.1)
    v.copy_(torch.rand(n, device="cuda", generator=g) * 0.01)
    a = [p.clone(), m.clone(), v.clone()]
    b = [p.clone(), m.clone(), v.clone()]
    sh_a = torch.zeros(n, dtype=torch.bfloat16, device="cuda") if with_shadow else None
    sh_b = torch.zeros(n, dtype=torch.bfloat16, device="cuda") if with_shadow else None
    e0 = e.clone()
    ss, bc = 2e-3, 0.0316
    dev2 = torch.tensor([ss, bc], device="cuda") if with_dev_step else None
    dev3 = torch.tensor([ss, bc, 0.25], device="cuda") if with_dev_step else None
    host = (0.0, 1.0) if with_dev_step else (ss, bc)
    ops.adam_step(a[0], grad, a[1], a[2], B1, B2, EPS, host[0], host[1], 0.5, dev_step=dev2, shadow=sh_a)
    ops.adam_ema_step(b[0], grad, b[1], b[2], e, B1, B2, EPS, host[0], host[1], 0.0 if with_dev_step else 0.25, 0.5,
                      dev_step=dev3, shadow=sh_b)
    assert not _same_bits(a[0], p)
    for x, y in zip(a, b):
        assert _same_bits(x, y)
    if with_shadow:
        assert torch.equal(sh_a.view(torch.int16), sh_b.view(torch.int16))
        assert torch.equal(sh_a, a[0].to(torch.bfloat16))
    # and the weight did arrive, from the device buffer or the argument (w < 0.5: e + w (p' - e), no contraction)
    assert torch.equal(e, e0 + 0.25 * (b[0] - e0))


SENTINEL = 0x7FC0BEEF      # a NaN with a payload


@pytest.mark.parametrize("with_ema", [False, True], ids=["adam", "adam_ema"])
@pytest.mark.parametrize("off", [1, 3])
@pytest.mark.parametrize("n", [1, 7, 9, 257, 2049])
def test_plain_entries_take_views_of_any_4_byte_alignment(n, off, with_ema):
    """ops.adam_step and ops.adam_ema_step on views that start `off` floats into 16-byte-aligned buffers (the shadow
    `off` bf16 into its own), shadow on: the same bits as the same call on aligned copies, and the sentinels on both
    sides of every view keep theirs.  The grouped entries, with which these two share the host side, demand 16-byte
    alignment; these two must not."""
    from qarig import ops
    pad = 8
    gen = torch.Generator(device="cuda").manual_seed(100 * n + off)
    vals = [torch.randn(n, device="cuda", generator=gen), torch.randn(n, device="cuda", generator=gen),
            torch.randn(n, device="cuda", generator=gen) * 0.1, torch.rand(n, device="cuda", generator=gen) * 0.01,
            torch.randn(n, device="cuda", generator=gen)]                          # p, g, m, v, ema

    def view_into(dtype, fill, as_dtype):
        buf = torch.full((off + n + pad,), fill, dtype=dtype, device="cuda")
        view = buf[off:off + n].view(as_dtype)
        assert buf.data_ptr() % 16 == 0 and view.data_ptr() == buf.data_ptr() + off * buf.element_size()
        return buf, view

    bufs, views = zip(*(view_into(torch.int32, SENTINEL, torch.float32) for _ in vals))
    for view, x in zip(views, vals):
        view.copy_(x)
    sbuf, sview = view_into(torch.int16, 0x7FC1, torch.bfloat16)
    aligned = [x.clone() for x in vals]
    shadow = torch.zeros(n, dtype=torch.bfloat16, device="cuda")
    assert all(x.data_ptr() % 16 == 0 for x in aligned + [shadow])
    for (p, g, m, v, e), sh in ((views, sview), (aligned, shadow)):
        if with_ema:
            ops.adam_ema_step(p, g, m, v, e, B1, B2, EPS, 2e-3, 0.0316, 0.25, 0.5, shadow=sh)
        else:
            ops.adam_step(p, g, m, v, B1, B2, EPS, 2e-3, 0.0316, 0.5, shadow=sh)
    torch.cuda.synchronize()
    for k, (view, x, x0) in enumerate(zip(views, aligned, vals)):
        assert _same_bits(view, x), k
        assert _same_bits(x, x0) == (k == 1 or (k == 4 and not with_ema)), k      # all moved but g (and an unused ema)
    assert torch.equal(sview.view(torch.int16), shadow.view(torch.int16))
    assert torch.equal(shadow, aligned[0].to(torch.bfloat16))
    for buf in bufs:
        assert bool((buf[:off] == SENTINEL).all()) and bool((buf[off + n:] == SENTINEL).all())
    assert bool((sbuf[:off] == 0x7FC1).all()) and bool((sbuf[off + n:] == 0x7FC1).all())


@pytest.mark.parametrize("off", [0, 4, 1])         # 0 and 4: 16-byte aligned views; 1: the scalar form
@pytest.mark.parametrize("n", [1, 3, 4, 1023, 2 ** 20 + 1])
def test_swap_is_bit_exact_and_stays_inside_its_views(n, off):
    from qarig import ops
    pad = 16
    g = torch.Generator(device="cuda").manual_seed(n + off)
    bufs, views, want = [], [], []
    for k in range(2):
        buf = torch.full((n + 2 * pad,), SENTINEL, dtype=torch.int32, device="cuda")
        bits = torch.randint(-2 ** 31, 2 ** 31 - 1, (n,), dtype=torch.int64, device="cuda", generator=g).to(torch.int32)
        bits[0] = 0x7FA00001 + k            # signalling-NaN patterns with payloads
        bits[-1] = -(0x00400123 + k)        # (negative int32: sign bit set, a NaN / denormal pattern)
        buf[off:off + n] = bits
        bufs.append(buf)
        views.append(buf.view(torch.float32)[off:off + n])
        want.append(bits.clone())
    ops.swap_(views[0], views[1])
    for k in range(2):
        assert torch.equal(bufs[k][off:off + n], want[1 - k])
        assert bool((bufs[k][:off] == SENTINEL).all()) and bool((bufs[k][off + n:] == SENTINEL).all())
    ops.swap_(views[0], views[1])       # twice: the identity
    for k in range(2):
        assert torch.equal(bufs[k][off:off + n], want[k])
        assert bool((bufs[k][:off] == SENTINEL).all()) and bool((bufs[k][off + n:] == SENTINEL).all())


def test_swap_argument_errors_return_minus_one_without_a_launch():
    from qarig import _lib, ops
    lib = _lib.load()
    a = torch.arange(8, dtype=torch.float32, device="cuda")
    b = torch.arange(8, 16, dtype=torch.float32, device="cuda")
    s = _lib.stream()
    assert lib.qarig_swap_f32(None, b.data_ptr(), 8, s) == -1
    assert lib.qarig_swap_f32(a.data_ptr(), None, 8, s) == -1
    assert lib.qarig_swap_f32(a.data_ptr(), b.data_ptr(), 0, s) == -1
    assert lib.qarig_swap_f32(a.data_ptr(), b.data_ptr(), -3, s) == -1
    assert lib.qarig_swap_f32(a.data_ptr(), a.data_ptr() + 16, 8, s) == -1 and "overlap" in _lib.last_error()
    assert lib.qarig_adam_ema_step(a.data_ptr(), b.data_ptr(), a.data_ptr(), a.data_ptr(), None, 8, 0.5, 0.999, 1e-8,
                                   1e-3, 1.0, 0.1, 1.0, None, None, s) == -1
    torch.cuda.synchronize()
    assert torch.equal(a.cpu(), torch.arange(8.0)) and torch.equal(b.cpu(), torch.arange(8.0, 16.0))
    with pytest.raises(ValueError):
        ops.swap_(a, b[:4])


# ----------------------------------------------------------------------------------- FlatAdam and the pipeline
@pytest.fixture(autouse=True)
def _position_table_on():
    from qarig import functional as QF
    old = QF.COND_TABLE_MIN_RATIO
    QF.COND_TABLE_MIN_RATIO = 0
    yield
    QF.COND_TABLE_MIN_RATIO = old


def _build(ema=None):
    """Decoder-only model of two layers, 64 wide, trained on windows of 12 of its 17 tokens."""
    from models.Codebook import Codebook
    from models.Transformer import Transformer
    from qarig.optim import FlatAdam
    torch.manual_seed(3)
    g = torch.Generator().manual_seed(4)
    lr_cb = Codebook(patch_dim=(8, 8), image_dim=(8, 8), image_channel=4, num_embeddings=16).cuda()
    hr_cb = Codebook(patch_dim=(2, 2), image_dim=(8, 8), image_channel=4, num_embeddings=32).cuda()
    with torch.no_grad():
        lr_cb.codebook.weight.copy_(torch.tanh(torch.randn(lr_cb.codebook.weight.shape, generator=g)))
        hr_cb.codebook.weight.copy_(torch.tanh(torch.randn((32, 16), generator=g)))
    m = _bare_model()
    with torch.no_grad():
        for p in m.parameters():
            if p.abs().max() == 0:
                p.copy_(torch.randn(p.shape, generator=g) * 0.05)
    opt = FlatAdam(m.parameters(), lr=1e-3, betas=(0.5, 0.999))
    if ema is not None:
        opt.enable_ema(ema)
    return lr_cb, hr_cb, m, opt


def _bare_model():
    from models.Transformer import Transformer
    return Transformer(use_encoder=False, use_pos_cond=True, num_enc_layers=None, num_dec_layers=2,
                       num_enc_embedding=None, num_dec_embedding=48, self_attn_heads=8, cross_attn_heads=None,
                       transformer_in_dim=64, transformer_out_dim=33, transformer_hidden_dim=128).cuda()


def _batches(n=5):
    g = torch.Generator().manual_seed(9)
    return [(torch.tanh(torch.randn((6, 4, 8, 8), generator=g)), torch.randint(0, 17 - 12 + 1, (6,), generator=g))
            for _ in range(n)]


def _eager_steps(lr_cb, hr_cb, m, opt, batches):
    from qarig import pipeline
    for z, rand in batches:
        hr_in, lr_in, hr_tg = pipeline.tokenize(z.cuda(), lr_cb, hr_cb, True)
        hr_in, hr_tg, pos = pipeline.slide(hr_in, hr_tg, 12, rand)
        pipeline.train_step(m, opt, hr_in, lr_in, hr_tg, pos, dp=False, pos_bound=17)


def test_captured_steps_equal_eager_steps_with_ema():
    from qarig import pipeline
    from qarig.optim import ema_weight
    lr_cb, hr_cb, m, opt_e = _build(ema=0.999)
    _eager_steps(lr_cb, hr_cb, m, opt_e, _batches())
    lr_cb, hr_cb, m, opt_off = _build()
    _eager_steps(lr_cb, hr_cb, m, opt_off, _batches())
    lr_cb, hr_cb, m, opt_g = _build(ema=0.999)
    assert opt_g._dev_step_buffer().numel() == 3 and opt_off._dev_step_buffer().numel() == 2
    step = pipeline.GraphedTrainStep(m, opt_g, lr_cb, hr_cb, True, 12, warmup=2)
    for z, rand in _batches():
        step(z.cuda(), rand)
    torch.cuda.synchronize()
    assert step.graph is not None and opt_g.step_count == 5
    assert opt_g.ema_count == 5 and opt_e.ema_count == 5
    assert _same_bits(opt_g.flat_param, opt_e.flat_param) and _same_bits(opt_g.flat_ema, opt_e.flat_ema)
    assert _same_bits(opt_e.flat_param, opt_off.flat_param)          # the EMA launch does not touch the training
    assert not _same_bits(opt_e.flat_ema, opt_e.flat_param)
    assert float(opt_g._dev_step[2]) == ema_weight(4, 0.999, True)


def test_enable_ema_after_a_capture_raises():
    from qarig import pipeline
    lr_cb, hr_cb, m, opt = _build()
    step = pipeline.GraphedTrainStep(m, opt, lr_cb, hr_cb, True, 12, warmup=1)
    for z, rand in _batches(2):
        step(z.cuda(), rand)
    assert step.graph is not None
    with pytest.raises(RuntimeError, match="captured"):
        opt.enable_ema(0.999)
    assert opt.flat_ema is None


def _generate(m, first, forced=None):
    """(tokens, the probability row of every draw) of a cached generation whose window slides.  forced: the
    draws (sampling.FUSED_DEBUG); which of an image's two candidate chunks is kept, and so the tokens, still
    follows the model's probabilities."""
    from qarig import sampling
    torch.manual_seed(5)
    sampling.FUSED_DEBUG = {"log": True, "forced": forced}
    try:
        toks = sampling.generate_tokens(m, first, None, 16, 0.7, True, 12, end_token=32, shift=16, num_beam=2,
                                        beam_width=4, mode="generate", use_kv_cache=True, sampler="fused")
        probs = sampling.FUSED_DEBUG["probs"][:sampling.FUSED_DEBUG["draws"]]
        return torch.cat((toks.flatten().float(), probs.flatten().float()))
    finally:
        sampling.FUSED_DEBUG = None


def _forced_draws(m, first):
    from qarig import sampling
    sampling.FUSED_DEBUG = {"log": True}
    try:
        sampling.generate_tokens(m, first, None, 16, 0.7, True, 12, end_token=32, shift=16, num_beam=2,
                                 beam_width=4, mode="generate", use_kv_cache=True, sampler="fused")
        draws, cols = sampling.FUSED_DEBUG["probs"].shape[:2]
    finally:
        sampling.FUSED_DEBUG = None
    return torch.randint(0, 32, (draws, cols), generator=torch.Generator().manual_seed(6))


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_ema_weights_context_serves_the_ema_everywhere_and_restores(precision):
    from qarig import ops, sampling
    old = ops.PRECISION
    ops.set_precision(precision)
    sampling.decode_cache_clear()
    try:
        lr_cb, hr_cb, m, opt = _build(ema=0.9)
        _eager_steps(lr_cb, hr_cb, m, opt, _batches(3))         # (bf16: the Adam pass has written the weight shadow)
        with torch.no_grad():                                   # <end> out of the way, in both sets of weights
            bias = m.classifier[1].linear_layer[0].bias
            bias[32] -= 20.0
            opt.ema_views()[[id(q) for q in opt.params].index(id(bias))][32] -= 20.0
        fresh = _bare_model()
        fresh.custom_load_state_dict({k: v.cpu() for k, v in opt.ema_state_dict(m).items()})
        fresh = fresh.cuda().eval()
        m.eval()
        g = torch.Generator().manual_seed(2)
        x = torch.randint(0, 48, (3, 12), generator=g).cuda()
        pos = (torch.arange(12)[None] + torch.randint(0, 5, (3, 1), generator=g)).cuda()
        first = torch.randint(0, 16, (3, 1), generator=g).cuda()
        with torch.no_grad():
            want_logits = fresh(x, None, pos, pos_bound=17)
            raw_logits = m(x, None, pos, pos_bound=17)
            forced = _forced_draws(fresh, first)
            want_gen = _generate(fresh, first, forced)
            raw_gen = _generate(m, first, forced)               # leaves a decode cache of the raw weights behind
            assert not torch.equal(raw_gen, want_gen) and not torch.equal(raw_logits, want_logits)
            param0, ema0 = opt.flat_param.clone(), opt.flat_ema.clone()
            with opt.ema_weights():
                assert _same_bits(opt.flat_param, ema0) and _same_bits(opt.flat_ema, param0)
                assert _same_bits(m(x, None, pos, pos_bound=17), want_logits)
                assert torch.equal(_generate(m, first, forced), want_gen)     # (leaves a cache of the EMA weights)
                with pytest.raises(RuntimeError):
                    opt.step()
                with pytest.raises(RuntimeError):
                    with opt.ema_weights():
                        pass
            assert _same_bits(opt.flat_param, param0) and _same_bits(opt.flat_ema, ema0)
            assert _same_bits(m(x, None, pos, pos_bound=17), raw_logits)
            assert torch.equal(_generate(m, first, forced), raw_gen)
        assert opt.step_count == 3 and opt.ema_count == 3
    finally:
        ops.set_precision(old)
        ops.lp_invalidate()
        sampling.decode_cache_clear()


def _synthetic_grads(opt, k):
    g = torch.Generator(device="cuda").manual_seed(100 + k)
    for q in opt.params:            # (the alignment padding between the slices keeps its zero gradient)
        q.grad.copy_(torch.randn(q.shape, device="cuda", generator=g) * 0.01)


def test_ema_state_round_trip_resumes_bitwise():
    from qarig.optim import FlatAdam
    _, _, m, opt = _build(ema=0.999)
    for k in range(5):
        _synthetic_grads(opt, k)
        opt.step()
    _, _, m1, opt1 = _build(ema=0.999)
    for k in range(3):
        _synthetic_grads(opt1, k)
        opt1.step()
    saved = {"model": {k: v.detach().clone().cpu() for k, v in m1.state_dict().items()},
             "model_ema": {k: v.cpu() for k, v in opt1.ema_state_dict(m1).items()},
             "model_ema_meta": opt1.ema_meta(), "model_optimizer": opt1.state_dict()}
    assert saved["model_ema_meta"] == {"decay": 0.999, "count": 3, "warmup": True}
    assert list(saved["model_ema"]) == list(saved["model"])
    m2 = _bare_model()
    m2.custom_load_state_dict(saved["model"])
    opt2 = FlatAdam(m2.cuda().parameters(), lr=1e-3, betas=(0.5, 0.999))
    opt2.load_state_dict(saved["model_optimizer"])
    opt2.enable_ema(saved["model_ema_meta"]["decay"], saved["model_ema_meta"]["warmup"])
    opt2.load_ema(saved["model_ema"], m2, saved["model_ema_meta"]["count"])
    assert _same_bits(opt2.flat_ema, opt1.flat_ema) and opt2.ema_count == 3
    for k in range(3, 5):
        _synthetic_grads(opt2, k)
        opt2.step()
    assert opt2.ema_count == opt.ema_count == 5
    assert _same_bits(opt2.flat_param, opt.flat_param) and _same_bits(opt2.flat_ema, opt.flat_ema)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _dp_worker(rank, world, port, q):
    from conftest import PKG, ROOT
    for p in (ROOT, PKG):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK="0")
    import torch.distributed as dist
    from qarig import functional as QF
    from qarig import optim as qoptim
    from qarig import parallel, pipeline
    QF.COND_TABLE_MIN_RATIO = 0
    parallel.init(backend="gloo", force=True)
    torch.cuda.set_device(0)
    qoptim.BUCKET_ELEMS = 40_000
    lr_cb, hr_cb, m, opt = _build()
    if rank == 1:
        with torch.no_grad():
            opt.flat_param.add_(1.0)          # rank 1 starts elsewhere: the broadcast has to carry both buffers
    opt.enable_ema(0.999)
    parallel.broadcast_params(opt)
    opt.enable_allreduce_overlap(force=True)
    assert len(opt._bucket_range) > 2
    for z, rand in _batches(3):
        hr_in, lr_in, hr_tg = pipeline.tokenize(parallel.shard(z).cuda(), lr_cb, hr_cb, True)
        hr_in, hr_tg, pos = pipeline.slide(hr_in, hr_tg, 12, parallel.shard(rand))
        pipeline.train_step(m, opt, hr_in, lr_in, hr_tg, pos, pos_bound=17)
    torch.cuda.synchronize()
    q.put((rank, opt.flat_ema.detach().cpu().numpy(), opt.flat_param.detach().cpu().numpy(), opt.ema_count))
    dist.barrier()
    dist.destroy_process_group()


def test_data_parallel_ranks_hold_the_same_ema():
    import queue
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = {}
    for _ in range(180):                      # poll: a crashed worker must not cost minutes
        try:
            r, ema, par, count = q.get(timeout=1)
            got[r] = (torch.from_numpy(ema), torch.from_numpy(par), count)
            if len(got) == 2:
                break
        except queue.Empty:
            if any(p.exitcode not in (None, 0) for p in procs):
                break
    for p in procs:
        p.join(timeout=30)
        if p.is_alive():
            p.kill()
    assert len(got) == 2 and all(p.exitcode == 0 for p in procs)
    assert got[0][2] == got[1][2] == 3
    assert _same_bits(got[0][0], got[1][0]) and _same_bits(got[0][1], got[1][1])
    assert not _same_bits(got[0][0], got[0][1])
