"""Gradient clipping above the kernels, on the GPU at the small model of tests/test_gpu_adamw_train.py: which
entries a step calls, graph replay against eager steps, a skipped step under replay, the model against the fp64
definition fed its own gradients, resuming, the refusals, two data-parallel ranks, and the command line."""
import functools
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import adamw_cases as A
import grad_clip_cases as C
from conftest import PKG

pytestmark = pytest.mark.gpu

V_ENC, V_DEC, V_OUT, S, N = 16, 40, 33, 16, 2
LAM = 0.1


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _model():
    from models.Transformer import Transformer
    torch.manual_seed(5)
    m = Transformer(use_encoder=True, use_pos_cond=True, num_enc_layers=1, num_dec_layers=2, num_enc_embedding=V_ENC,
                    num_dec_embedding=V_DEC, self_attn_heads=2, cross_attn_heads=2, transformer_in_dim=128,
                    transformer_out_dim=V_OUT, transformer_hidden_dim=256).cuda()
    g = torch.Generator().manual_seed(6)
    with torch.no_grad():
        for p in m.parameters():
            if p.abs().max() == 0:
                p.copy_(torch.randn(p.shape, generator=g) * 0.05)
    return m


def _optimizer(m, decay=LAM, ema=None, clip=None):
    from qarig.optim import FlatAdam, decay_parameters
    opt = FlatAdam(m.parameters(), lr=1e-3, betas=(0.5, 0.999))
    if ema is not None:
        opt.enable_ema(ema)
    if decay:
        opt.enable_weight_decay(decay, decay_parameters(m))
    if clip is not None:
        opt.enable_grad_clip(clip)
    return opt


def _data(k=0):
    g = torch.Generator().manual_seed(20 + k)
    x_dec = torch.randint(0, V_DEC, (N, S), generator=g).cuda()
    x_enc = torch.randint(0, V_ENC, (N, S), generator=g).cuda()
    tgt = torch.randint(0, V_OUT, (N, S), generator=g).cuda()
    pos = (torch.randint(0, 5, (N, 1), generator=g) + torch.arange(S)[None]).cuda()
    return x_dec, x_enc, tgt, pos


# ---- 1: which entries a step calls -----------------------------------------------------------------------------
NAMES = ("adam_step", "adam_ema_step", "adamw_step", "grad_clip_coef", "adam_clip_step")


def _spy(monkeypatch):
    from qarig import ops
    calls = []
    for name in NAMES:
        real = getattr(ops, name)
        monkeypatch.setattr(ops, name, (lambda real, name: lambda *a, **k: (calls.append(name), real(*a, **k))[1])(
            real, name))
    return calls


@pytest.mark.parametrize("decay", [0, LAM])
@pytest.mark.parametrize("ema", [None, 0.999])
def test_which_entries_a_step_calls(monkeypatch, ema, decay):
    from qarig import _lib
    calls = _spy(monkeypatch)
    off = _optimizer(_model(), decay=decay, ema=ema)
    assert off.clip_max_norm is None and not hasattr(off, "clip_state")
    before = _lib.N_CALLS
    off.step()
    off.advance_captured()
    off.step_captured()
    plain = "adamw_step" if decay else "adam_step" if ema is None else "adam_ema_step"
    assert calls == [plain] * 2 and _lib.N_CALLS - before == 2
    assert off._dev_step_buffer().numel() == (4 if decay else 2 if ema is None else 3)
    with pytest.raises(RuntimeError, match="enable_grad_clip"):
        off.clip_stats()
    del calls[:]
    on = _optimizer(_model(), decay=decay, ema=ema, clip=1.0)
    assert on.clip_state.dtype == torch.float64 and on.clip_state.tolist() == [0.0] * 4
    before = _lib.N_CALLS
    on.step()
    assert calls == ["grad_clip_coef", "adam_clip_step"] and _lib.N_CALLS - before == 2
    on.advance_captured()
    assert on._dev_step_buffer().numel() == 4
    if not decay:
        assert float(on._dev_step[3]) == 0.0          # no weight decay: the decay slot is filled with 0
    on.step_captured()
    assert calls == ["grad_clip_coef", "adam_clip_step"] * 2 and _lib.N_CALLS - before == 4
    assert set(on.clip_stats()) == {"norm", "coef", "skipped", "clipped"}


# ---- 2: graph replay against eager steps -----------------------------------------------------------------------
def _build_pipeline(decay, ema, clip):
    from models.Codebook import Codebook
    g = torch.Generator().manual_seed(4)
    lr_cb = Codebook(patch_dim=(4, 4), image_dim=(8, 8), image_channel=4, num_embeddings=V_ENC).cuda()
    hr_cb = Codebook(patch_dim=(2, 2), image_dim=(8, 8), image_channel=4, num_embeddings=V_OUT - 1).cuda()
    with torch.no_grad():
        lr_cb.codebook.weight.copy_(torch.tanh(torch.randn(lr_cb.codebook.weight.shape, generator=g)))
        hr_cb.codebook.weight.copy_(torch.tanh(torch.randn(hr_cb.codebook.weight.shape, generator=g)))
    m = _model()
    m.train()
    return lr_cb, hr_cb, m, _optimizer(m, decay=decay, ema=ema, clip=clip)


def _batches(n=5):
    g = torch.Generator().manual_seed(9)
    return [(torch.tanh(torch.randn((N, 4, 8, 8), generator=g)), torch.randint(0, 17 - S + 1, (N,), generator=g))
            for _ in range(n)]


def _schedule():
    from qarig.optim import LRSchedule
    return LRSchedule(1e-3, "cosine", warmup_steps=2, decay_steps=5)


def _eager(decay, ema, clip):
    """Five eager steps; returns the optimizer and, with the clip on, the norm of every step."""
    from qarig import pipeline
    lr_cb, hr_cb, m, opt = _build_pipeline(decay, ema, clip)
    sched, norms = _schedule(), []
    for z, rand in _batches():
        opt.param_groups[0]["lr"] = sched.lr(opt.step_count + 1)
        hr_in, lr_in, hr_tg = pipeline.tokenize(z.cuda(), lr_cb, hr_cb, False)
        hr_in, hr_tg, pos = pipeline.slide(hr_in, hr_tg, S, rand)
        pipeline.train_step(m, opt, hr_in, lr_in, hr_tg, pos, dp=False, pos_bound=17)
        if clip is not None:
            norms.append(opt.clip_stats()["norm"])
    return opt, norms


@functools.lru_cache(maxsize=None)
def _threshold():
    """A max_norm some of the five steps exceed and some do not: the median of the norms the same five batches
    give with the guard alone (the tests assert from the counters that both kinds did occur)."""
    _, norms = _eager(0, None, float("inf"))
    assert all(np.isfinite(norms)) and min(norms) > 0
    return float(sorted(norms)[2])


@pytest.mark.parametrize("decay", [0, LAM])
@pytest.mark.parametrize("ema", [None, 0.999])
def test_graph_replay_matches_eager_steps(ema, decay):
    from qarig import pipeline
    clip = _threshold()
    opt_e, norms = _eager(decay, ema, clip)
    stats_e = opt_e.clip_stats()
    print(f"threshold {clip:.6f}, norms {norms}, stats {stats_e}")
    assert 0 < stats_e["clipped"] < 5 and stats_e["skipped"] == 0          # both kinds of step occurred
    assert stats_e["clipped"] == sum(C.coef_def(x, clip) < 1.0 for x in norms)
    lr_cb, hr_cb, m, opt_g = _build_pipeline(decay, ema, clip)
    step, sched = pipeline.GraphedTrainStep(m, opt_g, lr_cb, hr_cb, False, S, warmup=2), _schedule()
    for z, rand in _batches():
        opt_g.param_groups[0]["lr"] = sched.lr(opt_g.step_count + 1)
        step(z.cuda(), rand)
    torch.cuda.synchronize()
    assert step.graph is not None and opt_g.step_count == 5 and opt_g._dev_step.numel() == 4
    assert _same_bits(opt_g.flat_param, opt_e.flat_param)
    assert _same_bits(opt_g.exp_avg, opt_e.exp_avg) and _same_bits(opt_g.exp_avg_sq, opt_e.exp_avg_sq)
    if ema is not None:
        assert _same_bits(opt_g.flat_ema, opt_e.flat_ema) and not _same_bits(opt_e.flat_ema, opt_e.flat_param)
    assert torch.equal(opt_g.clip_state.view(torch.int64), opt_e.clip_state.view(torch.int64))
    assert opt_g.clip_stats() == stats_e
    opt_off, _ = _eager(decay, ema, None)                 # the same data with the clip off ends elsewhere
    assert not _same_bits(opt_off.flat_param, opt_e.flat_param)
    assert not _same_bits(opt_off.exp_avg, opt_e.exp_avg)


# ---- 3: a skipped step under replay ----------------------------------------------------------------------------
def _synthetic_grads(opt, k):
    g = torch.Generator(device="cuda").manual_seed(100 + k)
    for q in opt.params:            # (the alignment padding between the slices keeps its zero gradient)
        q.grad.copy_(torch.randn(q.shape, device="cuda", generator=g) * 0.01)


def _state(opt):
    return [t.clone() for t in (opt.flat_param, opt.exp_avg, opt.exp_avg_sq, opt.flat_ema)]


def test_skipped_step_under_replay():
    """step_captured() alone in a graph, the norm launch included, replayed on finite gradients, on gradients with
    one NaN and on finite ones again: the second replay changes no bit, the third continues from the first with
    the scalars of step 3 (the host counts the skipped step)."""
    opt = _optimizer(_model(), ema=0.9, clip=0.05)
    opt._dev_step_buffer()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step_captured()
    start = _state(opt)
    states = []
    for k in range(3):
        _synthetic_grads(opt, k)
        if k == 1:
            opt.flat_grad[opt.total // 2] = float("nan")
        opt.advance_captured()
        graph.replay()
        torch.cuda.synchronize()
        states.append(_state(opt))
        stats = opt.clip_stats()
        assert stats["skipped"] == (1 if k >= 1 else 0)
        assert np.isfinite(stats["norm"]) == (k != 1)
    assert all(not _same_bits(a, b) for a, b in zip(start, states[0]))
    assert all(_same_bits(a, b) for a, b in zip(states[0], states[1]))
    assert all(not _same_bits(a, b) for a, b in zip(states[1], states[2]))
    assert opt.step_count == 3 and opt.ema_count == 3 and opt.clip_stats()["clipped"] == 2
    # eager, without the second step but with its counts
    ref = _optimizer(_model(), ema=0.9, clip=0.05)
    _synthetic_grads(ref, 0)
    ref.step()
    assert all(_same_bits(a, b) for a, b in zip(_state(ref), states[0]))
    ref.step_count += 1
    ref.ema_count += 1
    _synthetic_grads(ref, 2)
    ref.step()
    assert all(_same_bits(a, b) for a, b in zip(_state(ref), states[2]))
    # and an eager step on the NaN gradients skips likewise
    eager = _optimizer(_model(), ema=0.9, clip=0.05)
    _synthetic_grads(eager, 1)
    eager.flat_grad[eager.total // 2] = float("nan")
    eager.step()
    assert all(_same_bits(a, b) for a, b in zip(_state(eager), start))
    assert eager.clip_stats()["skipped"] == 1 and eager.step_count == 1


def test_bf16_weight_image_under_the_clip():
    """Reduced precision: the clipped launch writes the bf16 image of the parameters as the plain one does, and a
    skipped FIRST step leaves the image of the parameters as they stand, not an unwritten buffer."""
    from qarig import ops
    old = ops.PRECISION
    ops.set_precision("bf16")
    try:
        torch.manual_seed(2)
        m = torch.nn.Sequential(torch.nn.Linear(64, 129), torch.nn.Linear(129, 32)).cuda()
        opt = _optimizer(m, decay=0, clip=0.5)
        ps = list(m.parameters())
        before = opt.flat_param.clone()
        for p in ps:
            p.grad.copy_(torch.randn_like(p))
        opt.flat_grad[3] = float("inf")
        opt.step()                                                       # skipped
        assert opt.clip_stats()["skipped"] == 1 and _same_bits(opt.flat_param, before)
        for p in ps:
            assert torch.equal(opt.shadow_of(p), p.detach().to(torch.bfloat16))
        for p in ps:
            p.grad.copy_(torch.randn_like(p))
        opt.step()
        assert opt.clip_stats()["clipped"] == 1 and not _same_bits(opt.flat_param, before)
        for p in ps:
            assert torch.equal(opt.shadow_of(p), p.detach().to(torch.bfloat16))
    finally:
        ops.set_precision(old)


# ---- 4: the model against the fp64 definition fed its own gradients --------------------------------------------
def test_three_model_steps_against_the_fp64_definition():
    from qarig import functional as QF
    from qarig.optim import ema_weight
    m = _model()
    m.train()
    opt = _optimizer(m, ema=0.9, clip=1.0)
    p0, e0 = opt.flat_param.clone(), opt.flat_ema.clone()
    grads, got, scalars, norms = [], [], [], []
    for t in range(1, 4):
        x_dec, x_enc, tgt, pos = _data(t)
        opt.zero_grad()
        logits = m(x_dec=x_dec, x_enc=x_enc, pos_cond=pos, pos_bound=S + 5)
        QF.cross_entropy(logits.view(-1, V_OUT), tgt.flatten()).backward()
        grads.append(opt.flat_grad.clone())
        if t == 1:      # a max_norm the first step's own norm sets: steps clip by a real factor
            opt.enable_grad_clip(0.5 * C.norm_ref64(grads[0]))
        scalars.append(A.step_scalars(t, 1e-3, LAM, (0.5, 0.999), ema_weight(t - 1, 0.9, True)))
        opt.step()
        stats = opt.clip_stats()
        norms.append(stats["norm"])
        got.append(dict(p=opt.flat_param.clone(), m=opt.exp_avg.clone(), v=opt.exp_avg_sq.clone(),
                        ema=opt.flat_ema.clone(), coef=stats["coef"]))
    max_norm = opt.clip_max_norm
    for g, x, c in zip(grads, norms, got):
        want = C.norm_ref64(g)
        assert abs(x - want) <= C.bound_norm(opt.total) * want
        assert c["coef"] == C.coef_def(x, max_norm)
    assert got[0]["coef"] < 0.51 and opt.clip_stats()["clipped"] >= 1
    ref = C.clip_adamw_ref64(p0, grads, opt.decay_mask, scalars, A.f32(0.5), A.f32(0.999), A.f32(1e-8), 1.0,
                             max_norm, ema=e0, coefs=[g["coef"] for g in got], norms=norms)
    r = C.worst_ratios(ref, got)
    print("clipped model, 3 steps, {} elements: worst / bound  p {:.4f}  m {:.4f}  v {:.4f}  ema {:.4f}; "
          "coefs {}".format(opt.total, r["p"], r["m"], r["v"], r["ema"], [g["coef"] for g in got]))
    assert all(0.0 <= x <= 1.0 for x in r.values()), r
    unclipped = C.clip_adamw_ref64(p0, grads, opt.decay_mask, scalars, A.f32(0.5), A.f32(0.999), A.f32(1e-8), 1.0,
                                   float("inf"), ema=e0)
    assert C.worst_ratios(unclipped, got)["m"] > 1.0


# ---- 5: a state round trip -------------------------------------------------------------------------------------
def test_state_round_trip_continues_bitwise():
    sched = _schedule()

    def run(opt, ks):
        for k in ks:
            opt.param_groups[0]["lr"] = sched.lr(opt.step_count + 1)
            _synthetic_grads(opt, k)
            opt.step()

    opt = _optimizer(_model(), clip=0.05)
    run(opt, range(5))
    assert opt.clip_stats()["clipped"] == 5
    m1 = _model()
    opt1 = _optimizer(m1, clip=0.05)
    run(opt1, range(2))
    saved = {"model": {k: v.detach().clone().cpu() for k, v in m1.state_dict().items()},
             "model_optimizer": opt1.state_dict()}
    assert set(saved["model_optimizer"]) == {"state", "param_groups"}           # the layout is the plain one
    m2 = _model()
    m2.load_state_dict(saved["model"])
    opt2 = _optimizer(m2, clip=0.05)
    opt2.load_state_dict(saved["model_optimizer"])
    run(opt2, range(2, 5))
    assert opt2.step_count == 5 and _same_bits(opt2.flat_param, opt.flat_param)
    assert _same_bits(opt2.exp_avg, opt.exp_avg) and _same_bits(opt2.exp_avg_sq, opt.exp_avg_sq)
    assert opt2.clip_stats()["clipped"] == 3                 # the counts start again with the process


# ---- 6: refusals -----------------------------------------------------------------------------------------------
def test_enable_grad_clip_refusals():
    from qarig import pipeline
    lr_cb, hr_cb, m, opt = _build_pipeline(0, 0.9, None)
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            opt.enable_grad_clip(bad)
    with opt.ema_weights():
        with pytest.raises(RuntimeError, match="ema_weights"):
            opt.enable_grad_clip(1.0)
    assert opt.clip_max_norm is None
    step = pipeline.GraphedTrainStep(m, opt, lr_cb, hr_cb, False, S, warmup=1)
    for z, rand in _batches(2):
        step(z.cuda(), rand)
    assert step.graph is not None
    with pytest.raises(RuntimeError, match="captured"):
        opt.enable_grad_clip(1.0)
    assert opt.clip_max_norm is None and not hasattr(opt, "clip_state")


# ---- 7: two data-parallel ranks --------------------------------------------------------------------------------
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
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(world), LOCAL_RANK="0")
    import torch.distributed as dist
    from qarig import optim as qoptim
    from qarig import parallel, pipeline
    parallel.init(backend="gloo", force=True)
    torch.cuda.set_device(0)
    m = _model()
    qoptim.BUCKET_ELEMS = 50_000                     # several buckets on this small model
    opt = qoptim.FlatAdam(m.parameters(), lr=1e-3, betas=(0.5, 0.999))
    parallel.broadcast_params(opt.flat_param)
    opt.enable_grad_clip(1e-3)                       # far below any gradient norm of this model: every step clips
    opt.enable_allreduce_overlap(force=True)
    assert len(opt._bucket_range) > 2
    x = [torch.cat([a, b]) for a, b in zip(_data(1), _data(2))]         # four samples, two per rank
    x_dec, x_enc, tgt, pos = (parallel.shard(v.cpu()).cuda() for v in x)
    for _ in range(2):
        pipeline.train_step(m, opt, x_dec, x_enc, tgt, pos, pos_bound=S + 5)
    torch.cuda.synchronize()
    # by value (numpy): a torch tensor travels as a file descriptor that dies with this process
    q.put((rank, opt.clip_state.view(torch.int64).cpu().numpy(), opt.flat_param.view(torch.int32).cpu().numpy(),
           opt.clip_stats()))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_clip_alike():
    """Eager steps, overlapped bucket all-reduces over gloo: behind the exchange both ranks hold the same gradient
    bits, so the norm, the coefficient, the counts and the parameters are the same bits too -- no collective of
    the clip's own."""
    import queue
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = {}
    for _ in range(180):                      # poll: a crashed worker must not cost minutes
        try:
            item = q.get(timeout=1)
            got[item[0]] = item[1:]
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
    assert np.array_equal(got[0][0], got[1][0]), (got[0][2], got[1][2])
    assert np.array_equal(got[0][1], got[1][1])
    assert got[0][2] == got[1][2] and got[0][2]["clipped"] == 2 and got[0][2]["skipped"] == 0
    assert 0 < got[0][2]["coef"] < 1 and np.isfinite(got[0][2]["norm"])


# ---- 8: the command line: the fixtures of tests/test_gpu_adamw_train.py, copied ---------------------------------
BASE_KEYS = {"train_base_model", "use_sliding_window", "sliding_window", "num_enc_embedding", "num_dec_embedding",
             "num_enc_layers", "num_dec_layers", "self_attn_heads", "cross_attn_heads", "transformer_in_dim",
             "transformer_out_dim", "transformer_hidden_dim", "hidden_activation", "model", "model_optimizer"}


def _run(script, *args, cwd, ok=True):
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(PKG, script), *map(str, args)], cwd=cwd, env=env,
                       capture_output=True, text=True, timeout=300)
    if ok:
        assert r.returncode == 0, f"{script} failed:\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    return r


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    sys.path.insert(0, PKG)
    from dataset_loader._tinydb_json import write_all
    from models.Codebook import Codebook
    from models.FC_Decoder import FC_Decoder
    from utils.model_utils import save_model
    t = str(tmp_path_factory.mktemp("grad_clip_cli"))
    torch.manual_seed(0)
    rng = np.random.default_rng(0)
    recs = []
    for i in range(24):
        p = os.path.join(t, f"z{i}.npy")
        np.save(p, np.tanh(rng.standard_normal((4, 8, 8))).astype(np.float32))
        recs.append({"fmap_path": p, "image_path": ""})
    write_all(f"{t}/fmaps.json", recs)
    dec_cfg = dict(num_layers=2, image_channel=3, min_channel=8, max_channel=16, latent_channel=4,
                   hidden_activation_type="silu", use_final_dec_activation=True, decoder_activation_type="tanh")
    dec = FC_Decoder(num_layers=2, image_channel=3, min_channel=8, max_channel=16, latent_channel=4,
                     hidden_activation_type="silu", use_final_activation=True, final_activation_type="tanh")
    save_model(f"{t}/dec", "model.pt", dict(dec_cfg, model=dec.state_dict()))
    for name, patch, k in (("lr", 8, 8), ("hr", 2, 16)):
        cb = Codebook(patch_dim=(patch, patch), image_dim=(8, 8), image_channel=4, num_embeddings=k)
        with torch.no_grad():
            cb.codebook.weight.copy_(torch.tanh(torch.randn(cb.codebook.weight.shape)))
        save_model(f"{t}/cb_{name}", "codebook.pt",
                   dict(patch_dim=(patch, patch), image_dim=(8, 8), image_C=4, num_embeddings=k,
                        neighbourhood_range=1, global_steps=0, checkpoint=cb.state_dict()))
    json.dump(dict(model_lr=1e-3, num_enc_layers=1, num_dec_layers=2, cross_attn_heads=2, self_attn_heads=4,
                   in_dim=32, hidden_dim=64, hidden_activation="silu", use_sliding_window=False,
                   sliding_window=None), open(f"{t}/t_base.json", "w"))
    common = ["--device", "cuda", "--dataset-path", f"{t}/fmaps.json", "--decoder-path",
              f"{t}/dec/models_checkpoint/model.pt", "--batch-size", 4, "--checkpoint-step", 4, "--max-epoch", 1,
              "--test-num-sample", 3, "--train-base-model", "--lr-codebook-path",
              f"{t}/cb_lr/models_checkpoint/codebook.pt", "--hr-codebook-path",
              f"{t}/cb_hr/models_checkpoint/codebook.pt", "--config-path", f"{t}/t_base.json", "--max-steps", 6]
    out_on = _run("train_quantized_transformer.py", *common, "--out-dir", f"{t}/on", "--clip-grad-norm", 0.01,
                  "--max-skipped-steps", 2, cwd=t)
    out_off = _run("train_quantized_transformer.py", *common, "--out-dir", f"{t}/off", cwd=t)
    return dict(t=t, common=common, out_on=out_on.stdout + out_on.stderr, out_off=out_off.stdout + out_off.stderr)


def _step_lines(out):
    return [ln for ln in out.splitlines() if "Cum. Steps:" in ln]


def test_cli_with_the_flag(runs):
    t = runs["t"]
    md = torch.load(f"{t}/on/models_checkpoint/model_4.pt", map_location="cpu", weights_only=True)
    assert set(md) == BASE_KEYS | {"clip_grad_norm"} and md["clip_grad_norm"] == 0.01
    out = runs["out_on"]
    lines = _step_lines(out)
    assert len(lines) == 6
    block = out[out.index("Training Parameters."):out.index("Sampling Parameters.")]
    assert "Clip Grad Norm: 0.01" in block and "Max Skipped Steps: 2" in block
    clipped = []
    for ln in lines:
        tail = ln.split("Recon Loss: ")[1]
        assert 0 < float(tail.split(" |")[0]) < 100
        fields = [f.strip() for f in tail.split(" | ")[1:]]
        assert [f.split(":")[0] for f in fields] == ["Grad Norm", "Clipped", "Skipped"], ln
        norm, c, s = (f.split(": ")[1] for f in fields)
        assert float(norm) > 0 and np.isfinite(float(norm)) and int(s) == 0
        clipped.append(int(c))
    # a classifier over 17 symbols six steps from its initialisation: every gradient norm is far above 0.01
    assert clipped == [1, 2, 3, 4, 5, 6]


def test_cli_without_the_flag_nothing_is_added(runs):
    t = runs["t"]
    md = torch.load(f"{t}/off/models_checkpoint/model_4.pt", map_location="cpu", weights_only=True)
    assert set(md) == BASE_KEYS
    out = runs["out_off"]
    assert "Clip Grad Norm" not in out and "Max Skipped" not in out and "Grad Norm" not in out
    lines = _step_lines(out)
    assert len(lines) == 6
    for ln in lines:
        assert ln.rstrip().split(" | ")[-1].startswith("Recon Loss: ")


@pytest.mark.parametrize("flags", [("--clip-grad-norm", "0"), ("--clip-grad-norm", "-2"),
                                   ("--clip-grad-norm", "nan"), ("--clip-grad-norm", "1", "--max-skipped-steps", "-1")])
def test_cli_refuses_values_out_of_range(runs, flags):
    r = _run("train_quantized_transformer.py", *runs["common"], "--out-dir", f"{runs['t']}/bad", *flags,
             cwd=runs["t"], ok=False)
    assert r.returncode != 0
    assert not os.path.exists(f"{runs['t']}/bad/models_checkpoint")
