"""AdamW above the kernel, on the GPU at the small models of tests/test_gpu_dropout_train.py: what
FlatAdam.enable_weight_decay decays, which entry a step calls, graph replay against eager steps under a schedule
that changes the learning rate every step, the model against the fp64 definition fed its own gradients, resuming,
the refusals, and the command line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import adamw_cases as C
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


def _optimizer(m, decay=LAM, ema=None):
    from qarig.optim import FlatAdam, decay_parameters
    opt = FlatAdam(m.parameters(), lr=1e-3, betas=(0.5, 0.999))
    if ema is not None:
        opt.enable_ema(ema)
    if decay:
        opt.enable_weight_decay(decay, decay_parameters(m))
    return opt


def _data(k=0):
    g = torch.Generator().manual_seed(20 + k)
    x_dec = torch.randint(0, V_DEC, (N, S), generator=g).cuda()
    x_enc = torch.randint(0, V_ENC, (N, S), generator=g).cuda()
    tgt = torch.randint(0, V_OUT, (N, S), generator=g).cuda()
    pos = (torch.randint(0, 5, (N, 1), generator=g) + torch.arange(S)[None]).cuda()
    return x_dec, x_enc, tgt, pos


# ---- 1: what is decayed ----------------------------------------------------------------------------------------
def test_zero_gradient_step_moves_exactly_the_linear_weights():
    m = _model()
    opt = _optimizer(m)
    assert opt.param_groups[0]["weight_decay"] == LAM
    assert opt.decay_mask.dtype == torch.uint8 and opt.decay_mask.numel() == opt.total // 8
    linear = {id(mod.weight) for mod in m.modules() if isinstance(mod, torch.nn.Linear)}
    before = opt.flat_param.clone()
    opt.zero_grad()
    opt.step()
    c = C.f32(1e-3 * LAM)
    moved = 0
    for name, p in m.named_parameters():
        i = [id(q) for q in opt.params].index(id(p))
        o, n = opt.offsets[i], p.numel()
        old = before[o:o + n]
        if id(p) in linear:
            want = (old.double() * (-c) + old.double()).float()         # the fma: exact product, one rounding
            assert _same_bits(p.detach().flatten(), want), name
            assert not _same_bits(p.detach().flatten(), old), name
            moved += 1
        else:
            assert _same_bits(p.detach().flatten(), old), name
    assert moved == len(linear) > 0 and moved < len(opt.params)
    # the alignment padding between the slices holds zeros, decayed or not
    used = torch.zeros(opt.total, dtype=torch.bool, device="cuda")
    for p, o in zip(opt.params, opt.offsets):
        used[o:o + p.numel()] = True
    assert not opt.flat_param[~used].any()


# ---- 2: which entry a step calls -------------------------------------------------------------------------------
@pytest.mark.parametrize("ema", [None, 0.999])
def test_without_weight_decay_the_step_calls_the_plain_entries(monkeypatch, ema):
    from qarig import _lib, ops
    calls = []
    for name in ("adam_step", "adam_ema_step", "adamw_step"):
        real = getattr(ops, name)
        monkeypatch.setattr(ops, name, (lambda real, name: lambda *a, **k: (calls.append(name), real(*a, **k))[1])(
            real, name))
    m = _model()
    plain = _optimizer(m, decay=0, ema=ema)
    assert plain.decay_mask is None and plain.param_groups[0]["weight_decay"] == 0
    before = _lib.N_CALLS
    plain.step()
    plain.advance_captured()        # (fills the scalar buffer the captured form of the launch reads)
    plain.step_captured()
    assert calls == ["adam_step" if ema is None else "adam_ema_step"] * 2 and _lib.N_CALLS - before == 2
    assert plain._dev_step_buffer().numel() == (2 if ema is None else 3)
    del calls[:]
    decayed = _optimizer(_model(), ema=ema)
    before = _lib.N_CALLS
    decayed.step()
    decayed.advance_captured()
    decayed.step_captured()
    assert calls == ["adamw_step"] * 2 and _lib.N_CALLS - before == 2
    assert decayed._dev_step_buffer().numel() == 4


# ---- 3: graph replay against eager steps under a schedule ------------------------------------------------------
def _build_pipeline(decay, ema):
    from models.Codebook import Codebook
    g = torch.Generator().manual_seed(4)
    lr_cb = Codebook(patch_dim=(4, 4), image_dim=(8, 8), image_channel=4, num_embeddings=V_ENC).cuda()
    hr_cb = Codebook(patch_dim=(2, 2), image_dim=(8, 8), image_channel=4, num_embeddings=V_OUT - 1).cuda()
    with torch.no_grad():
        lr_cb.codebook.weight.copy_(torch.tanh(torch.randn(lr_cb.codebook.weight.shape, generator=g)))
        hr_cb.codebook.weight.copy_(torch.tanh(torch.randn(hr_cb.codebook.weight.shape, generator=g)))
    m = _model()
    m.train()
    return lr_cb, hr_cb, m, _optimizer(m, decay=decay, ema=ema)


def _batches(n=5):
    g = torch.Generator().manual_seed(9)
    return [(torch.tanh(torch.randn((N, 4, 8, 8), generator=g)), torch.randint(0, 17 - S + 1, (N,), generator=g))
            for _ in range(n)]


def _schedule():
    from qarig.optim import LRSchedule
    return LRSchedule(1e-3, "cosine", warmup_steps=2, decay_steps=5)


def _eager(decay, ema):
    from qarig import pipeline
    lr_cb, hr_cb, m, opt = _build_pipeline(decay, ema)
    sched, lrs = _schedule(), []
    for z, rand in _batches():
        opt.param_groups[0]["lr"] = sched.lr(opt.step_count + 1)
        lrs.append(opt.param_groups[0]["lr"])
        hr_in, lr_in, hr_tg = pipeline.tokenize(z.cuda(), lr_cb, hr_cb, False)
        hr_in, hr_tg, pos = pipeline.slide(hr_in, hr_tg, S, rand)
        pipeline.train_step(m, opt, hr_in, lr_in, hr_tg, pos, dp=False, pos_bound=17)
    return opt, lrs


@pytest.mark.parametrize("ema", [None, 0.999])
def test_graph_replay_matches_eager_steps_under_a_schedule(ema):
    from qarig import pipeline
    opt_e, lrs = _eager(LAM, ema)
    assert lrs[0] == 0.5e-3 and lrs[1] == lrs[2] == 1e-3 > lrs[3] > lrs[4] > 0       # the rate keeps changing
    lr_cb, hr_cb, m, opt_g = _build_pipeline(LAM, ema)
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
    assert float(opt_g._dev_step[3]) == C.f32(lrs[-1] * LAM)
    assert float(opt_g._dev_step[0]) == C.f32(lrs[-1] / (1 - 0.5 ** 5))
    opt_off, _ = _eager(0, ema)                       # and the decay did arrive
    assert not _same_bits(opt_off.flat_param, opt_e.flat_param)


# ---- 4: the model against the fp64 definition fed its own gradients --------------------------------------------
def test_three_model_steps_against_the_fp64_definition():
    from qarig import functional as QF
    m = _model()
    m.train()
    opt = _optimizer(m, ema=0.9)
    p0, e0 = opt.flat_param.clone(), opt.flat_ema.clone()
    from qarig.optim import ema_weight
    grads, got, scalars = [], [], []
    for t in range(1, 4):
        x_dec, x_enc, tgt, pos = _data(t)
        opt.zero_grad()
        logits = m(x_dec=x_dec, x_enc=x_enc, pos_cond=pos, pos_bound=S + 5)
        QF.cross_entropy(logits.view(-1, V_OUT), tgt.flatten()).backward()
        grads.append(opt.flat_grad.clone())
        scalars.append(C.step_scalars(t, 1e-3, LAM, (0.5, 0.999), ema_weight(t - 1, 0.9, True)))
        opt.step()
        got.append(dict(p=opt.flat_param.clone(), m=opt.exp_avg.clone(), v=opt.exp_avg_sq.clone(),
                        ema=opt.flat_ema.clone()))
    assert all(bool(g.any()) for g in grads)
    ref = C.adamw_ref64(p0, grads, opt.decay_mask, scalars, C.f32(0.5), C.f32(0.999), C.f32(1e-8), 1.0, ema=e0)
    r = C.worst_ratios(ref, got)
    print("adamw model, 3 steps, {} elements: worst / bound  p {:.4f}  m {:.4f}  v {:.4f}  ema {:.4f}".format(
        opt.total, r["p"], r["m"], r["v"], r["ema"]))
    assert all(0.0 <= x <= 1.0 for x in r.values()), r
    # the same gradients without the decay end elsewhere, by far more than the tolerance
    plain = C.adamw_ref64(p0, grads, torch.zeros_like(opt.decay_mask), scalars, C.f32(0.5), C.f32(0.999), C.f32(1e-8),
                          1.0, ema=e0)
    assert C.worst_ratios(plain, got)["p"] > 1.0


# ---- 5: a state round trip ------------------------------------------------------------------------------------
def _synthetic_grads(opt, k):
    g = torch.Generator(device="cuda").manual_seed(100 + k)
    for q in opt.params:            # (the alignment padding between the slices keeps its zero gradient)
        q.grad.copy_(torch.randn(q.shape, device="cuda", generator=g) * 0.01)


def test_state_round_trip_continues_bitwise():
    sched = _schedule()

    def run(opt, ks):
        for k in ks:
            opt.param_groups[0]["lr"] = sched.lr(opt.step_count + 1)
            _synthetic_grads(opt, k)
            opt.step()

    opt = _optimizer(_model())
    run(opt, range(5))
    m1 = _model()
    opt1 = _optimizer(m1)
    run(opt1, range(2))
    saved = {"model": {k: v.detach().clone().cpu() for k, v in m1.state_dict().items()},
             "model_optimizer": opt1.state_dict()}
    assert saved["model_optimizer"]["param_groups"][0]["weight_decay"] == LAM
    saved["model_optimizer"]["param_groups"][0]["weight_decay"] = 0.5          # ignored on load: the caller governs
    m2 = _model()
    m2.load_state_dict(saved["model"])
    opt2 = _optimizer(m2, decay=0)
    opt2.load_state_dict(saved["model_optimizer"])
    assert opt2.step_count == 2 and opt2.param_groups[0]["weight_decay"] == 0 and opt2.decay_mask is None
    from qarig.optim import decay_parameters
    opt2.enable_weight_decay(LAM, decay_parameters(m2))
    run(opt2, range(2, 5))
    assert opt2.step_count == 5 and _same_bits(opt2.flat_param, opt.flat_param)
    assert _same_bits(opt2.exp_avg, opt.exp_avg) and _same_bits(opt2.exp_avg_sq, opt.exp_avg_sq)


# ---- 6: refusals ----------------------------------------------------------------------------------------------
def test_enable_weight_decay_refusals():
    from qarig import pipeline
    from qarig.optim import decay_parameters
    lr_cb, hr_cb, m, opt = _build_pipeline(0, 0.9)
    with pytest.raises(ValueError):
        opt.enable_weight_decay(LAM, [torch.nn.Parameter(torch.zeros(8, device="cuda"))])      # not owned
    with pytest.raises(ValueError):
        opt.enable_weight_decay(0.0, decay_parameters(m))
    with opt.ema_weights():
        with pytest.raises(RuntimeError, match="ema_weights"):
            opt.enable_weight_decay(LAM, decay_parameters(m))
    assert opt.decay_mask is None
    step = pipeline.GraphedTrainStep(m, opt, lr_cb, hr_cb, False, S, warmup=1)
    for z, rand in _batches(2):
        step(z.cuda(), rand)
    assert step.graph is not None
    with pytest.raises(RuntimeError, match="captured"):
        opt.enable_weight_decay(LAM, decay_parameters(m))
    assert opt.decay_mask is None and opt.param_groups[0]["weight_decay"] == 0


# ---- 7: the command line: the fixtures of tests/test_gpu_dropout_train.py, copied -------------------------------
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
    t = str(tmp_path_factory.mktemp("adamw_cli"))
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
    out_on = _run("train_quantized_transformer.py", *common, "--out-dir", f"{t}/on", "--weight-decay", 0.01,
                  "--lr-schedule", "cosine", "--lr-warmup-steps", 2, "--lr-decay-steps", 6, cwd=t)
    out_off = _run("train_quantized_transformer.py", *common, "--out-dir", f"{t}/off", cwd=t)
    return dict(t=t, common=common, out_on=out_on.stdout + out_on.stderr, out_off=out_off.stdout + out_off.stderr)


def _step_lines(out):
    return [ln for ln in out.splitlines() if "Cum. Steps:" in ln]


def test_cli_with_the_flags(runs):
    from qarig.optim import LRSchedule
    t = runs["t"]
    md = torch.load(f"{t}/on/models_checkpoint/model_4.pt", map_location="cpu", weights_only=True)
    assert set(md) == BASE_KEYS | {"weight_decay", "lr_schedule", "lr_warmup_steps", "lr_decay_steps", "lr_min_ratio"}
    assert md["weight_decay"] == 0.01 and md["lr_schedule"] == "cosine" and md["lr_warmup_steps"] == 2
    assert md["lr_decay_steps"] == 6 and md["lr_min_ratio"] == 0.0
    assert md["model_optimizer"]["param_groups"][0]["weight_decay"] == 0.01
    out = runs["out_on"]
    lines = _step_lines(out)
    assert len(lines) == 6
    sched = LRSchedule(1e-3, "cosine", warmup_steps=2, decay_steps=6)
    logged = [ln.split("L.R.: ")[1].split(" |")[0] for ln in lines]
    assert logged == ["{:.8f}".format(sched.lr(k)) for k in range(1, 7)]
    # half the base rate in the warm-up, the base rate at its end and at u = 0, then down the cosine
    assert logged[0] == "0.00050000" and logged[1] == logged[2] == "0.00100000"
    assert 1e-3 > float(logged[3]) > float(logged[4]) > float(logged[5]) > 0
    block = out[out.index("Training Parameters."):out.index("Sampling Parameters.")]
    for text in ("Weight Decay: 0.01", "LR Schedule: cosine", "LR Warmup Steps: 2", "LR Decay Steps: 6",
                 "LR Min Ratio: 0.0"):
        assert text in block, text
    for ln in lines:
        assert 0 < float(ln.split("Recon Loss: ")[1].split(" |")[0]) < 100


def test_cli_without_the_flags_nothing_is_added(runs):
    t = runs["t"]
    md = torch.load(f"{t}/off/models_checkpoint/model_4.pt", map_location="cpu", weights_only=True)
    assert set(md) == BASE_KEYS
    assert md["model_optimizer"]["param_groups"][0]["weight_decay"] == 0
    out = runs["out_off"]
    assert "Weight Decay" not in out and "LR Schedule" not in out and "LR Warmup" not in out
    lines = _step_lines(out)
    assert len(lines) == 6 and all("L.R.: 0.00100000" in ln for ln in lines)


@pytest.mark.parametrize("flags", [("--weight-decay", "1.5"), ("--lr-schedule", "cosine"),
                                   ("--lr-schedule", "cosine", "--lr-warmup-steps", "5", "--lr-decay-steps", "4")])
def test_cli_refuses_values_out_of_range(runs, flags):
    r = _run("train_quantized_transformer.py", *runs["common"], "--out-dir", f"{runs['t']}/bad", *flags,
             cwd=runs["t"], ok=False)
    assert r.returncode != 0
    assert not os.path.exists(f"{runs['t']}/bad/models_checkpoint")
