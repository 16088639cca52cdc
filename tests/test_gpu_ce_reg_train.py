"""Label smoothing and z-loss through the layers above the kernel, on the GPU at tiny shapes (32 wide, 2 layers,
17 tokens in windows of 12, batch 6): the autograd node of QF.cross_entropy, pipeline.train_step (defaults unchanged,
the {objective, nll} pair against fp64 on the logits of the same forward), pipeline.GraphedTrainStep (replay equals
eager, bit for bit, the pair included) and train_quantized_transformer.py --label-smoothing / --z-loss (log lines,
checkpoint keys, argparse).  The kernel itself is tests/test_gpu_ce_reg.py's subject."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ce_reg_cases as G
from conftest import PKG

pytestmark = pytest.mark.gpu

EPS, ZETA = 0.1, 1e-4
GI = G.REG_GRID.index((EPS, ZETA))


def _build():
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
    m = Transformer(use_encoder=False, use_pos_cond=True, num_enc_layers=None, num_dec_layers=2, num_enc_embedding=None,
                    num_dec_embedding=48, self_attn_heads=4, cross_attn_heads=None, transformer_in_dim=32,
                    transformer_out_dim=33, transformer_hidden_dim=64).cuda()
    with torch.no_grad():
        for p in m.parameters():
            if p.abs().max() == 0:
                p.copy_(torch.randn(p.shape, generator=g) * 0.05)
    return lr_cb, hr_cb, m, FlatAdam(m.parameters(), lr=1e-3, betas=(0.5, 0.999))


def _batches(n):
    g = torch.Generator().manual_seed(9)
    return [(torch.tanh(torch.randn((6, 4, 8, 8), generator=g)), torch.randint(0, 17 - 12 + 1, (6,), generator=g))
            for _ in range(n)]


def _eager(n, **reg):
    """n eager steps: (flat_param, [loss as float], [pair as list])."""
    from qarig import pipeline
    lr_cb, hr_cb, m, opt = _build()
    losses, pairs = [], []
    for z, rand in _batches(n):
        hr_in, lr_in, hr_tg = pipeline.tokenize(z.cuda(), lr_cb, hr_cb, True)
        hr_in, hr_tg, pos = pipeline.slide(hr_in, hr_tg, 12, rand)
        loss = pipeline.train_step(m, opt, hr_in, lr_in, hr_tg, pos, dp=False, pos_bound=17, **reg)
        assert loss.dim() == 0 and loss.is_cuda
        pair = pipeline.loss_pair(loss)
        assert pair.shape == (2,) and pair.is_cuda and not pair.requires_grad
        losses.append(float(loss.detach()))
        pairs.append(pair.tolist())
    return opt.flat_param.detach().clone(), losses, pairs


def test_autograd_node():
    """QF.cross_entropy with regularisers: objective and nll are the ops outputs, the gradient of 0.5 loss is
    ops.scale_by(dlogits, 0.5), bit for bit; with both 0 it is the plain node."""
    from qarig import functional as QF
    from qarig import ops
    g = torch.Generator().manual_seed(11)
    x = (2.0 * torch.randn((6, 12, 33), generator=g)).cuda()
    t = torch.randint(0, 33, (6, 12), generator=g).cuda()
    pair, dl = ops.cross_entropy_fwd(x.view(-1, 33), t.flatten(), EPS, ZETA)
    assert pair.shape == (2,) and dl.shape == (72, 33)
    pair0, none = ops.cross_entropy_fwd(x.view(-1, 33), t.flatten(), EPS, ZETA, want_grad=False)
    assert none is None and torch.equal(pair0, pair)
    logits = x.clone().requires_grad_(True)
    loss = QF.cross_entropy(logits, t, EPS, ZETA)
    assert loss.dim() == 0 and loss.requires_grad
    assert torch.equal(loss.detach(), pair[0]) and torch.equal(loss.nll, pair[1]) and torch.equal(loss.pair, pair)
    assert not loss.nll.requires_grad and not loss.pair.requires_grad
    assert torch.equal(QF.loss_pair(loss), pair)
    (0.5 * loss).backward()
    want = ops.scale_by(dl, torch.tensor([0.5], device="cuda")).view(6, 12, 33)
    assert torch.equal(logits.grad, want)
    # against fp64 within the means' tolerance, on the logits' own rows
    ref = G.reg_ref_uncached(x.view(-1, 33).cpu(), t.flatten().cpu(), EPS, ZETA)
    for k, got, rows in (("mean_obj", pair[0], ref["obj"]), ("mean_nll", pair[1], ref["nll"])):
        err = float((got.cpu().double() - ref[k]).abs() / (G.U * rows.abs().mean()))
        print(f"MEASURED ce_reg_node {k} {err:.3f} {G.reg_tol((k, GI))}")
        assert err <= G.reg_tol((k, GI))
    # both 0: the plain node and entry, and the pair is the loss seen twice
    l0 = x.clone().requires_grad_(True)
    plain = QF.cross_entropy(l0, t)
    same = QF.cross_entropy(x.clone().requires_grad_(True), t, 0.0, 0.0)
    assert type(plain.grad_fn).__name__ == type(same.grad_fn).__name__ != type(loss.grad_fn).__name__
    assert torch.equal(plain, same) and not hasattr(plain, "pair")
    assert torch.equal(QF.loss_pair(plain), torch.stack([plain.detach(), plain.detach()]))
    for bad in ((1.0, 0.0), (-0.1, 0.0), (0.0, -1.0), (0.0, float("inf")), (float("nan"), 0.0)):
        with pytest.raises(ValueError):
            QF.cross_entropy(l0, t, *bad)


def test_train_step_defaults_unchanged_and_pair_against_fp64(monkeypatch):
    from qarig import functional as QF
    default, losses_d, pairs_d = _eager(3)
    zero, losses_z, pairs_z = _eager(3, label_smoothing=0.0, z_loss=0.0)
    assert torch.equal(default, zero) and losses_d == losses_z
    assert pairs_d == [[v, v] for v in losses_d] == pairs_z
    seen = []
    real = QF.cross_entropy

    def spy(logits, target, *a, **k):
        seen.append((logits.detach().clone(), target.detach().clone()))
        return real(logits, target, *a, **k)

    monkeypatch.setattr(QF, "cross_entropy", spy)
    reg, losses_r, pairs_r = _eager(3, label_smoothing=EPS, z_loss=ZETA)
    monkeypatch.setattr(QF, "cross_entropy", real)
    assert not torch.equal(reg, default)
    assert len(seen) == 3 and [p[0] for p in pairs_r] == losses_r
    for (logits, target), (obj, nll) in zip(seen, pairs_r):
        assert logits.shape == (72, 33)
        ref = G.reg_ref_uncached(logits.cpu(), target.cpu(), EPS, ZETA)
        for k, got, rows in (("mean_obj", obj, ref["obj"]), ("mean_nll", nll, ref["nll"])):
            err = float(abs(got - float(ref[k])) / (G.U * float(rows.abs().mean())))
            print(f"MEASURED ce_reg_train_step {k} {err:.3f} {G.reg_tol((k, GI))}")
            assert err <= G.reg_tol((k, GI)), (k, got, float(ref[k]))
        assert obj != nll


def test_graph_replay_matches_eager_steps():
    """Five GraphedTrainStep steps at (0.1, 1e-4), warm-up 2 then replay: the weights and the per-step
    {objective, nll} pairs of five eager steps, bit for bit; the pair is the graph's static output."""
    from qarig import pipeline
    want, losses_e, pairs_e = _eager(5, label_smoothing=EPS, z_loss=ZETA)
    lr_cb, hr_cb, m, opt = _build()
    step = pipeline.GraphedTrainStep(m, opt, lr_cb, hr_cb, True, 12, warmup=2, label_smoothing=EPS, z_loss=ZETA)
    losses_g, pairs_g, ptrs = [], [], []
    for z, rand in _batches(5):
        loss = step(z.cuda(), rand)
        pair = pipeline.loss_pair(loss)
        losses_g.append(float(loss))
        pairs_g.append(pair.tolist())
        ptrs.append((loss.data_ptr(), pair.data_ptr()))
    assert step.graph is not None and opt.step_count == 5
    assert torch.equal(opt.flat_param, want)
    assert losses_g == losses_e and pairs_g == pairs_e
    assert ptrs[2] == ptrs[3] == ptrs[4] and ptrs[2][0] == ptrs[2][1]      # static: the loss is the pair's first float
    with pytest.raises(ValueError):
        pipeline.GraphedTrainStep(m, opt, lr_cb, hr_cb, True, 12, label_smoothing=1.0)


# ---- the command line: the fixtures of tests/test_gpu_ema_cli.py, copied --------------------------------------

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
    t = str(tmp_path_factory.mktemp("ce_reg_cli"))
    torch.manual_seed(0)
    rng = np.random.default_rng(0)
    recs = []
    for i in range(12):
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
              f"{t}/dec/models_checkpoint/model.pt", "--batch-size", 4, "--checkpoint-step", 2, "--max-epoch", 1,
              "--test-num-sample", 3, "--train-base-model", "--lr-codebook-path",
              f"{t}/cb_lr/models_checkpoint/codebook.pt", "--hr-codebook-path",
              f"{t}/cb_hr/models_checkpoint/codebook.pt", "--config-path", f"{t}/t_base.json", "--max-steps", 3]
    out_reg = _run("train_quantized_transformer.py", *common, "--out-dir", f"{t}/reg", "--label-smoothing", EPS,
                   "--z-loss", ZETA, cwd=t)
    out_off = _run("train_quantized_transformer.py", *common, "--out-dir", f"{t}/off", cwd=t)
    return dict(t=t, common=common, out_reg=out_reg.stdout + out_reg.stderr, out_off=out_off.stdout + out_off.stderr)


def test_cli_with_the_flags(runs):
    t = runs["t"]
    md = torch.load(f"{t}/reg/models_checkpoint/model_2.pt", map_location="cpu", weights_only=True)
    assert set(md) == BASE_KEYS | {"label_smoothing", "z_loss"}
    assert md["label_smoothing"] == EPS and md["z_loss"] == ZETA
    assert type(md["label_smoothing"]) is float and type(md["z_loss"]) is float
    out = runs["out_reg"]
    steps = [ln for ln in out.splitlines() if "Cum. Steps:" in ln]
    assert len(steps) == 3 and all("| Recon Loss: " in ln and "| NLL: " in ln for ln in steps)
    for ln in steps:       # two numbers, both finite, not the same one twice
        obj, nll = float(ln.split("Recon Loss: ")[1].split(" |")[0]), float(ln.split("NLL: ")[1])
        assert 0 < nll < 100 and 0 < obj < 100 and obj != nll
    block = out[out.index("Training Parameters."):out.index("Sampling Parameters.")]
    assert f"Label Smoothing: {EPS}" in block and f"Z-Loss: {ZETA}" in block


def test_cli_without_the_flags_nothing_is_added(runs):
    t = runs["t"]
    md = torch.load(f"{t}/off/models_checkpoint/model_2.pt", map_location="cpu", weights_only=True)
    assert set(md) == BASE_KEYS
    out = runs["out_off"]
    assert "NLL" not in out and "Label Smoothing" not in out and "Z-Loss" not in out
    assert len([ln for ln in out.splitlines() if "Cum. Steps:" in ln]) == 3


@pytest.mark.parametrize("flag,value", [("--label-smoothing", "1.0"), ("--z-loss", "-1")])
def test_cli_refuses_values_out_of_range(runs, flag, value):
    r = _run("train_quantized_transformer.py", *runs["common"], "--out-dir", f"{runs['t']}/refused", flag, value,
             cwd=runs["t"], ok=False)
    assert r.returncode == 2 and flag in r.stderr and "usage:" in r.stderr
    assert not os.path.exists(f"{runs['t']}/refused")
