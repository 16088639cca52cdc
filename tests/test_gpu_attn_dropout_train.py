"""Attention-probability dropout through the layers above the kernels, on the GPU at a 2-layer encoder-decoder of
width 64 with 8 heads (head dim 8) and 2 x 33 tokens: eager steps against graph replay, with and without activation
checkpointing, ranks and repeats, the paths that must never see it (evaluation, the token scorer, cached generation),
the default step's C-ABI call count, both dropouts under one key, the refusals, and the command line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import PKG

pytestmark = pytest.mark.gpu

P, SEED = 0.25, 0x5EED0123456789
V_ENC, V_DEC, V_OUT, S, N = 16, 40, 33, 33, 2
SEQ = 65                                      # <start> + 64 HR tokens, windows of 33


def _model(ckpt=False):
    from models.Transformer import Transformer
    torch.manual_seed(5)
    m = Transformer(use_encoder=True, use_pos_cond=True, num_enc_layers=2, num_dec_layers=2, num_enc_embedding=V_ENC,
                    num_dec_embedding=V_DEC, self_attn_heads=8, cross_attn_heads=8, transformer_in_dim=64,
                    transformer_out_dim=V_OUT, transformer_hidden_dim=128, use_activation_checkpoint=ckpt).cuda()
    g = torch.Generator().manual_seed(6)
    with torch.no_grad():
        for p in m.parameters():
            if p.abs().max() == 0:
                p.copy_(torch.randn(p.shape, generator=g) * 0.05)
    return m


N_ATTN = 2 + 2 * 2              # encoder self-attention x 2, per decoder block self- and cross-attention


def _data(k=0):
    g = torch.Generator().manual_seed(20 + k)
    x_dec = torch.randint(0, V_DEC, (N, S), generator=g).cuda()
    x_enc = torch.randint(0, V_ENC, (N, 4), generator=g).cuda()
    tgt = torch.randint(0, V_OUT, (N, S), generator=g).cuda()
    pos = (torch.randint(0, 5, (N, 1), generator=g) + torch.arange(S)[None]).cuda()
    return x_dec, x_enc, tgt, pos


def _fwd_bwd(m, data, step=None):
    from qarig import functional as QF
    x_dec, x_enc, tgt, pos = data
    for p in m.parameters():
        p.grad = None
    if step is not None:
        m.dropout_key.set_step(step)
    logits = m(x_dec=x_dec, x_enc=x_enc, pos_cond=pos, pos_bound=S + 5)
    QF.cross_entropy(logits.view(-1, V_OUT), tgt.flatten()).backward()
    return logits.detach().clone(), {k: p.grad.detach().clone() for k, p in m.named_parameters()}


def _build_pipeline(ckpt=False):
    from models.Codebook import Codebook
    from qarig.optim import FlatAdam
    g = torch.Generator().manual_seed(4)
    lr_cb = Codebook(patch_dim=(8, 8), image_dim=(16, 16), image_channel=4, num_embeddings=V_ENC).cuda()
    hr_cb = Codebook(patch_dim=(2, 2), image_dim=(16, 16), image_channel=4, num_embeddings=V_OUT - 1).cuda()
    with torch.no_grad():
        lr_cb.codebook.weight.copy_(torch.tanh(torch.randn(lr_cb.codebook.weight.shape, generator=g)))
        hr_cb.codebook.weight.copy_(torch.tanh(torch.randn(hr_cb.codebook.weight.shape, generator=g)))
    m = _model(ckpt)
    m.train()
    return lr_cb, hr_cb, m, FlatAdam(m.parameters(), lr=1e-3, betas=(0.5, 0.999))


def _batches(n):
    g = torch.Generator().manual_seed(9)
    return [(torch.tanh(torch.randn((N, 4, 16, 16), generator=g)), torch.randint(0, SEQ - S + 1, (N,), generator=g))
            for _ in range(n)]


def _eager_steps(n, prepare, ckpt=False):
    from qarig import _lib, pipeline
    lr_cb, hr_cb, m, opt = _build_pipeline(ckpt)
    prepare(m)
    losses, calls = [], []
    for z, rand in _batches(n):
        hr_in, lr_in, hr_tg = pipeline.tokenize(z.cuda(), lr_cb, hr_cb, False)
        hr_in, hr_tg, pos = pipeline.slide(hr_in, hr_tg, S, rand)
        before = _lib.N_CALLS
        losses.append(float(pipeline.train_step(m, opt, hr_in, lr_in, hr_tg, pos, dp=False, pos_bound=SEQ).detach()))
        calls.append(_lib.N_CALLS - before)
    return opt.flat_param.detach().clone(), losses, calls


def _on(rank=0, p=P):
    return lambda m: m.enable_attention_dropout(p, SEED, rank=rank)


@pytest.fixture(scope="module")
def eager():
    """Three eager steps: attention dropout on at rank 0, never enabled."""
    return {"on": _eager_steps(3, _on()), "never": _eager_steps(3, lambda m: None)}


# ---- steps -------------------------------------------------------------------------------------------------------
def test_it_is_dropout_and_repeats_bit_for_bit(eager):
    flat, losses, calls = eager["on"]
    flat0, losses0, calls0 = eager["never"]
    assert losses != losses0 and not torch.equal(flat, flat0)
    assert calls == calls0                      # the dropout entries replace the plain ones: no further launch
    again = _eager_steps(3, _on())
    assert again[1] == losses and torch.equal(again[0], flat)


def test_two_ranks_draw_different_masks(eager):
    other = _eager_steps(3, _on(rank=1))
    assert other[1] != eager["on"][1]
    assert other[1][0] != eager["on"][1][0]     # already the first loss: same weights, another mask


def test_graph_replay_matches_eager_steps():
    from qarig import pipeline
    want, losses_e, _ = _eager_steps(4, _on())
    lr_cb, hr_cb, m, opt = _build_pipeline()
    key = m.enable_attention_dropout(P, SEED)
    assert key is m.dropout_key
    step = pipeline.GraphedTrainStep(m, opt, lr_cb, hr_cb, False, S, warmup=2)
    losses_g = [float(step(z.cuda(), rand)) for z, rand in _batches(4)]
    assert step.graph is not None and opt.step_count == 4 and key.buffer.tolist()[2] == 4
    assert losses_g == losses_e
    assert torch.equal(opt.flat_param, want)
    # enabling, disabling or re-keying after the capture is refused
    z, rand = _batches(1)[0]
    m.enable_dropout(0.1, SEED)                  # same key object: the captured step must still notice
    with pytest.raises(RuntimeError):
        step(z.cuda(), rand)
    m.disable_dropout()
    m.disable_attention_dropout()
    with pytest.raises(RuntimeError):
        step(z.cuda(), rand)


def test_activation_checkpoint_regenerates_the_mask():
    """Gradients with use_activation_checkpoint against without: every parameter whose gradient is bit-identical
    between the two with dropout off on this build (measured first) must be bit-identical with it on."""
    data = _data(3)
    same_at = {}
    for p in (0.0, P):
        out = []
        for ckpt in (False, True):
            m = _model(ckpt=ckpt)
            m.train()
            if p:
                m.enable_attention_dropout(p, SEED)
            out.append(_fwd_bwd(m, data, step=2 if p else None))
        (l0, g0), (l1, g1) = out
        same_at[p] = {k for k in g0 if torch.equal(g0[k], g1[k])}
        print(f"MEASURED checkpoint vs plain at p={p}: {len(same_at[p])} of {len(g0)} gradients bit-identical")
        assert torch.equal(l0, l1)
    assert len(same_at[0.0]) > 0
    assert same_at[0.0] <= same_at[P], sorted(same_at[0.0] - same_at[P])
    # whole steps: losses and parameters
    a, b = _eager_steps(3, _on()), _eager_steps(3, _on(), ckpt=True)
    plain = _eager_steps(3, lambda m: None, ckpt=True)
    never = _eager_steps(3, lambda m: None)
    # the control: with dropout off the checkpointed steps equal the plain ones bit for bit on this build (all
    # 162 gradients above), so the comparison below holds for all three steps and is never skipped
    assert plain[1] == never[1] and torch.equal(plain[0], never[0])
    assert a[1] == b[1] and torch.equal(a[0], b[0])


def test_the_mask_follows_the_step_word():
    m = _model()
    m.train()
    m.enable_attention_dropout(P, SEED)
    data = _data(1)
    l4, g4 = _fwd_bwd(m, data, step=4)
    l5, _ = _fwd_bwd(m, data, step=5)
    l4b, g4b = _fwd_bwd(m, data, step=4)
    assert not torch.equal(l4, l5) and torch.equal(l4, l4b)
    assert all(torch.equal(g4[k], g4b[k]) for k in g4)


# ---- the paths that never see it ---------------------------------------------------------------------------------
def test_eval_scorer_and_generation_are_untouched(monkeypatch):
    from qarig import _lib, ops, sampling
    from qarig.evaluate import TokenScorer
    lr_cb, hr_cb, plain, _ = _build_pipeline()
    dropped = _model()
    dropped.enable_attention_dropout(P, SEED)
    seen = []
    real_fwd = ops.attention_fwd

    def spy(*a, **k):
        seen.append(k.get("dropout", a[6] if len(a) > 6 else None))
        return real_fwd(*a, **k)

    monkeypatch.setattr(ops, "attention_fwd", spy)
    x_dec, x_enc, tgt, pos = _data(1)
    for m in (plain, dropped):
        m.eval()
    outs = [m(x_dec=x_dec, x_enc=x_enc, pos_cond=pos, pos_bound=S + 5) for m in (plain, dropped)]    # gradients on
    assert torch.equal(*outs)
    for m in (plain, dropped):
        m.train()
    with torch.no_grad():
        outs = [m(x_dec=x_dec, x_enc=x_enc, pos_cond=pos, pos_bound=S + 5) for m in (plain, dropped)]
    assert torch.equal(*outs)
    z = _batches(1)[0][0].cuda()
    res = []
    for m in (plain, dropped):
        sc = TokenScorer(m, lr_cb, hr_cb, False, S)
        sc.add_batch(z)
        res.append(sc.result())
    assert res[0] == res[1] and res[0]["tokens"] > 0
    first = torch.full((N, 1), V_OUT - 1, dtype=torch.int64).cuda()
    toks = []
    for m in (plain, dropped):
        m.eval()
        torch.manual_seed(3)
        with torch.no_grad():
            toks.append(sampling.generate_tokens(m, first, x_enc, 12, 0.05, True, S, end_token=V_DEC,
                                                 mode="generate", use_kv_cache=True))
    assert torch.equal(*toks)
    assert seen and all(d is None for d in seen)
    dropped.train()                                     # the control: a training forward does pass it
    dropped.dropout_key.set_step(1)
    dropped(x_dec=x_dec, x_enc=x_enc, pos_cond=pos, pos_bound=S + 5)
    assert [d is not None for d in seen[-N_ATTN:]] == [True] * N_ATTN
    assert sorted(d[2] for d in seen[-N_ATTN:]) == list(range(N_ATTN))


def test_train_step_with_p_zero_is_the_default_step(eager):
    never = eager["never"]
    zero = _eager_steps(3, lambda m: m.enable_attention_dropout(0.0, SEED))
    off_again = _eager_steps(3, lambda m: (m.enable_attention_dropout(P, SEED), m.disable_attention_dropout()))
    for other in (zero, off_again):
        assert other[2] == never[2] and other[1] == never[1] and torch.equal(other[0], never[0])
    m = _model()
    assert m.enable_attention_dropout(0, SEED) is None and m.dropout_key is None
    sd = set(m.state_dict())
    m.enable_attention_dropout(0.5, 1)
    assert set(m.state_dict()) == sd


# ---- one key for both features --------------------------------------------------------------------------------------
def test_both_dropouts_share_one_key(eager):
    both = _eager_steps(3, lambda m: (m.enable_dropout(0.1, SEED), m.enable_attention_dropout(P, SEED)))
    only_res = _eager_steps(3, lambda m: m.enable_dropout(0.1, SEED))
    assert all(np.isfinite(both[1]))
    assert both[1] != only_res[1] and both[1] != eager["on"][1]
    for first, second in (("enable_dropout", "enable_attention_dropout"), ("enable_attention_dropout", "enable_dropout")):
        m = _model()
        key = getattr(m, first)(0.1, SEED, rank=2)
        assert getattr(m, second)(0.2, SEED, rank=2) is key and m.dropout_key is key
        for bad in ((SEED + 1, 2), (SEED, 3)):
            with pytest.raises(ValueError):
                getattr(m, second)(0.2, bad[0], rank=bad[1])
    m = _model()
    m.enable_dropout(0.1, SEED)
    m.enable_attention_dropout(P, SEED)
    key = m.dropout_key
    m.disable_dropout()
    assert m.dropout_key is key                   # attention dropout still holds it
    m.disable_attention_dropout()
    assert m.dropout_key is None
    for bad in (1e-6, 0.91, 1.0, float("nan"), -0.1):
        with pytest.raises(ValueError):
            m.enable_attention_dropout(bad, 0)


def test_head_dim_128_models_are_refused_at_enable():
    from models.Transformer import Transformer
    m = Transformer(use_encoder=False, use_pos_cond=False, num_enc_layers=None, num_dec_layers=1,
                    num_enc_embedding=None, num_dec_embedding=V_DEC, self_attn_heads=1, cross_attn_heads=None,
                    transformer_in_dim=128, transformer_out_dim=V_OUT, transformer_hidden_dim=128).cuda()
    with pytest.raises(ValueError, match="128"):
        m.enable_attention_dropout(0.1, 0)
    assert m.dropout_key is None


# ---- the command line: the fixtures of tests/test_gpu_dropout_train.py, copied ---------------------------------
BASE_KEYS = {"train_base_model", "use_sliding_window", "sliding_window", "num_enc_embedding", "num_dec_embedding",
             "num_enc_layers", "num_dec_layers", "self_attn_heads", "cross_attn_heads", "transformer_in_dim",
             "transformer_out_dim", "transformer_hidden_dim", "hidden_activation", "model", "model_optimizer"}


def test_cli_with_the_flag(tmp_path):
    sys.path.insert(0, PKG)
    from dataset_loader._tinydb_json import write_all
    from models.Codebook import Codebook
    from models.FC_Decoder import FC_Decoder
    from utils.model_utils import save_model
    t = str(tmp_path)
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
    args = ["--device", "cuda", "--dataset-path", f"{t}/fmaps.json", "--decoder-path",
            f"{t}/dec/models_checkpoint/model.pt", "--batch-size", 4, "--checkpoint-step", 1, "--max-epoch", 1,
            "--test-num-sample", 3, "--train-base-model", "--lr-codebook-path",
            f"{t}/cb_lr/models_checkpoint/codebook.pt", "--hr-codebook-path",
            f"{t}/cb_hr/models_checkpoint/codebook.pt", "--config-path", f"{t}/t_base.json", "--max-steps", 2,
            "--out-dir", f"{t}/on", "--attn-dropout", 0.1, "--dropout-seed", "0x5EED"]
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(PKG, "train_quantized_transformer.py"), *map(str, args)], cwd=t,
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    md = torch.load(f"{t}/on/models_checkpoint/model_1.pt", map_location="cpu", weights_only=True)
    assert set(md) == BASE_KEYS | {"attn_dropout", "dropout_seed"}
    assert md["attn_dropout"] == 0.1 and type(md["attn_dropout"]) is float and md["dropout_seed"] == 0x5EED
    out = r.stdout + r.stderr
    block = out[out.index("Training Parameters."):out.index("Sampling Parameters.")]
    assert "Attention Dropout: 0.1" in block and f"Dropout Seed: {0x5EED}" in block and "\nDropout: " not in block
    steps = [ln for ln in out.splitlines() if "Cum. Steps:" in ln]
    assert len(steps) == 2
    for ln in steps:
        assert 0 < float(ln.split("Recon Loss: ")[1].split(" |")[0]) < 100
