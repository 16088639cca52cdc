"""Token noise through the layers above the kernels, on the GPU at the narrow model of
tests/test_gpu_attn_dropout_train.py (a 2-layer encoder-decoder of width 64, 2 x 33-token windows of 65): eager steps
against graph replay, repeats, ranks and resuming, the C-ABI call counts of the default step and of either stream,
the one key of all three regularisers, the paths that must never see noise, the scorer under noise against the NumPy
rule, and the command line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import token_noise_cases as TN
from conftest import PKG

pytestmark = pytest.mark.gpu

P_IN, P_COND, RANGE, SEED = 0.25, 0.5, 3, 0x5EED0123456789
V_ENC, V_DEC, V_OUT, S, N = 16, 40, 33, 33, 2
SEQ = 65                                      # <start> + 64 HR tokens, windows of 33


def _model():
    from models.Transformer import Transformer
    torch.manual_seed(5)
    m = Transformer(use_encoder=True, use_pos_cond=True, num_enc_layers=2, num_dec_layers=2, num_enc_embedding=V_ENC,
                    num_dec_embedding=V_DEC, self_attn_heads=8, cross_attn_heads=8, transformer_in_dim=64,
                    transformer_out_dim=V_OUT, transformer_hidden_dim=128).cuda()
    g = torch.Generator().manual_seed(6)
    with torch.no_grad():
        for p in m.parameters():
            if p.abs().max() == 0:
                p.copy_(torch.randn(p.shape, generator=g) * 0.05)
    return m


def _codebooks():
    from models.Codebook import Codebook
    g = torch.Generator().manual_seed(4)
    lr_cb = Codebook(patch_dim=(8, 8), image_dim=(16, 16), image_channel=4, num_embeddings=V_ENC).cuda()
    hr_cb = Codebook(patch_dim=(2, 2), image_dim=(16, 16), image_channel=4, num_embeddings=V_OUT - 1).cuda()
    with torch.no_grad():
        lr_cb.codebook.weight.copy_(torch.tanh(torch.randn(lr_cb.codebook.weight.shape, generator=g)))
        hr_cb.codebook.weight.copy_(torch.tanh(torch.randn(hr_cb.codebook.weight.shape, generator=g)))
    return lr_cb, hr_cb


def _build_pipeline():
    from qarig.optim import FlatAdam
    lr_cb, hr_cb = _codebooks()
    m = _model()
    m.train()
    return lr_cb, hr_cb, m, FlatAdam(m.parameters(), lr=1e-3, betas=(0.5, 0.999))


def _batches(n):
    g = torch.Generator().manual_seed(9)
    return [(torch.tanh(torch.randn((N, 4, 16, 16), generator=g)), torch.randint(0, SEQ - S + 1, (N,), generator=g))
            for _ in range(n)]


def _step(m, opt, lr_cb, hr_cb, z, rand):
    """One eager step as train_quantized_transformer.py makes it."""
    from qarig import pipeline
    if m.token_noise is not None:
        pipeline.set_dropout_step(m, opt)
    hr_in, lr_in, hr_tg, pos = pipeline.tokenize_window(z.cuda(), lr_cb, hr_cb, False, S, rand,
                                                        token_noise=m.token_noise)
    tokens = (hr_in.clone(), lr_in.clone(), hr_tg.clone())
    return pipeline.train_step(m, opt, hr_in, lr_in, hr_tg, pos, dp=False, pos_bound=SEQ).detach(), tokens


def _eager_steps(n, prepare, built=None, batches=None):
    from qarig import _lib
    lr_cb, hr_cb, m, opt = built or _build_pipeline()
    prepare(m)
    losses, calls, toks = [], [], []
    for z, rand in (batches or _batches(n)):
        before = _lib.N_CALLS
        loss, t = _step(m, opt, lr_cb, hr_cb, z, rand)
        calls.append(_lib.N_CALLS - before)
        losses.append(float(loss))
        toks.append(t)
    return opt.flat_param.detach().clone(), losses, calls, toks


def _on(rank=0, p_in=P_IN, p_cond=P_COND):
    return lambda m: m.enable_token_noise(p_in, p_cond, SEED, rank=rank, neighbour_range=RANGE)


@pytest.fixture(scope="module")
def eager():
    """Three eager steps: both streams on at rank 0, the input stream alone, never enabled."""
    return {"on": _eager_steps(3, _on()), "input": _eager_steps(3, _on(p_cond=0.0)),
            "never": _eager_steps(3, lambda m: None)}


# ---- steps -------------------------------------------------------------------------------------------------------
def test_it_is_noise_and_repeats_bit_for_bit(eager):
    flat, losses, calls, toks = eager["on"]
    flat0, losses0, calls0, toks0 = eager["never"]
    assert losses != losses0 and not torch.equal(flat, flat0)
    for (hr_in, lr_in, hr_tg), (hr_in0, lr_in0, hr_tg0) in zip(toks, toks0):
        assert not torch.equal(hr_in, hr_in0) and not torch.equal(lr_in, lr_in0)
        assert torch.equal(hr_tg, hr_tg0)                       # the targets stay clean
        assert torch.equal(hr_in[hr_in0 == V_OUT - 1], hr_in0[hr_in0 == V_OUT - 1])      # <start> too
    again = _eager_steps(3, _on())
    assert again[1] == losses and torch.equal(again[0], flat)


def test_the_tokens_of_a_step_are_the_rule_s(eager):
    """Step t reads key step t: the corrupted tokens equal the NumPy rule on the clean run's tokens."""
    t_in, t_cond = (int(round(p * 65536)) for p in (P_IN, P_COND))
    for step, ((hr_in, lr_in, _), (hr_in0, lr_in0, _), (_, rand)) in enumerate(
            zip(eager["on"][3], eager["never"][3], _batches(3)), start=1):
        want_lr = TN.noise(lr_in0.cpu().numpy(), V_ENC, t_cond, RANGE, SEED, 1, step, 0)
        assert np.array_equal(lr_in.cpu().numpy(), want_lr)
        # the windowed hr tokens: position w of sample n shows hr token rand[n] + w - 1, keyed on that index; the
        # rule is evaluated on a full-length stream holding the window's tokens at their places
        full = np.zeros((N, SEQ - 1), dtype=np.int64)
        for n in range(N):
            for w in range(S):
                j = int(rand[n]) + w - 1
                if j >= 0:
                    full[n, j] = int(hr_in0[n, w])
        noisy = TN.noise(full, V_OUT - 1, t_in, RANGE, SEED, 0, step, 0)
        for n in range(N):
            for w in range(S):
                j = int(rand[n]) + w - 1
                assert int(hr_in[n, w]) == (V_OUT - 1 if j < 0 else int(noisy[n, j])), (step, n, w)


def test_call_counts(eager, monkeypatch):
    from qarig import _lib
    never, inp, on = eager["never"][2], eager["input"][2], eager["on"][2]
    assert inp == never                          # one entry replaces the other
    assert on == [c + 1 for c in never]          # the encoder's lr tokens: exactly one more launch per step
    assert eager["input"][1] != eager["never"][1] and eager["input"][1] != eager["on"][1]
    # the never-enabled step makes the calls it made before the feature: tokenize_window through its earlier
    # signature, one plain assemble launch among them and neither noise entry
    names = []
    real = _lib.check
    monkeypatch.setattr(_lib, "check", lambda status, what: (names.append(what), real(status, what))[1])
    from qarig import ops, pipeline
    monkeypatch.setattr(ops, "check", _lib.check)
    lr_cb, hr_cb, m, opt = _build_pipeline()
    z, rand = _batches(1)[0]
    before = _lib.N_CALLS
    hr_in, lr_in, hr_tg, pos = pipeline.tokenize_window(z.cuda(), lr_cb, hr_cb, False, S, rand)
    pipeline.train_step(m, opt, hr_in, lr_in, hr_tg, pos, dp=False, pos_bound=SEQ)
    assert _lib.N_CALLS - before == never[0]
    assert names.count("qarig_assemble_tokens") == 1 and not [n for n in names if "noise" in n]
    assert m.dropout_key is None and m.token_noise is None


def test_two_ranks_draw_different_tokens(eager):
    other = _eager_steps(3, _on(rank=1))
    assert other[1] != eager["on"][1]
    assert not torch.equal(other[3][0][0], eager["on"][3][0][0])       # already the first step's decoder input
    assert not torch.equal(other[3][0][1], eager["on"][3][0][1])       # and its conditioning


def test_graph_replay_matches_eager_steps():
    from qarig import pipeline
    want, losses_e, _, _ = _eager_steps(4, _on())
    lr_cb, hr_cb, m, opt = _build_pipeline()
    key = m.enable_token_noise(P_IN, P_COND, SEED, neighbour_range=RANGE)
    assert key is m.dropout_key                   # token noise is the only user of the key: the step word is set
    step = pipeline.GraphedTrainStep(m, opt, lr_cb, hr_cb, False, S, warmup=2)
    losses_g = [float(step(z.cuda(), rand)) for z, rand in _batches(4)]
    assert step.graph is not None and opt.step_count == 4 and key.buffer.tolist()[2] == 4
    assert losses_g == losses_e
    assert torch.equal(opt.flat_param, want)
    # enabling, disabling or re-keying after the capture is refused
    z, rand = _batches(1)[0]
    m.enable_token_noise(P_IN, P_COND, SEED, neighbour_range=RANGE)        # same key object, a new state
    with pytest.raises(RuntimeError):
        step(z.cuda(), rand)
    m.disable_token_noise()
    with pytest.raises(RuntimeError):
        step(z.cuda(), rand)


def test_enabling_after_capture_raises():
    from qarig import pipeline
    lr_cb, hr_cb, m, opt = _build_pipeline()
    step = pipeline.GraphedTrainStep(m, opt, lr_cb, hr_cb, False, S, warmup=1)
    for z, rand in _batches(2):
        step(z.cuda(), rand)
    assert step.graph is not None
    m.enable_token_noise(P_IN, 0.0, SEED)
    z, rand = _batches(1)[0]
    with pytest.raises(RuntimeError):
        step(z.cuda(), rand)


def test_resume_continues_the_sequence(eager):
    from qarig.optim import FlatAdam
    want, losses_e, _, _ = eager["on"]
    built = _build_pipeline()
    lr_cb, hr_cb, m, opt = built
    batches = _batches(3)
    _, losses, _, _ = _eager_steps(2, _on(), built=built, batches=batches[:2])
    saved = {"model": {k: v.detach().clone() for k, v in m.state_dict().items()}, "optim": opt.state_dict()}
    m2 = _model()
    m2.train()
    m2.load_state_dict(saved["model"])
    opt2 = FlatAdam(m2.parameters(), lr=1e-3, betas=(0.5, 0.999))
    opt2.load_state_dict(saved["optim"])
    assert opt2.step_count == 2
    flat, last, _, _ = _eager_steps(1, _on(), built=(lr_cb, hr_cb, m2, opt2), batches=batches[2:])
    assert m2.dropout_key.step == 3
    assert losses + last == losses_e and torch.equal(flat, want)


# ---- one key for the three regularisers ----------------------------------------------------------------------------
def test_all_three_regularisers_share_one_key(eager):
    m = _model()
    key = m.enable_token_noise(P_IN, P_COND, SEED, rank=2, neighbour_range=RANGE)
    assert m.enable_dropout(0.1, SEED, rank=2) is key and m.enable_attention_dropout(0.2, SEED, rank=2) is key
    assert m.dropout_key is key and m.token_noise.key is key and m.token_noise.neighbour_range == RANGE
    for bad in ((SEED + 1, 2), (SEED, 3)):
        for enable in (lambda s, r: m.enable_token_noise(P_IN, 0.0, s, rank=r), lambda s, r: m.enable_dropout(0.1, s, rank=r),
                       lambda s, r: m.enable_attention_dropout(0.2, s, rank=r)):
            with pytest.raises(ValueError, match="share it"):
                enable(*bad)
    m.disable_dropout()
    m.disable_attention_dropout()
    assert m.dropout_key is key                   # token noise still holds it
    m.disable_token_noise()
    assert m.dropout_key is None and m.token_noise is None
    for first in ("enable_dropout", "enable_attention_dropout"):
        m = _model()
        key = getattr(m, first)(0.1, SEED)
        assert m.enable_token_noise(0.0, P_COND, SEED) is key
        with pytest.raises(ValueError, match="share it"):
            m.enable_token_noise(P_IN, 0.0, SEED, rank=1)
    # either probability may be 0; both 0 disables; the refusals
    m = _model()
    assert m.enable_token_noise(0, 0, SEED) is None and m.dropout_key is None
    assert m.enable_token_noise(P_IN, 0, SEED).seed == SEED and m.token_noise.t_cond == 0
    assert m.enable_token_noise(0, 0, SEED) is None and m.token_noise is None
    sd = set(m.state_dict())
    m.enable_token_noise(0, P_COND, SEED)
    assert m.token_noise.t_input == 0 and set(m.state_dict()) == sd
    for bad in ((1e-6, 0), (0.91, 0), (0, 1.0), (float("nan"), 0), (-0.1, 0)):
        with pytest.raises(ValueError):
            m.enable_token_noise(*bad, 0)
    with pytest.raises(ValueError):
        m.enable_token_noise(P_IN, 0, 0, neighbour_range=-1)
    from models.Transformer import Transformer
    base = Transformer(use_encoder=False, use_pos_cond=False, num_enc_layers=None, num_dec_layers=1,
                       num_enc_embedding=None, num_dec_embedding=V_DEC, self_attn_heads=2, cross_attn_heads=None,
                       transformer_in_dim=32, transformer_out_dim=V_OUT, transformer_hidden_dim=64).cuda()
    with pytest.raises(ValueError, match="encoder"):
        base.enable_token_noise(P_IN, P_COND, 0)
    assert base.dropout_key is None
    assert base.enable_token_noise(P_IN, 0, 0) is base.dropout_key
    # all three at once train, and differ from token noise alone
    all3 = _eager_steps(3, lambda mm: (mm.enable_dropout(0.1, SEED), mm.enable_attention_dropout(0.2, SEED),
                                       mm.enable_token_noise(P_IN, P_COND, SEED, neighbour_range=RANGE)))
    assert all(np.isfinite(all3[1])) and all3[1] != eager["on"][1]
    for a, b in zip(all3[3], eager["on"][3]):      # the same tokens: the three domains do not disturb one another
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---- the paths that never see it -----------------------------------------------------------------------------------
def test_eval_scoring_and_generation_make_no_noise_call(monkeypatch):
    from qarig import _lib, ops, sampling
    from qarig.evaluate import TokenScorer
    lr_cb, hr_cb = _codebooks()
    plain, noisy = _model(), _model()
    noisy.enable_token_noise(P_IN, P_COND, SEED, neighbour_range=RANGE)
    names = []
    real = _lib.check
    monkeypatch.setattr(_lib, "check", lambda status, what: (names.append(what), real(status, what))[1])
    monkeypatch.setattr(ops, "check", _lib.check)
    z = _batches(1)[0][0].cuda()
    res = []
    for m in (plain, noisy):
        m.eval()
        sc = TokenScorer(m, lr_cb, hr_cb, False, S)
        sc.add_batch(z)
        res.append(sc.result())
    assert res[0] == res[1] and res[0]["tokens"] > 0 and "input_noise" not in res[0]
    x_enc = lr_cb.get_patches_bmu(z, reshape=True)
    first = torch.full((N, 1), V_OUT - 1, dtype=torch.int64).cuda()
    toks = []
    for m in (plain, noisy):
        torch.manual_seed(3)
        with torch.no_grad():
            toks.append(sampling.generate_tokens(m, first, x_enc, 12, 0.05, True, S, end_token=V_DEC,
                                                 mode="generate", use_kv_cache=True))
    assert torch.equal(*toks)
    assert names and "qarig_assemble_tokens" in names and not [n for n in names if "noise" in n]


def test_scorer_under_noise_is_the_rule_and_zero_is_today(monkeypatch):
    from qarig import ops
    from qarig.evaluate import TokenScorer
    lr_cb, hr_cb = _codebooks()
    m = _model().eval()
    batches = [z.cuda() for z, _ in _batches(2)]
    t_in, t_cond = (int(round(p * 65536)) for p in (P_IN, P_COND))

    def score(**kw):
        sc = TokenScorer(m, lr_cb, hr_cb, False, S, **kw)
        for z in batches:
            sc.add_batch(z)
        return sc.result()

    today = score()
    assert score(input_noise=0, cond_noise=0, noise_range=0, noise_seed=0) == today
    got = score(input_noise=P_IN, cond_noise=P_COND, noise_range=RANGE, noise_seed=SEED)
    assert (got["input_noise"], got["cond_noise"], got["noise_range"], got["noise_seed"]) == (P_IN, P_COND, RANGE, SEED)
    assert got["nll_mean"] != today["nll_mean"] and got["tokens"] == today["tokens"]
    assert score(input_noise=P_IN, cond_noise=P_COND, noise_range=RANGE, noise_seed=SEED) == got
    # a plain scorer fed tokens corrupted by the NumPy rule: batch b reads step b, rank 0
    batch = [0]
    real_bmu_lr, real_assemble = lr_cb.get_patches_bmu, ops.assemble_tokens

    def lr_bmu(*a, **k):
        idx = real_bmu_lr(*a, **k)
        return torch.from_numpy(TN.noise(idx.cpu().numpy(), V_ENC, t_cond, RANGE, SEED, 1, batch[0], 0)).cuda()

    def assemble(lr_idx, hr_idx, base, k_lr, k_hr, offs=None, window=None, noise=None):
        assert noise is None
        hr_in, hr_tg, pos = real_assemble(lr_idx, hr_idx, base, k_lr, k_hr, offs, window)
        noisy = TN.noise(hr_idx.cpu().numpy(), k_hr, t_in, RANGE, SEED, 0, batch[0], 0)
        want = TN.assemble(None, hr_idx.cpu().numpy(), False, k_lr, k_hr, None if offs is None else offs.cpu().numpy(),
                           window, noisy_hr=noisy)[0]
        return torch.from_numpy(want).cuda(), hr_tg, pos

    monkeypatch.setattr(lr_cb, "get_patches_bmu", lr_bmu)
    monkeypatch.setattr(ops, "assemble_tokens", assemble)
    sc = TokenScorer(m, lr_cb, hr_cb, False, S)
    for b, z in enumerate(batches):
        batch[0] = b
        sc.add_batch(z)
    fed = sc.result()
    for k in fed:
        assert fed[k] == got[k], k
    with pytest.raises(ValueError):
        TokenScorer(m, lr_cb, hr_cb, True, S, cond_noise=P_COND)


# ---- the command line: the fixtures of tests/test_gpu_attn_dropout_train.py, for an encoder-decoder stage ---------
BASE_KEYS = {"train_base_model", "use_sliding_window", "sliding_window", "num_enc_embedding", "num_dec_embedding",
             "num_enc_layers", "num_dec_layers", "self_attn_heads", "cross_attn_heads", "transformer_in_dim",
             "transformer_out_dim", "transformer_hidden_dim", "hidden_activation", "model", "model_optimizer"}


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    sys.path.insert(0, PKG)
    from dataset_loader._tinydb_json import write_all
    from models.Codebook import Codebook
    from models.FC_Decoder import FC_Decoder
    from utils.model_utils import save_model
    t = str(tmp_path_factory.mktemp("token_noise_cli"))
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
    for name, patch, k in (("lr", 4, 8), ("hr", 2, 16)):
        cb = Codebook(patch_dim=(patch, patch), image_dim=(8, 8), image_channel=4, num_embeddings=k)
        with torch.no_grad():
            cb.codebook.weight.copy_(torch.tanh(torch.randn(cb.codebook.weight.shape)))
        save_model(f"{t}/cb_{name}", "codebook.pt",
                   dict(patch_dim=(patch, patch), image_dim=(8, 8), image_C=4, num_embeddings=k,
                        neighbourhood_range=1, global_steps=0, checkpoint=cb.state_dict()))
    json.dump(dict(model_lr=1e-3, num_enc_layers=1, num_dec_layers=2, cross_attn_heads=2, self_attn_heads=4,
                   in_dim=32, hidden_dim=64, hidden_activation="silu", use_sliding_window=True,
                   sliding_window=8), open(f"{t}/t.json", "w"))
    args = ["--device", "cuda", "--dataset-path", f"{t}/fmaps.json", "--decoder-path",
            f"{t}/dec/models_checkpoint/model.pt", "--batch-size", 4, "--checkpoint-step", 1, "--max-epoch", 1,
            "--test-num-sample", 3, "--lr-codebook-path", f"{t}/cb_lr/models_checkpoint/codebook.pt",
            "--hr-codebook-path", f"{t}/cb_hr/models_checkpoint/codebook.pt", "--config-path", f"{t}/t.json",
            "--max-steps", 2]
    return t, args


def _run(script, t, *args):
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, os.path.join(PKG, script), *map(str, args)], cwd=t, env=env,
                          capture_output=True, text=True, timeout=300)


def test_cli_with_the_three_flags(cli):
    t, args = cli
    r = _run("train_quantized_transformer.py", t, *args, "--out-dir", f"{t}/on", "--input-noise", 0.1, "--cond-noise",
             0.2, "--noise-range", 2, "--dropout-seed", "0x5EED", "--graph-step")
    assert r.returncode == 0, f"{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    md = torch.load(f"{t}/on/models_checkpoint/model_1.pt", map_location="cpu", weights_only=True)
    assert set(md) == BASE_KEYS | {"input_noise", "cond_noise", "noise_range", "dropout_seed"}
    assert (md["input_noise"], md["cond_noise"], md["noise_range"], md["dropout_seed"]) == (0.1, 0.2, 2, 0x5EED)
    out = r.stdout + r.stderr
    block = out[out.index("Training Parameters."):out.index("Sampling Parameters.")]
    assert "Input Noise: 0.1" in block and "Cond Noise: 0.2" in block and "Noise Range: 2" in block
    assert block.count(f"Dropout Seed: {0x5EED}") == 1 and "Dropout: " not in block
    steps = [ln for ln in out.splitlines() if "Cum. Steps:" in ln]
    assert len(steps) == 2
    for ln in steps:
        assert 0 < float(ln.split("Recon Loss: ")[1].split(" |")[0]) < 100
    # evaluate_transformer.py under the same noise records the four values; without the flags they are zeros
    score = ["--device", "cuda", "--dataset-path", f"{t}/fmaps.json", "--lr-codebook-path",
             f"{t}/cb_lr/models_checkpoint/codebook.pt", "--hr-codebook-path", f"{t}/cb_hr/models_checkpoint/codebook.pt",
             "--model-path", f"{t}/on/models_checkpoint/model_1.pt", "--batch-size", 4]
    r = _run("evaluate_transformer.py", t, *score, "--out-json", f"{t}/noisy.json", "--input-noise", 0.1, "--cond-noise",
             0.2, "--noise-range", 2, "--noise-seed", 7)
    assert r.returncode == 0, f"{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    r = _run("evaluate_transformer.py", t, *score, "--out-json", f"{t}/clean.json")
    assert r.returncode == 0, f"{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    noisy, clean = json.load(open(f"{t}/noisy.json")), json.load(open(f"{t}/clean.json"))
    assert [noisy[k] for k in ("input_noise", "cond_noise", "noise_range", "noise_seed")] == [0.1, 0.2, 2, 7]
    assert [clean[k] for k in ("input_noise", "cond_noise", "noise_range", "noise_seed")] == [0.0, 0.0, 0, 0]
    assert noisy["tokens"] == clean["tokens"] and noisy["nll_mean"] != clean["nll_mean"]


def test_cli_refusals(cli):
    t, args = cli
    r = _run("train_quantized_transformer.py", t, *args, "--out-dir", f"{t}/bad", "--train-base-model", "--cond-noise", 0.2)
    assert r.returncode != 0 and "--cond-noise does not go with --train-base-model" in r.stderr
    r = _run("train_quantized_transformer.py", t, *args, "--out-dir", f"{t}/bad", "--input-noise", 0.1, "--noise-range", 8)
    assert r.returncode != 0 and "use 0" in r.stderr
    assert not os.path.exists(f"{t}/bad/models_checkpoint")
