"""train_quantized_transformer.py --val-dataset-path and evaluate_transformer.py end to end on the GPU, at tiny shapes
(the pattern of tests/test_gpu_ema_cli.py: decoder, codebooks and latents written directly; the Transformer trained,
validated, checkpointed and scored through the two command lines).  A base model with a sliding window of 8 over 17
tokens: three evaluation windows, the last one counting a single position."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import PKG

pytestmark = pytest.mark.gpu

BASE_KEYS = {"train_base_model", "use_sliding_window", "sliding_window", "num_enc_embedding", "num_dec_embedding",
             "num_enc_layers", "num_dec_layers", "self_attn_heads", "cross_attn_heads", "transformer_in_dim",
             "transformer_out_dim", "transformer_hidden_dim", "hidden_activation", "model", "model_optimizer"}
RESULT_KEYS = {"tokens", "images", "nll_mean", "bits_per_token", "perplexity", "top1", "topk", "k",
               "per_position_nll", "per_position_count"}
N_VAL, SEQ = 6, 17


def _run(script, *args, cwd, ok=True):
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(PKG, script), *map(str, args)], cwd=cwd, env=env,
                       capture_output=True, text=True, timeout=300)
    if ok:
        assert r.returncode == 0, f"{script} failed:\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    return r


def _latents(t, name, n, seed):
    from dataset_loader._tinydb_json import write_all
    rng = np.random.default_rng(seed)
    recs = []
    for i in range(n):
        p = os.path.join(t, f"{name}{i}.npy")
        np.save(p, np.tanh(rng.standard_normal((4, 8, 8))).astype(np.float32))
        recs.append({"fmap_path": p, "image_path": ""})
    write_all(f"{t}/{name}.json", recs)
    return f"{t}/{name}.json"


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    sys.path.insert(0, PKG)
    from models.Codebook import Codebook
    from models.FC_Decoder import FC_Decoder
    from utils.model_utils import save_model
    t = str(tmp_path_factory.mktemp("eval_cli"))
    torch.manual_seed(0)
    train, val = _latents(t, "z", 12, 0), _latents(t, "v", N_VAL, 1)
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
                   in_dim=32, hidden_dim=64, hidden_activation="silu", use_sliding_window=True,
                   sliding_window=8), open(f"{t}/t_base.json", "w"))
    codebooks = ["--lr-codebook-path", f"{t}/cb_lr/models_checkpoint/codebook.pt", "--hr-codebook-path",
                 f"{t}/cb_hr/models_checkpoint/codebook.pt"]
    common = ["--device", "cuda", "--dataset-path", train, "--decoder-path", f"{t}/dec/models_checkpoint/model.pt",
              "--batch-size", 4, "--checkpoint-step", 2, "--max-epoch", 1, "--test-num-sample", 3,
              "--train-base-model", *codebooks, "--config-path", f"{t}/t_base.json"]
    out = {}
    r = _run("train_quantized_transformer.py", *common, "--max-steps", 3, "--out-dir", f"{t}/ema", "--ema-decay", 0.99,
             "--val-dataset-path", val, cwd=t)
    out["ema"] = r.stdout + r.stderr
    r = _run("train_quantized_transformer.py", *common, "--max-steps", 2, "--out-dir", f"{t}/val", "--val-dataset-path",
             val, "--val-step", 1, "--val-batches", 1, cwd=t)
    out["val"] = r.stdout + r.stderr
    r = _run("train_quantized_transformer.py", *common, "--max-steps", 3, "--out-dir", f"{t}/off", cwd=t)
    out["off"] = r.stdout + r.stderr
    score = ["--device", "cuda", "--dataset-path", val, *codebooks, "--batch-size", 4]
    return dict(t=t, out=out, score=score)


def _lines(path):
    return [json.loads(ln) for ln in open(path).read().splitlines()]


def test_training_with_validation_logs_one_line_per_evaluation(runs):
    t = runs["t"]
    lines = _lines(f"{t}/ema/val_log.jsonl")
    assert [ln["step"] for ln in lines] == [0, 2]                 # --val-step defaults to --checkpoint-step
    for ln in lines:
        assert set(ln) == {"step", "model", "model_ema"}
        for which in ("model", "model_ema"):
            r = ln[which]
            assert set(r) == RESULT_KEYS
            assert r["tokens"] == N_VAL * SEQ and r["images"] == N_VAL and r["per_position_count"] == [N_VAL] * SEQ
            assert r["nll_mean"] > 0 and r["bits_per_token"] == pytest.approx(r["nll_mean"] / np.log(2.0), rel=1e-14)
            assert 0.0 <= r["top1"] <= r["topk"] <= 1.0
    assert lines[1]["model"]["nll_mean"] != lines[1]["model_ema"]["nll_mean"]
    log = runs["out"]["ema"]
    assert log.count("Val Loss: ") == 2 and log.count("Val EMA Loss: ") == 2
    assert "bits/token" in log and "top-1" in log
    assert "Val Loss: {:.5f}".format(lines[1]["model"]["nll_mean"]) in log
    # the checkpoint schema is the EMA run's own
    md = torch.load(f"{t}/ema/models_checkpoint/model_2.pt", map_location="cpu", weights_only=True)
    assert set(md) == BASE_KEYS | {"model_ema", "model_ema_meta"}
    # without --ema-decay: one result set per line; --val-step 1, --val-batches 1
    lines = _lines(f"{t}/val/val_log.jsonl")
    assert [ln["step"] for ln in lines] == [0, 1]
    for ln in lines:
        assert set(ln) == {"step", "model"} and ln["model"]["images"] == 4 and ln["model"]["tokens"] == 4 * SEQ
    assert "EMA" not in runs["out"]["val"] and runs["out"]["val"].count("Val Loss: ") == 2
    md = torch.load(f"{t}/val/models_checkpoint/model_0.pt", map_location="cpu", weights_only=True)
    assert set(md) == BASE_KEYS


def test_without_the_flag_nothing_is_added(runs):
    t = runs["t"]
    assert "Val" not in runs["out"]["off"]
    assert not os.path.exists(f"{t}/off/val_log.jsonl")
    listing = set(os.listdir(f"{t}/off"))
    assert "models_checkpoint" in listing and not [f for f in listing if "val" in f.lower()], listing
    assert sorted(os.listdir(f"{t}/off/models_checkpoint")) == ["model_0.pt", "model_2.pt"]
    md = torch.load(f"{t}/off/models_checkpoint/model_2.pt", map_location="cpu", weights_only=True)
    assert set(md) == BASE_KEYS
    # the run with validation writes the same files plus the log
    assert set(os.listdir(f"{t}/ema")) == listing | {"val_log.jsonl"}


def test_evaluate_cli_reproduces_the_logged_validation_losses(runs):
    t = runs["t"]
    last = _lines(f"{t}/ema/val_log.jsonl")[-1]
    ckpt = f"{t}/ema/models_checkpoint/model_2.pt"
    r = _run("evaluate_transformer.py", *runs["score"], "--model-path", ckpt, "--out-json", f"{t}/raw.json", cwd=t)
    raw = json.load(open(f"{t}/raw.json"))
    assert raw["weights"] == "model" and len(raw["per_image_nll"]) == N_VAL
    assert raw["nll_mean"] == last["model"]["nll_mean"]                       # bit for bit
    assert raw["per_position_nll"] == last["model"]["per_position_nll"]
    assert "Eval Loss: {:.5f}".format(raw["nll_mean"]) in r.stdout + r.stderr
    _run("evaluate_transformer.py", *runs["score"], "--model-path", ckpt, "--out-json", f"{t}/avg.json", "--use-ema",
         "--topk", 3, cwd=t)
    avg = json.load(open(f"{t}/avg.json"))
    assert avg["weights"] == "model_ema" and avg["k"] == 3
    assert avg["nll_mean"] == last["model_ema"]["nll_mean"]
    assert avg["top1"] == last["model_ema"]["top1"] and avg["topk"] <= last["model_ema"]["topk"]
    assert sum(avg["per_image_nll"]) == pytest.approx(avg["nll_mean"] * avg["tokens"], rel=1e-13)


def test_use_ema_without_an_average_is_refused(runs):
    t = runs["t"]
    plain = f"{t}/off/models_checkpoint/model_2.pt"
    r = _run("evaluate_transformer.py", *runs["score"], "--model-path", plain, "--use-ema", "--max-batches", 1, cwd=t,
             ok=False)
    assert r.returncode != 0 and plain in (r.stdout + r.stderr) and "model_ema" in (r.stdout + r.stderr)
