"""train_quantized_transformer.py --ema-decay and generate_images.py --use-ema end to end on the GPU, at tiny
shapes.  The decoder, the codebooks and the latents are written directly (their command lines are
tests/test_gpu_cli.py's subject); the Transformer is trained, checkpointed, sampled and generated from through
the two command lines."""
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
    t = str(tmp_path_factory.mktemp("ema_cli"))
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
    out_ema = _run("train_quantized_transformer.py", *common, "--out-dir", f"{t}/ema", "--ema-decay", 0.99, cwd=t)
    out_off = _run("train_quantized_transformer.py", *common, "--out-dir", f"{t}/off", cwd=t)
    return dict(t=t, common=common, out_ema=out_ema.stdout + out_ema.stderr, out_off=out_off.stdout + out_off.stderr)


def _gen_config(t, name, model_path):
    json.dump({"0": dict(model_path=model_path, temperature=1.0,
                         lr_codebook_path=f"{t}/cb_lr/models_checkpoint/codebook.pt",
                         hr_codebook_path=f"{t}/cb_hr/models_checkpoint/codebook.pt", num_beam=2, beam_width=4)},
              open(f"{t}/{name}.json", "w"))
    return f"{t}/{name}.json"


def test_ema_checkpoint_entries_sample_grid_and_log(runs):
    t = runs["t"]
    md = torch.load(f"{t}/ema/models_checkpoint/model_2.pt", map_location="cpu", weights_only=True)
    assert set(md) == BASE_KEYS | {"model_ema", "model_ema_meta"}
    assert md["model_ema_meta"] == {"decay": 0.99, "count": 3, "warmup": True}
    assert type(md["model_ema_meta"]["count"]) is int and type(md["model_ema_meta"]["warmup"]) is bool
    assert list(md["model_ema"]) == list(md["model"])
    differs = 0
    for k, v in md["model"].items():
        e = md["model_ema"][k]
        assert e.shape == v.shape and e.dtype == v.dtype
        differs += int(not torch.equal(e, v))
    assert differs > len(md["model"]) // 2
    # loadable by the model's own loader
    from models.Transformer import Transformer
    m = Transformer(use_encoder=False, use_pos_cond=False, num_enc_layers=None, num_dec_layers=2,
                    num_enc_embedding=None, num_dec_embedding=md["num_dec_embedding"], self_attn_heads=4,
                    cross_attn_heads=None, transformer_in_dim=32, transformer_out_dim=17, transformer_hidden_dim=64)
    m.custom_load_state_dict(md["model_ema"])
    assert torch.equal(dict(m.state_dict())["dec_embedding.weight"], md["model_ema"]["dec_embedding.weight"])
    for steps in (0, 2):
        assert os.path.exists(f"{t}/ema/images/high_res_recon_ema_{steps}.jpg")
        assert os.path.exists(f"{t}/ema/images/high_res_recon_{steps}.jpg")
    assert "EMA decay: 0.99" in runs["out_ema"]


def test_without_the_flag_nothing_is_added(runs):
    t = runs["t"]
    md = torch.load(f"{t}/off/models_checkpoint/model_2.pt", map_location="cpu", weights_only=True)
    assert set(md) == BASE_KEYS
    assert not [f for f in os.listdir(f"{t}/off/images") if "ema" in f]
    assert "EMA" not in runs["out_off"]


def test_resume_restores_the_average_and_its_count(runs):
    t = runs["t"]
    common = [a for a in runs["common"]]
    common[common.index("--max-steps") + 1] = 1
    ckpt = f"{t}/ema/models_checkpoint/model_2.pt"
    _run("train_quantized_transformer.py", *common, "--out-dir", f"{t}/resumed", "--ema-decay", 0.99, "--model-path",
         ckpt, "--load-optim", cwd=t)
    _run("train_quantized_transformer.py", *common, "--out-dir", f"{t}/restarted", "--ema-decay", 0.99, "--model-path",
         ckpt, cwd=t)
    md = torch.load(f"{t}/resumed/models_checkpoint/model_0.pt", map_location="cpu", weights_only=True)
    assert md["model_ema_meta"] == {"decay": 0.99, "count": 4, "warmup": True}
    # without --load-optim the average starts over from the loaded parameters
    md0 = torch.load(f"{t}/restarted/models_checkpoint/model_0.pt", map_location="cpu", weights_only=True)
    assert md0["model_ema_meta"]["count"] == 1
    # one more update, of weight ema_weight(3) = 9 / 13 from the saved average or of ema_weight(0) = 0.9 from the
    # loaded parameters: the kernel's w >= 0.5 branch, restated in fp32
    from qarig.optim import ema_weight
    old = torch.load(ckpt, map_location="cpu", weights_only=True)
    for new_md, start, count in ((md, old["model_ema"], 3), (md0, old["model"], 0)):
        one_minus_w = 1.0 - torch.tensor(ema_weight(count, 0.99, True), dtype=torch.float32)
        for k, pn in new_md["model"].items():
            if pn.dtype == torch.float32 and k in dict(old["model"]):
                want = pn - (pn - start[k]) * one_minus_w
                assert torch.equal(new_md["model_ema"][k], want), k


def test_generate_use_ema_samples_from_the_average(runs):
    t = runs["t"]
    ckpt = f"{t}/ema/models_checkpoint/model_2.pt"
    md = torch.load(ckpt, map_location="cpu", weights_only=True)
    swapped = dict(md, model=md["model_ema"])
    os.makedirs(f"{t}/swapped", exist_ok=True)
    torch.save(swapped, f"{t}/swapped/model_2.pt")
    gen = ["--device", "cuda", "--decoder-path", f"{t}/dec/models_checkpoint/model.pt", "--num-images", 3, "--seed", 69]
    _run("generate_images.py", *gen, "--config-path", _gen_config(t, "gen_ema", ckpt), "--out-dir", f"{t}/g_ema",
         "--use-ema", cwd=t)
    _run("generate_images.py", *gen, "--config-path", _gen_config(t, "gen_swapped", f"{t}/swapped/model_2.pt"),
         "--out-dir", f"{t}/g_swapped", cwd=t)
    for f in ("recon_model_Cond", "recon_model_0"):
        a = open(f"{t}/g_ema/images/{f}.jpg", "rb").read()
        assert a == open(f"{t}/g_swapped/images/{f}.jpg", "rb").read()
    # a stage file without the entry: refused, by name
    plain = f"{t}/off/models_checkpoint/model_2.pt"
    r = _run("generate_images.py", *gen, "--config-path", _gen_config(t, "gen_plain", plain), "--out-dir",
             f"{t}/g_plain", "--use-ema", cwd=t, ok=False)
    assert r.returncode != 0 and plain in (r.stdout + r.stderr) and "model_ema" in (r.stdout + r.stderr)
