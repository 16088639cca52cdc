"""evaluate_generation.py and generate_images.py --save-latents end to end on the GPU at tiny shapes (the pattern of
tests/test_gpu_eval_cli.py: decoder, codebooks, a Transformer and latents written directly).  24 latents of 4 x 8 x 8,
pool 4: D = 16.  The latents sit on a 2^-12 grid, so that "real + 0.5" is exact in fp32 and the mean term has a closed
form to rounding."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import PKG

pytestmark = pytest.mark.gpu

N_REAL, C, H, W, POOL = 24, 4, 8, 8, 4
D = C * (H // POOL) * (W // POOL)
DIST_KEYS = {"fd", "mean_term", "cov_term", "clipped"}


def _run(script, *args, cwd, ok=True):
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(PKG, script), *map(str, args)], cwd=cwd, env=env,
                       capture_output=True, text=True, timeout=300)
    if ok:
        assert r.returncode == 0, f"{script} failed:\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    return r


@pytest.fixture(scope="module")
def box(tmp_path_factory):
    sys.path.insert(0, PKG)
    from dataset_loader._tinydb_json import write_all
    from models.Codebook import Codebook
    from models.FC_Decoder import FC_Decoder
    from models.Transformer import Transformer
    from utils.model_utils import save_model
    t = str(tmp_path_factory.mktemp("gen_eval_cli"))
    torch.manual_seed(0)
    rng = np.random.default_rng(0)
    real = (np.round(np.tanh(rng.standard_normal((N_REAL, C, H, W))) * 4096) / 4096).astype(np.float32)
    recs = []
    for i in range(N_REAL):
        p = os.path.join(t, f"z{i}.npy")
        np.save(p, real[i])
        recs.append({"fmap_path": p, "image_path": ""})
    write_all(f"{t}/real.json", recs)
    np.save(f"{t}/same.npy", real)
    np.save(f"{t}/moved.npy", real + np.float32(0.5))
    np.save(f"{t}/wrong_shape.npy", np.zeros((5, C, 4, 4), np.float32))
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
    # a one-stage (base) cascade: 8 LR + 16 HR embeddings, 16 + <end> outputs, no sliding window
    hp = dict(train_base_model=True, use_sliding_window=False, sliding_window=None, num_enc_embedding=None,
              num_dec_embedding=24, num_enc_layers=None, num_dec_layers=1, self_attn_heads=2, cross_attn_heads=None,
              transformer_in_dim=16, transformer_out_dim=17, transformer_hidden_dim=32, hidden_activation="silu")
    m = Transformer(use_encoder=False, use_pos_cond=False, num_enc_layers=None, num_dec_layers=1,
                    num_enc_embedding=None, num_dec_embedding=24, self_attn_heads=2, cross_attn_heads=None,
                    transformer_in_dim=16, transformer_out_dim=17, transformer_hidden_dim=32, hidden_activation="silu")
    save_model(f"{t}/tr", "model.pt", dict(hp, model=m.state_dict()))
    json.dump({"0": dict(model_path=f"{t}/tr/models_checkpoint/model.pt", temperature=1.0,
                         lr_codebook_path=f"{t}/cb_lr/models_checkpoint/codebook.pt",
                         hr_codebook_path=f"{t}/cb_hr/models_checkpoint/codebook.pt", num_beam=1, beam_width=4)},
              open(f"{t}/gen.json", "w"))
    paths = dict(dec=f"{t}/dec/models_checkpoint/model.pt", hr=f"{t}/cb_hr/models_checkpoint/codebook.pt")
    base = ["--device", "cuda", "--real-dataset-path", f"{t}/real.json", "--feature-pool", POOL, "--batch-size", 10]
    # the spectral norm of the real set's feature covariance, for the zero-distance bound
    pooled = real.astype(np.float64).reshape(N_REAL, C, H // POOL, POOL, W // POOL, POOL).mean(axis=(3, 5))
    norm = float(np.linalg.norm(np.cov(pooled.reshape(N_REAL, D), rowvar=False), 2))
    return dict(t=t, base=base, real=real, floor=2 * D * 2.0 ** -26 * norm, **paths)


def _score(box, name, *args, ok=True):
    t = box["t"]
    r = _run("evaluate_generation.py", *box["base"], *args, "--out-json", f"{t}/{name}.json", cwd=t, ok=ok)
    return (json.load(open(f"{t}/{name}.json")) if ok else None), r.stdout + r.stderr


def test_the_same_latents_are_at_distance_zero_and_the_floors_are_reported(box):
    r, log = _score(box, "same", "--generated-latents", f"{box['t']}/same.npy", "--hr-codebook-path", box["hr"])
    assert set(r) == {"counts", "dim", "pool", "space", "note", "fd_real_generated", "fd_quantised_generated",
                      "fd_real_quantised", "fd_real_split"}
    for key in ("fd_real_generated", "fd_quantised_generated", "fd_real_quantised", "fd_real_split"):
        assert set(r[key]) == DIST_KEYS and r[key]["fd"] == r[key]["mean_term"] + r[key]["cov_term"]
    assert (r["dim"], r["pool"], r["space"]) == (D, POOL, "latent") and "not fid" in r["note"].lower()
    assert r["counts"] == {"real": 24, "real_a": 12, "real_b": 12, "quantised": 24, "generated": 24}
    print(f"fd(real, the same latents) = {r['fd_real_generated']['fd']:.3e}, bound {box['floor']:.3e}")
    assert abs(r["fd_real_generated"]["fd"]) <= box["floor"]
    assert r["fd_real_quantised"]["fd"] > 0 and r["fd_real_split"]["fd"] > 0
    assert r["fd_quantised_generated"]["fd"] == pytest.approx(r["fd_real_quantised"]["fd"], rel=1e-9)
    assert "not FID" in log and "Warning" in log and "fewer than 2 D" in log        # 24 < 2 x 16 samples


def test_a_constant_offset_is_the_mean_term(box):
    r, _ = _score(box, "moved", "--generated-latents", f"{box['t']}/moved.npy")
    d = r["fd_real_generated"]
    assert d["mean_term"] == pytest.approx(D * 0.25, rel=1e-12)
    assert abs(d["cov_term"]) <= box["floor"]
    assert "fd_real_quantised" not in r and "quantised" not in r["counts"]           # no codebook given


def test_image_space(box):
    r, _ = _score(box, "image", "--generated-latents", f"{box['t']}/same.npy", "--space", "image", "--decoder-path",
                  box["dec"])
    from qarig import cli_common as cc
    dec, _ = cc.load_decoder(box["dec"], torch.device("cuda"))
    with torch.no_grad():
        img = dec.eval()(torch.from_numpy(box["real"]).cuda()).double().cpu().numpy()
    _, ic, ih, iw = img.shape
    dim = 3 * (ih // POOL) * (iw // POOL)
    assert ic == 3 and r["dim"] == dim and r["space"] == "image" and r["counts"]["generated"] == 24
    # 24 samples of `dim` > 24 features: a rank-deficient covariance against itself, the zero-eigenvalue bound again
    pooled = img.reshape(N_REAL, ic, ih // POOL, POOL, iw // POOL, POOL).mean(axis=(3, 5)).reshape(N_REAL, dim)
    floor = 2 * dim * 2.0 ** -26 * float(np.linalg.norm(np.cov(pooled, rowvar=False), 2))
    print(f"image space: fd(real, the same latents) = {r['fd_real_generated']['fd']:.3e}, bound {floor:.3e}")
    assert abs(r["fd_real_generated"]["fd"]) <= floor


def test_refusals(box):
    t = box["t"]
    _, log = _score(box, "bad", "--generated-latents", f"{t}/wrong_shape.npy", ok=False)
    assert "do not share an autoencoder" in log and "(5, 4, 4, 4)" in log and not os.path.exists(f"{t}/bad.json")
    base = [a for a in box["base"]]
    base[base.index("--feature-pool") + 1] = 1
    r = _run("evaluate_generation.py", *base, "--generated-latents", f"{t}/same.npy", "--space", "image",
             "--decoder-path", box["dec"], "--out-json", f"{t}/big.json", cwd=t, ok=False)
    assert r.returncode != 0 and "larger --feature-pool" in r.stdout + r.stderr and "1,024" in r.stdout + r.stderr
    assert not os.path.exists(f"{t}/big.json")


def test_generate_images_saves_the_latents_it_decodes(box):
    t = box["t"]
    gen = ["--device", "cuda", "--decoder-path", box["dec"], "--num-images", 5, "--seed", 7, "--config-path",
           f"{t}/gen.json"]
    _run("generate_images.py", *gen, "--out-dir", f"{t}/g1", "--save-latents", f"{t}/g1/latents.npy", cwd=t)
    _run("generate_images.py", *gen, "--out-dir", f"{t}/g2", "--save-latents", f"{t}/g2/latents.npy", cwd=t)
    z = np.load(f"{t}/g1/latents.npy")
    assert z.dtype == np.float32 and z.shape == (5, C, H, W)
    assert np.array_equal(z.view(np.uint32), np.load(f"{t}/g2/latents.npy").view(np.uint32))     # the same seed
    assert os.path.exists(f"{t}/g1/images/recon_model_0.jpg")
    # it is a quantised image: tokenising it with the stage's codebook and gathering those codes returns its bits
    from qarig import cli_common as cc
    cb, _ = cc.load_codebook(box["hr"], torch.device("cuda"))
    zt = torch.from_numpy(z).cuda()
    ids = cb.get_patches_bmu(zt, reshape=True)
    assert ids.shape == (5, 16) and torch.equal(cb.get_quantized_image(ids), zt)
    r, _ = _score(box, "generated", "--generated-latents", f"{t}/g1/latents.npy", "--hr-codebook-path", box["hr"])
    assert r["counts"]["generated"] == 5 and r["fd_real_generated"]["fd"] > 0
    assert r["fd_quantised_generated"]["fd"] > 0
