"""qarig.recon_eval.ReconScorer, evaluate_reconstruction.py and train_codebook.py --val-dataset-path on the GPU at
tiny shapes (the pattern of tests/test_gpu_eval_cli.py): latents 4 x 8 x 8, a 2-layer decoder giving 3 x 32 x 32,
codebooks of 8 codes (patch 8) and 16 codes (patch 2), written directly.  The scorer is compared with a plain fp64
NumPy evaluation of the same quantities from the product's own decoder outputs, batch by batch."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import recon_metric_cases as R
from conftest import PKG

pytestmark = pytest.mark.gpu

N_VAL = 6
CODEBOOK_KEYS = {"patch_dim", "image_dim", "image_C", "num_embeddings", "neighbourhood_range", "global_steps",
                 "checkpoint"}
ERROR_KEYS = {"mse", "mae", "max_abs", "psnr", "per_image_mse"}
IMAGE_KEYS = ERROR_KEYS | {"ssim", "per_image_ssim"}
USAGE_KEYS = {"codes", "used", "dead", "perplexity", "entropy_bits", "max_share", "counts"}


def _decoder():
    from models.FC_Decoder import FC_Decoder
    return FC_Decoder(num_layers=2, image_channel=3, min_channel=8, max_channel=16, latent_channel=4,
                      hidden_activation_type="silu", use_final_activation=True, final_activation_type="tanh")


def _codebook(patch, k):
    from models.Codebook import Codebook
    cb = Codebook(patch_dim=(patch, patch), image_dim=(8, 8), image_channel=4, num_embeddings=k)
    with torch.no_grad():
        cb.codebook.weight.copy_(torch.tanh(torch.randn(cb.codebook.weight.shape)))
    return cb


def _latents(n, seed):
    return np.tanh(np.random.default_rng(seed).standard_normal((n, 4, 8, 8))).astype(np.float32)


@pytest.fixture(scope="module")
def parts():
    torch.manual_seed(0)
    dec = _decoder()
    with torch.no_grad():        # (the default initialisation decodes everything to almost the same image)
        for p in dec.parameters():
            p.copy_(torch.randn(p.shape) * 0.25)
    dec = dec.cuda()
    cbs = {"lr": _codebook(8, 8).cuda(), "hr": _codebook(2, 16).cuda()}
    z = torch.from_numpy(_latents(N_VAL, 1)).cuda()
    rng = np.random.default_rng(2)
    images = torch.from_numpy(np.tanh(rng.standard_normal((N_VAL, 32, 32, 3))).astype(np.float32)).cuda()   # NHWC
    return dec, cbs, z, images


def _score(dec, cbs, z, images, batch):
    from qarig import recon_eval
    s = recon_eval.ReconScorer(dec, cbs)
    for i in range(0, len(z), batch):
        s.add_batch(z[i:i + batch], None if images is None else images[i:i + batch])
    return s.result()


def _plain(dec, cbs, z, images, batch):
    """The same quantities the plain way: decoder outputs of the same batches, errors and SSIM in NumPy fp64."""
    got = {}

    def add(key, a, b):
        got.setdefault(key, []).append((a.cpu().numpy(), b.cpu().numpy()))

    ids_all = {name: [] for name in cbs}
    dec.eval()
    with torch.no_grad():
        for i in range(0, len(z), batch):
            zb = z[i:i + batch]
            ref = dec(zb)
            im = images[i:i + batch].permute(0, 3, 1, 2).contiguous()
            add(("autoencoder", "vs_image"), ref, im)
            for name, cb in cbs.items():
                ids = cb.get_patches_bmu(zb, reshape=True)
                zq = cb.get_quantized_image(ids)
                img = dec(zq)
                add((name, "latent"), zq, zb)
                add((name, "vs_decoder"), img, ref)
                add((name, "vs_image"), img, im)
                ids_all[name].append(ids.flatten().cpu())
    dec.train()
    out = {}
    for key, pairs in got.items():
        a = np.concatenate([p[0] for p in pairs])
        b = np.concatenate([p[1] for p in pairs])
        e = R.ref_pair_error(a, b)
        E = a[0].size
        out[key] = dict(E=E, mse=math.fsum(e[:, 0]) / (len(a) * E), mae=math.fsum(e[:, 1]) / (len(a) * E),
                        max_abs=e[:, 2].max(), per_image_mse=e[:, 0] / E,
                        per_image_ssim=R.ref_ssim(a, b, R.gaussian_window()) if key[1] != "latent" else None)
    return out, {name: torch.cat(v) for name, v in ids_all.items()}


def test_scorer_matches_a_plain_fp64_evaluation(parts):
    dec, cbs, z, images = parts
    was = [m.training for m in (dec, *cbs.values())]
    r = _score(dec, cbs, z, images, 3)
    assert [m.training for m in (dec, *cbs.values())] == was            # modes restored
    want, ids = _plain(dec, cbs, z, images, 3)
    assert set(r) == {"images", "autoencoder", "codebooks"} and r["images"] == N_VAL
    assert set(r["autoencoder"]) == {"vs_image"} and list(r["codebooks"]) == ["lr", "hr"]
    blocks = dict(r["codebooks"], autoencoder=r["autoencoder"])
    for (name, cmp), w in want.items():
        g = blocks[name][cmp]
        assert set(g) == (ERROR_KEYS if cmp == "latent" else IMAGE_KEYS), (name, cmp)
        tol = N_VAL * w["E"] * 2.0 ** -52
        print(f"{name} {cmp}: mse {g['mse']:.6e} (plain {w['mse']:.6e}), psnr {g['psnr']}, ssim {g.get('ssim')}")
        assert abs(g["mse"] - w["mse"]) <= tol * w["mse"] and abs(g["mae"] - w["mae"]) <= tol * w["mae"]
        assert g["max_abs"] == w["max_abs"] and len(g["per_image_mse"]) == N_VAL
        assert (np.abs(np.array(g["per_image_mse"]) - w["per_image_mse"]) <= w["E"] * 2.0 ** -52 * w["per_image_mse"]).all()
        assert g["psnr"] == pytest.approx(10 * math.log10(4.0 / w["mse"]), rel=1e-12)
        if cmp != "latent":
            assert np.abs(np.array(g["per_image_ssim"]) - w["per_image_ssim"]).max() <= R.SSIM_TOL
            assert abs(g["ssim"] - float(w["per_image_ssim"].mean())) <= R.SSIM_TOL
    for name, cb in cbs.items():
        u = r["codebooks"][name]["usage"]
        assert set(u) == USAGE_KEYS
        counts = torch.bincount(ids[name], minlength=cb.num_embeddings).tolist()
        assert u["counts"] == counts and u["codes"] == cb.num_embeddings
        assert u["used"] == sum(c > 0 for c in counts) and u["dead"] == cb.num_embeddings - u["used"]
        p = np.array([c for c in counts if c > 0], np.float64) / sum(counts)
        assert u["perplexity"] == pytest.approx(float(np.exp(-(p * np.log(p)).sum())), rel=1e-12)
        assert u["max_share"] == max(counts) / sum(counts)
    assert sum(r["codebooks"]["lr"]["usage"]["counts"]) == N_VAL and sum(r["codebooks"]["hr"]["usage"]["counts"]) == N_VAL * 16


def test_batch_size_does_not_change_an_image(parts):
    dec, cbs, z, _ = parts
    a, b = _score(dec, cbs, z, None, 2), _score(dec, cbs, z, None, 3)
    assert "autoencoder" not in a and set(a["codebooks"]["hr"]) == {"latent", "vs_decoder", "usage"}
    for name in cbs:
        for cmp in ("latent", "vs_decoder"):
            for key in ("per_image_mse", "per_image_ssim", "mse", "mae", "max_abs", "ssim"):
                if key in a["codebooks"][name][cmp]:
                    assert a["codebooks"][name][cmp][key] == b["codebooks"][name][cmp][key], (name, cmp, key)
        assert a["codebooks"][name]["usage"] == b["codebooks"][name]["usage"]


def test_codebook_of_the_latents_own_patches_is_lossless(parts):
    from qarig import ops
    dec, _, z, _ = parts
    own = _codebook(8, 8).cuda()
    with torch.no_grad():
        own.codebook.weight[:N_VAL].copy_(ops.patchify(z, (8, 8)).reshape(N_VAL, -1))
    r = _score(dec, {"own": own}, z, None, 3)["codebooks"]["own"]
    assert r["latent"]["mse"] == 0.0 and r["latent"]["psnr"] is None and r["latent"]["max_abs"] == 0.0
    assert abs(r["vs_decoder"]["ssim"] - 1.0) <= R.SSIM_TOL and r["vs_decoder"]["mse"] == 0.0
    assert r["usage"]["used"] == N_VAL and r["usage"]["dead"] == 2
    assert r["usage"]["perplexity"] == pytest.approx(float(N_VAL), rel=1e-12)


def test_scorer_refuses_what_it_cannot_score(parts):
    from qarig import recon_eval
    dec, cbs, z, images = parts
    s = recon_eval.ReconScorer(dec, cbs)
    with pytest.raises(RuntimeError):
        s.result()
    with pytest.raises(ValueError, match=r"16.*32|32.*16"):
        s.add_batch(z[:2], images[:2, :16])
    assert dec.training and all(cb.training for cb in cbs.values())      # modes restored after the error, too

    class Cropped(torch.nn.Module):      # a decoder whose output is smaller than the SSIM window
        def forward(self, latent):
            return dec(latent)[:, :, :10, :12].contiguous()

    with pytest.raises(RuntimeError, match="10 x 12 is smaller than the window"):
        recon_eval.ReconScorer(Cropped(), cbs).add_batch(z[:2])
    # no codebooks: the autoencoder alone
    r = _score(dec, {}, z, images, 4)
    assert r["codebooks"] == {} and set(r["autoencoder"]["vs_image"]) == IMAGE_KEYS


# ---------------------------------------------------------------------------------------------- command lines
def _run(script, *args, cwd, ok=True):
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(PKG, script), *map(str, args)], cwd=cwd, env=env,
                       capture_output=True, text=True, timeout=300)
    if ok:
        assert r.returncode == 0, f"{script} failed:\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    return r


def _dataset(t, name, n, seed, images):
    from PIL import Image
    from dataset_loader._tinydb_json import write_all
    rng = np.random.default_rng(seed + 100)
    recs = []
    for i, zi in enumerate(_latents(n, seed)):
        p = os.path.join(t, f"{name}{i}.npy")
        np.save(p, zi)
        ip = ""
        if images:
            ip = os.path.join(t, f"{name}{i}.png")
            Image.fromarray(rng.integers(0, 256, (32, 32, 3), dtype=np.uint8)).save(ip)
        recs.append({"fmap_path": p, "image_path": ip})
    write_all(f"{t}/{name}.json", recs)
    return f"{t}/{name}.json"


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    from utils.model_utils import save_model
    t = str(tmp_path_factory.mktemp("recon_cli"))
    torch.manual_seed(0)
    train, val = _dataset(t, "z", 12, 0, False), _dataset(t, "v", N_VAL, 1, True)
    dec_cfg = dict(num_layers=2, image_channel=3, min_channel=8, max_channel=16, latent_channel=4,
                   hidden_activation_type="silu", use_final_dec_activation=True, decoder_activation_type="tanh")
    save_model(f"{t}/dec", "model.pt", dict(dec_cfg, model=_decoder().state_dict()))
    for name, patch, k in (("lr", 8, 8), ("hr", 2, 16)):
        save_model(f"{t}/cb_{name}", "codebook.pt",
                   dict(patch_dim=(patch, patch), image_dim=(8, 8), image_C=4, num_embeddings=k,
                        neighbourhood_range=1, global_steps=0, checkpoint=_codebook(patch, k).state_dict()))
    dec = f"{t}/dec/models_checkpoint/model.pt"
    score = ["--device", "cuda", "--dataset-path", val, "--decoder-path", dec, "--batch-size", 4]
    cbs = ["--codebook-path", f"{t}/cb_lr/models_checkpoint/codebook.pt", "--codebook-path",
           f"{t}/cb_hr/models_checkpoint/codebook.pt"]
    out = {}
    r = _run("evaluate_reconstruction.py", *score, *cbs, "--with-images", "--out-json", f"{t}/full/r.json", cwd=t)
    out["full"] = r.stdout + r.stderr
    _run("evaluate_reconstruction.py", *score, *cbs, "--out-json", f"{t}/plain.json", cwd=t)
    _run("evaluate_reconstruction.py", *score, *cbs, "--with-images", "--max-batches", 1, "--out-json",
         f"{t}/first.json", cwd=t)
    json.dump(dict(model_lr=1e-2, neighbourhood_step=2, image_H=8, image_W=8, image_C=4, patch_H=2, patch_W=2,
                   num_embeddings=16), open(f"{t}/cb.json", "w"))
    common = ["--device", "cuda", "--dataset-path", train, "--decoder-path", dec, "--batch-size", 4,
              "--checkpoint-step", 2, "--max-epoch", 1, "--max-steps", 3, "--config-path", f"{t}/cb.json"]
    r = _run("train_codebook.py", *common, "--out-dir", f"{t}/val", "--val-dataset-path", val, cwd=t)
    out["val"] = r.stdout + r.stderr
    r = _run("train_codebook.py", *common, "--out-dir", f"{t}/one", "--val-dataset-path", val, "--val-step", 1,
             "--val-batches", 1, cwd=t)
    out["one"] = r.stdout + r.stderr
    r = _run("train_codebook.py", *common, "--out-dir", f"{t}/off", cwd=t)
    out["off"] = r.stdout + r.stderr
    return dict(t=t, out=out, score=score)


def _tree(root):
    return sorted(os.path.relpath(os.path.join(dp, f), root) for dp, _, fs in os.walk(root) for f in fs)


def test_evaluate_cli_writes_the_result_dict(runs):
    t = runs["t"]
    full = json.load(open(f"{t}/full/r.json"))
    assert set(full) == {"images", "autoencoder", "codebooks"} and full["images"] == N_VAL
    assert list(full["codebooks"]) == ["codebook", "codebook_2"]           # the file stems, de-duplicated
    assert set(full["autoencoder"]) == {"vs_image"} and set(full["autoencoder"]["vs_image"]) == IMAGE_KEYS
    for name, k in (("codebook", 8), ("codebook_2", 16)):
        b = full["codebooks"][name]
        assert set(b) == {"latent", "vs_decoder", "vs_image", "usage"}
        assert set(b["latent"]) == ERROR_KEYS and set(b["vs_decoder"]) == IMAGE_KEYS == set(b["vs_image"])
        assert set(b["usage"]) == USAGE_KEYS and b["usage"]["codes"] == k == len(b["usage"]["counts"])
        for cmp in ("latent", "vs_decoder", "vs_image"):
            assert len(b[cmp]["per_image_mse"]) == N_VAL and b[cmp]["mse"] > 0
            assert b[cmp]["psnr"] == pytest.approx(10 * math.log10(4.0 / b[cmp]["mse"]), rel=1e-12)
        assert len(b["vs_image"]["per_image_ssim"]) == N_VAL and -1.0 <= b["vs_decoder"]["ssim"] <= 1.0
        assert b["vs_image"]["mse"] > b["vs_decoder"]["mse"]               # random images are far from everything
    log = runs["out"]["full"]
    assert log.count("Eval autoencoder Image MSE: ") == 1 and log.count(" Latent MSE: ") == 2
    assert "Eval codebook_2 Latent MSE: {:.6f}".format(full["codebooks"]["codebook_2"]["latent"]["mse"]) in log
    # without --with-images: no source-image comparison anywhere, the rest bit for bit the same
    plain = json.load(open(f"{t}/plain.json"))
    assert set(plain) == {"images", "codebooks"}
    for name in plain["codebooks"]:
        assert set(plain["codebooks"][name]) == {"latent", "vs_decoder", "usage"}
        for key in ("latent", "vs_decoder", "usage"):
            assert plain["codebooks"][name][key] == full["codebooks"][name][key]
    # --max-batches 1: the first batch's entries
    first = json.load(open(f"{t}/first.json"))
    assert first["images"] == 4
    assert first["autoencoder"]["vs_image"]["per_image_ssim"] == full["autoencoder"]["vs_image"]["per_image_ssim"][:4]
    for name in first["codebooks"]:
        for cmp in ("latent", "vs_decoder", "vs_image"):
            assert first["codebooks"][name][cmp]["per_image_mse"] == full["codebooks"][name][cmp]["per_image_mse"][:4]


def test_evaluate_cli_refuses_the_cpu(runs):
    r = _run("evaluate_reconstruction.py", "--device", "cpu", *runs["score"][2:], cwd=runs["t"], ok=False)
    assert r.returncode != 0 and "MI355X" in r.stdout + r.stderr


def _lines(path):
    return [json.loads(ln) for ln in open(path).read().splitlines()]


def test_codebook_training_with_validation(runs):
    t = runs["t"]
    lines = _lines(f"{t}/val/val_log.jsonl")
    assert [ln["step"] for ln in lines] == [0, 2]                          # --val-step defaults to --checkpoint-step
    for ln in lines:
        assert set(ln) == {"step", "codebook"} and set(ln["codebook"]) == {"latent", "vs_decoder", "usage"}
        assert set(ln["codebook"]["latent"]) == ERROR_KEYS - {"per_image_mse"}
        assert set(ln["codebook"]["vs_decoder"]) == IMAGE_KEYS - {"per_image_mse", "per_image_ssim"}
        assert sum(ln["codebook"]["usage"]["counts"]) == N_VAL * 16
    log = runs["out"]["val"]
    assert log.count("Val Latent MSE: ") == 2 and "Validation: 6 latents every 2 steps" in log
    last = lines[-1]["codebook"]
    assert "Val Latent MSE: {:.6f} | PSNR: {:.3f} | SSIM: {:.5f} | used: {} / 16 | perplexity: {:.2f}".format(
        last["latent"]["mse"], last["vs_decoder"]["psnr"], last["vs_decoder"]["ssim"], last["usage"]["used"],
        last["usage"]["perplexity"]) in log
    # the saved checkpoint scores the same, bit for bit
    _run("evaluate_reconstruction.py", *runs["score"], "--codebook-path", f"{t}/val/models_checkpoint/codebook_2.pt",
         "--out-json", f"{t}/ckpt.json", cwd=t)
    ckpt = json.load(open(f"{t}/ckpt.json"))["codebooks"]["codebook_2"]
    assert ckpt["latent"]["mse"] == last["latent"]["mse"] and ckpt["usage"] == last["usage"]
    assert ckpt["vs_decoder"]["mse"] == last["vs_decoder"]["mse"] and ckpt["vs_decoder"]["ssim"] == last["vs_decoder"]["ssim"]
    # --val-step 1, --val-batches 1
    lines = _lines(f"{t}/one/val_log.jsonl")
    assert [ln["step"] for ln in lines] == [0, 1, 2]
    assert all(sum(ln["codebook"]["usage"]["counts"]) == 4 * 16 for ln in lines)


def test_without_the_flag_nothing_is_added(runs):
    t = runs["t"]
    assert "Val" not in runs["out"]["off"] and "val" not in open(f"{t}/off/Codebook.log").read().lower()
    files = _tree(f"{t}/off")
    assert files == sorted(["Codebook.log", "images/image_plot_0.jpg", "images/image_plot_2.jpg",
                            "images/quant_image_plot_0.jpg", "images/quant_image_plot_2.jpg",
                            "models_checkpoint/codebook_0.pt", "models_checkpoint/codebook_2.pt"])
    assert _tree(f"{t}/val") == sorted(files + ["val_log.jsonl"])
    for run in ("off", "val"):
        md = torch.load(f"{t}/{run}/models_checkpoint/codebook_2.pt", map_location="cpu", weights_only=True)
        assert set(md) == CODEBOOK_KEYS and set(md["checkpoint"]) == {"codebook.weight"}
