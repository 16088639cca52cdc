"""Training against SSIM end to end: every parameter gradient of a small autoencoder under mse + 0.5 ssim_loss
against the oracle in fp64, and train_autoencoder.py with and without --ssim-weight.

The command-line runs use a dataset of exactly one batch (4 images, batch 4, three epochs = three steps) and start
from a checkpoint written here, so step 1 sees all four images under known weights: its logged numbers are
reproduced from the same images whatever order the loader drew them in."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import ssim_loss_cases as S
from conftest import PKG, grad_err, load_golden

pytestmark = pytest.mark.gpu

AE = dict(num_layers=2, image_channel=3, min_channel=8, max_channel=16, latent_channel=4, hidden_activation_type="silu",
          use_final_enc_activation=True, encoder_activation_type="tanh", use_final_dec_activation=True,
          decoder_activation_type="tanh")
PLAIN_LINE = r"Cum\. Steps: (\d+) \| Steps: 1 / 1 \| L\.R\.: \d\.\d{8} \| Recon Loss: (\d+\.\d{5})"
SSIM_LINE = PLAIN_LINE + r" \| MSE: (\d+\.\d{5}) \| SSIM: (-?\d+\.\d{5})"


def test_autoencoder_gradients_under_mse_plus_ssim_vs_oracle_fp64():
    """The gradient entering the decoder is accurate to one fp32 rounding; everything behind it is code already
    held to grad_err < 2e-5 (tests/test_gpu_conv.py), so that figure holds here too."""
    from models.Autoencoder import Autoencoder
    from oracle import ref_models as rm
    from qarig import functional as QF
    sd = {k: v.double().requires_grad_(True) for k, v in load_golden("autoencoder")["sd"].items()}
    x = torch.tanh(torch.randn((2, 3, 32, 32), generator=torch.Generator().manual_seed(11)))
    names = list(sd)
    recon = rm.autoencoder(sd, x.double(), enc_act="tanh")
    ref_ssim = S.torch_ssim(recon, x.double(), S.window("gauss11"))
    ref_loss = torch.mean((recon - x.double()) ** 2) + 0.5 * (1.0 - ref_ssim.mean())
    ref_grads = torch.autograd.grad(ref_loss, [sd[k] for k in names])
    m = Autoencoder(**AE)
    m.custom_load_state_dict({k: v.detach().float() for k, v in sd.items()})
    m = m.cuda()
    xg = x.cuda()
    out = m(xg)
    mse, term = QF.mse_loss(out, xg), QF.ssim_loss(out, xg)
    loss = mse + 0.5 * term
    loss.backward()
    got_loss, want_loss = float(loss.detach()), float(ref_loss.detach())
    print(f"loss {got_loss:.6f} (oracle {want_loss:.6f}), ssim {1 - float(term.detach()):.6f} "
          f"(oracle {float(ref_ssim.detach().mean()):.6f})")
    assert abs(got_loss - want_loss) < 1e-5 * max(1.0, abs(want_loss))
    got = dict(m.named_parameters())
    assert set(got) == set(names)
    for k, g in zip(names, ref_grads):
        err = grad_err(got[k].grad, g)
        print(f"  {k}: grad_err {err:.2e}")
        assert err < 2e-5, k
    # the SSIM term alone moves the gradients: mse by itself is not within the bound of the sum
    mse_grads = torch.autograd.grad(torch.mean((rm.autoencoder(sd, x.double(), enc_act="tanh") - x.double()) ** 2),
                                    [sd[k] for k in names])
    assert max(grad_err(a, b) for a, b in zip(mse_grads, ref_grads)) > 1e-2


def _run(*args, cwd):
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(PKG, "train_autoencoder.py"), *map(str, args)], cwd=cwd, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"train_autoencoder.py failed:\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    return r.stdout + r.stderr


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    from PIL import Image
    from dataset_loader._tinydb_json import write_all
    from models.Autoencoder import Autoencoder
    from utils.model_utils import save_model
    t = str(tmp_path_factory.mktemp("ssim_cli"))
    rng = np.random.default_rng(0)
    recs = []
    for i in range(4):
        p = os.path.join(t, f"img{i}.png")
        # smooth blobs plus noise: an untrained network's output is then not at SSIM 0
        base = np.kron(rng.integers(0, 255, (4, 4, 3)), np.ones((8, 8, 1)))
        Image.fromarray(np.clip(base + rng.integers(-20, 20, (32, 32, 3)), 0, 255).astype(np.uint8)).save(p)
        recs.append({"image_fpath": p})
    write_all(os.path.join(t, "dataset.json"), recs)
    json.dump(dict(AE, model_lr=1e-3), open(os.path.join(t, "ae.json"), "w"))
    torch.manual_seed(4)
    save_model(f"{t}/init", "model.pt", dict(AE, model={k: v.detach().clone() for k, v in Autoencoder(**AE).state_dict().items()}))
    common = ["--device", "cuda", "--dataset-path", f"{t}/dataset.json", "--batch-size", 4, "--checkpoint-step", 2,
              "--max-epoch", 3, "--config-path", f"{t}/ae.json", "--model-path", f"{t}/init/models_checkpoint/model.pt"]
    return t, common


def test_cli_with_the_flag_logs_and_checkpoints_the_ssim_term(setup):
    from dataset_loader.image_dataset import ImageDataset
    from models.Autoencoder import Autoencoder
    from qarig import ops
    from utils.model_utils import load_model
    t, common = setup
    log = _run(*common, "--out-dir", f"{t}/on", "--ssim-weight", 0.5, cwd=t)
    lines = [m for m in (re.search(SSIM_LINE + "$", ln) for ln in log.splitlines()) if m]
    assert [int(m.group(1)) for m in lines] == [1, 2, 3], log[-2000:]
    for step in (0, 2):
        ok, ck = load_model(f"{t}/on/models_checkpoint/model_{step}.pt")          # the weights-only unpickler
        assert ok and set(ck) == set(AE) | {"model", "model_optimizer", "ssim_weight"}
        assert type(ck["ssim_weight"]) is float and ck["ssim_weight"] == 0.5
    assert os.path.exists(f"{t}/on/images/recon_0.jpg") and os.path.exists(f"{t}/on/images/ground_truth_0.jpg")
    # step 1 from the starting weights on the four images (the saved JPEGs are lossy, the checkpoint of step 1 holds
    # the weights after the update: neither reproduces the step's reconstruction)
    ok, init = load_model(f"{t}/init/models_checkpoint/model.pt")
    m = Autoencoder(**AE)
    m.custom_load_state_dict(init["model"])
    m = m.cuda().train()
    ds = ImageDataset(f"{t}/dataset.json")
    x = torch.stack([ds[i] for i in range(4)]).cuda()
    recon = m(x).detach()
    ssim = float(ops.ssim(recon, x).mean())
    mse = float(((recon.double() - x.double()) ** 2).mean())
    loss, lmse, lssim = (float(lines[0].group(k)) for k in (2, 3, 4))
    print(f"step 1: logged loss {loss} mse {lmse} ssim {lssim}; recomputed mse {mse:.7f} ssim {ssim:.7f}")
    # five printed decimals (half a unit) plus the fp32 roundings of the loss terms
    assert abs(lssim - ssim) <= 6e-6 and abs(lmse - mse) <= 6e-6
    assert abs(loss - (mse + 0.5 * (1.0 - ssim))) <= 6e-6
    for m_ in lines:                                                            # the parts add up on every line
        assert abs(float(m_.group(2)) - (float(m_.group(3)) + 0.5 * (1.0 - float(m_.group(4))))) <= 2e-5


def test_cli_without_the_flag_is_unchanged(setup):
    """Passes before this feature as well: it is here to keep it so."""
    from utils.model_utils import load_model
    t, common = setup
    log = _run(*common, "--out-dir", f"{t}/off", cwd=t)
    steps = [ln for ln in log.splitlines() if "Cum. Steps" in ln]
    assert len(steps) == 3
    for i, ln in enumerate(steps):
        m = re.search(PLAIN_LINE + "$", ln)
        assert m and int(m.group(1)) == i + 1, ln
    assert "SSIM" not in log and "MSE:" not in log
    for step in (0, 2):
        ok, ck = load_model(f"{t}/off/models_checkpoint/model_{step}.pt")
        assert ok and set(ck) == set(AE) | {"model", "model_optimizer"}
    assert sorted(os.listdir(f"{t}/off/images")) == ["ground_truth_0.jpg", "ground_truth_2.jpg", "recon_0.jpg",
                                                     "recon_2.jpg"]
