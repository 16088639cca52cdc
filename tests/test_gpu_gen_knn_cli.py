"""evaluate_generation.py --knn / --save-neighbours end to end on the GPU at tiny shapes (the pattern of
tests/test_gpu_gen_eval_cli.py).  26 real and 15 generated latents of 4 x 8 x 8 on a 2^-12 grid, pool 4: D = 16, and
every pooled feature is exact in fp64, so the brute-force NumPy statistics see the very rows the kernels see."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gen_knn_cases as K
from conftest import PKG

pytestmark = pytest.mark.gpu

N_REAL, N_GEN, C, H, W, POOL = 26, 15, 4, 8, 8, 4
PLAIN_KEYS = {"counts", "dim", "pool", "space", "note", "fd_real_generated", "fd_real_split"}


def _run(*args, cwd, ok=True):
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(PKG, "evaluate_generation.py"), *map(str, args)], cwd=cwd, env=env,
                       capture_output=True, text=True, timeout=300)
    if ok:
        assert r.returncode == 0, f"evaluate_generation.py failed:\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    return r


def _pooled(z):
    n = z.shape[0]
    return z.astype(np.float64).reshape(n, C, H // POOL, POOL, W // POOL, POOL).mean(axis=(3, 5)).reshape(n, -1)


@pytest.fixture(scope="module")
def box(tmp_path_factory):
    sys.path.insert(0, PKG)
    from dataset_loader._tinydb_json import write_all
    t = str(tmp_path_factory.mktemp("gen_knn_cli"))
    rng = np.random.default_rng(0)
    real = (np.round(np.tanh(rng.standard_normal((N_REAL, C, H, W))) * 4096) / 4096).astype(np.float32)
    gen = (np.round(np.tanh(1.3 * rng.standard_normal((N_GEN, C, H, W)) + 0.1) * 4096) / 4096).astype(np.float32)
    gen[4] = real[9]                                      # a copied training sample
    recs = []
    for i in range(N_REAL):
        p = os.path.join(t, f"z{i}.npy")
        np.save(p, real[i])
        recs.append({"fmap_path": p, "image_path": ""})
    write_all(f"{t}/real.json", recs)
    np.save(f"{t}/gen.npy", gen)
    np.save(f"{t}/few.npy", gen[:3])
    base = ["--device", "cuda", "--real-dataset-path", f"{t}/real.json", "--feature-pool", POOL, "--batch-size", 7]
    return dict(t=t, base=base, fr=_pooled(real), fg=_pooled(gen))


def test_knn_adds_the_manifold_and_leaves_the_rest_alone(box):
    t = box["t"]
    _run(*box["base"], "--generated-latents", f"{t}/gen.npy", "--out-json", f"{t}/plain.json", cwd=t)
    r = _run(*box["base"], "--generated-latents", f"{t}/gen.npy", "--out-json", f"{t}/knn.json", "--knn", 3,
             "--save-neighbours", f"{t}/nn/neighbours.npz", cwd=t)
    plain, knn = json.load(open(f"{t}/plain.json")), json.load(open(f"{t}/knn.json"))
    assert set(plain) == PLAIN_KEYS and set(knn) == PLAIN_KEYS | {"manifold"}
    assert {k: v for k, v in knn.items() if k != "manifold"} == plain
    fr, fg = box["fr"], box["fg"]
    m = knn["manifold"]
    assert m["k"] == 3 and m["counts"] == {"real": 26, "real_a": 13, "real_b": 13, "generated": 15}
    assert m["dropped"] == {"real": 0, "real_a": 0, "real_b": 0, "generated": 0}
    assert m["real_generated"] == K.ref_metrics(fr, fg, 3)
    assert m["real_split"] == K.ref_metrics(fr[0::2], fr[1::2], 3)
    d = np.sqrt(((fg[:, None] - fr[None]) ** 2).sum(axis=2))
    near = np.sort(d.min(axis=1))
    # the copy: the Gram form leaves at most (D + 8) 2^-53 4 |a|^2 < 1e-13 of its squared distance of 0
    assert near[0] == 0.0 and 0.0 <= m["nn_generated_real"]["min"] == m["nn_generated_real"]["q01"] <= 1e-6
    for name, at in (("q10", 1), ("q50", 7)):
        assert m["nn_generated_real"][name] == pytest.approx(near[at], rel=1e-12)
    split = np.sort(np.sqrt(((fr[1::2][:, None] - fr[0::2][None]) ** 2).sum(axis=2)).min(axis=1))
    assert m["nn_real_split"]["q50"] == pytest.approx(split[6], rel=1e-12)
    assert "depend on k" in m["note"]
    log = r.stdout + r.stderr
    assert "precision=" in log and "coverage=" in log and "real_split" in log and "nearest-neighbour distance" in log
    # the neighbours file: what nearest_real returns, in dataset order
    z = np.load(f"{t}/nn/neighbours.npz")
    assert set(z.files) == {"index", "distance"} and z["index"].shape == z["distance"].shape == (N_GEN,)
    assert np.array_equal(z["index"], d.argmin(axis=1)) and z["index"][4] == 9 and 0.0 <= z["distance"][4] <= 1e-6
    from qarig import gen_eval
    shift = torch.from_numpy(fr[:7].mean(axis=0)).cuda()
    idx, d2 = gen_eval.nearest_real(torch.from_numpy(fg).cuda(), torch.from_numpy(fr).cuda(), shift)
    assert np.array_equal(z["index"], idx.cpu().numpy())
    assert np.allclose(z["distance"], np.sqrt(np.maximum(d2.cpu().numpy(), 0.0)), rtol=1e-12, atol=1e-6)
    assert np.allclose(z["distance"], d.min(axis=1), rtol=1e-12, atol=1e-6)


def test_the_cap_is_applied_and_logged(box):
    t = box["t"]
    r = _run(*box["base"], "--generated-latents", f"{t}/gen.npy", "--out-json", f"{t}/cap.json", "--knn", 3,
             "--knn-max-samples", 12, cwd=t)
    m = json.load(open(f"{t}/cap.json"))["manifold"]
    assert m["counts"] == {"real": 12, "real_a": 6, "real_b": 6, "generated": 12}
    assert m["dropped"] == {"real": 14, "real_a": 7, "real_b": 7, "generated": 3}
    assert m["real_generated"] == K.ref_metrics(box["fr"][:12], box["fg"][:12], 3)
    assert "--knn-max-samples 12 dropped 14 samples of set 'real'" in r.stdout + r.stderr


def test_too_few_samples_are_refused_with_a_clear_message(box):
    t = box["t"]
    r = _run(*box["base"], "--generated-latents", f"{t}/few.npy", "--out-json", f"{t}/few.json", "--knn", 3, cwd=t,
             ok=False)
    assert r.returncode != 0 and "--knn 3 needs at least 4 samples" in r.stdout + r.stderr
    assert "generated (3)" in r.stdout + r.stderr and not os.path.exists(f"{t}/few.json")
    r = _run(*box["base"], "--generated-latents", f"{t}/gen.npy", "--out-json", f"{t}/few.json", "--knn", 3,
             "--max-batches", 1, cwd=t, ok=False)                       # 7 real samples: halves of 4 and 3
    assert r.returncode != 0 and "real_b (3)" in r.stdout + r.stderr and not os.path.exists(f"{t}/few.json")
    r = _run(*box["base"], "--generated-latents", f"{t}/gen.npy", "--save-neighbours", f"{t}/x.npz", cwd=t, ok=False)
    assert r.returncode != 0 and "--save-neighbours needs --knn" in r.stdout + r.stderr
