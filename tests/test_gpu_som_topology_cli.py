"""evaluate_reconstruction.py --topology and train_codebook.py --val-topology on the GPU, on the tiny fixtures of
tests/test_gpu_recon_eval.py (latents 4 x 8 x 8, codebooks of 8 codes / patch 8 and 16 codes / patch 2)."""
import json
import re

import pytest
import torch

import test_gpu_recon_eval as G

pytestmark = pytest.mark.gpu

TOPOLOGY_KEYS = {"rows", "topographic_error", "within", "within_uniform", "mean_gap", "median_gap",
                 "quantisation_error", "second_error", "quantisation_mse", "ratio_hist", "lag",
                 "per_image_quantisation_error"}
LAG_KEYS = {"mean_distance", "all_pairs_mean", "lag_half"}


def _messages(log):
    """Log lines without their time stamps."""
    return [re.sub(r"^\S+ \S+ ", "", ln) for ln in log.splitlines() if re.match(r"^\d{4}-\d\d-\d\d ", ln)]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    from utils.model_utils import save_model
    t = str(tmp_path_factory.mktemp("topology_cli"))
    torch.manual_seed(0)
    train, val = G._dataset(t, "z", 12, 0, False), G._dataset(t, "v", G.N_VAL, 1, False)
    dec_cfg = dict(num_layers=2, image_channel=3, min_channel=8, max_channel=16, latent_channel=4,
                   hidden_activation_type="silu", use_final_dec_activation=True, decoder_activation_type="tanh")
    save_model(f"{t}/dec", "model.pt", dict(dec_cfg, model=G._decoder().state_dict()))
    for name, patch, k in (("lr", 8, 8), ("hr", 2, 16)):
        save_model(f"{t}/cb_{name}", "codebook.pt",
                   dict(patch_dim=(patch, patch), image_dim=(8, 8), image_C=4, num_embeddings=k,
                        neighbourhood_range=1, global_steps=0, checkpoint=G._codebook(patch, k).state_dict()))
    dec = f"{t}/dec/models_checkpoint/model.pt"
    cbs = [f"{t}/cb_lr/models_checkpoint/codebook.pt", f"{t}/cb_hr/models_checkpoint/codebook.pt"]
    score = ["--device", "cuda", "--dataset-path", val, "--decoder-path", dec, "--codebook-path", cbs[0],
             "--codebook-path", cbs[1]]
    out = {}
    for tag, extra in (("topo4", ["--batch-size", 4, "--topology"]), ("topo1", ["--batch-size", 1, "--topology"]),
                       ("plain", ["--batch-size", 4])):
        r = G._run("evaluate_reconstruction.py", *score, *extra, "--out-json", f"{t}/{tag}.json", cwd=t)
        out[tag] = r.stdout + r.stderr
    json.dump(dict(model_lr=1e-2, neighbourhood_step=2, image_H=8, image_W=8, image_C=4, patch_H=2, patch_W=2,
                   num_embeddings=16), open(f"{t}/cb.json", "w"))
    common = ["--device", "cuda", "--dataset-path", train, "--decoder-path", dec, "--batch-size", 4,
              "--checkpoint-step", 2, "--max-epoch", 1, "--max-steps", 2, "--config-path", f"{t}/cb.json"]
    r = G._run("train_codebook.py", *common, "--out-dir", f"{t}/val", "--val-dataset-path", val, "--val-step", 1,
               "--val-topology", cwd=t)
    out["val"] = r.stdout + r.stderr
    return dict(t=t, out=out, common=common, cbs=cbs, val=val)


def test_evaluate_cli_writes_the_topology_block(runs):
    from qarig import cli_common as cc
    from qarig.topology import TopologyScorer, topology_summary_line
    t = runs["t"]
    full = json.load(open(f"{t}/topo4.json"))
    assert list(full["codebooks"]) == ["codebook", "codebook_2"]
    # the same numbers from a TopologyScorer run here on the same checkpoints and latents
    device = torch.device("cuda", 0)
    cbs = {name: cc.load_codebook(path, device, name)[0] for name, path in zip(full["codebooks"], runs["cbs"])}
    scorer = TopologyScorer(cbs)
    z = torch.from_numpy(G._latents(G.N_VAL, 1)).cuda()
    for i in range(0, G.N_VAL, 3):
        scorer.add_batch(z[i:i + 3])
    here = scorer.result()
    for name, k, rows in (("codebook", 8, G.N_VAL), ("codebook_2", 16, G.N_VAL * 16)):
        b = full["codebooks"][name]
        assert set(b) == {"latent", "vs_decoder", "usage", "topology"}
        tb = b["topology"]
        assert set(tb) == TOPOLOGY_KEYS and set(tb["lag"]) == LAG_KEYS
        assert tb == json.loads(json.dumps(here[name]))
        assert tb["rows"] == rows == sum(tb["ratio_hist"]) and len(tb["per_image_quantisation_error"]) == G.N_VAL
        assert list(tb["within"]) == [str(r) for r in (1, 2, 4, 8) if r < k] == list(tb["within_uniform"])
        assert 0.0 <= tb["topographic_error"] <= 1.0 and 0.0 < tb["quantisation_error"] <= tb["second_error"]
        assert len(tb["lag"]["mean_distance"]) == k - 1 and tb["lag"]["all_pairs_mean"] > 0
        assert "Topology " + name + " TE: {:.4f} | within 2/4/8: ".format(tb["topographic_error"]) in runs["out"]["topo4"]
        assert topology_summary_line(name, here[name]) in runs["out"]["topo4"]
    assert runs["out"]["topo4"].count("Topology ") == 2
    # batch size 1 against 4: the same result, bit for bit
    assert json.load(open(f"{t}/topo1.json")) == full


def test_without_the_flag_the_output_is_what_it_was(runs):
    t = runs["t"]
    plain, full = json.load(open(f"{t}/plain.json")), json.load(open(f"{t}/topo4.json"))
    assert set(plain) == {"images", "codebooks"} and list(plain["codebooks"]) == ["codebook", "codebook_2"]
    for name, b in plain["codebooks"].items():
        assert set(b) == {"latent", "vs_decoder", "usage"}                     # the keys test_gpu_recon_eval asserts
        assert set(b["latent"]) == G.ERROR_KEYS and set(b["vs_decoder"]) == G.IMAGE_KEYS
        assert set(b["usage"]) == G.USAGE_KEYS
        assert b == {k: v for k, v in full["codebooks"][name].items() if k != "topology"}
    lines = _messages(runs["out"]["plain"])
    assert lines == [ln for ln in _messages(runs["out"]["topo4"]) if not ln.startswith("Topology ")]
    assert len(lines) == 2 and all(ln.startswith("Eval codebook") and " | images: 6" in ln for ln in lines)
    assert "opology" not in runs["out"]["plain"]


def test_codebook_training_logs_the_topology_of_the_validation_pass(runs):
    t = runs["t"]
    lines = G._lines(f"{t}/val/val_log.jsonl")
    assert [ln["step"] for ln in lines] == [0, 1]
    for ln in lines:
        assert set(ln) == {"step", "codebook"} and set(ln["codebook"]) == {"latent", "vs_decoder", "usage", "topology"}
        tb = ln["codebook"]["topology"]
        assert set(tb) == TOPOLOGY_KEYS - {"per_image_quantisation_error"} and tb["rows"] == G.N_VAL * 16
        assert set(ln["codebook"]["latent"]) == G.ERROR_KEYS - {"per_image_mse"}
    log = runs["out"]["val"]
    last = lines[-1]["codebook"]
    assert log.count(" | TE: ") == 2
    assert "| perplexity: {:.2f} | TE: {:.4f}".format(last["usage"]["perplexity"],
                                                     last["topology"]["topographic_error"]) in log


def test_val_topology_needs_the_held_out_set(runs):
    r = G._run("train_codebook.py", *runs["common"], "--out-dir", f"{runs['t']}/refused", "--val-topology",
               cwd=runs["t"], ok=False)
    assert r.returncode == 2 and "--val-topology needs --val-dataset-path" in r.stderr
    import os
    assert not os.path.exists(f"{runs['t']}/refused")
