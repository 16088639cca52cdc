"""Dropout through the layers above the kernel, on the GPU at the smallest models that have every site (width 128,
2 heads, 1 encoder + 2 decoder layers, 2 x 16 tokens; with and without the encoder and the position conditioning):
the model's sites against a torch-ops implementation whose mask is the NumPy reference's, the paths that must
never launch it, the default step's C-ABI call count, activation checkpointing, graph replay (plain and
segmented) against eager steps, resuming from the optimizer's step count, and the command line."""
import json
import multiprocessing as mp
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import dropout_cases as C
from conftest import PKG

pytestmark = pytest.mark.gpu

P, SEED = 0.1, 0x5EED0123456789
V_ENC, V_DEC, V_OUT, S, N = 16, 40, 33, 16, 2
CONFIGS = [(True, True), (False, True), (True, False), (False, False)]       # (use_encoder, use_pos_cond)


def _model(use_encoder=True, use_pos_cond=True, ckpt=False):
    from models.Transformer import Transformer
    torch.manual_seed(5)
    m = Transformer(use_encoder=use_encoder, use_pos_cond=use_pos_cond, num_enc_layers=1 if use_encoder else None,
                    num_dec_layers=2, num_enc_embedding=V_ENC if use_encoder else None, num_dec_embedding=V_DEC,
                    self_attn_heads=2, cross_attn_heads=2 if use_encoder else None, transformer_in_dim=128,
                    transformer_out_dim=V_OUT, transformer_hidden_dim=256, use_activation_checkpoint=ckpt).cuda()
    g = torch.Generator().manual_seed(6)
    with torch.no_grad():
        for p in m.parameters():
            if p.abs().max() == 0:
                p.copy_(torch.randn(p.shape, generator=g) * 0.05)
    return m


def _n_sites(use_encoder):
    return (2 if use_encoder else 1) + (2 if use_encoder else 0) + (3 if use_encoder else 2) * 2


def _data(k=0, use_encoder=True, use_pos_cond=True):
    g = torch.Generator().manual_seed(20 + k)
    x_dec = torch.randint(0, V_DEC, (N, S), generator=g).cuda()
    x_enc = torch.randint(0, V_ENC, (N, S), generator=g).cuda() if use_encoder else None
    tgt = torch.randint(0, V_OUT, (N, S), generator=g).cuda()
    pos = (torch.randint(0, 5, (N, 1), generator=g) + torch.arange(S)[None]).cuda() if use_pos_cond else None
    return x_dec, x_enc, tgt, pos


def _fwd_bwd(m, data, step=None):
    """(logits, {name: gradient}) of one forward + cross-entropy + backward; step: the key's step word first."""
    from qarig import functional as QF
    x_dec, x_enc, tgt, pos = data
    for p in m.parameters():
        p.grad = None
    if step is not None:
        m.dropout_key.set_step(step)
    logits = m(x_dec=x_dec, x_enc=x_enc, pos_cond=pos, pos_bound=S + 5 if pos is not None else None)
    QF.cross_entropy(logits.view(-1, V_OUT), tgt.flatten()).backward()
    return logits.detach().clone(), {k: p.grad.detach().clone() for k, p in m.named_parameters()}


def _torch_dropout(calls):
    """QF.dropout restated with torch ops, the mask from the NumPy reference and the key's host-side fields."""
    def dropout(x, p, site, key):
        t, s = C.threshold_and_scale(p)
        keep = C.mask(x.numel(), t, key.seed, site, key.step, key.rank)
        calls.append((site, tuple(x.shape), x.dtype, x.is_contiguous()))
        keep = torch.from_numpy(keep).to(x.device).view(x.shape)
        return torch.where(keep, x * float(s), torch.zeros((), dtype=x.dtype, device=x.device))
    return dropout


# ---- 1: the sites, against torch ops with the reference's mask ----------------------------------------------
@pytest.mark.parametrize("use_encoder,use_pos_cond", CONFIGS)
def test_model_sites_against_reference_mask(monkeypatch, use_encoder, use_pos_cond):
    from qarig import functional as QF
    m = _model(use_encoder, use_pos_cond)
    key = m.enable_dropout(P, SEED, rank=3)
    assert key is m.dropout_key and (key.seed, key.rank) == (SEED, 3)
    data = _data(0, use_encoder, use_pos_cond)
    m.train()
    logits_k, grads_k = _fwd_bwd(m, data, step=4)
    calls = []
    monkeypatch.setattr(QF, "dropout", _torch_dropout(calls))
    logits_t, grads_t = _fwd_bwd(m, data, step=4)
    monkeypatch.undo()
    # every site once, each under its own ordinal, all fp32 and contiguous
    residual_sites = _n_sites(use_encoder) - (2 if use_encoder else 1)
    want_sites = ([0] if use_encoder else []) + [1] + list(range(2, 2 + residual_sites))
    assert sorted(c[0] for c in calls) == want_sites, calls
    assert all(c[2] == torch.float32 and c[3] for c in calls)
    assert torch.equal(logits_k, logits_t)
    assert set(grads_k) == set(grads_t) and len(grads_k) > 10
    for k in grads_k:
        assert torch.equal(grads_k[k], grads_t[k]), k
    # and it is dropout: not the forward of the same model without it, and another step draws another mask
    m.disable_dropout()
    assert m.dropout_key is None
    logits_0, _ = _fwd_bwd(m, data)
    assert not torch.equal(logits_0, logits_k)
    m.enable_dropout(P, SEED, rank=3)
    logits_5, _ = _fwd_bwd(m, data, step=5)
    assert not torch.equal(logits_5, logits_k)


def test_enable_dropout_refuses_bad_probabilities():
    m = _model(False, False)
    for bad in (1e-6, 0.91, 1.0, float("nan"), -0.1):
        with pytest.raises(ValueError):
            m.enable_dropout(bad, 0)
    assert m.dropout_key is None
    assert m.enable_dropout(0, 0) is None and m.dropout_key is None
    sd = set(m.state_dict())
    m.enable_dropout(0.5, 1)
    assert set(m.state_dict()) == sd            # no buffer, no parameter: the reference's keys


# ---- 2: the paths that never launch it -------------------------------------------------------------------
def test_eval_and_no_grad_are_untouched(monkeypatch):
    from qarig import _lib, ops
    data = _data(1)
    x_dec, x_enc, tgt, pos = data
    plain, dropped = _model(), _model()
    dropped.enable_dropout(P, SEED)
    launches = []
    real = ops.dropout
    monkeypatch.setattr(ops, "dropout", lambda *a, **k: (launches.append(1), real(*a, **k))[1])

    def forward(m):
        before = _lib.N_CALLS
        y = m(x_dec=x_dec, x_enc=x_enc, pos_cond=pos, pos_bound=S + 5)
        return y, _lib.N_CALLS - before

    for mode in ("eval", "train"):
        for m in (plain, dropped):
            m.train(mode == "train")
        with torch.no_grad():
            (want, calls_plain), (got, calls_dropped) = forward(plain), forward(dropped)
        assert torch.equal(want, got) and calls_plain == calls_dropped > 0 and not launches, mode
    plain.eval()
    dropped.eval()
    (want, calls_plain), (got, calls_dropped) = forward(plain), forward(dropped)      # eval with gradients on
    assert torch.equal(want, got) and calls_plain == calls_dropped and not launches
    plain.train()
    dropped.train()
    dropped.dropout_key.set_step(1)
    (want, calls_plain), (got, calls_train) = forward(plain), forward(dropped)         # the control: train + grad
    assert len(launches) == _n_sites(True) and calls_train == calls_plain + _n_sites(True)
    assert not torch.equal(want, got)


# ---- 3: the default step makes the calls it made before -----------------------------------------------------
def _one_train_step(prepare):
    from qarig import _lib, pipeline
    from qarig.optim import FlatAdam
    m = _model()
    opt = FlatAdam(m.parameters(), lr=1e-3, betas=(0.5, 0.999))
    prepare(m)
    m.train()
    x_dec, x_enc, tgt, pos = _data(2)
    before = _lib.N_CALLS
    loss = pipeline.train_step(m, opt, x_dec, x_enc, tgt, pos, dp=False, pos_bound=S + 5)
    return _lib.N_CALLS - before, float(loss.detach()), opt.flat_param.detach().clone()


def test_train_step_with_p_zero_is_the_default_step():
    never = _one_train_step(lambda m: None)
    zero = _one_train_step(lambda m: m.enable_dropout(0.0, SEED))
    off_again = _one_train_step(lambda m: (m.enable_dropout(P, SEED), m.disable_dropout()))
    on = _one_train_step(lambda m: m.enable_dropout(P, SEED))
    for other in (zero, off_again):
        assert other[0] == never[0] and other[1] == never[1] and torch.equal(other[2], never[2])
    assert on[0] == never[0] + 2 * _n_sites(True)       # one launch per site forward, one backward; nothing else
    assert on[1] != never[1]


# ---- 4: activation checkpointing ---------------------------------------------------------------------------
def test_activation_checkpoint_regenerates_the_mask():
    """Gradients with use_activation_checkpoint against without, at p = 0.1: every parameter whose gradient is
    bit-identical between the two at p = 0 on this build (measured first) must be bit-identical at p = 0.1."""
    data = _data(3)
    same_at = {}
    for p in (0.0, P):
        out = []
        for ckpt in (False, True):
            m = _model(ckpt=ckpt)
            m.train()
            if p:
                m.enable_dropout(p, SEED)
            out.append(_fwd_bwd(m, data, step=2 if p else None))
        (l0, g0), (l1, g1) = out
        same_at[p] = {k for k in g0 if torch.equal(g0[k], g1[k])}
        print(f"MEASURED checkpoint vs plain at p={p}: {len(same_at[p])} of {len(g0)} gradients bit-identical, "
              f"logits identical: {torch.equal(l0, l1)}")
        assert torch.equal(l0, l1)
    assert len(same_at[0.0]) > 0
    assert same_at[0.0] <= same_at[P], sorted(same_at[0.0] - same_at[P])


# ---- 5: graph replay against eager steps ---------------------------------------------------------------------
def _build_pipeline():
    """Codebooks + the encoder-decoder model + FlatAdam: 4 LR tokens for the encoder, <start> + 16 HR tokens in
    windows of 16 for the decoder."""
    from models.Codebook import Codebook
    from qarig.optim import FlatAdam
    g = torch.Generator().manual_seed(4)
    lr_cb = Codebook(patch_dim=(4, 4), image_dim=(8, 8), image_channel=4, num_embeddings=V_ENC).cuda()
    hr_cb = Codebook(patch_dim=(2, 2), image_dim=(8, 8), image_channel=4, num_embeddings=V_OUT - 1).cuda()
    with torch.no_grad():
        lr_cb.codebook.weight.copy_(torch.tanh(torch.randn(lr_cb.codebook.weight.shape, generator=g)))
        hr_cb.codebook.weight.copy_(torch.tanh(torch.randn(hr_cb.codebook.weight.shape, generator=g)))
    m = _model()
    m.train()
    return lr_cb, hr_cb, m, FlatAdam(m.parameters(), lr=1e-3, betas=(0.5, 0.999))


def _batches(n=5):
    g = torch.Generator().manual_seed(9)
    return [(torch.tanh(torch.randn((N, 4, 8, 8), generator=g)), torch.randint(0, 17 - S + 1, (N,), generator=g))
            for _ in range(n)]


def _eager_steps(n=5, p=P, spy=None):
    from qarig import pipeline
    lr_cb, hr_cb, m, opt = _build_pipeline()
    if p:
        m.enable_dropout(p, SEED)
    losses = []
    for z, rand in _batches(n):
        hr_in, lr_in, hr_tg = pipeline.tokenize(z.cuda(), lr_cb, hr_cb, False)
        hr_in, hr_tg, pos = pipeline.slide(hr_in, hr_tg, S, rand)
        losses.append(float(pipeline.train_step(m, opt, hr_in, lr_in, hr_tg, pos, dp=False, pos_bound=17).detach()))
        if spy is not None:
            spy(opt.step_count)
    return opt.flat_param.detach().clone(), losses


@pytest.fixture(scope="module")
def eager_reference():
    flat, losses = _eager_steps()
    return flat.cpu(), losses


def test_eager_steps_draw_a_new_mask_each_step(monkeypatch):
    """One site's output read back on consecutive steps: the zeros are where the reference's mask of THAT step
    puts them (the step word follows the optimizer's count), so two steps differ."""
    from qarig import functional as QF
    real = QF.dropout
    seen, per_step = [], {}

    def wrapped(x, p, site, key):
        y = real(x, p, site, key)
        if site == 1:
            seen.append((key.step, y.detach().clone()))
        return y

    monkeypatch.setattr(QF, "dropout", wrapped)
    _eager_steps(3, spy=lambda count: per_step.setdefault(count, seen[-1]))
    t, _ = C.threshold_and_scale(P)
    zeros = []
    for count in (1, 2, 3):
        step, y = per_step[count]
        assert step == count
        keep = C.mask(y.numel(), t, SEED, 1, count, 0).reshape(y.shape)
        got = (y != 0).cpu().numpy()
        assert np.array_equal(got, keep)      # (an embedding + position output has no exact zeros of its own)
        zeros.append(got)
    assert not np.array_equal(zeros[0], zeros[1]) and not np.array_equal(zeros[1], zeros[2])


def test_graph_replay_matches_eager_steps(eager_reference):
    """Warm-up 2, capture, replay: losses and final parameters of five eager steps, bit for bit -- the replayed
    launches read the step word the host wrote before each replay (a replay that repeated the captured mask
    would leave other weights)."""
    from qarig import pipeline
    want, losses_e = eager_reference
    lr_cb, hr_cb, m, opt = _build_pipeline()
    key = m.enable_dropout(P, SEED)
    step = pipeline.GraphedTrainStep(m, opt, lr_cb, hr_cb, False, S, warmup=2)
    losses_g = [float(step(z.cuda(), rand)) for z, rand in _batches()]
    assert step.graph is not None and not step.segmented and opt.step_count == 5
    assert key.buffer.tolist()[2] == 5
    assert losses_g == losses_e
    assert torch.equal(opt.flat_param.cpu(), want)
    no_dropout, losses_0 = _eager_steps(5, p=0.0)
    assert not torch.equal(no_dropout.cpu(), want) and losses_0 != losses_e
    m.disable_dropout()
    with pytest.raises(RuntimeError):
        step(*[(z.cuda(), rand) for z, rand in _batches(1)][0])


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _segmented_worker(port, q):
    from conftest import PKG as pkg, ROOT as root
    for p in (root, pkg):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    import torch.distributed as dist
    from qarig import optim as qoptim
    from qarig import parallel, pipeline
    parallel.init(backend="gloo", force=True)
    torch.cuda.set_device(0)
    qoptim.BUCKET_ELEMS = 100_000                    # several buckets -> several graph segments
    lr_cb, hr_cb, m, opt = _build_pipeline()
    opt.enable_allreduce_overlap(force=True)
    m.enable_dropout(P, SEED, rank=parallel.rank())
    step = pipeline.GraphedTrainStep(m, opt, lr_cb, hr_cb, False, S, warmup=2)
    losses = [float(step(z.cuda(), rand)) for z, rand in _batches()]
    q.put((opt.flat_param.detach().cpu().numpy(), losses, step.segmented, len(step.graph.graphs)))
    dist.barrier()
    dist.destroy_process_group()


def test_segmented_graph_replay_matches_eager_steps(eager_reference):
    """The data-parallel form of the captured step (graph segments cut at the gradient buckets), one rank."""
    import queue
    want, losses_e = eager_reference
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    proc = ctx.Process(target=_segmented_worker, args=(_free_port(), q))
    proc.start()
    got = None
    for _ in range(180):
        try:
            got = q.get(timeout=1)
            break
        except queue.Empty:
            if proc.exitcode not in (None, 0):
                break
    proc.join(timeout=30)
    if proc.is_alive():
        proc.kill()
    assert got is not None and proc.exitcode == 0
    flat, losses, segmented, segments = got
    assert segmented and segments > 1
    assert losses == losses_e
    assert torch.equal(torch.from_numpy(flat), want)


# ---- 6: a resumed run continues the mask sequence ----------------------------------------------------------
def test_resume_continues_the_mask_sequence(eager_reference):
    from qarig import pipeline
    from qarig.optim import FlatAdam
    want, losses_e = eager_reference
    lr_cb, hr_cb, m, opt = _build_pipeline()
    m.enable_dropout(P, SEED)
    batches = _batches()
    losses = []

    def run(model, optimizer, some):
        for z, rand in some:
            hr_in, lr_in, hr_tg = pipeline.tokenize(z.cuda(), lr_cb, hr_cb, False)
            hr_in, hr_tg, pos = pipeline.slide(hr_in, hr_tg, S, rand)
            losses.append(float(pipeline.train_step(model, optimizer, hr_in, lr_in, hr_tg, pos, dp=False,
                                                    pos_bound=17).detach()))

    run(m, opt, batches[:3])
    saved = {"model": {k: v.detach().clone() for k, v in m.state_dict().items()}, "optim": opt.state_dict()}
    m2 = _model()
    m2.train()
    m2.load_state_dict(saved["model"])
    opt2 = FlatAdam(m2.parameters(), lr=1e-3, betas=(0.5, 0.999))
    opt2.load_state_dict(saved["optim"])
    assert opt2.step_count == 3
    m2.enable_dropout(P, SEED)
    run(m2, opt2, batches[3:])
    assert m2.dropout_key.step == 5
    assert losses == losses_e
    assert torch.equal(opt2.flat_param.cpu(), want)


# ---- 7: the command line: the fixtures of tests/test_gpu_ce_reg_train.py, copied ------------------------------
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
    t = str(tmp_path_factory.mktemp("dropout_cli"))
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
    out_on = _run("train_quantized_transformer.py", *common, "--out-dir", f"{t}/on", "--dropout", P,
                  "--dropout-seed", "0x5EED", cwd=t)
    out_off = _run("train_quantized_transformer.py", *common, "--out-dir", f"{t}/off", cwd=t)
    return dict(t=t, common=common, out_on=out_on.stdout + out_on.stderr, out_off=out_off.stdout + out_off.stderr)


def _step_lines(out):
    return [ln for ln in out.splitlines() if "Cum. Steps:" in ln]


def test_cli_with_the_flag(runs):
    t = runs["t"]
    md = torch.load(f"{t}/on/models_checkpoint/model_2.pt", map_location="cpu", weights_only=True)
    assert set(md) == BASE_KEYS | {"dropout", "dropout_seed"}
    assert md["dropout"] == P and type(md["dropout"]) is float
    assert md["dropout_seed"] == 0x5EED and type(md["dropout_seed"]) is int
    out = runs["out_on"]
    assert len(_step_lines(out)) == 3
    block = out[out.index("Training Parameters."):out.index("Sampling Parameters.")]
    assert f"Dropout: {P}" in block and f"Dropout Seed: {0x5EED}" in block
    for ln in _step_lines(out):
        assert 0 < float(ln.split("Recon Loss: ")[1].split(" |")[0]) < 100


def test_cli_without_the_flag_nothing_is_added(runs):
    t = runs["t"]
    md = torch.load(f"{t}/off/models_checkpoint/model_2.pt", map_location="cpu", weights_only=True)
    assert set(md) == BASE_KEYS
    assert "Dropout" not in runs["out_off"] and len(_step_lines(runs["out_off"])) == 3


@pytest.mark.parametrize("flag,value", [("--dropout", "0.95"), ("--dropout-seed", "-1")])
def test_cli_refuses_values_out_of_range(runs, flag, value):
    r = _run("train_quantized_transformer.py", *runs["common"], "--out-dir", f"{runs['t']}/refused", flag, value,
             cwd=runs["t"], ok=False)
    assert r.returncode == 2 and flag in r.stderr and "usage:" in r.stderr
    assert not os.path.exists(f"{runs['t']}/refused")
