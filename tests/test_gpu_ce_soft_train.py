"""SOM-neighbour soft targets through the layers above the kernel, on the GPU at the tiny shapes of
tests/test_gpu_ce_reg_train.py (32 wide, 2 layers, 17 tokens in windows of 12, batch 6; 32 HR codes + <end>): the
autograd node of QF.cross_entropy, pipeline.train_step (defaults unchanged to the bit and to the call, the
{objective, nll} pair against fp64 on the logits of the same forward), pipeline.GraphedTrainStep (replay equals eager,
bit for bit, the pair included) and train_quantized_transformer.py --neighbour-smoothing / --neighbour-range /
--neighbour-sigma (log lines, checkpoint keys, refusals).  The kernel itself is tests/test_gpu_ce_soft.py's subject."""
import os

import pytest
import torch

import ce_reg_cases as G
import ce_soft_cases as S
import test_gpu_ce_reg_train as T
from test_gpu_ce_reg_train import runs  # noqa: F401  (the module-scoped fixture: data, codebooks, a flagless run)

pytestmark = pytest.mark.gpu

EPS, ZETA, NU, RANGE, SIGMA, CODES = 0.1, 1e-4, 0.3, 2, 1.0, 32
SOFT = dict(label_smoothing=EPS, z_loss=ZETA, neighbour_smoothing=NU, neighbour_range=RANGE, codes=CODES)
GI = S.SOFT_GRID.index((EPS, ZETA, NU))


def _mean_tol(k):
    return S.soft_tol((k, GI))


def test_autograd_node():
    """QF.cross_entropy with soft targets: objective and nll are the ops outputs, the gradient of 0.5 loss is
    ops.scale_by(dlogits, 0.5), bit for bit; it is the regularised node, not a third one; with
    neighbour_smoothing = 0 the two earlier branches."""
    from qarig import functional as QF
    from qarig import ops
    g = torch.Generator().manual_seed(11)
    x = (2.0 * torch.randn((6, 12, 33), generator=g)).cuda()
    t = torch.randint(0, 33, (6, 12), generator=g).cuda()
    assert int((t == 32).sum()) > 0          # <end> targets among them
    pair, dl = ops.cross_entropy_fwd(x.view(-1, 33), t.flatten(), EPS, ZETA, NU, RANGE, None, CODES)
    assert pair.shape == (2,) and dl.shape == (72, 33)
    pair0, none = ops.cross_entropy_fwd(x.view(-1, 33), t.flatten(), EPS, ZETA, NU, RANGE, SIGMA, CODES, want_grad=False)
    assert none is None and torch.equal(pair0, pair)            # sigma defaults to range / 2
    logits = x.clone().requires_grad_(True)
    loss = QF.cross_entropy(logits, t, EPS, ZETA, neighbour_smoothing=NU, neighbour_range=RANGE, codes=CODES)
    assert loss.dim() == 0 and loss.requires_grad
    assert torch.equal(loss.detach(), pair[0]) and torch.equal(loss.nll, pair[1]) and torch.equal(loss.pair, pair)
    assert not loss.nll.requires_grad and not loss.pair.requires_grad
    assert torch.equal(QF.loss_pair(loss), pair)
    (0.5 * loss).backward()
    want = ops.scale_by(dl, torch.tensor([0.5], device="cuda")).view(6, 12, 33)
    assert torch.equal(logits.grad, want)
    # against fp64 within the means' tolerance, on the logits' own rows
    ref = S.soft_ref_uncached(x.view(-1, 33).cpu(), t.flatten().cpu(), CODES, RANGE, S.soft_table(RANGE, SIGMA), EPS,
                              ZETA, NU)
    for k, got, rows in (("mean_obj", pair[0], ref["obj"]), ("mean_nll", pair[1], ref["nll"])):
        err = float((got.cpu().double() - ref[k]).abs() / (G.U * rows.abs().mean()))
        print(f"MEASURED ce_soft_node {k} {err:.3f} {_mean_tol(k)}")
        assert err <= _mean_tol(k)
    # the plain nll is the regularised entry's, and the objective is not
    reg = QF.cross_entropy(x.clone().requires_grad_(True), t, EPS, ZETA)
    assert torch.equal(reg.nll, loss.nll) and not torch.equal(reg.detach(), loss.detach())
    assert type(reg.grad_fn).__name__ == type(loss.grad_fn).__name__
    # neighbour_smoothing = 0: the two earlier branches, bit for bit
    off = QF.cross_entropy(x.clone().requires_grad_(True), t, EPS, ZETA, neighbour_smoothing=0.0)
    assert torch.equal(off.pair, reg.pair) and type(off.grad_fn).__name__ == type(reg.grad_fn).__name__
    plain = QF.cross_entropy(x.clone().requires_grad_(True), t)
    same = QF.cross_entropy(x.clone().requires_grad_(True), t, neighbour_smoothing=0.0, neighbour_range=None)
    assert torch.equal(plain, same) and not hasattr(same, "pair")
    assert type(plain.grad_fn).__name__ == type(same.grad_fn).__name__ != type(loss.grad_fn).__name__
    with pytest.raises(TypeError):           # keyword-only
        QF.cross_entropy(logits, t, EPS, ZETA, NU, RANGE)
    for bad in (dict(neighbour_smoothing=1.0), dict(neighbour_smoothing=0.95, neighbour_range=2, codes=32),
                dict(neighbour_smoothing=0.2, codes=32), dict(neighbour_range=2), dict(neighbour_sigma=1.0),
                dict(neighbour_smoothing=0.2, neighbour_range=32, codes=32),
                dict(neighbour_smoothing=0.2, neighbour_range=2, neighbour_sigma=0.0, codes=32),
                dict(neighbour_smoothing=0.2, neighbour_range=2),
                dict(neighbour_smoothing=0.2, neighbour_range=2, codes=34)):
        with pytest.raises(ValueError):
            QF.cross_entropy(logits, t, EPS, ZETA, **bad)


def _eager_counted(n, monkeypatch, **kw):
    """T._eager with the C-ABI calls of each step counted and the cross-entropy entry watched: a hit is a call that
    passes neighbour_smoothing > 0 (argument 8 of qarig_cross_entropy_fused_fwd)."""
    from qarig import _lib, pipeline
    lib = _lib.load()
    hits, counts = [], []
    real_entry, real_step = lib.qarig_cross_entropy_fused_fwd, pipeline.train_step

    def entry(*a):
        if a[8] > 0:
            hits.append(1)
        return real_entry(*a)

    def step(*a, **k):
        before = _lib.N_CALLS
        out = real_step(*a, **k)
        counts.append(_lib.N_CALLS - before)
        return out

    monkeypatch.setattr(lib, "qarig_cross_entropy_fused_fwd", entry)
    monkeypatch.setattr(pipeline, "train_step", step)
    try:
        res = T._eager(n, **kw)
    finally:
        monkeypatch.setattr(pipeline, "train_step", real_step)
        monkeypatch.setattr(lib, "qarig_cross_entropy_fused_fwd", real_entry)
    return res, counts, len(hits)


def test_train_step_defaults_unchanged_and_pair_against_fp64(monkeypatch):
    from qarig import functional as QF
    (default, losses_d, pairs_d), calls_d, hits_d = _eager_counted(3, monkeypatch)
    (zero, losses_z, pairs_z), calls_z, hits_z = _eager_counted(
        3, monkeypatch, label_smoothing=0.0, z_loss=0.0, neighbour_smoothing=0.0, neighbour_range=None,
        neighbour_sigma=None, codes=None)
    assert torch.equal(default, zero) and losses_d == losses_z
    assert pairs_d == [[v, v] for v in losses_d] == pairs_z
    assert calls_d == calls_z and len(calls_d) == 3 and min(calls_d) > 0
    assert hits_d == hits_z == 0             # neither path asks for soft targets
    # the regularisers alone do not either, and make the calls they made
    (reg, _, pairs_reg), calls_reg, hits_reg = _eager_counted(3, monkeypatch, label_smoothing=EPS, z_loss=ZETA)
    assert hits_reg == 0
    seen = []
    real = QF.cross_entropy

    def spy(logits, target, *a, **k):
        seen.append((logits.detach().clone(), target.detach().clone()))
        return real(logits, target, *a, **k)

    monkeypatch.setattr(QF, "cross_entropy", spy)
    (soft, losses_s, pairs_s), calls_s, hits_s = _eager_counted(3, monkeypatch, **SOFT)
    monkeypatch.setattr(QF, "cross_entropy", real)
    assert hits_s == 3 and calls_s == calls_reg          # one launch pair for another: no extra call in the step
    assert not torch.equal(soft, default) and not torch.equal(soft, reg)
    assert len(seen) == 3 and [p[0] for p in pairs_s] == losses_s
    assert pairs_s[0][1] == pairs_reg[0][1] and pairs_s[0][0] != pairs_reg[0][0]     # step 1: same logits, same nll
    w = S.soft_table(RANGE, RANGE / 2.0)
    for (logits, target), (obj, nll) in zip(seen, pairs_s):
        assert logits.shape == (72, 33)
        ref = S.soft_ref_uncached(logits.cpu(), target.cpu(), CODES, RANGE, w, EPS, ZETA, NU)
        for k, got, rows in (("mean_obj", obj, ref["obj"]), ("mean_nll", nll, ref["nll"])):
            err = float(abs(got - float(ref[k])) / (G.U * float(rows.abs().mean())))
            print(f"MEASURED ce_soft_train_step {k} {err:.3f} {_mean_tol(k)}")
            assert err <= _mean_tol(k), (k, got, float(ref[k]))
        assert obj != nll


def test_graph_replay_matches_eager_steps():
    """Five GraphedTrainStep steps with soft targets, warm-up 2 then replay: the weights and the per-step
    {objective, nll} pairs of five eager steps, bit for bit; the weight table exists before the capture."""
    from qarig import ops, pipeline
    want, losses_e, pairs_e = T._eager(5, **SOFT)
    lr_cb, hr_cb, m, opt = T._build()
    step = pipeline.GraphedTrainStep(m, opt, lr_cb, hr_cb, True, 12, warmup=2, **SOFT)
    table = ops.neighbour_weights(RANGE, RANGE / 2.0, opt.flat_param.device)
    assert step._neighbour_weights is table and torch.equal(table.cpu(), S.soft_table(RANGE, RANGE / 2.0))
    losses_g, pairs_g, ptrs = [], [], []
    for z, rand in T._batches(5):
        loss = step(z.cuda(), rand)
        pair = pipeline.loss_pair(loss)
        losses_g.append(float(loss))
        pairs_g.append(pair.tolist())
        ptrs.append((loss.data_ptr(), pair.data_ptr()))
    assert step.graph is not None and opt.step_count == 5
    assert ops.neighbour_weights(RANGE, RANGE / 2.0, opt.flat_param.device) is table      # made once
    assert torch.equal(opt.flat_param, want)
    assert losses_g == losses_e and pairs_g == pairs_e
    assert ptrs[2] == ptrs[3] == ptrs[4] and ptrs[2][0] == ptrs[2][1]
    for bad in (dict(neighbour_smoothing=0.2), dict(neighbour_range=2), dict(neighbour_smoothing=0.2, neighbour_range=2),
                dict(label_smoothing=0.9, neighbour_smoothing=0.2, neighbour_range=2, codes=32)):
        with pytest.raises(ValueError):
            pipeline.GraphedTrainStep(m, opt, lr_cb, hr_cb, True, 12, **bad)


# ---- the command line ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def soft_run(runs):  # noqa: F811
    t = runs["t"]
    out = T._run("train_quantized_transformer.py", *runs["common"], "--out-dir", f"{t}/soft", "--label-smoothing", EPS,
                 "--neighbour-smoothing", NU, "--neighbour-range", RANGE, cwd=t)
    return out.stdout + out.stderr


def test_cli_with_the_flags(runs, soft_run):  # noqa: F811
    t = runs["t"]
    md = torch.load(f"{t}/soft/models_checkpoint/model_2.pt", map_location="cpu", weights_only=True)
    assert set(md) == T.BASE_KEYS | {"label_smoothing", "neighbour_smoothing", "neighbour_range", "neighbour_sigma"}
    assert md["neighbour_smoothing"] == NU and md["neighbour_range"] == RANGE and md["neighbour_sigma"] == RANGE / 2.0
    assert type(md["neighbour_smoothing"]) is float and type(md["neighbour_range"]) is int
    assert type(md["neighbour_sigma"]) is float
    steps = [ln for ln in soft_run.splitlines() if "Cum. Steps:" in ln]
    assert len(steps) == 3 and all("| Recon Loss: " in ln and "| NLL: " in ln for ln in steps)
    for ln in steps:       # two numbers, both finite, not the same one twice
        obj, nll = float(ln.split("Recon Loss: ")[1].split(" |")[0]), float(ln.split("NLL: ")[1])
        assert 0 < nll < 100 and 0 < obj < 100 and obj != nll
    block = soft_run[soft_run.index("Training Parameters."):soft_run.index("Sampling Parameters.")]
    i = next(k for k, ln in enumerate(block.splitlines()) if "Label Smoothing: " in ln)
    tail = "\n".join(block.splitlines()[i:i + 5])          # the startup lines follow `Label Smoothing:`
    assert f"Label Smoothing: {EPS}" in tail and f"Neighbour Smoothing: {NU}" in tail
    assert f"Neighbour Range: {RANGE}" in tail and f"Neighbour Sigma: {RANGE / 2.0}" in tail


def test_cli_neighbour_smoothing_alone(runs):  # noqa: F811
    """Without --label-smoothing / --z-loss: the three keys only, and still the two-number step line."""
    t = runs["t"]
    out = T._run("train_quantized_transformer.py", *runs["common"], "--out-dir", f"{t}/soft_alone",
                 "--neighbour-smoothing", NU, "--neighbour-range", 31, "--neighbour-sigma", 3.5, "--graph-step", cwd=t)
    md = torch.load(f"{t}/soft_alone/models_checkpoint/model_2.pt", map_location="cpu", weights_only=True)
    assert set(md) == T.BASE_KEYS | {"neighbour_smoothing", "neighbour_range", "neighbour_sigma"}
    assert (md["neighbour_smoothing"], md["neighbour_range"], md["neighbour_sigma"]) == (NU, 31, 3.5)
    steps = [ln for ln in (out.stdout + out.stderr).splitlines() if "Cum. Steps:" in ln]
    assert len(steps) == 3 and all("| Recon Loss: " in ln and "| NLL: " in ln for ln in steps)


def test_cli_without_the_flags_nothing_is_added(runs):  # noqa: F811
    t = runs["t"]
    md = torch.load(f"{t}/off/models_checkpoint/model_2.pt", map_location="cpu", weights_only=True)
    assert set(md) == T.BASE_KEYS
    out = runs["out_off"]
    assert "NLL" not in out and "Neighbour" not in out and "Label Smoothing" not in out
    assert len([ln for ln in out.splitlines() if "Cum. Steps:" in ln]) == 3
    md = torch.load(f"{t}/reg/models_checkpoint/model_2.pt", map_location="cpu", weights_only=True)
    assert set(md) == T.BASE_KEYS | {"label_smoothing", "z_loss"} and "Neighbour" not in runs["out_reg"]


REFUSALS = [
    ("nu-one", ["--neighbour-smoothing", "1.0", "--neighbour-range", "2"], "--neighbour-smoothing"),
    ("nu-negative", ["--neighbour-smoothing", "-0.1", "--neighbour-range", "2"], "--neighbour-smoothing"),
    ("nu-nan", ["--neighbour-smoothing", "nan", "--neighbour-range", "2"], "--neighbour-smoothing"),
    ("sum-one", ["--label-smoothing", "0.5", "--neighbour-smoothing", "0.5", "--neighbour-range", "2"],
     "--neighbour-smoothing"),
    ("no-range", ["--neighbour-smoothing", "0.2"], "--neighbour-range"),
    ("range-alone", ["--neighbour-range", "2"], "--neighbour-range"),
    ("sigma-alone", ["--neighbour-sigma", "1.0"], "--neighbour-sigma"),
    ("range-zero", ["--neighbour-smoothing", "0.2", "--neighbour-range", "0"], "--neighbour-range"),
    ("range-32", ["--neighbour-smoothing", "0.2", "--neighbour-range", "32"], "--neighbour-range"),
    ("sigma-zero", ["--neighbour-smoothing", "0.2", "--neighbour-range", "2", "--neighbour-sigma", "0"],
     "--neighbour-sigma"),
    ("sigma-negative", ["--neighbour-smoothing", "0.2", "--neighbour-range", "2", "--neighbour-sigma", "-1"],
     "--neighbour-sigma"),
    ("sigma-inf", ["--neighbour-smoothing", "0.2", "--neighbour-range", "2", "--neighbour-sigma", "inf"],
     "--neighbour-sigma"),
    ("sigma-nan", ["--neighbour-smoothing", "0.2", "--neighbour-range", "2", "--neighbour-sigma", "nan"],
     "--neighbour-sigma"),
]


@pytest.mark.parametrize("flags,named", [r[1:] for r in REFUSALS], ids=[r[0] for r in REFUSALS])
def test_cli_refusals(runs, flags, named):  # noqa: F811
    r = T._run("train_quantized_transformer.py", *runs["common"], "--out-dir", f"{runs['t']}/refused_soft", *flags,
               cwd=runs["t"], ok=False)
    assert r.returncode == 2 and named in r.stderr and "usage:" in r.stderr, r.stderr[-2000:]
    assert not os.path.exists(f"{runs['t']}/refused_soft")
