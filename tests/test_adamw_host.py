"""Host side of AdamW (qarig_adamw_step, FlatAdam.enable_weight_decay, --weight-decay / --lr-schedule): the fp64
definition against torch.optim.AdamW, the fp32 emulation of the kernel against the tolerances the GPU tests assert
(tests/adamw_cases.py derives them), the mutants those tolerances must reject, the group mask, the decay rule and
the learning-rate schedules.  No GPU."""
import math
import types

import numpy as np
import pytest
import torch

import adamw_cases as C

CASES = list(C.cases())


# ---- the definition ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("betas", C.BETAS)
def test_ref64_is_torch_adamw_with_two_groups(betas):
    """Five steps in double on the CPU: the elements of the masked groups as a parameter group with weight decay
    lambda, the others with 0.  Here the scalars are exact doubles (what the host computes before it rounds)."""
    rng = np.random.default_rng(5)
    n, steps, lam = 64 + 5, 5, 0.1
    p0 = rng.standard_normal(n)
    grads = [rng.standard_normal(n) for _ in range(steps)]
    mask = (rng.random((n + 7) // 8) < 0.5).astype(np.uint8)
    mask[-1] = 1                                        # (the partial group is decayed)
    dec = C.element_mask(mask, n)
    assert 0 < dec.sum() < n
    a = torch.nn.Parameter(torch.from_numpy(p0[dec].copy()))
    b = torch.nn.Parameter(torch.from_numpy(p0[~dec].copy()))
    opt = torch.optim.AdamW([dict(params=[a], weight_decay=lam), dict(params=[b], weight_decay=0.0)], lr=C.LR,
                            betas=betas, eps=C.EPS)
    scalars = [dict(step_size=C.LR / (1 - betas[0] ** t), bc2_sqrt=math.sqrt(1 - betas[1] ** t), ema_w=0.0,
                    decay=C.LR * lam) for t in range(1, steps + 1)]
    ref = C.adamw_ref64(p0, grads, mask, scalars, betas[0], betas[1], C.EPS)
    for t, g in enumerate(grads):
        a.grad = torch.from_numpy(g[dec].copy())
        b.grad = torch.from_numpy(g[~dec].copy())
        opt.step()
        want = np.empty(n)
        want[dec], want[~dec] = a.detach().numpy(), b.detach().numpy()
        rel = np.abs(ref[t]["p"] - want).max() / np.abs(want).max()
        assert rel <= 1e-12, (t, rel)
    # and the decay did something: the undecayed run ends elsewhere
    plain = C.adamw_ref64(p0, grads, np.zeros_like(mask), scalars, betas[0], betas[1], C.EPS)
    assert np.abs(plain[-1]["p"] - ref[-1]["p"])[dec].min() > 0
    assert np.array_equal(plain[-1]["p"][~dec], ref[-1]["p"][~dec])


# ---- the emulation against the tolerances --------------------------------------------------------------------
def _ratios(case, mutant=None, with_ema=True):
    x = C.make_inputs(case)
    ema = x["ema"] if with_ema else None
    ref = C.adamw_ref64(x["p"], x["grads"], x["mask"], x["scalars"], x["beta1"], x["beta2"], x["eps"],
                        x["grad_scale"], ema=ema)
    got = C.adamw_emulate32(x["p"], x["grads"], x["mask"], x["scalars"], x["beta1"], x["beta2"], x["eps"],
                            x["grad_scale"], ema=ema, mutant=mutant, lam=case["lam"])
    return C.worst_ratios(ref, got)


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_emulation_meets_the_tolerances(case):
    r = _ratios(case)
    print("emulation {}: worst / bound  p {:.4f}  m {:.4f}  v {:.4f}  ema {:.4f}".format(
        case["id"], r["p"], r["m"], r["v"], r["ema"]))
    assert all(0.0 <= x <= 1.0 for x in r.values()), r
    assert r["p"] > 0 and r["m"] > 0 and r["v"] > 0 and r["ema"] > 0       # (fp32 did round somewhere)


@pytest.mark.parametrize("mutant", C.MUTANTS)
def test_tolerances_reject_the_mutant(mutant):
    """Each wrong AdamW leaves the tolerance on the shared inputs (on p, or on the EMA for the mutant that moves
    only the EMA)."""
    rejected = []
    for case in CASES:
        r = _ratios(case, mutant)
        if max(r.values()) > 1.0:
            rejected.append((case["id"], max(r.values())))
    print(f"{mutant}: rejected on {len(rejected)} of {len(CASES)} cases, worst ratio "
          f"{max((x for _, x in rejected), default=0.0):.3g}")
    assert rejected, mutant
    # on the largest decay (lambda = 1) every mutant is out, at every scale and both beta pairs
    for case in CASES:
        if case["lam"] == 1.0:
            assert case["id"] in dict(rejected), (mutant, case["id"])


# ---- the emulation is the source: csrc/adam_element.h on the host, bit for bit ---------------------------------
@pytest.fixture(scope="module")
def element_exe(tmp_path_factory):
    return C.build_element_program(tmp_path_factory.mktemp("adam_element"))


@pytest.mark.parametrize("with_ema", [True, False], ids=["ema", "plain"])
@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_kernel_element_on_the_host_is_the_emulation(case, with_ema, element_exe):
    """The element function every kernel of csrc/optim.hip calls, compiled for the host and chained over the steps
    for each element (decayed by element_mask, the raw gradient and grad_scale as adam_kernel and the grouped
    kernel without the clip pass them): p, m, v and ema after every step carry adamw_emulate32's bits, and the
    shadow's conversion gives torch's bf16 of p."""
    x = C.make_inputs(case)
    ema = x["ema"] if with_ema else None
    want = C.adamw_emulate32(x["p"], x["grads"], x["mask"], x["scalars"], x["beta1"], x["beta2"], x["eps"],
                             x["grad_scale"], ema=ema)
    got = C.run_element_program(element_exe, x["p"], ema, C.element_mask(x["mask"], x["p"].shape[0]), x["beta1"],
                                x["beta2"], x["eps"],
                                [dict(s, g=g, scale=x["grad_scale"]) for g, s in zip(x["grads"], x["scalars"])])
    assert len(got) == len(want) == C.STEPS
    for t, (a, b) in enumerate(zip(got, want)):
        for k in ("p", "m", "v") + (("ema",) if with_ema else ()):
            assert np.array_equal(a[k], b[k].view(np.uint32)), (t, k)
        # the shadow: p rounded to nearest-even bf16, as torch rounds it
        bf16 = torch.from_numpy(b["p"]).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
        assert np.array_equal(a["shadow"], bf16.astype(np.uint32)), t
    assert not np.array_equal(got[-1]["p"], x["p"].view(np.uint32))


def test_fma_form_against_the_rounded_factor():
    """Why fma(-c, p, p): below 1 fp32 steps by 2^-24 = 6e-8, so at lr lambda = 1e-6 the factor fp32(1 - c) is
    1 - 17 x 2^-24 -- a decay of 1.0133e-6, off by 1.3 % (up to 3 % at other values, more for smaller c) -- while
    the fma form errs by half an ulp of p."""
    c = C.f32(1e-6)
    factor = float(np.float32(1.0) - np.float32(c))
    assert abs((1.0 - factor) - c) / c > 0.01
    p = np.float32(1.2345678)
    fma = float(np.float32(float(p) * -c + float(p)))
    assert abs(fma - float(p) * (1 - c)) <= 2.0 ** -24 * float(p)


# ---- the group mask ------------------------------------------------------------------------------------------
def test_decay_group_mask():
    from qarig.optim import decay_group_mask
    sizes = [1, 7, 8, 9, 24]
    flags = [True, False, True, True, False]
    offs, total = [], 0
    for s in sizes:
        offs.append(total)
        total += (s + 7) // 8 * 8
    total += 16                                                      # trailing padding groups
    m = decay_group_mask(sizes, offs, total, flags)
    assert m.dtype == torch.uint8 and m.device.type == "cpu" and m.numel() == total // 8
    #                   1  7  8  9(two groups)  24(three)  padding
    assert m.tolist() == [1, 0, 1, 1, 1, 0, 0, 0, 0, 0]
    flipped = decay_group_mask(sizes, offs, total, [not f for f in flags])
    assert flipped.tolist() == [0, 1, 0, 0, 0, 1, 1, 1, 0, 0]
    assert decay_group_mask(sizes, offs, total, [False] * 5).sum() == 0
    with pytest.raises(ValueError, match="multiple of 8"):
        decay_group_mask([4, 4], [0, 4], 8, [True, False])
    with pytest.raises(ValueError):
        decay_group_mask([4], [0], 8, [True, False])
    with pytest.raises(ValueError):
        decay_group_mask([16], [0], 8, [True])


def _tiny_transformer(use_encoder):
    from models.Transformer import Transformer
    return Transformer(use_encoder=use_encoder, use_pos_cond=True, num_enc_layers=1 if use_encoder else None,
                       num_dec_layers=2, num_enc_embedding=8 if use_encoder else None, num_dec_embedding=17,
                       self_attn_heads=2, cross_attn_heads=2 if use_encoder else None, transformer_in_dim=16,
                       transformer_out_dim=17, transformer_hidden_dim=32)


@pytest.mark.parametrize("use_encoder", [False, True])
def test_decay_parameters_are_exactly_the_linear_weights(use_encoder):
    from qarig.optim import decay_parameters
    m = _tiny_transformer(use_encoder)
    got = decay_parameters(m)
    want = [mod.weight for mod in m.modules() if isinstance(mod, torch.nn.Linear)]
    assert len(got) == len(want) > 0 and all(a is b for a, b in zip(got, want))
    assert len({id(p) for p in got}) == len(got)
    names = {id(p): n for n, p in m.named_parameters()}
    assert all(names[id(p)].endswith(".weight") and p.dim() == 2 for p in got)
    others = [n for n, p in m.named_parameters() if id(p) not in {id(q) for q in got}]
    assert any(n.endswith(".bias") for n in others)
    for mod in m.modules():
        if isinstance(mod, (torch.nn.Embedding, torch.nn.LayerNorm)):
            assert all(id(p) not in {id(q) for q in got} for p in mod.parameters())
    assert any("embedding" in n for n in others)


@pytest.mark.parametrize("wd", [0.0, -0.1, 1.5, float("nan"), float("inf")])
def test_enable_weight_decay_rejects_values_outside_its_range(wd):
    from qarig.optim import FlatAdam
    with pytest.raises(ValueError):         # the check comes before anything touches the optimizer
        FlatAdam.enable_weight_decay(types.SimpleNamespace(), wd, [])


# ---- schedules -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lr_step", [1, 2, 5])
def test_step_schedule_replays_the_loops_halvings(lr_step):
    """The training loop, literally: step t runs with the group's lr, then `global_steps % lr_step == 0 and
    global_steps > 0` halves it (global_steps = t - 1 at that point)."""
    from qarig import cli_common as cc
    from qarig.optim import LRSchedule
    base = 1e-3
    opt = types.SimpleNamespace(param_groups=[{"lr": base}])
    used, global_steps = [], 0
    for _ in range(3 * lr_step + 2):
        used.append(opt.param_groups[0]["lr"])
        if global_steps % lr_step == 0 and global_steps > 0:
            cc.halve_lr(opt)
        global_steps += 1
    s = LRSchedule(base, "step", lr_step=lr_step)
    assert [s.lr(t) for t in range(1, len(used) + 1)] == used
    assert used[0] == used[1] == base and used[-1] < base


@pytest.mark.parametrize("kind", ["step", "cosine"])
def test_warmup_is_linear_and_reaches_base(kind):
    from qarig.optim import LRSchedule
    base, W = 3e-4, 8
    s = LRSchedule(base, kind, lr_step=10 ** 6, warmup_steps=W, decay_steps=100)
    for t in range(1, W + 1):
        assert s.lr(t) == pytest.approx(base * t / W, rel=1e-15)
    assert s.lr(W) == base
    assert s.lr(1) == pytest.approx(base / W, rel=1e-15)


@pytest.mark.parametrize("W,T,r", [(0, 10, 0.0), (2, 5, 0.0), (4, 20, 0.1), (3, 4, 0.5), (0, 1, 1.0)])
def test_cosine_schedule(W, T, r):
    from qarig.optim import LRSchedule
    base = 1e-3
    s = LRSchedule(base, "cosine", warmup_steps=W, decay_steps=T, min_ratio=r)
    if W:
        assert s.lr(W) == base
    assert s.lr(W + 1) == base                          # u = 0: the decay starts from base
    for t in (T + 1, T + 2, 10 * T + 7):
        assert s.lr(t) == pytest.approx(base * r, rel=1e-15, abs=1e-19)
    seq = [s.lr(t) for t in range(W + 1, T + 2)]
    assert all(a >= b for a, b in zip(seq, seq[1:]))
    if r < 1.0 and T - W >= 2:
        assert all(a > b for a, b in zip(seq, seq[1:]))
    # the closed form, at one interior point
    if T - W >= 2:
        t = W + 2
        u = (t - 1 - W) / max(1, T - W)
        assert s.lr(t) == pytest.approx(base * (r + (1 - r) * 0.5 * (1 + math.cos(math.pi * u))), rel=1e-15)


@pytest.mark.parametrize("kwargs", [
    dict(base_lr=0.0, kind="step", lr_step=5), dict(base_lr=float("nan"), kind="step", lr_step=5),
    dict(base_lr=1e-3, kind="linear", lr_step=5), dict(base_lr=1e-3, kind="step"),
    dict(base_lr=1e-3, kind="step", lr_step=0), dict(base_lr=1e-3, kind="cosine"),
    dict(base_lr=1e-3, kind="cosine", decay_steps=0), dict(base_lr=1e-3, kind="cosine", decay_steps=4, warmup_steps=5),
    dict(base_lr=1e-3, kind="cosine", decay_steps=4, warmup_steps=-1),
    dict(base_lr=1e-3, kind="cosine", decay_steps=4, warmup_steps=1.5),
    dict(base_lr=1e-3, kind="cosine", decay_steps=4, min_ratio=1.5),
    dict(base_lr=1e-3, kind="cosine", decay_steps=4, min_ratio=float("nan"))])
def test_schedule_refuses_bad_arguments(kwargs):
    from qarig.optim import LRSchedule
    with pytest.raises(ValueError):
        LRSchedule(**kwargs)


def test_schedule_refuses_step_zero():
    from qarig.optim import LRSchedule
    with pytest.raises(ValueError):
        LRSchedule(1e-3, "step", lr_step=5).lr(0)


# ---- the command line's checks -------------------------------------------------------------------------------
def test_check_optimizer_args():
    from qarig import cli_common as cc
    assert cc.check_optimizer_args(0.0, "step", 0, None, 0.0) == (0.0, "step", 0, None, 0.0)
    assert cc.check_optimizer_args(0.01, "cosine", 2, 6, 0.1) == (0.01, "cosine", 2, 6, 0.1)
    for bad in [(-0.1, "step", 0, None, 0.0), (1.5, "step", 0, None, 0.0), (float("nan"), "step", 0, None, 0.0),
                (0.0, "cosine", 0, None, 0.0), (0.0, "cosine", 5, 4, 0.0), (0.0, "step", -1, None, 0.0),
                (0.0, "cosine", 0, 4, 1.5), (0.0, "linear", 0, None, 0.0), (0.0, "cosine", 0, 0, 0.0)]:
        with pytest.raises(ValueError):
            cc.check_optimizer_args(*bad)
    assert not cc.optimizer_args_are_default(0.0, "step", 1, None, 0.0)
    assert cc.optimizer_args_are_default(0.0, "step", 0, None, 0.0)
    assert not cc.optimizer_args_are_default(0.01, "step", 0, None, 0.0)
