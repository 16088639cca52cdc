"""The reduced-precision Linear / MLP nodes (qarig.functional_lp: two shells, a backend per number format) against
the fp32 nodes from the same weights, in every gradient situation the shells branch on -- not only "every leaf
requires a gradient and owns no .grad", which is what the tolerance tests of test_gpu_bf16 / test_gpu_fp8 /
test_gpu_mxfp8 run:
    all          every leaf requires a gradient, no .grad yet: the node returns the gradients;
    slots        every parameter owns a contiguous fp32 .grad filled with FILL: the kernels accumulate into it
                 (through a temporary where the padded width differs) and the node returns None;
    frozen       only the activations require a gradient: no weight / bias gradient product is launched;
    params-only  the input requires none: no input-gradient product.
Shapes: the smallest the nodes accept (1,024 rows; 128 -> 256 -> 128 or a ragged 130 columns).  Criterion and
bounds are those tests' own, per mode: "bf16" relative error of the tensor < 1.5e-2 and cosine > 0.9999
(test_lp_mlp_nodes_track_fp32_nodes); "fp8" cosine > 0.997 for outputs and input gradients, > 0.995 for weight
and bias gradients (test_f8_mlp_and_linear_nodes_track_fp32_nodes); "mxfp8" > 0.997 and > 0.99
(test_mx_nodes_track_fp32_nodes).  A slot must hold FILL + gradient afterwards: FILL is several times the largest
gradient entry, so a kernel that overwrote the slot instead of accumulating fails the same criterion."""
import functools
import itertools

import pytest
import torch

from conftest import rel_err

pytestmark = pytest.mark.gpu

ROWS, K, H = (2, 512), 128, 256
FILL = 1024.0
SITUATIONS = ("all", "slots", "frozen", "params-only")
NODE = {"bf16": "LP", "fp8": "LP", "mxfp8": "MX"}
LINEAR = [("linear_act", c) for c in itertools.product((1, 0), (0, 1), (0, 1))]        # bias, residual, act
MLP2 = [("mlp2", c) for c in itertools.product((128, 130), (0, 1))]                     # N, act2
MLP2X3 = [("mlp2x3", (a,)) for a in (0, 1)]                                             # act2


def _cos(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a * b).sum() / (a.norm() * b.norm()))


def _close(mode, name, got, want):
    if mode == "bf16":
        return rel_err(got, want) < 1.5e-2 and _cos(got, want) > 0.9999
    activation = name == "x" or name == "r" or name.startswith("y")
    return _cos(got, want) > (0.997 if activation else 0.995 if mode == "fp8" else 0.99)


@functools.lru_cache(maxsize=None)
def _data(kind, cfg):
    """(activations, parameters, incoming gradients) of one node: name -> tensor (or None)."""
    g = torch.Generator().manual_seed(11)
    rn = lambda *s, scale=1.0: (torch.randn(s, generator=g) * scale).cuda()
    acts, params = {"x": rn(*ROWS, K)}, {}
    if kind == "linear_act":
        bias, res, _ = cfg
        acts["r"] = rn(*ROWS, H) if res else None
        params = {"w": rn(H, K, scale=0.09), "b": rn(H, scale=0.1) if bias else None}
        widths = [H]
    else:
        N = cfg[0] if kind == "mlp2" else 128
        for blk in ("",) if kind == "mlp2" else ("q.", "k.", "v."):
            params.update({blk + "w1": rn(H, K, scale=0.09), blk + "b1": rn(H, scale=0.1),
                           blk + "w2": rn(N, H, scale=0.06), blk + "b2": rn(N, scale=0.1)})
        widths = [N] * (len(params) // 4)
    return acts, params, [rn(*ROWS, n) for n in widths]


def _run(kind, cfg, situation):
    """name -> result: outputs y<i>, then the gradient of every leaf that requires one (for `slots`: what was
    added to the slot)."""
    from qarig import functional as QF
    acts, params, dys = _data(kind, cfg)
    a = {n: None if t is None else t.clone().requires_grad_(situation != "params-only") for n, t in acts.items()}
    p = {n: None if t is None else torch.nn.Parameter(t.clone(), requires_grad=situation != "frozen")
         for n, t in params.items()}
    slots = {}
    if situation == "slots":
        for n, t in p.items():
            if t is not None:
                t.grad = slots[n] = torch.full_like(t, FILL)
    if kind == "linear_act":
        outs = [QF.linear_act(a["x"], p["w"], p["b"], a["r"], cfg[2])]
    elif kind == "mlp2":
        outs = [QF.mlp2(a["x"], p["w1"], p["b1"], p["w2"], p["b2"], 1, cfg[1])]
    else:
        outs = QF.mlp2x3(a["x"], [tuple(p[b + n] for n in ("w1", "b1", "w2", "b2")) for b in ("q.", "k.", "v.")],
                         1, cfg[0])
    torch.autograd.backward(list(outs), dys)
    res = {f"y{i}": y.detach() for i, y in enumerate(outs)}
    res["grad_fn"] = type(outs[0].grad_fn).__name__
    for n, t in {**a, **p}.items():
        if t is None or not t.requires_grad:
            assert t is None or t.grad is None
        elif n in slots:
            assert t.grad is slots[n], f"{n}: the node returned a gradient beside the .grad slot it was given"
            res[n] = t.grad - FILL
        else:
            res[n] = t.grad
    return res


@functools.lru_cache(maxsize=None)
def _fp32(kind, cfg):
    from qarig import functional as QF
    from qarig import ops
    old, ops.PRECISION = ops.PRECISION, "f32"
    grouped, QF.MLP_GROUPED = QF.MLP_GROUPED, "0"        # the three-block node, not the grouped launches
    try:
        return _run(kind, cfg, "all")
    finally:
        ops.PRECISION, QF.MLP_GROUPED = old, grouped


@pytest.mark.parametrize("kind,cfg", LINEAR + MLP2 + MLP2X3)
@pytest.mark.parametrize("mode", sorted(NODE))
def test_nodes_track_fp32_nodes_in_every_gradient_situation(mode, kind, cfg):
    from qarig import ops
    want = _fp32(kind, cfg)
    node = {"linear_act": "_LinearAct", "mlp2": "_MLP2", "mlp2x3": "_MLP2x3"}[kind]
    assert want["grad_fn"] == node + "Backward"
    old, ops.PRECISION = ops.PRECISION, mode
    try:
        for situation in SITUATIONS:
            got = _run(kind, cfg, situation)
            assert got.pop("grad_fn") == node + NODE[mode] + "Backward"
            leaves = {"all": set(want) - {"grad_fn"}, "slots": set(want) - {"grad_fn"},
                      "frozen": {n for n in want if n[0] in "yxr"},
                      "params-only": {n for n in want if n not in ("x", "r", "grad_fn")}}[situation]
            assert set(got) == leaves, (situation, sorted(got))
            for n, t in got.items():
                assert t.shape == want[n].shape and _close(mode, n, t, want[n]), (situation, n)
            assert not torch.equal(got["y0"], want["y0"])          # (the reduced-precision kernels did run)
    finally:
        ops.PRECISION = old
