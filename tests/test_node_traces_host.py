"""Every Linear / MLP autograd node, in every precision mode and gradient situation, issues the `qarig.ops` calls
that tests/node_traces.json records: same entry points, order, operands (which tensor, its shape, strides and
offset, whether it came from torch.zeros or torch.empty), scalar arguments, in-place writes into .grad slots,
_report_done calls and returned gradients.  The record was taken from the six hand-written reduced-precision
node classes and the fp32 three-block node before they were folded into shared shells (tests/node_trace.py says
how); it is the definition of what the shells must launch, not a snapshot to refresh."""
import json
import os

import pytest

import node_trace

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "node_traces.json")) as f:
    RECORDED = json.load(f)


def test_the_record_covers_every_case():
    assert sorted(RECORDED) == sorted(node_trace.cases())
    for entry in RECORDED.values():
        assert sorted(entry) == sorted(("forward",) + node_trace.SITUATIONS)


@pytest.mark.parametrize("situation", node_trace.SITUATIONS)
@pytest.mark.parametrize("key", sorted(node_trace.cases()))
def test_node_issues_the_recorded_launches(monkeypatch, key, situation):
    fwd, bwd = node_trace.trace(monkeypatch, key, situation)
    assert fwd == RECORDED[key]["forward"]
    assert bwd == RECORDED[key][situation]


def test_reduced_precision_cases_reach_the_reduced_precision_nodes():
    """The shapes are the smallest the nodes' own predicates accept: every non-fp32 case runs the node of its
    mode, not the fp32 fallback."""
    want = {"linear_act": "_LinearAct", "mlp2": "_MLP2", "mlp2x3": "_MLP2x3", "mlp2xg": "_MLP2"}
    for key, entry in RECORDED.items():
        node, mode = key.split("/")[:2]
        suffix = {"f32": "", "mxfp8": "MX"}.get(mode, "LP")
        outs = [l for l in entry["forward"] if l.startswith("out ")]
        assert outs and all(l.endswith(f" {want[node]}{suffix}Backward") for l in outs), key
