"""The training attention kernels -- the 4x4-MFMA family of csrc/attention.hip (head dims 4 ... 64), its bf16-product
instantiation and the lane-per-row family of csrc/attention_wide.hip (head dim 128, and 65 ... 127 zero-padded) --
on inputs whose answer is known exactly, compared with fp64 PER ROW: o, the saved log-sum-exp, dq, dk and dv.

The inputs, the measure and the tolerances are those of tests/attention_selectors.py (read its docstring first;
tests/test_attention_selectors_host.py shows on the CPU that an fp32 restatement of the kernels' formulation stays
within half of each tolerance, so a failure here is the kernel's).  In short: every query selects, with equal weight,
the visible keys whose +-1 code is nearest to its target's, so a key that is dropped (the last key of a ragged 8- or
16-key step, the first key of a new double-buffered chunk), duplicated, or leaked from behind the causal mask turns a
small-integer average into another one, and the online-softmax rescale factor is exactly 0 or 1; each row is judged
on its own absolute-sum scale, so a wrong early causal row or a wrong dk / dv row of a key that one query looks at
is not divided by the largest element of the tensor.

The log-sum-exp comes from ops.attention_fwd, which returns it.  Its base-2 unit is INTERNAL to the kernels (forward
and backward of one head dim always run on the same family); the test converts it to natural units and pins the
value only because the backward pass reads nothing else of the softmax.

Shapes (N = 2; heads cycle through 1, 3, 5, 6: one head, a ragged head group, a second group):
causal S in {1, 3, 16, 63, 64, 65, 129, 200, 257} and cross (1, 200), (130, 1), (65, 257), (200, 63) at d = 8 and 128;
{3, 65, 129} and (65, 257) at d = 4, 16, 32, 64; the zero-padded head dims 12 and 96 through
qarig.functional.attention at {65, 129}; every target pattern; the "offset" form (scores 2 gain b higher: |lse| up to
~650 base-2 units, the L2 term of the gradient tolerance) at S = 129 per head dim.  Workgroup geometries attn_qw /
attn_bw = (1, 1) and (4, 2) at d = 8 and 16, S = 257.  A Gaussian arm (q, k ~ 3 randn) covers the non-integer
arithmetic that selector data cannot.

QARIG_SELECTOR_REPORT=<file> writes the worst measured error per family and output in units of 2^-24
(profiles/r14_attention_selectors.txt is such a file)."""
import os

import pytest
import torch

import attention_selectors as A

pytestmark = pytest.mark.gpu

WORST = {}      # (family, data, output) -> [worst error in units of 2^-24, tolerance of that case, worst error / tolerance]


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("QARIG_SELECTOR_REPORT")
    if path and WORST:
        with open(path, "w") as f:
            f.write("# worst per-row error of the training attention kernels against fp64, in units of u = 2^-24\n"
                    "# (tests/test_gpu_attention_selectors.py; measure and tolerances: tests/attention_selectors.py)\n"
                    "# family data output worst_u tolerance_u_of_that_case worst_error_over_tolerance\n")
            for (fam, data, name), (e, t, r) in sorted(WORST.items()):
                f.write(f"{fam:5s} {data:9s} {name:4s} {e:12.3f} {t:12.1f} {r:8.3f}\n")


@pytest.fixture
def bf16_mode():
    from qarig import ops
    old = ops.PRECISION
    ops.PRECISION = "bf16"
    yield ops
    ops.PRECISION = old


@pytest.fixture
def option():
    from qarig import _lib
    saved = []

    def set_(name, value):
        saved.append((name, _lib.set_option(name, value)))

    yield set_
    for name, old in reversed(saved):
        _lib.set_option(name, old)


def _run_ops(case):
    """Forward and backward through the C ABI wrappers; the log-sum-exp in natural units."""
    from qarig import ops
    q, k, v, do = (A.to_rows(t).cuda() for t in (case.q, case.k, case.v, case.do))
    o, lse = ops.attention_fwd(q, k, v, case.H, case.causal)
    dq, dk, dv = ops.attention_bwd(q, k, v, o, do, lse, case.H, case.causal)
    got = {n: A.to_heads(t, case.H) for n, t in (("o", o), ("dq", dq), ("dk", dk), ("dv", dv))}
    got["lse"] = lse.double().cpu() * A.LN2
    return got


def _run_functional(case):
    """qarig.functional.attention (zero-pads the heads to the next kernel head dim); it does not return the lse."""
    from qarig import functional as QF
    b = [A.to_rows(t).cuda().requires_grad_(True) for t in (case.q, case.k, case.v)]
    o = QF.attention(b[0], b[1], b[2], case.H, case.causal)
    o.backward(A.to_rows(case.do).cuda())
    return {n: A.to_heads(t, case.H) for n, t in (("o", o), ("dq", b[0].grad), ("dk", b[1].grad), ("dv", b[2].grad))}


def _check(case, got, family, lp=False):
    err, tol = case.errors(got), case.tolerances(lp)
    print(f"{family} {case.kind} d={case.d} {case.Sq}x{case.Sk} H={case.H}: " +
          "  ".join(f"{n} {err[n] / A.U:.3g}u (tol {tol[n] / A.U:.4g}u)" for n in err))
    for n, e in err.items():
        w = WORST.setdefault((family, case.kind, n), [0.0, tol[n] / A.U, 0.0])
        if e / A.U > w[0]:
            w[0], w[1] = e / A.U, tol[n] / A.U
        w[2] = max(w[2], e / tol[n])
    for n, t in got.items():
        assert torch.isfinite(t).all(), f"{n}: non-finite values"
    for n, e in err.items():
        assert e <= tol[n], f"{n}: worst row {e / A.U:.4g} u, tolerance {tol[n] / A.U:.4g} u"


def _family(d):
    return "wide" if d > 64 else "mfma"


def _cases(dims):
    return [pytest.param(d, Sq, Sk, c, H, off, id=f"d{d}-{Sq}x{Sk}-{'causal' if c else 'cross'}-H{H}" +
                         ("-offset" if off else ""))
            for d in dims for (Sq, Sk, c, H, off) in A.selector_shapes(d)]


@pytest.mark.parametrize("pattern", A.PATTERNS)
@pytest.mark.parametrize("d,Sq,Sk,causal,H,offset", _cases((4, 8, 16, 32, 64, 128)))
def test_selector_rows_fp32(d, Sq, Sk, causal, H, offset, pattern):
    case = A.selector_case(Sq, Sk, H, d, causal, pattern, offset)
    _check(case, _run_ops(case), _family(d))


@pytest.mark.parametrize("pattern", A.PATTERNS)
@pytest.mark.parametrize("d,Sq,Sk,causal,H,offset", _cases((12, 96)))
def test_selector_rows_zero_padded_heads(d, Sq, Sk, causal, H, offset, pattern):
    """Head dims 12 (on the 16-wide MFMA kernel) and 96 (on the 128-wide family) with the model's own 1/sqrt(d)."""
    case = A.selector_case(Sq, Sk, H, d, causal, pattern, offset)
    _check(case, _run_functional(case), _family(d))


@pytest.mark.parametrize("pattern", A.PATTERNS)
@pytest.mark.parametrize("d", [8, 16])
@pytest.mark.parametrize("qw,bw", [(1, 1), (4, 2)])
def test_selector_rows_workgroup_geometries(option, qw, bw, d, pattern):
    """1 and 4 query slices, 1 and 2 key slices per head (the default is 2 / 2) at S = 257: five 64-row waves."""
    option("attn_qw", qw)
    option("attn_bw", bw)
    case = A.selector_case(257, 257, 5, d, True, pattern, False)
    _check(case, _run_ops(case), "mfma")


LP_SHAPES = [(3, 3, True, False), (65, 65, True, False), (129, 129, True, False), (257, 257, True, False),
             (65, 257, False, False), (129, 129, True, True)]      # Sq, Sk, causal, offset


@pytest.mark.parametrize("pattern", A.PATTERNS)
@pytest.mark.parametrize("d,Sq,Sk,causal,H,offset",
                         [pytest.param(d, Sq, Sk, c, A.HEAD_CYCLE[n % 4], off,
                                       id=f"d{d}-{Sq}x{Sk}-{'causal' if c else 'cross'}" + ("-offset" if off else ""))
                          for d in (8, 16, 64) for n, (Sq, Sk, c, off) in enumerate(LP_SHAPES)])
def test_selector_rows_bf16_products(bf16_mode, d, Sq, Sk, causal, H, offset, pattern):
    """ops.PRECISION = "bf16": every operand is exact in bf16 and every unnormalised probability that carries weight
    is 1, so o and the lse hold the fp32 tolerance; the gradients carry the bf16 roundings of p and dS.  (o holds it
    because the kernel divides the rounded PV product by the sum of the ROUNDED probabilities: with the unrounded sum
    the offset form and the masked targets, whose largest score lies hundreds of units from zero, measured 134 - 179 u.)"""
    case = A.selector_case(Sq, Sk, H, d, causal, pattern, offset)
    _check(case, _run_ops(case), "lp", lp=True)


@pytest.mark.parametrize("Sq,Sk,causal,H,d", A.GAUSSIAN_SHAPES)
def test_gaussian_rows_fp32(Sq, Sk, causal, H, d):
    case = A.gaussian_case(Sq, Sk, H, d, causal)
    _check(case, _run_ops(case), _family(d))
