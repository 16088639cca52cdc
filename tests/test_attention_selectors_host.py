"""CPU self-test of tests/attention_selectors.py: the selector inputs select, they are exact in bf16, the closed-form
fp64 reference agrees with torch's autograd, and an fp32 restatement of the kernels' formulation stays within HALF of
every tolerance that tests/test_gpu_attention_selectors.py applies on the GPU -- so the reference and the measure
pass on their own and a failure there is the kernel's."""
import pytest
import torch

import attention_selectors as A

# Sq, Sk, causal, H, d: chunk / wave / head-group edges, both families, a cross shape, d with and without spare columns
SHAPES = [(3, 3, True, 3, 4), (65, 65, True, 5, 8), (257, 257, True, 1, 8), (129, 129, True, 6, 16),
          (65, 257, False, 3, 64), (200, 63, False, 6, 8), (129, 129, True, 3, 128), (130, 1, False, 5, 128)]


def test_selector_parameters():
    assert [A.selector_params(d) for d in (4, 8, 12, 16, 32, 64, 96, 128)] == \
        [(3, 32), (7, 64), (10, 64), (10, 64), (10, 128), (10, 128), (10, 128), (10, 256)]


@pytest.mark.parametrize("offset", [False, True])
@pytest.mark.parametrize("Sq,Sk,causal,H,d", SHAPES)
def test_selector_rows_select_and_survive_bf16(Sq, Sk, causal, H, d, offset):
    b, gain = A.selector_params(d)
    for pattern in A.PATTERNS:
        c = A.selector_case(Sq, Sk, H, d, causal, pattern, offset)
        mass, spread = A.selector_mass(c)
        assert mass >= 1 - 1e-7, (pattern, mass)
        assert spread < 1e-12, (pattern, spread)
        for t in (c.q, c.k, c.v, c.do):
            assert torch.equal(t.bfloat16().double(), t) and torch.equal(t.float().double(), t)
        # the raw score is the Hamming distance to the target's code
        j = torch.arange(Sk)
        ham = sum((((j[None, None, None, :] ^ c.pi[..., None]) >> t) & 1) for t in range(b))
        want = -2.0 * gain * ham + (2.0 * gain * b if offset else 0.0)
        assert torch.equal(c.q @ c.k.transpose(-1, -2), want.double())
        assert 2 * gain / d ** 0.5 >= 24.0
        # heads differ
        if H > 1 and Sk > 1 and Sq > 1:
            assert not torch.equal(c.q[:, 0], c.q[:, 1])


@pytest.mark.parametrize("Sq,Sk,causal,H,d", SHAPES[:5])
def test_closed_form_reference_is_torch_autograd(Sq, Sk, causal, H, d):
    for case in (A.selector_case(Sq, Sk, H, d, causal, "rand", False), A.gaussian_case(Sq, Sk, H, d, causal)):
        want = A.autograd_reference(case.q, case.k, case.v, case.do, causal)
        for name, err in case.errors(want).items():      # two fp64 evaluations: rounding at 2^-53 of the same scale
            assert err < 1e-12, (name, err)
    # the layout helpers invert each other
    assert torch.equal(A.to_heads(A.to_rows(case.q), H), case.q.float().double())


def test_measure_sees_one_wrong_row_and_one_leaked_key():
    c = A.selector_case(65, 65, 3, 8, True, "next", False)
    tol = c.tolerances()
    good = {n: t.clone() for n, t in c.ref.items()}
    assert all(e == 0.0 for e in c.errors(good).values())
    bad = {n: t.clone() for n, t in c.ref.items()}
    bad["dk"][1, 2, 64, 3] += 1e-3          # one element of the row of the key that one query sees
    assert c.errors(bad)["dk"] > tol["dk"]
    # one key past the diagonal: the masked target itself becomes visible
    q, k, v, do = c.q, c.k, c.v, c.do
    s = (q @ k.transpose(-1, -2) / 8 ** 0.5).masked_fill(torch.triu(torch.ones(65, 65, dtype=torch.bool), 2),
                                                         float("-inf"))
    leak = {"o": torch.softmax(s, -1) @ v, "lse": torch.logsumexp(s, -1)}
    err = c.errors(leak)
    assert err["o"] > 1e-2 and err["lse"] > 1e-2


@pytest.mark.parametrize("offset", [False, True])
@pytest.mark.parametrize("Sq,Sk,causal,H,d", SHAPES)
def test_fp32_restatement_within_half_of_the_selector_tolerances(Sq, Sk, causal, H, d, offset):
    families = ("wide",) if d == 128 else ("mfma", "lp")
    for pattern in A.PATTERNS:
        c = A.selector_case(Sq, Sk, H, d, causal, pattern, offset)
        for fam in families:
            got = A.restate_fp32(c.q, c.k, c.v, c.do, causal, fam)
            err, tol = c.errors(got), c.tolerances(lp=fam == "lp")
            for name in A.OUTPUTS:
                assert torch.isfinite(got[name]).all()
                assert err[name] <= 0.5 * tol[name], (fam, pattern, name, err[name] / A.U, tol[name] / A.U)


@pytest.mark.parametrize("Sq,Sk,causal,H,d", A.GAUSSIAN_SHAPES)
def test_fp32_restatement_within_half_of_the_gaussian_tolerance(Sq, Sk, causal, H, d):
    c = A.gaussian_case(Sq, Sk, H, d, causal)
    got = A.restate_fp32(c.q, c.k, c.v, c.do, causal, "wide" if d == 128 else "mfma")
    err, tol = c.errors(got), c.tolerances()
    for name in A.OUTPUTS:
        assert err[name] <= 0.5 * tol[name], (name, err[name] / A.U, tol[name] / A.U)


def test_case_lists_cover_what_the_gpu_file_states():
    full = A.selector_shapes(8)
    assert [s[0] for s in full[:9]] == list(A.CAUSAL_LENGTHS) and all(s[2] for s in full[:9])
    assert [(s[0], s[1]) for s in full[9:13]] == list(A.CROSS_SHAPES) and not any(s[2] for s in full[9:13])
    assert A.selector_shapes(128) == full
    for d in (4, 8, 12, 16, 32, 64, 96, 128):
        sh = A.selector_shapes(d)
        assert sum(s[4] for s in sh) == 1                              # the offset form at one length
        assert {s[3] for s in sh} <= set(A.HEAD_CYCLE)
        if d not in (12, 96):
            assert {s[3] for s in sh} == set(A.HEAD_CYCLE)
