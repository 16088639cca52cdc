"""CPU self-test of tests/gemm_selectors.py: the inputs are what they claim, the closed-form references are the fp64
matrix product, the faithful emulation of gemm_x3's arithmetic passes every family (bit-exactly where the family is
exact, within HALF of the tolerance elsewhere -- on the GPU test's own inputs, from which the tolerances are fixed),
every mutant of it is rejected by the families named in REJECTED_BY, and the measure sees one wrong element.  So the
references and the measure pass on their own, and a failure of tests/test_gpu_gemm_selectors.py is the kernel's."""
import math

import pytest
import torch

import gemm_selectors as S

SMALL = [(128, 128, 64), (96, 160, 64)]          # M, N, K: emulated densely, product by product
ARMS = [("pow2", False), ("pow2", True), ("prod", False), ("prod", True), ("few", False), ("few", True)]
BF16_MIN_NORMAL = 2.0 ** -126

# mutant -> the (family, mirror) arms it must fail.  A one-hot power of two has an h piece only, so the arm whose
# one-hot side is A (mirror) cannot see a fault of A's m or l plane, and so on; `prod` and `few` carry all six terms
# on both sides; `scale` (power-of-two invariance) sees what mixes rows or columns, not what stays inside them.
BOTH = [("prod", False), ("prod", True)]
REJECTED_BY = {
    "drop_lh": [("pow2", False)] + BOTH,
    "drop_hl": [("pow2", True)] + BOTH,
    "drop_mm": BOTH,
    "drop_mh": [("pow2", False)] + BOTH,
    "drop_hm": [("pow2", True)] + BOTH,
    "rot_l_a": [("pow2", False)] + BOTH,
    "rot_l_b": [("pow2", True)] + BOTH,
    "swap_rows_l_a": [("pow2", False), ("scale", None)] + BOTH,
    "swap_rows_l_b": [("pow2", True), ("scale", None)] + BOTH,
    "mm_other_half": BOTH,
    "shift_m_b": [("pow2", True), ("scale", None)] + BOTH,
}


def _tol(family):
    return {"prod": S.PROD_TOL_U, "few": S.FEW_TOL_U}[family]


def _passes(C, case):
    """The GPU test's verdict on a result of a Sparse case."""
    if case.family == "pow2":
        return torch.equal(C, case.ref.float())
    return S.worst_u(C, case.ref, case.denom) <= _tol(case.family)


def test_kappa_is_onto_at_every_shape_and_neighbours_differ():
    shapes = [(M, N, K) for M, N, K, _ in S.ALL_SHAPES] + [(M, N, K) for _, M, N, K, _ in S.GROUPED_SHAPES] + SMALL + \
             [(M, N, K) for ak, bk in S.LAYOUTS for M, N, K, _ in S.shapes_for(S.ALL_SHAPES, ak, bk)]
    for (M, N, K) in set(shapes):
        assert K % 32 == 0 and K <= min(M, N)
        for X in (M, N):
            k = S.kappa(X, K, 11)
            assert sorted(set(k[:K].tolist())) == list(range(K))
            d = (k[1:] - k[:-1]) % K
            assert (d == S.stride_of(K) % K).all() and S.stride_of(K) % 2 == 1 and math.gcd(S.stride_of(K), K) == 1
            assert (k[1:] // 8 != k[:-1] // 8).all()                      # another k octet, hence another ...
        q = K // S.T_FEW
        assert q % 16 == 0


@pytest.mark.parametrize("M,N,K", SMALL + [(256, 512, 256)])
def test_inputs_are_what_they_claim(M, N, K):
    for family, mirror in ARMS:
        c = S.sparse_case(family, M, N, K, mirror)
        T = S.T_FEW if family == "few" else 1
        sparse, dense = (c.A, c.B) if mirror else (c.B, c.A)
        assert c.A.shape == (M, K) and c.B.shape == (N, K) and c.A.dtype == c.B.dtype == torch.float32
        assert ((sparse != 0).sum(1) == T).all() and (dense != 0).all()
        assert sorted(set(c.pos.flatten().tolist())) == list(range(K))    # every k carries a term
        if family == "pow2":
            m, e = torch.frexp(c.val)
            assert (m == 0.5).all() and (e - 1).min() >= -12 and (e - 1).max() <= 12
            assert torch.equal(c.ref.float().double(), c.ref)             # the answer is an fp32 number
        if family == "few":
            q = K // T
            assert (c.pos // q == torch.arange(T)[None, :]).all()         # one term in each quarter of K
            assert (c.val > 0).any() and (c.val < 0).any() and (c.out != 0).all()
        for v in ((c.D, c.val) if family != "pow2" else (c.D,)):
            h, m, l = S.split3(v)
            assert torch.equal(h.double() + m.double() + l.double(), v.double())
            assert float((l != 0).float().mean()) > 0.9                   # "full": the low piece is in play
            for p in (h, m, l):
                assert torch.equal(p.bfloat16().float(), p)
                assert ((p == 0) | (p.abs() >= BF16_MIN_NORMAL)).all()
            assert v.abs().min() >= 2.0 ** -100
    d = S.dense_case(M, N, K)
    for v in (d.A0, d.B0, d.A, d.B):
        assert v.abs().min() >= 2.0 ** -100 and v.abs().max() < 2.0 ** 40
        for p in S.split3(v):
            assert ((p == 0) | (p.abs() >= BF16_MIN_NORMAL)).all()
    assert d.s.min() >= -30 and d.s.max() <= 30 and d.t.min() >= -30 and d.t.max() <= 30
    assert torch.equal(d.A, d.A0 * torch.exp2(d.s)[:, None]) and torch.equal(torch.frexp(d.A)[0], torch.frexp(d.A0)[0])
    A, B = d.nonfinite()
    assert (~torch.isfinite(A)).sum() == 1 and (~torch.isfinite(B)).sum() == 1 and torch.isinf(A[d.bad_a])


@pytest.mark.parametrize("M,N,K", SMALL + [(256, 512, 256)])
def test_closed_form_references_are_the_fp64_product(M, N, K):
    for family, mirror in ARMS:
        c = S.sparse_case(family, M, N, K, mirror)
        want = c.A.double() @ c.B.double().t()
        assert float(((c.ref - want).abs() / c.denom).max()) < 1e-15 * S.T_FEW
        den = c.A.double().abs() @ c.B.double().abs().t()
        assert float(((c.denom - den).abs() / den).max()) < 1e-15 * S.T_FEW
        assert (c.denom >= c.ref.abs()).all() and (c.denom > 0).all()


@pytest.mark.parametrize("M,N,K", SMALL)
def test_faithful_emulation_passes_every_family(M, N, K):
    for family, mirror in ARMS:
        c = S.sparse_case(family, M, N, K, mirror)
        for sk in (1, 2, 4):
            for acc in ((False, True) if family == "few" else (False,)):
                C = S.emulate(c.A, c.B, splitk=sk, out=c.out if acc else None)
                # the term-wise form used at the GPU test's shapes is the same arithmetic
                assert torch.equal(C, S.emulate_terms(c, splitk=sk, accumulate=acc))
                ref, den = c.target(acc)
                if family == "pow2":
                    assert torch.equal(C, ref.float()), (mirror, sk)
                else:
                    assert S.worst_u(C, ref, den) <= 0.5 * _tol(family), (family, mirror, sk, acc)
    # family 1 is exact because of the kernels' ORDER: the same terms with h w first round
    c = S.sparse_case("pow2", M, N, K, False)
    assert not torch.equal(S.emulate(c.A, c.B, order=S.INEXACT_ORDER), c.ref.float())
    # family 4: bit-exact invariance under power-of-two row and column scales, and the global tolerance
    d = S.dense_case(M, N, K)
    for sk in (1, 2):
        C0 = S.emulate(d.A0, d.B0, splitk=sk)
        assert torch.equal(S.emulate(d.A, d.B, splitk=sk), C0 * d.scale)
        assert S.global_err(C0, d.ref0) < d.global_tol


def test_tolerances_are_twice_the_emulation_on_the_gpu_tests_own_inputs():
    """Over every shape, arm, split count, accumulate form and group that tests/test_gpu_gemm_selectors.py runs."""
    for family in ("prod", "few"):
        w = S.emulation_worst(family)
        print(f"{family}: faithful emulation worst {w:.3f} u, tolerance {_tol(family)} u")
        assert w <= 0.5 * _tol(family)
        assert _tol(family) == math.ceil(2 * w)


@pytest.mark.parametrize("mutant", S.MUTANTS)
def test_every_mutant_is_rejected(mutant):
    M, N, K = SMALL[0]
    arms = REJECTED_BY[mutant]
    assert arms and any(f in ("pow2", "prod") for f, _ in arms)
    for family, mirror in arms:
        if family == "scale":
            d = S.dense_case(M, N, K)
            assert not torch.equal(S.emulate(d.A, d.B, mutant=mutant), S.emulate(d.A0, d.B0, mutant=mutant) * d.scale)
            continue
        c = S.sparse_case(family, M, N, K, mirror)
        C = S.emulate(c.A, c.B, mutant=mutant)
        assert not _passes(C, c), (mutant, family, mirror)
        if family == "prod":
            assert S.worst_u(C, c.ref, c.denom) > 16 * S.PROD_TOL_U          # (a lost l piece: up to 2^-17 = 128 u)


def test_dropped_terms_stand_far_above_the_tolerance():
    """Family 2 on the CPU emulation: lh / hl ~128 u, mm ~256 u, mh / hm ~65 k u against a tolerance of a few u."""
    c = S.sparse_case("prod", 128, 128, 64, False)
    floor = {"drop_lh": 64, "drop_hl": 64, "drop_mm": 128, "drop_mh": 2 ** 15, "drop_hm": 2 ** 15}
    for mutant, least in floor.items():
        assert S.worst_u(S.emulate(c.A, c.B, mutant=mutant), c.ref, c.denom) > least, mutant


def test_measure_sees_one_wrong_element():
    M, N, K = SMALL[0]
    for family, mirror in ARMS:
        c = S.sparse_case(family, M, N, K, mirror)
        good = S.emulate(c.A, c.B)
        assert _passes(good, c)
        r = (c.ref.abs() / c.denom)
        m, n = divmod(int(r.argmax()), N)         # (for `few`: an element that does not cancel)
        bad = good.clone()
        bad[m, n] *= 1 + 2.0 ** -15
        assert not _passes(bad, c), (family, mirror)
        if family != "pow2":
            e = S.errors_u(bad, c.ref, c.denom)
            wrong = e > _tol(family)
            assert int(wrong.sum()) == 1 and S.failing(bad, c, wrong)[0][:3] == (m, n, c.positions(m, n))


def test_case_tables_route_where_they_say():
    """The dispatch arithmetic of csrc/gemm.hip on the shape tables: each x3 case reaches its kernel in every layout,
    and the K = 256 shapes would not in the (kc, kc) layout (the skinny-M kernel takes them first)."""
    for kernel, (opts, shapes) in S.KERNELS.items():
        for ak, bk in S.LAYOUTS:
            for (M, N, K, sk) in S.shapes_for(shapes, ak, bk):
                assert S.routes_to(kernel, M, N, K, sk, ak, bk), (kernel, M, N, K, sk, ak, bk)
                assert K % (16 * sk) == 0 and (K // S.T_FEW) % 16 == 0 and (K // sk) % (K // S.T_FEW) == 0
    assert not S.routes_to("x3half", 256, 512, 256, 2, True, True) and S.routes_to("x3half", 256, 512, 256, 2, True, False)
    assert not S.routes_to("x3auto", 256, 512, 64, 1, True, True) and not S.routes_to("x3half", 2048, 1536, 64, 1, True, True)
    for (G, M, N, K, sk) in S.GROUPED_SHAPES:
        assert S.grouped_routes_to_x3(G, M, N, K, sk)
    assert not S.grouped_routes_to_x3(1, 512, 512, 64, 1)
