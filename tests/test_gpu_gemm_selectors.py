"""The fp32-result GEMM kernels -- the three split-bf16 kernels of csrc/gemm_x3.hip (128 x 128 tile, 64 x 64 "half"
tile, grouped) in every operand layout, and the fp32-MFMA kernels of csrc/gemm.hip / gemm64.hip as the control arm --
on operands whose answer is known exactly, judged PER ELEMENT.

The inputs, the measure and the tolerances are those of tests/gemm_selectors.py (read its docstring first;
tests/test_gemm_selectors_host.py shows on the CPU that a faithful emulation of gemm_x3's arithmetic is bit-exact on
families 1 and 4 and stays within half of the tolerances of families 2 and 3, and that every mutant -- a small term
dropped, an l plane rotated in k or with rows exchanged, mm read from the other k half, an m plane shifted by a
column -- is rejected, so a failure here is the kernel's).  In short: one-hot and few-term operands route ONE known
(row, k) against ONE known (column, k) into each output element, so a low piece that a staging map sends to another
row, k position or plane, or a cross term that is missing, shows at full size in the elements it touches instead of
at 2^-17 of one term of a Gaussian sum; power-of-two row and column scales must pass through bit for bit.

Kernels and the smallest shapes that reach them (csrc/gemm.hip gemm_dispatch, qarig_gemm_f32_grouped;
gemm_selectors.routes_to restates the arithmetic and every test asserts it):
    x3half     gemm_x3_half_kernel      gemm_x3 = 1   (256, 512, 64), (256, 512, 256) / 2 splits, (512, 512, 256) / 4
    x3full     gemm_x3_kernel           gemm_x3 = 2   (512, 1024, 64), (512, 1024, 256) / 2, (1024, 1024, 512) / 4
    x3auto     gemm_x3_kernel           gemm_x3 = 1   (2048, 1536, 64): 192 tiles, the half form steps aside
    x3grouped  gemm_x3_grouped_kernel   gemm_x3 = 1   2 x (512, 512, 64), 3 x (512, 512, 256) / 2
    f32, f32ring (gemm_tile64 = 0), f32regs (gemm_dma = 0), f32grouped: gemm_x3 = 0 on the same shapes
in all four (a_kcontig, b_kcontig) layouts, three for the grouped entry.  In the (kc, kc) layout the dispatch hands
M <= 512, K % 256 == 0 to the skinny-M kernel before any option is read, so there the K = 256 shapes run at K = 192
(two splits) and 384 (four): gemm_selectors.shapes_for.

On one-hot operands both arithmetics agree bit for bit, so agreement does not show which kernel ran: the `scale`
test also runs its unscaled Gaussian product under gemm_x3 = 0 and requires the two results to DIFFER in their bits
(the device of test_gpu_switches.py), for every x3 (kernel, shape, layout, split).

QARIG_GEMM_SELECTOR_REPORT=<file> writes the worst measured error per kernel, family and layout
(profiles/r15_gemm_selectors.txt is such a file)."""
import os

import pytest
import torch

import gemm_selectors as S

pytestmark = pytest.mark.gpu

WORST = {}      # (kernel, family, layout) -> [worst error in u (exact families: mismatching elements), tolerance in u, cases]


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("QARIG_GEMM_SELECTOR_REPORT")
    if path and WORST:
        with open(path, "w") as f:
            f.write("# worst per-element error of the fp32-result GEMM kernels, in units of u = 2^-24 of the element's own\n"
                    "# scale (tests/test_gpu_gemm_selectors.py; families, measure and tolerances: tests/gemm_selectors.py).\n"
                    "# pow2, scale, nonfinite are bit-exact families: the figure is the number of mismatching elements.\n"
                    "# kernel family layout cases worst tolerance worst_over_tolerance\n")
            for (kernel, family, layout), (e, t, n) in sorted(WORST.items()):
                if t:
                    f.write(f"{kernel:10s} {family:9s} {layout:5s} {n:3d} {e:8.3f} u {t:5.1f} u {e / t:6.3f}\n")
                else:
                    f.write(f"{kernel:10s} {family:9s} {layout:5s} {n:3d} {int(e):8d} mismatches, exact\n")


@pytest.fixture
def option():
    from qarig import _lib
    saved = []

    def set_(name, value):
        saved.append((name, _lib.set_option(name, value)))

    yield set_
    for name, old in reversed(saved):
        _lib.set_option(name, old)


def _layout(ak, bk):
    return ("kc" if ak else "xc") + "," + ("kc" if bk else "xc")


def _record(kernel, family, ak, bk, worst, tol):
    w = WORST.setdefault((kernel, family, _layout(ak, bk)), [0.0, tol, 0])
    w[0], w[2] = max(w[0], worst), w[2] + 1


def _cases(nonfinite=False):
    out = []
    for kernel, (_, shapes) in S.KERNELS.items():
        for ak, bk in S.LAYOUTS:
            for (M, N, K, sk) in S.shapes_for(shapes[1:2] if nonfinite and len(shapes) > 1 else shapes, ak, bk):
                out.append(pytest.param(kernel, 0, M, N, K, sk, ak, bk, id=f"{kernel}-{M}x{N}x{K}-sk{sk}-{_layout(ak, bk)}"))
    for kernel in S.GROUPED_KERNELS:
        for ak, bk in S.GROUPED_LAYOUTS:
            for (G, M, N, K, sk) in (S.GROUPED_SHAPES[1:] if nonfinite else S.GROUPED_SHAPES):
                out.append(pytest.param(kernel, G, M, N, K, sk, ak, bk,
                                        id=f"{kernel}-{G}x{M}x{N}x{K}-sk{sk}-{_layout(ak, bk)}"))
    return out


CASES = pytest.mark.parametrize("kernel,G,M,N,K,sk,ak,bk", _cases())


def _select(option, kernel, G, M, N, K, sk, ak, bk):
    """Sets the kernel's options and asserts that the dispatch sends this case to it."""
    from qarig import _lib
    if G:
        opts = S.GROUPED_KERNELS[kernel]
        assert S.grouped_routes_to_x3(G, M, N, K, sk) and (ak or not bk)
    else:
        opts = S.KERNELS[kernel][0]
        assert S.routes_to(kernel, M, N, K, sk, ak, bk)
        if kernel in ("x3full", "x3auto"):
            assert _lib.load().qarig_gemm_x3_ok(M, N, K, sk) == 1
    for name, value in opts.items():
        option(name, value)


def _dev(t, kcontig):
    return (t if kcontig else t.t().contiguous()).cuda()


def _products(G, As, Bs, sk, ak, bk, outs=None):
    """[C] on the CPU of the products A_g B_g^T (A_g (M, K), B_g (N, K) on the CPU, handed over in the layout asked
    for), one ops.gemm call (G = 0) or one grouped launch; outs: what to accumulate into."""
    from qarig import ops
    acc = outs is not None
    if not G:
        C = ops.gemm(_dev(As[0], ak), _dev(Bs[0], bk), a_kcontig=ak, b_kcontig=bk, splitk=sk,
                     out=outs[0].cuda() if acc else None, accumulate=acc)
        return [C.cpu()]
    M, K = As[0].shape
    N = Bs[0].shape[0]
    Cs = [o.cuda() for o in outs] if acc else [torch.empty((M, N), device="cuda") for _ in range(G)]
    ops.gemm_grouped([_dev(a, ak) for a in As], [_dev(b, bk) for b in Bs], Cs, M, N, K, a_kcontig=ak, b_kcontig=bk,
                     splitk=sk, accumulate=acc)
    return [c.cpu() for c in Cs]


def _sparse(family, G, M, N, K, mirror):
    return [S.sparse_case(family, M, N, K, mirror, g) for g in range(max(G, 1))]


@CASES
def test_one_hot_power_of_two_is_bit_exact(option, kernel, G, M, N, K, sk, ak, bk):
    """Family 1 and its mirror: C(m, n) = A(m, kappa(n)) 2^e(n) bit for bit, in every kernel."""
    _select(option, kernel, G, M, N, K, sk, ak, bk)
    for mirror in (False, True):
        cases = _sparse("pow2", G, M, N, K, mirror)
        Cs = _products(G, [c.A for c in cases], [c.B for c in cases], sk, ak, bk)
        for g, (c, C) in enumerate(zip(cases, Cs)):
            want = c.ref.float()
            bad = ~((C == want) & torch.isfinite(C))
            _record(kernel, "pow2", ak, bk, int(bad.sum()), 0.0)
            assert torch.equal(C, want), \
                f"mirror={mirror} group {g}: {int(bad.sum())} elements differ; (m, n, k, got, want): {S.failing(C, c, bad)}"


def _judge(kernel, family, ak, bk, C, case, ref, den, tol, what):
    assert torch.isfinite(C).all(), f"{what}: non-finite values"
    e = S.errors_u(C, ref, den)
    worst = float(e.max())
    print(f"{kernel} {family} {what}: worst {worst:.3f} u (tolerance {tol} u)")
    _record(kernel, family, ak, bk, worst, tol)
    assert worst <= tol, (f"{what}: worst element {worst:.4g} u, tolerance {tol} u, {int((e > tol).sum())} elements above; "
                          f"(m, n, k, got, ref without out): {S.failing(C, case, e > tol)}")


@CASES
def test_one_hot_full_value_is_one_product_per_element(option, kernel, G, M, N, K, sk, ak, bk):
    """Family 2 and its mirror: one full x full product per output, all six cross terms in it, relative to itself."""
    _select(option, kernel, G, M, N, K, sk, ak, bk)
    for mirror in (False, True):
        cases = _sparse("prod", G, M, N, K, mirror)
        Cs = _products(G, [c.A for c in cases], [c.B for c in cases], sk, ak, bk)
        for g, (c, C) in enumerate(zip(cases, Cs)):
            _judge(kernel, "prod", ak, bk, C, c, c.ref, c.denom, S.PROD_TOL_U, f"mirror={mirror} group {g}")


@CASES
def test_few_terms_across_the_reduction(option, kernel, G, M, N, K, sk, ak, bk):
    """Family 3 and its mirror: four full terms per element, one per quarter of K (k steps, k-tiles, slabs), plain
    and accumulated into a full-valued `out`."""
    _select(option, kernel, G, M, N, K, sk, ak, bk)
    for mirror in (False, True):
        cases = _sparse("few", G, M, N, K, mirror)
        for acc in (False, True):
            Cs = _products(G, [c.A for c in cases], [c.B for c in cases], sk, ak, bk,
                           outs=[c.out.clone() for c in cases] if acc else None)
            for g, (c, C) in enumerate(zip(cases, Cs)):
                ref, den = c.target(acc)
                _judge(kernel, "few", ak, bk, C, c, ref, den, S.FEW_TOL_U, f"mirror={mirror} accumulate={acc} group {g}")


@CASES
def test_power_of_two_scales_pass_through_bit_for_bit(option, kernel, G, M, N, K, sk, ak, bk):
    """Family 4: the kernel's own Gaussian product C0 holds the global fp32 tolerance, rows of A and columns of B scaled
    by powers of two give C0 2^(s + t) bit for bit, and (x3 kernels) C0 differs in its bits from the fp32-MFMA
    kernels' result on the same operands: the kernel under test ran."""
    _select(option, kernel, G, M, N, K, sk, ak, bk)
    cases = [S.dense_case(M, N, K, g) for g in range(max(G, 1))]
    C0s = _products(G, [d.A0 for d in cases], [d.B0 for d in cases], sk, ak, bk)
    Cs = _products(G, [d.A for d in cases], [d.B for d in cases], sk, ak, bk)
    for g, (d, C0, C) in enumerate(zip(cases, C0s, Cs)):
        err = S.global_err(C0, d.ref0)
        print(f"{kernel} scale group {g}: max|err| / max|ref| {err:.3g} (tolerance {d.global_tol:.3g})")
        assert err < d.global_tol
        want = C0 * d.scale
        bad = ~((C == want) & torch.isfinite(C))
        _record(kernel, "scale", ak, bk, int(bad.sum()), 0.0)
        rows, cols = bad.any(1).nonzero().flatten()[:8].tolist(), bad.any(0).nonzero().flatten()[:8].tolist()
        assert torch.equal(C, want), f"group {g}: {int(bad.sum())} elements differ, first rows {rows}, first columns {cols}"
    if kernel.startswith("x3"):
        option("gemm_x3", 0)
        F0s = _products(G, [d.A0 for d in cases], [d.B0 for d in cases], sk, ak, bk)
        for g, (d, C0, F0) in enumerate(zip(cases, C0s, F0s)):
            assert S.global_err(F0, d.ref0) < d.global_tol
            assert not torch.equal(C0, F0), f"group {g}: the same bits as under gemm_x3 = 0 -- the x3 kernel did not run"


@pytest.mark.parametrize("kernel,G,M,N,K,sk,ak,bk", _cases(nonfinite=True))
def test_nonfinite_operands_stay_in_their_row_and_column(option, kernel, G, M, N, K, sk, ak, bk):
    """Family 5: one inf in A(i, k) and one NaN in B(j, k') make row i and column j non-finite (gemm_x3 gives NaN
    where the fp32 chain gives +-inf: either will do) and leave every other element bit-identical to the clean run."""
    _select(option, kernel, G, M, N, K, sk, ak, bk)
    cases = [S.dense_case(M, N, K, g) for g in range(max(G, 1))]
    clean = _products(G, [d.A0 for d in cases], [d.B0 for d in cases], sk, ak, bk)
    dirty = [d.nonfinite() for d in cases]
    got = _products(G, [a for a, _ in dirty], [b for _, b in dirty], sk, ak, bk)
    for g, (d, C0, C) in enumerate(zip(cases, clean, got)):
        i, j = d.bad_a[0], d.bad_b[0]
        assert torch.isfinite(C0).all()
        assert not torch.isfinite(C[i, :]).any(), f"group {g}: finite elements in row {i}"
        assert not torch.isfinite(C[:, j]).any(), f"group {g}: finite elements in column {j}"
        rest = torch.ones((M, N), dtype=torch.bool)
        rest[i, :] = False
        rest[:, j] = False
        bad = rest & ~(C == C0)
        _record(kernel, "nonfinite", ak, bk, int(bad.sum()), 0.0)
        assert not bad.any(), f"group {g}: {int(bad.sum())} elements outside row {i} and column {j} changed: " \
                              f"{bad.nonzero()[:6].tolist()}"
