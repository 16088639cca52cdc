"""The split-K reductions behind gemm() (slab_reduce_vec_kernel and the scalar slab_reduce_kernel /
slab_reduce_rowsum_kernel of csrc/gemm.hip) through ops.slab_reduce, bit for bit against a CPU loop that adds the
slabs z ascending in fp32 from 0.0f and the accumulate operand last.

(M, N) in {(128, 128), (512, 2048)} on a sub-view of a wider buffer (ldc = N + 8 > N: rows 16-B aligned, so the
16-B kernel), nslab in {1, 2, 8, 32} (below, at and past the 8 slabs of one unrolled load group, with a second and a
fourth trip), accumulate on and off, with and without the row-sum blocks behind the slab blocks; one ragged N = 130
(no multiple of 4) and one ldc off a multiple of 4 stay on the scalar kernels.  The slabs hold values of very
different magnitude, so another summation order would show.  Everything outside the written region of the padded
output must keep its bits."""
import pytest
import torch

pytestmark = pytest.mark.gpu

PAD_ROWS, GUARD = 3, -7.25


def _slabs(nslab, M, N, seed):
    gen = torch.Generator().manual_seed(seed)
    v = torch.randn((nslab, M, N), generator=gen)
    return v * torch.exp2(torch.randint(-12, 13, (nslab, M, N), generator=gen).float())


def _cpu_sum(slabs, base):
    s = torch.zeros(slabs.shape[1:], dtype=torch.float32)
    for z in range(slabs.shape[0]):
        s = s + slabs[z]
    return s if base is None else base + s


def _run(M, N, ldc, nslab, accumulate, rowsum, seed):
    from qarig import ops
    slabs = _slabs(nslab, M, N, seed)
    gen = torch.Generator().manual_seed(seed + 1)
    buf = torch.full((M + PAD_ROWS, ldc), GUARD)
    buf[:M, :N] = torch.randn((M, N), generator=gen)
    want = buf.clone()
    want[:M, :N] = _cpu_sum(slabs, buf[:M, :N] if accumulate else None)
    gbuf = buf.cuda()
    rs_part = rs_out = rs_want = None
    if rowsum:
        part = _slabs(nslab, M, 1, seed + 2)[:, :, 0].contiguous()
        rs0 = torch.randn(M + PAD_ROWS, generator=gen)
        rs_want = rs0.clone()
        rs_want[:M] = _cpu_sum(part, rs0[:M] if accumulate else None)
        rs_part, rs_out = part.cuda(), rs0.cuda()
    ops.slab_reduce(slabs.cuda(), gbuf, M, N, accumulate=accumulate, rs_part=rs_part,
                    rs_out=None if rs_out is None else rs_out[:M])
    where = (M, N, ldc, nslab, accumulate, rowsum)
    assert torch.equal(gbuf.cpu(), want), where       # the sums, and the guard values around them
    if rowsum:
        assert torch.equal(rs_out.cpu(), rs_want), where


@pytest.mark.parametrize("rowsum", (False, True), ids=("plain", "rowsum"))
@pytest.mark.parametrize("accumulate", (False, True), ids=("store", "accumulate"))
@pytest.mark.parametrize("nslab", (1, 2, 8, 32))
@pytest.mark.parametrize("M,N", ((128, 128), (512, 2048)))
def test_slab_reduce_vector_form(M, N, nslab, accumulate, rowsum):
    _run(M, N, N + 8, nslab, accumulate, rowsum, seed=M + nslab)


@pytest.mark.parametrize("rowsum", (False, True), ids=("plain", "rowsum"))
@pytest.mark.parametrize("accumulate", (False, True), ids=("store", "accumulate"))
@pytest.mark.parametrize("M,N,ldc", ((128, 130, 136), (128, 128, 131)), ids=("ragged_n", "ragged_ld"))
def test_slab_reduce_scalar_form(M, N, ldc, accumulate, rowsum):
    _run(M, N, ldc, 8, accumulate, rowsum, seed=N + ldc)


def test_slab_reduce_through_a_split_gemm():
    """The launch behind a split-K weight-gradient product: gemm(splitk = 8, a_rowsum) into a strided C equals the
    same product with the slabs written out and reduced on the CPU in slab order -- i.e. run to run and against
    the unsplit kernels' own slab sums the order has not moved."""
    from qarig import ops
    gen = torch.Generator().manual_seed(5)
    M, N, K = 256, 512, 1024
    A = torch.randn((K, M), generator=gen).cuda()          # dT: reduction-major, as in a weight gradient
    B = torch.randn((K, N), generator=gen).cuda()
    C1 = torch.zeros((M, N + 8), device="cuda")
    C2 = torch.zeros((M, N + 8), device="cuda")
    r1 = torch.zeros(M, device="cuda")
    r2 = torch.zeros(M, device="cuda")
    ops.gemm(A, B, a_kcontig=False, b_kcontig=False, splitk=8, out=C1[:, :N], a_rowsum=r1)
    ops.gemm(A, B, a_kcontig=False, b_kcontig=False, splitk=8, out=C2[:, :N], a_rowsum=r2)
    assert torch.equal(C1, C2) and torch.equal(r1, r2)
    assert (C1[:, N:] == 0).all()
    ref = A.double().t() @ B.double()
    assert float((C1[:, :N].double() - ref).abs().max() / ref.abs().max()) < 1e-5
    assert float((r1.double() - A.double().sum(0)).abs().max() / A.double().sum(0).abs().max()) < 1e-5
