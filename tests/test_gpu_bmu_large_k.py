"""The coarse-pass BMU search beyond 1,024 codes: the codebook goes through LDS in chunks over a (row block) x
(chunk group) grid, a finalize kernel merges the partial (min, index, second-smallest) states in code order, applies
the single-image form's certificate and re-scans the other rows against the fp32 codebook.  Every assertion on
indices is bit-equality with the C oracle (oracle/bmu_oracle.c), as in test_gpu_core.py's
test_bmu_coarse_pass_bit_exact."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BMU_COARSE_EPS = 1e-5       # csrc/bmu.hip


@pytest.fixture
def option():
    from qarig import _lib
    saved = []

    def set_(name, value):
        saved.append((name, _lib.set_option(name, value)))

    yield set_
    for name, old in reversed(saved):
        _lib.set_option(name, old)


def _certificate_bounds(x, w, p):
    """(lo, hi): rows whose gap between the two smallest t = -2 x.w + |w|^2 (fp64) is below eps -- the coarse values
    are within eps of t, so their gap is below 3 eps and the row MUST be re-scanned -- and rows whose gap is below
    5 eps -- a re-scanned row has a coarse gap of at most 3 eps, hence a true gap of at most 5 eps: only these MAY
    be.  eps as in the kernel: 1e-5 (1.001 |x|^2 + 2 max |w|^2)."""
    from oracle import bmu as obmu
    xp = torch.from_numpy(obmu.patchify(x.numpy(), (p, p)).copy()).double()
    wd = w.double()
    w2 = (wd * wd).sum(1)
    w2max = float(w2.max())
    lo = hi = 0
    for r0 in range(0, xp.shape[0], 1024):
        xb = xp[r0:r0 + 1024]
        t = -2.0 * xb @ wd.T + w2[None]
        two = torch.topk(t, 2, dim=1, largest=False).values
        gap = two[:, 1] - two[:, 0]
        eps = BMU_COARSE_EPS * (1.001 * (xb * xb).sum(1) + 2.0 * w2max)
        lo += int((gap < eps).sum())
        hi += int((gap < 5.0 * eps).sum())
    return lo, hi


def _search_every_way(x, w, p):
    """The common procedure: unprepared, prepared twice (the second call takes the cached image), prepared after the
    codebook changed; all equal to the oracle, prepared and unprepared re-scan counts equal.  Returns that count."""
    from qarig import ops
    from oracle import bmu as obmu
    xc = x.cuda()
    want = obmu.bmu(x.numpy(), w.numpy(), (p, p))
    got, cnt = ops.bmu_coarse(xc, w.cuda(), (p, p))
    assert np.array_equal(got.cpu().numpy(), want), int((got.cpu().numpy() != want).sum())
    cnt = int(cnt.item())
    wc = w.cuda()
    for _ in range(2):
        got_p, cnt_p = ops.bmu_coarse(xc, wc, (p, p), prepared=True)
        assert np.array_equal(got_p.cpu().numpy(), want), int((got_p.cpu().numpy() != want).sum())
        assert int(cnt_p.item()) == cnt
    assert id(wc) in ops._bmu_images
    wc.mul_(-1.0)                                   # the codebook changes: the image must follow
    got_n, _ = ops.bmu_coarse(xc, wc, (p, p), prepared=True)
    assert np.array_equal(got_n.cpu().numpy(), obmu.bmu(x.numpy(), (-w).numpy(), (p, p)))
    return cnt, want.size


@pytest.mark.parametrize("N,C,H,W,p,K,kind", [
    (2, 4, 64, 64, 1, 8192, "trained"),      # BASELINE configs[4]'s codebook, 8,192 rows
    (3, 4, 34, 26, 1, 1056, "trained"),      # 33 tiles: a partial last chunk; 2,652 rows: a partial last row block
    (2, 4, 64, 64, 2, 2048, "trained"),      # D = 16
    (2, 2, 64, 64, 2, 4096, "trained"),      # D = 8
    (1, 4, 8, 8, 1, 2048, "fresh"),          # 64 rows, (nearly) every one re-scanned
    (1, 4, 16, 16, 1, 2048, "dups"),         # duplicated codes in different chunks, patches that ARE codes
    (1, 4, 16, 16, 1, 2048, "tiny"),         # denormal-range data: every chunk inexact -> every row re-scanned
    (1, 4, 16, 16, 1, 2048, "wide"),         # large dynamic range
])
def test_bmu_chunked_coarse_pass_bit_exact(N, C, H, W, p, K, kind):
    g = torch.Generator().manual_seed(N + 3 * p + K + len(kind))
    D = C * p * p
    x = torch.tanh(torch.randn((N, C, H, W), generator=g))
    w = torch.tanh(torch.randn((K, D), generator=g))
    if kind == "fresh":
        w = (torch.rand((K, D), generator=g) * 2 - 1) / K
    elif kind == "dups":
        w[K - 1] = w[1]                              # the lower index must win across chunks
        w[K // 2 + 3] = w[3]
        img = w[:64].reshape(1, 64, C, p, p)         # patches that are codebook rows (d = 0, clamp): codes 0..63
        x[0, :, :8 * p, :8 * p] = img.reshape(8, 8, C, p, p).permute(2, 0, 3, 1, 4).reshape(C, 8 * p, 8 * p)
    elif kind == "tiny":
        x = x * 1e-39
        w = w * 1e-39
    elif kind == "wide":
        x = x * torch.exp(4 * torch.randn((N, 1, H, W), generator=g))
        w = w * torch.exp(4 * torch.randn((K, 1), generator=g))
    cnt, rows = _search_every_way(x, w, p)
    if kind == "trained":
        lo, hi = _certificate_bounds(x, w, p)
        print(f"K={K} D={D} rows={rows}: re-scanned {cnt}, must {lo}, may {hi}")
        assert lo <= cnt <= hi, (lo, cnt, hi)
    if kind == "tiny":
        assert cnt == rows


def test_bmu_chunked_coarse_pass_on_near_ties_across_chunks():
    """test_gpu_core.py's constructed near-ties (pairs w, w + s e_j with s swept over 1e-6 ... 3e-3) with the twin
    of code i at i + K/2: every pair straddles two chunks, so the certificate rests on the second-smallest value
    that the cross-chunk merge produces."""
    from qarig import ops
    from oracle import bmu as obmu
    from oracle import ref_models as rm
    g = torch.Generator().manual_seed(321)
    N, C, H, W, p, K = 8, 4, 32, 32, 2, 2048
    D = C * p * p
    base = torch.tanh(torch.randn((K // 2, D), generator=g))
    s = torch.exp(torch.empty(K // 2).uniform_(float(np.log(1e-6)), float(np.log(3e-3)), generator=g))
    s = s * (torch.randint(0, 2, (K // 2,), generator=g) * 2 - 1)
    twin = base.clone()
    twin[torch.arange(K // 2), torch.randint(0, D, (K // 2,), generator=g)] += s
    w = torch.cat((base, twin), 0).contiguous()
    x = torch.tanh(torch.randn((N, C, H, W), generator=g))
    xp = torch.from_numpy(obmu.patchify(x.numpy(), (p, p)).copy())
    near = torch.arange(0, xp.shape[0], 3)           # a third of the patches sit close to a code
    xp[near] = base[torch.randint(0, K // 2, (near.numel(),), generator=g)] + 0.05 * torch.randn((near.numel(), D), generator=g)
    x = rm.unpatchify(xp.reshape(N, -1, D), (H, W), (p, p)).contiguous()
    want = obmu.bmu(x.numpy(), w.numpy(), (p, p))
    for prepared in (False, True):
        got, cnt = ops.bmu_coarse(x.cuda(), w.cuda(), (p, p), prepared=prepared)
        assert np.array_equal(got.cpu().numpy(), want), int((got.cpu().numpy() != want).sum())
        assert 0 < int(cnt.item()) < want.size
    _, gap = obmu.bmu_f64(x.numpy(), w.numpy(), (p, p))
    assert (gap < 1e-7).any() and (gap > 1e-3).any()


def test_bmu_dispatch_takes_the_chunked_form_under_the_option(option):
    """ops.bmu on an nn.Parameter codebook of 8,192 codes: bmu_coarse = 1 forces the chunked form (the second search
    of the unchanged parameter builds its image), bmu_coarse = 0 never takes it; the oracle's indices either way."""
    from qarig import ops
    from oracle import bmu as obmu
    g = torch.Generator().manual_seed(78)
    x = torch.tanh(torch.randn((2, 4, 64, 64), generator=g))            # 8,192 rows
    w = torch.nn.Parameter(torch.tanh(torch.randn((8192, 4), generator=g)).cuda(), requires_grad=False)
    xc = x.cuda()
    want = obmu.bmu(x.numpy(), w.detach().cpu().numpy(), (1, 1))
    ops.bmu_invalidate()
    option("bmu_coarse", 1)
    for call in range(3):
        assert np.array_equal(ops.bmu(xc, w, (1, 1)).cpu().numpy(), want), call
        assert (id(w) in ops._bmu_images) == (call >= 1)
    option("bmu_coarse", 0)
    assert np.array_equal(ops.bmu(xc, w, (1, 1)).cpu().numpy(), want)
    ops.bmu_invalidate()
