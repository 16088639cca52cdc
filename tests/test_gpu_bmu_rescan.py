"""The literal re-scan behind every BMU search form, reached through 1-ulp twins.

Every form (resident, small, mma, coarse, chunked coarse and the two finalize kernels) scans t = -2 x.w + |w|^2 and
hands the rows whose minimum another candidate may tie with to ONE routine that restates the definition
(csrc/bmu.hip bmu_rescan).  Exact duplicates do not test that routine: their t is identical, so bmu_merge already
picks the lower index.  Here code 2i+1 is code 2i with one element moved by one ulp: the two t differ, the two
d = sqrtf(max(t + |x|^2, 0)) mostly do not, and in the rows counted as `overridden` below the NEARER code (fp64) is
the higher index, which loses to the rounding of t + |x|^2 / sqrt plus the first-index rule.  A scan over t alone
answers those rows wrong; only the re-scan answers them as oracle/bmu_oracle.c does.

Prepared image of the K = 96, D = 16 codebook below (qarig_bmu_prepare: 96 x 100 B of planes and |w|^2, then max |w|^2
and the inexact flag; the header's last 8 bytes are padding and left out), SHA-256, recorded on an MI355X from the
library of commit 570c3f4 (the parent of the commit that made the two prepare kernels one):
    fa2b9acbbad57188c27a416e95ba46eb9f97d4f8c8c091dbdf503ef3ad40d635"""
import functools
import hashlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

IMAGE_SHA256 = "fa2b9acbbad57188c27a416e95ba46eb9f97d4f8c8c091dbdf503ef3ad40d635"


@pytest.fixture
def option():
    from qarig import _lib
    saved = []

    def set_(name, value):
        saved.append((name, _lib.set_option(name, value)))

    yield set_
    for name, old in reversed(saved):
        _lib.set_option(name, old)


@functools.lru_cache(maxsize=None)
def _twins(N, C, H, W, p, K):
    """(x, w, oracle indices) of the construction, its precondition asserted on the CPU: in at least a quarter of
    the rows the oracle returns the lower index of a twin pair while fp64 returns the higher."""
    from oracle import bmu as obmu
    rng = np.random.default_rng(5)
    D = C * p * p
    base = np.tanh(rng.standard_normal((K // 2, D))).astype(np.float32)
    twin = base.copy()
    e = rng.integers(0, D, K // 2)
    up = rng.integers(0, 2, K // 2) == 1
    at = (np.arange(K // 2), e)
    twin[at] = np.nextafter(base[at], np.where(up, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32))
    assert (twin != base).sum() == K // 2
    w = np.stack((base, twin), 1).reshape(K, D)
    x = np.tanh(rng.standard_normal((N, C, H, W))).astype(np.float32)
    want = obmu.bmu(x, w, (p, p))
    near, _ = obmu.bmu_f64(x, w, (p, p))
    overridden = int(((want % 2 == 0) & (near == want + 1)).sum())
    print(f"{(N, C, H, W, p, K)}: {overridden} of {want.size} rows overridden")
    assert 4 * overridden >= want.size, (overridden, want.size)
    want.setflags(write=False)
    return torch.from_numpy(x), torch.from_numpy(w), want


def _check_bmu(case):
    from qarig import ops
    x, w, want = _twins(*case)
    p = case[4]
    got = ops.bmu(x.cuda(), w.cuda(), (p, p)).cpu().numpy()
    assert np.array_equal(got, want), int((got != want).sum())


@pytest.mark.parametrize("case", [
    (2, 3, 16, 16, 1, 96),       # D = 3: resident, scalar staging
    (2, 4, 16, 16, 1, 96),       # D = 4
    (2, 2, 16, 16, 2, 96),       # D = 8
    (2, 3, 16, 16, 2, 96),       # D = 12
    (2, 4, 16, 16, 2, 832),      # resident, two chunks -> bmu_finalize_kernel
    (2, 4, 16, 16, 1, 3072),     # the same at D = 4
    (2, 2, 32, 32, 4, 96),       # D = 32: bmu_small_kernel, one split
    (2, 2, 32, 32, 4, 320),      # ... three splits -> bmu_finalize_kernel
    (2, 4, 32, 32, 4, 96),       # D = 64
    (2, 8, 32, 32, 4, 96),       # D = 128: bmu_mma_kernel, one split
    (2, 8, 32, 32, 4, 320),      # ... three
])
def test_bmu_exact_forms_on_one_ulp_twins(option, case):
    option("bmu_coarse", 0)
    _check_bmu(case)


@pytest.mark.parametrize("groups", [0, 1])
@pytest.mark.parametrize("cs", [1, 2, 4])
def test_bmu_resident_single_chunk_on_one_ulp_twins(option, cs, groups):
    """D = 16, one chunk: the re-scan reads the codes back from the resident kernel's LDS fragments."""
    option("bmu_coarse", 0)
    option("bmu_cs", cs)
    option("bmu_groups", groups)
    _check_bmu((2, 4, 16, 16, 2, 96))


@pytest.mark.parametrize("prepared", [False, True])
@pytest.mark.parametrize("K", [96, 2048])
def test_bmu_coarse_forms_on_one_ulp_twins(K, prepared):
    """Single-image (K = 96) and chunked (K = 2048) coarse pass: a 1-ulp twin can never be certified, so every row
    takes the re-scan; the prepared image of the K = 96 codebook has the recorded bytes."""
    from qarig import ops
    x, w, want = _twins(2, 4, 16, 16, 2, K)
    wc = w.cuda()
    got, cnt = ops.bmu_coarse(x.cuda(), wc, (2, 2), prepared=prepared)
    got = got.cpu().numpy()
    assert np.array_equal(got, want), int((got != want).sum())
    assert int(cnt.item()) == want.size
    if prepared and K == 96:
        img = ops.bmu_image(wc).cpu().numpy().tobytes()
        assert len(img) == K * 100 + 16
        digest = hashlib.sha256(img[:K * 100 + 8]).hexdigest()
        print("image sha256", digest)
        assert digest == IMAGE_SHA256
