"""qarig_pool_features / qarig_moments_add and FeatureMoments on the GPU against the longdouble references and derived
tolerances of tests/gen_eval_cases.py -- the same check families that tests/test_gen_eval_host.py shows to reject a
wrong lane map, a dropped shift, a dropped partial tile, ... on a NumPy emulation.  Integer inputs bit for bit."""
import numpy as np
import pytest
import torch

import gen_eval_cases as G
from qarig import _lib, gen_eval, ops

pytestmark = pytest.mark.gpu


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


class GpuBackend:
    def moments(self, batches, shift, D, gram_init=None):
        count = torch.zeros(1, dtype=torch.int64, device="cuda")
        total = torch.zeros(D, dtype=torch.float64, device="cuda")
        gram = torch.zeros((D, D), dtype=torch.float64, device="cuda") if gram_init is None else _dev(gram_init)
        sh = None if shift is None else _dev(shift)
        for f in batches:
            ops.moments_add(_dev(f), (count, total, gram), sh)
        return int(count.item()), total.cpu().numpy(), gram.cpu().numpy()

    def pool(self, z, P):
        return ops.pool_features(_dev(z), P).cpu().numpy()

    def feature_moments(self, dim, shift):
        return gen_eval.FeatureMoments(dim, None if shift is None else _dev(shift))


@pytest.mark.parametrize("dim", G.DIMS)
def test_moments_add_per_element(dim):
    worst = G.family_elements(GpuBackend(), dim)
    print(f"moments_add D = {dim}: worst fraction of the bound {worst:.3f}")


def test_moments_add_at_the_largest_dim():
    n, D = G.BIG
    worst = G.family_elements(GpuBackend(), D, rows=(n,))
    print(f"moments_add D = {D}, n = {n}: worst fraction of the bound {worst:.3f}")


def test_accumulation_and_determinism():
    worst = G.family_accumulate(GpuBackend())
    print(f"three calls against one: worst fraction of the bound {worst:.3f}")


def test_untouched_accumulator_elements():
    G.family_untouched(GpuBackend())


def test_pool_features():
    worst = G.family_pool(GpuBackend())
    print(f"pool_features: worst fraction of the bound {worst:.3f}")


def test_feature_moments_mean_and_cov():
    worst = G.family_feature_moments(GpuBackend(), _dev)
    print(f"FeatureMoments mean / cov: worst fraction of the derived tolerance {worst:.3f}")
    with pytest.raises(ValueError):
        m = gen_eval.FeatureMoments(4)
        m.add(torch.zeros((1, 4), dtype=torch.float64, device="cuda"))
        m.result()                                                     # n = 1


def test_a_nan_feature_stays_in_its_row_and_column():
    f = G.features("int", 6, 33, seed=61)
    f[2, 20] = np.nan
    _, total, gram = GpuBackend().moments([f], None, 33)
    hit = np.zeros((33, 33), bool)
    hit[20, :] = hit[:, 20] = True
    keep = G.maintained(33)
    assert np.isnan(gram[keep & hit]).all() and not np.isnan(gram[keep & ~hit]).any()
    assert np.isnan(total[20]) and not np.isnan(np.delete(total, 20)).any()


def test_refusals():
    z = torch.zeros(1, 2, 4, 4)
    with pytest.raises(RuntimeError):
        ops.pool_features(z, 2)
    with pytest.raises(RuntimeError):
        gen_eval.FeatureMoments(4).add(torch.zeros(3, 4, dtype=torch.float64))
    with pytest.raises(RuntimeError):
        ops.pool_features(z.cuda(), 3)
    assert "pool" in _lib.last_error()
    with pytest.raises(RuntimeError):
        ops.pool_features(torch.zeros(1, 5, 16, 16, device="cuda"), 1)                # D = 1280
    assert "1280" in _lib.last_error()
    f = torch.zeros((4, 8), dtype=torch.float64, device="cuda")
    with pytest.raises(RuntimeError):                                                 # the sum aliases the features
        ops.moments_add(f, (torch.zeros(1, dtype=torch.int64, device="cuda"), f[0],
                            torch.zeros((8, 8), dtype=torch.float64, device="cuda")))
    assert "alias" in _lib.last_error()
    torch.cuda.synchronize()
