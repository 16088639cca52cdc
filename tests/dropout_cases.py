"""The counter-based dropout mask restated in NumPy (uint64 arithmetic, vectorised over calls), the (T, s) rule and
the case lists shared by tests/test_dropout_host.py, tests/test_gpu_dropout.py and tests/test_gpu_dropout_train.py.

Definition (include/qarig.h qarig_dropout): Philox4x32-10, key (seed_lo, seed_hi), counter (e >> 3, site, step,
rank); element e reads word (e & 7) >> 1 of the call, low 16 bits when e is even, high 16 when odd; kept iff that
value >= T; y = x * s where kept, +0.0 where dropped; T = round(p 65536), s = fp32(65536 / (65536 - T)).

The mutants (keyword arguments of `mask`) are the mistakes the host checks must tell from the definition."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = np.uint64(0xFFFFFFFF)
MAX_T = 58982

# (counter, key, output) -- the known answers of the Random123 distribution's kat_vectors for philox4x32-10
KNOWN_ANSWERS = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def philox4x32(c0, c1, c2, c3, k0, k1, rounds=10):
    """Four uint64 arrays (values < 2^32) per call; counters broadcast against each other."""
    c0, c1, c2, c3 = np.broadcast_arrays(*[np.asarray(c, dtype=np.uint64) for c in (c0, c1, c2, c3)])
    k0, k1 = np.uint64(k0), np.uint64(k1)
    for _ in range(rounds):
        p0 = np.uint64(M0) * c0
        p1 = np.uint64(M1) * c2
        n0 = (p1 >> np.uint64(32)) ^ c1 ^ k0
        n2 = (p0 >> np.uint64(32)) ^ c3 ^ k1
        c0, c1, c2, c3 = n0, p1 & MASK32, n2, p0 & MASK32
        k0 = (k0 + np.uint64(W0)) & MASK32
        k1 = (k1 + np.uint64(W1)) & MASK32
    return c0, c1, c2, c3


def threshold_and_scale(p):
    """(T, s as np.float32), ValueError unless 0 < T <= 58982."""
    p = float(p)
    if not 0.0 < p < 1.0:
        raise ValueError(p)
    t = int(round(p * 65536.0))
    if not 0 < t <= MAX_T:
        raise ValueError(p)
    return t, np.float32(65536.0 / (65536.0 - t))


def values16(n, seed, site, step, rank, rounds=10, swap_halves=False, drop=()):
    """The 16-bit value of each of the elements 0 ... n-1 (uint32 array).  drop: counter words left at 0
    ("site", "step", "rank") -- mutants."""
    calls = (n + 7) // 8
    c = np.arange(calls, dtype=np.uint64)
    words = philox4x32(c, 0 if "site" in drop else site, 0 if "step" in drop else step,
                       0 if "rank" in drop else rank, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF, rounds)
    w = np.stack(words, axis=1)                                  # (calls, 4)
    lo, hi = w & np.uint64(0xFFFF), w >> np.uint64(16)
    if swap_halves:
        lo, hi = hi, lo
    v = np.stack([lo, hi], axis=2).reshape(calls * 8)            # word-major, low half first
    return v[:n].astype(np.uint32)


def mask(n, threshold, seed, site, step, rank, strict=False, **mutant):
    """Boolean keep-mask of n elements.  strict: `>` for `>=` (mutant)."""
    v = values16(n, seed, site, step, rank, **mutant)
    return v > threshold if strict else v >= threshold


def apply(x, threshold, scale, seed, site, step, rank):
    """The expected output for an fp32 array x (any shape; the flat C-order index is the element index)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    keep = mask(x.size, threshold, seed, site, step, rank).reshape(x.shape)
    with np.errstate(all="ignore"):
        y = x * np.float32(scale)
    return np.where(keep, y, np.float32(0.0)).astype(np.float32)


# ---- case lists ----------------------------------------------------------------------------------------------
SEED = 0x5EED
STAT_N = 1 << 20
STAT_PS = (0.1, 0.25, 0.5)
STAT_STREAMS = ((0, 1, 0), (1, 1, 0), (0, 2, 0), (0, 1, 1), (37, 1000, 3))       # (site, step, rank)
SIGMAS = 5.0

GOOD_PS = (0.1, 0.25, 0.5, 0.9)
GOOD_T = {0.1: 6554, 0.25: 16384, 0.5: 32768, 0.9: 58982}
BAD_PS = (0.0, 1e-6, 0.91, 1.0, float("nan"))

# the kernel's sizes: around one call (8), around the 16-byte vector (4), around a wave's and a workgroup's worth of
# calls, and an odd size of several workgroups
KERNEL_NS = (1, 7, 8, 9, 63, 64, 65, 255, 256, 257, 2051)
KERNEL_PS = (0.1, 0.5, 0.9)
KERNEL_STREAMS = ((0, 1, 0), (5, 1, 0), (0, 7, 0), (0, 1, 2), (5, 7, 2))          # two sites, two steps, two ranks
KERNEL_SEED = 0x0123456789ABCDEF                                                    # both key words in use


def special_values(n, rng):
    """fp32 data with +-0, NaN, +-inf, denormals and large magnitudes strewn through it."""
    x = rng.standard_normal(n).astype(np.float32)
    specials = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 1e-45, -1e-45, 1.1754942e-38, -5e-40, 3.0e38, -3.0e38],
                        dtype=np.float32)
    idx = rng.permutation(n)[:min(n, 4 * specials.size)]
    x[idx] = specials[np.arange(idx.size) % specials.size]
    return x
