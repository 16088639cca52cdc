"""The attention-probability dropout mask restated in NumPy and an fp64 reference of the dropped attention, shared by
tests/test_attn_dropout_host.py, tests/test_gpu_attn_dropout.py and tests/test_gpu_attn_dropout_train.py.

Definition (include/qarig.h qarig_attention_dropout_fwd): element (n, h, i, j) -- query i against key j in head h of
sequence n at attention site `site` -- reads the Philox4x32-10 call with key (seed_lo, seed_hi) and counter
((n H + h) Sq + i, 2^31 | site << 23 | j >> 3, step, rank); of its four words key j takes word (j & 7) >> 1, the low
16 bits when j is even and the high 16 when odd, and is kept iff that value >= T.

Reference (P the undropped softmax, M the keep mask, s the fp32 scale the kernel receives):
    o = (M s P) V,  lse that of P,  dS = P (M s dO V^T - delta),  delta = dO . o,  dV = (M s P)^T dO.
The per-row scales are attention_selectors.reference's absolute-sum contractions with the mask inside the sums."""
import math

import numpy as np
import torch

import attention_selectors as A
import dropout_cases as C

HIGH_BIT = 0x80000000
MAX_SITE = 255
MAX_SK = 1 << 26


def _fields(words, j):
    """The 16-bit field of key j (array) from the four word arrays of its call."""
    w = np.choose((j & 7) >> 1, words)
    return np.where(j & 1, w >> np.uint64(16), w & np.uint64(0xFFFF)).astype(np.uint32)


def keep_elements(n, h, i, j, H, Sq, threshold, seed, site, step, rank, swap_ij=False, no_high_bit=False,
                  shift2=False, no_step=False):
    """Keep bits of the listed elements (integer arrays broadcast against each other), one Philox call per element.
    The keyword flags are the mutants tests/test_attn_dropout_host.py must tell from the definition."""
    n, h, i, j = np.broadcast_arrays(*[np.asarray(a, dtype=np.uint64) for a in (n, h, i, j)])
    if swap_ij:
        i, j = j, i
    c0 = ((n * np.uint64(H) + h) * np.uint64(Sq) + i) & C.MASK32
    c1 = np.uint64((0 if no_high_bit else HIGH_BIT) | (site << 23)) | (j >> np.uint64(2 if shift2 else 3))
    words = C.philox4x32(c0, c1, 0 if no_step else step, rank, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    return _fields(words, j.astype(np.int64)) >= threshold


def mask(N, H, Sq, Sk, threshold, seed, site, step, rank):
    """Boolean keep mask (N, H, Sq, Sk), one Philox call per eight keys."""
    groups = (Sk + 7) // 8
    c0 = np.arange(N * H * Sq, dtype=np.uint64).reshape(N, H, Sq, 1) & C.MASK32
    c1 = np.uint64(HIGH_BIT | (site << 23)) | np.arange(groups, dtype=np.uint64)
    words = C.philox4x32(c0, c1, step, rank, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    w = np.stack(words, axis=-1)                                   # (N, H, Sq, groups, 4)
    v = np.stack([w & np.uint64(0xFFFF), w >> np.uint64(16)], axis=-1).reshape(N, H, Sq, groups * 8)
    return v[..., :Sk] >= np.uint64(threshold)


def reference(q, k, v, do, causal, keep, scale):
    """attention_selectors.reference with the keep mask (bool, (N,H,Sq,Sk)) and the scale s: (ref, row scales)."""
    d = q.shape[-1]
    Sq, Sk = q.shape[2], k.shape[2]
    rs = 1.0 / math.sqrt(d)
    s = q @ k.transpose(-1, -2) * rs
    if causal:
        s = s.masked_fill(A._mask(Sq, Sk), float("-inf"))
    lse = torch.logsumexp(s, -1)
    P = torch.exp(s - lse[..., None])
    Ms = torch.as_tensor(keep).double() * float(scale)
    Pd = P * Ms
    o = Pd @ v
    dP = do @ v.transpose(-1, -2)
    delta = (do * o).sum(-1, keepdim=True)
    dS = P * (Ms * dP - delta)
    ref = {"o": o, "lse": lse, "dq": dS @ k * rs, "dk": dS.transpose(-1, -2) @ q * rs, "dv": Pd.transpose(-1, -2) @ do}
    oa = Pd @ v.abs()
    dSa = P * (Ms * (do.abs() @ v.abs().transpose(-1, -2)) + (do.abs() * oa).sum(-1, keepdim=True))
    scl = {"o": oa, "dq": dSa @ k.abs() * rs, "dk": dSa.transpose(-1, -2) @ q.abs() * rs,
           "dv": Pd.transpose(-1, -2) @ do.abs()}
    return ref, {name: t.amax(-1) for name, t in scl.items()}


SEED = 0x0123456789ABCDEF           # both key words in use
STREAMS = ((0, 1, 0), (5, 1, 0), (0, 7, 0), (0, 1, 2), (255, 7, 2))         # (site, step, rank)
READOUT_SHAPES = ((2, 5, 8, 70, 128), (2, 3, 4, 65, 64), (1, 2, 64, 9, 256), (1, 6, 16, 130, 256))   # N, H, d, Sq, Sk
GAUSSIAN_SHAPES = ((70, 70, True, 3, 4), (130, 130, True, 5, 8), (200, 200, False, 6, 8), (65, 257, False, 3, 8),
                   (129, 129, True, 3, 16), (65, 65, True, 2, 32), (17, 17, True, 1, 64))       # Sq, Sk, causal, H, d
