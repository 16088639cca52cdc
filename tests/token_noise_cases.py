"""The token-noise rule restated in NumPy on top of tests/dropout_cases.philox4x32, and the case tables shared by
tests/test_token_noise_host.py, tests/test_gpu_token_noise.py and tests/test_gpu_token_noise_train.py.

Definition (include/qarig.h qarig_token_noise): token j of the full, un-windowed stream (S tokens) of sample n makes
one Philox4x32-10 call, key (seed_lo, seed_hi), counter (n S + j, 2^30 | stream, step, rank); with out[4] its result
the token is unchanged iff (out[0] & 0xffff) >= T, and otherwise becomes lo + (out[1] span >> 32), where R = 0 gives
lo = 0, span = K and R > 0 gives lo = max(0, id - R), hi = min(K - 1, id + R), span = hi - lo + 1.  An id outside
[0, K) passes through.  Stream 0: the decoder's hr tokens (j the index into hr); stream 1: the encoder's lr tokens.

The mutants (keyword arguments of `noise`) are the mistakes the host checks must tell from the definition."""
import numpy as np

import dropout_cases as C

DOMAIN = 0x40000000
MAX_T = C.MAX_T


def noise(ids, K, T, R, seed, stream, step, rank, index=None, no_clamp=False, modulo=False, decide_from_1=False):
    """ids: int64 (N,S), the whole stream.  index: the (N,S) array used as the counter's token index in place of
    the absolute n S + j (the `window index` mutant passes a window-relative one).  Returns the corrupted ids."""
    ids = np.asarray(ids, dtype=np.int64)
    N, S = ids.shape
    c0 = (np.arange(N, dtype=np.uint64)[:, None] * np.uint64(S) + np.arange(S, dtype=np.uint64)[None, :]
          if index is None else np.asarray(index, dtype=np.uint64))
    o0, o1, _, _ = C.philox4x32(c0 & C.MASK32, DOMAIN | stream, step, rank, seed & 0xFFFFFFFF,
                                (seed >> 32) & 0xFFFFFFFF)
    decide = o1 if decide_from_1 else o0
    replace = (decide & np.uint64(0xFFFF)) < np.uint64(T)
    if R > 0:
        lo, hi = ids - R, ids + R
        if not no_clamp:
            lo, hi = np.maximum(lo, 0), np.minimum(hi, K - 1)
    else:
        lo, hi = np.zeros_like(ids), np.full_like(ids, K - 1)
    span = (hi - lo + 1).astype(np.uint64)
    draw = (o1 % np.maximum(span, np.uint64(1))) if modulo else ((o1 * span) >> np.uint64(32))
    new = lo + draw.astype(np.int64)
    inside = (ids >= 0) & (ids < K)
    return np.where(replace & inside, new, ids)


def assemble(lr, hr, base, k_lr, k_hr, offs, W, noisy_hr=None):
    """(hr_in, hr_tg, pos) of qarig_assemble_tokens in NumPy; noisy_hr: the hr tokens the decoder input reads (the
    targets always read hr).  offs None: the whole sequence, W ignored."""
    hr = np.asarray(hr, dtype=np.int64)
    N, S_hr = hr.shape
    src = hr if noisy_hr is None else noisy_hr
    if base:
        full_in = np.concatenate([np.asarray(lr, dtype=np.int64), src + k_lr], axis=1)
    else:
        full_in = np.concatenate([np.full((N, 1), k_hr, dtype=np.int64), src], axis=1)
    s_in = full_in.shape[1]
    full_tg = np.concatenate([hr, np.full((N, s_in - S_hr), k_hr, dtype=np.int64)], axis=1)
    if offs is None:
        return full_in, full_tg, None
    pos = np.asarray(offs, dtype=np.int64)[:, None] + np.arange(W, dtype=np.int64)[None, :]
    return np.take_along_axis(full_in, pos, 1), np.take_along_axis(full_tg, pos, 1), pos


def tokens(N, S, K, rng):
    """Random ids with 0 and K - 1 planted in every row, so that both clamps fire wherever R > 0."""
    ids = rng.integers(0, K, (N, S)).astype(np.int64)
    ids[:, 0] = 0
    ids[:, -1] = K - 1
    if S > 4:
        ids[:, 2] = K - 1
        ids[:, 3] = 0
    return ids


# ---- case tables -------------------------------------------------------------------------------------------------
SEED = 0x0123456789ABCDEF           # both key words in use
N, S_HR = 3, 37
S_LRS = (1, 4)
KS = (5, 513, 8192)
RS = (0, 1, 7)
TS = (1, 32768, 58982)
STREAMS = ((0, 1, 0), (1, 1, 0), (0, 2, 0), (0, 1, 1))      # (stream, step, rank): two steps, two ranks
# (K, R, T, stream, step, rank) of the host comparison: every K x R at T = 32768, every T at (513, 1), every stream
HOST_CASES = [(K, R, 32768, 0, 7, 2) for K in KS for R in RS] + [(513, 1, T, 1, 3, 0) for T in TS] + \
             [(513, 7, 58982, s, st, rk) for s, st, rk in STREAMS]
STAT_N = 1 << 16
STAT_TS = (6554, 32768, 58982)
STAT_STREAMS = ((0, 1, 0), (1, 5, 0), (0, 1000, 3))        # (stream, step, rank)
SIGMAS = 5.0
