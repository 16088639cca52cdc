// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11) and the
// keep rule of csrc/dropout.hip, in plain C++ for host and device: tests/test_dropout_host.py compiles this
// header for the host alone and checks the known answers and the element layout against the NumPy reference.
// The attention-probability counters and keep rule of csrc/attention.hip follow the same way
// (tests/test_attn_dropout_host.py).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define QARIG_HD __host__ __device__
#else
#define QARIG_HD
#endif

#define QARIG_DROPOUT_MAX_THRESHOLD 58982u   // round(0.9 * 65536)
#define QARIG_DROPOUT_BLOCK 256              // threads per workgroup, eight elements per thread-iteration
#define QARIG_DROPOUT_MAX_BLOCKS 8192        // grid cap: larger launches wrap the grid-stride loop
#define QARIG_ATTN_DROPOUT_SITES 256u        // attention sites 0 ... 255: eight bits of the second counter word
#define QARIG_ATTN_DROPOUT_MAX_SK (1 << 26)  // key index >> 3 fits the 23 bits below the site

namespace qarig {

QARIG_HD inline void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                   uint32_t out[4]) {
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;       // (the bump after the tenth round is dead code the compiler drops)
        k1 += 0xBB67AE85u;
    }
    out[0] = c0;
    out[1] = c1;
    out[2] = c2;
    out[3] = c3;
}

// Element j (0 ... 7, or 0 ... 3 within either half) of a call whose word `w` = out[j >> 1] it reads: the low
// 16 bits when j is even, the high 16 when odd; kept iff that value >= threshold.
QARIG_HD inline bool dropout_value(uint32_t w, int j, uint32_t threshold) {
    return ((j & 1) ? (w >> 16) : (w & 0xffffu)) >= threshold;
}

// ---- attention-probability dropout --------------------------------------------------------------------------
// Element (n, h, i, j) = query i against key j in head h of sequence n, at attention site `site`: the call
// philox4x32_10(c0, c1, step, rank, seed_lo, seed_hi) with c0 = (n H + h) Sq + i and c1 = 2^31 | site << 23 | j >> 3
// serves the eight keys j & ~7 ... j | 7 of one query, 16 bits each by the rule above.  The set high bit of c1
// keeps these counters apart from those of csrc/dropout.hip, whose second word is a small site ordinal.
QARIG_HD inline uint32_t attn_dropout_c0(uint32_t n, uint32_t H, uint32_t h, uint32_t Sq, uint32_t i) {
    return (n * H + h) * Sq + i;
}
QARIG_HD inline uint32_t attn_dropout_c1(uint32_t site, uint32_t j) {
    return 0x80000000u | (site << 23) | (j >> 3);
}
// The keep bits of the eight keys of one call: bit b = key (j & ~7) + b.
QARIG_HD inline uint32_t attn_dropout_keep8(const uint32_t out[4], uint32_t threshold) {
    uint32_t m = 0;
#pragma unroll
    for (int b = 0; b < 8; ++b) m |= (uint32_t)dropout_value(out[b >> 1], b, threshold) << b;
    return m;
}
QARIG_HD inline bool attn_dropout_keep(uint32_t n, uint32_t H, uint32_t h, uint32_t Sq, uint32_t i, uint32_t j,
                                       uint32_t site, uint32_t threshold, uint32_t step, uint32_t rank,
                                       uint32_t seed_lo, uint32_t seed_hi) {
    uint32_t out[4];
    philox4x32_10(attn_dropout_c0(n, H, h, Sq, i), attn_dropout_c1(site, j), step, rank, seed_lo, seed_hi, out);
    return dropout_value(out[(j & 7) >> 1], (int)(j & 7), threshold);
}

// ---- token noise --------------------------------------------------------------------------------
// Token j of the full, un-windowed stream (S tokens) of sample n: one call philox4x32_10(c0, c1, step, rank,
// seed_lo, seed_hi) with c0 = n S + j and c1 = 2^30 | stream (0: the decoder's hr tokens, j the index into hr;
// 1: the encoder's lr tokens).  Bit 30 set and bit 31 clear keeps these counters apart from the other two
// domains under the same key: the second word of a model's residual dropout is a site ordinal below 2 + (number
// of residual layers), a few hundred at most (models.Transformer.enable_dropout refuses one at or past 2^30; the
// bare qarig_dropout entry takes any 32-bit site), and the attention domain above sets bit 31.
// The token is unchanged iff (out[0] & 0xffff) >= threshold -- the sense of dropout_value, replace rate
// threshold / 65536 -- and otherwise becomes lo + ((uint64)out[1] span >> 32), where range == 0 draws from the
// whole codebook (lo = 0, span = K) and range > 0 from the SOM neighbourhood [max(0, id - range),
// min(K - 1, id + range)], clamped at the ends of the axis.  The draw may return id itself: the effective change
// rate is threshold / 65536 (1 - 1 / span).  An id outside [0, K) passes through (the embedding kernel flags it).
#define QARIG_TOKEN_NOISE_DOMAIN 0x40000000u
#define QARIG_TOKEN_NOISE_STREAMS 2u         // 0: decoder input (hr), 1: encoder input (lr)

QARIG_HD inline uint32_t token_noise_c1(uint32_t stream) { return QARIG_TOKEN_NOISE_DOMAIN | stream; }
QARIG_HD inline int64_t token_noise_id(int64_t id, uint32_t c0, uint32_t stream, int K, uint32_t threshold, int range,
                                       uint32_t step, uint32_t rank, uint32_t seed_lo, uint32_t seed_hi) {
    if (id < 0 || id >= K) return id;
    uint32_t out[4];
    philox4x32_10(c0, token_noise_c1(stream), step, rank, seed_lo, seed_hi, out);
    if (dropout_value(out[0], 0, threshold)) return id;
    int64_t lo = 0, span = K;
    if (range > 0) {
        lo = id - range > 0 ? id - range : 0;
        const int64_t hi = id + range < K - 1 ? id + range : K - 1;
        span = hi - lo + 1;
    }
    return lo + (int64_t)(((uint64_t)out[1] * (uint64_t)span) >> 32);
}

}  // namespace qarig
