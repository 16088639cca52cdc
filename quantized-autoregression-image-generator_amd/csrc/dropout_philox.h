// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11) and the
// keep rule of csrc/dropout.hip, in plain C++ for host and device: tests/test_dropout_host.py compiles this
// header for the host alone and checks the known answers and the element layout against the NumPy reference.
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

}  // namespace qarig
