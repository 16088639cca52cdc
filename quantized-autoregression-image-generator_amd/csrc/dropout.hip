// Counter-based dropout: y[e] = keep(e) ? x[e] * scale : +0, where keep(e) is a pure function of
// (seed, rank, step, site, e) -- no generator state and no stored mask, so backward, checkpoint recomputation
// and a replayed graph regenerate the forward mask by construction.
//
// Philox4x32-10, key (seed_lo, seed_hi), counter (e >> 3, site, step, rank): one call serves eight consecutive
// elements, 16 bits each -- element e takes word (e & 7) >> 1 of the call, low half when e is even, high half
// when odd -- and is kept iff that value >= threshold (drop rate threshold / 65536).
#include "dropout_philox.h"
#include "qarig_common.h"

namespace qarig {

// One thread-iteration = one Philox call = eight elements = 32 bytes each way.  VEC: x and y are both 16-byte
// aligned, full groups move as two 16-byte loads and two 16-byte stores; the last (partial) group, and every
// group of an unaligned launch, moves element by element.  The mask is a function of the element index alone:
// both paths take it from the same call.
template <bool VEC>
__global__ void dropout_kernel(const float* x, float* y, int64_t n, uint32_t threshold, float scale,
                               uint32_t site, const uint32_t* __restrict__ key) {
    const uint32_t k0 = key[0], k1 = key[1], step = key[2], rank = key[3];
    const int64_t groups = (n + 7) >> 3;
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < groups;
         c += (int64_t)gridDim.x * blockDim.x) {
        uint32_t r[4];
        philox4x32_10((uint32_t)c, site, step, rank, k0, k1, r);
        const int64_t e0 = c << 3;
        if (VEC && e0 + 8 <= n) {
            const f32x4 a = *(const f32x4*)(x + e0);
            const f32x4 b = *(const f32x4*)(x + e0 + 4);
            f32x4 ya, yb;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                ya[j] = dropout_value(r[j >> 1], j, threshold) ? a[j] * scale : 0.0f;
                yb[j] = dropout_value(r[2 + (j >> 1)], j, threshold) ? b[j] * scale : 0.0f;
            }
            *(f32x4*)(y + e0) = ya;
            *(f32x4*)(y + e0 + 4) = yb;
        } else {
            const int m = n - e0 < 8 ? (int)(n - e0) : 8;
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (j < m) v[j] = x[e0 + j];
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (j < m) y[e0 + j] = dropout_value(r[j >> 1], j, threshold) ? v[j] * scale : 0.0f;
        }
    }
}

}  // namespace qarig

using namespace qarig;

// y = dropout(x): n fp32 elements, threshold in [1, 58982] (p <= 0.9), scale = 65536 / (65536 - threshold)
// rounded to fp32 by the host, site the call site's ordinal.  key: DEVICE uint32[4] {seed_lo, seed_hi, step,
// rank}, read by the kernel in eager and captured launches alike.  y may be x itself; any other overlap is
// refused.  n <= 2^34: the call index e >> 3 is one 32-bit counter word.
extern "C" int qarig_dropout(const float* x, float* y, int64_t n, uint32_t threshold, float scale,
                             uint32_t site, const uint32_t* key, void* stream) {
    QARIG_CHECK_ARG(x && y && key, "dropout: null pointer");
    QARIG_CHECK_ARG(n > 0 && n <= (1LL << 34), "dropout: n must lie in [1, 2^34]");
    QARIG_CHECK_ARG(threshold >= 1 && threshold <= QARIG_DROPOUT_MAX_THRESHOLD,
                    "dropout: threshold must lie in [1, 58982] (0 < p <= 0.9)");
    const uintptr_t ux = (uintptr_t)x, uy = (uintptr_t)y;
    QARIG_CHECK_ARG(ux % 4 == 0 && uy % 4 == 0, "dropout: buffers must be 4-byte aligned");
    QARIG_CHECK_ARG(ux == uy || ux + 4 * (uint64_t)n <= uy || uy + 4 * (uint64_t)n <= ux,
                    "dropout: x and y overlap without being the same buffer");
    const int64_t groups = (n + 7) >> 3;
    int64_t blocks = (groups + QARIG_DROPOUT_BLOCK - 1) / QARIG_DROPOUT_BLOCK;
    if (blocks > QARIG_DROPOUT_MAX_BLOCKS) blocks = QARIG_DROPOUT_MAX_BLOCKS;
    if (ux % 16 == 0 && uy % 16 == 0)
        hipLaunchKernelGGL(dropout_kernel<true>, dim3((int)blocks), dim3(QARIG_DROPOUT_BLOCK), 0,
                           (hipStream_t)stream, x, y, n, threshold, scale, site, key);
    else
        hipLaunchKernelGGL(dropout_kernel<false>, dim3((int)blocks), dim3(QARIG_DROPOUT_BLOCK), 0,
                           (hipStream_t)stream, x, y, n, threshold, scale, site, key);
    QARIG_CHECK_LAUNCH("dropout");
    return QARIG_OK;
}
