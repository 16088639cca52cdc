// SOM topology evaluation, the reductions behind qarig/topology.py (the search itself, qarig_bmu_top2, lives in
// bmu.hip beside the definition of the distance):
//   qarig_topology_rows     per-image fp64 sums of d1, d2, d1^2 and integer histograms of |idx1 - idx2| and d1 / d2;
//   qarig_code_lag_profile  sum_t |w_t - w_{t+r}| for every lag r along the codebook's index axis, fp64.
// Every floating-point sum has one fixed order (a strided chain per thread, the wave butterfly, the four waves in
// order), so an image's sums do not depend on its batch and a lag's sum not on the launch; the histograms are
// integer atomics, exact in any order.
#include "qarig_common.h"

namespace qarig {

__device__ __forceinline__ double topo_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// Block sum of one value per thread (256 threads): the butterfly, then waves 0..3 in order; thread 0's result.
__device__ __forceinline__ double topo_block_sum(double v, double* red) {
    v = topo_wave_sum(v);
    __syncthreads();   // thread 0 has read the previous sum's slots
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// One workgroup per image.  Thread t takes rows t, t + 256, ... of the image in ascending order.  The histograms
// are counted in LDS first (the 32 ratio bins and the first TOPO_GAP_LDS gap bins: a row's two atomics on a
// handful of hot global addresses made the launch 333 us at 65,536 rows) and added to memory once per workgroup.
constexpr int TOPO_GAP_LDS = 8192;
__global__ __launch_bounds__(256) void topology_rows_kernel(const int64_t* __restrict__ idx1,
                                                            const int64_t* __restrict__ idx2,
                                                            const float* __restrict__ d1, const float* __restrict__ d2,
                                                            int seq, int K, double* __restrict__ img_sums,
                                                            unsigned long long* __restrict__ gap_hist,
                                                            unsigned long long* __restrict__ ratio_hist,
                                                            int* __restrict__ bad) {
    __shared__ double red[4];
    extern __shared__ unsigned topo_hist[];      // [32] ratio bins, [min(K, TOPO_GAP_LDS)] gap bins
    const int kl = min(K, TOPO_GAP_LDS);
    for (int i = threadIdx.x; i < 32 + kl; i += 256) topo_hist[i] = 0;
    __syncthreads();
    const int64_t n = blockIdx.x;
    double s1 = 0.0, s2 = 0.0, sq = 0.0;
    for (int i = threadIdx.x; i < seq; i += 256) {
        const int64_t r = n * seq + i;
        const double a = (double)d1[r], b = (double)d2[r];
        s1 += a;
        s2 += b;
        sq += a * a;                          // exact: 24-bit significands
        const int64_t i1 = idx1[r], i2 = idx2[r];
        const int64_t gap = i1 < i2 ? i2 - i1 : i1 - i2;
        if (i1 < 0 || i1 >= K || i2 < 0 || i2 >= K) atomicExch(bad, 1);
        else if (gap < kl) atomicAdd(&topo_hist[32 + gap], 1u);
        else atomicAdd(gap_hist + gap, 1ULL);
        const double q = 32.0 * a / b;        // d2 == 0 (then d1 == 0 too): NaN; d1 == d2: 32; both land in bin 31
        const int bin = q < 31.0 ? (q > 0.0 ? (int)q : 0) : 31;
        atomicAdd(&topo_hist[bin], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 32 + kl; i += 256) {
        const unsigned c = topo_hist[i];
        if (c) atomicAdd(i < 32 ? ratio_hist + i : gap_hist + (i - 32), (unsigned long long)c);
    }
    s1 = topo_block_sum(s1, red);
    s2 = topo_block_sum(s2, red);
    sq = topo_block_sum(sq, red);
    if (threadIdx.x == 0) {
        img_sums[n * 3] = s1;
        img_sums[n * 3 + 1] = s2;
        img_sums[n * 3 + 2] = sq;
    }
}

// One workgroup per lag r = blockIdx.x + 1.  Thread t takes the pairs (t, t + r), (t + 256, t + 256 + r), ...
__global__ __launch_bounds__(256) void code_lag_kernel(const float* __restrict__ w, int K, int D,
                                                       double* __restrict__ lag_sum) {
    __shared__ double red[4];
    const int r = blockIdx.x + 1;
    double s = 0.0;
    for (int t = threadIdx.x; t + r < K; t += 256) {
        const float* a = w + (int64_t)t * D;
        const float* b = a + (int64_t)r * D;
        double acc = 0.0;
        for (int e = 0; e < D; ++e) {
            const double d = (double)a[e] - (double)b[e];
            acc = fma(d, d, acc);
        }
        s += sqrt(acc);
    }
    s = topo_block_sum(s, red);
    if (threadIdx.x == 0) lag_sum[r] = s;
}

}  // namespace qarig

using namespace qarig;

extern "C" int qarig_topology_rows(const int64_t* idx1, const int64_t* idx2, const float* d1, const float* d2, int N,
                                   int seq, int K, double* img_sums, int64_t* gap_hist, int64_t* ratio_hist,
                                   int* bad_flag, void* stream) {
    QARIG_CHECK_ARG(idx1 && idx2 && d1 && d2 && img_sums && gap_hist && ratio_hist && bad_flag,
                    "topology_rows: null pointer");
    QARIG_CHECK_ARG(qarig_dims_ok({N, seq}, 1LL << 24, (1LL << 31) - 1) && K >= 2 && K <= (1 << 24),
                    "topology_rows: need N, seq >= 1, N seq < 2^31, 2 <= K <= 2^24");
    hipLaunchKernelGGL(topology_rows_kernel, dim3((unsigned)N), dim3(256),
                       (32 + (size_t)(K < TOPO_GAP_LDS ? K : TOPO_GAP_LDS)) * 4, (hipStream_t)stream, idx1, idx2, d1, d2,
                       seq, K, img_sums, (unsigned long long*)gap_hist, (unsigned long long*)ratio_hist, bad_flag);
    QARIG_CHECK_LAUNCH("topology_rows");
    return QARIG_OK;
}

extern "C" int qarig_code_lag_profile(const float* codebook, int K, int D, double* lag_sum, void* stream) {
    QARIG_CHECK_ARG(codebook && lag_sum, "code_lag_profile: null pointer");
    QARIG_CHECK_ARG(K >= 2 && qarig_dims_ok({K, D}), "code_lag_profile: need 2 <= K, 1 <= D, at most 2^24 each");
    hipLaunchKernelGGL(code_lag_kernel, dim3((unsigned)(K - 1)), dim3(256), 0, (hipStream_t)stream, codebook, K, D,
                       lag_sum);
    QARIG_CHECK_LAUNCH("code_lag_profile");
    return QARIG_OK;
}
