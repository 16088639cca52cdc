// Generation evaluation: pooled fp64 features of a latent batch (pool_features_kernel) and their first and second
// moments, added into fp64 accumulators that stay on the device for a whole sample set (moments_add_kernel).  The
// Gram products run on v_mfma_f64_16x16x4_f64; every output element belongs to one wave (one lane for the sums),
// the rows are visited in ascending order and nothing is added atomically, so equal inputs and an equal call
// sequence give equal bits.
#include "qarig_common.h"

namespace qarig {

typedef double f64x4 __attribute__((ext_vector_type(4)));

// One thread per feature (n, c, i, j): the P x P block in raster order, fp64, one division.
__global__ __launch_bounds__(256) void pool_features_kernel(const float* __restrict__ z, int64_t total, int C, int H,
                                                            int W, int P, double* __restrict__ f) {
    const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (o >= total) return;
    const int ow = W / P, oh = H / P;
    const int j = (int)(o % ow);
    const int i = (int)((o / ow) % oh);
    const int64_t nc = o / ((int64_t)ow * oh);                  // n C + c
    const float* src = z + (nc * H + (int64_t)i * P) * W + (int64_t)j * P;
    double s = 0.0;
    for (int y = 0; y < P; ++y)
        for (int x = 0; x < P; ++x) s += (double)src[(int64_t)y * W + x];
    f[o] = s / (double)(P * P);
}

constexpr int MOM_TILE = 16;      // the MFMA's output tile
constexpr int MOM_GROUP = 4;      // tiles of one tile row that a wave owns: one A fragment feeds four products
constexpr int MOM_DEPTH = 2;      // MFMA steps (of four rows) whose fragments are loaded together
constexpr int MOM_SUM_ROWS = 16;  // rows of a column whose loads a `sum` lane keeps in flight

// groups of tile row ti among T tile columns: the tiles ti ... T - 1, four to a wave
__host__ __device__ __forceinline__ int mom_row_groups(int T, int ti) { return (T - ti + MOM_GROUP - 1) / MOM_GROUP; }

// a_r = f_r - shift for row r, column c; exactly zero outside the (n, D) extent (after the subtraction: a padded row
// must not contribute -shift).
__device__ __forceinline__ double mom_load(const double* __restrict__ f, const double* __restrict__ shift, int n, int D,
                                           int r, int c) {
    if (r >= n || c >= D) return 0.0;
    const double v = f[(int64_t)r * D + c];
    return shift ? v - shift[c] : v;
}

// Waves 0 ... G - 1 own the Gram tiles (tile row ti, tile columns tj0 ... tj0 + 3, tj0 >= ti); waves G ... own 64
// columns of `sum` each, a column per lane; the first of those also owns `count`.
// Fragments of v_mfma_f64_16x16x4_f64: A[i = lane & 15][k = lane >> 4], B[k = lane >> 4][j = lane & 15], one double
// per lane; C/D register q of a lane is (row (lane >> 4) + 4 q, column lane & 15) -- NOT the f32 16x16x4 map.
__global__ __launch_bounds__(256) void moments_add_kernel(const double* __restrict__ f, int n, int D,
                                                          const double* __restrict__ shift, int gram_waves,
                                                          int64_t* __restrict__ count, double* __restrict__ sum,
                                                          double* __restrict__ gram) {
    const int lane = threadIdx.x & 63;
    int w = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    const int T = (D + MOM_TILE - 1) / MOM_TILE;
    if (w >= gram_waves) {
        const int c = (w - gram_waves) * 64 + lane;
        if (w == gram_waves && lane == 0) count[0] += n;
        if (c >= D) return;
        const double sh = shift ? shift[c] : 0.0;
        double s = sum[c];
        int r = 0;
        for (; r + MOM_SUM_ROWS <= n; r += MOM_SUM_ROWS) {          // the loads of a batch in flight together,
            double v[MOM_SUM_ROWS];                                 // the additions in row order all the same
#pragma unroll
            for (int j = 0; j < MOM_SUM_ROWS; ++j) v[j] = f[(int64_t)(r + j) * D + c];
#pragma unroll
            for (int j = 0; j < MOM_SUM_ROWS; ++j) s += v[j] - sh;
        }
        for (; r < n; ++r) s += f[(int64_t)r * D + c] - sh;
        sum[c] = s;
        return;
    }
    int ti = 0;
    for (int g = mom_row_groups(T, 0); w >= g; g = mom_row_groups(T, ti)) {      // wave-uniform, at most 64 trips
        w -= g;
        ++ti;
    }
    const int i0 = ti * MOM_TILE;
    const int j0 = (ti + w * MOM_GROUP) * MOM_TILE;
    const int x = lane & 15, h = lane >> 4;

    f64x4 acc[MOM_GROUP];
#pragma unroll
    for (int t = 0; t < MOM_GROUP; ++t)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int row = i0 + h + 4 * q, col = j0 + t * MOM_TILE + x;
            acc[t][q] = (row < D && col < D) ? gram[(int64_t)row * D + col] : 0.0;
        }

    // rows in ascending steps of four; the fragments of the next MOM_DEPTH steps are in flight while this batch's
    // products issue (rows past n load as zeros, so the last batch may overshoot)
    double a[MOM_DEPTH], b[MOM_DEPTH][MOM_GROUP];
#pragma unroll
    for (int d = 0; d < MOM_DEPTH; ++d) {
        a[d] = mom_load(f, shift, n, D, 4 * d + h, i0 + x);
#pragma unroll
        for (int t = 0; t < MOM_GROUP; ++t) b[d][t] = mom_load(f, shift, n, D, 4 * d + h, j0 + t * MOM_TILE + x);
    }
    for (int r0 = 0; r0 < n; r0 += 4 * MOM_DEPTH) {
        double na[MOM_DEPTH], nb[MOM_DEPTH][MOM_GROUP];
#pragma unroll
        for (int d = 0; d < MOM_DEPTH; ++d) {
            const int rn = r0 + 4 * (MOM_DEPTH + d) + h;
            na[d] = mom_load(f, shift, n, D, rn, i0 + x);
#pragma unroll
            for (int t = 0; t < MOM_GROUP; ++t) nb[d][t] = mom_load(f, shift, n, D, rn, j0 + t * MOM_TILE + x);
        }
#pragma unroll
        for (int d = 0; d < MOM_DEPTH; ++d)
#pragma unroll
            for (int t = 0; t < MOM_GROUP; ++t)
                acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[d], b[d][t], acc[t], 0, 0, 0);
#pragma unroll
        for (int d = 0; d < MOM_DEPTH; ++d) {
            a[d] = na[d];
#pragma unroll
            for (int t = 0; t < MOM_GROUP; ++t) b[d][t] = nb[d][t];
        }
    }

#pragma unroll
    for (int t = 0; t < MOM_GROUP; ++t)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int row = i0 + h + 4 * q, col = j0 + t * MOM_TILE + x;
            if (row < D && col < D) gram[(int64_t)row * D + col] = acc[t][q];
        }
}

static inline bool mom_overlap(const void* p, size_t pb, const void* q, size_t qb) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a < b + qb && b < a + pb;
}

}  // namespace qarig

using namespace qarig;

// z (N,C,H,W) fp32 contiguous -> f (N, D) fp64, D = C (H/P) (W/P), feature (c, i, j) = the mean of its P x P block.
extern "C" int qarig_pool_features(const float* z, int N, int C, int H, int W, int P, double* f, void* stream) {
    QARIG_CHECK_ARG(z && f, "pool_features: null pointer");
    QARIG_CHECK_DIMS("pool_features", N, C, H, W);
    QARIG_CHECK_ARG(P >= 1 && P <= H && P <= W && H % P == 0 && W % P == 0,
                    "pool_features: the pool %d must divide the latent's %d x %d", P, H, W);
    const int64_t D = (int64_t)C * (H / P) * (W / P);
    QARIG_CHECK_ARG(D >= 1 && D <= 1024, "pool_features: %lld features per sample, at most 1024 are supported "
                    "(use a larger pool)", (long long)D);
    const int64_t total = (int64_t)N * D;                      // <= 2^34
    QARIG_CHECK_ARG(!mom_overlap(z, (size_t)N * C * H * W * 4, f, (size_t)total * 8),
                    "pool_features: the features alias the latents");
    hipLaunchKernelGGL(pool_features_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       z, total, C, H, W, P, f);
    QARIG_CHECK_LAUNCH("pool_features");
    return QARIG_OK;
}

// f (n, D) fp64, ld = D; shift (D) fp64 or NULL.  ADDS count += n, sum += sum_r a_r and the upper triangle of
// 16 x 16 tiles of gram += sum_r a_r a_r^T, a_r = f_r - shift, into accumulators the caller zeroed once.
extern "C" int qarig_moments_add(const double* f, int n, int D, const double* shift, int64_t* count, double* sum,
                                 double* gram, void* stream) {
    QARIG_CHECK_ARG(f && count && sum && gram, "moments_add: null pointer");
    QARIG_CHECK_ARG(D >= 1 && D <= 1024, "moments_add: D = %d, need 1 ... 1024", D);
    QARIG_CHECK_ARG(n >= 1 && n <= (1 << 20), "moments_add: n = %d, need 1 ... 2^20", n);
    const size_t fb = (size_t)n * D * 8;
    QARIG_CHECK_ARG(!mom_overlap(f, fb, count, 8) && !mom_overlap(f, fb, sum, (size_t)D * 8) &&
                        !mom_overlap(f, fb, gram, (size_t)D * D * 8),
                    "moments_add: an accumulator aliases the features");
    const int T = (D + MOM_TILE - 1) / MOM_TILE;
    int gram_waves = 0;
    for (int ti = 0; ti < T; ++ti) gram_waves += mom_row_groups(T, ti);
    const int waves = gram_waves + (D + 63) / 64;              // <= 544 + 16
    hipLaunchKernelGGL(moments_add_kernel, dim3((waves + 3) / 4), dim3(256), 0, (hipStream_t)stream, f, n, D, shift,
                       gram_waves, count, sum, gram);
    QARIG_CHECK_LAUNCH("moments_add");
    return QARIG_OK;
}
