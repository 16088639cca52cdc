// Generation evaluation: k-nearest-neighbour statistics between two sets of fp64 feature rows (qarig/gen_eval.py
// manifold_metrics / nearest_real).  Two entries over one sweep: the k smallest squared distances of every query row
// (qarig_knn_smallest) and the number of x rows whose ball a query row falls into (qarig_ball_count).
//
// d2(i, j) = (|a_i|^2 + |b_j|^2) - 2 sum_c a_ic b_jc with a = q - shift, b = x - shift.  The inner products run on
// v_mfma_f64_16x16x4_f64, the feature index ascending in steps of four from a zero accumulator; the squared norms come
// from one kernel, one wave per row, in an order that depends on the row's length alone.  Every factor is commutative,
// so d2 is a function of the unordered pair of rows and the shift: its bits do not depend on which row is the query,
// on where a row sits, on the tile it lands in or on how the x axis is split over workgroups.  A top-k under a total
// order and an integer count do not depend on the order of the candidates either: no floating-point atomics, equal
// inputs give equal bits.
#include "qarig_common.h"
#include <utility>

extern "C" size_t qarig_knn_workspace_bytes(int nq, int nx, int D, int k);

namespace qarig {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int KNN_MAX_K = 8;
constexpr int KNN_ROWS = 64;                   // query rows of a workgroup: a strip of 16 per wave
constexpr int KNN_COLS = 64;                   // x rows of a column block: four 16 x 16 tiles per wave
constexpr int KNN_CHUNK = 32;                  // features staged through LDS at a time
constexpr int KNN_LD = KNN_CHUNK + 4;          // LDS row stride in doubles: 16 rows x 4 k of a fragment read hit 64 distinct banks
constexpr int KNN_MIN_BLOCKS = 4;              // column blocks a workgroup sweeps at least (where there are as many)
constexpr int KNN_TARGET_WGS = 1024;
constexpr int KNN_EMPTY = 0x7fffffff;          // the index of an empty slot while lists are merged; written as -1

// a_rc = f_rc - shift_c; exactly zero outside the (n, D) extent (after the subtraction)
__device__ __forceinline__ double knn_load(const double* __restrict__ f, const double* __restrict__ shift, int n, int D,
                                           int r, int c) {
    if (r >= n || c >= D) return 0.0;
    const double v = f[(int64_t)r * D + c];
    return shift ? v - shift[c] : v;
}

// columns c, c + 1 (c even) of row r; vec: D is even and f, shift are 16-byte aligned
__device__ __forceinline__ double2 knn_load2(const double* __restrict__ f, const double* __restrict__ shift, int n,
                                             int D, int r, int c, bool vec) {
    if (vec) {
        if (r >= n || c >= D) return make_double2(0.0, 0.0);
        double2 v = *reinterpret_cast<const double2*>(f + (int64_t)r * D + c);
        if (shift) {
            const double2 s = *reinterpret_cast<const double2*>(shift + c);
            v.x -= s.x;
            v.y -= s.y;
        }
        return v;
    }
    return make_double2(knn_load(f, shift, n, D, r, c), knn_load(f, shift, n, D, r, c + 1));
}

// THE squared distance of both entries: the two norms first (fp addition commutes), the doubled product exact.
__device__ __forceinline__ double knn_d2(double norm_a, double norm_b, double dot) {
    return (norm_a + norm_b) - 2.0 * dot;
}

// (value, index) order: ordinary < on doubles, equal values to the lower index; false whenever d is NaN
__device__ __forceinline__ bool knn_before(double d, int j, double v, int i) { return d < v || (d == v && j < i); }

template <int K>
struct KnnList {
    double v[K];
    int i[K];
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int s = 0; s < K; ++s) {
            v[s] = __builtin_inf();
            i[s] = KNN_EMPTY;
        }
    }
    __device__ __forceinline__ void insert(double d, int j) {
        if (!knn_before(d, j, v[K - 1], i[K - 1])) return;
        v[K - 1] = d;
        i[K - 1] = j;
#pragma unroll
        for (int s = K - 1; s > 0; --s) {
            const bool up = knn_before(v[s], i[s], v[s - 1], i[s - 1]);
            const double tv = v[s];
            const int ti = i[s];
            v[s] = up ? v[s - 1] : tv;
            i[s] = up ? i[s - 1] : ti;
            v[s - 1] = up ? tv : v[s - 1];
            i[s - 1] = up ? ti : i[s - 1];
        }
    }
};

// |a_r|^2 of every row of q (rows 0 ... nq - 1 of `norms`) and of x (rows nq ...): one wave per row, lane l takes the
// features l, l + 64, ... in ascending order, then a butterfly over the lanes.
__global__ __launch_bounds__(256) void knn_norms_kernel(const double* __restrict__ q, int nq,
                                                        const double* __restrict__ x, int nx, int D,
                                                        const double* __restrict__ shift, double* __restrict__ norms) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= nq + nx) return;
    const double* f = row < nq ? q : x;
    const int r = row < nq ? row : row - nq;
    double s = 0.0;
    for (int c = lane; c < D; c += 64) {
        const double a = knn_load(f, shift, r + 1, D, r, c);
        s += a * a;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) norms[row] = s;
}

struct KnnSweep {
    const double* q;
    const double* x;
    const double* shift;
    const double* norms;       // (nq + nx)
    const double* r2;          // (nx), ball count only
    double* d2_out;            // (splits, nq, k)
    int* idx_out;              // (splits, nq, k)
    int* count_out;            // (splits, nq), ball count only
    int nq, nx, D, k, self_offset, blocks_per_split, vec;
};

// Workgroup (blockIdx.x, blockIdx.y) = (64 query rows, a run of column blocks of 64 x rows).  Wave w owns the query
// strip 16 w ... 16 w + 15 and, per column block, four 16 x 16 accumulators (C/D map of the f64 MFMA: register g of a
// lane is row (lane >> 4) + 4 g, column lane & 15 -- NOT the f32 map).  Both operands go through LDS in chunks of 32
// features, shift subtracted, zeros past the extents; the next chunk's global loads are in flight while this chunk's
// products issue.  K = 0: ball count.
template <int K>
__global__ __launch_bounds__(256) void knn_sweep_kernel(KnnSweep p) {
    constexpr bool BALL = K == 0;
    constexpr int KL = BALL ? 1 : K;
    __shared__ double lq[KNN_ROWS * KNN_LD];
    __shared__ double lx[KNN_COLS * KNN_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lx16 = lane & 15, h = lane >> 4;
    const int i0 = blockIdx.x * KNN_ROWS;
    const int col_blocks = (p.nx + KNN_COLS - 1) / KNN_COLS;
    const int jb0 = blockIdx.y * p.blocks_per_split;
    const int jb1 = min(col_blocks, jb0 + p.blocks_per_split);
    const int chunks = (p.D + KNN_CHUNK - 1) / KNN_CHUNK;
    const int sr = tid >> 4, sc = (tid & 15) * 2;        // staging: rows sr + 16 u, features sc, sc + 1 of the chunk
    const bool vec = p.vec != 0;

    double nrm_q[4];
    int row[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        row[g] = i0 + wave * 16 + h + 4 * g;
        nrm_q[g] = row[g] < p.nq ? p.norms[row[g]] : 0.0;
    }
    KnnList<KL> best[4];
    int inside[4] = {0, 0, 0, 0};
#pragma unroll
    for (int g = 0; g < 4; ++g) best[g].clear();

    double2 rq[4], rx[4];
    int jb = jb0, kc = 0;                                // the (column block, chunk) whose operands rq / rx hold
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        rq[u] = knn_load2(p.q, p.shift, p.nq, p.D, i0 + sr + 16 * u, sc, vec);
        rx[u] = knn_load2(p.x, p.shift, p.nx, p.D, jb * KNN_COLS + sr + 16 * u, sc, vec);
    }
    f64x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = (f64x4){0.0, 0.0, 0.0, 0.0};

    while (jb < jb1) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            *reinterpret_cast<double2*>(lq + (sr + 16 * u) * KNN_LD + sc) = rq[u];
            *reinterpret_cast<double2*>(lx + (sr + 16 * u) * KNN_LD + sc) = rx[u];
        }
        __syncthreads();
        const int cur_jb = jb;
        const bool last_chunk = kc + 1 == chunks;
        if (last_chunk) {
            ++jb;
            kc = 0;
        } else {
            ++kc;
        }
        if (jb < jb1) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                rq[u] = knn_load2(p.q, p.shift, p.nq, p.D, i0 + sr + 16 * u, kc * KNN_CHUNK + sc, vec);
                rx[u] = knn_load2(p.x, p.shift, p.nx, p.D, jb * KNN_COLS + sr + 16 * u, kc * KNN_CHUNK + sc, vec);
            }
        }
#pragma unroll
        for (int s = 0; s < KNN_CHUNK / 4; ++s) {
            const double a = lq[(wave * 16 + lx16) * KNN_LD + 4 * s + h];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const double b = lx[(t * 16 + lx16) * KNN_LD + 4 * s + h];
                acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[t], 0, 0, 0);
            }
        }
        __syncthreads();
        if (!last_chunk) continue;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int j = cur_jb * KNN_COLS + t * 16 + lx16;
            const bool j_ok = j < p.nx;
            const double nrm_x = j_ok ? p.norms[p.nq + j] : 0.0;
            const double rad = (BALL && j_ok) ? p.r2[j] : 0.0;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const double d = knn_d2(nrm_q[g], nrm_x, acc[t][g]);
                const bool ok = j_ok && row[g] < p.nq && !(p.self_offset >= 0 && j == p.self_offset + row[g]);
                if (BALL) inside[g] += (ok && d <= rad) ? 1 : 0;
                else if (ok) best[g].insert(d, j);
            }
            acc[t] = (f64x4){0.0, 0.0, 0.0, 0.0};
        }
    }

    // the 16 lanes of a row (equal lane >> 4) merge: after four exchanges every one of them holds the row's result
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            if (BALL) {
                inside[g] += __shfl_xor(inside[g], o, 64);
            } else {
                double ov[KL];
                int oi[KL];
#pragma unroll
                for (int s = 0; s < KL; ++s) {
                    ov[s] = __shfl_xor(best[g].v[s], o, 64);
                    oi[s] = __shfl_xor(best[g].i[s], o, 64);
                }
#pragma unroll
                for (int s = 0; s < KL; ++s) best[g].insert(ov[s], oi[s]);
            }
        }
    }
    if (lx16 != 0) return;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        if (row[g] >= p.nq) continue;
        const int64_t o = (int64_t)blockIdx.y * p.nq + row[g];
        if (BALL) {
            p.count_out[o] = inside[g];
        } else {
#pragma unroll
            for (int s = 0; s < KL; ++s)
                if (s < p.k) {
                    p.d2_out[o * p.k + s] = best[g].v[s];
                    p.idx_out[o * p.k + s] = best[g].i[s] == KNN_EMPTY ? -1 : best[g].i[s];
                }
        }
    }
}

// One thread per query row: the splits' partial lists (splits, nq, k) merged into (nq, k).
__global__ __launch_bounds__(256) void knn_merge_kernel(const double* __restrict__ pd, const int* __restrict__ pi,
                                                        int splits, int nq, int k, double* __restrict__ d2_out,
                                                        int* __restrict__ idx_out) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= nq) return;
    KnnList<KNN_MAX_K> best;
    best.clear();
    for (int s = 0; s < splits; ++s)
        for (int e = 0; e < k; ++e) {
            const int64_t o = ((int64_t)s * nq + r) * k + e;
            const int j = pi[o];
            if (j >= 0) best.insert(pd[o], j);
        }
#pragma unroll
    for (int e = 0; e < KNN_MAX_K; ++e)
        if (e < k) {
            d2_out[(int64_t)r * k + e] = best.v[e];
            idx_out[(int64_t)r * k + e] = best.i[e] == KNN_EMPTY ? -1 : best.i[e];
        }
}

__global__ __launch_bounds__(256) void knn_count_sum_kernel(const int* __restrict__ part, int splits, int nq,
                                                            int* __restrict__ count_out) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= nq) return;
    int c = 0;
    for (int s = 0; s < splits; ++s) c += part[(int64_t)s * nq + r];
    count_out[r] = c;
}

struct KnnPlan {
    int splits, blocks_per_split;
    size_t norm_bytes, part_bytes;       // part_bytes: the partial lists (or counts) of splits > 1
};

static inline bool knn_extents_ok(int nq, int nx, int D, int k) {
    return D >= 1 && D <= 1024 && nq >= 1 && nq <= (1 << 20) && nx >= 1 && nx <= (1 << 20) && k >= 1 &&
           k <= KNN_MAX_K;
}

// Column blocks are dealt to workgroups in runs: at least KNN_MIN_BLOCKS each, as many as keep about KNN_TARGET_WGS
// workgroups in the launch.
static inline KnnPlan knn_plan(int nq, int nx, int k) {
    const int row_blocks = (nq + KNN_ROWS - 1) / KNN_ROWS, col_blocks = (nx + KNN_COLS - 1) / KNN_COLS;
    const int want = (KNN_TARGET_WGS + row_blocks - 1) / row_blocks;
    int per = (col_blocks + want - 1) / want;
    if (per < KNN_MIN_BLOCKS) per = KNN_MIN_BLOCKS < col_blocks ? KNN_MIN_BLOCKS : col_blocks;
    KnnPlan pl;
    pl.blocks_per_split = per;
    pl.splits = (col_blocks + per - 1) / per;
    pl.norm_bytes = (((size_t)nq + nx) * 8 + 15) & ~(size_t)15;
    pl.part_bytes = pl.splits > 1 ? (size_t)pl.splits * nq * k * 12 : 0;
    return pl;
}

static inline bool knn_overlap(const void* p, size_t pb, const void* q, size_t qb) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return p && q && a < b + qb && b < a + pb;
}

// The checks both entries share; `outs` are their outputs (pointer, bytes), `r2` is NULL for knn_smallest.
static int knn_check(const char* what, const double* q, int nq, const double* x, int nx, int D, const double* shift,
                     const double* r2, int k, int self_offset, const void* ws, size_t ws_bytes,
                     std::initializer_list<std::pair<const void*, size_t>> outs) {
    QARIG_CHECK_ARG(q && x && ws, "%s: null pointer", what);
    for (const auto& o : outs) QARIG_CHECK_ARG(o.first, "%s: null pointer", what);
    QARIG_CHECK_ARG(D >= 1 && D <= 1024, "%s: D = %d, need 1 ... 1024", what, D);
    QARIG_CHECK_ARG(nq >= 1 && nq <= (1 << 20), "%s: nq = %d, need 1 ... 2^20", what, nq);
    QARIG_CHECK_ARG(nx >= 1 && nx <= (1 << 20), "%s: nx = %d, need 1 ... 2^20", what, nx);
    QARIG_CHECK_ARG(k >= 1 && k <= KNN_MAX_K, "%s: k = %d, need 1 ... %d", what, k, KNN_MAX_K);
    QARIG_CHECK_ARG(self_offset == -1 || (self_offset >= 0 && self_offset <= nx - nq),
                    "%s: self_offset = %d, need -1 or 0 ... nx - nq = %d", what, self_offset, nx - nq);
    QARIG_CHECK_ARG(nx - (self_offset >= 0 ? 1 : 0) >= k, "%s: %d candidates per query, fewer than k = %d", what,
                    nx - (self_offset >= 0 ? 1 : 0), k);
    const size_t need = qarig_knn_workspace_bytes(nq, nx, D, k);
    if (ws_bytes < need) {
        qarig_set_error("%s: the workspace holds %zu bytes, %zu are needed", what, ws_bytes, need);
        return QARIG_ERR_WORKSPACE;
    }
    const std::pair<const void*, size_t> ins[] = {{q, (size_t)nq * D * 8}, {x, (size_t)nx * D * 8},
                                                  {shift, (size_t)D * 8}, {r2, (size_t)nx * 8}};
    for (const auto& in : ins) {
        QARIG_CHECK_ARG(!knn_overlap(ws, need, in.first, in.second), "%s: the workspace overlaps an input", what);
        for (const auto& o : outs)
            QARIG_CHECK_ARG(!knn_overlap(o.first, o.second, in.first, in.second), "%s: an output overlaps an input",
                            what);
    }
    return QARIG_OK;
}

static void knn_launch_norms(const double* q, int nq, const double* x, int nx, int D, const double* shift,
                             double* norms, hipStream_t stream) {
    hipLaunchKernelGGL(knn_norms_kernel, dim3((unsigned)((nq + nx + 3) / 4)), dim3(256), 0, stream, q, nq, x, nx, D,
                       shift, norms);
}

static inline int knn_vec(const double* q, const double* x, const double* shift, int D) {
    return (D % 2 == 0 && (uintptr_t)q % 16 == 0 && (uintptr_t)x % 16 == 0 && (uintptr_t)shift % 16 == 0) ? 1 : 0;
}

}  // namespace qarig

using namespace qarig;

extern "C" size_t qarig_knn_workspace_bytes(int nq, int nx, int D, int k) {
    if (!knn_extents_ok(nq, nx, D, k)) return 0;
    const KnnPlan pl = knn_plan(nq, nx, k);
    return pl.norm_bytes + pl.part_bytes;
}

extern "C" int qarig_knn_smallest(const double* q, int nq, const double* x, int nx, int D, const double* shift, int k,
                                  int self_offset, double* d2_out, int* idx_out, void* ws, size_t ws_bytes,
                                  void* stream) {
    const size_t out_d = knn_extents_ok(nq, nx, D, k) ? (size_t)nq * k * 8 : 0;
    const int st = knn_check("knn_smallest", q, nq, x, nx, D, shift, nullptr, k, self_offset, ws, ws_bytes,
                             {{d2_out, out_d}, {idx_out, out_d / 2}});
    if (st != QARIG_OK) return st;
    const KnnPlan pl = knn_plan(nq, nx, k);
    double* norms = (double*)ws;
    double* part_d = (double*)((char*)ws + pl.norm_bytes);
    int* part_i = (int*)(part_d + (size_t)pl.splits * nq * k);
    const bool direct = pl.splits == 1;
    knn_launch_norms(q, nq, x, nx, D, shift, norms, (hipStream_t)stream);
    QARIG_CHECK_LAUNCH("knn_smallest (norms)");
    KnnSweep p{q, x, shift, norms, nullptr, direct ? d2_out : part_d, direct ? idx_out : part_i, nullptr,
               nq, nx, D, k, self_offset, pl.blocks_per_split, knn_vec(q, x, shift, D)};
    const dim3 grid((unsigned)((nq + KNN_ROWS - 1) / KNN_ROWS), (unsigned)pl.splits);
    if (k == 1) hipLaunchKernelGGL(knn_sweep_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, p);
    else if (k <= 4) hipLaunchKernelGGL(knn_sweep_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL(knn_sweep_kernel<KNN_MAX_K>, grid, dim3(256), 0, (hipStream_t)stream, p);
    QARIG_CHECK_LAUNCH("knn_smallest");
    if (!direct) {
        hipLaunchKernelGGL(knn_merge_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                           part_d, part_i, pl.splits, nq, k, d2_out, idx_out);
        QARIG_CHECK_LAUNCH("knn_smallest (merge)");
    }
    return QARIG_OK;
}

extern "C" int qarig_ball_count(const double* q, int nq, const double* x, int nx, int D, const double* shift,
                                const double* r2, int self_offset, int* count_out, void* ws, size_t ws_bytes,
                                void* stream) {
    QARIG_CHECK_ARG(r2, "ball_count: null pointer");
    const size_t out_b = knn_extents_ok(nq, nx, D, 1) ? (size_t)nq * 4 : 0;
    const int st = knn_check("ball_count", q, nq, x, nx, D, shift, r2, 1, self_offset, ws, ws_bytes,
                             {{count_out, out_b}});
    if (st != QARIG_OK) return st;
    const KnnPlan pl = knn_plan(nq, nx, 1);
    double* norms = (double*)ws;
    int* part = (int*)((char*)ws + pl.norm_bytes);
    const bool direct = pl.splits == 1;
    knn_launch_norms(q, nq, x, nx, D, shift, norms, (hipStream_t)stream);
    QARIG_CHECK_LAUNCH("ball_count (norms)");
    KnnSweep p{q, x, shift, norms, r2, nullptr, nullptr, direct ? count_out : part,
               nq, nx, D, 1, self_offset, pl.blocks_per_split, knn_vec(q, x, shift, D)};
    const dim3 grid((unsigned)((nq + KNN_ROWS - 1) / KNN_ROWS), (unsigned)pl.splits);
    hipLaunchKernelGGL(knn_sweep_kernel<0>, grid, dim3(256), 0, (hipStream_t)stream, p);
    QARIG_CHECK_LAUNCH("ball_count");
    if (!direct) {
        hipLaunchKernelGGL(knn_count_sum_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0,
                           (hipStream_t)stream, part, pl.splits, nq, count_out);
        QARIG_CHECK_LAUNCH("ball_count (sum)");
    }
    return QARIG_OK;
}
