// Held-out evaluation: per-row negative log-likelihood and rank of the target among the logits
// (token_score_kernel), and their reduction per image, per position and in total into fp64 / int64
// accumulators that stay on the device for a whole dataset (score_reduce_kernel).  One wave per row /
// per output element; no floating-point atomics, so two runs over the same rows are bit-identical.
#include "qarig_common.h"
#include "row_sweep.h"

namespace qarig {

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// The arithmetic of the cross-entropy row kernel (loss.hip) on its sweeps (row_sweep.h): lane partial sums in
// ascending trips, the 64-lane butterfly, nll = log s - (x[t] - mx).  x[t] is read first, so the rank is counted in
// the sweep that finds the maximum (neither depends on the order).
__global__ __launch_bounds__(256) void token_score_kernel(const float* __restrict__ logits,
                                                          const int64_t* __restrict__ target, int M, int C,
                                                          int64_t ignore_index, float* __restrict__ row_nll,
                                                          int* __restrict__ row_rank, int* __restrict__ bad) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const int64_t t = target[row];
    if (t == ignore_index || t < 0 || t >= C) {      // wave-uniform: a skipped row, or a target no class has
        if (lane == 0) {
            if (t != ignore_index) atomicExch(bad, 1);
            row_nll[row] = 0.0f;
            row_rank[row] = -1;
        }
        return;
    }
    const float* x = logits + (int64_t)row * C;
    const float xt = x[t];
    const int ti = (int)t;
    float mx = -INFINITY;
    int above = 0;
    row_sweep(x, C, lane, [&](float v, int col) {
        mx = fmaxf(mx, v);
        above += (int)((v > xt) | ((v == xt) & (col < ti)));        // | and &: selects, no branch per column
    });
    mx = wave_max(mx);
    above = wave_sum_i(above);
    float s = 0.0f;
    row_sweep(x, C, lane, [&](float v, int) { s += expf(v - mx); });
    s = wave_sum(s);
    if (lane == 0) {
        row_nll[row] = logf(s) - (xt - mx);
        row_rank[row] = above;
    }
}

// Waves 0 ... N-1 own img_nll[n], waves N ... N+S-1 own pos_nll / pos_cnt[pos0 + s], wave N+S owns totals.
// fp64 sums: per lane in ascending trips, then the butterfly -- one fixed order.
__global__ __launch_bounds__(256) void score_reduce_kernel(const float* __restrict__ row_nll,
                                                           const int* __restrict__ row_rank, int N, int S,
                                                           int pos0, int topk, double* __restrict__ img_nll,
                                                           double* __restrict__ pos_nll,
                                                           int64_t* __restrict__ pos_cnt,
                                                           int64_t* __restrict__ totals) {
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w < N) {
        const float* v = row_nll + w * S;
        double a = 0.0;
        for (int s = lane; s < S; s += 64) a += (double)v[s];
        a = wave_sum_d(a);
        if (lane == 0) img_nll[w] += a;
    } else if (w < (int64_t)N + S) {
        const int64_t s = w - N;
        double a = 0.0;
        int cnt = 0;
        for (int n = lane; n < N; n += 64) {
            a += (double)row_nll[(int64_t)n * S + s];
            cnt += row_rank[(int64_t)n * S + s] >= 0 ? 1 : 0;
        }
        a = wave_sum_d(a);
        cnt = wave_sum_i(cnt);
        if (lane == 0) {
            pos_nll[pos0 + s] += a;
            pos_cnt[pos0 + s] += cnt;
        }
    } else if (w == (int64_t)N + S) {
        const int64_t M = (int64_t)N * S;
        int counted = 0, top1 = 0, top = 0;      // at most 2^40 / 64 rows per lane: see the entry's extent check
        int64_t done = 0;
        if ((reinterpret_cast<uintptr_t>(row_rank) & 15) == 0) {
            const int4* q = reinterpret_cast<const int4*>(row_rank);
            for (int64_t i = lane; i < M / 4; i += 64) {
                const int4 r = q[i];
                counted += (r.x >= 0) + (r.y >= 0) + (r.z >= 0) + (r.w >= 0);
                top1 += (r.x == 0) + (r.y == 0) + (r.z == 0) + (r.w == 0);
                top += (r.x >= 0 && r.x < topk) + (r.y >= 0 && r.y < topk) + (r.z >= 0 && r.z < topk) +
                       (r.w >= 0 && r.w < topk);
            }
            done = M / 4 * 4;
        }
        for (int64_t i = done + lane; i < M; i += 64) {
            const int r = row_rank[i];
            counted += r >= 0;
            top1 += r == 0;
            top += r >= 0 && r < topk;
        }
        counted = wave_sum_i(counted);
        top1 = wave_sum_i(top1);
        top = wave_sum_i(top);
        if (lane == 0) {
            totals[0] += counted;
            totals[1] += top1;
            totals[2] += top;
        }
    }
}

}  // namespace qarig

using namespace qarig;

// logits (M,C) fp32 contiguous, target int64 (M).  row_nll[r] = log sum_c exp(x[c] - mx) - (x[t] - mx);
// row_rank[r] = #{c : x[c] > x[t]} + #{c < t : x[c] == x[t]} (0: the target is the arg-max, ties to the
// smaller index).  target == ignore_index: (0, -1); any other target outside [0,C): (0, -1) and *bad_flag set.
extern "C" int qarig_token_score(const float* logits, const int64_t* target, int M, int C, int64_t ignore_index,
                                 float* row_nll, int* row_rank, int* bad_flag, void* stream) {
    QARIG_CHECK_ARG(logits && target && row_nll && row_rank && bad_flag && M > 0 && C > 0,
                    "token_score: bad arguments");
    QARIG_CHECK_DIMS("token_score", M, C);
    hipLaunchKernelGGL(token_score_kernel, dim3((M + 3) / 4), dim3(256), 0, (hipStream_t)stream, logits, target,
                       M, C, ignore_index, row_nll, row_rank, bad_flag);
    QARIG_CHECK_LAUNCH("token_score");
    return QARIG_OK;
}

// Rows r = n S + s of one scored batch, column s at absolute position pos0 + s < P, ADDED into caller-zeroed
// accumulators: img_nll (N) and pos_nll (P) fp64, pos_cnt (P) and totals (3: counted rows, rank == 0,
// 0 <= rank < topk) int64.  N S below 2^31 (the total counts of one launch are 32-bit per wave).
extern "C" int qarig_score_reduce(const float* row_nll, const int* row_rank, int N, int S, int pos0, int P,
                                  int topk, double* img_nll, double* pos_nll, int64_t* pos_cnt, int64_t* totals,
                                  void* stream) {
    QARIG_CHECK_ARG(row_nll && row_rank && img_nll && pos_nll && pos_cnt && totals, "score_reduce: null pointer");
    QARIG_CHECK_ARG(qarig_dims_ok({N, S}, 1LL << 24, (1LL << 31) - 1),
                    "score_reduce: N and S must be positive, at most 2^24 each, their product below 2^31");
    QARIG_CHECK_ARG(P > 0 && P <= (1 << 24) && pos0 >= 0 && pos0 <= P - S && topk >= 0,
                    "score_reduce: need 0 <= pos0, pos0 + S <= P <= 2^24, topk >= 0");
    const int64_t waves = (int64_t)N + S + 1;
    hipLaunchKernelGGL(score_reduce_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                       row_nll, row_rank, N, S, pos0, topk, img_nll, pos_nll, pos_cnt, totals);
    QARIG_CHECK_LAUNCH("score_reduce");
    return QARIG_OK;
}
