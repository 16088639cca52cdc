// Single-token decode step (generate_images.py:256-345 evaluates the decoder once per sampled
// token): the Linear layers of ONE new row per sequence are weight-streaming matrix-vector
// products -- 1 to 4 MB of fp32 weights against <= 16 activation rows -- chained by data
// dependencies, ~80 launches per token.  Such a launch is not bandwidth-bound (16 KB per CU) but
// LATENCY-bound: its time is the number of dependent memory round trips on its critical path.
// decode_linear_kernel therefore issues EVERY load of the launch before it waits for anything:
// the activation rows, the LayerNorm operands, the epilogue operands of the lane's final output
// and the weights (non-temporal, fully coalesced: a workgroup streams a contiguous run of weight
// rows, 4 KB per load instruction); one wait, fma chains on the vector ALU, a halving butterfly
// across the wave, one LDS hand-over between the waves that share a column, epilogue, store.
// Every summation order is fixed (no atomics): results are run-to-run bit-reproducible.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qarig_common.h"

namespace qarig {

// The operands a launch needs to issue its loads come first, as individual kernel arguments: the first 16
// dwords of the kernel-argument segment are preloaded into SGPRs by the command processor
// (-mllvm -amdgpu-kernarg-preload-count=16 in build.py for this file), so the first loads do not wait for a
// scalar-cache miss on the argument segment the host has just written.  The rest travels as a struct.
struct DecLin {
    const float* bias; int64_t bias_gs;      // (N) per group, or null
    float* C; int64_t ldc, c_gs;             // out (M, N) per group
    const float* residual; int64_t ldr;      // (M, N) added before the activation, or null
    const float* mul; int64_t ldmul;         // (M, N) elementwise factor on the output, or null; ldmul 0: one row
    const float* gamma; const float* beta;   // LN = 1: nn.LayerNorm affine form (K)
    const float* scale; const float* shift;  // LN = 2: AdaLN rows (M, K) at ldmod; LN = 3: one row for all
    int64_t ldmod;
    float eps;
};

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ float4 ld4_nt(const float* p) {
#ifdef QARIG_DECODE_NO_NT       // ablation build (tools/): weights through the default cache policy
    return ld4(p);
#else
    typedef float v4 __attribute__((ext_vector_type(4)));
    const v4 r = __builtin_nontemporal_load(reinterpret_cast<const v4*>(p));
    return make_float4(r.x, r.y, r.z, r.w);
#endif
}

// Weight element types of the streaming kernels.  A lane's weight load carries E consecutive weights of a row and
// meets E activations (E / 4 float4): fp32, 16 B = 4 weights; bf16 (row-major (N, K) images as qarig_cast_bf16 writes
// them), 16 B = 8 weights, or 8 B = 4 weights for K = 256, where 64 lanes cover a row as they do in fp32.  bf16 -> fp32
// is exact -- a shift for the low half of a dword, a mask for the high half: no rounding mode, subnormals pass.
struct bf16w { uint16_t bits; };
__device__ __forceinline__ float bf16_lo(uint32_t d) { return __uint_as_float(d << 16); }
__device__ __forceinline__ float bf16_hi(uint32_t d) { return __uint_as_float(d & 0xffff0000u); }
template <typename WT, int E> struct WLoad;
template <> struct WLoad<float, 4> {
    float4 r;
    __device__ __forceinline__ void issue(const float* p) { r = ld4_nt(p); }
    __device__ __forceinline__ void get(float4 (&w)[1]) const { w[0] = r; }
};
template <> struct WLoad<bf16w, 8> {
    typedef uint32_t v4 __attribute__((ext_vector_type(4)));
    v4 r;
    __device__ __forceinline__ void issue(const bf16w* p) {
#ifdef QARIG_DECODE_NO_NT
        r = *reinterpret_cast<const v4*>(p);
#else
        r = __builtin_nontemporal_load(reinterpret_cast<const v4*>(p));
#endif
    }
    __device__ __forceinline__ void get(float4 (&w)[2]) const {
        w[0] = make_float4(bf16_lo(r.x), bf16_hi(r.x), bf16_lo(r.y), bf16_hi(r.y));
        w[1] = make_float4(bf16_lo(r.z), bf16_hi(r.z), bf16_lo(r.w), bf16_hi(r.w));
    }
};
template <> struct WLoad<bf16w, 4> {
    typedef uint32_t v2 __attribute__((ext_vector_type(2)));
    v2 r;
    __device__ __forceinline__ void issue(const bf16w* p) {
#ifdef QARIG_DECODE_NO_NT
        r = *reinterpret_cast<const v2*>(p);
#else
        r = __builtin_nontemporal_load(reinterpret_cast<const v2*>(p));
#endif
    }
    __device__ __forceinline__ void get(float4 (&w)[1]) const {
        w[0] = make_float4(bf16_lo(r.x), bf16_hi(r.x), bf16_lo(r.y), bf16_hi(r.y));
    }
};

template <int CTRL>
__device__ __forceinline__ float dpp_lane(float x) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), CTRL, 0xf, 0xf, true));
}

// Sums V per-lane values over the 64 lanes of a wave in about 3 V vector instructions instead of 6 V
// shuffles: at every step a lane hands half of its values to a partner lane and keeps the sums of the
// other half.  The four steps inside a 16-lane row are DPP operands (row_mirror, row_half_mirror, two
// quad permutations: no LDS round trip); the two steps across rows are ds_bpermute exchanges, issued
// back to back per step.  Returns the number of the value whose wave total v[0] holds on this lane;
// `owner` is true on exactly one lane per value.  Fixed order: bit-reproducible.
template <int V>
__device__ __forceinline__ int wave_sum_multi(float (&v)[V], int lane, bool& owner) {
    static_assert(V >= 1 && V <= 64 && (V & (V - 1)) == 0, "power of two, at most the wave");
    int idx = 0, dup = 0;
#define QARIG_ROW_STEP(CTRL, BIT, N0)                                       \
    if constexpr ((N0) > 1) {                                               \
        constexpr int n = (N0) / 2;                                         \
        const bool up = (lane & (BIT)) != 0;                                \
        _Pragma("unroll") for (int i = 0; i < n; ++i) {                     \
            const float send = up ? v[i] : v[i + n];                        \
            const float keep = up ? v[i + n] : v[i];                        \
            v[i] = keep + dpp_lane<CTRL>(send);                             \
        }                                                                   \
        if (up) idx += n;                                                   \
    } else {                                                                \
        v[0] += dpp_lane<CTRL>(v[0]);                                       \
        dup |= (BIT);                                                       \
    }
    constexpr int N1 = V, N2 = N1 > 1 ? N1 / 2 : 1, N3 = N2 > 1 ? N2 / 2 : 1, N4 = N3 > 1 ? N3 / 2 : 1,
                  N5 = N4 > 1 ? N4 / 2 : 1, N6 = N5 > 1 ? N5 / 2 : 1;
    QARIG_ROW_STEP(0x140, 8, N1)    // row_mirror: lane i <-> 15 - i
    QARIG_ROW_STEP(0x141, 4, N2)    // row_half_mirror: i <-> 7 - i
    QARIG_ROW_STEP(0x4E, 2, N3)     // quad_perm [2,3,0,1]
    QARIG_ROW_STEP(0xB1, 1, N4)     // quad_perm [1,0,3,2]
#undef QARIG_ROW_STEP
#define QARIG_XROW_STEP(MASK, N0)                                           \
    if constexpr ((N0) > 1) {                                               \
        constexpr int n = (N0) / 2;                                         \
        const bool up = (lane & (MASK)) != 0;                               \
        float got[n];                                                       \
        _Pragma("unroll") for (int i = 0; i < n; ++i) got[i] = __shfl_xor(up ? v[i] : v[i + n], MASK, 64); \
        _Pragma("unroll") for (int i = 0; i < n; ++i) v[i] = (up ? v[i + n] : v[i]) + got[i];              \
        if (up) idx += n;                                                   \
    } else {                                                                \
        v[0] += __shfl_xor(v[0], MASK, 64);                                 \
        dup |= (MASK);                                                      \
    }
    QARIG_XROW_STEP(16, N5)
    QARIG_XROW_STEP(32, N6)
#undef QARIG_XROW_STEP
    owner = (lane & dup) == 0;
    return idx;
}

// MR: activation rows held (M padded up); LN: 0 none, 1 gamma/beta, 2 scale/shift rows, 3 one scale/shift
// row for every activation row (all rows of a decode step sit at the same window position);
// WT, E: the weight element type and the weights per load (WLoad); a "unit" below is E consecutive k;
// J: weight loads per thread; KS: 1-K chunks of a weight row per thread (K = 256 E KS when KS > 1).
// 256 threads.  K/E = kq units per row:
//   KS == 1: kq in {64, 128, 256}; the workgroup's load pass j covers 256/kq whole rows,
//            thread t sits in row group t / kq at unit t % kq; a column is summed over kq/64 waves;
//   KS  > 1: kq = 256 KS; passes j = c KS + s cover chunk s of row c; a column is summed over all 4 waves.
template <typename WT, int E, int MR, int LN, int J, int KS>
__global__ __launch_bounds__(256) void decode_linear_kernel(const float* __restrict__ Xb, const WT* __restrict__ Wb,
                                                            int64_t ldx, int64_t ldw, int M, int N, int K, int act,
                                                            int64_t x_gs, int64_t w_gs, DecLin p) {
    static_assert(J % KS == 0 && (LN == 0 || KS == 1) && LN >= 0 && LN <= 3 && (E == 4 || E == 8), "");
    constexpr int Q = E / 4;            // float4 of activations per unit
    constexpr int ES = E == 4 ? 2 : 3;  // log2 E
    constexpr int NC = J / KS;          // distinct columns per thread
    constexpr int V = NC * MR;          // partial sums per thread
    __shared__ float red[4][V];
    __shared__ float stat[4][MR];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int g = blockIdx.y;
    // kq = K/E is a power of two (host-checked): shifts instead of integer divisions
    const int kqs = KS == 1 ? 31 - __builtin_clz(K >> ES) : 8;    // log2 kq (KS > 1: of the 256-unit chunk)
    const int cgs = KS == 1 ? 8 - kqs : 0;                          // log2 CG, CG = 256 / kq row groups per pass
    const int WS = 4 >> cgs;                                        // waves that share a column
    const int cg = KS == 1 ? t >> kqs : 0;                          // wave-uniform
    const int kc = KS == 1 ? t & ((1 << kqs) - 1) : t;
    constexpr int ncs = NC == 1 ? 0 : (NC == 2 ? 1 : 2);
    const int cws = ncs + cgs;                                      // log2 CW, CW = NC * CG columns of this workgroup
    const int n0 = blockIdx.x << cws;
    const float* X = Xb + (int64_t)g * x_gs;
    const WT* W = Wb + (int64_t)g * w_gs;

    // ---- every load of the launch, oldest first in the order they are needed.  No load sits behind a
    //      branch (the compiler waits for a conditional load where its value meets the alternative):
    //      rows / columns past the end re-read the last one, absent operands read X; what they produce
    //      is never stored.
    const int Ml = M - 1, Nl = N - 1;
    float4 xv[KS][MR][Q];
#pragma unroll
    for (int s = 0; s < KS; ++s)
#pragma unroll
        for (int m = 0; m < MR; ++m)
#pragma unroll
            for (int q = 0; q < Q; ++q)
                xv[s][m][q] = ld4(X + (int64_t)min(m, Ml) * ldx + E * (kc + 256 * s) + 4 * q);
    float4 lg[Q], lb[Q], ls[LN == 2 ? MR : 1][Q], lh[LN == 2 ? MR : 1][Q];
    if (LN == 1 || LN == 3) {
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            lg[q] = ld4((LN == 1 ? p.gamma : p.scale) + E * kc + 4 * q);
            lb[q] = ld4((LN == 1 ? p.beta : p.shift) + E * kc + 4 * q);
        }
    }
    if (LN == 2) {
#pragma unroll
        for (int m = 0; m < MR; ++m) {
            const int64_t mo = (int64_t)min(m, Ml) * p.ldmod + E * kc;
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                ls[m][q] = ld4(p.scale + mo + 4 * q);
                lh[m][q] = ld4(p.shift + mo + 4 * q);
            }
        }
    }
    // the output this thread will finish: row t / CW, column t % CW
    const int om = t >> cws, ocl = t & ((1 << cws) - 1);
    const int on = n0 + ocl;
    const bool oval = om < M && on < N;
    const int omc = min(om, Ml), onc = min(on, Nl);
    const float eb = *(p.bias ? p.bias + (int64_t)g * p.bias_gs + onc : X);
    const float er = *(p.residual ? p.residual + (int64_t)omc * p.ldr + onc : X);
    const float em = *(p.mul ? p.mul + (int64_t)omc * p.ldmul + onc : X);
    WLoad<WT, E> wv[J];
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const int c = j / KS, s = j % KS;
        wv[j].issue(W + (int64_t)min(n0 + (c << cgs) + cg, Nl) * ldw + E * (kc + 256 * s));
    }
    __builtin_amdgcn_sched_barrier(0);      // nothing that waits for a load moves in front of the last issue

    // ---- LayerNorm of the rows on the way in (two passes: mean, then centred squares --
    //      layernorm_fwd_kernel's form); the weights are still in flight
    if (LN) {
        const float invK = 1.0f / (float)K;       // K is a power of two here: exact
        float s1[MR];
#pragma unroll
        for (int m = 0; m < MR; ++m) {
            s1[m] = (xv[0][m][0].x + xv[0][m][0].y) + (xv[0][m][0].z + xv[0][m][0].w);
#pragma unroll
            for (int q = 1; q < Q; ++q) s1[m] += (xv[0][m][q].x + xv[0][m][q].y) + (xv[0][m][q].z + xv[0][m][q].w);
        }
        bool own;
        int idx = wave_sum_multi<MR>(s1, lane, own);
        if (own) stat[w][idx] = s1[0];
        __syncthreads();
        float mean[MR];
#pragma unroll
        for (int m = 0; m < MR; ++m) {
            float a = stat[cg * WS][m];
#pragma nounroll
            for (int i = 1; i < WS; ++i) a += stat[cg * WS + i][m];
            mean[m] = a * invK;
        }
        __syncthreads();
        float s2[MR];
#pragma unroll
        for (int m = 0; m < MR; ++m) {
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                float4& x = xv[0][m][q];
                x.x -= mean[m]; x.y -= mean[m]; x.z -= mean[m]; x.w -= mean[m];
                float sq = q == 0 ? x.x * x.x : fmaf(x.x, x.x, s2[m]);
                sq = fmaf(x.y, x.y, sq); sq = fmaf(x.z, x.z, sq); sq = fmaf(x.w, x.w, sq);
                s2[m] = sq;
            }
        }
        idx = wave_sum_multi<MR>(s2, lane, own);
        if (own) stat[w][idx] = s2[0];
        __syncthreads();
#pragma unroll
        for (int m = 0; m < MR; ++m) {
            float a = stat[cg * WS][m];
#pragma nounroll
            for (int i = 1; i < WS; ++i) a += stat[cg * WS + i][m];
            // v_rsq_f32: 1 ulp of 1 / sqrt() -- 6e-8 relative on the row, far inside the 2e-6 of the parity tests
            // (every vector instruction of this single-wave-per-SIMD kernel is on the launch's critical path)
            const float rstd = __builtin_amdgcn_rsqf(a * invK + p.eps);
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                float4& x = xv[0][m][q];
                const float4 gg = LN == 2 ? ls[LN == 2 ? m : 0][q] : lg[q];
                const float4 hh = LN == 2 ? lh[LN == 2 ? m : 0][q] : lb[q];
                x.x = fmaf(x.x * rstd, gg.x, hh.x); x.y = fmaf(x.y * rstd, gg.y, hh.y);
                x.z = fmaf(x.z * rstd, gg.z, hh.z); x.w = fmaf(x.w * rstd, gg.w, hh.w);
            }
        }
    }

    // ---- partial dot products: k ascending inside the thread's chunk(s)
    float acc[V];
#pragma unroll
    for (int i = 0; i < V; ++i) acc[i] = 0.0f;
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const int c = j / KS, s = j % KS;
        float4 wq[Q];
        wv[j].get(wq);
#pragma unroll
        for (int m = 0; m < MR; ++m) {
            float a = acc[c * MR + m];
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                a = fmaf(wq[q].x, xv[s][m][q].x, a); a = fmaf(wq[q].y, xv[s][m][q].y, a);
                a = fmaf(wq[q].z, xv[s][m][q].z, a); a = fmaf(wq[q].w, xv[s][m][q].w, a);
            }
            acc[c * MR + m] = a;
        }
    }
    bool own;
    const int idx = wave_sum_multi<V>(acc, lane, own);
    if (own) red[w][idx] = acc[0];
    __syncthreads();
    if (oval) {
        const int c = ocl >> cgs, ocg = ocl & ((1 << cgs) - 1);
        float v = red[ocg * WS][c * MR + om];
#pragma nounroll
        for (int i = 1; i < WS; ++i) v += red[ocg * WS + i][c * MR + om];
        if (p.bias) v += eb;
        if (p.residual) v += er;
        v = act == ACT_SILU ? v * sigmoid_f(v) : act_fwd(v, act);
        if (p.mul) v *= em;
        p.C[(int64_t)g * p.c_gs + (int64_t)om * p.ldc + on] = v;
    }
}


// Which value's total lane `lane` holds after wave_sum_multi<V>, and whether it is that value's owner -- known
// from the lane number alone, so a lane can request the epilogue operands of its output before anything else.
template <int V>
__device__ __forceinline__ int wave_sum_multi_index(int lane, bool& owner) {
    int idx = 0, dup = 0, n = V;
#pragma unroll
    for (int step = 0; step < 6; ++step) {
        const int bit = step == 0 ? 8 : (step == 1 ? 4 : (step == 2 ? 2 : (step == 3 ? 1 : (step == 4 ? 16 : 32))));
        if (n > 1) {
            n >>= 1;
            if (lane & bit) idx += n;
        } else {
            dup |= bit;
        }
    }
    owner = (lane & dup) == 0;
    return idx;
}

// 5 ... 16 activation rows (the candidate chunks of a few images as one batch): the ROWS are split over the four
// waves of the workgroup -- wave w owns rows 4w .. 4w+3 -- and every wave streams the workgroup's whole run of
// weight rows (CW columns; the three later waves hit the lines the first one brought in).  Against holding all 16
// rows in every lane (decode_linear_kernel<16, ...>: 2,057 instructions in its LayerNorm form, every one of them on
// the critical path of a single-wave-per-SIMD launch) a lane now carries 4 rows: a quarter of the LayerNorm and
// statistics arithmetic, sums that stay inside the wave (no LDS hand-over, no workgroup barrier at all), the same
// fma count.  WT, E as in decode_linear_kernel; KW: 64-unit chunks of a weight row per lane (K = 64 E KW); a lane's
// loads j = c KW + s cover chunk s of column c.
template <typename WT, int E, int LN, int CW, int KW>
__global__ __launch_bounds__(256) void decode_linear_rows_kernel(const float* __restrict__ Xb, const WT* __restrict__ Wb,
                                                                 int64_t ldx, int64_t ldw, int M, int N, int K, int act,
                                                                 int64_t x_gs, int64_t w_gs, DecLin p) {
    static_assert(LN >= 0 && LN <= 3 && CW * 4 <= 64 && (E == 4 || E == 8), "");
    constexpr int Q = E / 4;
    constexpr int V = CW * 4;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (4 * w >= M) return;                 // a whole wave without rows (no barrier below)
    const int g = blockIdx.y;
    const int n0 = blockIdx.x * CW;
    const float* X = Xb + (int64_t)g * x_gs;
    const WT* W = Wb + (int64_t)g * w_gs;
    const int Ml = M - 1, Nl = N - 1;
    float4 xv[KW][4][Q];
#pragma unroll
    for (int s = 0; s < KW; ++s)
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int q = 0; q < Q; ++q)
                xv[s][m][q] = ld4(X + (int64_t)min(4 * w + m, Ml) * ldx + E * (lane + 64 * s) + 4 * q);
    float4 lg[(LN == 1 || LN == 3) ? KW : 1][Q], lb[(LN == 1 || LN == 3) ? KW : 1][Q];
    float4 ls[LN == 2 ? KW : 1][4][Q], lh[LN == 2 ? KW : 1][4][Q];
    if (LN == 1 || LN == 3) {
#pragma unroll
        for (int s = 0; s < KW; ++s)
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                lg[s][q] = ld4((LN == 1 ? p.gamma : p.scale) + E * (lane + 64 * s) + 4 * q);
                lb[s][q] = ld4((LN == 1 ? p.beta : p.shift) + E * (lane + 64 * s) + 4 * q);
            }
    }
    if (LN == 2) {
#pragma unroll
        for (int s = 0; s < KW; ++s)
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const int64_t mo = (int64_t)min(4 * w + m, Ml) * p.ldmod + E * (lane + 64 * s);
#pragma unroll
                for (int q = 0; q < Q; ++q) {
                    ls[s][m][q] = ld4(p.scale + mo + 4 * q);
                    lh[s][m][q] = ld4(p.shift + mo + 4 * q);
                }
            }
    }
    bool own;
    const int oidx = wave_sum_multi_index<V>(lane, own);
    const int om = 4 * w + (oidx & 3), on = n0 + (oidx >> 2);
    const bool oval = own && om < M && on < N;
    const int omc = min(om, Ml), onc = min(on, Nl);
    const float eb = *(p.bias ? p.bias + (int64_t)g * p.bias_gs + onc : X);
    const float er = *(p.residual ? p.residual + (int64_t)omc * p.ldr + onc : X);
    const float em = *(p.mul ? p.mul + (int64_t)omc * p.ldmul + onc : X);
    WLoad<WT, E> wv[CW * KW];
#pragma unroll
    for (int c = 0; c < CW; ++c)
#pragma unroll
        for (int s = 0; s < KW; ++s)
            wv[c * KW + s].issue(W + (int64_t)min(n0 + c, Nl) * ldw + E * (lane + 64 * s));
    __builtin_amdgcn_sched_barrier(0);

    if (LN) {
        const float invK = 1.0f / (float)K;
        float s1[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            float a = 0.0f;
#pragma unroll
            for (int s = 0; s < KW; ++s)
#pragma unroll
                for (int q = 0; q < Q; ++q)
                    a += (xv[s][m][q].x + xv[s][m][q].y) + (xv[s][m][q].z + xv[s][m][q].w);
            s1[m] = a;
        }
        bool o4;
        wave_sum_multi<4>(s1, lane, o4);          // value m's total on the lanes with (lane >> 2) & 3 == m
        float mean[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) mean[m] = __shfl(s1[0], 4 * m, 64) * invK;
        float s2[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            float sq = 0.0f;
#pragma unroll
            for (int s = 0; s < KW; ++s)
#pragma unroll
                for (int q = 0; q < Q; ++q) {
                    float4& x = xv[s][m][q];
                    x.x -= mean[m]; x.y -= mean[m]; x.z -= mean[m]; x.w -= mean[m];
                    sq = fmaf(x.x, x.x, sq); sq = fmaf(x.y, x.y, sq); sq = fmaf(x.z, x.z, sq); sq = fmaf(x.w, x.w, sq);
                }
            s2[m] = sq;
        }
        wave_sum_multi<4>(s2, lane, o4);
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const float rstd = __builtin_amdgcn_rsqf(__shfl(s2[0], 4 * m, 64) * invK + p.eps);
#pragma unroll
            for (int s = 0; s < KW; ++s)
#pragma unroll
                for (int q = 0; q < Q; ++q) {
                    float4& x = xv[s][m][q];
                    const float4 gg = LN == 2 ? ls[LN == 2 ? s : 0][m][q] : lg[LN == 2 ? 0 : s][q];
                    const float4 hh = LN == 2 ? lh[LN == 2 ? s : 0][m][q] : lb[LN == 2 ? 0 : s][q];
                    x.x = fmaf(x.x * rstd, gg.x, hh.x); x.y = fmaf(x.y * rstd, gg.y, hh.y);
                    x.z = fmaf(x.z * rstd, gg.z, hh.z); x.w = fmaf(x.w * rstd, gg.w, hh.w);
                }
        }
    }

    float acc[V];
#pragma unroll
    for (int i = 0; i < V; ++i) acc[i] = 0.0f;
#pragma unroll
    for (int c = 0; c < CW; ++c)
#pragma unroll
        for (int s = 0; s < KW; ++s) {
            float4 wq[Q];
            wv[c * KW + s].get(wq);
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                float a = acc[c * 4 + m];
#pragma unroll
                for (int q = 0; q < Q; ++q) {
                    a = fmaf(wq[q].x, xv[s][m][q].x, a); a = fmaf(wq[q].y, xv[s][m][q].y, a);
                    a = fmaf(wq[q].z, xv[s][m][q].z, a); a = fmaf(wq[q].w, xv[s][m][q].w, a);
                }
                acc[c * 4 + m] = a;
            }
        }
    bool own2;
    wave_sum_multi<V>(acc, lane, own2);        // lands where wave_sum_multi_index said
    if (oval) {
        float v = acc[0];
        if (p.bias) v += eb;
        if (p.residual) v += er;
        v = act == ACT_SILU ? v * sigmoid_f(v) : act_fwd(v, act);
        if (p.mul) v *= em;
        p.C[(int64_t)g * p.c_gs + (int64_t)om * p.ldc + on] = v;
    }
}

// ---------------------------------------------------------------------------------------------
// Device-resident state of the sampling loop (generate_images.py:256-345): the host replays captured
// graphs and never reads a token back between them.  int32 control words:
enum DecCtl : int {
    CTL_LEN = 0,     // window index of the token the next decoder step evaluates
    CTL_CUR = 1,     // window index at which the current chunk of beam_width tokens starts
    CTL_DRAW = 2,    // sampling draws made so far (row of the uniform / forced-token / probability-log buffers)
    CTL_CAND = 3,    // candidate chunks of the current chunk position evaluated so far
    CTL_TOK = 4,     // decoder steps since the candidate began = the chunk slot the next draw fills
    CTL_RING = 5,    // tokens in the window step's token ring (the slid window ends in front of it)
    CTL_WORDS = 8
};

// First launch of a step: x[b] = table[ids[b]] + pe[len] (Transformer.py:154-167: embedding + the
// sinusoid of the window index) and, when the stage keeps a per-position table of every projection of
// `cond` (ScaleLayer / ShiftLayer of all layers, models/layers.py:100-153, 258-304: cond depends on
// the token's position alone and the positions of a stage are known before its loop), the copy of
// this position's row of it into the buffer the step's launches read.
__global__ __launch_bounds__(256) void decode_embed_kernel(const int64_t* __restrict__ ids, int B, int D, int V,
                                                           const float* __restrict__ table,
                                                           const float* __restrict__ pe, int* __restrict__ ctl,
                                                           int len_arg, int max_len,
                                                           const float* __restrict__ proj_table, int64_t PD,
                                                           float* __restrict__ x, float* __restrict__ proj_row,
                                                           int* __restrict__ bad) {
    int L = ctl ? ctl[CTL_LEN] : len_arg;
    L = min(max(L, 0), max_len - 1);
    const int64_t nx = (int64_t)B * D / 4, total = nx + PD / 4;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        if (i < nx) {
            const int b = (int)(i / (D / 4)), c = (int)(i - (int64_t)b * (D / 4)) * 4;
            const int64_t id = ids[b];
            float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
            if (id < 0 || id >= V) {
                if (c == 0) atomicExch(bad, 1);
            } else {
                t = ld4(table + id * D + c);
                if (pe) {
                    const float4 q = ld4(pe + (int64_t)L * D + c);
                    t.x += q.x; t.y += q.y; t.z += q.z; t.w += q.w;
                }
            }
            *reinterpret_cast<float4*>(x + (int64_t)b * D + c) = t;
        } else {
            const int64_t j = (i - nx) * 4;
            *reinterpret_cast<float4*>(proj_row + j) = ld4(proj_table + (int64_t)L * PD + j);
        }
    }
    // a step has begun: the draw behind it fills the next slot of the chunk (no workgroup of this launch reads it)
    if (ctl && blockIdx.x == 0 && threadIdx.x == 0) ctl[CTL_TOK] += 1;
}

__device__ __forceinline__ float exp2_fast(float x) { return __builtin_amdgcn_exp2f(x); }
template <int CTRL> __device__ __forceinline__ float dpp_max_step(float x) { return fmaxf(x, dpp_lane<CTRL>(x)); }
__device__ __forceinline__ float wave_max_dpp(float x) {
    x = dpp_max_step<0x140>(x); x = dpp_max_step<0x141>(x); x = dpp_max_step<0x4E>(x); x = dpp_max_step<0xB1>(x);
    x = fmaxf(x, __shfl_xor(x, 16, 64));
    return fmaxf(x, __shfl_xor(x, 32, 64));
}

// One query row per sequence against its cached keys / values: a wave per (sequence, head), the four
// waves of a workgroup on four adjacent heads (they read the same 128-B lines at head dim 8), a lane
// per key.  Rows are loaded without waiting for the length word and masked afterwards; the running
// softmax of a lane's keys is combined over the wave with one DPP maximum and one multi-value sum.
// Contract (tests/test_gpu_decode_attention.py):
//   - with L the attended length, cache rows at or beyond it never reach the result, whatever they hold
//     (NaN included: what is computed from them is selected away, never multiplied by zero) -- that covers
//     the stale slot L of an append, whose key and value come from k_new / v_new (`fresh`), and every load
//     stays inside the max_len rows of the cache;
//   - the length word is clamped, to [0, max_len - 1] when appending (the new row is written to row L of
//     every head and nothing else is) and to [0, max_len] when read-only (nothing is written);
//   - a read-only call whose clamped length is 0 attends no key and its output is not defined (0 / 0); the
//     host-side length is refused in that case.
template <int HD>
__global__ __launch_bounds__(256) void decode_attention_kernel(
    const float* __restrict__ q, const float* __restrict__ k_new, const float* __restrict__ v_new,
    float* __restrict__ kc, float* __restrict__ vc, int64_t bstride, int64_t hstride, int64_t rstride, int H,
    int len_arg, const int* __restrict__ ctl, int max_len, float c2, const float* __restrict__ o_mul,
    int64_t ldmul, float* __restrict__ o) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int hq = (H + 3) >> 2;
    const int n = blockIdx.x / hq, h = (blockIdx.x - n * hq) * 4 + w;
    if (h >= H) return;                      // whole wave; no workgroup barrier below
    const int D = H * HD;
    const bool app = k_new != nullptr;
    const int64_t row = (int64_t)n * D + h * HD;
    // cache row j of head h: n * bstride + h * hstride + j * rstride (row-major rows of H * d floats, or
    // head-major -- DecodeCache's layout: a head's keys contiguous, a wave-level load is one 2-KB run at d = 8)
    float* kb = kc + (int64_t)n * bstride + (int64_t)h * hstride;
    float* vb = vc + (int64_t)n * bstride + (int64_t)h * hstride;
    constexpr int U = HD <= 16 ? 4 : (HD <= 32 ? 2 : 1);     // keys per lane and pass (128 registers of rows)
    float qv[HD], kn[HD], vn[HD];
#pragma unroll
    for (int c = 0; c < HD; c += 4) {
        const float4 a = ld4(q + row + c);
        qv[c] = a.x; qv[c + 1] = a.y; qv[c + 2] = a.z; qv[c + 3] = a.w;
        const float4 b = ld4((app ? k_new : q) + row + c), d = ld4((app ? v_new : q) + row + c);
        kn[c] = b.x; kn[c + 1] = b.y; kn[c + 2] = b.z; kn[c + 3] = b.w;
        vn[c] = d.x; vn[c + 1] = d.y; vn[c + 2] = d.z; vn[c + 3] = d.w;
    }
    float4 kk[U][HD / 4], vv[U][HD / 4];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int j = min(lane + 64 * u, max_len - 1);
#pragma unroll
        for (int c = 0; c < HD / 4; ++c) {
            kk[u][c] = ld4(kb + (int64_t)j * rstride + 4 * c);
            vv[u][c] = ld4(vb + (int64_t)j * rstride + 4 * c);
        }
    }
    const float mq = *(o_mul ? o_mul + (int64_t)n * ldmul + h * HD + min(lane, HD - 1) : q + row);
    int L = ctl ? ctl[CTL_LEN] : len_arg;
    L = min(max(L, 0), app ? max_len - 1 : max_len);
    const int Sk = L + (app ? 1 : 0);
    if (app && lane < HD) {                  // the new row joins the cache (off the critical path)
        kb[(int64_t)L * rstride + lane] = k_new[row + lane];
        vb[(int64_t)L * rstride + lane] = v_new[row + lane];
    }
    float m = -INFINITY, l = 0.0f, ov[HD];
#pragma unroll
    for (int c = 0; c < HD; ++c) ov[c] = 0.0f;
    for (int j0 = 0; j0 < Sk; j0 += 64 * U) {
        if (j0 > 0) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int j = min(j0 + lane + 64 * u, max_len - 1);
#pragma unroll
                for (int c = 0; c < HD / 4; ++c) {
                    kk[u][c] = ld4(kb + (int64_t)j * rstride + 4 * c);
                    vv[u][c] = ld4(vb + (int64_t)j * rstride + 4 * c);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int j = j0 + lane + 64 * u;
            const bool fresh = app && j == L;      // the new row comes from its source, not from the cache
            float dot = 0.0f;
#pragma unroll
            for (int c = 0; c < HD / 4; ++c) {
                dot = fmaf(qv[4 * c], fresh ? kn[4 * c] : kk[u][c].x, dot);
                dot = fmaf(qv[4 * c + 1], fresh ? kn[4 * c + 1] : kk[u][c].y, dot);
                dot = fmaf(qv[4 * c + 2], fresh ? kn[4 * c + 2] : kk[u][c].z, dot);
                dot = fmaf(qv[4 * c + 3], fresh ? kn[4 * c + 3] : kk[u][c].w, dot);
            }
            if (j < Sk) {
                const float t = dot * c2;
                const float mn = fmaxf(m, t);
                const float alpha = exp2_fast(m - mn);
                const float pr = exp2_fast(t - mn);
                l = l * alpha + pr;
#pragma unroll
                for (int c = 0; c < HD / 4; ++c) {
                    ov[4 * c] = fmaf(pr, fresh ? vn[4 * c] : vv[u][c].x, ov[4 * c] * alpha);
                    ov[4 * c + 1] = fmaf(pr, fresh ? vn[4 * c + 1] : vv[u][c].y, ov[4 * c + 1] * alpha);
                    ov[4 * c + 2] = fmaf(pr, fresh ? vn[4 * c + 2] : vv[u][c].z, ov[4 * c + 2] * alpha);
                    ov[4 * c + 3] = fmaf(pr, fresh ? vn[4 * c + 3] : vv[u][c].w, ov[4 * c + 3] * alpha);
                }
                m = mn;
            }
        }
    }
    const float Mx = wave_max_dpp(m);
    const float sc = m == -INFINITY ? 0.0f : exp2_fast(m - Mx);
    // {l, o[0..HD)} summed over the wave together: value number 0 is l, 1 + c is o[c]
    constexpr int NV = HD < 8 ? 8 : (HD < 16 ? 16 : (HD < 32 ? 32 : 64));
    static_assert(HD + 1 <= NV || HD == 64, "");
    if constexpr (HD < 64) {
        float r[NV];
        r[0] = l * sc;
#pragma unroll
        for (int c = 0; c < HD; ++c) r[1 + c] = ov[c] * sc;
#pragma unroll
        for (int c = HD + 1; c < NV; ++c) r[c] = 0.0f;
        bool own;
        const int idx = wave_sum_multi<NV>(r, lane, own);
        // value 0 (l) ends on lane 0 (no bit of its number set); lane c < HD holds o_mul[c]
        const float lt = __shfl(r[0], 0, 64);
        const float mv = __shfl(mq, min(max(idx - 1, 0), HD - 1), 64);
        if (own && idx >= 1 && idx <= HD) {
            const float t = r[0] / lt;
            o[row + idx - 1] = o_mul ? t * mv : t;
        }
    } else {
        float lsum[1] = {l * sc};
        bool own;
        wave_sum_multi<1>(lsum, lane, own);
        float r[64];
#pragma unroll
        for (int c = 0; c < 64; ++c) r[c] = ov[c] * sc;
        const int idx = wave_sum_multi<64>(r, lane, own);
        const float mv = __shfl(mq, idx, 64);
        const float t = r[0] / lsum[0];
        o[row + idx] = o_mul ? t * mv : t;
    }
}

// The head dims decode_attention_kernel is not instantiated for (every other multiple of 4 up to 128): a key's
// channels are shared by G adjacent lanes.  Lane s of a group holds the 16-B chunks s, s + G, s + 2 G, ... of q,
// of the group's keys and values and of the output (the group reads a row as consecutive 16-B pieces); C4 chunks
// per lane bound the head dim at 4 G C4, the head dim itself arrives at run time.  Rows are compact: what follows
// channel d - 1 is the next head's data (or the next row's, or nothing at all), so chunks at or beyond d are not
// loaded and their registers stay 0.  A key's partial dots are summed inside the group by an xor butterfly (every
// lane of the group ends with the same bits), the softmax state is replicated in it.
template <int G, int C4> struct GroupedAttn {
    static constexpr int NG = 64 / G;            // keys a wave covers per load
    static constexpr int U = 16 / C4;            // keys per lane and pass (128 registers of rows, as above)
    static constexpr int KEYS = NG * U;          // keys per wave and pass
    static constexpr int V = 4 * C4;             // output channels per lane
    static constexpr int NF = V * G >= 64 ? V * G / 64 : 1;   // of which it holds the wave totals of NF at the end
};
constexpr int grouped_keys_per_pass(int d) {
    return d < 16 ? GroupedAttn<2, 2>::KEYS : d < 32 ? GroupedAttn<2, 4>::KEYS
         : d < 64 ? GroupedAttn<4, 4>::KEYS : GroupedAttn<4, 8>::KEYS;
}

// Sums V per-lane values over the lanes that hold the same slice of a row (lane bits G ... 32), halving the values a
// lane carries at every step like wave_sum_multi.  Afterwards v[0 .. NF) are the totals of the values number
// group_sum_index<V, G>() ... + NF.  Fixed order: bit-reproducible.
template <int V, int G>
__device__ __forceinline__ void group_sum_multi(float (&v)[V], int lane) {
    static_assert(V >= 1 && V <= 64 && (V & (V - 1)) == 0 && (G == 2 || G == 4), "");
#define QARIG_GROUP_STEP(MASK, N0)                                              \
    if constexpr ((MASK) >= G) {                                                \
        if constexpr ((N0) > 1) {                                               \
            constexpr int n = (N0) / 2;                                         \
            const bool up = (lane & (MASK)) != 0;                               \
            float got[n];                                                       \
            _Pragma("unroll") for (int i = 0; i < n; ++i) {                     \
                const float lo = v[i], hi = v[i + n];       /* values, not a choice between two addresses */ \
                got[i] = __shfl_xor(up ? lo : hi, MASK, 64);                    \
                v[i] = up ? hi : lo;                                            \
            }                                                                   \
            _Pragma("unroll") for (int i = 0; i < n; ++i) v[i] += got[i];       \
        } else {                                                                \
            v[0] += __shfl_xor(v[0], MASK, 64);                                 \
        }                                                                       \
    }
    constexpr int N1 = V, N2 = N1 > 1 ? N1 / 2 : 1, N3 = N2 > 1 ? N2 / 2 : 1, N4 = N3 > 1 ? N3 / 2 : 1,
                  N5 = N4 > 1 ? N4 / 2 : 1;
    QARIG_GROUP_STEP(32, N1)
    QARIG_GROUP_STEP(16, N2)
    QARIG_GROUP_STEP(8, N3)
    QARIG_GROUP_STEP(4, N4)
    QARIG_GROUP_STEP(2, N5)
#undef QARIG_GROUP_STEP
}
// The number of the first value whose total group_sum_multi<V, G> leaves on `lane`; `owner` is true on exactly
// one lane per value and slice.
template <int V, int G>
__device__ __forceinline__ int group_sum_index(int lane, bool& owner) {
    int idx = 0, dup = 0, n = V;
#pragma unroll
    for (int mask = 32; mask >= G; mask >>= 1) {
        if (n > 1) {
            n >>= 1;
            if (lane & mask) idx += n;
        } else {
            dup |= mask;
        }
    }
    owner = (lane & dup) == 0;
    return idx;
}

// decode_attention_kernel's contract, word for word, for 4 <= d <= 4 G C4, d % 4 == 0.
template <int G, int C4>
__global__ __launch_bounds__(256) void decode_attention_grouped_kernel(
    const float* __restrict__ q, const float* __restrict__ k_new, const float* __restrict__ v_new,
    float* __restrict__ kc, float* __restrict__ vc, int64_t bstride, int64_t hstride, int64_t rstride, int H, int d,
    int len_arg, const int* __restrict__ ctl, int max_len, float c2, const float* __restrict__ o_mul,
    int64_t ldmul, float* __restrict__ o) {
    using T = GroupedAttn<G, C4>;
    constexpr int NG = T::NG, U = T::U, V = T::V, NF = T::NF;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int hq = (H + 3) >> 2;
    const int n = blockIdx.x / hq, h = (blockIdx.x - n * hq) * 4 + w;
    if (h >= H) return;                      // whole wave; no workgroup barrier below
    const int s = lane & (G - 1), g = lane / G;
    const bool app = k_new != nullptr;
    const int64_t row = (int64_t)n * H * d + h * d;
    float* kb = kc + (int64_t)n * bstride + (int64_t)h * hstride;
    float* vb = vc + (int64_t)n * bstride + (int64_t)h * hstride;
    // chunks s, s + G, ... below d / 4 are this lane's: the first nch of its C4
    const int nch = (d / 4 - s + G - 1) / G;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 qv[C4], kn[C4], vn[C4];
#pragma unroll
    for (int i = 0; i < C4; ++i) {
        qv[i] = kn[i] = vn[i] = zero4;
        if (i < nch) {
            const int c = 4 * (s + G * i);
            qv[i] = ld4(q + row + c);
            kn[i] = ld4((app ? k_new : q) + row + c);
            vn[i] = ld4((app ? v_new : q) + row + c);
        }
    }
    float4 kk[U][C4], vv[U][C4];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int j = min(g + NG * u, max_len - 1);
#pragma unroll
        for (int i = 0; i < C4; ++i) {
            kk[u][i] = vv[u][i] = zero4;
            if (i < nch) {
                kk[u][i] = ld4(kb + (int64_t)j * rstride + 4 * (s + G * i));
                vv[u][i] = ld4(vb + (int64_t)j * rstride + 4 * (s + G * i));
            }
        }
    }
    // the NF output channels whose wave totals end on this lane, and their o_mul
    bool own;
    const int idx = group_sum_index<V, G>(lane, own);
    int och[NF];
    float mq[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f) {
        const int li = idx + f;
        och[f] = 4 * (s + G * (li >> 2)) + (li & 3);
        if (!own || och[f] >= d) och[f] = -1;
        mq[f] = (o_mul && och[f] >= 0) ? o_mul[(int64_t)n * ldmul + h * d + och[f]] : 1.0f;
    }
    int L = ctl ? ctl[CTL_LEN] : len_arg;
    L = min(max(L, 0), app ? max_len - 1 : max_len);
    const int Sk = L + (app ? 1 : 0);
    if (app) {                               // the new row joins the cache (off the critical path)
        for (int c = lane; c < d; c += 64) {
            kb[(int64_t)L * rstride + c] = k_new[row + c];
            vb[(int64_t)L * rstride + c] = v_new[row + c];
        }
    }
    float m = -INFINITY, l = 0.0f;
    float4 ov[C4];
#pragma unroll
    for (int i = 0; i < C4; ++i) ov[i] = zero4;
    for (int j0 = 0; j0 < Sk; j0 += T::KEYS) {
        if (j0 > 0) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int j = min(j0 + g + NG * u, max_len - 1);
#pragma unroll
                for (int i = 0; i < C4; ++i) {
                    if (i < nch) {
                        kk[u][i] = ld4(kb + (int64_t)j * rstride + 4 * (s + G * i));
                        vv[u][i] = ld4(vb + (int64_t)j * rstride + 4 * (s + G * i));
                    }
                }
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int j = j0 + g + NG * u;
            const bool fresh = app && j == L;      // the new row comes from its source, not from the cache
            float dot = 0.0f;
#pragma unroll
            for (int i = 0; i < C4; ++i) {         // chunks at or beyond d: 0 * 0, never loaded
                dot = fmaf(qv[i].x, fresh ? kn[i].x : kk[u][i].x, dot);
                dot = fmaf(qv[i].y, fresh ? kn[i].y : kk[u][i].y, dot);
                dot = fmaf(qv[i].z, fresh ? kn[i].z : kk[u][i].z, dot);
                dot = fmaf(qv[i].w, fresh ? kn[i].w : kk[u][i].w, dot);
            }
            dot += dpp_lane<0xB1>(dot);            // quad_perm [1,0,3,2]: the group's other lane(s)
            if constexpr (G == 4) dot += dpp_lane<0x4E>(dot);      // quad_perm [2,3,0,1]
            if (j < Sk) {
                const float t = dot * c2;
                const float mn = fmaxf(m, t);
                const float alpha = exp2_fast(m - mn);
                const float pr = exp2_fast(t - mn);
                l = l * alpha + pr;
#pragma unroll
                for (int i = 0; i < C4; ++i) {
                    ov[i].x = fmaf(pr, fresh ? vn[i].x : vv[u][i].x, ov[i].x * alpha);
                    ov[i].y = fmaf(pr, fresh ? vn[i].y : vv[u][i].y, ov[i].y * alpha);
                    ov[i].z = fmaf(pr, fresh ? vn[i].z : vv[u][i].z, ov[i].z * alpha);
                    ov[i].w = fmaf(pr, fresh ? vn[i].w : vv[u][i].w, ov[i].w * alpha);
                }
                m = mn;
            }
        }
    }
    const float Mx = wave_max_dpp(m);
    const float sc = m == -INFINITY ? 0.0f : exp2_fast(m - Mx);
    float lt = l * sc;                       // replicated in a group: summed over the groups only
#pragma unroll
    for (int mask = 32; mask >= G; mask >>= 1) lt += __shfl_xor(lt, mask, 64);
    float r[V];
#pragma unroll
    for (int i = 0; i < C4; ++i) {
        r[4 * i] = ov[i].x * sc; r[4 * i + 1] = ov[i].y * sc; r[4 * i + 2] = ov[i].z * sc; r[4 * i + 3] = ov[i].w * sc;
    }
    group_sum_multi<V, G>(r, lane);
#pragma unroll
    for (int f = 0; f < NF; ++f) {
        if (och[f] >= 0) {
            const float t = r[f] / lt;
            o[row + och[f]] = o_mul ? t * mq[f] : t;
        }
    }
}

__device__ __forceinline__ int wave_min_int(int x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x = min(x, __shfl_xor(x, o, 64));
    return x;
}
__device__ __forceinline__ int wave_max_int(int x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x = max(x, __shfl_xor(x, o, 64));
    return x;
}

// One sampling draw per row, as generate_images.py:289-304 makes it (train_quantized_transformer.py:
// 626-636 in "train" mode): probs = softmax(logits / T); generate mode zeroes the <end> probability;
// a token is drawn in proportion to probs -- by inverse CDF from ONE uniform of the caller's generator
// (torch.multinomial consumes its generator differently: the same distribution, not the same stream) --
// the running product of the chosen probabilities is updated, train mode maps a drawn <end> to 0, and the
// token (+ shift: the base stage's vocabulary offset) is appended: to ids (the next step's input) and to
// slot `slot` of the row's chunk.  forced (optional, >= 0 entries): tokens to take instead of drawing
// (tests replay the reference's recorded draws); probs_log (optional): receives the row it sampled from.
// A wave per row; every sum runs in a fixed order.
__global__ __launch_bounds__(64) void decode_sample_kernel(
    const float* __restrict__ logits, int64_t ldl, int B, int V, float temperature, int end_token,
    int generate_mode, int64_t shift, const float* __restrict__ uniforms, const int64_t* __restrict__ forced,
    int* __restrict__ ctl, int slot, int bw, int max_draws, int inc_len, int beams, int64_t* __restrict__ ids,
    int64_t* __restrict__ chunk, float* __restrict__ comb, float* __restrict__ probs_log) {
    __shared__ float part[64];
    const int b = blockIdx.x, lane = threadIdx.x;
    if (slot < 0) slot = min(max(ctl[CTL_TOK], 0), bw - 1);     // the slot the device counts
    // beams == 0: row b draws from column b of draw row ctl[2] + slot (B columns).  beams > 0: the rows are
    // `beams` candidate chunks per image evaluated as one batch, and every draw keeps the number the reference's
    // candidate-after-candidate loop gives it (generate_images.py:262-304): row b = image * beams + candidate
    // reads column `image` of draw row ctl[2] + candidate * bw + slot (B / beams columns)
    const int dcol = beams > 0 ? b / beams : b, dcols = beams > 0 ? B / beams : B;
    const int d = min(max(ctl[CTL_DRAW] + (beams > 0 ? (b - dcol * beams) * bw : 0) + slot, 0), max_draws - 1);
    const float* z = logits + (int64_t)b * ldl;
    const int per = (V + 63) / 64, i0 = min(V, lane * per), i1 = min(V, i0 + per);
    float mx = -INFINITY;
    for (int i = i0; i < i1; ++i) mx = fmaxf(mx, z[i] / temperature);
    mx = wave_max_dpp(mx);
    float s[1] = {0.0f};
    for (int i = i0; i < i1; ++i) s[0] += expf(z[i] / temperature - mx);
    bool own;
    wave_sum_multi<1>(s, lane, own);
    const float S = s[0];
    auto prob = [&](int i) {
        const float pr = expf(z[i] / temperature - mx) / S;
        return (generate_mode && i == end_token) ? 0.0f : pr;
    };
    float ps = 0.0f;
    int last_nz = -1;
    float* lg = probs_log ? probs_log + ((int64_t)d * dcols + dcol) * V : nullptr;
    for (int i = i0; i < i1; ++i) {
        const float pr = prob(i);
        ps += pr;
        if (pr > 0.0f) last_nz = i;
        if (lg) lg[i] = pr;
    }
    part[lane] = ps;
    __syncthreads();
    float base = 0.0f, total = 0.0f;
    for (int k = 0; k < 64; ++k) {
        if (k == lane) base = total;
        total += part[k];
    }
    const float target = uniforms[(int64_t)d * dcols + dcol] * total;
    int cand = 0x7fffffff;
    float run = base;
    for (int i = i0; i < i1; ++i) {
        const float pr = prob(i);
        run += pr;
        if (pr > 0.0f && run > target && cand == 0x7fffffff) cand = i;
    }
    cand = wave_min_int(cand);
    const int fallback = wave_max_int(last_nz);       // rounding left the target at or past the total
    int64_t nxt = cand == 0x7fffffff ? max(fallback, 0) : cand;
    if (forced) {
        const int64_t f = forced[(int64_t)d * dcols + dcol];
        if (f >= 0 && f < V) nxt = f;
    }
    if (lane == 0) {
        comb[b] *= prob((int)nxt);
        if (!generate_mode && nxt == end_token) nxt = 0;      // reference HACK: <end> -> index 0
        ids[b] = nxt + shift;
        chunk[(int64_t)b * bw + slot] = nxt + shift;
        if (b == 0 && inc_len) ctl[CTL_LEN] += 1;             // no other workgroup of this launch reads it
    }
}

// ---- decode_sample_kernel's draw from a top-k / nucleus (top-p) filtered row -----------------------------------
// A workgroup of four waves per row.  The row is staged ONCE in LDS (logits / T coalesced in, then exp, then the
// probabilities -- one expf and one division per entry); thread t owns the contiguous entries [t per, (t + 1) per)
// with per odd, so the 64 lanes of a wave read 64 different banks.  Every workgroup-wide sum has one shape: the
// thread's entries in index order, a fixed butterfly over the wave (wave_sum_multi), the four wave totals in wave
// order -- at most 129 + 6 + 4 roundings at V = 32,768 (65 + 6 + 4 at 16,385): 8e-6 of the total at worst, run-to-
// run bit-reproducible.  Two slots per hand-over buffer, used alternately: one barrier per sum.
constexpr int SF_THREADS = 256;
constexpr int SF_MAX_V = 32768;       // 128 KB of the 160 KB of LDS; a larger V is refused by the entry point

template <int NV>
__device__ __forceinline__ void sf_block_sum(float (&v)[NV], float (*red)[4][4], int& phase, int lane, int w) {
    bool own;
    const int idx = wave_sum_multi<NV>(v, lane, own);
    float (*r)[4] = red[phase & 1];
    ++phase;
    if (own) r[w][idx] = v[0];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NV; ++j) v[j] = ((r[0][j] + r[1][j]) + r[2][j]) + r[3][j];
}

// Number of x over the threads in front of this one (thread order = index order of the entries they own).
__device__ __forceinline__ int sf_block_rank(int x, int (*ired)[4][2], int& phase, int lane, int w) {
    int inc = x;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(inc, o, 64);
        if (lane >= o) inc += y;
    }
    int (*r)[2] = ired[phase & 1];
    ++phase;
    if (lane == 63) r[w][0] = inc;
    __syncthreads();
    int off = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k)
        if (k < w) off += r[k][0];
    return off + inc - x;
}

// The largest T with f(T) >= want, f(T) = the number (MASS: the sum) of the entries whose bits are >= T.  The
// entries are non-negative floats, so the order of their uint32 images is their order, and at most 1: bits 29..0
// decide.  Two bits per round -- three candidates counted in one pass over the row, fifteen rounds, no sort.
// f does not increase with T, in fp32 too: a candidate's sum runs over a subset of the next lower one's
// non-negative terms in the same order.
template <bool MASS>
__device__ __forceinline__ uint32_t sf_threshold(const float* row, int i0, int i1, float want, float (*red)[4][4],
                                                 int& phase, int lane, int w) {
    uint32_t T = 0;
    for (int sh = 28; sh >= 0; sh -= 2) {
        const uint32_t c1 = T | (1u << sh), c2 = T | (2u << sh), c3 = T | (3u << sh);
        float a[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 4
        for (int i = i0; i < i1; ++i) {
            const float x = row[i];
            const uint32_t u = __float_as_uint(x);
            const float y = MASS ? x : 1.0f;
            a[0] += u >= c1 ? y : 0.0f;
            a[1] += u >= c2 ? y : 0.0f;
            a[2] += u >= c3 ? y : 0.0f;
        }
        sf_block_sum<4>(a, red, phase, lane, w);
        T = a[2] >= want ? c3 : (a[1] >= want ? c2 : (a[0] >= want ? c1 : T));
    }
    return T;
}

// qarig_decode_sample_filtered (include/qarig.h).  probs as decode_sample_kernel computes them; then only zeroing:
//   top_k > 0: the top_k largest non-zero entries stay (the k-th largest value T by sf_threshold on counts; the
//              entries equal to T stay in index order until top_k are kept); fewer non-zero entries: nothing to do;
//   top_p < 1: of what is left, in descending order (equal entries: lower index first) an entry stays iff the mass
//              strictly in front of it is < top_p * (mass left) -- T by sf_threshold on sums: the largest T with
//              sum(entries >= T) >= top_p * total, so sum(entries > T) < top_p * total and the first entry equal to
//              T always stays; the r-th one stays iff sum(entries > T) + r T is still below.
// Kept entries keep their values (no renormalisation: the draw scales its target by the row's total).  From there
// on decode_sample_kernel's statements on the filtered row: the inverse-CDF draw, the last non-zero entry when
// rounding leaves the target at or past the total, forced tokens (taken whether or not they were kept -- comb then
// takes the filtered value, possibly 0), the product, the train-mode <end> -> 0, the counters, the draw numbers.
__global__ __launch_bounds__(SF_THREADS) void decode_sample_filtered_kernel(
    const float* __restrict__ logits, int64_t ldl, int B, int V, float temperature, int end_token,
    int generate_mode, int64_t shift, const float* __restrict__ uniforms, const int64_t* __restrict__ forced,
    int* __restrict__ ctl, int slot, int bw, int max_draws, int inc_len, int beams, int64_t* __restrict__ ids,
    int64_t* __restrict__ chunk, float* __restrict__ comb, float* __restrict__ probs_log, int top_k, float top_p) {
    extern __shared__ float sf_row[];           // V floats
    __shared__ float red[2][4][4];
    __shared__ int ired[2][4][2];
    __shared__ float part[SF_THREADS];
    __shared__ float wtot[4];
    float* row = sf_row;
    const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
    int phase = 0;
    if (slot < 0) slot = min(max(ctl[CTL_TOK], 0), bw - 1);
    const int dcol = beams > 0 ? b / beams : b, dcols = beams > 0 ? B / beams : B;
    const int d = min(max(ctl[CTL_DRAW] + (beams > 0 ? (b - dcol * beams) * bw : 0) + slot, 0), max_draws - 1);
    const float* z = logits + (int64_t)b * ldl;
    float mx = -INFINITY;
    for (int i = t; i < V; i += SF_THREADS) {
        const float x = z[i] / temperature;
        row[i] = x;
        mx = fmaxf(mx, x);
    }
    mx = wave_max_dpp(mx);
    {
        float (*r)[4] = red[phase & 1];
        ++phase;
        if (lane == 0) r[w][0] = mx;
        __syncthreads();                        // the staged row is whole, too
        mx = fmaxf(fmaxf(r[0][0], r[1][0]), fmaxf(r[2][0], r[3][0]));
    }
    const int per = ((V + SF_THREADS - 1) / SF_THREADS) | 1;
    const int i0 = min(V, t * per), i1 = min(V, i0 + per);
    float s[1] = {0.0f};
#pragma unroll 4
    for (int i = i0; i < i1; ++i) {
        const float e = expf(row[i] - mx);
        row[i] = e;
        s[0] += e;
    }
    sf_block_sum<1>(s, red, phase, lane, w);
    const float S = s[0];
    float nz[1] = {0.0f};
#pragma unroll 4
    for (int i = i0; i < i1; ++i) {
        float pr = row[i] / S;
        if (generate_mode && i == end_token) pr = 0.0f;
        row[i] = pr;
        nz[0] += pr > 0.0f ? 1.0f : 0.0f;
    }
    if (top_k > 0) {
        sf_block_sum<1>(nz, red, phase, lane, w);         // counts are whole numbers below 2^24: exact
        if ((float)top_k < nz[0]) {
            const uint32_t T = sf_threshold<false>(row, i0, i1, (float)top_k, red, phase, lane, w);
            float gt[1] = {0.0f};
            int eq = 0;
#pragma unroll 4
            for (int i = i0; i < i1; ++i) {
                const uint32_t u = __float_as_uint(row[i]);
                gt[0] += u > T ? 1.0f : 0.0f;
                eq += u == T ? 1 : 0;
            }
            sf_block_sum<1>(gt, red, phase, lane, w);
            const int ties = top_k - (int)gt[0];
            int rank = sf_block_rank(eq, ired, phase, lane, w);
            for (int i = i0; i < i1; ++i) {
                const uint32_t u = __float_as_uint(row[i]);
                if (u < T) row[i] = 0.0f;
                else if (u == T) {
                    if (rank >= ties) row[i] = 0.0f;
                    ++rank;
                }
            }
        }
    }
    if (top_p < 1.0f) {
        float m[1] = {0.0f};
#pragma unroll 4
        for (int i = i0; i < i1; ++i) m[0] += row[i];
        sf_block_sum<1>(m, red, phase, lane, w);
        const float want = top_p * m[0];
        const uint32_t T = sf_threshold<true>(row, i0, i1, want, red, phase, lane, w);
        const float tv = __uint_as_float(T);
        float gt[1] = {0.0f};
        int eq = 0;
#pragma unroll 4
        for (int i = i0; i < i1; ++i) {
            const float x = row[i];
            const uint32_t u = __float_as_uint(x);
            gt[0] += u > T ? x : 0.0f;
            eq += u == T ? 1 : 0;
        }
        sf_block_sum<1>(gt, red, phase, lane, w);
        int rank = sf_block_rank(eq, ired, phase, lane, w);
        for (int i = i0; i < i1; ++i) {
            const uint32_t u = __float_as_uint(row[i]);
            if (u < T) row[i] = 0.0f;
            else if (u == T) {
                if (rank > 0 && !(fmaf((float)rank, tv, gt[0]) < want)) row[i] = 0.0f;
                ++rank;
            }
        }
    }
    // ---- the draw, on the filtered row
    float ps = 0.0f;
    int last_nz = -1;
#pragma unroll 4
    for (int i = i0; i < i1; ++i) {
        const float pr = row[i];
        ps += pr;
        if (pr > 0.0f) last_nz = i;
    }
    part[t] = ps;
    __syncthreads();                            // the filtered row is whole
    if (probs_log) {
        float* lg = probs_log + ((int64_t)d * dcols + dcol) * V;
        for (int i = t; i < V; i += SF_THREADS) lg[i] = row[i];
    }
    float base = 0.0f, wsum = 0.0f;
    for (int k = 0; k < 64; ++k) {
        if (k == lane) base = wsum;
        wsum += part[64 * w + k];
    }
    if (lane == 0) wtot[w] = wsum;
    __syncthreads();
    float off = 0.0f, total = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (k == w) off = total;
        total += wtot[k];
    }
    const float target = uniforms[(int64_t)d * dcols + dcol] * total;
    int cand = 0x7fffffff;
    float run = off + base;
#pragma unroll 4
    for (int i = i0; i < i1; ++i) {
        const float pr = row[i];
        run += pr;
        if (pr > 0.0f && run > target && cand == 0x7fffffff) cand = i;
    }
    cand = wave_min_int(cand);
    int fallback = wave_max_int(last_nz);         // rounding left the target at or past the total
    {
        int (*r)[2] = ired[phase & 1];
        ++phase;
        if (lane == 0) { r[w][0] = cand; r[w][1] = fallback; }
        __syncthreads();
        cand = min(min(r[0][0], r[1][0]), min(r[2][0], r[3][0]));
        fallback = max(max(r[0][1], r[1][1]), max(r[2][1], r[3][1]));
    }
    if (t == 0) {
        int64_t nxt = cand == 0x7fffffff ? max(fallback, 0) : cand;
        if (forced) {
            const int64_t f = forced[(int64_t)d * dcols + dcol];
            if (f >= 0 && f < V) nxt = f;
        }
        comb[b] *= row[nxt];
        if (!generate_mode && nxt == end_token) nxt = 0;      // reference HACK: <end> -> index 0
        ids[b] = nxt + shift;
        chunk[(int64_t)b * bw + slot] = nxt + shift;
        if (b == 0 && inc_len) ctl[CTL_LEN] += 1;             // no other workgroup of this launch reads it
    }
}

// After a candidate chunk (all rows have drawn beam_width tokens): per image, the beam with the largest
// probability product (first one on ties: torch.argmax) competes with the best chunk kept so far --
// generate_images.py:325-337 keeps the earlier candidate unless the new product is larger -- and the
// counters move on: next candidate, the draws it consumed, the cache position back at the chunk start.
// take[n] = 1 + winning beam when the new chunk replaces the kept one, else 0.
__global__ __launch_bounds__(64) void decode_decide_kernel(int* __restrict__ ctl, int N, int NB, int bw, int draws,
                                                           float* __restrict__ comb,
                                                           const int64_t* __restrict__ chunk,
                                                           float* __restrict__ best_p,
                                                           int64_t* __restrict__ best_chunk,
                                                           int* __restrict__ take) {
    const int cand = ctl[CTL_CAND];
    for (int n = threadIdx.x; n < N; n += 64) {
        int pb = 0;
        float c = comb[(int64_t)n * NB];
        for (int k = 1; k < NB; ++k)
            if (comb[(int64_t)n * NB + k] > c) { c = comb[(int64_t)n * NB + k]; pb = k; }
        const bool tk = cand == 0 || !(best_p[n] >= c);
        take[n] = tk ? pb + 1 : 0;
        if (tk) {
            best_p[n] = c;
            for (int j = 0; j < bw; ++j) best_chunk[(int64_t)n * bw + j] = chunk[((int64_t)n * NB + pb) * bw + j];
        }
        for (int k = 0; k < NB; ++k) comb[(int64_t)n * NB + k] = 1.0f;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        ctl[CTL_CAND] = cand + 1;
        ctl[CTL_DRAW] += draws;
        ctl[CTL_LEN] = ctl[CTL_CUR];
        ctl[CTL_TOK] = 0;
    }
}

// Cache rows [cur, cur + R) of every layer, keys and values: restore == 0 saves the winning beam's rows
// of the images whose chunk was just kept (take[n] > 0) into the staging copy; restore == 1 writes the
// staged rows into EVERY beam of every image (the kept chunk becomes the common prefix).
// kv (layers * 2, N * NB, H, max_len, d) head-major; staged (layers * 2, N, H, R, d).
__global__ __launch_bounds__(256) void decode_rows_kernel(const int* __restrict__ ctl, float* __restrict__ kv,
                                                          float* __restrict__ staged,
                                                          const int* __restrict__ take, int layers2, int N,
                                                          int NB, int H, int R, int d, int max_len, int restore) {
    const int cur = ctl[CTL_CUR];
    const int64_t dq = d / 4;
    const int64_t per = (restore ? (int64_t)NB : 1) * H * R * dq;
    const int64_t total = (int64_t)layers2 * N * per;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        int64_t r_ = i;
        const int c = (int)(r_ % dq); r_ /= dq;
        const int r = (int)(r_ % R); r_ /= R;
        const int h = (int)(r_ % H); r_ /= H;
        int bm = 0;
        if (restore) { bm = (int)(r_ % NB); r_ /= NB; }
        const int n = (int)(r_ % N);
        const int l2 = (int)(r_ / N);
        const int row = cur + r;
        if (row < 0 || row >= max_len) continue;
        float* st = staged + ((((int64_t)l2 * N + n) * H + h) * R + r) * d + 4 * c;
        if (restore) {
            float* dst = kv + ((((int64_t)l2 * N * NB + (int64_t)n * NB + bm) * H + h) * max_len + row) * d + 4 * c;
            *reinterpret_cast<float4*>(dst) = ld4(st);
        } else {
            const int tk = take[n];
            if (tk <= 0) continue;
            const float* src = kv + ((((int64_t)l2 * N * NB + (int64_t)n * NB + (tk - 1)) * H + h) * max_len + row) * d + 4 * c;
            *reinterpret_cast<float4*>(st) = ld4(src);
        }
    }
}

// Prefix prefill: the keys and values a batched pass over the prefix produced, token-major k / v
// (images, P1, H * d) with row stride ld and image stride bs (floats), into rows [0, P1) of one layer of the
// head-major cache kv (2, images * NB, H, max_len, d) -- every candidate row of an image gets the same rows.
// One 16-B load per item, NB 16-B stores; consecutive lanes walk a head's rows, so the stores of a wave are one run.
__global__ __launch_bounds__(256) void decode_cache_fill_kernel(const float* __restrict__ k,
                                                                const float* __restrict__ v, int64_t ld, int64_t bs,
                                                                float* __restrict__ kv, int images, int NB, int H,
                                                                int d, int P1, int max_len) {
    const int64_t dq = d / 4;
    const int64_t per = (int64_t)H * P1 * dq;
    const int64_t total = 2 * (int64_t)images * per;
    const int64_t half = (int64_t)images * NB * H * max_len * d;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        int64_t r_ = i;
        const int c = (int)(r_ % dq); r_ /= dq;
        const int t = (int)(r_ % P1); r_ /= P1;
        const int h = (int)(r_ % H); r_ /= H;
        const int n = (int)(r_ % images);
        const int hv = (int)(r_ / images);
        const float* src = (hv ? v : k) + (int64_t)n * bs + (int64_t)t * ld + (int64_t)h * d + 4 * c;
        const float4 val = ld4(src);
        float* dst = kv + hv * half + ((((int64_t)n * NB) * H + h) * max_len + t) * d + 4 * c;
        for (int b = 0; b < NB; ++b)
            *reinterpret_cast<float4*>(dst + (int64_t)b * H * max_len * d) = val;
    }
}

// The kept chunk becomes part of the sequence: tokens[n][cur + j] = best_chunk[n][j]; its last token is
// the input of the step that produces the next chunk's first logits, at window index cur + bw - 1.
__global__ __launch_bounds__(64) void decode_commit_kernel(int* __restrict__ ctl, int N, int NB, int bw,
                                                           const int64_t* __restrict__ best_chunk,
                                                           int64_t* __restrict__ tokens, int64_t ldt,
                                                           int64_t* __restrict__ ids) {
    const int cur = ctl[CTL_CUR];
    for (int n = threadIdx.x; n < N; n += 64) {
        for (int j = 0; j < bw; ++j)
            if (cur + j >= 0 && cur + j < ldt) tokens[(int64_t)n * ldt + cur + j] = best_chunk[(int64_t)n * bw + j];
        for (int k = 0; k < NB; ++k) ids[(int64_t)n * NB + k] = best_chunk[(int64_t)n * bw + bw - 1];
    }
    __syncthreads();
    if (threadIdx.x == 0) ctl[CTL_LEN] = cur + bw - 1;
}

// Behind that step: the next chunk starts.
__global__ void decode_advance_kernel(int* __restrict__ ctl, int bw) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        ctl[CTL_CUR] += bw;
        ctl[CTL_LEN] = ctl[CTL_CUR];
        ctl[CTL_CAND] = 0;
        ctl[CTL_TOK] = 0;
    }
}

// ---------------------------------------------------------------------------------------------
// The slid window (generate_images.py:275-290) from the device-resident token ring: the window is the
// W1 = window - 1 tokens in front of ring length n = ctl[CTL_RING], start = n - W1.  Token s of sequence r:
// x[r][s] = E[ring[r][start + s]] + pe[s] (pe row s: the window-relative sinusoid of position s + 1,
// Transformer.py:154-167) and its row of the stage's conditioning table: the absolute position of ring
// column j -- 0 for the first token, j + pos_off behind it (the numbering the loop appends).  Wp = W1 + 1
// adds the duplicate of the last token that makes R x Wp whole 128-row tiles.  Ids outside [0, V),
// positions outside [0, P) and a window start outside the ring set *bad and are clamped: never dereferenced.
__global__ __launch_bounds__(256) void window_assemble_kernel(
    const int64_t* __restrict__ ring, int64_t ldr, const int* __restrict__ ctl, int R, int W1, int Wp, int D, int V,
    const float* __restrict__ table, const float* __restrict__ pe, int P, int pos_off, float* __restrict__ x,
    int* __restrict__ rowmap, int* __restrict__ last_map, int* __restrict__ bad) {
    int start = ctl[CTL_RING] - W1;
    if (start < 0 || (int64_t)start + W1 > ldr) {
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicExch(bad, 1);
        start = (int)min(max((int64_t)start, (int64_t)0), ldr - W1);
    }
    const int dq = D / 4;
    const int64_t total = (int64_t)R * Wp * dq;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t t = i / dq;                     // token row r * Wp + s
        const int c = (int)(i - t * dq) * 4;
        const int r = (int)(t / Wp), s = (int)(t - (int64_t)r * Wp);
        const int j = start + min(s, W1 - 1);         // the pad row repeats the last token and its position
        const int64_t id = ring[(int64_t)r * ldr + j];
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (id < 0 || id >= V) {
            if (c == 0) atomicExch(bad, 1);
        } else {
            v = ld4(table + id * D + c);
            const float4 q = ld4(pe + (int64_t)s * D + c);
            v.x += q.x; v.y += q.y; v.z += q.z; v.w += q.w;
        }
        *reinterpret_cast<float4*>(x + t * D + c) = v;
        if (c == 0 && rowmap) {
            int p = j == 0 ? 0 : j + pos_off;
            if (p < 0 || p >= P) {
                atomicExch(bad, 1);
                p = min(max(p, 0), P - 1);
            }
            rowmap[t] = p;
            if (last_map && s == W1 - 1) last_map[r] = p;
        }
    }
}

// The sampled ids join the ring: ring[b][n] = ids[b], n = ctl[CTL_RING] += 1 (the host's torch.cat of
// generate_images.py:306-310).  A column outside the ring sets *bad and writes nothing.
__global__ __launch_bounds__(64) void window_append_kernel(int* __restrict__ ctl, const int64_t* __restrict__ ids,
                                                           int64_t* __restrict__ ring, int B, int64_t ldr,
                                                           int* __restrict__ bad) {
    const int n = ctl[CTL_RING];
    const bool ok = n >= 0 && n < ldr;
    for (int b = threadIdx.x; b < B; b += 64)
        if (ok) ring[(int64_t)b * ldr + n] = ids[b];
    if (!ok && threadIdx.x == 0) atomicExch(bad, 1);
    __syncthreads();
    if (threadIdx.x == 0) ctl[CTL_RING] = n + 1;
}
}  // namespace qarig

using namespace qarig;

// Shapes the streaming kernel takes: M <= 16 rows, K/4 in {64, 128, 256} or K in {2048, 4096};
// a LayerNorm prologue only with K <= 1024 (a workgroup's threads cover whole rows).
extern "C" int qarig_decode_linear_supported(int M, int N, int K, int ln) {
    if (M < 1 || M > 16 || N < 1 || K < 256) return 0;
    if (K == 256 || K == 512 || K == 1024) return 1;
    return (K == 2048 || K == 4096) && !ln;
}

template <typename WT>
struct DecLinHead { const float* X; const WT* W; int64_t ldx, ldw; int M, N, K, act; int64_t x_gs, w_gs; };

// E weights per load: kq = K/E units per row.  bf16 images take E = 8 (16-B loads) except at K = 256, where 8-B loads
// keep 64 lanes on a row (E = 4: the fp32 mapping of K = 256); E = 4 is instantiated for that K alone.
template <typename WT, int E, int MR, int LN>
static void launch_decode_linear(const DecLinHead<WT>& h, const DecLin& p, int groups, hipStream_t st) {
    constexpr bool f32 = sizeof(WT) == 4;
    const int kq = h.K / E;
    auto grid = [&](int cw) { return dim3((h.N + cw - 1) / cw, groups); };
    auto wgs = [&](int cw) { return (int64_t)((h.N + cw - 1) / cw) * groups; };
#define QARIG_DL(J, KS, CW)                                                                                         \
    hipLaunchKernelGGL((decode_linear_kernel<WT, E, MR, LN, J, KS>), grid(CW), dim3(256), 0, st, h.X, h.W, h.ldx, h.ldw, \
                       h.M, h.N, h.K, h.act, h.x_gs, h.w_gs, p)
    if (kq <= 256) {
        const int CG = 256 / kq;
        // 16 KB of weights (fp32; 4 load passes) per workgroup while that leaves >= 256 workgroups, else fewer
        // (16 rows of per-row AdaLN operands leave no registers for four loads)
        if constexpr (!(MR == 16 && LN == 2)) {
            if (wgs(4 * CG) >= 256) { QARIG_DL(4, 1, 4 * CG); return; }
        }
        if (wgs(2 * CG) >= 256) QARIG_DL(2, 1, 2 * CG);
        else QARIG_DL(1, 1, CG);
    } else if constexpr (LN == 0 && (f32 || E == 8)) {
        if (kq == 512) {
            if (wgs(2) >= 256) QARIG_DL(4, 2, 2);
            else QARIG_DL(2, 2, 1);
        } else if constexpr (f32) {
            QARIG_DL(4, 4, 1);
        }
    }
#undef QARIG_DL
}

/* C-ABI: see include/qarig.h */
// 5 ... 16 rows, K <= 512 E: the row-split kernel.  CW columns per workgroup: 16 load passes while that leaves
// >= 256 workgroups, else a quarter of it.
template <typename WT, int E, int LN>
static bool launch_decode_linear_rows(const DecLinHead<WT>& h, const DecLin& p, int groups, hipStream_t st) {
    constexpr bool f32 = sizeof(WT) == 4;
    const int kw = h.K / (64 * E);
    // one wave per 4 rows; <= 4 rows: single-wave workgroups, so four times the workgroups for the bytes per CU
    const int threads = 64 * ((h.M + 3) / 4);
    const int64_t want = h.M <= 4 ? 1024 : 256;
    auto wgs = [&](int cw) { return (int64_t)((h.N + cw - 1) / cw) * groups; };
#define QARIG_DR(CW, KW)                                                                                      \
    hipLaunchKernelGGL((decode_linear_rows_kernel<WT, E, LN, CW, KW>), dim3((h.N + CW - 1) / CW, groups), dim3(threads), \
                       0, st, h.X, h.W, h.ldx, h.ldw, h.M, h.N, h.K, h.act, h.x_gs, h.w_gs, p)
    if (kw == 1) {
        if (wgs(16) >= want) QARIG_DR(16, 1); else QARIG_DR(4, 1);
        return true;
    }
    if constexpr (f32 || E == 8) {
        switch (kw) {
            case 2: if (wgs(8) >= want) QARIG_DR(8, 2); else QARIG_DR(2, 2); return true;
            case 4:         // a bf16 row of 4 chunks is K = 2048: no LayerNorm form (qarig_decode_linear_supported)
                if constexpr (f32 || LN == 0) {
                    if (wgs(4) >= want) QARIG_DR(4, 4); else QARIG_DR(1, 4);
                    return true;
                }
                return false;
            case 8:
                if constexpr (LN == 0) {
                    if (wgs(2) >= want) QARIG_DR(2, 8); else QARIG_DR(1, 8);
                    return true;
                }
                return false;
            default: return false;
        }
    }
    return false;
#undef QARIG_DR
}

template <typename WT, int E, int MR>
static void launch_decode_linear_ln(int ln, const DecLinHead<WT>& h, const DecLin& p, int groups, hipStream_t st) {
    switch (ln) {
        case 0: launch_decode_linear<WT, E, MR, 0>(h, p, groups, st); break;
        case 1: launch_decode_linear<WT, E, MR, 1>(h, p, groups, st); break;
        case 2: launch_decode_linear<WT, E, MR, 2>(h, p, groups, st); break;
        default: launch_decode_linear<WT, E, MR, 3>(h, p, groups, st); break;
    }
}

template <typename WT, int E>
static bool launch_decode_linear_rows_ln(int ln, const DecLinHead<WT>& h, const DecLin& p, int groups, hipStream_t st) {
    switch (ln) {
        case 0: return launch_decode_linear_rows<WT, E, 0>(h, p, groups, st);
        case 1: return launch_decode_linear_rows<WT, E, 1>(h, p, groups, st);
        case 2: return launch_decode_linear_rows<WT, E, 2>(h, p, groups, st);
        default: return launch_decode_linear_rows<WT, E, 3>(h, p, groups, st);
    }
}

// The two entry points below: WA = weight elements per 16 B (strides and the group stride are multiples of it).
template <typename WT>
static int decode_linear_entry(const float* X, int64_t ldx, int64_t x_gs, float eps, const float* gamma,
                               const float* beta, const float* scale, const float* shift, int64_t ldmod, const WT* W,
                               int64_t ldw, int64_t w_gs, const float* bias, int64_t bias_gs, const float* residual,
                               int64_t ldr, const float* mul, int64_t ldmul, float* C, int64_t ldc, int64_t c_gs,
                               int groups, int M, int N, int K, int act, void* stream) {
    constexpr bool f32 = sizeof(WT) == 4;
    constexpr int WA = 16 / (int)sizeof(WT);
    QARIG_CHECK_ARG(X && W && C, "decode_linear: null operand");
    QARIG_CHECK_ARG(groups >= 1 && groups <= 65535, "decode_linear: bad group count %d", groups);
    QARIG_CHECK_ARG((gamma == nullptr) == (beta == nullptr), "decode_linear: gamma/beta pair");
    QARIG_CHECK_ARG((scale == nullptr) == (shift == nullptr), "decode_linear: scale/shift pair");
    QARIG_CHECK_ARG(!(gamma && scale), "decode_linear: affine and AdaLN forms are exclusive");
    const int ln = gamma ? 1 : (scale ? (ldmod == 0 ? 3 : 2) : 0);
    QARIG_CHECK_ARG(qarig_decode_linear_supported(M, N, K, ln),
                    "decode_linear: needs M <= 16 and K in {256, 512, 1024} (2048, 4096 without a "
                    "LayerNorm prologue) (M=%d N=%d K=%d)", M, N, K);
    QARIG_CHECK_DIMS("decode_linear", groups, N, K);
    QARIG_CHECK_ARG(act >= 0 && act <= 3, "decode_linear: bad activation id");
    QARIG_CHECK_ARG(!ln || eps > 0.0f, "decode_linear: eps must be positive");
    auto al16 = [](const void* q) { return ((uintptr_t)q & 15) == 0; };
    QARIG_CHECK_ARG(al16(X) && al16(W) && ldx % 4 == 0 && ldw % WA == 0 && x_gs % 4 == 0 && w_gs % WA == 0 &&
                        al16(gamma) && al16(beta) && al16(scale) && al16(shift) && ldmod % 4 == 0,
                    "decode_linear: operands must be 16-B aligned");
    QARIG_CHECK_ARG(ldx >= K && ldw >= K && ldc >= N && (!residual || ldr >= N) && (!mul || ldmul == 0 || ldmul >= N) &&
                        (!scale || ldmod == 0 || ldmod >= K),
                    "decode_linear: a row stride is shorter than its row");
    const DecLinHead<WT> h{X, W, ldx, ldw, M, N, K, act, x_gs, w_gs};
    const DecLin p{bias, bias_gs, C, ldc, c_gs, residual, ldr, mul, ldmul, gamma, beta, scale, shift, ldmod, eps};
    hipStream_t st = (hipStream_t)stream;
    if constexpr (f32) {
        bool done = false;
        if ((M > 4 && g_qarig_opt.decode_rows != 0) || g_qarig_opt.decode_rows == 2)
            done = launch_decode_linear_rows_ln<WT, 4>(ln, h, p, groups, st);
        if (done) {
        } else if (M <= 4) {
            launch_decode_linear_ln<WT, 4, 4>(ln, h, p, groups, st);
        } else {
            launch_decode_linear_ln<WT, 4, 16>(ln, h, p, groups, st);
        }
    } else {
        // the row-split kernel takes every K of a bf16 image (K = 4096 is 8 chunks of 512), so 5 ... 16 rows always
        // run on it: the all-rows kernel exists for <= 4 rows only (the decode_rows = 0 ablation is an fp32 one)
        const bool rows = M > 4 || g_qarig_opt.decode_rows == 2;
        bool done = true;
        if (K == 256) {
            if (rows) done = launch_decode_linear_rows_ln<WT, 4>(ln, h, p, groups, st);
            else launch_decode_linear_ln<WT, 4, 4>(ln, h, p, groups, st);
        } else {
            if (rows) done = launch_decode_linear_rows_ln<WT, 8>(ln, h, p, groups, st);
            else launch_decode_linear_ln<WT, 8, 4>(ln, h, p, groups, st);
        }
        QARIG_CHECK_ARG(done, "decode_linear: no bf16-weight kernel for M=%d K=%d ln=%d", M, K, ln);
    }
    QARIG_CHECK_LAUNCH("decode_linear");
    return QARIG_OK;
}

extern "C" int qarig_decode_linear_f32(const float* X, int64_t ldx, int64_t x_gs, float eps,
                                       const float* gamma, const float* beta, const float* scale,
                                       const float* shift, int64_t ldmod, const float* W, int64_t ldw,
                                       int64_t w_gs, const float* bias, int64_t bias_gs,
                                       const float* residual, int64_t ldr, const float* mul,
                                       int64_t ldmul, float* C, int64_t ldc, int64_t c_gs, int groups,
                                       int M, int N, int K, int act, void* stream) {
    return decode_linear_entry<float>(X, ldx, x_gs, eps, gamma, beta, scale, shift, ldmod, W, ldw, w_gs, bias, bias_gs,
                                      residual, ldr, mul, ldmul, C, ldc, c_gs, groups, M, N, K, act, stream);
}

extern "C" int qarig_decode_linear_bf16w(const float* X, int64_t ldx, int64_t x_gs, float eps,
                                         const float* gamma, const float* beta, const float* scale,
                                         const float* shift, int64_t ldmod, const void* W, int64_t ldw,
                                         int64_t w_gs, const float* bias, int64_t bias_gs,
                                         const float* residual, int64_t ldr, const float* mul,
                                         int64_t ldmul, float* C, int64_t ldc, int64_t c_gs, int groups,
                                         int M, int N, int K, int act, void* stream) {
    return decode_linear_entry<bf16w>(X, ldx, x_gs, eps, gamma, beta, scale, shift, ldmod, (const bf16w*)W, ldw, w_gs,
                                      bias, bias_gs, residual, ldr, mul, ldmul, C, ldc, c_gs, groups, M, N, K, act,
                                      stream);
}


extern "C" int qarig_decode_embed(const int64_t* ids, int B, int D, int V, const float* table,
                                  const float* pe, int* ctl, int len, int max_len,
                                  const float* proj_table, int64_t proj_row_floats, float* x,
                                  float* proj_row, int* bad_flag, void* stream) {
    QARIG_CHECK_ARG(ids && table && x && bad_flag, "decode_embed: null pointer");
    QARIG_CHECK_ARG(B > 0 && D > 0 && V > 0 && max_len > 0 && D % 4 == 0, "decode_embed: bad extents (D %% 4 == 0)");
    QARIG_CHECK_DIMS("decode_embed", B, D);
    QARIG_CHECK_DIMS("decode_embed", V, D);
    QARIG_CHECK_DIMS("decode_embed", max_len, D);
    QARIG_CHECK_ARG(ctl || (len >= 0 && len < max_len), "decode_embed: len out of range");
    QARIG_CHECK_ARG(proj_row_floats >= 0 && proj_row_floats % 4 == 0 && proj_row_floats <= (1LL << 30) &&
                        (proj_row_floats == 0 || (proj_table && proj_row)),
                    "decode_embed: projection row must be a multiple of 4 floats with both pointers given");
    QARIG_CHECK_ARG(proj_row_floats == 0 || qarig_dims_ok({max_len, proj_row_floats}), "decode_embed: table too large");
    auto al16 = [](const void* q) { return ((uintptr_t)q & 15) == 0; };
    QARIG_CHECK_ARG(al16(table) && al16(pe) && al16(x) && al16(proj_table) && al16(proj_row),
                    "decode_embed: operands must be 16-B aligned");
    const int64_t items = (int64_t)B * D / 4 + proj_row_floats / 4;
    const int blocks = (int)((items + 255) / 256 < 1024 ? (items + 255) / 256 : 1024);
    hipLaunchKernelGGL(decode_embed_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, ids, B, D, V, table, pe,
                       ctl, len, max_len, proj_table, proj_row_floats, x, proj_row, bad_flag);
    QARIG_CHECK_LAUNCH("decode_embed");
    return QARIG_OK;
}

static bool decode_head_dim_instantiated(int d) { return d == 4 || d == 8 || d == 16 || d == 32 || d == 64; }

// Keys a wave covers per pass of its loop at head dim d (0: unsupported): 64 lanes x decode_attention_kernel's U
// for the instantiated dims, the grouped kernel's own constant for every other multiple of 4 up to 128.
extern "C" int qarig_decode_attention_keys_per_pass(int d) {
    if (d < 4 || d > 128 || d % 4) return 0;
    if (decode_head_dim_instantiated(d)) return d <= 16 ? 256 : (d <= 32 ? 128 : 64);
    return grouped_keys_per_pass(d);
}

extern "C" int qarig_decode_attention(const float* q, const float* k_new, const float* v_new, float* kcache,
                                      float* vcache, int B, int H, int d, int len, const int* len_dev,
                                      int max_len, int64_t batch_stride, int64_t head_stride, int64_t row_stride,
                                      float sqrt_d, const float* o_mul, int64_t ldmul, float* o, void* stream) {
    QARIG_CHECK_ARG(q && kcache && vcache && o, "decode_attention: null pointer");
    QARIG_CHECK_ARG((k_new == nullptr) == (v_new == nullptr), "decode_attention: k_new and v_new go together");
    QARIG_CHECK_ARG(B > 0 && H > 0 && d > 0 && max_len > 0 && sqrt_d > 0.0f, "decode_attention: bad extents");
    QARIG_CHECK_DIMS("decode_attention", B, H, max_len);
    QARIG_CHECK_ARG(qarig_decode_attention_keys_per_pass(d) > 0,
                    "decode_attention: head dim %d unsupported (multiples of 4 from 4 to 128)", d);
    QARIG_CHECK_ARG((long long)B * H < (1LL << 31), "decode_attention: bad extents");
    const bool row_major = head_stride == d && row_stride == (int64_t)H * d && batch_stride >= (int64_t)max_len * H * d;
    const bool head_major = row_stride == d && head_stride >= (int64_t)max_len * d && head_stride <= (1LL << 40) &&
                            batch_stride >= (int64_t)H * head_stride;
    QARIG_CHECK_ARG((row_major || head_major) && batch_stride % 4 == 0 && head_stride % 4 == 0,
                    "decode_attention: cache strides are neither row-major (rows of H * d) nor head-major "
                    "(a head's max_len rows of d), or shorter than max_len rows");
    QARIG_CHECK_ARG(!o_mul || ldmul == 0 || ldmul >= (int64_t)H * d, "decode_attention: ldmul shorter than a row");
    auto al16 = [](const void* p) { return ((uintptr_t)p & 15) == 0; };
    QARIG_CHECK_ARG(al16(q) && al16(k_new) && al16(v_new) && al16(kcache) && al16(vcache),
                    "decode_attention: operands must be 16-B aligned");
    if (!len_dev) {
        QARIG_CHECK_ARG(len >= 0 && (k_new ? len < max_len : (len > 0 && len <= max_len)),
                        "decode_attention: len out of range for the cache");
    }
    const float c2 = 1.4426950408889634f / sqrt_d;
    const dim3 grid(B * ((H + 3) / 4)), block(256);
    hipStream_t st = (hipStream_t)stream;
#define QARIG_DA(HD)                                                                                          \
    hipLaunchKernelGGL((decode_attention_kernel<HD>), grid, block, 0, st, q, k_new, v_new, kcache, vcache,    \
                       batch_stride, head_stride, row_stride, H, len, len_dev, max_len, c2, o_mul, ldmul, o)
#define QARIG_DAG(G, C4)                                                                                      \
    static_assert(GroupedAttn<G, C4>::KEYS == grouped_keys_per_pass(4 * G * C4 - 4), "");                     \
    hipLaunchKernelGGL((decode_attention_grouped_kernel<G, C4>), grid, block, 0, st, q, k_new, v_new, kcache, \
                       vcache, batch_stride, head_stride, row_stride, H, d, len, len_dev, max_len, c2, o_mul, \
                       ldmul, o)
    if (!decode_head_dim_instantiated(d)) {     // every other multiple of 4 up to 128: the bucket that holds it
        if (d < 16) {
            QARIG_DAG(2, 2);
        } else if (d < 32) {
            QARIG_DAG(2, 4);
        } else if (d < 64) {
            QARIG_DAG(4, 4);
        } else {
            QARIG_DAG(4, 8);
        }
    } else
    switch (d) {
        case 4: QARIG_DA(4); break;
        case 8: QARIG_DA(8); break;
        case 16: QARIG_DA(16); break;
        case 32: QARIG_DA(32); break;
        default: QARIG_DA(64); break;
    }
#undef QARIG_DAG
#undef QARIG_DA
    QARIG_CHECK_LAUNCH("decode_attention");
    return QARIG_OK;
}

extern "C" int qarig_decode_sample(const float* logits, int64_t ldl, int B, int V, float temperature,
                                   int end_token, int generate_mode, int64_t shift, const float* uniforms,
                                   const int64_t* forced, int* ctl, int slot, int beam_width, int max_draws,
                                   int inc_len, int beams, int64_t* ids, int64_t* chunk, float* comb,
                                   float* probs_log, void* stream) {
    QARIG_CHECK_ARG(logits && uniforms && ctl && ids && chunk && comb, "decode_sample: null pointer");
    QARIG_CHECK_ARG(B > 0 && V > 0 && beam_width > 0 && max_draws > 0 && slot >= -1 && slot < beam_width,
                    "decode_sample: bad extents");
    QARIG_CHECK_DIMS("decode_sample", B, V);
    QARIG_CHECK_DIMS("decode_sample", max_draws, B);
    QARIG_CHECK_DIMS("decode_sample", B, beam_width);
    QARIG_CHECK_ARG(ldl >= V && temperature > 0.0f, "decode_sample: ldl < V or temperature <= 0");
    QARIG_CHECK_ARG(beams >= 0 && (beams == 0 || B % beams == 0), "decode_sample: beams must divide the rows");
    QARIG_CHECK_ARG(!probs_log || qarig_dims_ok({max_draws, B, V}), "decode_sample: probability log too large");
    hipLaunchKernelGGL(decode_sample_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, logits, ldl, B, V,
                       temperature, end_token, generate_mode, shift, uniforms, forced, ctl, slot, beam_width,
                       max_draws, inc_len, beams, ids, chunk, comb, probs_log);
    QARIG_CHECK_LAUNCH("decode_sample");
    return QARIG_OK;
}

extern "C" int qarig_decode_sample_filtered(const float* logits, int64_t ldl, int B, int V, float temperature,
                                            int end_token, int generate_mode, int64_t shift, const float* uniforms,
                                            const int64_t* forced, int* ctl, int slot, int beam_width, int max_draws,
                                            int inc_len, int beams, int64_t* ids, int64_t* chunk, float* comb,
                                            float* probs_log, int top_k, float top_p, void* stream) {
    QARIG_CHECK_ARG(logits && uniforms && ctl && ids && chunk && comb, "decode_sample_filtered: null pointer");
    QARIG_CHECK_ARG(B > 0 && V > 0 && beam_width > 0 && max_draws > 0 && slot >= -1 && slot < beam_width,
                    "decode_sample_filtered: bad extents");
    QARIG_CHECK_DIMS("decode_sample_filtered", B, V);
    QARIG_CHECK_DIMS("decode_sample_filtered", max_draws, B);
    QARIG_CHECK_DIMS("decode_sample_filtered", B, beam_width);
    QARIG_CHECK_ARG(ldl >= V && temperature > 0.0f, "decode_sample_filtered: ldl < V or temperature <= 0");
    QARIG_CHECK_ARG(beams >= 0 && (beams == 0 || B % beams == 0), "decode_sample_filtered: beams must divide the rows");
    QARIG_CHECK_ARG(!probs_log || qarig_dims_ok({max_draws, B, V}), "decode_sample_filtered: probability log too large");
    QARIG_CHECK_ARG(top_k >= 0, "decode_sample_filtered: top_k must be >= 0 (0: off), got %d", top_k);
    QARIG_CHECK_ARG(top_p > 0.0f && top_p <= 1.0f, "decode_sample_filtered: top_p must be in (0, 1] (1: off), got %g",
                    (double)top_p);
    QARIG_CHECK_ARG(V <= SF_MAX_V, "decode_sample_filtered: the row is staged in LDS, V = %d exceeds %d", V, SF_MAX_V);
    const size_t lds = (size_t)V * sizeof(float);
    static bool allowed = false;
    if (!allowed && lds > 48 * 1024) {          // beyond the default dynamic allowance: V up to 16,385 needs 64 KB + 4 B
        (void)hipFuncSetAttribute((const void*)decode_sample_filtered_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  SF_MAX_V * (int)sizeof(float));
        allowed = true;
    }
    hipLaunchKernelGGL(decode_sample_filtered_kernel, dim3(B), dim3(SF_THREADS), lds, (hipStream_t)stream, logits, ldl,
                       B, V, temperature, end_token, generate_mode, shift, uniforms, forced, ctl, slot, beam_width,
                       max_draws, inc_len, beams, ids, chunk, comb, probs_log, top_k, top_p);
    QARIG_CHECK_LAUNCH("decode_sample_filtered");
    return QARIG_OK;
}

extern "C" int qarig_decode_decide(int* ctl, int N, int NB, int beam_width, int draws, float* comb,
                                   const int64_t* chunk, float* best_p, int64_t* best_chunk, int* take, void* stream) {
    QARIG_CHECK_ARG(ctl && comb && chunk && best_p && best_chunk && take, "decode_decide: null pointer");
    QARIG_CHECK_ARG(N > 0 && NB > 0 && beam_width > 0 && draws >= 0 && draws <= (1 << 24), "decode_decide: bad extents");
    QARIG_CHECK_DIMS("decode_decide", N, NB, beam_width);
    hipLaunchKernelGGL(decode_decide_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, ctl, N, NB, beam_width, draws,
                       comb, chunk, best_p, best_chunk, take);
    QARIG_CHECK_LAUNCH("decode_decide");
    return QARIG_OK;
}

extern "C" int qarig_decode_rows(const int* ctl, float* kv, float* staged, const int* take, int layers2, int N,
                                 int NB, int H, int R, int d, int max_len, int restore, void* stream) {
    QARIG_CHECK_ARG(ctl && kv && staged && (restore || take), "decode_rows: null pointer");
    QARIG_CHECK_ARG(layers2 > 0 && N > 0 && NB > 0 && H > 0 && R > 0 && d > 0 && d % 4 == 0 && max_len > 0,
                    "decode_rows: bad extents (d %% 4 == 0)");
    QARIG_CHECK_DIMS("decode_rows", layers2, N, NB, max_len);
    QARIG_CHECK_DIMS("decode_rows", layers2, N, NB, R);
    QARIG_CHECK_DIMS("decode_rows", max_len, H, d);
    QARIG_CHECK_DIMS("decode_rows", R, H, d);
    QARIG_CHECK_ARG(qarig_dims_ok({layers2, (long long)N * NB, (long long)max_len * H * d}, 1LL << 40, 1LL << 44),
                    "decode_rows: cache too large");
    QARIG_CHECK_ARG((((uintptr_t)kv | (uintptr_t)staged) & 15) == 0, "decode_rows: operands must be 16-B aligned");
    const int64_t total = (int64_t)layers2 * N * (restore ? NB : 1) * H * R * (d / 4);
    const int blocks = (int)((total + 255) / 256 < 2048 ? (total + 255) / 256 : 2048);
    hipLaunchKernelGGL(decode_rows_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, ctl, kv, staged, take,
                       layers2, N, NB, H, R, d, max_len, restore);
    QARIG_CHECK_LAUNCH("decode_rows");
    return QARIG_OK;
}

extern "C" int qarig_decode_cache_fill(const float* k, const float* v, int64_t ld, int64_t batch_stride, float* kv,
                                       int images, int beams, int H, int d, int P1, int max_len, void* stream) {
    QARIG_CHECK_ARG(k && v && kv, "decode_cache_fill: null pointer");
    QARIG_CHECK_ARG(images > 0 && beams > 0 && H > 0 && d > 0 && d % 4 == 0 && P1 > 0 && max_len > 0,
                    "decode_cache_fill: bad extents (d %% 4 == 0)");
    QARIG_CHECK_ARG(P1 <= max_len, "decode_cache_fill: %d prefix rows for a cache of %d", P1, max_len);
    QARIG_CHECK_DIMS("decode_cache_fill", images, beams, H, max_len);
    QARIG_CHECK_DIMS("decode_cache_fill", max_len, H, d);
    QARIG_CHECK_ARG(qarig_dims_ok({2, (long long)images * beams, (long long)max_len * H * d}, 1LL << 40, 1LL << 44),
                    "decode_cache_fill: cache too large");
    QARIG_CHECK_ARG(ld >= (int64_t)H * d && ld % 4 == 0 && ld <= (1LL << 32),
                    "decode_cache_fill: row stride shorter than H * d, or no multiple of 4");
    QARIG_CHECK_ARG(batch_stride >= 0 && batch_stride % 4 == 0 && batch_stride <= (1LL << 40) &&
                    (images == 1 || batch_stride >= (int64_t)(P1 - 1) * ld + (int64_t)H * d),
                    "decode_cache_fill: image stride shorter than the rows of an image, or no multiple of 4");
    QARIG_CHECK_ARG((((uintptr_t)k | (uintptr_t)v | (uintptr_t)kv) & 15) == 0,
                    "decode_cache_fill: operands must be 16-B aligned");
    const int64_t total = 2 * (int64_t)images * H * P1 * (d / 4);
    const int blocks = (int)((total + 255) / 256 < 2048 ? (total + 255) / 256 : 2048);
    hipLaunchKernelGGL(decode_cache_fill_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, k, v, ld,
                       batch_stride, kv, images, beams, H, d, P1, max_len);
    QARIG_CHECK_LAUNCH("decode_cache_fill");
    return QARIG_OK;
}

extern "C" int qarig_decode_commit(int* ctl, int N, int NB, int beam_width, const int64_t* best_chunk,
                                   int64_t* tokens, int64_t ldt, int64_t* ids, void* stream) {
    QARIG_CHECK_ARG(ctl && best_chunk && tokens && ids, "decode_commit: null pointer");
    QARIG_CHECK_ARG(N > 0 && NB > 0 && beam_width > 0 && ldt > 0, "decode_commit: bad extents");
    QARIG_CHECK_DIMS("decode_commit", N, NB, beam_width);
    QARIG_CHECK_ARG(qarig_dims_ok({N, ldt}, 1LL << 40), "decode_commit: token buffer too large");
    hipLaunchKernelGGL(decode_commit_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, ctl, N, NB, beam_width,
                       best_chunk, tokens, ldt, ids);
    QARIG_CHECK_LAUNCH("decode_commit");
    return QARIG_OK;
}

extern "C" int qarig_decode_advance(int* ctl, int beam_width, void* stream) {
    QARIG_CHECK_ARG(ctl && beam_width > 0, "decode_advance: bad arguments");
    hipLaunchKernelGGL(decode_advance_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, ctl, beam_width);
    QARIG_CHECK_LAUNCH("decode_advance");
    return QARIG_OK;
}

extern "C" int qarig_window_step_supported(int R, int window, int D, int H) {
    if (R < 1 || R > 16 || window < 2 || window > 65536 || D < 4 || D % 4 || H < 1 || D % H) return 0;
    return qarig_decode_attention_keys_per_pass(D / H) > 0;
}

extern "C" int qarig_window_assemble(const int64_t* ring, int64_t ldr, const int* ctl, int R, int W1, int Wp, int D,
                                     int V, const float* table, const float* pe, int P, int pos_off, float* x,
                                     int* rowmap, int* last_map, int* bad_flag, void* stream) {
    QARIG_CHECK_ARG(ring && ctl && table && pe && x && bad_flag, "window_assemble: null pointer");
    QARIG_CHECK_ARG(R > 0 && W1 > 0 && (Wp == W1 || (int64_t)Wp == (int64_t)W1 + 1) && D > 0 && D % 4 == 0 && V > 0 && ldr >= W1,
                    "window_assemble: bad extents (Wp = W1 or W1 + 1, D %% 4 == 0, ldr >= W1)");
    QARIG_CHECK_ARG(!rowmap || (P > 0 && pos_off >= 0 && pos_off <= 1), "window_assemble: rowmap needs P > 0, pos_off 0 or 1");
    QARIG_CHECK_ARG(!last_map || rowmap, "window_assemble: last_map needs rowmap");
    QARIG_CHECK_DIMS("window_assemble", R, Wp, D);
    QARIG_CHECK_DIMS("window_assemble", V, D);
    QARIG_CHECK_ARG(qarig_dims_ok({R, ldr}, 1LL << 24, 1LL << 40), "window_assemble: ring too large");
    auto al16 = [](const void* q) { return ((uintptr_t)q & 15) == 0; };
    QARIG_CHECK_ARG(al16(table) && al16(pe) && al16(x), "window_assemble: operands must be 16-B aligned");
    const int64_t items = (int64_t)R * Wp * (D / 4);
    const int blocks = (int)((items + 255) / 256 < 2048 ? (items + 255) / 256 : 2048);
    hipLaunchKernelGGL(window_assemble_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, ring, ldr, ctl, R, W1,
                       Wp, D, V, table, pe, P, pos_off, x, rowmap, last_map, bad_flag);
    QARIG_CHECK_LAUNCH("window_assemble");
    return QARIG_OK;
}

// The last real query of every window against its keys: decode_attention_kernel in its row-major
// (token-major) addressing, no appended row, n_keys keys of the `rows` the projections wrote.
extern "C" int qarig_window_attention(const float* q, const float* k, const float* v, int R, int H, int d,
                                      int n_keys, int rows, int64_t batch_stride, const float* o_mul, int64_t ldmul,
                                      float* o, void* stream) {
    QARIG_CHECK_ARG(q && k && v && o, "window_attention: null pointer");
    QARIG_CHECK_ARG(qarig_decode_attention_keys_per_pass(d) > 0,
                    "window_attention: head dim %d unsupported (multiples of 4 from 4 to 128)", d);
    QARIG_CHECK_ARG(R > 0 && H > 0 && n_keys > 0 && rows >= n_keys, "window_attention: bad extents (0 < n_keys <= rows)");
    QARIG_CHECK_DIMS("window_attention", R, H, rows);
    QARIG_CHECK_ARG(batch_stride >= (int64_t)rows * H * d && batch_stride % 4 == 0 && batch_stride <= (1LL << 40),
                    "window_attention: batch stride shorter than rows * H * d");
    return qarig_decode_attention(q, nullptr, nullptr, const_cast<float*>(k), const_cast<float*>(v), R, H, d, n_keys,
                                  nullptr, rows, batch_stride, d, (int64_t)H * d, sqrtf((float)d), o_mul, ldmul, o,
                                  stream);
}

extern "C" int qarig_window_append(int* ctl, const int64_t* ids, int64_t* ring, int B, int64_t ldr, int* bad_flag,
                                   void* stream) {
    QARIG_CHECK_ARG(ctl && ids && ring && bad_flag, "window_append: null pointer");
    QARIG_CHECK_ARG(B > 0 && ldr > 0 && qarig_dims_ok({B, ldr}, 1LL << 24, 1LL << 40), "window_append: bad extents");
    hipLaunchKernelGGL(window_append_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, ctl, ids, ring, B, ldr,
                       bad_flag);
    QARIG_CHECK_LAUNCH("window_append");
    return QARIG_OK;
}
