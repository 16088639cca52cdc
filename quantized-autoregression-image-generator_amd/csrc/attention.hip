// Fused multi-head attention, forward and backward, for the reference's
// AttentionLayer core (models/layers.py:433-474): split heads, QK^T / sqrt(d),
// causal mask (additive 2e9 then -inf == plain causal for finite logits), softmax,
// PV, merge heads.  q/k/v/o stay in the (N, S, H*d) layout the surrounding Linear
// layers produce -- no head permute, no (N,H,Sq,Sk) score tensor in HBM.
//
// The reference runs 64 heads on a 512-wide model: head dim 8.  A 32x32 or 16x16 MFMA tile
// wastes 2-4x of its lanes on a K = 8 / N = 8 contraction, so both contractions run on the
// 16-block form v_mfma_f32_4x4x1_16B_f32: sixteen independent 4x4 outer products per
// instruction, no padding at any head dim that is a multiple of 4, at the full fp32 matrix
// rate.  The mapping keeps ONE QUERY PER LANE (block b = lane/4, column j = lane%4):
//   S^T  : D[i][j] += A[i] * B[j],  A = K[key k0+i][c]  (4 key rows, from LDS),
//                                   B = Q[query of the lane][c]  (the lane's own register)
//          -> after c = 0..d-1 each lane holds the scores of ITS query against 4 keys;
//   PV   : D[i][j] += A[i] * B[j],  A = V[key][c = 4g+i] (from a transposed LDS image),
//                                   B = p(query of the lane, key)  (own register)
//          -> each lane accumulates O[its query][4g..4g+3] in the 4 result registers.
// So the online softmax (max, exp2, sum, rescale) needs no cross-lane traffic at all, the
// matrix pipe does the 4*d FMAs per (query, key) pair and the VALU only the ~10 softmax
// operations.  An MFMA is a k-ordered fma chain, so the numbers are those of the scalar loops
// `dot = fma(q_c, k_c, dot)` (c ascending) and `o_c = fma(p, v_c, o_c)` (keys ascending).
//
// Work split: a workgroup = 4 ADJACENT HEADS x (QW x 64) queries, one wave per (head, 64-query
// slice).  Four heads of head dim 8 are one 128-B line of every (N,S,512) row, so the K/V chunk
// a workgroup stages (coalesced 128-B row segments -> LDS, once) serves all its waves and
// every fetched line is used whole; with QW = 4 a 256-token sequence's K/V are read exactly once.
// Chunks are double-buffered: the global loads of chunk t+1 are issued before the
// MFMAs of chunk t and written to the other LDS buffer after them; one barrier per chunk.
// Backward = two such passes (lane per query for dQ, lane per key for dK/dV), probabilities
// recomputed from the saved log-sum-exp: deterministic, no atomics.
//
// Softmax runs in base 2: scores are scaled by c = log2(e)/sqrt(d) in one multiply and
// exponentiated with v_exp_f32 (2^x).  Against exp((q.k)/sqrt(d) - m) this perturbs each
// probability by <= ~1e-7 absolute (the product rounding is |x| * 2^-24 in the exponent
// and terms with large |x| are themselves tiny), two orders inside the 1e-5 tolerance
// stated for attention tensors; the saved LSE is kept in base-2 units (internal).  The backward
// passes recompute p = exp2(s * c - L) from that fp32 L, whose rounding (|L| * 2^-24) sits in the
// exponent: their probabilities carry a relative error proportional to |lse| * 2^-24, about
// 0.5 |L| 2^-24 ln 2, which only scores far from zero (|L| in the hundreds) make visible.
#include <stdlib.h>

#include "dropout_philox.h"
#include "qarig_common.h"

namespace qarig {

struct AttnDims {
    int N, Sq, Sk, H, causal;
    float c2;   // log2(e) / sqrt(d)
    float rsd;  // 1 / sqrt(d)
};
// Attention-probability dropout (DROP = true instantiations): the mask of csrc/dropout_philox.h is
// regenerated in registers by all three passes; `key` is the device key {seed_lo, seed_hi, step, rank}.  The plain
// kernels keep AttnDims as their argument, so their argument segment and code are what they were.
struct AttnDropDims : AttnDims {
    uint32_t threshold;
    float scale;
    uint32_t c1;            // 2^31 | site << 23
    const uint32_t* key;
};
template <bool DROP> struct DimsOf { typedef AttnDims T; };
template <> struct DimsOf<true> { typedef AttnDropDims T; };

// y[g'] bit r = x[r] bit g' within every aligned group of eight lanes (g = lane & 7): an 8 x 8 bit transpose in
// three butterfly exchanges (lane ^ 4, ^ 2, ^ 1), each one swizzle and a select.
template <int S, uint32_t LO>
__device__ __forceinline__ uint32_t transpose8_stage(uint32_t x, int lane) {
    const uint32_t y = (uint32_t)__builtin_amdgcn_ds_swizzle((int)x, 0x1f | (S << 10));   // lane ^ S, within 32
    return (lane & S) ? (((y >> S) & LO) | (x & ~LO)) : ((x & LO) | ((y & LO) << S));
}
__device__ __forceinline__ uint32_t transpose8(uint32_t x, int lane) {
    x = transpose8_stage<4, 0x0fu>(x, lane);
    x = transpose8_stage<2, 0x33u>(x, lane);
    return transpose8_stage<1, 0x55u>(x, lane);
}

__device__ __forceinline__ float exp2_fast(float x) { return __builtin_amdgcn_exp2f(x); }

constexpr int HPB = 4;   // heads per workgroup (adjacent: one 128-B line at head dim 8)

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_4x4x1f32(a, b, c, 0, 0, 0);
}

// Precision of the two contractions.  LP = false: fp32 operands, v_mfma_f32_4x4x1_16B_f32 (the
// parity mode: an exact fp32 fma chain).  LP = true (BASELINE config 5, opt-in): operands rounded
// to bf16 on their way into LDS / registers, v_mfma_f32_4x4x4_16B_bf16 contracts four c's (S, dP)
// or four keys / queries (PV, dQ, dK, dV) per instruction; accumulators, softmax, LSE and all
// tensors in HBM stay fp32.
typedef short s16x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint32_t pack2_bf16(float a, float b) {
    typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
    typedef float f32x2_t __attribute__((ext_vector_type(2)));
    const f32x2_t f = {a, b};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(f, bf16x2_t));
}
__device__ __forceinline__ s16x4 pack4_bf16(float a, float b, float c, float d) {
    const uint2 u = make_uint2(pack2_bf16(a, b), pack2_bf16(c, d));
    return __builtin_bit_cast(s16x4, u);
}
template <bool LP> struct Elem { typedef float T; };
template <> struct Elem<true> { typedef unsigned short T; };

// Geometry shared by the three kernels.  A chunk holds CH rows (keys, or queries in the dK/dV
// pass) of the workgroup's 4 heads; every thread moves exactly one float4 per tensor per chunk.
//   row image  R[row][4*HD + 4]   : fragment = reads of row (r0 + lane%4): conflict-free
//   transposed T[4*HD][CH + 4]    : fragment = reads of column group (4g + lane%4)
// (elements are fp32, or bf16 in the reduced-precision mode; strides in elements)
template <int HD>
struct Geo {
    static constexpr int W = HPB * HD;       // elements per staged row
    static constexpr int V4 = W / 4;         // float4 per staged row
    static constexpr int RS = W + 4;         // row-image stride
    __device__ static int chunk_rows() { return blockDim.x / V4; }
};

// One thread's float4 of a chunk: row = f / V4 of [row0, row0 + CH), columns 4*(f % V4) of the
// workgroup's head group; zero outside the tensor or beyond the last head.
template <int HD>
__device__ __forceinline__ float4 chunk_load(const float* __restrict__ base, int D, int row0,
                                             int limit, int cols_valid) {
    const int f = threadIdx.x;
    const int r = f / Geo<HD>::V4, c4 = f - r * Geo<HD>::V4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row0 + r < limit && c4 * 4 < cols_valid)
        v = *reinterpret_cast<const float4*>(base + (int64_t)(row0 + r) * D + c4 * 4);
    return v;
}
template <int HD, typename T>
__device__ __forceinline__ void chunk_store_rows(T* R, float4 v) {
    const int f = threadIdx.x;
    const int r = f / Geo<HD>::V4, c4 = f - r * Geo<HD>::V4;
    if constexpr (sizeof(T) == 4)
        *reinterpret_cast<float4*>(R + r * Geo<HD>::RS + c4 * 4) = v;
    else
        *reinterpret_cast<uint2*>(R + r * Geo<HD>::RS + c4 * 4) =
            make_uint2(pack2_bf16(v.x, v.y), pack2_bf16(v.z, v.w));
}
template <int HD, typename T>
__device__ __forceinline__ void chunk_store_transposed(T* Tp, int ts, float4 v) {
    const int f = threadIdx.x;
    const int r = f / Geo<HD>::V4, c4 = f - r * Geo<HD>::V4;
    T* t = Tp + (c4 * 4) * ts + r;
    if constexpr (sizeof(T) == 4) {
        t[0] = v.x; t[ts] = v.y; t[2 * ts] = v.z; t[3 * ts] = v.w;
    } else {
        const uint32_t lo = pack2_bf16(v.x, v.y), hi = pack2_bf16(v.z, v.w);
        t[0] = (T)(lo & 0xffffu); t[ts] = (T)(lo >> 16);
        t[2 * ts] = (T)(hi & 0xffffu); t[3 * ts] = (T)(hi >> 16);
    }
}

// The lane's own row (query, or key in the dK/dV pass): the B operand of the c-contractions.
template <bool LP, int HD> struct Own { float f[HD]; };
template <int HD> struct Own<true, HD> { s16x4 b[HD / 4]; };
template <bool LP, int HD>
__device__ __forceinline__ void own_load(Own<LP, HD>& o, const float* p, bool active) {
#pragma unroll
    for (int c = 0; c < HD; c += 4) {
        float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
        if (active) t = *reinterpret_cast<const float4*>(p + c);
        if constexpr (LP) o.b[c / 4] = pack4_bf16(t.x, t.y, t.z, t.w);
        else { o.f[c] = t.x; o.f[c + 1] = t.y; o.f[c + 2] = t.z; o.f[c + 3] = t.w; }
    }
}
// s[i] += sum_c R[row i = lane%4 of the 4 staged rows][c] * own[c]   (c ascending)
template <bool LP, int HD, typename T>
__device__ __forceinline__ void dot_rows(f32x4& s, const T* rowp, const Own<LP, HD>& own) {
#pragma unroll
    for (int g = 0; g < HD / 4; ++g) {
        if constexpr (LP) {
            const s16x4 ka = *reinterpret_cast<const s16x4*>(rowp + 4 * g);
            s = __builtin_amdgcn_mfma_f32_4x4x4bf16_1k(ka, own.b[g], s, 0, 0, 0);
        } else {
            const f32x4 ka = *reinterpret_cast<const f32x4*>(rowp + 4 * g);
#pragma unroll
            for (int c = 0; c < 4; ++c) s = mfma4(ka[c], own.f[4 * g + c], s);
        }
    }
}
// Four per-lane values (probabilities / score gradients of 4 consecutive staged rows).
template <bool LP> struct Vals { float v[4]; };
template <> struct Vals<true> { s16x4 b; };
template <bool LP>
__device__ __forceinline__ Vals<LP> make_vals(float a, float b, float c, float d) {
    Vals<LP> r;
    if constexpr (LP) r.b = pack4_bf16(a, b, c, d);
    else { r.v[0] = a; r.v[1] = b; r.v[2] = c; r.v[3] = d; }
    return r;
}
// Sum of the lane's four bf16 values as the matrix pipe reads them: the PV product against a column of ones
// (every row of the 4x4 result holds it), off the vector ALU that bounds the forward pass.
__device__ __forceinline__ float sum4_bf16(s16x4 b) {
    const s16x4 ones = {0x3f80, 0x3f80, 0x3f80, 0x3f80};
    return __builtin_amdgcn_mfma_f32_4x4x4bf16_1k(ones, b, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0)[0];
}
// o[i] += sum over the 4 staged rows r of T[column 4g + i][r] * vals[r]   (r ascending)
template <bool LP, typename T>
__device__ __forceinline__ void acc_cols(f32x4& o, const T* trp, const Vals<LP>& x) {
    if constexpr (LP) {
        const s16x4 va = *reinterpret_cast<const s16x4*>(trp);
        o = __builtin_amdgcn_mfma_f32_4x4x4bf16_1k(va, x.b, o, 0, 0, 0);
    } else {
        const f32x4 va = *reinterpret_cast<const f32x4*>(trp);
#pragma unroll
        for (int r = 0; r < 4; ++r) o = mfma4(va[r], x.v[r], o);
    }
}

// Forward.  Lane = query; wave = (head hh = wave % 4, query slice qq = wave / 4).
template <int HD, int MAXT, bool LP, bool DROP>
__global__ __launch_bounds__(MAXT) void attn_fwd_kernel(const float* __restrict__ q,
                                                        const float* __restrict__ k,
                                                        const float* __restrict__ v,
                                                        typename DimsOf<DROP>::T a,
                                                        float* __restrict__ o,
                                                        float* __restrict__ lse) {
    typedef typename Elem<LP>::T T;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    T* smem = reinterpret_cast<T*>(smem_raw);
    constexpr int G = HD / 4;
    constexpr int KS = HD <= 8 ? 16 : 8;    // keys per online-softmax step
    constexpr int NQ = KS / 4;
    const int CH = Geo<HD>::chunk_rows();
    const int TS = CH + 4;
    const int QW = blockDim.x >> 8;                    // query slices (waves per head)
    const int QB = QW * 64;
    const int qblocks = (a.Sq + QB - 1) / QB;
    const int hgroups = (a.H + HPB - 1) / HPB;
    // heaviest (latest) query blocks first under the causal mask
    int bid = blockIdx.x;
    const int hg = bid % hgroups; bid /= hgroups;
    const int n = bid % a.N; bid /= a.N;
    const int qb = qblocks - 1 - bid;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // provably wave-uniform
    const int hh = wave & 3, qq = wave >> 2;
    const int h = hg * HPB + hh;
    const bool head_ok = h < a.H;
    const int D = a.H * HD;
    const int q0 = qb * QB + qq * 64;                  // first query of this wave
    const int i = q0 + lane;
    const bool active = head_ok && i < a.Sq;
    const int li = lane & 3;
    const int cols_valid = (a.H - hg * HPB) * HD;      // columns of the head group inside the tensor

    // buffer b: K rows at b * BUF, V transposed behind them (integer offsets into `smem`: the
    // accesses stay ds_* instructions)
    const int BUF = CH * Geo<HD>::RS + Geo<HD>::W * TS;
    const int VOFF = CH * Geo<HD>::RS;

    Own<LP, HD> qv;
    own_load<LP, HD>(qv, q + ((int64_t)n * a.Sq + (active ? i : 0)) * D + h * HD, active);
    f32x4 ov[G];
#pragma unroll
    for (int g = 0; g < G; ++g) ov[g] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m = -INFINITY, l = 0.0f;
    // LP: the output is normalised by the sum of the probabilities AS ROUNDED for the PV product, so it is a convex
    // combination of the V rows whatever the rounding took (and whatever residual the fma below leaves on the
    // largest score: exp2(fma(s, c2, -fl(s c2))) is 1 + O(|s c2| 2^-24), which the bf16 rounding turns into 1 in
    // the numerator only); the saved LSE keeps the unrounded sum
    float lr = 0.0f;

    const float* kb = k + (int64_t)n * a.Sk * D + hg * HPB * HD;
    const float* vb = v + (int64_t)n * a.Sk * D + hg * HPB * HD;
    const int jend_blk = a.causal ? min(a.Sk, qb * QB + QB) : a.Sk;   // keys the workgroup needs
    const int jend = a.causal ? min(a.Sk, q0 + 64) : a.Sk;            // keys this wave needs
    const int nchunks = (jend_blk + CH - 1) / CH;

    float4 rk = chunk_load<HD>(kb, D, 0, a.Sk, cols_valid);
    float4 rv = chunk_load<HD>(vb, D, 0, a.Sk, cols_valid);
    chunk_store_rows<HD>(smem, rk);
    chunk_store_transposed<HD>(smem + VOFF, TS, rv);
    __syncthreads();
    for (int t = 0; t < nchunks; ++t) {
        const int c0 = t * CH;
        if (t + 1 < nchunks) {                         // next chunk: loads in flight under the MFMAs
            rk = chunk_load<HD>(kb, D, c0 + CH, a.Sk, cols_valid);
            rv = chunk_load<HD>(vb, D, c0 + CH, a.Sk, cols_valid);
        }
        const T* Kc = smem + (t & 1) * BUF + hh * HD;
        const T* Vc = smem + (t & 1) * BUF + VOFF + (hh * HD) * TS;
        const int jw = min(c0 + CH, jend);
        for (int j0 = c0; j0 < jw; j0 += KS) {
            const int jj = j0 - c0;
            // S^T for KS keys: NQ accumulators of 4 keys each, c ascending
            f32x4 s[NQ];
            const T* kr = Kc + (jj + li) * Geo<HD>::RS;
#pragma unroll
            for (int u = 0; u < NQ; ++u) {
                s[u] = f32x4{0.f, 0.f, 0.f, 0.f};
                dot_rows<LP, HD>(s[u], kr + 4 * u * Geo<HD>::RS, qv);
            }
            // raw scores; the scale (c2 > 0) enters once on the maximum and inside the exponent's fma
            if (j0 + KS > jw || (a.causal && j0 + KS - 1 > q0)) {     // wave-uniform: edge steps only
#pragma unroll
                for (int r = 0; r < KS; ++r)
                    if (j0 + r >= jw || (a.causal && j0 + r > i)) s[r >> 2][r & 3] = -INFINITY;
            }
            float mc = s[0][0];
#pragma unroll
            for (int r = 1; r < KS; ++r) mc = fmaxf(mc, s[r >> 2][r & 3]);
            const float mn = fmaxf(m, mc * a.c2);
            const float msafe = mn == -INFINITY ? 0.0f : mn;     // fully masked so far: p = 0
            const float alpha = exp2_fast(m - msafe);
            l *= alpha;
            if constexpr (LP) lr *= alpha;
#pragma unroll
            for (int g = 0; g < G; ++g) ov[g] *= alpha;
            float p[KS];
            typedef float f32x2 __attribute__((ext_vector_type(2)));
            f32x2 lsum = {0.0f, 0.0f};
            const f32x2 c2v = {a.c2, a.c2}, nm = {-msafe, -msafe};
#pragma unroll
            for (int r = 0; r < KS; r += 2) {
                const f32x2 sv = {s[r >> 2][r & 3], s[(r + 1) >> 2][(r + 1) & 3]};
                const f32x2 d = __builtin_elementwise_fma(sv, c2v, nm);      // v_pk_fma_f32
                const f32x2 pv2 = {exp2_fast(d[0]), exp2_fast(d[1])};
                p[r] = pv2[0]; p[r + 1] = pv2[1];
                lsum += pv2;                                                  // v_pk_add_f32
            }
            l += lsum[0] + lsum[1];
            m = mn;
            if constexpr (DROP) {
                // l, m and lr are those of the undropped softmax; the PV product takes +0 where dropped.  One call
                // per eight keys, made by every lane (the key words and c0 are loop invariants); masked keys have
                // p = 0 already.
                const uint32_t dc0 = attn_dropout_c0((uint32_t)n, (uint32_t)a.H, (uint32_t)h, (uint32_t)a.Sq, (uint32_t)i);
                bool keep[KS];
#pragma unroll
                for (int e = 0; e < KS / 8; ++e) {
                    uint32_t w[4];
                    philox4x32_10(dc0, a.c1 | (uint32_t)((j0 >> 3) + e), a.key[2], a.key[3], a.key[0], a.key[1], w);
#pragma unroll
                    for (int r = 0; r < 8; ++r) keep[8 * e + r] = dropout_value(w[r >> 1], r, a.threshold);
                }
#pragma unroll
                for (int u = 0; u < NQ; ++u) {
                    if constexpr (LP) lr += sum4_bf16(pack4_bf16(p[4 * u], p[4 * u + 1], p[4 * u + 2], p[4 * u + 3]));
                    const Vals<LP> pv = make_vals<LP>(keep[4 * u] ? p[4 * u] : 0.0f, keep[4 * u + 1] ? p[4 * u + 1] : 0.0f,
                                                      keep[4 * u + 2] ? p[4 * u + 2] : 0.0f,
                                                      keep[4 * u + 3] ? p[4 * u + 3] : 0.0f);
#pragma unroll
                    for (int g = 0; g < G; ++g) acc_cols<LP>(ov[g], Vc + (4 * g + li) * TS + jj + 4 * u, pv);
                }
            } else {
            // PV: keys ascending per output column group
#pragma unroll
            for (int u = 0; u < NQ; ++u) {
                const Vals<LP> pv = make_vals<LP>(p[4 * u], p[4 * u + 1], p[4 * u + 2], p[4 * u + 3]);
                if constexpr (LP) lr += sum4_bf16(pv.b);
#pragma unroll
                for (int g = 0; g < G; ++g) acc_cols<LP>(ov[g], Vc + (4 * g + li) * TS + jj + 4 * u, pv);
            }
            }
        }
        if (t + 1 < nchunks) {
            chunk_store_rows<HD>(smem + ((t + 1) & 1) * BUF, rk);
            chunk_store_transposed<HD>(smem + ((t + 1) & 1) * BUF + VOFF, TS, rv);
        }
        __syncthreads();
    }
    if (active) {
        float* op = o + ((int64_t)n * a.Sq + i) * D + h * HD;
        if constexpr (DROP) {
            const float inv = a.scale / (LP ? lr : l);
#pragma unroll
            for (int g = 0; g < G; ++g)
                *reinterpret_cast<float4*>(op + 4 * g) =
                    make_float4(ov[g][0] * inv, ov[g][1] * inv, ov[g][2] * inv, ov[g][3] * inv);
        } else {
        const float inv = 1.0f / (LP ? lr : l);
#pragma unroll
        for (int g = 0; g < G; ++g)
            *reinterpret_cast<float4*>(op + 4 * g) =
                make_float4(ov[g][0] * inv, ov[g][1] * inv, ov[g][2] * inv, ov[g][3] * inv);
        }
        lse[((int64_t)n * a.H + h) * a.Sq + i] = m + log2f(l);   // base-2 units
    }
}

// dQ pass: lane = query; per chunk the K rows, V rows and K transposed.  Also emits
// delta[i] = sum_c dO[i][c] * O[i][c].
template <int HD, int MAXT, bool LP, bool DROP>
__global__ __launch_bounds__(MAXT) void attn_bwd_dq_kernel(
    const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
    const float* __restrict__ o, const float* __restrict__ dO, const float* __restrict__ lse,
    typename DimsOf<DROP>::T a, float* __restrict__ dq, float* __restrict__ delta) {
    typedef typename Elem<LP>::T T;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    T* smem = reinterpret_cast<T*>(smem_raw);
    constexpr int G = HD / 4;
    constexpr int KS = HD <= 8 ? 16 : 8;    // keys per step
    constexpr int NQ = KS / 4;
    const int CH = Geo<HD>::chunk_rows();
    const int TS = CH + 4;
    const int QW = blockDim.x >> 8;
    const int QB = QW * 64;
    const int qblocks = (a.Sq + QB - 1) / QB;
    const int hgroups = (a.H + HPB - 1) / HPB;
    int bid = blockIdx.x;
    const int hg = bid % hgroups; bid /= hgroups;
    const int n = bid % a.N; bid /= a.N;
    const int qb = qblocks - 1 - bid;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // provably wave-uniform
    const int hh = wave & 3, qq = wave >> 2;
    const int h = hg * HPB + hh;
    const bool head_ok = h < a.H;
    const int D = a.H * HD;
    const int q0 = qb * QB + qq * 64;
    const int i = q0 + lane;
    const bool active = head_ok && i < a.Sq;
    const int li = lane & 3;
    const int cols_valid = (a.H - hg * HPB) * HD;
    // buffer b at b * BUF: K rows | V rows | K transposed
    const int BUF = 2 * CH * Geo<HD>::RS + Geo<HD>::W * TS;
    const int VOFF = CH * Geo<HD>::RS, TOFF = 2 * CH * Geo<HD>::RS;

    const int64_t roff = ((int64_t)n * a.Sq + (active ? i : 0)) * D + h * HD;
    Own<LP, HD> qv, dov;
    own_load<LP, HD>(qv, q + roff, active);
    own_load<LP, HD>(dov, dO + roff, active);
    float dl = 0.0f;                     // delta from the fp32 tensors in both modes
#pragma unroll
    for (int c = 0; c < HD; c += 4) {
        float4 tg = make_float4(0.f, 0.f, 0.f, 0.f), to = tg;
        if (active) {
            tg = *reinterpret_cast<const float4*>(dO + roff + c);
            to = *reinterpret_cast<const float4*>(o + roff + c);
        }
        dl = fmaf(tg.x, to.x, dl); dl = fmaf(tg.y, to.y, dl);
        dl = fmaf(tg.z, to.z, dl); dl = fmaf(tg.w, to.w, dl);
    }
    const float L = active ? lse[((int64_t)n * a.H + h) * a.Sq + i] : 0.0f;
    f32x4 acc[G];
#pragma unroll
    for (int g = 0; g < G; ++g) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};

    const float* kb = k + (int64_t)n * a.Sk * D + hg * HPB * HD;
    const float* vb = v + (int64_t)n * a.Sk * D + hg * HPB * HD;
    const int jend_blk = a.causal ? min(a.Sk, qb * QB + QB) : a.Sk;
    const int jend = a.causal ? min(a.Sk, q0 + 64) : a.Sk;
    const int nchunks = (jend_blk + CH - 1) / CH;

    float4 rk = chunk_load<HD>(kb, D, 0, a.Sk, cols_valid);
    float4 rv = chunk_load<HD>(vb, D, 0, a.Sk, cols_valid);
    chunk_store_rows<HD>(smem, rk);
    chunk_store_rows<HD>(smem + VOFF, rv);
    chunk_store_transposed<HD>(smem + TOFF, TS, rk);
    __syncthreads();
    for (int t = 0; t < nchunks; ++t) {
        const int c0 = t * CH;
        if (t + 1 < nchunks) {
            rk = chunk_load<HD>(kb, D, c0 + CH, a.Sk, cols_valid);
            rv = chunk_load<HD>(vb, D, c0 + CH, a.Sk, cols_valid);
        }
        const T* Kc = smem + (t & 1) * BUF + hh * HD;
        const T* Vc = smem + (t & 1) * BUF + VOFF + hh * HD;
        const T* Tc = smem + (t & 1) * BUF + TOFF + (hh * HD) * TS;
        const int jw = min(c0 + CH, jend);
        for (int j0 = c0; j0 < jw; j0 += KS) {
            const int jj = j0 - c0;
            f32x4 s[NQ], dpv[NQ];
            const T* kr = Kc + (jj + li) * Geo<HD>::RS;
            const T* vr = Vc + (jj + li) * Geo<HD>::RS;
#pragma unroll
            for (int u = 0; u < NQ; ++u) {
                s[u] = f32x4{0.f, 0.f, 0.f, 0.f};
                dpv[u] = s[u];
                dot_rows<LP, HD>(s[u], kr + 4 * u * Geo<HD>::RS, qv);
                dot_rows<LP, HD>(dpv[u], vr + 4 * u * Geo<HD>::RS, dov);
            }
            if constexpr (DROP) {          // dS = P (M s dPd - delta): a dropped element still carries -P delta
                const uint32_t dc0 = attn_dropout_c0((uint32_t)n, (uint32_t)a.H, (uint32_t)h, (uint32_t)a.Sq, (uint32_t)i);
#pragma unroll
                for (int e = 0; e < KS / 8; ++e) {
                    uint32_t w[4];
                    philox4x32_10(dc0, a.c1 | (uint32_t)((j0 >> 3) + e), a.key[2], a.key[3], a.key[0], a.key[1], w);
#pragma unroll
                    for (int r = 0; r < 8; ++r) {
                        const float x = dpv[2 * e + (r >> 2)][r & 3];
                        dpv[2 * e + (r >> 2)][r & 3] = dropout_value(w[r >> 1], r, a.threshold) ? x * a.scale : 0.0f;
                    }
                }
            }
            float ds[KS];
#pragma unroll
            for (int u = 0; u < NQ; ++u)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    ds[4 * u + r] = exp2_fast(fmaf(s[u][r], a.c2, -L)) * (dpv[u][r] - dl);
            if (j0 + KS > jw || (a.causal && j0 + KS - 1 > q0)) {
#pragma unroll
                for (int r = 0; r < KS; ++r)
                    if (j0 + r >= jw || (a.causal && j0 + r > i)) ds[r] = 0.0f;
            }
#pragma unroll
            for (int u = 0; u < NQ; ++u) {
                const Vals<LP> dv4 = make_vals<LP>(ds[4 * u], ds[4 * u + 1], ds[4 * u + 2], ds[4 * u + 3]);
#pragma unroll
                for (int g = 0; g < G; ++g) acc_cols<LP>(acc[g], Tc + (4 * g + li) * TS + jj + 4 * u, dv4);
            }
        }
        if (t + 1 < nchunks) {
            T* nb = smem + ((t + 1) & 1) * BUF;
            chunk_store_rows<HD>(nb, rk);
            chunk_store_rows<HD>(nb + VOFF, rv);
            chunk_store_transposed<HD>(nb + TOFF, TS, rk);
        }
        __syncthreads();
    }
    if (active) {
#pragma unroll
        for (int g = 0; g < G; ++g)
            *reinterpret_cast<float4*>(dq + roff + 4 * g) =
                make_float4(acc[g][0] * a.rsd, acc[g][1] * a.rsd, acc[g][2] * a.rsd, acc[g][3] * a.rsd);
        delta[((int64_t)n * a.H + h) * a.Sq + i] = dl;
    }
}

// dK/dV pass: lane = key; per chunk of queries the Q rows, dO rows and both transposed, plus
// the chunk's LSE and delta values (wave-uniform per query: read as LDS broadcasts).
template <int HD, int MAXT, bool LP, bool DROP>
__global__ __launch_bounds__(MAXT) void attn_bwd_dkv_kernel(
    const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
    const float* __restrict__ dO, const float* __restrict__ lse, const float* __restrict__ delta,
    typename DimsOf<DROP>::T a, float* __restrict__ dk, float* __restrict__ dv) {
    typedef typename Elem<LP>::T T;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    T* smem = reinterpret_cast<T*>(smem_raw);
    constexpr int G = HD / 4;
    const int CH = Geo<HD>::chunk_rows();
    const int TS = CH + 4;
    const int KW = blockDim.x >> 8;
    const int KB = KW * 64;
    const int hgroups = (a.H + HPB - 1) / HPB;
    int bid = blockIdx.x;
    const int hg = bid % hgroups; bid /= hgroups;
    const int n = bid % a.N; bid /= a.N;
    const int kbk = bid;                                // earliest key blocks are the heaviest (causal)
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int hh = wave & 3, kq = wave >> 2;
    const int h = hg * HPB + hh;
    const bool head_ok = h < a.H;
    const int D = a.H * HD;
    const int k0 = kbk * KB + kq * 64;                  // first key of this wave
    const int j = k0 + lane;
    const bool active = head_ok && j < a.Sk;
    const int li = lane & 3;
    const int cols_valid = (a.H - hg * HPB) * HD;
    // per buffer (elements of T): Q rows | dO rows | Q^T | dO^T; the LSE / delta arrays
    // ([2 buffers][LSE[4][CH] | delta[4][CH]] floats) sit behind both image buffers
    const int BUF = 2 * CH * Geo<HD>::RS + 2 * Geo<HD>::W * TS;
    const int GOFF = CH * Geo<HD>::RS, QTOFF = 2 * CH * Geo<HD>::RS;
    const int GTOFF = QTOFF + Geo<HD>::W * TS;
    float* ldbase = reinterpret_cast<float*>(smem_raw + (((size_t)2 * BUF * sizeof(T) + 15) & ~(size_t)15));
    const int LDBUF = 2 * HPB * CH;

    const int64_t roff = ((int64_t)n * a.Sk + (active ? j : 0)) * D + h * HD;
    Own<LP, HD> kv, vv;
    own_load<LP, HD>(kv, k + roff, active);
    own_load<LP, HD>(vv, v + roff, active);
    f32x4 dka[G], dva[G];
#pragma unroll
    for (int g = 0; g < G; ++g) { dka[g] = f32x4{0.f, 0.f, 0.f, 0.f}; dva[g] = dka[g]; }

    const float* qbase = q + (int64_t)n * a.Sq * D + hg * HPB * HD;
    const float* gbase = dO + (int64_t)n * a.Sq * D + hg * HPB * HD;
    const float* lb = lse + ((int64_t)n * a.H + hg * HPB) * a.Sq;
    const float* db = delta + ((int64_t)n * a.H + hg * HPB) * a.Sq;
    // causal: only queries i >= first key of the workgroup matter
    const int ibeg_blk = a.causal ? (kbk * KB) / CH * CH : 0;
    const int ibeg = a.causal ? k0 : 0;                 // first query this wave needs
    const int nchunks = a.Sq > ibeg_blk ? (a.Sq - ibeg_blk + CH - 1) / CH : 0;
    // LSE / delta of the chunk: HPB * CH values, one per thread while they last
    const int lrow = threadIdx.x / CH, lcol = threadIdx.x - lrow * CH;
    const bool lth = threadIdx.x < HPB * CH;
    auto load_ld = [&](int c0, float& rl, float& rd) {
        rl = 0.0f; rd = 0.0f;
        if (lth && hg * HPB + lrow < a.H && c0 + lcol < a.Sq) {
            rl = lb[(int64_t)lrow * a.Sq + c0 + lcol];
            rd = db[(int64_t)lrow * a.Sq + c0 + lcol];
        }
    };
    float4 rq, rg;
    float rl, rd;
    if (nchunks > 0) {
        rq = chunk_load<HD>(qbase, D, ibeg_blk, a.Sq, cols_valid);
        rg = chunk_load<HD>(gbase, D, ibeg_blk, a.Sq, cols_valid);
        load_ld(ibeg_blk, rl, rd);
        chunk_store_rows<HD>(smem, rq);
        chunk_store_rows<HD>(smem + GOFF, rg);
        chunk_store_transposed<HD>(smem + QTOFF, TS, rq);
        chunk_store_transposed<HD>(smem + GTOFF, TS, rg);
        if (lth) { ldbase[threadIdx.x] = rl; ldbase[HPB * CH + threadIdx.x] = rd; }
    }
    __syncthreads();
    for (int t = 0; t < nchunks; ++t) {
        const int c0 = ibeg_blk + t * CH;
        if (t + 1 < nchunks) {
            rq = chunk_load<HD>(qbase, D, c0 + CH, a.Sq, cols_valid);
            rg = chunk_load<HD>(gbase, D, c0 + CH, a.Sq, cols_valid);
            load_ld(c0 + CH, rl, rd);
        }
        const T* cb = smem + (t & 1) * BUF;
        const T* Qc = cb + hh * HD;
        const T* Gc = cb + GOFF + hh * HD;
        const T* QTc = cb + QTOFF + (hh * HD) * TS;
        const T* GTc = cb + GTOFF + (hh * HD) * TS;
        const float* Lc = ldbase + (t & 1) * LDBUF + hh * CH;
        const float* Dc = Lc + HPB * CH;
        const int i1 = min(c0 + CH, a.Sq);
        // first 8-aligned step that holds a query this wave needs
        int i0 = c0;
        if (ibeg > c0) i0 = c0 + ((ibeg - c0) & ~7);
        for (; i0 < i1; i0 += 8) {
            const int ii = i0 - c0;
            f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = s0, d0 = s0, d1 = s0;
            const T* qr = Qc + (ii + li) * Geo<HD>::RS;
            const T* gr = Gc + (ii + li) * Geo<HD>::RS;
            dot_rows<LP, HD>(s0, qr, kv);
            dot_rows<LP, HD>(s1, qr + 4 * Geo<HD>::RS, kv);
            dot_rows<LP, HD>(d0, gr, vv);
            dot_rows<LP, HD>(d1, gr + 4 * Geo<HD>::RS, vv);
            const f32x4 La = *reinterpret_cast<const f32x4*>(Lc + ii);
            const f32x4 Lb = *reinterpret_cast<const f32x4*>(Lc + ii + 4);
            const f32x4 Da = *reinterpret_cast<const f32x4*>(Dc + ii);
            const f32x4 Db = *reinterpret_cast<const f32x4*>(Dc + ii + 4);
            float p[8], ds[8];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                p[r] = exp2_fast(fmaf(s0[r], a.c2, -La[r]));
                p[4 + r] = exp2_fast(fmaf(s1[r], a.c2, -Lb[r]));
            }
            if (i0 + 8 > i1 || (a.causal && i0 < k0 + 63)) {         // wave-uniform: edge steps only
#pragma unroll
                for (int r = 0; r < 8; ++r)
                    if (i0 + r >= i1 || (a.causal && j > i0 + r)) p[r] = 0.0f;
            }
            if constexpr (DROP) {
                // lane g = lane & 7 of an aligned group of eight makes the call of query i0 + g for the group's
                // eight keys (k0 is a multiple of 64, so the group shares j >> 3); the group then transposes its
                // 8 x 8 keep bits
                uint32_t w[4];
                philox4x32_10(attn_dropout_c0((uint32_t)n, (uint32_t)a.H, (uint32_t)h, (uint32_t)a.Sq,
                                              (uint32_t)(i0 + (lane & 7))),
                              a.c1 | ((uint32_t)j >> 3), a.key[2], a.key[3], a.key[0], a.key[1], w);
                const uint32_t mk = transpose8(attn_dropout_keep8(w, a.threshold), lane);   // bit r: query i0 + r
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const bool ka = (mk >> r) & 1u, kb = (mk >> (4 + r)) & 1u;
                    ds[r] = p[r] * ((ka ? d0[r] * a.scale : 0.0f) - Da[r]);
                    ds[4 + r] = p[4 + r] * ((kb ? d1[r] * a.scale : 0.0f) - Db[r]);
                    p[r] = ka ? p[r] : 0.0f;              // dV = s sum M P dO: s at the store
                    p[4 + r] = kb ? p[4 + r] : 0.0f;
                }
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    ds[r] = p[r] * (d0[r] - Da[r]);
                    ds[4 + r] = p[4 + r] * (d1[r] - Db[r]);
                }
            }
            const Vals<LP> pa = make_vals<LP>(p[0], p[1], p[2], p[3]);
            const Vals<LP> pb = make_vals<LP>(p[4], p[5], p[6], p[7]);
            const Vals<LP> da = make_vals<LP>(ds[0], ds[1], ds[2], ds[3]);
            const Vals<LP> dbv = make_vals<LP>(ds[4], ds[5], ds[6], ds[7]);
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const T* gt = GTc + (4 * g + li) * TS + ii;
                const T* qt = QTc + (4 * g + li) * TS + ii;
                if constexpr (LP) {
                    acc_cols<LP>(dva[g], gt, pa);
                    acc_cols<LP>(dka[g], qt, da);
                    acc_cols<LP>(dva[g], gt + 4, pb);
                    acc_cols<LP>(dka[g], qt + 4, dbv);
                } else {       // the fp32 chains interleaved as before: dV and dK, query ascending
                    const f32x4 ga = *reinterpret_cast<const f32x4*>(gt);
                    const f32x4 gb4 = *reinterpret_cast<const f32x4*>(gt + 4);
                    const f32x4 qa = *reinterpret_cast<const f32x4*>(qt);
                    const f32x4 qb4 = *reinterpret_cast<const f32x4*>(qt + 4);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        dva[g] = mfma4(ga[r], p[r], dva[g]);
                        dka[g] = mfma4(qa[r], ds[r], dka[g]);
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        dva[g] = mfma4(gb4[r], p[4 + r], dva[g]);
                        dka[g] = mfma4(qb4[r], ds[4 + r], dka[g]);
                    }
                }
            }
        }
        if (t + 1 < nchunks) {
            T* nb = smem + ((t + 1) & 1) * BUF;
            chunk_store_rows<HD>(nb, rq);
            chunk_store_rows<HD>(nb + GOFF, rg);
            chunk_store_transposed<HD>(nb + QTOFF, TS, rq);
            chunk_store_transposed<HD>(nb + GTOFF, TS, rg);
            float* nl = ldbase + ((t + 1) & 1) * LDBUF;
            if (lth) { nl[threadIdx.x] = rl; nl[HPB * CH + threadIdx.x] = rd; }
        }
        __syncthreads();
    }
    if (active) {
#pragma unroll
        for (int g = 0; g < G; ++g) {
            *reinterpret_cast<float4*>(dk + roff + 4 * g) =
                make_float4(dka[g][0] * a.rsd, dka[g][1] * a.rsd, dka[g][2] * a.rsd, dka[g][3] * a.rsd);
            if constexpr (DROP) dva[g] *= a.scale;
            *reinterpret_cast<float4*>(dv + roff + 4 * g) =
                make_float4(dva[g][0], dva[g][1], dva[g][2], dva[g][3]);
        }
    }
}


}  // namespace qarig

using namespace qarig;

#define QARIG_HD_DISPATCH(d, ...)                                              \
    switch (d) {                                                                 \
        case 4: { constexpr int HD = 4; __VA_ARGS__; } break;                           \
        case 8: { constexpr int HD = 8; __VA_ARGS__; } break;                           \
        case 16: { constexpr int HD = 16; __VA_ARGS__; } break;                         \
        case 32: { constexpr int HD = 32; __VA_ARGS__; } break;                         \
        case 64: { constexpr int HD = 64; __VA_ARGS__; } break;                         \
        default:                                                                 \
            qarig_set_error("attention: head dim %d unsupported (4,8,16,32,64,128)", d); \
            return QARIG_ERR_ARG;                                                \
    }

// csrc/attention_wide.hip: head dim 128 (heads of 65 ... 128 arrive zero-padded), exact fp32 in every precision mode
int qarig_attention_wide_fwd(const float* q, const float* k, const float* v, int N, int Sq, int Sk, int H,
                             int causal, float sqrt_d, float* o, float* lse, hipStream_t st);
int qarig_attention_wide_bwd(const float* q, const float* k, const float* v, const float* o, const float* dO,
                             const float* lse, int N, int Sq, int Sk, int H, int causal, float sqrt_d, float* dq,
                             float* dk, float* dv, float* delta, hipStream_t st);
static int attn_wide_check(int N, int Sq, int Sk, int H, int causal) {
    QARIG_CHECK_ARG(N > 0 && Sq > 0 && Sk > 0 && H > 0, "attention: bad extents");
    QARIG_CHECK_DIMS("attention", N, Sq, H);
    QARIG_CHECK_DIMS("attention", N, Sk, H);
    QARIG_CHECK_ARG(H <= 65535 && N <= 65535, "attention (wide heads): more than 65535 heads or sequences");
    QARIG_CHECK_ARG(!causal || Sq == Sk, "attention: causal needs Sq == Sk (self-attention)");
    return QARIG_OK;
}

static int attn_check(int N, int Sq, int Sk, int H, int d, int causal) {
    QARIG_CHECK_ARG(N > 0 && Sq > 0 && Sk > 0 && H > 0 && d > 0, "attention: bad extents");
    QARIG_CHECK_DIMS("attention", N, Sq, H);
    QARIG_CHECK_DIMS("attention", N, Sk, H);
    QARIG_CHECK_ARG(d == 4 || d == 8 || d == 16 || d == 32 || d == 64,
                    "attention: head dim %d unsupported (4,8,16,32,64,128)", d);
    QARIG_CHECK_ARG((long long)N * ((H + 3) / 4) * ((Sq > Sk ? Sq : Sk) / 64 + 1) < (1LL << 31),
                    "attention: too many workgroups");
    QARIG_CHECK_ARG(!causal || Sq == Sk, "attention: causal needs Sq == Sk (self-attention)");
    return QARIG_OK;
}

// Launch geometry: a workgroup covers 4 adjacent heads x (W x 64) rows (queries; keys in the
// dK/dV pass), W waves per head.  W = 4 reads a 256-token sequence's K/V exactly once but leaves
// one 16-wave workgroup per CU; all three passes default to W = 2.
// Options attn_qw / attn_bw override (1, 2 or 4; tuning knob, any value is correct).
static int attn_waves(int rows, int d, int option, int dflt, int wmax) {
    int w = option > 0 ? option : dflt;
    w = w >= 4 ? 4 : (w >= 2 ? 2 : 1);
    if (w > wmax) w = wmax;
    while (w > 1 && (w / 2) * 64 >= rows) w /= 2;      // no more slices than the rows need
    while (w < wmax && (w * 256) / d < 8) w *= 2;       // a chunk holds at least 8 rows
    return w;
}

// register budget: 1024-thread workgroups (4 waves per SIMD) cap a wave at 128 VGPRs, enough for
// the forward pass up to head dim 16; wider heads and the backward passes run 512 threads
#define QARIG_FWD_MAXT(HD) ((HD) <= 16 ? 1024 : 512)

template <typename K>
static int attn_set_lds(K kernel, size_t bytes, const char* what) {
    if (bytes > 160 * 1024) {
        qarig_set_error("%s: needs %zu B of LDS", what, bytes);
        return QARIG_ERR_ARG;
    }
    if (bytes > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        if (e != hipSuccess) {
            qarig_set_error("%s: hipFuncSetAttribute(%zu B LDS): %s", what, bytes, hipGetErrorString(e));
            return QARIG_ERR_LAUNCH;
        }
    }
    return QARIG_OK;
}

// floats of LDS per double-buffered chunk set: `rows` row images + `tr` transposed images (+ LSE/delta)
static size_t attn_lds_bytes(int threads, int d, int rows, int tr, bool ld, int lp) {
    const int W = HPB * d, CH = threads / (W / 4);
    const size_t img = 2 * (lp ? 2 : 4) * ((size_t)rows * CH * (W + 4) + (size_t)tr * W * (CH + 4));
    return ((img + 15) & ~(size_t)15) + (ld ? 2 * sizeof(float) * 2 * HPB * CH : 0);
}

// The arguments the dropout entries add, and what they refuse before any launch.
struct AttnDropArgs {
    uint32_t threshold;
    float scale;
    uint32_t site;
    const uint32_t* key;
};
static int attn_drop_check(const AttnDropArgs& dr, int N, int Sq, int Sk, int H, int d) {
    QARIG_CHECK_ARG(dr.key, "attention dropout: null key");
    QARIG_CHECK_ARG(d != 128, "attention dropout: head dim 128 (the wide-head kernels) is not supported");
    QARIG_CHECK_ARG(dr.threshold >= 1 && dr.threshold <= QARIG_DROPOUT_MAX_THRESHOLD,
                    "attention dropout: threshold must lie in [1, 58982] (0 < p <= 0.9)");
    QARIG_CHECK_ARG(dr.scale > 0.0f && dr.scale <= 16.0f, "attention dropout: scale must lie in (0, 16]");
    QARIG_CHECK_ARG(dr.site < QARIG_ATTN_DROPOUT_SITES, "attention dropout: site must be below 256");
    QARIG_CHECK_ARG(Sk <= QARIG_ATTN_DROPOUT_MAX_SK, "attention dropout: more than 2^26 keys");
    QARIG_CHECK_ARG(N <= 0 || Sq <= 0 || H <= 0 || (long long)N * H * Sq < (1LL << 32),
                    "attention dropout: N * H * Sq must stay below 2^32 (one counter word)");
    return QARIG_OK;
}
template <bool DROP>
static typename DimsOf<DROP>::T attn_dims(const AttnDims& a, const AttnDropArgs* dr) {
    typename DimsOf<DROP>::T ad;
    static_cast<AttnDims&>(ad) = a;
    if constexpr (DROP) {
        ad.threshold = dr->threshold;
        ad.scale = dr->scale;
        ad.c1 = attn_dropout_c1(dr->site, 0);
        ad.key = dr->key;
    }
    return ad;
}

template <bool LP, bool DROP = false>
static int attention_fwd_impl(const float* q, const float* k, const float* v, int N, int Sq, int Sk,
                              int H, int d, int causal, float sqrt_d, float* o, float* lse, void* stream,
                              const AttnDropArgs* dr = nullptr) {
    QARIG_CHECK_ARG(q && k && v && o && lse, "attention_fwd: null pointer");
    if constexpr (DROP)
        if (int e = attn_drop_check(*dr, N, Sq, Sk, H, d)) return e;
    if (d == 128) {
        if (int e = attn_wide_check(N, Sq, Sk, H, causal)) return e;
        QARIG_CHECK_ARG(sqrt_d > 0.0f, "attention: sqrt_d must be positive");
        return qarig_attention_wide_fwd(q, k, v, N, Sq, Sk, H, causal, sqrt_d, o, lse, (hipStream_t)stream);
    }
    if (int e = attn_check(N, Sq, Sk, H, d, causal)) return e;
    AttnDims a{N, Sq, Sk, H, causal, 1.4426950408889634f / sqrt_d, 1.0f / sqrt_d};
    // measured (tools/attn_bench.py, 64 x 256 tokens, 64 heads of 8): W = 1 / 2 / 4 -> 100 / 100 /
    // 124 us; W = 2 reads K and V 1.5x (1.25x of the launch's algorithmic bytes in all) where
    // W = 1 reads them 2.5x, and keeps two workgroups per CU to even out the causal imbalance
    const int W = attn_waves(Sq, d, g_qarig_opt.attn_qw, 2, d <= 16 ? 4 : 2);
    const int threads = 256 * W, rows = 64 * W;
    const size_t lds = attn_lds_bytes(threads, d, 1, 1, false, LP);
    dim3 grid((unsigned)(N * ((H + HPB - 1) / HPB) * ((Sq + rows - 1) / rows))), block(threads);
    const typename DimsOf<DROP>::T ad = attn_dims<DROP>(a, dr);
    QARIG_HD_DISPATCH(d, {
        auto kern = attn_fwd_kernel<HD, QARIG_FWD_MAXT(HD), LP, DROP>;
        if (int e = attn_set_lds(kern, lds, "attention_fwd")) return e;
        hipLaunchKernelGGL(kern, grid, block, lds, (hipStream_t)stream, q, k, v, ad, o, lse);
    });
    QARIG_CHECK_LAUNCH("attention_fwd");
    return QARIG_OK;
}

template <bool LP, bool DROP = false>
static int attention_bwd_impl(const float* q, const float* k, const float* v, const float* o,
                              const float* dO, const float* lse, int N, int Sq, int Sk, int H, int d,
                              int causal, float sqrt_d, float* dq, float* dk, float* dv, float* delta,
                              void* stream, const AttnDropArgs* dr = nullptr) {
    QARIG_CHECK_ARG(q && k && v && o && dO && lse && dq && dk && dv && delta,
                    "attention_bwd: null pointer");
    if constexpr (DROP)
        if (int e = attn_drop_check(*dr, N, Sq, Sk, H, d)) return e;
    if (d == 128) {
        if (int e = attn_wide_check(N, Sq, Sk, H, causal)) return e;
        QARIG_CHECK_ARG(sqrt_d > 0.0f, "attention: sqrt_d must be positive");
        return qarig_attention_wide_bwd(q, k, v, o, dO, lse, N, Sq, Sk, H, causal, sqrt_d, dq, dk, dv, delta,
                                        (hipStream_t)stream);
    }
    if (int e = attn_check(N, Sq, Sk, H, d, causal)) return e;
    AttnDims a{N, Sq, Sk, H, causal, 1.4426950408889634f / sqrt_d, 1.0f / sqrt_d};
    const int hgroups = (H + HPB - 1) / HPB;
    const typename DimsOf<DROP>::T ad = attn_dims<DROP>(a, dr);
    {
        const int W = attn_waves(Sq, d, g_qarig_opt.attn_bw, 2, 2);
        const int threads = 256 * W, rows = 64 * W;
        const size_t lds = attn_lds_bytes(threads, d, 2, 1, false, LP);
        dim3 grid((unsigned)(N * hgroups * ((Sq + rows - 1) / rows))), block(threads);
        QARIG_HD_DISPATCH(d, {
            auto kern = attn_bwd_dq_kernel<HD, 512, LP, DROP>;
            if (int e = attn_set_lds(kern, lds, "attention_bwd dq")) return e;
            hipLaunchKernelGGL(kern, grid, block, lds, (hipStream_t)stream, q, k, v, o, dO, lse, ad, dq, delta);
        });
        QARIG_CHECK_LAUNCH("attention_bwd dq");
    }
    {
        const int W = attn_waves(Sk, d, g_qarig_opt.attn_bw, 2, 2);
        const int threads = 256 * W, rows = 64 * W;
        const size_t lds = attn_lds_bytes(threads, d, 2, 2, true, LP);
        dim3 grid((unsigned)(N * hgroups * ((Sk + rows - 1) / rows))), block(threads);
        QARIG_HD_DISPATCH(d, {
            auto kern = attn_bwd_dkv_kernel<HD, 512, LP, DROP>;
            if (int e = attn_set_lds(kern, lds, "attention_bwd dkv")) return e;
            hipLaunchKernelGGL(kern, grid, block, lds, (hipStream_t)stream, q, k, v, dO, lse, delta, ad, dk, dv);
        });
        QARIG_CHECK_LAUNCH("attention_bwd dkv");
    }
    return QARIG_OK;
}

// q: (N,Sq,H*d); k,v: (N,Sk,H*d); o: (N,Sq,H*d); lse: (N,H,Sq).  sqrt_d is passed by
// the host as float(d ** 0.5), the divisor the reference uses (layers.py:446).
extern "C" int qarig_attention_fwd(const float* q, const float* k, const float* v, int N, int Sq,
                                   int Sk, int H, int d, int causal, float sqrt_d, float* o,
                                   float* lse, void* stream) {
    return attention_fwd_impl<false>(q, k, v, N, Sq, Sk, H, d, causal, sqrt_d, o, lse, stream);
}

// delta: caller-provided (N,H,Sq) scratch.
extern "C" int qarig_attention_bwd(const float* q, const float* k, const float* v, const float* o,
                                   const float* dO, const float* lse, int N, int Sq, int Sk, int H,
                                   int d, int causal, float sqrt_d, float* dq, float* dk, float* dv,
                                   float* delta, void* stream) {
    return attention_bwd_impl<false>(q, k, v, o, dO, lse, N, Sq, Sk, H, d, causal, sqrt_d, dq, dk, dv,
                                     delta, stream);
}

// The same two entry points with the QK^T / PV (and dS-side) products on the bf16 MFMA
// (operands rounded to bf16, fp32 accumulation, softmax and tensors): BASELINE config 5's
// reduced-precision attention; opt-in, never the fp32 parity path.
extern "C" int qarig_attention_lp_fwd(const float* q, const float* k, const float* v, int N, int Sq,
                                      int Sk, int H, int d, int causal, float sqrt_d, float* o,
                                      float* lse, void* stream) {
    return attention_fwd_impl<true>(q, k, v, N, Sq, Sk, H, d, causal, sqrt_d, o, lse, stream);
}
extern "C" int qarig_attention_lp_bwd(const float* q, const float* k, const float* v, const float* o,
                                      const float* dO, const float* lse, int N, int Sq, int Sk, int H,
                                      int d, int causal, float sqrt_d, float* dq, float* dk, float* dv,
                                      float* delta, void* stream) {
    return attention_bwd_impl<true>(q, k, v, o, dO, lse, N, Sq, Sk, H, d, causal, sqrt_d, dq, dk, dv,
                                    delta, stream);
}

// The four entries above with attention-probability dropout: o = ((M s) . softmax(S)) V with the keep
// mask M of csrc/dropout_philox.h, regenerated by the two backward passes; lse is that of the undropped softmax.
// threshold and scale as for qarig_dropout, site < 256, key = DEVICE uint32[4] {seed_lo, seed_hi, step, rank}.
// Head dim 128 is refused.
extern "C" int qarig_attention_dropout_fwd(const float* q, const float* k, const float* v, int N, int Sq, int Sk,
                                           int H, int d, int causal, float sqrt_d, float* o, float* lse,
                                           void* stream, uint32_t threshold, float scale, uint32_t site,
                                           const uint32_t* key) {
    const AttnDropArgs dr{threshold, scale, site, key};
    return attention_fwd_impl<false, true>(q, k, v, N, Sq, Sk, H, d, causal, sqrt_d, o, lse, stream, &dr);
}
extern "C" int qarig_attention_dropout_bwd(const float* q, const float* k, const float* v, const float* o,
                                           const float* dO, const float* lse, int N, int Sq, int Sk, int H, int d,
                                           int causal, float sqrt_d, float* dq, float* dk, float* dv, float* delta,
                                           void* stream, uint32_t threshold, float scale, uint32_t site,
                                           const uint32_t* key) {
    const AttnDropArgs dr{threshold, scale, site, key};
    return attention_bwd_impl<false, true>(q, k, v, o, dO, lse, N, Sq, Sk, H, d, causal, sqrt_d, dq, dk, dv, delta,
                                           stream, &dr);
}
extern "C" int qarig_attention_dropout_lp_fwd(const float* q, const float* k, const float* v, int N, int Sq, int Sk,
                                              int H, int d, int causal, float sqrt_d, float* o, float* lse,
                                              void* stream, uint32_t threshold, float scale, uint32_t site,
                                              const uint32_t* key) {
    const AttnDropArgs dr{threshold, scale, site, key};
    return attention_fwd_impl<true, true>(q, k, v, N, Sq, Sk, H, d, causal, sqrt_d, o, lse, stream, &dr);
}
extern "C" int qarig_attention_dropout_lp_bwd(const float* q, const float* k, const float* v, const float* o,
                                              const float* dO, const float* lse, int N, int Sq, int Sk, int H, int d,
                                              int causal, float sqrt_d, float* dq, float* dk, float* dv,
                                              float* delta, void* stream, uint32_t threshold, float scale,
                                              uint32_t site, const uint32_t* key) {
    const AttnDropArgs dr{threshold, scale, site, key};
    return attention_bwd_impl<true, true>(q, k, v, o, dO, lse, N, Sq, Sk, H, d, causal, sqrt_d, dq, dk, dv, delta,
                                          stream, &dr);
}

// One decode step with a KV cache (generation; no reference counterpart - the reference
// re-runs the whole window per token, generate_images.py:283-307).  q, k_new, v_new, o:
// (B, H*d); kcache/vcache: row j of sequence n at n*batch_stride + j*H*d, at least max_len
// rows.  Attends keys 0..len-1 from the cache plus, when k_new/v_new are non-NULL, the new
// key, which is also stored at row len.  With k_new == NULL (cross-attention against
// precomputed encoder K/V) the cache is read-only.  len_dev (device int, optional)
// overrides len so the call can sit inside a captured graph.  o_mul (B, H*d), optional: the
// output is multiplied elementwise by it (the residual layer's scale(cond), layers.py:293-295).
extern "C" int qarig_attention_decode(const float* q, const float* k_new, const float* v_new,
                                      float* kcache, float* vcache, int B, int H, int d, int len,
                                      const int* len_dev, int max_len, int64_t batch_stride,
                                      float sqrt_d, const float* o_mul, float* o, void* stream) {
    // the decode step's kernels live in decode.hip; this entry keeps o_mul as one row per sequence
    return qarig_decode_attention(q, k_new, v_new, kcache, vcache, B, H, d, len, len_dev, max_len, batch_stride, d,
                                  (int64_t)H * d, sqrt_d, o_mul, (int64_t)H * d, o, stream);
}
