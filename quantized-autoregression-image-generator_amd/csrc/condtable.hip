// Position-table form of the conditioning path.
//
// In the reference every decoder block projects the conditioning tensor `cond` (N,S,D)
// through its ScaleLayer/ShiftLayer Linear layers for EVERY token (models/layers.py:100-153,
// 258-304): 6 (base) or 9 (encoder-decoder) 512x512 GEMMs per layer over N*S rows, 20 % of the
// model's FLOPs.  But `cond` is a function of the token's integer position alone
// (Transformer.py:154-167: pos_cond -> sinusoid -> pos_cond_layer), and a training batch holds
// a few hundred distinct positions among its tens of thousands of tokens.  The host therefore
// evaluates pos_cond_layer and every projection ONCE PER DISTINCT POSITION (a (P,D) table, P =
// position bound) and the per-token consumers read their row of the table through an index:
//   * AdaLN modulate: qarig_layernorm_fwd/bwd with mod_idx (norm.hip);
//   * ResidualLinearLayer's x * scale(cond): qarig_mul_rows_fwd/bwd (here).
// Row r of a GEMM depends on row r of its input only, so the forward values are those of the
// per-token evaluation; in the backward pass the per-token gradients of a table row are summed
// in a fixed order (qarig_segment_sum over the row map built by qarig_rowmap_build):
// deterministic, no atomics.
#include "qarig_common.h"

namespace qarig {

// cnt[p] = number of tokens with idx == p; bad flag for indices outside [0, P).
__global__ __launch_bounds__(256) void rowmap_count_kernel(const int* __restrict__ idx, int M, int P,
                                                           int* __restrict__ cnt,
                                                           int* __restrict__ bad) {
    const int p = blockIdx.x;
    int c = 0;
    for (int r = threadIdx.x; r < M; r += 256) {
        const int v = idx[r];
        c += v == p;
        if (p == 0 && (v < 0 || v >= P)) atomicExch(bad, 1);
    }
    __shared__ int part[4];
    c = (int)wave_sum((float)c);     // counts <= 2^24: exact in fp32
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) cnt[p] = part[0] + part[1] + part[2] + part[3];
}

// offsets[0..P] = exclusive prefix sum of cnt[0..P-1]; one block.
__global__ __launch_bounds__(256) void rowmap_scan_kernel(const int* __restrict__ cnt, int P,
                                                          int* __restrict__ offsets) {
    __shared__ int carry;
    __shared__ int buf[256];
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int base = 0; base < P; base += 256) {
        const int i = base + threadIdx.x;
        const int v = i < P ? cnt[i] : 0;
        buf[threadIdx.x] = v;
        __syncthreads();
        for (int o = 1; o < 256; o <<= 1) {          // Hillis-Steele inclusive scan
            const int t = threadIdx.x >= o ? buf[threadIdx.x - o] : 0;
            __syncthreads();
            buf[threadIdx.x] += t;
            __syncthreads();
        }
        if (i < P) offsets[i] = carry + buf[threadIdx.x] - v;
        __syncthreads();
        if (threadIdx.x == 255) carry += buf[255];
        __syncthreads();
    }
    if (threadIdx.x == 0) offsets[P] = carry;
}

// rows[offsets[p] ...] = the tokens with idx == p, ascending.  One wave per table row.
__global__ __launch_bounds__(64) void rowmap_fill_kernel(const int* __restrict__ idx, int M,
                                                         const int* __restrict__ offsets,
                                                         int* __restrict__ rows) {
    const int p = blockIdx.x, lane = threadIdx.x;
    int run = offsets[p];
    for (int base = 0; base < M; base += 64) {
        const int r = base + lane;
        const bool hit = r < M && idx[r] == p;
        const unsigned long long m = __ballot(hit);
        if (hit) rows[run + __popcll(m & ((1ull << lane) - 1ull))] = r;
        run += __popcll(m);
    }
}

// out[p][c] = sum over the tokens t of table row p of src[t][c].  The block's SG sub-groups
// take the row's tokens round-robin (sub-group s: entries s, s+SG, ...; two loads in flight
// each) and their partial sums are added in sub-group order: a fixed order, so the result is
// run-to-run identical, while 2*SG row reads are in flight instead of one.
constexpr int SEG_GROUPS = 4;
__global__ __launch_bounds__(512) void segment_sum_kernel(const float* __restrict__ src,
                                                          const int* __restrict__ offsets,
                                                          const int* __restrict__ rows, int D,
                                                          float* __restrict__ out) {
    __shared__ float4 part[SEG_GROUPS][128];
    const int p = blockIdx.x;
    const int beg = offsets[p], end = offsets[p + 1];
    const int sg = threadIdx.x >> 7, t = threadIdx.x & 127;
    for (int c0 = blockIdx.y * 512; c0 < D; c0 += gridDim.y * 512) {
        const int c = c0 + t * 4;
        float4 a0 = make_float4(0.f, 0.f, 0.f, 0.f), a1 = a0;
        if (c < D) {
            int e = beg + sg;
            for (; e + SEG_GROUPS < end; e += 2 * SEG_GROUPS) {
                const float4 v0 = *reinterpret_cast<const float4*>(src + (int64_t)rows[e] * D + c);
                const float4 v1 = *reinterpret_cast<const float4*>(src + (int64_t)rows[e + SEG_GROUPS] * D + c);
                a0.x += v0.x; a0.y += v0.y; a0.z += v0.z; a0.w += v0.w;
                a1.x += v1.x; a1.y += v1.y; a1.z += v1.z; a1.w += v1.w;
            }
            if (e < end) {
                const float4 v0 = *reinterpret_cast<const float4*>(src + (int64_t)rows[e] * D + c);
                a0.x += v0.x; a0.y += v0.y; a0.z += v0.z; a0.w += v0.w;
            }
        }
        __syncthreads();
        part[sg][t] = make_float4(a0.x + a1.x, a0.y + a1.y, a0.z + a1.z, a0.w + a1.w);
        __syncthreads();
        if (sg == 0 && c < D) {
            float4 r = part[0][t];
#pragma unroll
            for (int g = 1; g < SEG_GROUPS; ++g) {
                r.x += part[g][t].x; r.y += part[g][t].y; r.z += part[g][t].z; r.w += part[g][t].w;
            }
            *reinterpret_cast<float4*>(out + (int64_t)p * D + c) = r;
        }
    }
}

// y[r][c] = a[r][c] * tab[idx[r]][c]
__global__ void mul_rows_kernel(const float* __restrict__ a, const float* __restrict__ tab,
                                const int* __restrict__ idx, float* __restrict__ y, int M, int D4) {
    const int64_t total = (int64_t)M * D4;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int r = (int)(i / D4), c4 = (int)(i - (int64_t)r * D4);
        const float4 av = reinterpret_cast<const float4*>(a)[i];
        const float4 bv = reinterpret_cast<const float4*>(tab)[(int64_t)idx[r] * D4 + c4];
        reinterpret_cast<float4*>(y)[i] = make_float4(av.x * bv.x, av.y * bv.y, av.z * bv.z, av.w * bv.w);
    }
}

// da = dy * tab[idx[r]],  db_tok = dy * a  (per token; the caller segment-sums it)
__global__ void mul_rows_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ a,
                                    const float* __restrict__ tab, const int* __restrict__ idx,
                                    float* __restrict__ da, float* __restrict__ db_tok, int M,
                                    int D4) {
    const int64_t total = (int64_t)M * D4;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int r = (int)(i / D4), c4 = (int)(i - (int64_t)r * D4);
        const float4 d = reinterpret_cast<const float4*>(dy)[i];
        const float4 av = reinterpret_cast<const float4*>(a)[i];
        const float4 bv = reinterpret_cast<const float4*>(tab)[(int64_t)idx[r] * D4 + c4];
        reinterpret_cast<float4*>(da)[i] = make_float4(d.x * bv.x, d.y * bv.y, d.z * bv.z, d.w * bv.w);
        reinterpret_cast<float4*>(db_tok)[i] = make_float4(d.x * av.x, d.y * av.y, d.z * av.z, d.w * av.w);
    }
}

// ---------------------------------------------------------------------------------------------
// Backward kernels with the table sums inside.  One workgroup of 8 waves per table position p
// walks the position's tokens rows[offsets[p] .. offsets[p+1]), one wave per token row, writes the
// per-token gradient and keeps the per-token table contribution in registers instead of writing
// an (M,D) tensor for segment_sum_kernel to read back.  The sums are formed in
// segment_sum_kernel's order, so the tables are bit-identical to the two-step path: wave w takes
// the entries beg + (w & 3) + 4 * (w >> 2) + 8 j, i.e. waves 0..3 hold accumulator a0 of
// sub-groups 0..3 and waves 4..7 their a1; the sub-group total is a0 + a1 and the totals are added
// in sub-group order.  D == NV * 256, so that one wave holds a whole row (float4 i of a lane covers
// columns (i * 64 + lane) * 4 ...).  The next row's loads are issued before the current row is
// worked on, and its row index one visit earlier still: two rows per wave are in flight.
constexpr int TB_WAVES = 2 * SEG_GROUPS;

__device__ __forceinline__ void f4_acc(float4& a, const float4 v) {
    a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
}

// part[q][w][c] holds, on entry, nothing; acc[q][i] are this wave's sums.  Adds a0 + a1 per
// sub-group, then the sub-group totals in order, and writes out_q[p][:] for q < NQ.
template <int NV, int NQ>
__device__ __forceinline__ void table_sums_store(float4 (&part)[NQ][SEG_GROUPS][NV * 64],
                                                 const float4 (&acc)[NQ][NV], int p, int D,
                                                 float* const (&out)[NQ]) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (w >= SEG_GROUPS) {
#pragma unroll
        for (int q = 0; q < NQ; ++q)
#pragma unroll
            for (int i = 0; i < NV; ++i) part[q][w - SEG_GROUPS][i * 64 + lane] = acc[q][i];
    }
    __syncthreads();
    if (w < SEG_GROUPS) {   // the slot's only reader is the thread that overwrites it
#pragma unroll
        for (int q = 0; q < NQ; ++q)
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                const float4 a1 = part[q][w][i * 64 + lane], a0 = acc[q][i];
                part[q][w][i * 64 + lane] = make_float4(a0.x + a1.x, a0.y + a1.y, a0.z + a1.z, a0.w + a1.w);
            }
    }
    __syncthreads();
    for (int t = threadIdx.x; t < NQ * NV * 64; t += TB_WAVES * 64) {
        const int q = t / (NV * 64), c = t - q * (NV * 64);
        float4 r = part[q][0][c];
#pragma unroll
        for (int g = 1; g < SEG_GROUPS; ++g) f4_acc(r, part[q][g][c]);
        *reinterpret_cast<float4*>(out[q] + (int64_t)p * D + c * 4) = r;
    }
}

// AdaLN backward, scale-table form: per token exactly layernorm_bwd_kernel<NV>'s arithmetic (dx, with
// dx_add where given); per position dscale[p] = sum dy * xhat and dshift[p] = sum dy.
template <int NV>
__global__ __launch_bounds__(TB_WAVES * 64) void layernorm_bwd_table_kernel(
    const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ mean_in,
    const float* __restrict__ rstd_in, const float* __restrict__ scale_tab,
    const int* __restrict__ offsets, const int* __restrict__ rows, int D, float* __restrict__ dx,
    const float* __restrict__ dx_add, float* __restrict__ dscale, float* __restrict__ dshift) {
    __shared__ float4 part[2][SEG_GROUPS][NV * 64];
    const int p = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int beg = offsets[p], end = offsets[p + 1];
    float4 acc[2][NV];    // [0]: dy * xhat, [1]: dy
    float4 m[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        acc[0][i] = acc[1][i] = make_float4(0.f, 0.f, 0.f, 0.f);
        m[i] = *reinterpret_cast<const float4*>(scale_tab + (int64_t)p * D + (i * 64 + lane) * 4);
    }
    struct Row {
        float4 xv[NV], d[NV], a[NV];
        float mean, rstd;
    };
    auto load = [&](Row& t, int row) {
        const int64_t off = (int64_t)row * D;
        t.mean = mean_in[row];
        t.rstd = rstd_in[row];
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int c = (i * 64 + lane) * 4;
            t.xv[i] = *reinterpret_cast<const float4*>(x + off + c);
            t.d[i] = *reinterpret_cast<const float4*>(dy + off + c);
            if (dx_add) t.a[i] = *reinterpret_cast<const float4*>(dx_add + off + c);
        }
    };
    int e = beg + (w & (SEG_GROUPS - 1)) + SEG_GROUPS * (w / SEG_GROUPS);
    int r_cur = e < end ? rows[e] : 0;
    int r_nxt = e + TB_WAVES < end ? rows[e + TB_WAVES] : 0;
    Row cur = {};
    if (e < end) load(cur, r_cur);
    for (; e < end; e += TB_WAVES) {
        Row nxt = cur;
        const int r_nn = e + 2 * TB_WAVES < end ? rows[e + 2 * TB_WAVES] : 0;
        if (e + TB_WAVES < end) load(nxt, r_nxt);
        const int64_t off = (int64_t)r_cur * D;
        const float mean = cur.mean, rstd = cur.rstd;
        float4 h[NV], g[NV];
        float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const float4 xv = cur.xv[i], d = cur.d[i];
            h[i] = make_float4((xv.x - mean) * rstd, (xv.y - mean) * rstd, (xv.z - mean) * rstd,
                               (xv.w - mean) * rstd);
            g[i] = make_float4(d.x * m[i].x, d.y * m[i].y, d.z * m[i].z, d.w * m[i].w);
            s1 += (g[i].x + g[i].y) + (g[i].z + g[i].w);
            s2 = fmaf(g[i].x, h[i].x, s2); s2 = fmaf(g[i].y, h[i].y, s2);
            s2 = fmaf(g[i].z, h[i].z, s2); s2 = fmaf(g[i].w, h[i].w, s2);
        }
        s1 = wave_sum(s1) / (float)D;
        s2 = wave_sum(s2) / (float)D;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int c = (i * 64 + lane) * 4;
            const float4 d = cur.d[i];
            float4 r = make_float4(rstd * ((g[i].x - s1) - h[i].x * s2), rstd * ((g[i].y - s1) - h[i].y * s2),
                                   rstd * ((g[i].z - s1) - h[i].z * s2), rstd * ((g[i].w - s1) - h[i].w * s2));
            if (dx_add) {
                const float4 a = cur.a[i];
                r = make_float4(a.x + r.x, a.y + r.y, a.z + r.z, a.w + r.w);
            }
            *reinterpret_cast<float4*>(dx + off + c) = r;
            f4_acc(acc[0][i], make_float4(d.x * h[i].x, d.y * h[i].y, d.z * h[i].z, d.w * h[i].w));
            f4_acc(acc[1][i], d);
        }
        cur = nxt;
        r_cur = r_nxt;
        r_nxt = r_nn;
    }
    float* const out[2] = {dscale, dshift};
    table_sums_store<NV, 2>(part, acc, p, D, out);
}

// Gate backward: da[r] = dy[r] * tab[p] per token, dg[p] = sum dy[r] * a[r] per position.
template <int NV>
__global__ __launch_bounds__(TB_WAVES * 64) void mul_rows_bwd_table_kernel(
    const float* __restrict__ dy, const float* __restrict__ a, const float* __restrict__ tab,
    const int* __restrict__ offsets, const int* __restrict__ rows, int D, float* __restrict__ da,
    float* __restrict__ dg) {
    __shared__ float4 part[1][SEG_GROUPS][NV * 64];
    const int p = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int beg = offsets[p], end = offsets[p + 1];
    float4 acc[1][NV];
    float4 b[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        acc[0][i] = make_float4(0.f, 0.f, 0.f, 0.f);
        b[i] = *reinterpret_cast<const float4*>(tab + (int64_t)p * D + (i * 64 + lane) * 4);
    }
    struct Row {
        float4 d[NV], av[NV];
    };
    auto load = [&](Row& t, int row) {
        const int64_t off = (int64_t)row * D;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int c = (i * 64 + lane) * 4;
            t.d[i] = *reinterpret_cast<const float4*>(dy + off + c);
            t.av[i] = *reinterpret_cast<const float4*>(a + off + c);
        }
    };
    int e = beg + (w & (SEG_GROUPS - 1)) + SEG_GROUPS * (w / SEG_GROUPS);
    int r_cur = e < end ? rows[e] : 0;
    int r_nxt = e + TB_WAVES < end ? rows[e + TB_WAVES] : 0;
    Row cur = {};
    if (e < end) load(cur, r_cur);
    for (; e < end; e += TB_WAVES) {
        Row nxt = cur;
        const int r_nn = e + 2 * TB_WAVES < end ? rows[e + 2 * TB_WAVES] : 0;
        if (e + TB_WAVES < end) load(nxt, r_nxt);
        const int64_t off = (int64_t)r_cur * D;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int c = (i * 64 + lane) * 4;
            const float4 d = cur.d[i], av = cur.av[i];
            *reinterpret_cast<float4*>(da + off + c) =
                make_float4(d.x * b[i].x, d.y * b[i].y, d.z * b[i].z, d.w * b[i].w);
            f4_acc(acc[0][i], make_float4(d.x * av.x, d.y * av.y, d.z * av.z, d.w * av.w));
        }
        cur = nxt;
        r_cur = r_nxt;
        r_nxt = r_nn;
    }
    float* const out[1] = {dg};
    table_sums_store<NV, 1>(part, acc, p, D, out);
}

}  // namespace qarig

using namespace qarig;

static dim3 ct_grid(int64_t total) {
    int64_t b = (total + 255) / 256;
    return dim3((unsigned)(b > 8192 ? 8192 : (b < 1 ? 1 : b)));
}

// Row map of an index vector: offsets (P+1 ints) and rows (M ints) such that
// rows[offsets[p] .. offsets[p+1]) lists, ascending, the tokens r with idx[r] == p.
// counts: P ints of scratch.  *bad_flag (device int, caller-zeroed) is set if an index lies
// outside [0, P) (the host raises IndexError, as nn.Embedding would).
extern "C" int qarig_rowmap_build(const int* idx, int M, int P, int* counts, int* offsets, int* rows,
                                  int* bad_flag, void* stream) {
    QARIG_CHECK_ARG(idx && counts && offsets && rows && bad_flag && M > 0 && P > 0,
                    "rowmap_build: bad arguments");
    QARIG_CHECK_DIMS("rowmap_build", M);
    QARIG_CHECK_DIMS("rowmap_build", P);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(rowmap_count_kernel, dim3(P), dim3(256), 0, st, idx, M, P, counts, bad_flag);
    QARIG_CHECK_LAUNCH("rowmap count");
    hipLaunchKernelGGL(rowmap_scan_kernel, dim3(1), dim3(256), 0, st, counts, P, offsets);
    QARIG_CHECK_LAUNCH("rowmap scan");
    hipLaunchKernelGGL(rowmap_fill_kernel, dim3(P), dim3(64), 0, st, idx, M, offsets, rows);
    QARIG_CHECK_LAUNCH("rowmap fill");
    return QARIG_OK;
}

// out (P,D) = per-table-row sums of src (M,D) in ascending token order.  D % 4 == 0, 16-B aligned.
extern "C" int qarig_segment_sum(const float* src, const int* offsets, const int* rows, int P, int D,
                                 float* out, void* stream) {
    QARIG_CHECK_ARG(src && offsets && rows && out && P > 0 && D > 0 && D % 4 == 0 &&
                        ((((uintptr_t)src | (uintptr_t)out)) & 15) == 0,
                    "segment_sum: bad arguments (D %% 4 == 0, 16-B aligned)");
    QARIG_CHECK_DIMS("segment_sum", P, D);
    hipLaunchKernelGGL(segment_sum_kernel, dim3(P, (D + 511) / 512), dim3(512), 0,
                       (hipStream_t)stream, src, offsets, rows, D, out);
    QARIG_CHECK_LAUNCH("segment_sum");
    return QARIG_OK;
}

// ResidualLinearLayer's x * scale(cond) with scale(cond) given as a position table
// (models/layers.py:293-295): y[r] = a[r] * tab[idx[r]].
extern "C" int qarig_mul_rows_fwd(const float* a, const float* tab, const int* idx, float* y, int M,
                                  int D, void* stream) {
    QARIG_CHECK_ARG(a && tab && idx && y && M > 0 && D > 0 && D % 4 == 0 &&
                        ((((uintptr_t)a | (uintptr_t)tab | (uintptr_t)y)) & 15) == 0,
                    "mul_rows_fwd: bad arguments (D %% 4 == 0, 16-B aligned)");
    QARIG_CHECK_DIMS("mul_rows_fwd", M, D);
    hipLaunchKernelGGL(mul_rows_kernel, ct_grid((int64_t)M * (D / 4)), dim3(256), 0,
                       (hipStream_t)stream, a, tab, idx, y, M, D / 4);
    QARIG_CHECK_LAUNCH("mul_rows_fwd");
    return QARIG_OK;
}

extern "C" int qarig_mul_rows_bwd(const float* dy, const float* a, const float* tab, const int* idx,
                                  float* da, float* db_tok, int M, int D, void* stream) {
    QARIG_CHECK_ARG(dy && a && tab && idx && da && db_tok && M > 0 && D > 0 && D % 4 == 0 &&
                        ((((uintptr_t)dy | (uintptr_t)a | (uintptr_t)tab | (uintptr_t)da |
                           (uintptr_t)db_tok)) & 15) == 0,
                    "mul_rows_bwd: bad arguments (D %% 4 == 0, 16-B aligned)");
    QARIG_CHECK_DIMS("mul_rows_bwd", M, D);
    hipLaunchKernelGGL(mul_rows_bwd_kernel, ct_grid((int64_t)M * (D / 4)), dim3(256), 0,
                       (hipStream_t)stream, dy, a, tab, idx, da, db_tok, M, D / 4);
    QARIG_CHECK_LAUNCH("mul_rows_bwd");
    return QARIG_OK;
}

// AdaLN backward (scale-table form) with the table gradients inside: dx (M,D) as qarig_layernorm_bwd with
// mod_idx writes it, dscale / dshift (P,D) as qarig_segment_sum of dy * xhat and of dy would -- bit-identical,
// without the (M,D) dy * xhat tensor.  offsets / rows: the row map of the index vector (qarig_rowmap_build);
// tokens no position lists (indices outside [0,P): the bad-index flag is up) get no dx.  D = 256, 512 or
// 1024, 16-B aligned.
extern "C" int qarig_layernorm_bwd_table(const float* dy, const float* x, const float* mean, const float* rstd,
                                         const float* scale_tab, const int* offsets, const int* rows, int M, int P,
                                         int D, float* dx, const float* dx_add, float* dscale, float* dshift,
                                         void* stream) {
    QARIG_CHECK_ARG(dy && x && mean && rstd && scale_tab && offsets && rows && dx && dscale && dshift && M > 0 &&
                        P > 0 && (D == 256 || D == 512 || D == 1024) &&
                        ((((uintptr_t)dy | (uintptr_t)x | (uintptr_t)scale_tab | (uintptr_t)dx | (uintptr_t)dx_add |
                           (uintptr_t)dscale | (uintptr_t)dshift)) & 15) == 0,
                    "layernorm_bwd_table: bad arguments (D = 256, 512 or 1024, 16-B aligned)");
    QARIG_CHECK_DIMS("layernorm_bwd_table", M, D);
    QARIG_CHECK_DIMS("layernorm_bwd_table", P, D);
#define QARIG_LNT_LAUNCH(NV)                                                                                  \
    hipLaunchKernelGGL((layernorm_bwd_table_kernel<NV>), dim3(P), dim3(TB_WAVES * 64), 0, (hipStream_t)stream, \
                       dy, x, mean, rstd, scale_tab, offsets, rows, D, dx, dx_add, dscale, dshift)
    switch (D / 256) {
        case 1: QARIG_LNT_LAUNCH(1); break;
        case 2: QARIG_LNT_LAUNCH(2); break;
        default: QARIG_LNT_LAUNCH(4); break;
    }
#undef QARIG_LNT_LAUNCH
    QARIG_CHECK_LAUNCH("layernorm_bwd_table");
    return QARIG_OK;
}

// Gate backward with the table gradient inside: da (M,D) as qarig_mul_rows_bwd writes it, dg (P,D) as
// qarig_segment_sum of dy * a would -- bit-identical, without the (M,D) product tensor.  Row map, D and
// alignment as for qarig_layernorm_bwd_table.
extern "C" int qarig_mul_rows_bwd_table(const float* dy, const float* a, const float* tab, const int* offsets,
                                        const int* rows, int M, int P, int D, float* da, float* dg, void* stream) {
    QARIG_CHECK_ARG(dy && a && tab && offsets && rows && da && dg && M > 0 && P > 0 &&
                        (D == 256 || D == 512 || D == 1024) &&
                        ((((uintptr_t)dy | (uintptr_t)a | (uintptr_t)tab | (uintptr_t)da | (uintptr_t)dg)) & 15) == 0,
                    "mul_rows_bwd_table: bad arguments (D = 256, 512 or 1024, 16-B aligned)");
    QARIG_CHECK_DIMS("mul_rows_bwd_table", M, D);
    QARIG_CHECK_DIMS("mul_rows_bwd_table", P, D);
#define QARIG_MRT_LAUNCH(NV)                                                                                 \
    hipLaunchKernelGGL((mul_rows_bwd_table_kernel<NV>), dim3(P), dim3(TB_WAVES * 64), 0, (hipStream_t)stream, \
                       dy, a, tab, offsets, rows, D, da, dg)
    switch (D / 256) {
        case 1: QARIG_MRT_LAUNCH(1); break;
        case 2: QARIG_MRT_LAUNCH(2); break;
        default: QARIG_MRT_LAUNCH(4); break;
    }
#undef QARIG_MRT_LAUNCH
    QARIG_CHECK_LAUNCH("mul_rows_bwd_table");
    return QARIG_OK;
}
