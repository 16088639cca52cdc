// Reduced-precision GEMM for BASELINE config 5 (opt-in; never the fp32 parity path):
// bf16 operands IN HBM, products on v_mfma_f32_32x32x16_bf16, fp32 accumulation, the same
// fused fp32 epilogue as the fp32 kernels (gemm_epilogue.h) plus optional bf16 copies of the
// outputs for the next GEMM.  Replaces the Linear contractions of models/layers.py:234-254,
// 330-340, 389-418 when qarig.ops precision is "bf16".
//
//   NT:  C[M,N] = sum_k A[m][k] * B[n][k]      A (M,K), B (N,K) bf16, reduction-contiguous
//        (forward  x W^T;  input gradient  dT W  with the W^T shadow as B)
//   TN:  C[M,N] = sum_k A[k][m] * B[k][n]      A (K,M), B (K,N) bf16, reduction-major
//        (weight gradient  dT^T x: both operands are the row-major activations as they lie)
//   NN:  C[M,N] = sum_k A[m][k] * B[k][n]      A (M,K) reduction-contiguous, B (K,N) reduction-major
//        (input gradient  dT W  on the weight shadow AS STORED (N_out,K_in): no W^T copy)
//
// Tile 128 x 128 x 64, 4 waves (2x2), each wave 2x2 accumulators of 32x32; the operand tiles
// go global -> LDS by global_load_lds_dwordx4 (no VGPR staging) into a 2-stage ring, one
// barrier per k-tile (the structure of gemm_dma_kernel).  The LDS image is lane-linear, so
// the bank swizzles sit on the SOURCE address and on the read (guide rule 21):
//   NT tile [128 rows][64 k]   (128-B rows):  16-B chunk c of row r at chunk c ^ ((r >> 1) & 7): two
//        rows share one 256-B bank line, and a ds_read_b128 lane group (16 lanes, NOT contiguous:
//        rows {0-3,12-15,20-27} or {4-11,16-19,28-31} of the fragment) must land on 16 distinct
//        16-B slots of it -- (r & 7) leaves every read 2-way conflicted (SQ_LDS_BANK_CONFLICT was
//        44 % of the LDS cycles);
//        fragments = one ds_read_b128 per (32-row tile, 16-deep k-step);
//   TN tile [64 k][128 x]      (256-B rows):  chunk c of k-row r at c ^ (((r&3)<<2) | ((r>>2)&3));
//        fragments = two ds_read_b64_tr_b16 (the hardware transpose read: 4 k-rows x 16 columns
//        per 16-lane group, delivered column-major), so the reduction-major activations feed
//        the MFMA without a transposed copy in HBM.
#include <stdlib.h>

#include "gemm_epilogue.h"

namespace qarig {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) void* lds_ptr_lp;
typedef __attribute__((address_space(1))) const void* glb_ptr_lp;
typedef unsigned short bf16_t;   // storage type of a bf16 element

constexpr int LBK = 64;                         // 2-byte elements of reduction depth per staged tile

__device__ __forceinline__ unsigned lds_addr_lp(const bf16_t* p) {
    return (unsigned)(uintptr_t)(__attribute__((address_space(3))) const bf16_t*)p;
}
__device__ __forceinline__ int tn_swz(int r) { return ((r & 3) << 2) | ((r >> 2) & 3); }

// ---------------------------------------------------------------------------------
// The two tiles.  128: 4 waves (2 x 2), two workgroups per CU on 64 KB of static LDS each.
// 256: 16 waves (4 x 4, each the same 64 x 64 sub-tile), one workgroup per CU with a 2-stage ring
// of 64 KB stages (128 KB of dynamic LDS).  Why the second exists: the 128 x 128 tile keeps
// 2 x 32 KB of operands in flight per CU; at ~1 us of DMA latency that bounds it near 1 PF however
// the loop is scheduled (slope of time against K at M = 32768: 0.137 us per k).  A 256 x 256 tile
// does twice the MFMA work per byte, so the same 64 KB in flight covers twice the rate.
// Operand images: NT tiles are [ROWS rows][64 k] (128-B rows whatever the tile); TN tiles
// [64 k][ROWS x] with 2 ROWS-byte rows, chunk c of k-row r at c ^ tn_swz(r) (the swizzle permutes
// inside 256-B halves, which is what the transposing reads need).
template <int ROWS_>
struct LpTile {
    static constexpr int ROWS = ROWS_;
    static constexpr int WAVES = ROWS / 64;          // per side (2 or 4); wave w has sub-tile (w / WAVES, w % WAVES)
    static constexpr int WAVES_LOG2 = WAVES == 2 ? 1 : 2;
    static constexpr int DMAS = (ROWS / 8) / (WAVES * WAVES);   // 1 KiB DMA instructions per wave and operand tile
    static constexpr int OP = ROWS * LBK;            // bf16 elements per operand tile (16 / 32 KB)
    static constexpr int STAGE = 2 * OP;             // A then B
    static constexpr int PITCH = 2 * ROWS;           // bytes per k-row of a TN image
    static constexpr int CHUNKS_LOG2 = ROWS == 128 ? 4 : 5;     // log2 of its 16-B chunks (PITCH / 16)
    static_assert(ROWS == 128 || ROWS == 256, "the two tiles");
};
constexpr int LPB = 256;                             // extent of the larger tile (host side)

// This wave's share of one operand tile: LpTile::DMAS instructions of 1 KiB.
template <bool TN, int ROWS>
__device__ __forceinline__ void lp_stage(const bf16_t* __restrict__ P, int64_t ld, int x0, int k0,
                                         bf16_t* tile, int wave, int lane) {
    constexpr int PER = LpTile<ROWS>::DMAS;
    constexpr int SH = LpTile<ROWS>::CHUNKS_LOG2;   // TN: 64 >> SH k-rows per instruction
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int q = wave * PER + i;
        const bf16_t* src;
        if (!TN) {   // [x][k]: 8 rows x 128 B per instruction
            const int r = q * 8 + (lane >> 3);
            const int c = (lane & 7) ^ ((r >> 1) & 7);
            src = P + (int64_t)(x0 + r) * ld + k0 + c * 8;
        } else {     // [k][x]: 4 k-rows x 256 B (2 x 512 B) per instruction
            const int r = q * (64 >> SH) + (lane >> SH);
            const int c = (lane & ((1 << SH) - 1)) ^ tn_swz(r);
            src = P + (int64_t)(k0 + r) * ld + x0 + c * 8;
        }
        __builtin_amdgcn_global_load_lds((glb_ptr_lp)src, (lds_ptr_lp)(tile + q * 512), 16, 0, 0);
    }
}

// A bf16 MFMA operand.  The LDS reads are inline asm (hipcc would otherwise drain the DMA queue in
// front of every LDS read); their destination registers are touched again only in value(), which
// callers invoke behind the lgkmcnt wait.
//   NT image: one ds_read_b128 per fragment;
//   TN image: two ds_read_b64_tr_b16 (the hardware transpose read: 4 k-rows x 16 columns per
//   16-lane group, delivered column-major), so the reduction-major activations feed the MFMA
//   without a transposed copy in HBM.
typedef short s16x4_lp __attribute__((ext_vector_type(4)));
typedef short s16x8_lp __attribute__((ext_vector_type(8)));
template <bool TN> struct LpFrag {
    bf16x8 v;
    __device__ __forceinline__ bf16x8 value() const { return v; }
};
template <> struct LpFrag<true> {
    s16x4_lp lo, hi;
    __device__ __forceinline__ bf16x8 value() const {
        const s16x8_lp both = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        return __builtin_bit_cast(bf16x8, both);
    }
};
// 32x32x16: the 32-row (column) tile starting at x0 for k-step ks (16 deep): lane l holds element
// j = operand(x0 + (l & 31), k = 16 ks + 8 (l >> 5) + j).
template <bool TN, int PITCH>
__device__ __forceinline__ void lp_frag(const bf16_t* tile, int x0, int ks, int lane, LpFrag<TN>& f) {
    if constexpr (!TN) {
        const int r = x0 + (lane & 31);
        const int c = (ks * 2 + (lane >> 5)) ^ ((r >> 1) & 7);
        const unsigned a = lds_addr_lp(tile) + r * 128 + (c << 4);
        asm volatile("ds_read_b128 %0, %1" : "=v"(f.v) : "v"(a));
    } else {
        const int g = lane >> 4, w = lane & 15, q = w >> 2, p = w & 3;
        const int ch = ((x0 + 16 * (g & 1)) >> 3) + (p >> 1);
        const int r0 = ks * 16 + 8 * (g >> 1) + q;
        const int r1 = r0 + 4;
        const unsigned base = lds_addr_lp(tile) + 8 * (p & 1);
        const unsigned a0 = base + PITCH * r0 + ((ch ^ tn_swz(r0)) << 4);
        const unsigned a1 = base + PITCH * r1 + ((ch ^ tn_swz(r1)) << 4);
        asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(f.lo) : "v"(a0));
        asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(f.hi) : "v"(a1));
    }
}
// 16x16x32: lane l holds row (column) x0 + (l & 15), k = 32 ks + 8 (l >> 4) ... + 7.
template <bool TN, int PITCH>
__device__ __forceinline__ void lp16_frag(const bf16_t* tile, int x0, int ks, int lane, LpFrag<TN>& f) {
    if constexpr (!TN) {
        const int r = x0 + (lane & 15);
        const int c = (ks * 4 + (lane >> 4)) ^ ((r >> 1) & 7);
        const unsigned a = lds_addr_lp(tile) + r * 128 + (c << 4);
        asm volatile("ds_read_b128 %0, %1" : "=v"(f.v) : "v"(a));
    } else {   // PITCH-byte k-rows: two transposing reads of 4 k-rows x 16 columns per 16-lane group
        const int g = lane >> 4, w = lane & 15, q = w >> 2, p = w & 3;
        const int ch = (x0 >> 3) + (p >> 1);
        const int r0 = ks * 32 + 8 * g + q;
        const int r1 = r0 + 4;
        const unsigned base = lds_addr_lp(tile) + 8 * (p & 1);
        const unsigned a0 = base + PITCH * r0 + ((ch ^ tn_swz(r0)) << 4);
        const unsigned a1 = base + PITCH * r1 + ((ch ^ tn_swz(r1)) << 4);
        asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(f.lo) : "v"(a0));
        asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(f.hi) : "v"(a1));
    }
}

// fp8 (OCP e4m3) operands: BASELINE config 5 names the fp8 MFMA.  NT layout only (the forward
// products x W^T): A (M,K) and B (N,K) are bytes; products on v_mfma_f32_32x32x64_f8f6f4 (64 deep
// per instruction, twice the bf16 rate), fp32 accumulation.  A 128-deep k-tile is 128 bytes per
// row: the LDS image, its DMA and its chunk swizzle are exactly those of the bf16 NT tile
// (lp_stage<false> on the bytes seen as 2-byte elements).
// Fragment for k-step ks (64 deep): lane l holds the 32 bytes k = 64 ks + 32 (l >> 5) ... + 31 of
// row x0 + (l & 31) = two 16-B chunks.
typedef int i32x8_f8 __attribute__((ext_vector_type(8)));
typedef int i32x4_f8 __attribute__((ext_vector_type(4)));
struct F8Frag {
    i32x4_f8 lo, hi;
    __device__ __forceinline__ i32x8_f8 value() const {
        return i32x8_f8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    }
};
// MX: the block-scaled instruction takes its 64 k as four 16-byte groups -- bytes 0-15 of lanes 0-31,
// bytes 0-15 of lanes 32-63, bytes 16-31 of lanes 0-31, bytes 16-31 of lanes 32-63 -- and scales
// the first 32 with the byte of lanes 0-31, the last 32 with that of lanes 32-63 (measured on exact
// data: tests/test_gpu_mxfp8.py).  So lane l holds k = 64 ks + 16 (l >> 5) ... + 15 and 64 ks + 32 +
// 16 (l >> 5) ... + 15 there, and each 32-block of memory meets one scale.  (Unscaled, any order
// that A and B share gives the same sums.)
template <bool MX>
__device__ __forceinline__ void f8_frag(const bf16_t* tile, int x0, int ks, int lane, F8Frag& f) {
    const int r = x0 + (lane & 31);
    const int c0 = MX ? ks * 4 + (lane >> 5) : ks * 4 + (lane >> 5) * 2;
    const int c1 = MX ? c0 + 2 : c0 + 1;
    const unsigned base = lds_addr_lp(tile) + r * 128;
    const unsigned a0 = base + (((c0) ^ ((r >> 1) & 7)) << 4), a1 = base + (((c1) ^ ((r >> 1) & 7)) << 4);
    asm volatile("ds_read_b128 %0, %1" : "=v"(f.lo) : "v"(a0));
    asm volatile("ds_read_b128 %0, %1" : "=v"(f.hi) : "v"(a1));
}

// MX (OCP microscaling, include/qarig.h "MX-e4m3"): each operand carries one e8m0 scale byte per 32
// elements along k, row-major (rows, K/32); a 128-deep k-tile needs 4 contiguous bytes of each row.
// In k-step ks, lanes 0-31 feed the scale byte of block 2 ks of their row and lanes 32-63 that of
// block 2 ks + 1 (f8_frag<true> lays the bytes out to match) to v_mfma_scale_f32_32x32x64_f8f6f4
// (op_sel 0: the byte sits in bits 0-7), the hardware multiplies every 32-product group by
// 2^(Ea - 127) 2^(Eb - 127), and the epilogue has no dequantisation factor.  The scale dwords ride
// in the operand ring (mx_stage_scales), behind its two stages.
struct MxScales {
    const unsigned char* sa; int64_t ldsa;   // (M, K/32) scale bytes of A, row stride in bytes
    const unsigned char* sb; int64_t ldsb;   // (N, K/32) of B
    int splitk; float* slabs;
};
// A k-tile's scales travel with its operand tiles: this wave's DMA of ROWS x 4 bytes of A (waves
// 0..ROWS/64-1) or of B (the next ROWS/64 waves), 64 rows per instruction, into the stage's scale image
// [A rows][B rows] of dwords; the loop's vmcnt wait and barrier cover it like the operand tiles.
template <int ROWS>
__device__ __forceinline__ void mx_stage_scales(const MxScales& mx, int m0, int n0, int k0, bf16_t* img,
                                                int wave, int lane) {
    constexpr int PER = ROWS / 64;
    if (wave < 2 * PER) {
        const bool b = wave >= PER;
        const int r = (b ? wave - PER : wave) * 64 + lane;
        const unsigned char* src = b ? mx.sb + (int64_t)(n0 + r) * mx.ldsb : mx.sa + (int64_t)(m0 + r) * mx.ldsa;
        __builtin_amdgcn_global_load_lds((glb_ptr_lp)(src + (k0 >> 5)), (lds_ptr_lp)(img + wave * 128), 4, 0, 0);
    }
}
// This lane's byte address in a stage's scale image: row `row` of the A (b = 0) or B half, byte
// lane >> 5; fragment i of k-step ks then reads byte offset 128 i + 2 ks (an immediate, so the loop
// keeps one address register per operand).  Inline asm like the fragment reads: the value is
// consumed behind the lgkmcnt wait.
__device__ __forceinline__ unsigned mx_scale_addr(const bf16_t* img, int row, int lane) {
    return lds_addr_lp(img) + row * 4 + (lane >> 5);
}
template <int OFF>
__device__ __forceinline__ void mx_scale_read(unsigned addr, int& v) {
    asm volatile("ds_read_u8 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "i"(OFF));
}
// fragment I of k-step ks: ks is 0 or 1 and a constant once the caller's loop is unrolled
template <int I>
__device__ __forceinline__ void mx_scale_read_frag(unsigned addr, int ks, int& v) {
    if (ks == 0) mx_scale_read<128 * I>(addr, v);
    else mx_scale_read<128 * I + 2>(addr, v);
}

// ---------------------------------------------------------------------------------
// The three math policies.  Each owns the accumulator type, the fragments of NB k-steps (Frags<NB>:
// NF fragments of FROWS rows per side and k-step), the request of one A / B fragment from a stage
// (frag_a / frag_b), the MX scale reads of k-steps [ks0, ks0 + NB) for the wave's sub-tile at rows xa
// of A and xb of B (scales; `sc` = the stage's scale image), and the MFMAs on a batch (mma).  The
// loop over a batch's fragments is lp_ring's: with it inside the policy, behind one more call, the
// TN 256-tile 32x32x16 kernel spilled its zeroed accumulators (232 B of scratch per lane against 52).
//   KSTEPS   k-steps per stage;
//   KDIV     operand elements per 2-byte element of the staged image;
//   SPLITK   whether blockIdx.z slices K;
//   SC       bf16_t units of scale image per stage and tile row;
//   BIG_PRE  what the 256-tile epilogue prefetches (gemm_epilogue.h).
struct LpNoParams {};
__device__ __forceinline__ void acc_zero(Acc16& acc) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc.t[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
}

// bf16 on v_mfma_f32_32x32x16_bf16: 2 x 2 accumulators of 32 x 32, four 16-deep k-steps.
template <bool A_TN, bool B_TN>
struct LpMath32 {
    static constexpr bool TNA = A_TN, TNB = B_TN;
    using AccT = Acc;
    using Params = LpNoParams;
    static constexpr int KSTEPS = 4, KDIV = 1, SC = 0, BIG_PRE = 1;
    static constexpr bool SPLITK = true;
    template <int NB> struct Frags { LpFrag<TNA> a[NB][2]; LpFrag<TNB> b[NB][2]; };
    template <int ROWS>
    static __device__ __forceinline__ void stage_params(const Params&, int, int, int, bf16_t*, int, int) {}
    static constexpr int NF = 2, FROWS = 32;   // fragments per side and k-step, rows of each
    template <int PITCH>
    static __device__ __forceinline__ void frag_a(const bf16_t* t, int x0, int ks, int lane, LpFrag<TNA>& f) {
        lp_frag<TNA, PITCH>(t, x0, ks, lane, f);
    }
    template <int PITCH>
    static __device__ __forceinline__ void frag_b(const bf16_t* t, int x0, int ks, int lane, LpFrag<TNB>& f) {
        lp_frag<TNB, PITCH>(t, x0, ks, lane, f);
    }
    template <int ROWS, int NB>
    static __device__ __forceinline__ void scales(Frags<NB>&, const bf16_t*, int, int, int, int) {}
    template <int NB>
    static __device__ __forceinline__ void mma(AccT& acc, const Frags<NB>& f) {
#pragma unroll
        for (int ks = 0; ks < NB; ++ks)
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc.t[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.a[ks][i].value(), f.b[ks][j].value(),
                                                                          acc.t[i][j], 0, 0, 0);
    }
};

// bf16 on v_mfma_f32_16x16x32_bf16 (option lp_mfma16 = 1, the default): same bytes, same LDS images,
// same cycles per FLOP as the 32x32x16 form; the chip is reported to hold a higher clock on this
// shape under load (MI355X_MICROARCH.md, DVFS give-back item 7), so both exist and wall time decides.
// 4 x 4 accumulators of 16 x 16, two 32-deep k-steps.
template <bool A_TN, bool B_TN>
struct LpMath16 {
    static constexpr bool TNA = A_TN, TNB = B_TN;
    using AccT = Acc16;
    using Params = LpNoParams;
    static constexpr int KSTEPS = 2, KDIV = 1, SC = 0, BIG_PRE = 1;
    static constexpr bool SPLITK = true;
    template <int NB> struct Frags { LpFrag<TNA> a[NB][4]; LpFrag<TNB> b[NB][4]; };
    template <int ROWS>
    static __device__ __forceinline__ void stage_params(const Params&, int, int, int, bf16_t*, int, int) {}
    static constexpr int NF = 4, FROWS = 16;   // fragments per side and k-step, rows of each
    template <int PITCH>
    static __device__ __forceinline__ void frag_a(const bf16_t* t, int x0, int ks, int lane, LpFrag<TNA>& f) {
        lp16_frag<TNA, PITCH>(t, x0, ks, lane, f);
    }
    template <int PITCH>
    static __device__ __forceinline__ void frag_b(const bf16_t* t, int x0, int ks, int lane, LpFrag<TNB>& f) {
        lp16_frag<TNB, PITCH>(t, x0, ks, lane, f);
    }
    template <int ROWS, int NB>
    static __device__ __forceinline__ void scales(Frags<NB>&, const bf16_t*, int, int, int, int) {}
    template <int NB>
    static __device__ __forceinline__ void mma(AccT& acc, const Frags<NB>& f) {
#pragma unroll
        for (int ks = 0; ks < NB; ++ks)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    acc.t[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f.a[ks][i].value(), f.b[ks][j].value(),
                                                                          acc.t[i][j], 0, 0, 0);
    }
};

// e4m3 on v_mfma_(scale_)f32_32x32x64_f8f6f4: two 64-deep k-steps.  MX = false: per-tensor scales,
// applied by the epilogue, no split-K.  MX = true: the block scales of MxScales ride in the ring and
// go to the instruction; blockIdx.z slices K like the bf16 products do (fp32 slabs reduced by
// qarig_slab_reduce_f32).
template <bool MX>
struct LpMathF8 {
    static constexpr bool TNA = false, TNB = false;
    using AccT = Acc;
    using Params = MxScales;
    static constexpr int KSTEPS = 2, KDIV = 2, SC = MX ? 4 : 0, BIG_PRE = MX ? 1 : 0;
    static constexpr bool SPLITK = MX;
    template <int NB> struct Frags { F8Frag a[NB][2], b[NB][2]; int ea[NB][2], eb[NB][2]; };
    template <int ROWS>
    static __device__ __forceinline__ void stage_params(const Params& mx, int m0, int n0, int k0, bf16_t* img,
                                                        int wave, int lane) {
        if constexpr (MX) mx_stage_scales<ROWS>(mx, m0, n0, k0, img, wave, lane);
    }
    static constexpr int NF = 2, FROWS = 32;
    template <int PITCH>
    static __device__ __forceinline__ void frag_a(const bf16_t* t, int x0, int ks, int lane, F8Frag& f) {
        f8_frag<MX>(t, x0, ks, lane, f);
    }
    template <int PITCH>
    static __device__ __forceinline__ void frag_b(const bf16_t* t, int x0, int ks, int lane, F8Frag& f) {
        f8_frag<MX>(t, x0, ks, lane, f);
    }
    // the scale bytes of k-steps [ks0, ks0 + NB), behind the fragment requests (B's rows follow A's ROWS)
    template <int ROWS, int NB>
    static __device__ __forceinline__ void scales(Frags<NB>& f, const bf16_t* sc, int xa, int xb, int ks0, int lane) {
        if constexpr (MX) {
            const unsigned sa = mx_scale_addr(sc, xa + (lane & 31), lane);
            const unsigned sb = mx_scale_addr(sc, ROWS + xb + (lane & 31), lane);
#pragma unroll
            for (int ks = 0; ks < NB; ++ks) {
                mx_scale_read_frag<0>(sa, ks0 + ks, f.ea[ks][0]);
                mx_scale_read_frag<1>(sa, ks0 + ks, f.ea[ks][1]);
            }
#pragma unroll
            for (int ks = 0; ks < NB; ++ks) {
                mx_scale_read_frag<0>(sb, ks0 + ks, f.eb[ks][0]);
                mx_scale_read_frag<1>(sb, ks0 + ks, f.eb[ks][1]);
            }
        }
    }
    template <int NB>
    static __device__ __forceinline__ void mma(AccT& acc, const Frags<NB>& f) {
#pragma unroll
        for (int ks = 0; ks < NB; ++ks)
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    if constexpr (MX)
                        acc.t[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(
                            f.a[ks][i].value(), f.b[ks][j].value(), acc.t[i][j], 0, 0, 0, f.ea[ks][i], 0, f.eb[ks][j]);
                    else
                        acc.t[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(
                            f.a[ks][i].value(), f.b[ks][j].value(), acc.t[i][j], 0, 0, 0, 0, 0, 0);
                }
    }
};

// ---------------------------------------------------------------------------------
// The ring loop of all six kernels: tile T on math P.  `lds`: 2 stages of T::STAGE (then 2 scale
// images, MX); A / B, lda / ldb and the staged k offsets count 2-byte elements, K and the split-K
// slices count operand elements (P::KDIV of them per 2-byte element).  The host guarantees that
// K / splitk is a multiple of the k-tile.
template <class T, class P>
__device__ __forceinline__ void lp_ring(bf16_t* lds, const bf16_t* A, int64_t lda, const bf16_t* B, int64_t ldb,
                                        const GemmEpilogue& ep, int M, int N, int K, int tiles_n, int splitk,
                                        float* slabs, const typename P::Params& pp) {
    constexpr int ROWS = T::ROWS;
    constexpr int BK = LBK * P::KDIV;                   // operand elements per k-tile
    constexpr int SC = P::SC * ROWS;                    // scale image per stage (bf16_t units)
    // Fragments requested per lgkmcnt wait.  128-tile: the whole stage, then one wait -- the other
    // resident waves' MFMAs cover the reads (interleaving reads per k-step measured 8-17 % slower).
    // 256-tile: half a stage at a time (4 waves per SIMD: 128 VGPRs each).
    constexpr int NB = ROWS == 128 ? P::KSTEPS : P::KSTEPS / 2;
    bf16_t* const scl = lds + 2 * T::STAGE;
    const int tile = xcd_remap(blockIdx.x, gridDim.x);
    const int tm = tile / tiles_n, tn = tile - tm * tiles_n;
    const int m0 = tm * ROWS, n0 = tn * ROWS;
    int k_begin = 0, k_end = K;
    if (P::SPLITK && splitk > 1) {
        const int per = K / splitk;
        k_begin = blockIdx.z * per;
        k_end = k_begin + per;
    }
    const int nk = (k_end - k_begin) / BK;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> T::WAVES_LOG2, wn = wave & (T::WAVES - 1);

    typename P::AccT acc;
    acc_zero(acc);
    if (nk > 0) {
        lp_stage<P::TNA, ROWS>(A, lda, m0, k_begin / P::KDIV, lds, wave, lane);
        lp_stage<P::TNB, ROWS>(B, ldb, n0, k_begin / P::KDIV, lds + T::OP, wave, lane);
        P::template stage_params<ROWS>(pp, m0, n0, k_begin, scl, wave, lane);
        for (int kt = 0; kt < nk; ++kt) {
            // this wave's DMAs of tile kt have landed, then (barrier) everybody's; the same barrier
            // retires all reads of tile kt-1, whose stage is refilled right after it
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            const int st = kt & 1;
            if (kt + 1 < nk) {
                const int kn = k_begin / P::KDIV + (kt + 1) * LBK;
                lp_stage<P::TNA, ROWS>(A, lda, m0, kn, lds + (st ^ 1) * T::STAGE, wave, lane);
                lp_stage<P::TNB, ROWS>(B, ldb, n0, kn, lds + (st ^ 1) * T::STAGE + T::OP, wave, lane);
                P::template stage_params<ROWS>(pp, m0, n0, P::KDIV * kn, scl + (st ^ 1) * SC, wave, lane);
            }
            const bf16_t* ta = lds + st * T::STAGE;
            const bf16_t* tb = ta + T::OP;
#pragma unroll
            for (int ks0 = 0; ks0 < P::KSTEPS; ks0 += NB) {
                typename P::template Frags<NB> f;
#pragma unroll
                for (int ks = 0; ks < NB; ++ks)
#pragma unroll
                    for (int i = 0; i < P::NF; ++i) {
                        P::template frag_a<T::PITCH>(ta, wm * 64 + i * P::FROWS, ks0 + ks, lane, f.a[ks][i]);
                        P::template frag_b<T::PITCH>(tb, wn * 64 + i * P::FROWS, ks0 + ks, lane, f.b[ks][i]);
                    }
                P::template scales<ROWS, NB>(f, scl + st * SC, wm * 64, wn * 64, ks0, lane);
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_sched_barrier(0);
                P::template mma<NB>(acc, f);
                if constexpr (NB < P::KSTEPS) __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
    __syncthreads();                      // ring no longer in use: the epilogue stages through it
    float* const stage = reinterpret_cast<float*>(lds);
    if constexpr (ROWS == 128 && __is_same(typename P::AccT, Acc))
        gemm_epilogue_wide<2>(acc, ep, stage, m0, n0, M, N, splitk, slabs);
    else   // one 8 KB slice per wave
        gemm_epilogue_wave<2, typename P::AccT, ROWS == 128 ? 2 : P::BIG_PRE>(
            acc, ep, stage + wave * (32 * 64), m0 + wm * 64, n0 + wn * 64, M, N, splitk, slabs);
}

// The entry points: a tile, a math policy and the LDS they run in.
template <bool TNA, bool TNB>
__global__ __launch_bounds__(NTHREADS, 2) void gemm_lp_kernel(const bf16_t* __restrict__ A, int64_t lda,
                                                              const bf16_t* __restrict__ B, int64_t ldb,
                                                              GemmEpilogue ep, int M, int N, int K,
                                                              int tiles_n, int splitk, float* slabs) {
    __shared__ __attribute__((aligned(16))) bf16_t lds[2 * LpTile<128>::STAGE];   // 64 KB: 2 workgroups per CU
    lp_ring<LpTile<128>, LpMath32<TNA, TNB>>(lds, A, lda, B, ldb, ep, M, N, K, tiles_n, splitk, slabs, {});
}
template <bool TNA, bool TNB>
__global__ __launch_bounds__(1024, 1) void gemm_lp_big_kernel(const bf16_t* __restrict__ A, int64_t lda,
                                                              const bf16_t* __restrict__ B, int64_t ldb,
                                                              GemmEpilogue ep, int M, int N, int K,
                                                              int tiles_n, int splitk, float* slabs) {
    extern __shared__ __attribute__((aligned(16))) bf16_t ldsb[];   // 2 x 64 KB
    lp_ring<LpTile<256>, LpMath32<TNA, TNB>>(ldsb, A, lda, B, ldb, ep, M, N, K, tiles_n, splitk, slabs, {});
}
template <bool TNA, bool TNB>
__global__ __launch_bounds__(NTHREADS, 2) void gemm_lp16_kernel(const bf16_t* __restrict__ A, int64_t lda,
                                                                const bf16_t* __restrict__ B, int64_t ldb,
                                                                GemmEpilogue ep, int M, int N, int K,
                                                                int tiles_n, int splitk, float* slabs) {
    __shared__ __attribute__((aligned(16))) bf16_t lds[2 * LpTile<128>::STAGE];   // 64 KB: 2 workgroups per CU
    lp_ring<LpTile<128>, LpMath16<TNA, TNB>>(lds, A, lda, B, ldb, ep, M, N, K, tiles_n, splitk, slabs, {});
}
template <bool TNA, bool TNB>
__global__ __launch_bounds__(1024, 1) void gemm_lp_big16_kernel(const bf16_t* __restrict__ A, int64_t lda,
                                                                const bf16_t* __restrict__ B, int64_t ldb,
                                                                GemmEpilogue ep, int M, int N, int K,
                                                                int tiles_n, int splitk, float* slabs) {
    extern __shared__ __attribute__((aligned(16))) bf16_t ldsm[];   // 2 x 64 KB
    lp_ring<LpTile<256>, LpMath16<TNA, TNB>>(ldsm, A, lda, B, ldb, ep, M, N, K, tiles_n, splitk, slabs, {});
}

// The e4m3 kernels see their byte matrices as 2-byte elements: leading dimensions halve.  The MX
// instantiations (gemm_f8_kernel<true, MxScales>) take the MxScales as one more argument, which also
// carries their split-K; the per-tensor ones (gemm_f8_kernel<false>) keep the argument list, and so
// the kernarg layout, they always had.
__device__ __forceinline__ MxScales mx_scales() { return MxScales{nullptr, 0, nullptr, 0, 1, nullptr}; }
__device__ __forceinline__ MxScales mx_scales(const MxScales& m) { return m; }

template <bool MX, class... MxArg>
__global__ __launch_bounds__(NTHREADS, 2) void gemm_f8_kernel(const unsigned char* __restrict__ A, int64_t lda,
                                                              const unsigned char* __restrict__ B, int64_t ldb,
                                                              GemmEpilogue ep, int M, int N, int K, int tiles_n,
                                                              MxArg... mx_arg) {
    __shared__ __attribute__((aligned(16))) bf16_t lds[2 * LpTile<128>::STAGE + 2 * LpMathF8<MX>::SC * 128];   // 64 KB (+2 KB MX)
    const MxScales mx = mx_scales(mx_arg...);
    lp_ring<LpTile<128>, LpMathF8<MX>>(lds, reinterpret_cast<const bf16_t*>(A), lda / 2,
                                       reinterpret_cast<const bf16_t*>(B), ldb / 2, ep, M, N, K, tiles_n, mx.splitk,
                                       mx.slabs, mx);
}
template <bool MX, class... MxArg>
__global__ __launch_bounds__(1024, 1) void gemm_f8_big_kernel(const unsigned char* __restrict__ A, int64_t lda,
                                                              const unsigned char* __restrict__ B, int64_t ldb,
                                                              GemmEpilogue ep, int M, int N, int K, int tiles_n,
                                                              MxArg... mx_arg) {
    extern __shared__ __attribute__((aligned(16))) bf16_t ldsf[];   // 2 x 64 KB (+ 2 x 2 KB MX)
    const MxScales mx = mx_scales(mx_arg...);
    lp_ring<LpTile<256>, LpMathF8<MX>>(ldsf, reinterpret_cast<const bf16_t*>(A), lda / 2,
                                       reinterpret_cast<const bf16_t*>(B), ldb / 2, ep, M, N, K, tiles_n, mx.splitk,
                                       mx.slabs, mx);
}


// |x| maximum of a tensor as the bit pattern of a non-negative float (they order like
// unsigned integers): *amax_bits must be zero before the launch.
// With `bf` the bf16 copy of x (what the backward products read) is written in the same pass.
__global__ __launch_bounds__(256) void amax_kernel(const float* __restrict__ x, int64_t n4,
                                                   unsigned* __restrict__ amax_bits, uint2* __restrict__ bf) {
    float m = 0.0f;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4;
         i += (int64_t)gridDim.x * blockDim.x) {
        const float4 v = reinterpret_cast<const float4*>(x)[i];
        m = fmaxf(fmaxf(m, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
        if (bf) bf[i] = make_uint2(pack_bf16x2(v.x, v.y), pack_bf16x2(v.z, v.w));
    }
    m = wave_max(m);
    __shared__ float wmax[4];              // one atomic per workgroup: they all hit one L2 line
    if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0)
        atomicMax(amax_bits, __float_as_uint(fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]))));
}
// dst = e4m3(src * 448 / amax) (round to nearest even, saturating), *inv_scale = amax / 448: the
// factor that takes products of the quantised values back.  amax = 0 quantises with scale 1.
constexpr float F8_MAX = 448.0f;
__global__ __launch_bounds__(256) void cast_fp8_kernel(const float* __restrict__ src, int64_t n4,
                                                       const unsigned* __restrict__ amax_bits,
                                                       unsigned* __restrict__ dst, float* __restrict__ inv_scale) {
    const float amax = __uint_as_float(*amax_bits);
    const float scale = amax > 0.0f ? F8_MAX / amax : 1.0f;
    if (blockIdx.x == 0 && threadIdx.x == 0) *inv_scale = amax > 0.0f ? amax / F8_MAX : 1.0f;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4;
         i += (int64_t)gridDim.x * blockDim.x) {
        const float4 v = reinterpret_cast<const float4*>(src)[i];
        int p = __builtin_amdgcn_cvt_pk_fp8_f32(v.x * scale, v.y * scale, 0, false);
        p = __builtin_amdgcn_cvt_pk_fp8_f32(v.z * scale, v.w * scale, p, true);
        dst[i] = (unsigned)p;
    }
}

// ---- MX-e4m3 quantiser (format: include/qarig.h) ----------------------------------------------
// e8m0 exponent of a 32-element block with maximum |x| = amax: the smallest e with amax <= 448 2^e,
// clamped to [-127, 127]; 0 for an all-zero block.  amax = 1.m 2^p: e = p - 8, plus one when
// 1.m > 1.75 (448 = 1.75 2^8).  Subnormal maxima give p - 8 < -127 and clamp.
__device__ __forceinline__ int mx_exponent(float amax) {
    const unsigned u = __float_as_uint(amax);
    if (u == 0u) return 0;
    const int e = (int)(u >> 23) - 135 + ((u & 0x7fffffu) > 0x600000u ? 1 : 0);
    return e < -127 ? -127 : (e > 127 ? 127 : e);
}
// 2^-e as an fp32 (normal for every e this format produces from finite input: e <= 121)
__device__ __forceinline__ float mx_inv_scale(int e) { return __uint_as_float((unsigned)(127 - e) << 23); }
// four e4m3 bytes of x * 2^-e, round to nearest even
__device__ __forceinline__ unsigned mx_pack4(float4 v, float s) {
    int p = __builtin_amdgcn_cvt_pk_fp8_f32(v.x * s, v.y * s, 0, false);
    p = __builtin_amdgcn_cvt_pk_fp8_f32(v.z * s, v.w * s, p, true);
    return (unsigned)p;
}

// One pass over a 64-row x 128-column tile of src (R, C) (fp32, or bf16 with BF), each output optional:
//   q  (R, C) bytes + qs (R, C/32): the row form, blocks of 32 columns of one row;
//   qt (C, Rp) bytes + qts (C, Rp/32): the transposed form, blocks of 32 rows of one column
//      (Rp = R rounded up to 128; rows R..Rp-1 are zeros with scale byte 127);
//   part[blockIdx.y][C]: the tile's column sums (fp32; colsum_reduce_kernel adds the tiles up).
// Phase 1: each wave takes 16 rows, a row per 32 lanes per instruction (float4 each), so a row
// block is 8 lanes and its maximum is three xor-shuffles; the fp32 tile goes to LDS.  Phase 2:
// thread (column, 32-row half) quantises one transposed block from LDS into a byte image, which
// phase 3 stores as 64-byte column segments.
constexpr int MXQ_R = 64, MXQ_C = 128;
template <bool BF>
__global__ __launch_bounds__(256) void mx_quant_kernel(const void* __restrict__ src_, int64_t ld, int R, int C,
                                                       unsigned char* __restrict__ q, unsigned char* __restrict__ qs,
                                                       unsigned char* __restrict__ qt, unsigned char* __restrict__ qts,
                                                       int Rp, float* __restrict__ part) {
    __shared__ float4 tile[MXQ_R][MXQ_C / 4];                 // 32 KB
    __shared__ unsigned tq[MXQ_C][MXQ_R / 4 + 1];             // transposed bytes (+1: odd dword pitch)
    __shared__ float4 red[3][MXQ_C / 4];
    const int r0 = blockIdx.y * MXQ_R, c0 = blockIdx.x * MXQ_C;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int cl = lane & 31;                                  // float4 column within the tile
    const int c = c0 + 4 * cl;
    float4 sum = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 2
    for (int it = 0; it < 8; ++it) {
        const int rl = wave * 16 + it * 2 + (lane >> 5);
        const int r = r0 + rl;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r < R) {
            if constexpr (BF) {
                const uint2 b = *reinterpret_cast<const uint2*>(reinterpret_cast<const bf16_t*>(src_) + (int64_t)r * ld + c);
                v = make_float4(bf16_bits_to_f32(b.x & 0xffffu), bf16_bits_to_f32(b.x >> 16),
                                bf16_bits_to_f32(b.y & 0xffffu), bf16_bits_to_f32(b.y >> 16));
            } else {
                v = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(src_) + (int64_t)r * ld + c);
            }
        }
        tile[rl][cl] = v;
        sum.x += v.x; sum.y += v.y; sum.z += v.z; sum.w += v.w;
        if (q && r < R) {
            float m = fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w)));
            m = fmaxf(m, __shfl_xor(m, 1, 64));
            m = fmaxf(m, __shfl_xor(m, 2, 64));
            m = fmaxf(m, __shfl_xor(m, 4, 64));
            const int e = mx_exponent(m);
            *reinterpret_cast<unsigned*>(q + (int64_t)r * C + c) = mx_pack4(v, mx_inv_scale(e));
            if ((lane & 7) == 0) qs[(int64_t)r * (C / 32) + c / 32] = (unsigned char)(e + 127);
        }
    }
    if (part) {
        sum.x += __shfl_xor(sum.x, 32, 64); sum.y += __shfl_xor(sum.y, 32, 64);
        sum.z += __shfl_xor(sum.z, 32, 64); sum.w += __shfl_xor(sum.w, 32, 64);
        if (wave > 0 && lane < 32) red[wave - 1][cl] = sum;
    }
    __syncthreads();
    if (part && wave == 0 && lane < 32) {
#pragma unroll
        for (int g = 0; g < 3; ++g) {
            const float4 t = red[g][cl];
            sum.x += t.x; sum.y += t.y; sum.z += t.z; sum.w += t.w;
        }
        *reinterpret_cast<float4*>(part + (int64_t)blockIdx.y * C + c) = sum;
    }
    if (!qt) return;
    {
        const int col = threadIdx.x & (MXQ_C - 1), half = threadIdx.x >> 7;
        const float* tf = reinterpret_cast<const float*>(tile);
        float m = 0.0f;
#pragma unroll
        for (int i = 0; i < 32; ++i) m = fmaxf(m, fabsf(tf[(half * 32 + i) * MXQ_C + col]));
        const int e = mx_exponent(m);
        const float s = mx_inv_scale(e);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int rr = half * 32 + 4 * i;
            const float4 v = make_float4(tf[rr * MXQ_C + col], tf[(rr + 1) * MXQ_C + col],
                                         tf[(rr + 2) * MXQ_C + col], tf[(rr + 3) * MXQ_C + col]);
            tq[col][half * 8 + i] = mx_pack4(v, s);
        }
        qts[(int64_t)(c0 + col) * (Rp / 32) + r0 / 32 + half] = (unsigned char)(e + 127);
    }
    __syncthreads();
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int chunk = h * 256 + threadIdx.x;            // 16-B chunk: column chunk / 4, part chunk % 4
        const int col = chunk >> 2, pc = chunk & 3;
        const uint4 v = make_uint4(tq[col][pc * 4], tq[col][pc * 4 + 1], tq[col][pc * 4 + 2], tq[col][pc * 4 + 3]);
        *reinterpret_cast<uint4*>(qt + (int64_t)(c0 + col) * Rp + r0 + pc * 16) = v;
    }
}

// dst[i] = bf16(src[i]), round to nearest even; n % 8 == 0, 16-B aligned.
__global__ void cast_bf16_kernel(const float* __restrict__ src, bf16_t* __restrict__ dst, int64_t n8) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8;
         i += (int64_t)gridDim.x * blockDim.x) {
        const float4 a = reinterpret_cast<const float4*>(src)[2 * i];
        const float4 b = reinterpret_cast<const float4*>(src)[2 * i + 1];
        reinterpret_cast<uint4*>(dst)[i] = make_uint4(pack_bf16x2(a.x, a.y), pack_bf16x2(a.z, a.w),
                                                      pack_bf16x2(b.x, b.y), pack_bf16x2(b.z, b.w));
    }
}
__global__ void cast_bf16_tail_kernel(const float* __restrict__ src, bf16_t* __restrict__ dst,
                                      int64_t begin, int64_t n) {
    const int64_t i = begin + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = (bf16_t)(pack_bf16x2(src[i], 0.0f) & 0xffffu);
}

// Cast with the column sums riding along: dst = bf16(src) for src (M, N) fp32 and
// part[blockIdx.y][n] = sum of the block's CS_ROWS rows of column n (fixed order).  The bias
// gradient of a Linear layer is the column sum of the same dT that the weight-gradient GEMM
// needs in bf16, so one pass over dT yields both.
constexpr int CS_ROWS = 64;     // rows per block: 4 row groups of 16, combined in group order
__global__ __launch_bounds__(512) void cast_colsum_kernel(const float* __restrict__ src, int64_t ld,
                                                          int M, int N, bf16_t* __restrict__ dst,
                                                          float* __restrict__ part) {
    __shared__ float4 red[3][128];
    const int ct = threadIdx.x & 127, rg = threadIdx.x >> 7;
    const int c = (blockIdx.x * 128 + ct) * 4;
    const bool in = c < N;
    const int r0 = blockIdx.y * CS_ROWS + rg * 16, r1 = min(M, r0 + 16);
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    if (in)
        for (int r = r0; r < r1; ++r) {
            const float4 v = *reinterpret_cast<const float4*>(src + (int64_t)r * ld + c);
            if (dst)
                *reinterpret_cast<uint2*>(dst + (int64_t)r * N + c) =
                    make_uint2(pack_bf16x2(v.x, v.y), pack_bf16x2(v.z, v.w));
            s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
        }
    if (rg > 0) red[rg - 1][ct] = s;
    __syncthreads();
    if (rg == 0 && in) {
#pragma unroll
        for (int g = 0; g < 3; ++g) {
            const float4 t = red[g][ct];
            s.x += t.x; s.y += t.y; s.z += t.z; s.w += t.w;
        }
        *reinterpret_cast<float4*>(part + (int64_t)blockIdx.y * N + c) = s;
    }
}
// the same sums from a bf16 tensor (dT1 of an MLP exists only in bf16 in this mode)
__global__ __launch_bounds__(512) void colsum_bf16_kernel(const bf16_t* __restrict__ src, int64_t ld,
                                                          int M, int N, float* __restrict__ part) {
    __shared__ float4 red[3][128];
    const int ct = threadIdx.x & 127, rg = threadIdx.x >> 7;
    const int c = (blockIdx.x * 128 + ct) * 4;
    const bool in = c < N;
    const int r0 = blockIdx.y * CS_ROWS + rg * 16, r1 = min(M, r0 + 16);
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    if (in)
        for (int r = r0; r < r1; ++r) {
            const uint2 v = *reinterpret_cast<const uint2*>(src + (int64_t)r * ld + c);
            s.x += bf16_bits_to_f32(v.x & 0xffffu); s.y += bf16_bits_to_f32(v.x >> 16);
            s.z += bf16_bits_to_f32(v.y & 0xffffu); s.w += bf16_bits_to_f32(v.y >> 16);
        }
    if (rg > 0) red[rg - 1][ct] = s;
    __syncthreads();
    if (rg == 0 && in) {
#pragma unroll
        for (int g = 0; g < 3; ++g) {
            const float4 t = red[g][ct];
            s.x += t.x; s.y += t.y; s.z += t.z; s.w += t.w;
        }
        *reinterpret_cast<float4*>(part + (int64_t)blockIdx.y * N + c) = s;
    }
}
// out[n] (+)= sum over the `chunks` partial rows, in a fixed order: 4 interleaved chunk groups per
// column summed in parallel, then combined in group order (a serial walk over 128+ chunks is
// latency-bound: 15 us per bias gradient)
__global__ __launch_bounds__(256) void colsum_reduce_kernel(const float* __restrict__ part, int chunks,
                                                            int N, float* __restrict__ out, int accumulate) {
    __shared__ float red[3][64];
    const int ct = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + ct;
    float s = 0.0f;
    if (c < N)
        for (int z0 = g; z0 < chunks; z0 += 32) {      // 8 loads in flight, added in chunk order
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int z = z0 + 4 * u;
                v[u] = z < chunks ? part[(int64_t)z * N + c] : 0.0f;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) s += v[u];
        }
    if (g > 0) red[g - 1][ct] = s;
    __syncthreads();
    if (g == 0 && c < N) {
        s = ((s + red[0][ct]) + red[1][ct]) + red[2][ct];
        out[c] = accumulate ? out[c] + s : s;
    }
}

// dst[c][r] = bf16(src[r][c]) for src (R, C) row-major with leading dimension lds_: the W^T
// shadow of a Linear weight.  64 x 64 tiles through LDS, coalesced on both sides.
__global__ __launch_bounds__(256) void cast_transpose_bf16_kernel(const float* __restrict__ src,
                                                                  int64_t ld, int R, int C,
                                                                  bf16_t* __restrict__ dst) {
    __shared__ float t[64][65];
    const int r0 = blockIdx.y * 64, c0 = blockIdx.x * 64;
    for (int idx = threadIdx.x; idx < 64 * 64; idx += 256) {
        const int r = idx >> 6, c = idx & 63;
        t[r][c] = (r0 + r < R && c0 + c < C) ? src[(int64_t)(r0 + r) * ld + c0 + c] : 0.0f;
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < 64 * 32; idx += 256) {
        const int c = idx >> 5, r = (idx & 31) * 2;
        if (c0 + c < C && r0 + r < R) {
            const uint32_t v = pack_bf16x2(t[r][c], t[r + 1][c]);
            if (r0 + r + 1 < R && ((R & 1) == 0))
                *reinterpret_cast<uint32_t*>(dst + (int64_t)(c0 + c) * R + r0 + r) = v;
            else {
                dst[(int64_t)(c0 + c) * R + r0 + r] = (bf16_t)(v & 0xffffu);
                if (r0 + r + 1 < R) dst[(int64_t)(c0 + c) * R + r0 + r + 1] = (bf16_t)(v >> 16);
            }
        }
    }
}
}  // namespace qarig

using namespace qarig;

extern "C" int qarig_slab_reduce_f32(const float* slabs, float* out, int64_t ldc, int M, int N,
                                     int nslab, int accumulate, void* stream);

// fp32 -> bf16 (round to nearest even) of n contiguous elements; dst holds n 16-bit values.
// New entry (no reference counterpart): the operand conversion of the reduced-precision mode.
extern "C" int qarig_cast_bf16(const float* src, void* dst, int64_t n, void* stream) {
    QARIG_CHECK_ARG(src && dst && n > 0 && n <= (1LL << 40), "cast_bf16: bad arguments");
    QARIG_CHECK_ARG((((uintptr_t)src | (uintptr_t)dst) & 15) == 0, "cast_bf16: 16-B aligned buffers");
    const int64_t n8 = n / 8;
    if (n8 > 0) {
        int blocks = (int)((n8 + 255) / 256);
        if (blocks > 4096) blocks = 4096;
        hipLaunchKernelGGL(cast_bf16_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, src,
                           (bf16_t*)dst, n8);
    }
    if (n8 * 8 < n)
        hipLaunchKernelGGL(cast_bf16_tail_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, src,
                           (bf16_t*)dst, n8 * 8, n);
    QARIG_CHECK_LAUNCH("cast_bf16");
    return QARIG_OK;
}

// dst (C, R) bf16 = transpose of src (R, C) fp32 (row stride ld).
extern "C" int qarig_cast_transpose_bf16(const float* src, int64_t ld, int R, int C, void* dst,
                                         void* stream) {
    QARIG_CHECK_ARG(src && dst && R > 0 && C > 0 && ld >= C, "cast_transpose_bf16: bad arguments");
    QARIG_CHECK_DIMS("cast_transpose_bf16", R, C);
    QARIG_CHECK_ARG(((uintptr_t)dst & 3) == 0, "cast_transpose_bf16: 4-B aligned destination");
    hipLaunchKernelGGL(cast_transpose_bf16_kernel, dim3((C + 63) / 64, (R + 63) / 64), dim3(256), 0,
                       (hipStream_t)stream, src, ld, R, C, (bf16_t*)dst);
    QARIG_CHECK_LAUNCH("cast_transpose_bf16");
    return QARIG_OK;
}

extern "C" size_t qarig_cast_colsum_workspace_bytes(int M, int N) {
    if (M < 1 || N < 1 || M > (1 << 24) || N > (1 << 24)) return 0;
    return (size_t)((M + CS_ROWS - 1) / CS_ROWS) * N * sizeof(float);
}

// colsum[n] (+)= sum_m src[m][n], and (dst != NULL) dst = bf16(src); src fp32 (src_is_bf16 = 0) or
// bf16 (1; dst must be NULL).  N % 4 == 0, rows 16-B (8-B for bf16) aligned.  The bias gradient
// of nn.Linear (models/layers.py:243-250) in the reduced-precision mode.
extern "C" int qarig_cast_colsum(const void* src, int64_t ld, int src_is_bf16, int M, int N, void* dst,
                                 float* colsum, int accumulate, void* workspace, size_t ws_bytes,
                                 void* stream) {
    QARIG_CHECK_ARG(src && colsum && M > 0 && N > 0 && N % 4 == 0 && ld >= N && ld % 4 == 0,
                    "cast_colsum: bad arguments");
    QARIG_CHECK_DIMS("cast_colsum", M, N);
    QARIG_CHECK_ARG(!(src_is_bf16 && dst), "cast_colsum: a bf16 source is not re-cast");
    QARIG_CHECK_ARG(((uintptr_t)src & (src_is_bf16 ? 7 : 15)) == 0 && (!dst || ((uintptr_t)dst & 7) == 0),
                    "cast_colsum: misaligned buffers");
    if (!workspace || ws_bytes < qarig_cast_colsum_workspace_bytes(M, N)) {
        qarig_set_error("cast_colsum: workspace too small");
        return QARIG_ERR_WORKSPACE;
    }
    const int chunks = (M + CS_ROWS - 1) / CS_ROWS;
    dim3 grid((N / 4 + 127) / 128, chunks), block(512);
    hipStream_t st = (hipStream_t)stream;
    if (src_is_bf16)
        hipLaunchKernelGGL(colsum_bf16_kernel, grid, block, 0, st, (const bf16_t*)src, ld, M, N, (float*)workspace);
    else
        hipLaunchKernelGGL(cast_colsum_kernel, grid, block, 0, st, (const float*)src, ld, M, N, (bf16_t*)dst,
                           (float*)workspace);
    QARIG_CHECK_LAUNCH("cast_colsum");
    hipLaunchKernelGGL(colsum_reduce_kernel, dim3((N + 63) / 64), dim3(256), 0, st, (const float*)workspace,
                       chunks, N, colsum, accumulate);
    QARIG_CHECK_LAUNCH("cast_colsum reduce");
    return QARIG_OK;
}

extern "C" size_t qarig_gemm_lp_workspace_bytes(int M, int N, int splitk) {
    if (M < 1 || N < 1 || splitk > (1 << 16)) return 0;
    return splitk > 1 ? (size_t)splitk * M * N * sizeof(float) : 0;
}

// 1 when the shape can run on the reduced-precision kernel (else the caller uses qarig_gemm_f32).
extern "C" int qarig_gemm_lp_supported(int M, int N, int K, int splitk) {
    if (splitk < 1) splitk = 1;
    if (!qarig_dims_ok({M, N}) || !qarig_dims_ok({M, K}) || !qarig_dims_ok({N, K}) || splitk > 4096) return 0;
    return M > 0 && N > 0 && K > 0 && M % BM == 0 && N % BN == 0 && K % splitk == 0 &&
           (K / splitk) % LBK == 0;
}

// ---- what qarig_gemm_lp, qarig_gemm_f8 and qarig_gemm_mx share --------------------------------
// Alignment of the operands (ld_mult: 8 elements for bf16, 16 bytes for e4m3), of the fp32 epilogue
// tensors and of the bf16 outputs, and the epilogues that accumulate and split-K allow.  `name`
// is the entry point's, for the error text; ld_min (0: none) and scales_ok are qarig_gemm_mx's own checks, which
// sit between the shared ones.
static int lp_check_args(const char* name, const void* A, int64_t lda, const void* B, int64_t ldb, int ld_mult,
                         int64_t ld_min, bool scales_ok, const float* C, int64_t ldc, const float* bias, const float* residual,
                         int64_t ldr, const float* preact, int64_t ldp, int act, const void* gradz, int64_t ldz,
                         int gradz_is_bf16, int splitk, int accumulate, const void* Cb, int64_t ldcb,
                         const void* Pb, int64_t ldpb) {
    auto al16 = [](const void* p) { return ((uintptr_t)p & 15) == 0; };
    QARIG_CHECK_ARG(al16(A) && al16(B) && lda % ld_mult == 0 && ldb % ld_mult == 0 &&
                        (ld_min == 0 || (lda >= ld_min && ldb >= ld_min)),
                    "%s: operands 16-B aligned, ld %% %d", name, ld_mult);
    QARIG_CHECK_ARG(scales_ok, "%s: scales 4-B aligned, ld %% 4", name);
    auto ok4 = [&](const void* p, int64_t ld) { return !p || (al16(p) && ld % 4 == 0); };
    auto ok4b = [](const void* p, int64_t ld) { return !p || (((uintptr_t)p & 7) == 0 && ld % 4 == 0); };
    QARIG_CHECK_ARG(ok4(C, ldc) && ok4(bias, 4) && ok4(residual, ldr) && ok4(preact, ldp) &&
                        (gradz_is_bf16 ? ok4b(gradz, ldz) : ok4(gradz, ldz)),
                    "%s: fp32 epilogue tensors 16-B aligned, ld %% 4", name);
    QARIG_CHECK_ARG(ok4b(Cb, ldcb) && ok4b(Pb, ldpb), "%s: bf16 outputs 8-B aligned, ld %% 4", name);
    const bool plain = C && !bias && !residual && !preact && !gradz && act == ACT_NONE && !Cb && !Pb;
    QARIG_CHECK_ARG(!accumulate || plain, "%s: accumulate supports the plain epilogue only", name);
    QARIG_CHECK_ARG(splitk <= 1 || plain, "%s: split-K supports the plain epilogue only", name);
    return QARIG_OK;
}

// 256 x 256 tiles where they still give every CU a workgroup; option lp_big = 0 / 1 overrides
static bool use_big_tile(int M, int N, int splitk) {
    const int big_env = g_qarig_opt.lp_big;
    const long big_tiles = (long)(M / LPB) * (N / LPB) * splitk;
    return M % LPB == 0 && N % LPB == 0 && big_env != 0 && (big_env == 1 || big_tiles >= 224);
}

// The kernels by family (bf16 32x32x16, bf16 16x16x32, e4m3 per tensor, MX-e4m3), tile (128, 256)
// and layout (NT, TN, NN; e4m3 is NT only).  The three families' argument lists differ, so an entry
// point casts its pointer back to the type it launches with.
enum { LP_F32 = 0, LP_F16 = 1, LP_F8 = 2, LP_FMX = 3 };
using LpKernel = void (*)(const bf16_t*, int64_t, const bf16_t*, int64_t, GemmEpilogue, int, int, int, int, int, float*);
using F8Kernel = void (*)(const unsigned char*, int64_t, const unsigned char*, int64_t, GemmEpilogue, int, int, int, int);
using MxKernel = void (*)(const unsigned char*, int64_t, const unsigned char*, int64_t, GemmEpilogue, int, int, int, int,
                          MxScales);
#define LP_LAYOUTS(k) {(const void*)k<false, false>, (const void*)k<true, true>, (const void*)k<false, true>}
static const void* const lp_kernels[4][2][3] = {
    {LP_LAYOUTS(gemm_lp_kernel), LP_LAYOUTS(gemm_lp_big_kernel)},
    {LP_LAYOUTS(gemm_lp16_kernel), LP_LAYOUTS(gemm_lp_big16_kernel)},
    {{(const void*)gemm_f8_kernel<false>}, {(const void*)gemm_f8_big_kernel<false>}},
    {{(const void*)gemm_f8_kernel<true, MxScales>}, {(const void*)gemm_f8_big_kernel<true, MxScales>}},
};
#undef LP_LAYOUTS

// Which kernel runs an (M, N) product and on what grid.  The 256-tile's ring (and MX scale images)
// is dynamic LDS past the default limit: each of its kernels is allowed it the first time it is chosen.
struct LpLaunch {
    const void* kernel;
    const char* what;   // for the launch error text
    dim3 grid, block;
    int lds, tiles_n;
};
static LpLaunch lp_launch(int family, int layout, int M, int N, int splitk) {
    const bool big = use_big_tile(M, N, splitk);
    const int rows = big ? LPB : 128;
    static const char* const names[4][2] = {{"gemm_lp", "gemm_lp big"}, {"gemm_lp", "gemm_lp big16"},
                                            {"gemm_f8", "gemm_f8 big"}, {"gemm_mx", "gemm_mx big"}};
    LpLaunch l{lp_kernels[family][big][layout], names[family][big], dim3((M / rows) * (N / rows), 1, splitk), dim3(big ? 1024 : NTHREADS),
               0, N / rows};
    if (big) {
        l.lds = 2 * LpTile<LPB>::STAGE * (int)sizeof(bf16_t) + (family == LP_FMX ? 2 * 2 * LPB * 4 : 0);
        static bool allowed[4][3];
        if (!allowed[family][layout]) {
            (void)hipFuncSetAttribute(l.kernel, hipFuncAttributeMaxDynamicSharedMemorySize, l.lds);
            allowed[family][layout] = true;
        }
    }
    return l;
}

// After the launch: split-K's slabs are summed into C.
static int lp_finish(const void* workspace, float* C, int64_t ldc, int M, int N, int splitk, int accumulate,
                     void* stream) {
    if (splitk > 1)
        return qarig_slab_reduce_f32((const float*)workspace, C, ldc, M, N, splitk, accumulate, stream);
    return QARIG_OK;
}

// C (fp32, optional) / Cb (bf16, optional) = epilogue(A B^T) with bf16 operands.
// layout 0 = NT (A (M,K), B (N,K)), 1 = TN (A (K,M), B (K,N)); lda/ldb in elements.
// Epilogue arguments as qarig_gemm_f32 (bias, residual, preact, act, gradz/gact, splitk,
// accumulate); Cb / Pb: optional bf16 copies of the output / of the saved pre-activation.
extern "C" int qarig_gemm_lp(const void* A, int64_t lda, const void* B, int64_t ldb, int layout,
                             float* C, int64_t ldc, int M, int N, int K, const float* bias,
                             const float* residual, int64_t ldr, float* preact, int64_t ldp, int act,
                             const void* gradz, int64_t ldz, int gradz_is_bf16, int gact, int splitk,
                             int accumulate, void* Cb, int64_t ldcb, void* Pb, int64_t ldpb,
                             void* workspace, size_t ws_bytes, void* stream) {
    QARIG_CHECK_ARG(A && B && (C || Cb), "gemm_lp: null operand");
    QARIG_CHECK_ARG(layout >= 0 && layout <= 2, "gemm_lp: layout must be 0 (NT), 1 (TN) or 2 (NN)");
    QARIG_CHECK_ARG(act >= 0 && act <= 3 && gact >= 0 && gact <= 3, "gemm_lp: bad activation id");
    if (splitk < 1) splitk = 1;
    QARIG_CHECK_ARG(qarig_gemm_lp_supported(M, N, K, splitk),
                    "gemm_lp: needs M,N %% 128 == 0 and K/splitk %% 64 == 0 (M=%d N=%d K=%d splitk=%d)",
                    M, N, K, splitk);
    if (const int rc = lp_check_args("gemm_lp", A, lda, B, ldb, 8, 0, true, C, ldc, bias, residual, ldr, preact, ldp, act,
                                     gradz, ldz, gradz_is_bf16, splitk, accumulate, Cb, ldcb, Pb, ldpb))
        return rc;
    if (accumulate && splitk == 1) { residual = C; ldr = ldc; }
    if (splitk > 1 && (!workspace || ws_bytes < qarig_gemm_lp_workspace_bytes(M, N, splitk))) {
        qarig_set_error("gemm_lp: workspace too small");
        return QARIG_ERR_WORKSPACE;
    }
    GemmEpilogue ep{C, ldc, bias, residual, ldr, preact, ldp, act,
                    gradz_is_bf16 ? nullptr : (const float*)gradz, ldz, gact, nullptr,
                    (unsigned short*)Cb, ldcb, (unsigned short*)Pb, ldpb,
                    gradz_is_bf16 ? (const unsigned short*)gradz : nullptr, ldz};
    const LpLaunch l = lp_launch(g_qarig_opt.lp_mfma16 ? LP_F16 : LP_F32, layout, M, N, splitk);
    hipLaunchKernelGGL(((LpKernel)l.kernel), l.grid, l.block, l.lds, (hipStream_t)stream, (const bf16_t*)A, lda,
                       (const bf16_t*)B, ldb, ep, M, N, K, l.tiles_n, splitk, (float*)workspace);
    QARIG_CHECK_LAUNCH(l.what);
    return lp_finish(workspace, C, ldc, M, N, splitk, accumulate, stream);
}

// ---- fp8 (e4m3) operands: see gemm_f8_kernel ------------------------------------------------
extern "C" int qarig_gemm_f8_supported(int M, int N, int K) {
    return M > 0 && N > 0 && K > 0 && M % BM == 0 && N % BN == 0 && K % 128 == 0;
}

// dst (n bytes, e4m3) = quantised src (n floats) with one scale for the tensor; scratch[0] receives
// the |x| maximum (as float bits; zeroed here), inv_scale[0] the dequantisation factor; bf16_dst
// (optional, n elements) the bf16 copy of src, written by the pass that finds the maximum.
extern "C" int qarig_cast_fp8(const float* src, int64_t n, void* dst, float* inv_scale, void* scratch,
                              void* bf16_dst, void* stream) {
    QARIG_CHECK_ARG(src && dst && inv_scale && scratch, "cast_fp8: null pointer");
    QARIG_CHECK_ARG(((uintptr_t)bf16_dst & 7) == 0, "cast_fp8: bf16 copy 8-B aligned");
    QARIG_CHECK_ARG(n > 0 && n % 4 == 0 && n < (1LL << 40), "cast_fp8: n must be a positive multiple of 4");
    QARIG_CHECK_ARG((((uintptr_t)src & 15) | ((uintptr_t)dst & 3) | ((uintptr_t)scratch & 3)) == 0,
                    "cast_fp8: src 16-B aligned, dst 4-B aligned");
    hipStream_t st = (hipStream_t)stream;
    const int64_t n4 = n / 4;
    int blocks = (int)((n4 + 255) / 256 < 1024 ? (n4 + 255) / 256 : 1024);
    if (hipMemsetAsync(scratch, 0, 4, st) != hipSuccess) {
        qarig_set_error("cast_fp8: memset failed");
        return QARIG_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(amax_kernel, dim3(blocks), dim3(256), 0, st, src, n4, (unsigned*)scratch,
                       (uint2*)bf16_dst);
    QARIG_CHECK_LAUNCH("cast_fp8 amax");
    hipLaunchKernelGGL(cast_fp8_kernel, dim3(blocks), dim3(256), 0, st, src, n4, (const unsigned*)scratch,
                       (unsigned*)dst, inv_scale);
    QARIG_CHECK_LAUNCH("cast_fp8");
    return QARIG_OK;
}

// C[M,N] = epilogue(inv_a * inv_b * sum_k A8[m][k] B8[n][k]): A8 (M,K), B8 (N,K) e4m3 bytes,
// inv_a / inv_b the device scalars qarig_cast_fp8 wrote.  Epilogue options as qarig_gemm_lp
// (no backward fusion, no split-K, no accumulate).
extern "C" int qarig_gemm_f8(const void* A, int64_t lda, const void* B, int64_t ldb, const float* inv_a,
                             const float* inv_b, float* C, int64_t ldc, int M, int N, int K,
                             const float* bias, const float* residual, int64_t ldr, float* preact,
                             int64_t ldp, int act, void* Cb, int64_t ldcb, void* Pb, int64_t ldpb,
                             void* stream) {
    QARIG_CHECK_ARG(A && B && inv_a && inv_b && (C || Cb), "gemm_f8: null operand");
    QARIG_CHECK_ARG(act >= 0 && act <= 3, "gemm_f8: bad activation id");
    QARIG_CHECK_ARG(qarig_gemm_f8_supported(M, N, K),
                    "gemm_f8: needs M,N %% 128 == 0 and K %% 128 == 0 (M=%d N=%d K=%d)", M, N, K);
    if (const int rc = lp_check_args("gemm_f8", A, lda, B, ldb, 16, 0, true, C, ldc, bias, residual, ldr, preact, ldp, act,
                                     nullptr, 0, 0, 1, 0, Cb, ldcb, Pb, ldpb))
        return rc;
    GemmEpilogue ep{C, ldc, bias, residual, ldr, preact, ldp, act, nullptr, 0, 0, nullptr,
                    (unsigned short*)Cb, ldcb, (unsigned short*)Pb, ldpb, nullptr, 0, inv_a, inv_b};
    const LpLaunch l = lp_launch(LP_F8, 0, M, N, 1);
    hipLaunchKernelGGL(((F8Kernel)l.kernel), l.grid, l.block, l.lds, (hipStream_t)stream, (const unsigned char*)A, lda,
                       (const unsigned char*)B, ldb, ep, M, N, K, l.tiles_n);
    QARIG_CHECK_LAUNCH(l.what);
    return QARIG_OK;
}

// ---- MX-e4m3 operands (include/qarig.h): quantiser and block-scaled GEMM ----------------------
extern "C" size_t qarig_mx_quant_workspace_bytes(int R, int C) {
    if (R < 1 || C < 1 || R > (1 << 24) || C > (1 << 24)) return 0;
    return (size_t)((R + 127) / 128 * 2) * C * sizeof(float);
}

// One pass over src (R, C) (fp32, or bf16 when src_is_bf16; row stride ld elements), writing any of:
// the row form q (R, C) + q_scale (R, C/32); the transposed form qt (C, Rp) + qt_scale (C, Rp/32),
// Rp = R rounded up to 128, zero padded; colsum[c] (+)= sum_r src[r][c] (fp32, fixed order).
// C % 128 == 0.  Replaces the operand casts of the reduced-precision Linear products
// (models/layers.py:234-254, 330-340, 389-418) and, for colsum, the bias gradient of
// models/layers.py:243-250 (as qarig_cast_colsum does for bf16).
extern "C" int qarig_mx_quant(const void* src, int64_t ld, int src_is_bf16, int R, int C, void* q, void* q_scale,
                              void* qt, void* qt_scale, float* colsum, int accumulate, void* workspace,
                              size_t ws_bytes, void* stream) {
    QARIG_CHECK_ARG(src && R > 0 && C > 0 && C % MXQ_C == 0 && ld >= C, "mx_quant: bad arguments (C %% 128 == 0)");
    QARIG_CHECK_DIMS("mx_quant", R, C);
    QARIG_CHECK_ARG((q != nullptr) == (q_scale != nullptr) && (qt != nullptr) == (qt_scale != nullptr) &&
                        (q || qt || colsum), "mx_quant: each form needs its bytes and its scales");
    QARIG_CHECK_ARG(((uintptr_t)src & (src_is_bf16 ? 7 : 15)) == 0 && ld % 4 == 0 && ((uintptr_t)q & 3) == 0 &&
                        ((uintptr_t)qt & 15) == 0, "mx_quant: misaligned buffers");
    const int Rp = (R + 127) / 128 * 128;
    const int chunks = Rp / MXQ_R;
    if (colsum && (!workspace || ws_bytes < qarig_mx_quant_workspace_bytes(R, C))) {
        qarig_set_error("mx_quant: workspace too small");
        return QARIG_ERR_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    float* part = colsum ? (float*)workspace : nullptr;
    dim3 grid(C / MXQ_C, chunks), block(256);
    if (src_is_bf16)
        hipLaunchKernelGGL(mx_quant_kernel<true>, grid, block, 0, st, src, ld, R, C, (unsigned char*)q,
                           (unsigned char*)q_scale, (unsigned char*)qt, (unsigned char*)qt_scale, Rp, part);
    else
        hipLaunchKernelGGL(mx_quant_kernel<false>, grid, block, 0, st, src, ld, R, C, (unsigned char*)q,
                           (unsigned char*)q_scale, (unsigned char*)qt, (unsigned char*)qt_scale, Rp, part);
    QARIG_CHECK_LAUNCH("mx_quant");
    if (colsum) {
        hipLaunchKernelGGL(colsum_reduce_kernel, dim3((C + 63) / 64), dim3(256), 0, st, (const float*)part, chunks,
                           C, colsum, accumulate);
        QARIG_CHECK_LAUNCH("mx_quant colsum");
    }
    return QARIG_OK;
}

// 1 when C = A B^T on MX operands can run: M, N % 128 == 0, K % splitk == 0, (K / splitk) % 128 == 0.
extern "C" int qarig_gemm_mx_supported(int M, int N, int K, int splitk) {
    if (splitk < 1) splitk = 1;
    if (!qarig_dims_ok({M, N}) || !qarig_dims_ok({M, K}) || !qarig_dims_ok({N, K}) || splitk > 4096) return 0;
    return M > 0 && N > 0 && K > 0 && M % BM == 0 && N % BN == 0 && K % splitk == 0 && (K / splitk) % 128 == 0;
}

extern "C" size_t qarig_gemm_mx_workspace_bytes(int M, int N, int splitk) {
    return qarig_gemm_lp_workspace_bytes(M, N, splitk);
}

// C / Cb = epilogue(sum_k A[m][k] B[n][k]) with A (M, K) and B (N, K) in MX-e4m3 row form (bytes,
// lda / ldb in bytes) and their scales sA (M, K/32), sB (N, K/32) (row strides ldsa / ldsb in bytes).
// Epilogue arguments, split-K and accumulate as qarig_gemm_lp.  Replaces the Linear contractions of
// models/layers.py:234-254, 330-340, 389-418 (forward, input and weight gradients) in "mxfp8" mode.
extern "C" int qarig_gemm_mx(const void* A, int64_t lda, const void* sA, int64_t ldsa, const void* B, int64_t ldb,
                             const void* sB, int64_t ldsb, float* C, int64_t ldc, int M, int N, int K,
                             const float* bias, const float* residual, int64_t ldr, float* preact, int64_t ldp,
                             int act, const void* gradz, int64_t ldz, int gradz_is_bf16, int gact, int splitk,
                             int accumulate, void* Cb, int64_t ldcb, void* Pb, int64_t ldpb, void* workspace,
                             size_t ws_bytes, void* stream) {
    QARIG_CHECK_ARG(A && B && sA && sB && (C || Cb), "gemm_mx: null operand");
    QARIG_CHECK_ARG(act >= 0 && act <= 3 && gact >= 0 && gact <= 3, "gemm_mx: bad activation id");
    if (splitk < 1) splitk = 1;
    QARIG_CHECK_ARG(qarig_gemm_mx_supported(M, N, K, splitk),
                    "gemm_mx: needs M,N %% 128 == 0 and K/splitk %% 128 == 0 (M=%d N=%d K=%d splitk=%d)", M, N,
                    K, splitk);
    const bool scales_ok = ((uintptr_t)sA & 3) == 0 && ((uintptr_t)sB & 3) == 0 && ldsa % 4 == 0 && ldsb % 4 == 0 &&
                           ldsa >= K / 32 && ldsb >= K / 32;
    if (const int rc = lp_check_args("gemm_mx", A, lda, B, ldb, 16, K, scales_ok, C, ldc, bias, residual, ldr, preact, ldp, act,
                                     gradz, ldz, gradz_is_bf16, splitk, accumulate, Cb, ldcb, Pb, ldpb))
        return rc;
    if (accumulate && splitk == 1) { residual = C; ldr = ldc; }
    if (splitk > 1 && (!workspace || ws_bytes < qarig_gemm_mx_workspace_bytes(M, N, splitk))) {
        qarig_set_error("gemm_mx: workspace too small");
        return QARIG_ERR_WORKSPACE;
    }
    GemmEpilogue ep{C, ldc, bias, residual, ldr, preact, ldp, act,
                    gradz_is_bf16 ? nullptr : (const float*)gradz, ldz, gact, nullptr,
                    (unsigned short*)Cb, ldcb, (unsigned short*)Pb, ldpb,
                    gradz_is_bf16 ? (const unsigned short*)gradz : nullptr, ldz, nullptr, nullptr};
    MxScales mx{(const unsigned char*)sA, ldsa, (const unsigned char*)sB, ldsb, splitk, (float*)workspace};
    const LpLaunch l = lp_launch(LP_FMX, 0, M, N, splitk);
    hipLaunchKernelGGL(((MxKernel)l.kernel), l.grid, l.block, l.lds, (hipStream_t)stream, (const unsigned char*)A, lda,
                       (const unsigned char*)B, ldb, ep, M, N, K, l.tiles_n, mx);
    QARIG_CHECK_LAUNCH(l.what);
    return lp_finish(workspace, C, ldc, M, N, splitk, accumulate, stream);
}
