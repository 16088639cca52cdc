/* qarig.h -- C ABI of libqarig_hip.so: the MI355X (gfx950) hot path of the
 * quantized-autoregressive image pipeline (conv autoencoder -> SOM/BMU codebook ->
 * cascaded Transformer).
 *
 * The reference (Vinmwaura/Quantized-Autoregression-Image-Generator) has no FFI: its
 * boundary for this path is the Python class surface of models/ (SURVEY.md 8b).
 * Each entry point below replaces the body of one reference method / ATen call
 * site, cited as `reference file:line`.  The Python mirror of that class surface
 * (quantized-autoregression-image-generator_amd/models/) binds these with ctypes;
 * INTEGRATION.md shows the stub a reference maintainer would add.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer (HIP), fp32 unless stated, contiguous in the
 *    stated layout; token / index tensors are int64;
 *  - the library never allocates, frees or synchronises: outputs and workspaces are
 *    caller-owned, `stream` is a hipStream_t passed as void* (NULL = default stream);
 *  - return 0 on success, <0 on error (QARIG_ERR_*); qarig_last_error() gives the
 *    message of the calling thread's last failure.  Nothing throws across the ABI.
 */
#ifndef QARIG_H
#define QARIG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QARIG_OK 0
#define QARIG_ERR_ARG -1
#define QARIG_ERR_LAUNCH -2
#define QARIG_ERR_WORKSPACE -3

/* activation ids -- reference models/layers.py:74-80 get_activation */
#define QARIG_ACT_NONE 0
#define QARIG_ACT_SILU 1
#define QARIG_ACT_TANH 2
#define QARIG_ACT_SIGMOID 3

int qarig_version(void);
const char* qarig_target_arch(void);
int qarig_last_error(char* buf, size_t n);
/* Kernel-selection options: each only chooses between kernels that must give the same results
 * (tests/test_gpu_switches.py runs the parity tests under every one).  Names: gemm_dma (1), gemm_pair
 * (-1 auto), bmu_cs (0 auto), bmu_groups (-1 auto), bmu_coarse (-1 auto), attn_qw / attn_bw (0 auto),
 * lp_big (-1 auto), lp_mfma16 (1), convt_pair (1), conv_ring (1), gemm_xcd_splits (1).  Returns the previous value, INT_MIN
 * for an unknown name.  No reference counterpart. */
int qarig_set_option(const char* name, int value);

/* ---- Codebook ---------------------------------------------------------------- */

/* Codebook.get_patches_bmu -- models/Codebook.py:77-99 (patchify layers.py:8-34,
 * torch.cdist + torch.argmin).  x: (N,C,H,W); codebook: (K,D), D = C*pH*pW;
 * out_idx: int64 (N * (H/pH) * (W/pW)), patch-grid row-major. */
size_t qarig_bmu_workspace_bytes(int64_t rows, int K);
int qarig_bmu_fwd(const float* x, int N, int C, int H, int W, int pH, int pW,
                  const float* codebook, int K, int D, int64_t* out_idx, void* workspace,
                  size_t ws_bytes, void* stream);

/* qarig_bmu_fwd with the codebook's prepared image (qarig_bmu_prepare below; NULL = none): where the
 * dispatch takes the coarse-pass kernel, its workgroups copy the image into LDS (global -> LDS DMA) instead
 * of each converting the codebook.  For a codebook that does not change between calls (tokenising a
 * dataset, the Transformer training loop); same indices. */
int qarig_bmu_fwd_prepared(const float* x, int N, int C, int H, int W, int pH, int pW,
                           const float* codebook, int K, int D, int64_t* out_idx, void* workspace,
                           size_t ws_bytes, const void* prepared, void* stream);

/* The same search through a coarse pass on the bf16 MFMA (every operand split into three bf16
 * pieces that add up to it exactly, six products on top of |w|^2 per 32 x 32 tile), a per-row certificate
 * (second-smallest - smallest > 3 eps, eps a proven bound of the coarse error) and the literal
 * fp32 re-scan of every row without one: bit-identical indices to qarig_bmu_fwd's exact kernels.
 * qarig_bmu_fwd takes this form by itself where it applies (D <= 16, D % 4 == 0, K % 32 == 0,
 * K <= 1024, >= 24576 rows); this entry forces it and counts the re-scanned rows into
 * uncertified[0] (device unsigned[8], caller-zeroed, may be NULL; [1..3] += clock64() cycles of the
 * staging / scan / finish phases of every block, [4] += blocks: tools/bmu_bench.py).  K <= 1024: one
 * LDS image holds the whole codebook.  models/Codebook.py:77-99. */
int qarig_bmu_fwd_coarse(const float* x, int N, int C, int H, int W, int pH, int pW,
                         const float* codebook, int K, int D, int64_t* out_idx,
                         unsigned* uncertified, const void* prepared, void* stream);
/* The same for every K the coarse form takes (K % 32 == 0, 32 <= K <= 16384).  Beyond 1,024 codes the
 * codebook goes through LDS in chunks of whole 32-code tiles over a (row block) x (chunk group) grid; every
 * (row, group) leaves its partial (coarse minimum, index, second-smallest) and every chunk its max |w|^2 and
 * inexact flag in `workspace` (qarig_bmu_coarse_workspace_bytes(rows, K) bytes; 0 and unused for K <= 1024),
 * and a finalize kernel merges them in code order, applies the same certificate and re-scans the other rows,
 * one wave per row, against the fp32 codebook: the same bit-identical indices.  uncertified as above
 * (re-scanned rows are counted by the finalize kernel; [5] += its clock64() cycles per block, [6] += its
 * blocks).  qarig_bmu_fwd takes this form only under option bmu_coarse = 1.  Returns the workspace error
 * when ws_bytes is too small. */
size_t qarig_bmu_coarse_workspace_bytes(int64_t rows, int K);
int qarig_bmu_fwd_coarse_ws(const float* x, int N, int C, int H, int W, int pH, int pW,
                            const float* codebook, int K, int D, int64_t* out_idx,
                            unsigned* uncertified, const void* prepared, void* workspace,
                            size_t ws_bytes, void* stream);
/* The staged form of a codebook for `prepared` above (may be NULL: every workgroup then stages the
 * codebook itself): qarig_bmu_prepare_bytes(K, D) bytes (0 = the coarse form does not apply), written
 * by qarig_bmu_prepare.  A frozen codebook -- tokenising a dataset (generate_fmap_dataset.py /
 * train_quantized_transformer.py:412-421 call get_patches_bmu with fixed codebooks every step) -- is
 * prepared once; its image must be rebuilt after the codebook changes.  K <= 1024: K * 100 + 16 bytes
 * (three planes of bf16 pieces, |w|^2, max |w|^2 and an inexact flag); 1024 < K <= 16384: that layout per
 * 512-code chunk, chunk after chunk (the chunking of an image is fixed: a search given one uses it). */
size_t qarig_bmu_prepare_bytes(int K, int D);
int qarig_bmu_prepare(const float* codebook, int K, int D, void* image, void* stream);

/* ---- SOM topology evaluation (additive, no reference counterpart) -------------- */

/* The two best-matching units of every patch row.  x, patch dims and codebook as qarig_bmu_fwd; 2 <= K <= 16384
 * (else QARIG_ERR_ARG), any D.  Per row r of N*(H/pH)*(W/pW): idx1, idx2 int64, d1, d2 fp32.  d(r,k) is the literal
 * definition of the search (fp32 fma chains for |w|^2 and |x|^2, the ascending chain of -2 w x, then
 * sqrtf(max((acc + w2) + x2, 0))); candidates are ordered by (d, k) lexicographically, (d1, idx1) is the minimum
 * and (d2, idx2) the minimum over k != idx1.  So idx1 equals qarig_bmu_fwd's index on every input that search
 * takes by this definition (more than 25 rows or more than 25 codes; with at most 25 of both qarig_bmu_fwd follows
 * torch.cdist into the direct form sqrt(sum (x - w)^2), this entry does not), duplicate
 * codes give d2 == d1 with idx2 > idx1, a row equal to a code gives d1 == 0.  Indices are always in [0, K): a NaN
 * distance is never taken and an unfilled slot reports d = +inf.  Every output element is written once, the
 * result of a row does not depend on N or on the other rows, no atomics. */
int qarig_bmu_top2(const float* x, int N, int C, int H, int W, int pH, int pW, const float* codebook, int K, int D,
                   int64_t* idx1, int64_t* idx2, float* d1, float* d2, void* stream);
/* Reduction of one qarig_bmu_top2 call of N images of seq rows each (N seq < 2^31, 2 <= K <= 2^24).
 * img_sums (N,3) fp64, written: {sum d1, sum d2, sum d1^2} per image, fp64 throughout in one fixed order (thread t
 * of 256 adds rows t, t + 256, ... in ascending order, then a 64-lane butterfly, then the four waves in order),
 * so an image's bits do not depend on its batch.  gap_hist int64 [K] += histogram of |idx1 - idx2|; ratio_hist
 * int64 [32] += histogram of min(31, floor(32 (double)d1 / (double)d2)), bin 31 where d2 == 0 (integer atomics;
 * both caller-initialised).  A row with an index outside [0, K) sets *bad_flag and is left out of gap_hist. */
int qarig_topology_rows(const int64_t* idx1, const int64_t* idx2, const float* d1, const float* d2, int N, int seq,
                        int K, double* img_sums, int64_t* gap_hist, int64_t* ratio_hist, int* bad_flag,
                        void* stream);
/* lag_sum fp64 [K]: lag_sum[r] = sum_{t=0}^{K-1-r} |w_t - w_{t+r}|_2 for r = 1 ... K-1 ([0] is not written);
 * codebook (K,D) fp32, K >= 2.  Differences, squares (fma, e ascending), sqrt and sums in fp64; one workgroup per
 * lag, thread t of 256 adds t, t + 256, ... in ascending order, then the butterfly and the four waves in order.
 * No atomics. */
int qarig_code_lag_profile(const float* codebook, int K, int D, double* lag_sum, void* stream);

/* ---- Linear algebra core ----------------------------------------------------- */

/* C[M,N] = epilogue(sum_k A(m,k) B(n,k)).  a_kcontig: A stored [M][K] (1) or
 * [K][M] (0); same for B over N.  Epilogue, in order: + bias[n]; + residual[m][n];
 * store to preact (if given); act(); * act'(gradz[m][n]) with activation id gact (if
 * gradz given); store to C.  splitk > 1 splits the reduction
 * over grid.z through fp32 slabs in `workspace`, summed in fixed order (the epilogue then
 * runs in the reduce pass; used for skinny-M decode GEMMs).  accumulate != 0
 * (plain epilogue only) adds the product to what C already holds (weight gradients are
 * accumulated straight into the flat .grad buffer).  a_rowsum (optional, [M]) receives
 * sum_k A(m,k) (added to it when accumulate): with A = dT^T this is the bias gradient,
 * computed from the A tiles the weight-gradient GEMM stages anyway.
 * Replaces nn.Linear (+activation) inside LinearLayer / ResidualLinearLayer
 * (models/layers.py:234-304) forward, and the three autograd contractions.
 * Ragged weight gradient (qarig_gemm_ragged_tn(M, N, K) != 0: a_kcontig = b_kcontig = 0, M = 128 q + r
 * output rows with q >= 2 and 1 <= r <= 8, N % 128 == 0, reduction K >= 4096 in whole 16-deep tiles --
 * the classifier's 513 = K_hr + 1 rows, models/Transformer.py:82-102 -- plain epilogue, 16-B aligned
 * operands, workspace given): the first 128 q rows run as the product of that shape, the last r rows
 * through per-row-block partials in the workspace summed in ascending order (no atomics: the same bits
 * on every run).  qarig_gemm_workspace_bytes(M, N, splitk) knows neither the layout nor K, so it includes the
 * partials (128 * r * (N + 1) floats) for EVERY M = 128 q + r with q >= 2, 1 <= r <= 8, whether the route is
 * taken or not.  A caller picks splitk for 128 q rows; without a workspace the call keeps its old kernels. */
int qarig_gemm_ragged_tn(int M, int N, int K);
/* Ragged forward product (qarig_gemm_ragged_nt(M, N, K) != 0: a_kcontig = b_kcontig = 1, N = 128 q + r output
 * columns with q >= 2 and 1 <= r <= 8, M >= 4096 rows in whole 128-row tiles, K in whole 16-deep tiles,
 * r * K <= 16384; taken with splitk = 1, no residual / gradz / accumulate / a_rowsum, 16-B aligned operands
 * and ldc, ldp multiples of 4 -- a dense (M, 513) output keeps the kernels it had): the first 128 q columns
 * run as the product of that shape at the caller's ldc, the last r columns on a kernel that streams A once,
 * with the same bias / pre-activation / activation epilogue and one fixed summation order. */
int qarig_gemm_ragged_nt(int M, int N, int K);
size_t qarig_gemm_workspace_bytes(int M, int N, int splitk);
int qarig_gemm_f32(const float* A, int64_t lda, int a_kcontig, const float* B, int64_t ldb,
                   int b_kcontig, float* C, int64_t ldc, int M, int N, int K, const float* bias,
                   const float* residual, int64_t ldr, float* preact, int64_t ldp, int act,
                   const float* gradz, int64_t ldz, int gact, int splitk, int accumulate,
                   float* a_rowsum, void* workspace, size_t ws_bytes, void* stream);

/* `groups` (1..16) products of ONE shape as one launch: C_g = epilogue(A_g B_g^T), every argument of
 * qarig_gemm_f32 with the pointers given as host arrays of `groups` device pointers (a NULL array =
 * that epilogue input absent for every group; entries of one array may repeat, e.g. a shared A).
 * Strides, layouts, activation ids, splitk and accumulate are common to the groups.
 * sum_groups != 0: C[0] (+)= sum_g A_g B_g^T (plain epilogue), summed over (g, split) in ascending
 * order.  Interior shapes only (qarig_gemm_grouped_supported: M, N multiples of 128, whole 16-deep
 * tiles per split, 16-B aligned operands).  The q / k / v two-layer MLPs of an attention layer
 * (models/layers.py:389-418) -- forward, both input gradients and both weight gradients -- run as
 * one such launch per product instead of three; the cross-attention k / v MLPs of every decoder
 * layer (models/layers.py:538-599, all reading the encoder output, models/Transformer.py:179-191)
 * as one launch per product for all layers. */
int qarig_gemm_grouped_supported(int M, int N, int K, int splitk);
size_t qarig_gemm_grouped_workspace_bytes(int groups, int M, int N, int splitk, int sum_groups);
int qarig_gemm_f32_grouped(int groups, const float* const* A, int64_t lda, int a_kcontig,
                           const float* const* B, int64_t ldb, int b_kcontig, float* const* C,
                           int64_t ldc, int M, int N, int K, const float* const* bias,
                           const float* const* residual, int64_t ldr, float* const* preact,
                           int64_t ldp, int act, const float* const* gradz, int64_t ldz, int gact,
                           int splitk, int accumulate, int sum_groups, float* const* a_rowsum,
                           void* workspace, size_t ws_bytes, void* stream);

/* Strided groups: C_g = act(A W_g^T + bias_g) for any number of groups that share A (M, K), with
 * W_g = W + g * w_gs (N, K), C_g = C + g * c_gs (M, N) and bias_g = bias + g * bias_gs (bias may be
 * NULL), as ONE launch of groups * (M / 128) * (N / 128) tiles on the kernel of qarig_gemm_f32's
 * interior shapes; a tile's result does not depend on the group count.  The training forward of
 * every ScaleLayer / ShiftLayer projection of a position table (models/layers.py:100-153, 258-304)
 * whose row count is a multiple of 128.  Shapes: qarig_gemm_grouped_supported(M, N, K, 1); 16-B
 * aligned operands, strides multiples of 4 elements, groups must not overlap. */
int qarig_gemm_f32_strided(const float* A, int64_t lda, const float* W, int64_t ldw, int64_t w_gs,
                           float* C, int64_t ldc, int64_t c_gs, const float* bias, int64_t bias_gs,
                           int groups, int M, int N, int K, int act, void* stream);

/* Opt-in reduced precision (BASELINE config 5: "fp8/bf16 MFMA attn/FFN"; never the fp32 parity
 * mode).  The Linear contractions of models/layers.py:234-304, 330-340, 389-418 with bf16
 * OPERANDS IN HBM, products on v_mfma_f32_32x32x16_bf16, fp32 accumulation and the same fused
 * fp32 epilogue as qarig_gemm_f32.  layout 0 = NT: A (M,K), B (N,K), reduction-contiguous
 * (forward x W^T; input gradient dT W with the W^T shadow as B); layout 1 = TN: A (K,M), B (K,N),
 * reduction-major (weight gradient dT^T x from the row-major activations, transposed on the LDS
 * read by ds_read_b64_tr_b16); layout 2 = NN: A (M,K) reduction-contiguous, B (K,N)
 * reduction-major (input gradient dT W on the weight shadow exactly as stored: no W^T copy).
 * A, B: bf16 (16-bit) elements, lda / ldb in elements.
 * C: fp32 output (may be NULL when Cb is given); Cb / Pb: optional bf16 copies of the output /
 * of the saved pre-activation for a consumer GEMM.  Shapes: qarig_gemm_lp_supported.
 * Every matrix argument of qarig_gemm_lp / _f8 / _mx has a leading dimension of its own (a view of a
 * larger buffer is a valid argument) under these rules, QARIG_ERR_ARG otherwise, nothing written:
 *  - A, B: 16-B aligned; lda, ldb % 8 elements (bf16) / % 16 bytes (e4m3; qarig_gemm_mx also
 *    lda, ldb >= K);
 *  - MX scale bytes sA, sB: 4-B aligned, ldsa, ldsb % 4 and >= K / 32;
 *  - C, bias, residual, preact and an fp32 gradz: 16-B aligned, leading dimension % 4;
 *  - Cb, Pb and a bf16 gradz: 8-B aligned, leading dimension % 4. */
int qarig_gemm_lp_supported(int M, int N, int K, int splitk);
size_t qarig_gemm_lp_workspace_bytes(int M, int N, int splitk);
int qarig_gemm_lp(const void* A, int64_t lda, const void* B, int64_t ldb, int layout, float* C,
                  int64_t ldc, int M, int N, int K, const float* bias, const float* residual,
                  int64_t ldr, float* preact, int64_t ldp, int act, const void* gradz, int64_t ldz,
                  int gradz_is_bf16, int gact, int splitk, int accumulate, void* Cb, int64_t ldcb,
                  void* Pb, int64_t ldpb, void* workspace, size_t ws_bytes, void* stream);

/* fp8 (OCP e4m3) forward products of the same Linear layers (BASELINE config 5 names the fp8
 * MFMA; models/layers.py:234-254, 389-418): A (M,K) and B (N,K) are e4m3 BYTES quantised per
 * tensor by qarig_cast_fp8 (scale 448 / max|x|; lda / ldb in bytes), products on
 * v_mfma_f32_32x32x64_f8f6f4, fp32 accumulation, the accumulator multiplied by the two device
 * scalars inv_a[0] * inv_b[0] before the usual epilogue.  qarig_cast_fp8: dst = n bytes,
 * inv_scale[0] receives max|x| / 448, scratch = 4 bytes of device memory (receives max|x|),
 * bf16_dst = optional bf16 copy of src from the same pass (the backward products read it). */
int qarig_gemm_f8_supported(int M, int N, int K);
int qarig_cast_fp8(const float* src, int64_t n, void* dst, float* inv_scale, void* scratch,
                   void* bf16_dst, void* stream);
int qarig_gemm_f8(const void* A, int64_t lda, const void* B, int64_t ldb, const float* inv_a,
                  const float* inv_b, float* C, int64_t ldc, int M, int N, int K, const float* bias,
                  const float* residual, int64_t ldr, float* preact, int64_t ldp, int act, void* Cb,
                  int64_t ldcb, void* Pb, int64_t ldpb, void* stream);

/* MX-e4m3 ("mxfp8" mode: every product of the reduced-precision Linear nodes, forward and backward;
 * models/layers.py:234-254, 330-340, 389-418).  The format (OCP microscaling, e4m3 elements):
 *  - elements are OCP e4m3fn bytes; each block of 32 consecutive elements along the product's
 *    reduction dimension has one e8m0 scale byte E = e + 127 (value 2^e);
 *  - e is the smallest integer with max|x| over the block <= 448 * 2^e (no element saturates),
 *    clamped to [-127, 127]; an all-zero block has e = 0;
 *  - element = round-to-nearest-even of x * 2^-e to e4m3fn (the multiplication is exact in fp32);
 *  - non-finite input is out of scope: a NaN does not enter its block's maximum and quantises to the
 *    e4m3 NaN byte; an infinity gives its block e = 120 and unspecified elements.
 * Every operand is a (rows, K) byte matrix blocked along K with scales (rows, K/32):
 *  - row form of a tensor (R, C): as stored, blocked along C, scales (R, C/32);
 *  - transposed form: (C, Rp), Rp = R rounded up to 128, blocked along R, scales (C, Rp/32); the
 *    padding columns are zero (scale byte 127).
 * forward x W^T = (x row, W row); input gradient dT W = (dT row, W transposed); weight gradient
 * dT^T x = (dT transposed, x transposed): every product is NT on one kernel.
 * qarig_mx_quant: one pass over src (fp32, or bf16 with src_is_bf16; row stride ld elements,
 * C % 128 == 0) writing any of the row form (q, q_scale), the transposed form (qt, qt_scale) and
 * colsum (+)= the fp32 column sums (workspace: qarig_mx_quant_workspace_bytes, needed with colsum).
 * qarig_gemm_mx: C = epilogue(sum_k A[m][k] B[n][k]) on v_mfma_scale_f32_32x32x64_f8f6f4 with
 * the scale bytes applied in the instruction; A, B bytes (lda / ldb in bytes), sA (M, K/32), sB
 * (N, K/32) (ldsa / ldsb in bytes); epilogue, split-K (workspace: qarig_gemm_mx_workspace_bytes)
 * and accumulate as qarig_gemm_lp.  Shapes: qarig_gemm_mx_supported. */
size_t qarig_mx_quant_workspace_bytes(int R, int C);
int qarig_mx_quant(const void* src, int64_t ld, int src_is_bf16, int R, int C, void* q, void* q_scale,
                   void* qt, void* qt_scale, float* colsum, int accumulate, void* workspace,
                   size_t ws_bytes, void* stream);
int qarig_gemm_mx_supported(int M, int N, int K, int splitk);
size_t qarig_gemm_mx_workspace_bytes(int M, int N, int splitk);
int qarig_gemm_mx(const void* A, int64_t lda, const void* sA, int64_t ldsa, const void* B, int64_t ldb,
                  const void* sB, int64_t ldsb, float* C, int64_t ldc, int M, int N, int K,
                  const float* bias, const float* residual, int64_t ldr, float* preact, int64_t ldp,
                  int act, const void* gradz, int64_t ldz, int gradz_is_bf16, int gact, int splitk,
                  int accumulate, void* Cb, int64_t ldcb, void* Pb, int64_t ldpb, void* workspace,
                  size_t ws_bytes, void* stream);

/* Operand conversion of the reduced-precision mode (no reference counterpart): fp32 -> bf16,
 * round to nearest even; n contiguous elements, or the transpose (C, R) of a (R, C) matrix
 * with row stride ld (the W^T shadow of an nn.Linear weight). */
int qarig_cast_bf16(const float* src, void* dst, int64_t n, void* stream);
int qarig_cast_transpose_bf16(const float* src, int64_t ld, int R, int C, void* dst, void* stream);
/* colsum[n] (+)= sum_m src[m][n] in a fixed order -- the bias gradient of nn.Linear
 * (models/layers.py:243-250) -- and, when dst is given, dst = bf16(src) in the same pass over
 * src (fp32, or bf16 with src_is_bf16 = 1 and dst NULL). */
size_t qarig_cast_colsum_workspace_bytes(int M, int N);
int qarig_cast_colsum(const void* src, int64_t ld, int src_is_bf16, int M, int N, void* dst,
                      float* colsum, int accumulate, void* workspace, size_t ws_bytes, void* stream);

/* 1 when qarig_gemm_f32 runs an (M, N, K) product on 64 x 64 tiles (whole 64-tiles, 16-deep k-tiles, fewer
 * than 192 tiles of 128 x 128: the 512-wide Linear products of a 2,048-row shard, models/layers.py:291-304);
 * a caller that chooses the reduction split counts those tiles. */
int qarig_gemm_tile64(int M, int N, int K);

/* 1 when, under option gemm_x3 (qarig_set_option("gemm_x3", 1); off by default), qarig_gemm_f32 runs an
 * (M, N, K) product with `splitk` reduction splits on the bf16 matrix pipe: both fp32 operands split on
 * the fly into three bf16 pieces that add up to them exactly, six products per block accumulated in fp32
 * (csrc/gemm_x3.hip: whole 128 x 128 tiles and 32-deep k-tiles per split).  Same operands, epilogue and
 * tolerances as the fp32-MFMA kernels (models/layers.py:234-254, 330-340); non-finite operands give NaN. */
int qarig_gemm_x3_ok(int M, int N, int K, int splitk);

/* `groups` independent skinny products in one launch, C_g = act(A_g W_g^T + bias_g) with
 * X_g = X + g * x_gs (a_gs == 0 shares the activations).  Decode steps use it for the q/k/v
 * MLPs (models/layers.py:389-418) and for every projection of the conditioning vector
 * (ScaleLayer/ShiftLayer, models/layers.py:100-153, 258-304) of all layers at once.
 * Requires M <= 512, K % 256 == 0, reduction-contiguous 16-B aligned operands. */
int qarig_gemm_grouped_skinny_f32(const float* A, int64_t lda, int64_t a_gs, const float* W,
                                  int64_t ldw, int64_t w_gs, float* C, int64_t ldc, int64_t c_gs,
                                  const float* bias, int64_t bias_gs, int groups, int M, int N,
                                  int K, int act, void* stream);

/* The decode step's fused form of the launch above: C_g = act(LN(X) W_g^T + bias_g) [* mul].
 * The activations X (M, K) are shared by the groups and LayerNorm'ed over K on the way in
 * (biased variance, eps) -- nn.LayerNorm's affine form (gamma, beta: K) or the AdaLN form
 * scale(cond) * LN(x) + shift(cond) (scale, shift: (M, K) rows at ldmod; reference
 * models/layers.py:130-153); all four null = no normalisation.  mul (M, N) at ldmul, optional, is
 * an elementwise factor on the output, the same for every group (ResidualLinearLayer's
 * x * scale(cond), models/layers.py:258-304).  Replaces the LayerNorm launch in front of a block's
 * first Linear and the gate multiply behind its last (generate_images.py:283-290 evaluates these
 * per generated token).  Same shape rules as qarig_gemm_grouped_skinny_f32. */
int qarig_gemm_skinny_ln_f32(const float* X, int64_t ldx, float eps, const float* gamma,
                             const float* beta, const float* scale, const float* shift,
                             int64_t ldmod, const float* W, int64_t ldw, int64_t w_gs, float* C,
                             int64_t ldc, int64_t c_gs, const float* bias, int64_t bias_gs,
                             const float* mul, int64_t ldmul, int groups, int M, int N, int K,
                             int act, void* stream);

/* The Linear of a single-token decode step (generate_images.py:283-286 evaluates the decoder per
 * sampled token; with a key/value cache only the new row of each sequence is computed):
 *   C_g = act(LN(X_g) W_g^T + bias_g + residual) * mul        M <= 16 rows, `groups` products.
 * A weight-streaming kernel whose loads are all issued before its first wait (the step is a chain
 * of ~80 dependent launches, each bound by its memory round trips, not by bytes).  LN over K:
 * nn.LayerNorm's affine form (gamma, beta: K) or AdaLN's scale(cond) * LN(x) + shift(cond)
 * (scale, shift rows at ldmod, models/layers.py:130-153; ldmod == 0: ONE row for every activation
 * row -- the rows of a decode step share their window position); residual (M, N): the skip input
 * of ResidualLinearLayer (models/layers.py:291-304); mul (M, N) at ldmul (0: one row): its
 * x * scale(cond) gate applied by the producer.  X_g = X + g * x_gs (0 shares X).
 * qarig_decode_linear_supported: M <= 16 and K in {256, 512, 1024} (2048, 4096 when ln == 0). */
int qarig_decode_linear_supported(int M, int N, int K, int ln);
int qarig_decode_linear_f32(const float* X, int64_t ldx, int64_t x_gs, float eps,
                            const float* gamma, const float* beta, const float* scale,
                            const float* shift, int64_t ldmod, const float* W, int64_t ldw,
                            int64_t w_gs, const float* bias, int64_t bias_gs, const float* residual,
                            int64_t ldr, const float* mul, int64_t ldmul, float* C, int64_t ldc,
                            int64_t c_gs, int groups, int M, int N, int K, int act, void* stream);

/* The same launch with the weights streamed as bf16: W is a row-major (N, K) bf16 image of the fp32 weight
 * (qarig_cast_bf16: rounded once, to nearest even), ldw and w_gs in bf16 elements -- half the bytes per token
 * of the Linear layers generate_images.py:283-286 evaluates per sampled token (models/layers.py:60-98).
 * Only the weights are reduced: X, LN, the fp32 accumulation, bias / residual / act / mul and C are as in
 * qarig_decode_linear_f32, and bf16 -> fp32 is exact, so the result is that entry's on the rounded weights
 * (same fixed summation order per shape, no atomics).  Same shapes (qarig_decode_linear_supported) and
 * checks, plus ldw % 8 == 0, w_gs % 8 == 0 and W 16-B aligned.  Weight-only: not the fp32 parity mode. */
int qarig_decode_linear_bf16w(const float* X, int64_t ldx, int64_t x_gs, float eps,
                              const float* gamma, const float* beta, const float* scale,
                              const float* shift, int64_t ldmod, const void* W, int64_t ldw,
                              int64_t w_gs, const float* bias, int64_t bias_gs, const float* residual,
                              int64_t ldr, const float* mul, int64_t ldmul, float* C, int64_t ldc,
                              int64_t c_gs, int groups, int M, int N, int K, int act, void* stream);

/* ---- Device-resident sampling loop (generate_images.py:256-345) ------------------------------
 * The reference samples a token, appends it on the host and re-runs the decoder.  Here the loop's
 * state stays on the device and the host only enqueues launches, never reading a token back: `ctl` is an int32 array
 * of QARIG_DECODE_CTL_WORDS words -- [0] window index of the token the next step evaluates,
 * [1] window index at which the current chunk of beam_width tokens starts, [2] draws made so far
 * (row of the uniform / forced / log buffers), [3] candidate chunks evaluated at this position,
 * [4] decoder steps since the candidate began (the chunk slot the next draw fills), [5] tokens in the
 * window step's token ring (qarig_window_*). */
#define QARIG_DECODE_CTL_WORDS 8

/* Keys a wave of qarig_decode_attention / qarig_window_attention covers per pass of its loop at head dim d
 * (the constant the launch uses: 256 / 128 / 64 for d = 4 ... 16 / 32 / 64, the grouped kernel's own for the
 * other multiples of 4 up to 128), or 0 when d is not supported.  Lengths around its multiples are the
 * kernel's edge cases. */
int qarig_decode_attention_keys_per_pass(int d);

/* First launch of a step: x[b] = table[ids[b]] + pe[len] (models/Transformer.py:154-167; pe may be
 * NULL), len = ctl[0] (ctl NULL: the `len` argument), and the copy of row `len` of proj_table
 * (max_len rows of proj_row_floats floats: every ScaleLayer / ShiftLayer projection of `cond` --
 * models/layers.py:100-153, 258-304 -- evaluated once per window position of the stage) into
 * proj_row.  With ctl it also counts the step: ctl[4] += 1.  An id outside [0, V) sets *bad_flag and
 * yields a zero row. */
int qarig_decode_embed(const int64_t* ids, int B, int D, int V, const float* table, const float* pe,
                       int* ctl, int len, int max_len, const float* proj_table,
                       int64_t proj_row_floats, float* x, float* proj_row, int* bad_flag, void* stream);

/* qarig_attention_decode with the cache layout given by strides -- row j of head h of sequence n at
 * n * batch_stride + h * head_stride + j * row_stride: row-major (head_stride = d, row_stride = H * d) or
 * head-major (row_stride = d, head_stride >= max_len * d: a head's keys contiguous, what the kernel's
 * lane-per-key loads coalesce on) -- and the o_mul factor at row stride ldmul (0: one row for every
 * sequence).  The same contract on the cache's contents and on an out-of-range len_dev.
 * d: a multiple of 4 from 4 to 128.  4, 8, 16, 32 and 64 run a lane-per-key kernel; every other one a kernel
 * whose keys are shared by groups of 2 or 4 lanes (rows stay compact: channels at or beyond d are never
 * loaded).  Any other d is refused. */
int qarig_decode_attention(const float* q, const float* k_new, const float* v_new, float* kcache,
                           float* vcache, int B, int H, int d, int len, const int* len_dev,
                           int max_len, int64_t batch_stride, int64_t head_stride, int64_t row_stride,
                           float sqrt_d, const float* o_mul, int64_t ldmul, float* o, void* stream);

/* One sampling draw per row as generate_images.py:289-304 makes it (train_quantized_transformer.py:
 * 626-636 with generate_mode == 0): probs = softmax(logits / temperature), generate mode zeroes
 * probs[end_token], a token is drawn in proportion to probs by inverse CDF from uniforms[draw][b]
 * (draw = ctl[2] + slot; slot == -1: the slot the device counts, ctl[4]; the reference's
 * torch.multinomial consumes its generator differently: same distribution, not the same stream), comb[b] *= probs[token], train mode maps <end> to 0,
 * token + shift goes to ids[b] and chunk[b][slot]; inc_len != 0 advances ctl[0].  forced (optional):
 * entries >= 0 are taken instead of drawing; probs_log (optional, (max_draws, B, V)): the rows
 * sampled from.  beams > 0: the B rows are `beams` independent candidate chunks per image evaluated as
 * one batch while every draw keeps the number the reference's candidate-after-candidate loop gives it
 * (generate_images.py:262-304): row image * beams + c reads column `image` of draw row
 * ctl[2] + c * beam_width + slot; uniforms / forced / probs_log then have B / beams columns. */
int qarig_decode_sample(const float* logits, int64_t ldl, int B, int V, float temperature,
                        int end_token, int generate_mode, int64_t shift, const float* uniforms,
                        const int64_t* forced, int* ctl, int slot, int beam_width, int max_draws,
                        int inc_len, int beams, int64_t* ids, int64_t* chunk, float* comb,
                        float* probs_log, void* stream);

/* qarig_decode_sample with the row filtered before the draw (a kernel of its own: a workgroup per row, the
 * row staged once in LDS, the cuts found by a bitwise threshold search instead of a sort).  probs is computed
 * as above; filtering only zeroes entries:
 *   top_k (0: off): the top_k largest non-zero entries stay; equal entries at the cut stay in index order
 *     (lower index first); top_k >= the number of non-zero entries changes nothing;
 *   top_p (in (0, 1], 1: off), on what top_k left: with q = probs / sum(probs) in descending order (equal
 *     entries: lower index first), an entry stays iff the q-mass strictly in front of it is < top_p; the
 *     largest entry always stays.
 * Kept entries keep their values -- no renormalisation: the draw scales its target by the row's total, and
 * comb takes the probability it would take without a filter.  forced tokens are taken whether or not they
 * were kept (comb then takes the filtered value, possibly 0); probs_log receives the filtered row.  Every
 * sum runs in a fixed order: the same input gives the same bits.  top_k < 0, top_p outside (0, 1] or NaN,
 * and V > 32768 (the row must fit LDS) are refused with status -1. */
int qarig_decode_sample_filtered(const float* logits, int64_t ldl, int B, int V, float temperature,
                                 int end_token, int generate_mode, int64_t shift, const float* uniforms,
                                 const int64_t* forced, int* ctl, int slot, int beam_width, int max_draws,
                                 int inc_len, int beams, int64_t* ids, int64_t* chunk, float* comb,
                                 float* probs_log, int top_k, float top_p, void* stream);

/* After a candidate chunk: per image the beam with the largest product (first on ties) replaces the
 * kept chunk unless the kept product is >= (generate_images.py:325-337); take[n] = 1 + that beam or
 * 0; comb is reset to 1, ctl: candidate + 1, draws + `draws` (the draw rows the candidate set consumed),
 * len back to the chunk start. */
int qarig_decode_decide(int* ctl, int N, int NB, int beam_width, int draws, float* comb,
                        const int64_t* chunk, float* best_p, int64_t* best_chunk, int* take, void* stream);

/* Cache rows [ctl[1], ctl[1] + R) of the head-major kv (layers2 = layers * 2, N * NB, H, max_len, d):
 * restore == 0 copies the winning beam's rows of the images with take[n] > 0 into staged
 * (layers2, N, H, R, d); restore == 1 writes the staged rows into every beam of every image. */
int qarig_decode_rows(const int* ctl, float* kv, float* staged, const int* take, int layers2, int N,
                      int NB, int H, int R, int d, int max_len, int restore, void* stream);

/* Prefix prefill: token-major k / v (images, P1, H * d), row stride ld and image stride batch_stride in
 * floats (a column sub-view of a wider buffer is fine), into rows [0, P1) of ONE layer of the head-major
 * cache, kv (2, images * beams, H, max_len, d): keys into half 0, values into half 1, the same rows into
 * every one of the `beams` candidate rows of an image.  Nothing else of kv is written.  16-B loads and
 * stores: d % 4 == 0, ld % 4 == 0, batch_stride % 4 == 0, 16-B aligned operands.  P1 > max_len, a row
 * stride shorter than H * d, null or misaligned pointers and non-positive extents are refused (-1). */
int qarig_decode_cache_fill(const float* k, const float* v, int64_t ld, int64_t batch_stride, float* kv,
                            int images, int beams, int H, int d, int P1, int max_len, void* stream);

/* tokens[n][ctl[1] + j] = best_chunk[n][j]; ids of every beam = the chunk's last token;
 * ctl[0] = ctl[1] + beam_width - 1 (the step that follows produces the next chunk's first logits). */
int qarig_decode_commit(int* ctl, int N, int NB, int beam_width, const int64_t* best_chunk,
                        int64_t* tokens, int64_t ldt, int64_t* ids, void* stream);

/* ctl[1] += beam_width; ctl[0] = ctl[1]; ctl[3] = 0. */
int qarig_decode_advance(int* ctl, int beam_width, void* stream);

/* ---- Device-resident evaluation of the slid window (generate_images.py:275-290) ----------------
 * Once the window slides, the reference re-runs the decoder on the last window - 1 tokens with
 * window-relative positional embeddings (models/Transformer.py:154-167, dec_pos_index = 1..Seq) and reads
 * the last token's logits.  These entry points keep that evaluation a replay of one captured graph. */

/* 1 when R sequences (1..16), a window of `window` tokens, model width D (a multiple of 4) and H
 * self-attention heads (head dim D / H a multiple of 4 from 4 to 128) fit the window step, else 0. */
int qarig_window_step_supported(int R, int window, int D, int H);

/* The window in front of ring length n = ctl[5]: start = n - W1; x[r][s] = table[ring[r][start + s]] +
 * pe[s] for s < W1 (pe row s: the sinusoid of window position s + 1, models/Transformer.py:154-167), the
 * row s = W1 of Wp = W1 + 1 repeats s = W1 - 1 (whole 128-row tiles).  rowmap[r * Wp + s] (optional):
 * the token's row of the stage's conditioning table -- its absolute position, 0 for ring column 0 and
 * column + pos_off behind it (generate_images.py:306-322 numbers appended tokens cur + tok + 1);
 * last_map[r] (optional): that of the last real token.  An id outside [0, V), a position outside [0, P)
 * or a start outside the ring sets *bad_flag and is clamped. */
int qarig_window_assemble(const int64_t* ring, int64_t ldr, const int* ctl, int R, int W1, int Wp, int D,
                          int V, const float* table, const float* pe, int P, int pos_off, float* x,
                          int* rowmap, int* last_map, int* bad_flag, void* stream);

/* Masked self-attention of the window's last real token (models/layers.py:433-474, the last row of the
 * causal softmax(q k^T / sqrt(d)) v): q (R, H * d), k / v token-major rows of H * d floats, `rows` per
 * sequence at batch_stride, the first n_keys of them attended (a pad row behind them is ignored);
 * o = result (* o_mul at row stride ldmul, 0: one row for all).  d as for qarig_decode_attention. */
int qarig_window_attention(const float* q, const float* k, const float* v, int R, int H, int d, int n_keys,
                           int rows, int64_t batch_stride, const float* o_mul, int64_t ldmul, float* o,
                           void* stream);

/* The sampled token joins the sequence (generate_images.py:306-310, a torch.cat on the host there):
 * ring[b][ctl[5]] = ids[b], ctl[5] += 1.  A column outside the ring sets *bad_flag and writes nothing. */
int qarig_window_append(int* ctl, const int64_t* ids, int64_t* ring, int B, int64_t ldr, int* bad_flag,
                        void* stream);

/* out[N] = column sums of X[M][N] in a fixed order (bias / LayerNorm-affine grads). */
size_t qarig_colsum_workspace_bytes(int M, int N);
int qarig_colsum_f32(const float* X, int64_t ldx, int M, int N, float* out, int accumulate,
                     void* workspace, size_t ws_bytes, void* stream);

/* The reductions qarig_gemm_f32 launches behind a split-K product, as an entry of their own:
 * out[M][N] (ld ldc) (+)= sum_z slabs[z][M][N], z ascending from 0.0f, and, where rs_part / rs_out
 * are given, rs_out[M] (+)= sum_z rs_part[z][M] in the same launch.  16-B accesses when N % 4 == 0,
 * ldc % 4 == 0 and slabs / out are 16-B aligned, scalar otherwise: the same bits either way. */
int qarig_slab_reduce_rowsum_f32(const float* slabs, float* out, int64_t ldc, int M, int N, int nslab,
                                 int accumulate, const float* rs_part, float* rs_out, void* stream);

/* ---- Codebook (continued) ------------------------------------------------------ */

/* patchify / unpatchify -- models/layers.py:8-34 / :37-71.  image (N,C,H,W) <->
 * patches (N*Seq, C*pH*pW).  H,W must be multiples of the patch here. */
int qarig_patchify_fwd(const float* image, int N, int C, int H, int W, int pH, int pW,
                       float* patches, void* stream);
int qarig_unpatchify_fwd(const float* patches, int N, int C, int H, int W, int pH, int pW,
                         float* image, void* stream);

/* Codebook.get_quantized_image -- models/Codebook.py:138-154: image = unpatchify(
 * codebook[ids]).  ids int64 (N*Seq); *bad_flag (device int, caller-zeroed) is set on
 * an id outside [0,K). */
int qarig_codebook_gather_image(const int64_t* ids, int N, int C, int H, int W, int pH, int pW,
                                const float* codebook, int K, float* image, int* bad_flag,
                                void* stream);

/* nn.Embedding row gather out[r] = table[ids[r]] -- models/Codebook.py:132,144. */
int qarig_gather_rows(const int64_t* ids, int64_t R, int D, int K, const float* table, float* out,
                      int* bad_flag, void* stream);

/* Gaussian index-neighbourhood weights g[r][j] = exp(-(j-bmu[r])^2 / two_var) --
 * models/Codebook.py:112-126 (the (R,K)@(K,D) product then goes through qarig_gemm_f32). */
int qarig_som_weights_fwd(const int64_t* bmu, int64_t R, int K, float two_var, float* g,
                          void* stream);

/* The same neighbourhood without the (R,K) matrix: out[j] = sum_{|j-b| <= reach} exp(-(j-b)^2 / two_var) in[b]
 * over a (K,D) table.  models/Codebook.py:112-130's product equals gather_rows(bmu, band(codebook)) and its
 * codebook gradient band(embedding_bwd(bmu, dq)); `reach` bounds the dropped weights (host: < 2^-40). */
int qarig_som_band(const float* in, int K, int D, float two_var, int reach, float* out, void* stream);

/* counts (int64 [K]) += histogram of ids -- the per-unit BMU usage count of
 * prune_codebook.py:129-142. */
int qarig_index_histogram(const int64_t* ids, int64_t n, int K, int64_t* counts, int* bad_flag,
                          void* stream);

/* ---- Transformer pieces ------------------------------------------------------- */

/* get_positional_embeddings -- models/layers.py:83-96.  pos fp32 (R,), freq (D/2,)
 * (host-computed exactly as the reference does), out (R,D) = [sin | cos]. */
int qarig_posemb_fwd(const float* pos, int R, int D, const float* freq, float* out, void* stream);

/* Token assembly of the training hot loop (train_quantized_transformer.py:423-484) in one launch:
 * from the LR / HR BMU indices to the windowed decoder input, target and absolute positions
 * (base: [lr | hr + k_lr] / enc-dec: [<start> | hr]; target [hr | <end>]; window of W tokens
 * starting at offs[n]; pos = offs[n] + w).  Replaces cat + unfold + gather + arange on the host.
 * *bad_flag (device int, caller-zeroed, may be NULL) is set on a window start outside
 * [0, S_in - W]; the window is then clamped (torch.gather would raise). */
int qarig_assemble_tokens(const int64_t* lr, int S_lr, const int64_t* hr, int S_hr, int N, int base,
                          int k_lr, int k_hr, const int64_t* offs, int W, int64_t* hr_in,
                          int64_t* hr_tg, int64_t* pos, int* bad_flag, void* stream);

/* Token noise (additive: the reference has none): a training-time corruption of the tokens a stage
 * READS -- the teacher-forced hr tokens of the decoder input (stream 0) and the lr tokens an encoder conditions on
 * (stream 1) -- with the targets left clean.  Token j of the full, un-windowed stream (S tokens) of sample n makes
 * one Philox4x32-10 call (that of qarig_dropout below) with key (seed_lo, seed_hi) and counter
 * (n S + j, 2^30 | stream, step, rank); bit 30 set and bit 31 clear keeps the counters apart from residual dropout
 * (small site ordinals) and attention dropout (bit 31 set) under the same key.  With out[4] the call's result the
 * token is unchanged iff (out[0] & 0xffff) >= threshold (replace rate threshold / 65536) and otherwise becomes
 * lo + ((uint64)out[1] span >> 32): range == 0 draws from the whole codebook (lo = 0, span = K), range > 0 from
 * the SOM neighbourhood [lo, hi] = [max(0, id - range), min(K - 1, id + range)], span = hi - lo + 1.  The draw may
 * return the id itself: the effective change rate is threshold / 65536 (1 - 1 / span).  An id outside [0, K)
 * passes through (qarig_embedding_fwd flags it).  key: DEVICE uint32[4] {seed_lo, seed_hi, step, rank}.
 *
 * qarig_assemble_tokens_noise is qarig_assemble_tokens with stream 0 applied to the hr tokens of hr_in, in the hr
 * codebook's range (K = k_hr) and before the base model's + k_lr; j is the index into hr, so a token's noise does
 * not depend on the window that shows it.  <start> and the base model's leading lr tokens are never corrupted;
 * hr_tg and pos are the plain entry's bits.  qarig_token_noise corrupts a whole (N,S) tensor (out may be ids
 * itself; any other overlap is refused) and agrees with the fused entry for stream 0 over hr.  Refused (-1)
 * without a launch: null pointers, threshold outside [1, 58982], range < 0, K < 1, N S >= 2^31 (N S_hr for the
 * fused entry), stream_id outside {0, 1}. */
int qarig_assemble_tokens_noise(const int64_t* lr, int S_lr, const int64_t* hr, int S_hr, int N, int base,
                                int k_lr, int k_hr, const int64_t* offs, int W, int64_t* hr_in,
                                int64_t* hr_tg, int64_t* pos, int* bad_flag, uint32_t threshold, int range,
                                const uint32_t* key, void* stream);
int qarig_token_noise(const int64_t* ids, int64_t* out, int N, int S, int K, uint32_t threshold, int range,
                      int stream_id, const uint32_t* key, void* stream);

/* nn.Embedding + additive position table -- models/Transformer.py:127-139,154-167.
 * ids int64 (M = N*S); pe (S,D) or NULL; out (M,D). */
int qarig_embedding_fwd(const int64_t* ids, int M, int S, int D, int V, const float* table,
                        const float* pe, float* out, int* bad_flag, void* stream);
/* dtable[v] = sum_{m: ids[m]==v} dy[m], m ascending (autograd of nn.Embedding). */
int qarig_embedding_bwd(const int64_t* ids, int M, int D, int V, const float* dy, float* dtable,
                        void* stream);

/* nn.LayerNorm(D) (gamma,beta) / AdaLNZero modulation (scale,shift per token) --
 * models/layers.py:130-153,327,499,559.  Exactly one of the pairs, or neither. */
int qarig_layernorm_fwd(const float* x, int M, int D, float eps, const float* gamma,
                        const float* beta, const float* scale, const float* shift,
                        const int* mod_idx, float* y, float* mean, float* rstd, void* stream);
/* dx_add (optional, (M,D)): added to dx -- the gradient that reaches the same x through the block's
 * skip connection (models/layers.py:362-366, 530-534, 595-599), so that autograd's accumulation
 * of the two contributions is not a separate elementwise launch. */
int qarig_layernorm_bwd(const float* dy, const float* x, const float* mean, const float* rstd,
                        const float* gamma, const float* scale, const int* mod_idx, int M, int D,
                        float* dx, float* dy_xhat, const float* dx_add, void* stream);

/* Position-table form of the conditioning path.  `cond` (models/Transformer.py:154-167) is a
 * function of the token's integer position alone, so pos_cond_layer and every
 * ScaleLayer/ShiftLayer projection (models/layers.py:100-153, 258-304) are evaluated once per
 * distinct position into (P,D) tables and the per-token consumers index them:
 *   - qarig_layernorm_fwd/bwd with mod_idx (int32 (M,)): scale/shift row = table[mod_idx[row]];
 *     mod_idx == NULL keeps the per-token (M,D) scale/shift form;
 *   - qarig_mul_rows_fwd/bwd: y[r] = a[r] * tab[idx[r]] (ResidualLinearLayer's x * scale(cond));
 *   - qarig_rowmap_build + qarig_segment_sum: gradient of a table row = sum of its tokens'
 *     per-token gradients in ascending token order (deterministic, no atomics).
 * counts: P ints scratch; offsets: P+1 ints; rows: M ints; *bad_flag is set when an index is
 * outside [0,P). */
int qarig_rowmap_build(const int* idx, int M, int P, int* counts, int* offsets, int* rows,
                       int* bad_flag, void* stream);
int qarig_segment_sum(const float* src, const int* offsets, const int* rows, int P, int D,
                      float* out, void* stream);
int qarig_mul_rows_fwd(const float* a, const float* tab, const int* idx, float* y, int M, int D,
                       void* stream);
int qarig_mul_rows_bwd(const float* dy, const float* a, const float* tab, const int* idx, float* da,
                       float* db_tok, int M, int D, void* stream);
/* The two backward passes above with the table sums inside: one workgroup per table position walks
 * the position's tokens (offsets / rows of qarig_rowmap_build), writes the per-token gradient and adds
 * the table contribution in registers, in qarig_segment_sum's order -- dx / da and the (P,D) tables
 * are bit-identical to qarig_layernorm_bwd (mod_idx, dy_xhat) / qarig_mul_rows_bwd followed by
 * qarig_segment_sum, without the (M,D) intermediate and its launches.  Positions without tokens get
 * zeros.  D = 256, 512 or 1024, 16-B aligned; dx_add optional. */
int qarig_layernorm_bwd_table(const float* dy, const float* x, const float* mean, const float* rstd,
                              const float* scale_tab, const int* offsets, const int* rows, int M, int P,
                              int D, float* dx, const float* dx_add, float* dscale, float* dshift,
                              void* stream);
int qarig_mul_rows_bwd_table(const float* dy, const float* a, const float* tab, const int* offsets,
                             const int* rows, int M, int P, int D, float* da, float* dg, void* stream);

/* AttentionLayer core -- models/layers.py:433-474.  q (N,Sq,H*d); k,v (N,Sk,H*d);
 * o (N,Sq,H*d); lse (N,H,Sq); sqrt_d = float(d ** 0.5). */
int qarig_attention_fwd(const float* q, const float* k, const float* v, int N, int Sq, int Sk,
                        int H, int d, int causal, float sqrt_d, float* o, float* lse,
                        void* stream);
int qarig_attention_bwd(const float* q, const float* k, const float* v, const float* o,
                        const float* dO, const float* lse, int N, int Sq, int Sk, int H, int d,
                        int causal, float sqrt_d, float* dq, float* dk, float* dv, float* delta,
                        void* stream);

/* The same attention (models/layers.py:433-474) with the QK^T / PV products and their backward
 * counterparts on the bf16 MFMA (operands rounded to bf16; fp32 accumulation, softmax, LSE and
 * tensors): BASELINE config 5's reduced-precision attention.  Opt-in; same arguments. */
int qarig_attention_lp_fwd(const float* q, const float* k, const float* v, int N, int Sq, int Sk, int H,
                           int d, int causal, float sqrt_d, float* o, float* lse, void* stream);
int qarig_attention_lp_bwd(const float* q, const float* k, const float* v, const float* o,
                           const float* dO, const float* lse, int N, int Sq, int Sk, int H, int d,
                           int causal, float sqrt_d, float* dq, float* dk, float* dv, float* delta,
                           void* stream);

/* The four entries above with attention-probability dropout: o = ((M s) . softmax(S)) V, where the
 * keep bit M of element (n, h, i, j) -- query i against key j, head h, sequence n -- comes from the Philox call
 * of qarig_dropout below with counter ((n H + h) Sq + i, 2^31 | site << 23 | j >> 3, step, rank): one call
 * serves the keys j & ~7 ... j | 7 of one query, key j reads word (j & 7) >> 1, low half when j is even, and is
 * kept iff that value >= threshold.  The mask is regenerated in registers by the forward and both backward
 * passes; lse is that of the undropped softmax; dS = P (M s dP - delta), dV = s sum_i M P dO.  threshold and
 * scale as for qarig_dropout; key: DEVICE uint32[4] {seed_lo, seed_hi, step, rank}.  Refused (-1) without a
 * launch: a null key, head dim 128, threshold outside [1, 58982], site >= 256, Sk > 2^26, N H Sq >= 2^32. */
int qarig_attention_dropout_fwd(const float* q, const float* k, const float* v, int N, int Sq, int Sk, int H,
                                int d, int causal, float sqrt_d, float* o, float* lse, void* stream,
                                uint32_t threshold, float scale, uint32_t site, const uint32_t* key);
int qarig_attention_dropout_bwd(const float* q, const float* k, const float* v, const float* o,
                                const float* dO, const float* lse, int N, int Sq, int Sk, int H, int d,
                                int causal, float sqrt_d, float* dq, float* dk, float* dv, float* delta,
                                void* stream, uint32_t threshold, float scale, uint32_t site,
                                const uint32_t* key);
int qarig_attention_dropout_lp_fwd(const float* q, const float* k, const float* v, int N, int Sq, int Sk, int H,
                                   int d, int causal, float sqrt_d, float* o, float* lse, void* stream,
                                   uint32_t threshold, float scale, uint32_t site, const uint32_t* key);
int qarig_attention_dropout_lp_bwd(const float* q, const float* k, const float* v, const float* o,
                                   const float* dO, const float* lse, int N, int Sq, int Sk, int H, int d,
                                   int causal, float sqrt_d, float* dq, float* dk, float* dv, float* delta,
                                   void* stream, uint32_t threshold, float scale, uint32_t site,
                                   const uint32_t* key);

/* Single-token decode step against a KV cache.  The reference has no cache: it re-runs the
 * whole window for every sampled token (generate_images.py:283-307,
 * train_quantized_transformer.py:600-640); this computes the same attention row
 * (models/layers.py:433-474 for the last query) from cached keys/values.  q,k_new,v_new,o
 * (B,H*d); cache row j of sequence n at n*batch_stride + j*H*d.  k_new/v_new non-NULL:
 * stored at row len and attended as the last key; NULL: read-only cache (cross-attention).
 * len_dev (device int, optional) overrides len for graph replay.  o_mul (B,H*d), optional:
 * multiplies the output (ResidualLinearLayer's x * scale(cond), models/layers.py:293-295).
 * Cache rows at or beyond the attended length are never used, whatever they hold (NaN included),
 * the stale row `len` of an append among them: a cache need not be cleared between uses.  A host
 * len outside the cache is refused; *len_dev is clamped instead, to [0, max_len - 1] when appending
 * (the new row goes to the clamped row) and to [0, max_len] when read-only, and nothing outside the
 * max_len rows is read or written.  A read-only *len_dev <= 0 attends no key: o is not defined. */
int qarig_attention_decode(const float* q, const float* k_new, const float* v_new, float* kcache,
                           float* vcache, int B, int H, int d, int len, const int* len_dev,
                           int max_len, int64_t batch_stride, float sqrt_d, const float* o_mul,
                           float* o, void* stream);

/* Cross-entropy, mean over rows, fused with d/dlogits: one rows launch and one mean launch (csrc/loss.hip).
 * qarig_cross_entropy_fused_fwd states the whole contract; the four entries behind it are its special cases, kept
 * with their signatures, and every one of them writes the bits the superset writes for the same numbers.
 *
 * logits fp32, rows at ld_logits >= C (columns C .. ld_logits - 1 are never read); target int64 (M).  With all three
 * numbers 0: nn.CrossEntropyLoss() as the reference trains with (train_quantized_transformer.py:337,496-502).
 * Otherwise (additive; the reference trains with none of them) F.cross_entropy(logits, target, label_smoothing = eps)
 * + zeta mean_r(logsumexp(logits[r])^2), and SOM-neighbour soft targets.  Per row, mx = max x, s = sum exp(x - mx),
 * logs = log s, lse = mx + logs, p[c] = exp((x[c] - mx) - logs):
 *   nll = logs - (x[t] - mx),  u = logs - (1 / C) sum_c (x[c] - mx),  obj = (1 - eps) nll + eps u + zeta lse^2,
 *   d obj / d x[c] = p[c] (1 + 2 zeta lse) - (1 - eps) [c == t] - eps / C.
 * Soft targets: the codebooks are one-dimensional self-organising maps, code t +- 1 decodes to almost the patch of
 * code t, and part of the smoothing mass goes there.  The leading `codes` classes lie on the SOM axis; classes
 * codes .. C - 1 are special (<end>) and are nobody's neighbour.  For a row with target t < codes, with w = weights
 * (DEVICE, range + 1 floats of the index distance, weights[0] = 1) and nu = neighbour_smoothing:
 *   lo = max(0, t - range), hi = min(codes - 1, t + range),  q[j] = w[|j - t|] / sum_{i = lo .. hi} w[|i - t|]
 *   h = logs - sum_j q[j] (x[j] - mx)            (cross-entropy against q, from the shifted logits as u is)
 *   obj = (1 - eps - nu) nll + eps u + nu h + zeta lse^2
 *   d obj / d x[c] = p[c] (1 + 2 zeta lse) - (1 - eps - nu) [c == t] - eps / C - nu q[c]
 * -- the window is clamped at the ends of the axis and renormalised.  A row whose target is special takes nu = 0: the
 * objective and gradient at neighbour_smoothing = 0, bit for bit.  A table entry of exactly 0 takes its column out of
 * the window.
 * Accepted: M, C positive, at most 2^24 each, product at most 2^40; C <= ld_logits <= 2^31, and with dlogits
 * C <= ld_dlogits <= 2^31; label_smoothing in [0, 1); z_loss finite and >= 0; neighbour_smoothing in [0, 1);
 * label_smoothing + neighbour_smoothing < 1 (as fp32); 0 < codes <= C; with neighbour_smoothing > 0: 1 <= range <= 31
 * and weights non-NULL (at neighbour_smoothing = 0 range and weights are not looked at).  Anything else is refused
 * before a launch.
 * loss: 2 floats = {mean obj, mean plain nll}.  row_ws: 2 M floats, the row objectives then the row nlls.  dlogits:
 * NULL, or rows at ld_dlogits = d(mean obj)/d(logits), columns C .. ld_dlogits - 1 written as exact +0 (the
 * classifier's logits stay in their (M, 528) GEMM output buffer and the input-gradient GEMM reduces over the zero
 * columns); nothing behind row M - 1's ld_dlogits columns is written; NULL leaves the losses bit for bit.
 * A term whose coefficient is 0 is not evaluated: with all three 0 both losses are the plain mean loss and both halves
 * of row_ws its row losses, and label_smoothing = 0 never forms 0 * inf on rows with -inf entries.  With
 * label_smoothing > 0 such a row's objective, and loss[0], are +inf as torch's are; its nll and its gradient stay
 * finite, the -inf columns getting (-eps / C) / M.  A window column holding -inf makes the row objective +inf (as u
 * does); its gradient element is the finite (-eps / C - nu q[c]) / M.  A target outside [0,C) sets *bad_flag and its
 * row adds 0 to both means.  A row's outputs depend on that row alone (no floating-point atomics, one fixed summation
 * order, 4-byte loads at every alignment); a row holding NaN is undefined in that row alone. */
int qarig_cross_entropy_fused_fwd(const float* logits, int64_t ld_logits, const int64_t* target, int M, int C,
                                  int codes, float label_smoothing, float z_loss, float neighbour_smoothing, int range,
                                  const float* weights, float* loss, float* dlogits, int64_t ld_dlogits, float* row_ws,
                                  int* bad_flag, void* stream);
/* The superset at (0, 0, 0) on dense rows, with the plain ABI: loss 1 float (the mean loss), row_ws M floats (the row
 * losses); neither the second loss nor a second half of row_ws is written. */
int qarig_cross_entropy_fwd(const float* logits, const int64_t* target, int M, int C, float* loss,
                            float* dlogits, float* row_ws, int* bad_flag, void* stream);
/* The same with the superset's leading dimensions; qarig_cross_entropy_fwd is its ld == C case. */
int qarig_cross_entropy_ld_fwd(const float* logits, int64_t ld_logits, const int64_t* target, int M, int C,
                               float* loss, float* dlogits, int64_t ld_dlogits, float* row_ws, int* bad_flag,
                               void* stream);
/* The superset on dense rows (ld = C) at neighbour_smoothing = 0: label smoothing and z-loss. */
int qarig_cross_entropy_reg_fwd(const float* logits, const int64_t* target, int M, int C, float label_smoothing,
                                float z_loss, float* loss, float* dlogits, float* row_ws, int* bad_flag,
                                void* stream);
/* The superset on dense rows (ld = C). */
int qarig_cross_entropy_soft_fwd(const float* logits, const int64_t* target, int M, int C, int codes,
                                 float label_smoothing, float z_loss, float neighbour_smoothing, int range,
                                 const float* weights, float* loss, float* dlogits, float* row_ws, int* bad_flag,
                                 void* stream);

/* Held-out evaluation (additive; the reference has none), csrc/score.hip.
 * qarig_token_score: logits (M,C) fp32 contiguous, target int64 (M).  Per row, in the shifted form of the
 * cross-entropy kernel: row_nll = log sum_c exp(x[c] - max) - (x[t] - max) (nats) and
 * row_rank = #{c : x[c] > x[t]} + #{c < t : x[c] == x[t]} -- 0: the target is the arg-max, ties go to the
 * smaller index.  A row whose target equals ignore_index gives (0, -1); any other target outside [0,C) gives
 * (0, -1) and sets *bad_flag.  A row holding NaN or +-inf is undefined in that row alone.
 * qarig_score_reduce: rows r = n S + s of one scored batch, column s at absolute position pos0 + s < P, ADDED
 * into accumulators the caller zeroed once: img_nll (N) += sum_s row_nll, pos_nll (P)[pos0 + s] += sum_n
 * row_nll (both fp64), pos_cnt (P)[pos0 + s] += #{n : rank >= 0}, totals (3) += {rows with rank >= 0, with
 * rank == 0, with 0 <= rank < topk} (int64).  Every output element belongs to one wave, the fp64 sums run in
 * one fixed order and nothing is added atomically: equal inputs give equal bits.  N S < 2^31. */
int qarig_token_score(const float* logits, const int64_t* target, int M, int C, int64_t ignore_index,
                      float* row_nll, int* row_rank, int* bad_flag, void* stream);
int qarig_score_reduce(const float* row_nll, const int* row_rank, int N, int S, int pos0, int P, int topk,
                       double* img_nll, double* pos_nll, int64_t* pos_cnt, int64_t* totals, void* stream);

/* Reconstruction evaluation (additive; the reference has none), csrc/recon.hip.  Both entries write their
 * outputs (they do not add), use no floating-point atomics and sum in one fixed order, so equal inputs give
 * equal bits; every partial sum belongs to one image, so an image's value does not depend on which other
 * images share its launch.  NaN or +-inf in an image stays in that image's outputs.
 * qarig_pair_error: a, b = N contiguous images of E fp32 elements, base pointers 4-byte aligned (16-byte loads
 * where an image's address allows them, 4-byte loads otherwise: the same values in the same order either way).
 * out (N,3) fp64 = {sum (a-b)^2, sum |a-b|, max |a-b|} per image; differences, squares and sums in fp64.  One
 * workgroup per 4,096-element chunk of an image writes a partial triple to ws, one wave per image adds the
 * chunk partials in ascending order.  ws: qarig_pair_error_workspace_bytes(N, E) bytes (0: bad extents).
 * qarig_ssim: a, b (N,C,H,W) fp32 contiguous; out (N) fp64 = mean structural similarity (Wang et al. 2004) per
 * image, per channel, over the (H - taps + 1) x (W - taps + 1) "valid" positions only.  The window is separable
 * with 1-D weights win, a HOST array of `taps` doubles (taps odd, 1 ... 15) that reaches the kernel by value.
 * With w over the window: mx = sum w x, sx2 = sum w x^2 - mx^2, sxy = sum w x y - mx my,
 * map = (2 mx my + c1)(2 sxy + c2) / ((mx^2 + my^2 + c1)(sx2 + sy2 + c2)).  The five window moments are
 * accumulated in fp64 from the fp32 pixels (sum w x^2 - mx^2 cancels almost completely on smooth regions, where
 * c2 decides the score).  H < taps or W < taps is an argument error.  One workgroup per (image, channel,
 * 16 x 16 tile of outputs) writes a partial to ws, one wave per image adds them in ascending (channel, tile)
 * order.  ws: qarig_ssim_workspace_bytes(N, C, H, W, taps) bytes (0: bad arguments). */
size_t qarig_pair_error_workspace_bytes(int N, int64_t E);
int qarig_pair_error(const float* a, const float* b, int N, int64_t E, double* out, void* ws, size_t ws_bytes,
                     void* stream);
size_t qarig_ssim_workspace_bytes(int N, int C, int H, int W, int taps);
int qarig_ssim(const float* a, const float* b, int N, int C, int H, int W, const double* win, int taps, double c1,
               double c2, double* out, void* ws, size_t ws_bytes, void* stream);

/* Training against SSIM (additive), csrc/recon.hip.  With x = a (the prediction), y = b (data) and, per valid
 * position, A1 = 2 mx my + c1, A2 = 2 sxy + c2, B1 = mx^2 + my^2 + c1, B2 = sx2 + sy2 + c2, v = A1 A2 / (B1 B2):
 *   P = dv/dmx = 2 my (A2 - A1) / (B1 B2) - 2 mx v (1/B1 - 1/B2),  Q = dv/d(sum w x^2) = -v / B2,
 *   R = dv/d(sum w x y) = 2 A1 / (B1 B2).
 * qarig_ssim_fwd_maps: qarig_ssim (out bit-identical, same ws) that also writes maps (3,N,C,oh,ow) fp64 =
 * {P, Q, R}, oh = H - taps + 1, ow = W - taps + 1; qarig_ssim_maps_bytes gives its size (0: bad arguments).
 * qarig_ssim_bwd: da (N,C,H,W) fp32, written in full (not added to) =
 *   da(q) = g[n] / (C oh ow) * sum_ij w_i w_j [P + 2 a(q) Q + b(q) R](q - (i,j))   over the valid q - (i,j),
 * the gradient of sum_n g[n] out[n] with respect to a; g (N) fp64 on the device, win and taps as in the forward
 * (a HOST array, applied in correlation order: no symmetry assumed).  One workgroup per (image, channel, 16 x 16
 * tile of input pixels), the maps' halo and a horizontal pass in LDS, fp64 fma throughout, one rounding to fp32;
 * no atomics, every pixel written by one thread, image n's gradient a function of image n and g[n] alone.  Maps
 * and moments stay fp64: the terms of da(q) cancel to 1e-4 of their magnitude sum.  Both entries check their
 * arguments as qarig_ssim does, with N C ceil(H/16) ceil(W/16) < 2^31, and refuse outputs that alias inputs. */
size_t qarig_ssim_maps_bytes(int N, int C, int H, int W, int taps);
int qarig_ssim_fwd_maps(const float* a, const float* b, int N, int C, int H, int W, const double* win, int taps,
                        double c1, double c2, double* out, double* maps, void* ws, size_t ws_bytes, void* stream);
int qarig_ssim_bwd(const float* a, const float* b, const double* maps, const double* g, int N, int C, int H, int W,
                   const double* win, int taps, float* da, void* stream);

/* Generation evaluation (additive; the reference has none), csrc/moments.hip: the features and moments behind a
 * Frechet distance between two sample sets in latent space (qarig/gen_eval.py).  No floating-point atomics, one
 * fixed summation order: equal inputs and an equal call sequence give equal bits.
 * qarig_pool_features: z (N,C,H,W) fp32 contiguous; f (N, D) fp64, D = C (H/P) (W/P), written in full.  Feature
 * (c, i, j) of a sample is the mean of its P x P block: the block summed in fp64 in raster order, divided by P^2
 * once (P = 1: a conversion).  Refused: P not dividing H and W, D outside 1 ... 1024, null pointers, N < 1, f
 * overlapping z.
 * qarig_moments_add: f (n, D) fp64 with ld = D; shift (D) fp64, NULL = zeros.  With a_r = f_r - shift (fp64), ADDED
 * into accumulators the caller zeroed once: count (int64) += n, sum (D) += sum_r a_r, gram (D,D) row-major
 * (i, j) += sum_r a_ri a_rj for every (i, j) with floor(j/16) >= floor(i/16) -- the upper triangle of 16 x 16
 * tiles, diagonal tiles whole; every other element of gram keeps its bits (the host mirrors the result).  The
 * products run on v_mfma_f64_16x16x4_f64, rows in ascending steps of four; each tile belongs to one wave, which
 * loads it, accumulates and stores it.  A NaN feature stays in its row and column of gram.  Refused: D outside
 * 1 ... 1024, n outside 1 ... 2^20, null f / count / sum / gram, accumulators that alias f. */
int qarig_pool_features(const float* z, int N, int C, int H, int W, int P, double* f, void* stream);
int qarig_moments_add(const double* f, int n, int D, const double* shift, int64_t* count, double* sum, double* gram,
                      void* stream);

/* Generation evaluation, k-nearest-neighbour statistics (additive; the reference has none), csrc/knn.hip: the two
 * primitives behind precision / recall, density / coverage and nearest-real-neighbour distances (qarig/gen_eval.py
 * manifold_metrics, nearest_real).  q (nq, D) and x (nx, D) fp64 with ld = D; shift (D) fp64, NULL = zeros.  With
 * a_i = q_i - shift and b_j = x_j - shift (fp64),
 *   d2(i, j) = (|a_i|^2 + |b_j|^2) - 2 sum_c a_ic b_jc:
 * the inner product on v_mfma_f64_16x16x4_f64, the feature index ascending in steps of four from a zero
 * accumulator, operands zero past D after the subtraction; |.|^2 in one order that depends on D alone (lane l of a
 * wave sums the features l, l + 64, ... ascending, then a butterfly).  d2 is a function of the unordered pair of rows
 * and the shift: its bits do not depend on which row is the query, on a row's position, on the tile or on how the
 * queries are split over calls; both entries take it from one device function.  |got - exact| <=
 * (D + 8) 2^-53 (|a_i|^2 + |b_j|^2 + 2 sum_c |a_ic| |b_jc|): choose the shift near the data.  No floating-point
 * atomics; equal inputs give equal bits.
 * qarig_knn_smallest: for every query row the k smallest d2 over the rows of x, ascending, into d2_out (nq, k) with
 * their x indices in idx_out (nq, k).  Order by (value, index): equal values go to the lower index.  self_offset >= 0:
 * query i IS x row self_offset + i, and that one row is no candidate -- by index, never by value (a duplicate at
 * distance 0 is a neighbour); -1: no row is excluded.  Comparisons are ordinary < on doubles: a NaN distance never
 * enters a list; slots no candidate qualified for hold +inf and index -1.
 * qarig_ball_count: count_out[i] = the number of x rows j (row self_offset + i excluded when self_offset >= 0) with
 * d2(i, j) <= r2[j], r2 (nx) fp64: the radius belongs to the x row.  NaN is never inside.
 * Both need a workspace of qarig_knn_workspace_bytes(nq, nx, D, k) bytes (the norms and, where the x axis is split
 * over workgroups, per-split partial lists; 0: bad extents; ball_count: any k).  Refused: D outside 1 ... 1024, nq or
 * nx outside 1 ... 2^20, k outside 1 ... 8, self_offset neither -1 nor in 0 ... nx - nq, fewer than k candidates
 * (nx - (self_offset >= 0) < k), null pointers (shift excepted), outputs or the workspace overlapping an input, a
 * workspace that is too small (QARIG_ERR_WORKSPACE). */
size_t qarig_knn_workspace_bytes(int nq, int nx, int D, int k);
int qarig_knn_smallest(const double* q, int nq, const double* x, int nx, int D, const double* shift, int k,
                       int self_offset, double* d2_out, int* idx_out, void* ws, size_t ws_bytes, void* stream);
int qarig_ball_count(const double* q, int nq, const double* x, int nx, int D, const double* shift, const double* r2,
                     int self_offset, int* count_out, void* ws, size_t ws_bytes, void* stream);

/* F.mse_loss (mean) + d/dpred -- train_autoencoder.py:215-217, train_codebook.py:233-235. */
size_t qarig_mse_workspace_bytes(void);
int qarig_mse_fwd(const float* pred, const float* target, int64_t n, float* loss, float* dpred,
                  float* part_ws, void* stream);

/* torch.optim.Adam step on a flat buffer -- train_quantized_transformer.py:317-320.
 * dev_step (optional device float[2] = {lr / (1 - beta1^t), sqrt(1 - beta2^t)}) overrides the two
 * per-step scalars (graph replay).  shadow_bf16 (optional, n x 2 bytes): the updated parameters rounded to
 * bf16 from the same pass (the reduced-precision GEMMs' weight operands). */
int qarig_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float beta1,
                    float beta2, float eps, float step_size, float bc2_sqrt, float grad_scale,
                    const float* dev_step, void* shadow_bf16, void* stream);

/* The same step, with an exponential moving average of the parameters kept by the same launch (additive: the
 * reference has none): ema (n floats, in place) <- lerp(ema, p_new, ema_w) in the two-branch form of exp_avg,
 * so ema_w = 1 copies p_new, ema_w = 0 leaves ema alone and ema == p_new stays, all exactly.  dev_step
 * (optional) is a device float[3] here, {step_size, bc2_sqrt, ema_w}.  p, m, v and shadow_bf16 come out
 * bit-identical to qarig_adam_step on the same inputs. */
int qarig_adam_ema_step(float* p, const float* g, float* m, float* v, float* ema, int64_t n, float beta1,
                        float beta2, float eps, float step_size, float bc2_sqrt, float ema_w,
                        float grad_scale, const float* dev_step, void* shadow_bf16, void* stream);

/* AdamW: the same step behind a decoupled weight decay (additive: the reference trains without), as
 * torch.optim.AdamW with a decayed and an undecayed group, from one launch.  Normative, per element i:
 *   decay_mask[i >> 3] != 0:  pd = fmaf(-decay, p[i], p[i])    one rounding; decay = fp32(lr * lambda), the
 *                             product taken in double on the host and rounded once.  (Not p * fp32(1 - lr lambda):
 *                             below 1 fp32 steps by 2^-24, so at lr lambda = 1e-6 that factor is 1 - 17 x 2^-24, a
 *                             decay 1.3 % off, and the error grows without bound as lr lambda falls to 2^-25.)
 *   decay_mask[i >> 3] == 0:  pd = p[i], its bits untouched.
 *   then qarig_adam_step's expressions with pd in the place of p[i]:
 *     gi = g[i] * grad_scale;  w = 1 - beta1;  mn = w < 0.5 ? m + w (gi - m) : gi - (gi - m)(1 - w);
 *     vn = v beta2 + (1 - beta2) gi gi;  denom = sqrtf(vn) / bc2_sqrt + eps;  pn = pd - step_size (mn / denom);
 *     ema (when given) <- the two-branch lerp of ema towards pn by ema_w;  shadow_bf16 (when given) <- the
 *     nearest-even bf16 of pn.
 * decay_mask: ceil(n / 8) bytes on the device, one per group of 8 consecutive elements (FlatAdam's slices start
 * on multiples of 8 floats, so a group never spans two parameters).  ema may be NULL.  dev_step (optional) is
 * ALWAYS a device float[4] here, {step_size, bc2_sqrt, ema_w, decay}, and overrides the four host values (ema_w
 * is ignored without ema).  One thread-iteration moves one group with 16-byte accesses; the last group of an n
 * that is no multiple of 8 goes element by element and nothing at or behind n is written.  With a mask of zeros
 * p, m, v, ema and shadow_bf16 come out bit-identical to qarig_adam_step / qarig_adam_ema_step.
 * Refused (-1) without a launch: null p, g, m, v or decay_mask; n outside [1, 2^40]; p, g, m, v, ema or
 * shadow_bf16 not 16-byte aligned; a host decay outside [0, 1) or NaN; ema or shadow_bf16 overlapping p. */
int qarig_adamw_step(float* p, const float* g, float* m, float* v, float* ema, const unsigned char* decay_mask,
                     int64_t n, float beta1, float beta2, float eps, float step_size, float bc2_sqrt,
                     float ema_w, float decay, float grad_scale, const float* dev_step, void* shadow_bf16,
                     void* stream);

/* Global-norm gradient clipping with a guard for non-finite gradients (additive: the reference trains without),
 * torch.nn.utils.clip_grad_norm_'s rule on one flat buffer, decided and applied on the device.
 *
 * qarig_grad_clip_coef -- two launches.  Normative:
 *   s_i  = fp32(g[i] * grad_scale)                  the value the Adam entries use, one fp32 rounding
 *   sum  = sum_i (double)s_i * (double)s_i          every product exact (48 bits in 53), accumulated in fp64
 *   norm = sqrt(sum)                                fp64; cannot overflow (2^40 squares of fp32 values < 1e90)
 *   coef = fp32(min(1, max_norm / (norm + 1e-6)))   evaluated in double, rounded once; max_norm = +inf gives 1
 *   norm not finite (<=> some s_i is not finite):   coef = 0 and the step counts as skipped
 * Summation order (fixed: the same data give the same bits on every call and every rank).  Stage 1 runs
 * B = min(ceil(n / 1024), QARIG_GRAD_NORM_PARTIALS) workgroups of 256 threads.  Lane l of workgroup b owns the
 * 16-byte vectors j = 256 b + l + 256 B t, t = 0, 1, ...; it adds their elements to ONE fp64 accumulator, trips
 * ascending, the four elements of a vector in index order (four trips' loads are in flight before the first
 * use).  The lane whose sequence reaches j = floor(n / 4) then adds the n % 4 tail elements in order; nothing at
 * or behind n is read.  A wave adds its 64 accumulators by the xor butterfly with offsets 32, 16, 8, 4, 2, 1 (x
 * <- x + x[lane ^ o]); the workgroup adds its four wave sums as ((w0 + w1) + w2) + w3 and stores partials[b] (a
 * vector store).  Stage 2, one workgroup: thread t adds partials[t], partials[t + 256], ... ascending, then the
 * same butterfly and wave order.
 * state: FOUR doubles that live across steps.  The call writes state[0] = norm and state[1] = coef, adds 1 to
 * state[2] (steps skipped so far) when norm is not finite, and adds 1 to state[3] (steps clipped so far) when
 * norm is finite and coef < 1.  The caller zeroes state once.  partials: QARIG_GRAD_NORM_PARTIALS doubles of
 * scratch (the first B are written).  No atomics.
 * Refused (-1) without a launch: null g, partials or state; n outside [1, 2^40]; g not 16-byte aligned
 * (partials, state: 8-byte); max_norm not > 0, or NaN; grad_scale not finite.
 *
 * qarig_adam_clip_step -- qarig_adamw_step's arguments plus clip_state (the four doubles above, read only).
 * Every thread first reads clip_state[0] and clip_state[1].  If clip_state[0] is not finite the kernel returns at
 * once: p, m, v, ema and shadow_bf16 keep their bits (the step is skipped).  Otherwise, per element,
 *   gi = fp32(fp32(g[i] * grad_scale) * coef),  coef = fp32(clip_state[1])       two roundings, no contraction
 * and the rest is qarig_adamw_step's arithmetic with this gi.  decay_mask may be NULL (no element is decayed and
 * the host decay is not looked at); ema may be NULL; dev_step (optional) is ALWAYS a device float[4], {step_size,
 * bc2_sqrt, ema_w, decay}.  At coef == 1 every output is bit-identical to qarig_adam_step / qarig_adam_ema_step
 * (no mask) or qarig_adamw_step (mask) on the same inputs.  Refused (-1) without a launch: as qarig_adamw_step
 * (a null decay_mask excepted), plus a null or misaligned clip_state. */
#define QARIG_GRAD_NORM_PARTIALS 2048
int qarig_grad_clip_coef(const float* g, int64_t n, float grad_scale, double max_norm, double* partials,
                         double* state, void* stream);
int qarig_adam_clip_step(float* p, const float* g, float* m, float* v, float* ema, const unsigned char* decay_mask,
                         int64_t n, float beta1, float beta2, float eps, float step_size, float bc2_sqrt,
                         float ema_w, float decay, float grad_scale, const float* dev_step, void* shadow_bf16,
                         const double* clip_state, void* stream);

/* Exchanges two fp32 buffers of n elements in place, bit for bit (NaN payloads included): 16-byte accesses
 * where both buffers are 16-byte aligned, with a scalar tail; scalar throughout otherwise.  The buffers must
 * not overlap; null pointers, n <= 0 and overlapping ranges are refused (-1) without a launch. */
int qarig_swap_f32(float* a, float* b, int64_t n, void* stream);

/* elementwise helpers (ResidualLinearLayer gate, models/layers.py:293-295) */
int qarig_mul_fwd(const float* a, const float* b, float* y, int64_t n, void* stream);
int qarig_mul_bwd(const float* dy, const float* a, const float* b, float* da, float* db, int64_t n,
                  void* stream);
int qarig_act_fwd(const float* x, float* y, int64_t n, int act, void* stream);
int qarig_act_bwd(const float* dy, const float* z, float* dz, int64_t n, int act, void* stream);
int qarig_scale_by(const float* x, const float* s, float* y, int64_t n, void* stream);

/* Counter-based dropout (additive: the reference has none).  y[e] = x[e] * scale where element e is kept, +0.0
 * where it is dropped (a dropped NaN or inf becomes 0), e the flat index into n contiguous fp32 elements.  The
 * keep-bit is a pure function of (seed, rank, step, site, e): Philox4x32-10 (multipliers D2511F53 / CD9E8D57,
 * Weyl constants 9E3779B9 / BB67AE85) with key (seed_lo, seed_hi) and counter (e >> 3, site, step, rank); of the
 * call's four words element e reads word (e & 7) >> 1, its low 16 bits when e is even and its high 16 bits when
 * odd, and is kept iff that value >= threshold.  The drop rate is threshold / 65536 and the caller passes
 * scale = 65536 / (65536 - threshold) rounded to fp32 once.  key: DEVICE uint32[4] {seed_lo, seed_hi, step,
 * rank}, read by the kernel (a replayed graph sees the step its host wrote last).  Backward is the same call
 * on dy.  16-byte accesses where x and y are both 16-byte aligned, element by element otherwise and in the
 * tail; the mask never depends on the path.  y may be x; any other overlap, null pointers, n outside
 * [1, 2^34] and threshold outside [1, 58982] (p <= 0.9) are refused (-1) without a launch. */
int qarig_dropout(const float* x, float* y, int64_t n, uint32_t threshold, float scale, uint32_t site,
                  const uint32_t* key, void* stream);

/* ---- Conv autoencoder ----------------------------------------------------------- */

/* nn.Conv2d(k<=4, stride, padding) + bias + activation, NCHW -- ConvLayer /
 * DownsampleConvLayer, models/layers.py:157-184, 211-230 (3x3, stride 1|2, pad 1 in the
 * reference).  x (N,Cin,H,W); w (Cout,Cin,k,k); y (N,Cout,Ho,Wo); preact (optional,
 * same shape as y) receives the pre-activation. */
int qarig_conv2d_fwd(const float* x, int N, int Cin, int H, int W, const float* w,
                     const float* bias, int Cout, int k, int stride, int pad, int act, float* y,
                     float* preact, void* stream);
/* The same with a scratch buffer for a tap-major copy of the weights: the 3x3 / stride 1 / padding 1
 * layers whose tiles are whole (Cin % 16, Cout % 128, N*H*W % 128, W % 4 == 0, input < 2 GB) then run on
 * the LDS-DMA ring kernel; every other geometry takes the path of qarig_conv2d_fwd.  Results differ
 * by the summation order only (tap-major instead of channel-major). */
size_t qarig_conv2d_fwd_workspace_bytes(int Cin, int Cout, int k);
/* ... plus, at few images (generate_images.py:366 decodes the 1-8 images just sampled), room for the
 * partial sums of a launch whose reduction is split 2-8 ways because its tiles alone would leave CUs
 * idle (<= 256 workgroups): given this much scratch the call splits, given only the size above it
 * does not.  The split changes the summation order (parts added in order after the k-loop).
 * This and the three other *_workspace_bytes_n functions below answer from the plan that drives the launch
 * itself (csrc/conv.hip conv_ring_plan), with padding 1 and aligned pointers assumed: slabs are counted exactly
 * for the geometries whose launch takes the ring kernel and splits, and a geometry the launch keeps off the ring
 * (grid rows not a multiple of 4 wide, an input of 2 GB or more, option conv_ring = 0, ...) gets the size above. */
size_t qarig_conv2d_fwd_workspace_bytes_n(int N, int Cin, int H, int W, int Cout, int k, int stride);
/* flags: QARIG_CONV_PACKED_VALID = the head of `workspace` still holds the re-ordered weights an earlier
 * call with the same w, geometry and workspace wrote there (inference: the weights do not change between
 * calls) -- the re-ordering launch is skipped.  0 otherwise. */
#define QARIG_CONV_PACKED_VALID 1
int qarig_conv2d_fwd_ws(const float* x, int N, int Cin, int H, int W, const float* w,
                        const float* bias, int Cout, int k, int stride, int pad, int act, float* y,
                        float* preact, void* workspace, size_t ws_bytes, int flags, void* stream);

/* nn.ConvTranspose2d(4, stride 2, padding 1) + bias + activation -- UpsampleConvLayer,
 * models/layers.py:188-207.  x (N,Cin,H,W); w (Cin,Cout,4,4); y (N,Cout,2H,2W). */
size_t qarig_conv_transpose2d_workspace_bytes(int Cin, int Cout);
/* the same plus the split launch's slabs at few images (see qarig_conv2d_fwd_workspace_bytes_n) */
size_t qarig_conv_transpose2d_workspace_bytes_n(int N, int Cin, int H, int W, int Cout);
int qarig_conv_transpose2d_fwd(const float* x, int N, int Cin, int H, int W, const float* w,
                               const float* bias, int Cout, int act, float* y, float* preact,
                               void* workspace, size_t ws_bytes, int flags, void* stream);

/* autograd of the conv layers (dT = dy * act'(preact), via qarig_act_bwd, first) */
size_t qarig_conv2d_bwd_data_workspace_bytes(int Cin, int Cout, int k);
/* ... plus room for the split slabs of a few-image launch (3x3 / stride 1; the stride-2 input gradient is never
 * split; see qarig_conv2d_fwd_workspace_bytes_n) */
size_t qarig_conv2d_bwd_data_workspace_bytes_n(int N, int Cin, int H, int W, int Cout, int k, int stride);
/* qarig_conv2d_bwd_data accepts k 1..4, stride 1..2 and 0 <= pad < k (anything else: QARIG_ERR_ARG,
 * "conv2d_bwd_data: unsupported geometry", nothing launched) and writes every element of dx: input positions
 * that no output window reads (rows and columns past the last window, the odd positions of a 1x1 / stride-2
 * layer) receive zero. */
int qarig_conv2d_bwd_data(const float* dT, int N, int Cout, int Ho, int Wo, const float* w, int Cin,
                          int k, int stride, int pad, int H, int W, float* dx, void* workspace,
                          size_t ws_bytes, void* stream);
int qarig_conv_transpose2d_bwd_data(const float* dT, int N, int Cout, int H, int W, const float* w,
                                    int Cin, float* dx, void* stream);
/* ... with a scratch buffer (16 * Cin * Cout floats) for tap-major weights: whole-tile layers on the strided ring
 * kernel, every other geometry as above. */
/* scratch of the _ws form: the tap-major weights (qarig_conv_transpose2d_workspace_bytes) + the split slabs of a
 * few-image launch */
size_t qarig_conv_transpose2d_bwd_data_workspace_bytes_n(int N, int Cin, int H, int W, int Cout);
int qarig_conv_transpose2d_bwd_data_ws(const float* dT, int N, int Cout, int H, int W, const float* w,
                                       int Cin, float* dx, void* workspace, size_t ws_bytes, void* stream);
/* G (N,Cg,Gh,Gw) correlated with im2col_{k,stride,pad}(X (N,Cx,H,W)) -> dw (Cg, Cx*k*k).
 * Conv2d: G=dT, X=input.  ConvTranspose2d(4,2,1): G=input, X=dT, k=4, stride=2, pad=1. */
size_t qarig_conv_wgrad_workspace_bytes(int Cg, int K2, int P);
int qarig_conv_wgrad(const float* G, int N, int Cg, int Gh, int Gw, const float* X, int Cx, int H,
                     int W, int k, int stride, int pad, float* dw, void* workspace, size_t ws_bytes,
                     void* stream);
int qarig_conv_bias_grad(const float* G, int N, int C, int HW, float* db, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* QARIG_H */
