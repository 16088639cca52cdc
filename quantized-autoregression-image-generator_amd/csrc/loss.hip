// Cross-entropy (mean over rows) forward fused with its gradient w.r.t. the logits:
// nn.CrossEntropyLoss() as the reference trains with
// (train_quantized_transformer.py:337,496-502).  One wave per row.
#include "qarig_common.h"

namespace qarig {

__global__ __launch_bounds__(256) void ce_rows_kernel(const float* __restrict__ logits,
                                                      int64_t ld_logits,
                                                      const int64_t* __restrict__ target, int M,
                                                      int C, float inv_m,
                                                      float* __restrict__ row_loss,
                                                      float* __restrict__ dlogits, int64_t ld_dlogits,
                                                      int* __restrict__ bad) {
    // rows at leading dimensions ld_logits / ld_dlogits >= C: columns C .. ld_logits - 1 of the logits are never
    // read, columns C .. ld_dlogits - 1 of the gradient receive exact zeros (a GEMM reduces over them)
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const float* x = logits + (int64_t)row * ld_logits;
    float mx = -INFINITY;
    for (int c = lane; c < C; c += 64) mx = fmaxf(mx, x[c]);
    mx = wave_max(mx);
    float s = 0.0f;
    for (int c = lane; c < C; c += 64) s += expf(x[c] - mx);
    s = wave_sum(s);
    // log s - (x[t] - mx) and exp((x - mx) - log s): every rounding happens at the magnitude of the loss, not of
    // the logits (mx + log s first costs ulp(|mx|) -- 6e-5 at logits near 1000)
    const float logs = logf(s);
    const int64_t t = target[row];
    const bool ok = t >= 0 && t < C;
    if (lane == 0) {
        if (!ok) atomicExch(bad, 1);
        row_loss[row] = ok ? logs - (x[t] - mx) : 0.0f;
    }
    if (dlogits) {
        float* d = dlogits + (int64_t)row * ld_dlogits;
        for (int c = lane; c < C; c += 64) {
            const float p = expf((x[c] - mx) - logs);
            d[c] = (p - ((int64_t)c == t ? 1.0f : 0.0f)) * inv_m;
        }
        for (int64_t c = C + lane; c < ld_dlogits; c += 64) d[c] = 0.0f;
    }
}

// mean of row_loss[M], fixed order: 256 strided partial sums, then a tree.
__global__ __launch_bounds__(256) void mean_kernel(const float* __restrict__ v, int M, float inv_m,
                                                   float* __restrict__ out) {
    __shared__ float red[256];
    float s = 0.0f;
    for (int i = threadIdx.x; i < M; i += 256) s += v[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = red[0] * inv_m;
}

// F.mse_loss(pred, target) (mean) and d/dpred = 2 (pred - target) / n, fixed-order sum.  The gradient is the
// product with inv_n = 1 / n corrected by one Newton step (nf = (float)n): the quotient to within one rounding, so
// two roundings (a - b, the quotient) and 2 u of the exact value; the bare product would add the rounding of 1 / n.
__global__ __launch_bounds__(256) void mse_partial_kernel(const float* __restrict__ a,
                                                          const float* __restrict__ b, int64_t n,
                                                          float inv_n, float nf, float* __restrict__ part,
                                                          float* __restrict__ da) {
    __shared__ float red[256];
    float s = 0.0f;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float d = a[i] - b[i];
        s = fmaf(d, d, s);
        if (da) {
            const float t = 2.0f * d, q = t * inv_n;
            da[i] = fmaf(fmaf(-q, nf, t), inv_n, q);
        }
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}

}  // namespace qarig

using namespace qarig;

constexpr int MSE_BLOCKS = 1024;

extern "C" size_t qarig_mse_workspace_bytes(void) { return MSE_BLOCKS * sizeof(float); }

// F.mse_loss (train_autoencoder.py:215-217, train_codebook.py:233-235): loss (1 float),
// dpred (n floats or NULL).  part_ws: qarig_mse_workspace_bytes().
extern "C" int qarig_mse_fwd(const float* pred, const float* target, int64_t n, float* loss,
                             float* dpred, float* part_ws, void* stream) {
    QARIG_CHECK_ARG(pred && target && loss && part_ws && n > 0 && n <= (1LL << 40), "mse: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    const float inv_n = 1.0f / (float)n;
    hipLaunchKernelGGL(mse_partial_kernel, dim3(MSE_BLOCKS), dim3(256), 0, st, pred, target, n,
                       inv_n, (float)n, part_ws, dpred);
    QARIG_CHECK_LAUNCH("mse partial");
    hipLaunchKernelGGL(mean_kernel, dim3(1), dim3(256), 0, st, part_ws, MSE_BLOCKS, inv_n, loss);
    QARIG_CHECK_LAUNCH("mse mean");
    return QARIG_OK;
}

// logits (M,C) fp32, target int64 (M,).  loss: 1 float.  dlogits (M,C) or NULL =
// d(mean CE)/d(logits).  row_ws: M floats of scratch.  *bad_flag set on a target
// outside [0,C).
// The same with leading dimensions: logits rows at ld_logits >= C (columns C .. ld_logits - 1 are never read),
// dlogits rows at ld_dlogits >= C, columns C .. ld_dlogits - 1 written as exact zeros -- the classifier's
// (M, 528) logits buffer and the zero-padded dlogits its input-gradient GEMM reduces over.  Loss, row_ws and
// dlogits[:, :C] carry the bits of the dense entry, which is the ld == C case of this one.
extern "C" int qarig_cross_entropy_ld_fwd(const float* logits, int64_t ld_logits, const int64_t* target, int M, int C,
                                          float* loss, float* dlogits, int64_t ld_dlogits, float* row_ws,
                                          int* bad_flag, void* stream) {
    QARIG_CHECK_ARG(logits && target && loss && row_ws && bad_flag && M > 0 && C > 0,
                    "cross_entropy: bad arguments");
    QARIG_CHECK_DIMS("cross_entropy", M, C);
    QARIG_CHECK_ARG(ld_logits >= C && (!dlogits || ld_dlogits >= C) && ld_logits <= (1LL << 31) &&
                        ld_dlogits <= (1LL << 31),
                    "cross_entropy: leading dimensions must be at least C = %d (got %lld, %lld)", C,
                    (long long)ld_logits, (long long)ld_dlogits);
    hipStream_t st = (hipStream_t)stream;
    const float inv_m = 1.0f / (float)M;
    hipLaunchKernelGGL(ce_rows_kernel, dim3((M + 3) / 4), dim3(256), 0, st, logits, ld_logits, target, M, C,
                       inv_m, row_ws, dlogits, ld_dlogits, bad_flag);
    QARIG_CHECK_LAUNCH("cross_entropy rows");
    hipLaunchKernelGGL(mean_kernel, dim3(1), dim3(256), 0, st, row_ws, M, inv_m, loss);
    QARIG_CHECK_LAUNCH("cross_entropy mean");
    return QARIG_OK;
}

extern "C" int qarig_cross_entropy_fwd(const float* logits, const int64_t* target, int M, int C,
                                       float* loss, float* dlogits, float* row_ws, int* bad_flag,
                                       void* stream) {
    return qarig_cross_entropy_ld_fwd(logits, C, target, M, C, loss, dlogits, C, row_ws, bad_flag, stream);
}

// ---- cross-entropy with label smoothing and z-loss (additive; the reference trains with neither) ----------------
// Per row, mx = max x, s = sum exp(x - mx), logs = log s, lse = mx + logs, p = exp((x - mx) - logs):
//   nll = logs - (x[t] - mx),  u = logs - (1 / C) sum (x - mx)  (cross-entropy against the uniform distribution),
//   obj = (1 - eps) nll + eps u + zeta lse^2,  d obj / d x[c] = p (1 + 2 zeta lse) - (1 - eps) [c == t] - eps / C.
// u comes from the SHIFTED sum, accumulated in the sweep that forms s: sum x - C mx rounds at the magnitude of the
// logits (0.03 at logits near 1000), the shifted sum at the magnitude of the loss.  Only lse^2 sees ulp(|mx|): it
// is the quantity the z-loss penalises.  A term whose coefficient is 0 is not evaluated (EPS / ZL are compiled
// out), so eps = 0 never forms 0 * inf on a row with -inf entries, and <false, false> is ce_rows_kernel's
// arithmetic operation for operation: the same bits.  The sweeps are token_score_kernel's: four trips' loads in
// flight, the sum in its own order (lane partial sums in ascending trips, then the butterfly).  4-byte loads only:
// column c stays on lane c % 64 whatever the row's alignment (C = 513 rows are 4-byte aligned).
namespace qarig {

//
// NB (SOM-neighbour soft targets): the leading `codes` classes lie on the codebook's one-dimensional
// SOM axis, and a row with target t < codes spreads nu over the codes within R of t, by a table w[0 .. R] of the
// index distance (w[0] = 1), clamped at the ends of the axis and renormalised:
//   lo = max(0, t - R), hi = min(codes - 1, t + R),  q[j] = w[|j - t|] / sum_{lo <= i <= hi} w[|i - t|],
//   h = logs - sum_j q[j] (x[j] - mx),  obj = (1 - eps - nu) nll + eps u + nu h + zeta lse^2,
//   d obj / d x[c] = p (1 + 2 zeta lse) - (1 - eps - nu) [c == t] - eps / C - nu q[c].
// R <= 31: the window t - R .. t + R holds at most 63 columns, so each lane owns at most one of them, the unique
// c = lane (mod 64) -- the lane that reads and writes column c in every sweep.  It gathers w and x[c] once, q[c]
// stays in its register, the normaliser and the weighted shifted sum are two more butterflies behind the sweeps, and
// behind the gradient sweep the lane rewrites the one element it owns with nu q[c] taken off (a test per element
// inside the sweep cost 6.6 % at 32,768 x 8,193; this costs nothing).  A row whose target is a special class (t >= codes) takes nu = 0 by selects: no window, the
// objective and the gradient of the <EPS, ZL, false> kernel bit for bit.  A window column with weight exactly 0 (an
// underflowed table entry) is no window column, so a -inf there is never multiplied by it.  <., ., false> is the
// kernel as it was, operation for operation.
template <bool EPS, bool ZL, bool NB>
__global__ __launch_bounds__(256) void ce_reg_rows_kernel(const float* __restrict__ logits,
                                                          const int64_t* __restrict__ target, int M, int C,
                                                          float inv_m, float eps, float zeta, int codes, float nu,
                                                          int R, const float* __restrict__ w,
                                                          float* __restrict__ row_obj, float* __restrict__ row_nll,
                                                          float* __restrict__ dlogits, int* __restrict__ bad) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const float* x = logits + (int64_t)row * C;
    const int64_t t = target[row];
    const bool ok = t >= 0 && t < C;
    const float xt = ok ? x[t] : 0.0f;
    const bool soft = NB && ok && t < codes;     // wave-uniform: the row's target is a code
    int wc = -1;                                 // this lane's window column, -1: none
    float wq = 0.0f, xw = 0.0f;                  // its table entry (later q[wc]) and its logit
    if (NB) {       // the two gathered loads are issued here and first waited for behind the sweeps
        if (soft) {
            const int ti = (int)t, first = ti - R;
            const int off = (lane - first) & 63, cc = first + off;       // the c = lane (mod 64) at or after t - R
            if (off <= 2 * R && cc >= 0 && cc < codes) {
                const int dist = cc < ti ? ti - cc : cc - ti;
                const float wd = w[dist];
                if (wd > 0.0f) {
                    wc = cc;
                    wq = wd;
                    xw = x[cc];
                }
            }
        }
    }
    float mx = -INFINITY;
    int c = lane;
    for (; c + 192 < C; c += 256) {
        const float v0 = x[c], v1 = x[c + 64], v2 = x[c + 128], v3 = x[c + 192];
        mx = fmaxf(fmaxf(mx, v0), fmaxf(fmaxf(v1, v2), v3));
    }
    for (; c < C; c += 64) mx = fmaxf(mx, x[c]);
    mx = wave_max(mx);
    float s = 0.0f, sh = 0.0f;
    c = lane;
    for (; c + 192 < C; c += 256) {
        const float v0 = x[c], v1 = x[c + 64], v2 = x[c + 128], v3 = x[c + 192];
        const float d0 = v0 - mx, d1 = v1 - mx, d2 = v2 - mx, d3 = v3 - mx;
        s += expf(d0);
        s += expf(d1);
        s += expf(d2);
        s += expf(d3);
        if (EPS) {
            sh += d0;
            sh += d1;
            sh += d2;
            sh += d3;
        }
    }
    for (; c < C; c += 64) {
        const float d = x[c] - mx;
        s += expf(d);
        if (EPS) sh += d;
    }
    s = wave_sum(s);
    const float logs = logf(s);
    const float nll = logs - (xt - mx);
    float obj = nll, f = 1.0f;
    float hot = EPS ? 1.0f - eps : 1.0f;
    if (NB) {
        const float nur = soft ? nu : 0.0f;
        hot -= nur;
        if (!EPS) obj = hot * nll;
    }
    if (EPS) {
        sh = wave_sum(sh);
        const float u = logs - sh / (float)C;        // +inf on a row with -inf entries, as torch gives
        obj = fmaf(eps, u, hot * nll);
    }
    if (NB) {
        const float z = wave_sum(wq);
        wq = wc >= 0 ? wq / z : 0.0f;
        const float hs = wave_sum(wc >= 0 ? wq * (xw - mx) : 0.0f);
        const float h = logs - hs;                   // +inf where a window column holds -inf, as u is
        obj = soft ? fmaf(nu, h, obj) : obj;
    }
    if (ZL) {
        const float lse = mx + logs, zl = zeta * lse;
        obj = fmaf(zl, lse, obj);
        f = fmaf(2.0f, zl, 1.0f);
    }
    if (lane == 0) {
        if (!ok) atomicExch(bad, 1);
        row_obj[row] = ok ? obj : 0.0f;
        row_nll[row] = ok ? nll : 0.0f;
    }
    if (!dlogits) return;
    float* d = dlogits + (int64_t)row * C;
    const float epsc = eps / (float)C;
    auto unscaled = [&](float v, int col) {
        const float p = expf((v - mx) - logs);
        const float h = (int64_t)col == t ? hot : 0.0f;
        float g = ZL ? fmaf(p, f, -h) : p - h;
        if (EPS) g -= epsc;
        return g;
    };
    auto grad = [&](float v, int col) { return unscaled(v, col) * inv_m; };
    c = lane;
    for (; c + 192 < C; c += 256) {
        const float v0 = x[c], v1 = x[c + 64], v2 = x[c + 128], v3 = x[c + 192];
        d[c] = grad(v0, c);
        d[c + 64] = grad(v1, c + 64);
        d[c + 128] = grad(v2, c + 128);
        d[c + 192] = grad(v3, c + 192);
    }
    for (; c < C; c += 64) d[c] = grad(x[c], c);
    // the window: each lane corrects the one element it owns and has just written itself, so the sweep above carries
    // no per-element test for it
    if (NB && wc >= 0) d[wc] = (unscaled(xw, wc) - nu * wq) * inv_m;
}

// mean_kernel on both columns of row_ws in one launch: block b reduces v[b M ... b M + M) into out[b], each in
// mean_kernel's order.
__global__ __launch_bounds__(256) void mean2_kernel(const float* __restrict__ v, int M, float inv_m,
                                                    float* __restrict__ out) {
    __shared__ float red[256];
    v += (int64_t)blockIdx.x * M;
    float s = 0.0f;
    for (int i = threadIdx.x; i < M; i += 256) s += v[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = red[0] * inv_m;
}

}  // namespace qarig

// F.cross_entropy(logits, target, label_smoothing = eps) + zeta mean(logsumexp(logits)^2) and its gradient.
// loss: 2 floats {mean objective, mean plain nll}.  row_ws: 2 M floats, the row objectives then the row nlls.
extern "C" int qarig_cross_entropy_reg_fwd(const float* logits, const int64_t* target, int M, int C,
                                           float label_smoothing, float z_loss, float* loss, float* dlogits,
                                           float* row_ws, int* bad_flag, void* stream) {
    QARIG_CHECK_ARG(logits && target && loss && row_ws && bad_flag && M > 0 && C > 0,
                    "cross_entropy_reg: bad arguments");
    QARIG_CHECK_DIMS("cross_entropy_reg", M, C);
    QARIG_CHECK_ARG(label_smoothing >= 0.0f && label_smoothing < 1.0f,
                    "cross_entropy_reg: label_smoothing must lie in [0, 1)");
    QARIG_CHECK_ARG(z_loss >= 0.0f && z_loss < INFINITY, "cross_entropy_reg: z_loss must be finite and >= 0");
    hipStream_t st = (hipStream_t)stream;
    const float inv_m = 1.0f / (float)M;
    const bool e = label_smoothing > 0.0f, z = z_loss > 0.0f;
    auto kernel = e ? (z ? ce_reg_rows_kernel<true, true, false> : ce_reg_rows_kernel<true, false, false>)
                    : (z ? ce_reg_rows_kernel<false, true, false> : ce_reg_rows_kernel<false, false, false>);
    hipLaunchKernelGGL(kernel, dim3((M + 3) / 4), dim3(256), 0, st, logits, target, M, C, inv_m, label_smoothing,
                       z_loss, C, 0.0f, 0, (const float*)nullptr, row_ws, row_ws + M, dlogits, bad_flag);
    QARIG_CHECK_LAUNCH("cross_entropy_reg rows");
    hipLaunchKernelGGL(mean2_kernel, dim3(2), dim3(256), 0, st, row_ws, M, inv_m, loss);
    QARIG_CHECK_LAUNCH("cross_entropy_reg mean");
    return QARIG_OK;
}

// The same with SOM-neighbour soft targets (additive): of the smoothing mass, neighbour_smoothing goes
// to the codes within `range` of the target on the SOM axis, by weights[|j - t|] (device, range + 1 floats,
// weights[0] = 1), clamped to the `codes` leading classes and renormalised; rows whose target is one of the special
// classes codes .. C - 1 take neighbour_smoothing = 0.  At neighbour_smoothing = 0 the call IS
// qarig_cross_entropy_reg_fwd (range and weights are then not looked at).
extern "C" int qarig_cross_entropy_soft_fwd(const float* logits, const int64_t* target, int M, int C, int codes,
                                            float label_smoothing, float z_loss, float neighbour_smoothing, int range,
                                            const float* weights, float* loss, float* dlogits, float* row_ws,
                                            int* bad_flag, void* stream) {
    QARIG_CHECK_ARG(logits && target && loss && row_ws && bad_flag && M > 0 && C > 0,
                    "cross_entropy_soft: bad arguments");
    QARIG_CHECK_DIMS("cross_entropy_soft", M, C);
    QARIG_CHECK_ARG(label_smoothing >= 0.0f && label_smoothing < 1.0f,
                    "cross_entropy_soft: label_smoothing must lie in [0, 1)");
    QARIG_CHECK_ARG(z_loss >= 0.0f && z_loss < INFINITY, "cross_entropy_soft: z_loss must be finite and >= 0");
    QARIG_CHECK_ARG(neighbour_smoothing >= 0.0f && neighbour_smoothing < 1.0f,
                    "cross_entropy_soft: neighbour_smoothing must lie in [0, 1)");
    QARIG_CHECK_ARG(label_smoothing + neighbour_smoothing < 1.0f,
                    "cross_entropy_soft: label_smoothing + neighbour_smoothing must stay below 1");
    QARIG_CHECK_ARG(codes > 0 && codes <= C, "cross_entropy_soft: codes must lie in [1, C = %d] (got %d)", C, codes);
    if (!(neighbour_smoothing > 0.0f))
        return qarig_cross_entropy_reg_fwd(logits, target, M, C, label_smoothing, z_loss, loss, dlogits, row_ws,
                                           bad_flag, stream);
    QARIG_CHECK_ARG(range >= 1 && range <= 31, "cross_entropy_soft: range must lie in [1, 31] (got %d)", range);
    QARIG_CHECK_ARG(weights, "cross_entropy_soft: neighbour_smoothing > 0 needs the weight table");
    hipStream_t st = (hipStream_t)stream;
    const float inv_m = 1.0f / (float)M;
    const bool e = label_smoothing > 0.0f, z = z_loss > 0.0f;
    auto kernel = e ? (z ? ce_reg_rows_kernel<true, true, true> : ce_reg_rows_kernel<true, false, true>)
                    : (z ? ce_reg_rows_kernel<false, true, true> : ce_reg_rows_kernel<false, false, true>);
    hipLaunchKernelGGL(kernel, dim3((M + 3) / 4), dim3(256), 0, st, logits, target, M, C, inv_m, label_smoothing,
                       z_loss, codes, neighbour_smoothing, range, weights, row_ws, row_ws + M, dlogits, bad_flag);
    QARIG_CHECK_LAUNCH("cross_entropy_soft rows");
    hipLaunchKernelGGL(mean2_kernel, dim3(2), dim3(256), 0, st, row_ws, M, inv_m, loss);
    QARIG_CHECK_LAUNCH("cross_entropy_soft mean");
    return QARIG_OK;
}
