// Cross-entropy (mean over rows) forward fused with its gradient w.r.t. the logits:
// nn.CrossEntropyLoss() as the reference trains with
// (train_quantized_transformer.py:337,496-502), with the additive label smoothing, z-loss and SOM-neighbour soft
// targets, and F.mse_loss.  One wave per row; one row kernel, one mean kernel, one launcher.
#include "qarig_common.h"
#include "row_sweep.h"

namespace qarig {

// block b: out[b] = inv_m * sum of v[b M ... b M + M), fixed order: 256 strided partial sums, then a tree.  One block
// for the plain cross-entropy and the MSE, two for the {objective, nll} columns of row_ws.
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

// ---- the cross-entropy row kernel: plain, and with label smoothing, z-loss (additive; the reference trains with
// neither) and SOM-neighbour soft targets ------------------------------------------------------------------------
// Per row, mx = max x, s = sum exp(x - mx), logs = log s, lse = mx + logs, p = exp((x - mx) - logs):
//   nll = logs - (x[t] - mx),  u = logs - (1 / C) sum (x - mx)  (cross-entropy against the uniform distribution),
//   obj = (1 - eps) nll + eps u + zeta lse^2,  d obj / d x[c] = p (1 + 2 zeta lse) - (1 - eps) [c == t] - eps / C.
// log s - (x[t] - mx) and exp((x - mx) - log s): every rounding happens at the magnitude of the loss, not of the
// logits (mx + log s first costs ulp(|mx|) -- 6e-5 at logits near 1000).  u comes from the SHIFTED sum, accumulated
// in the sweep that forms s: sum x - C mx rounds at the magnitude of the logits (0.03 at logits near 1000), the
// shifted sum at the magnitude of the loss.  Only lse^2 sees ulp(|mx|): it is the quantity the z-loss penalises.  A
// term whose coefficient is 0 is not evaluated (EPS / ZL are compiled out), so eps = 0 never forms 0 * inf on a row
// with -inf entries, and <false, false, false> is the plain cross-entropy: obj = nll, gradient (p - [c == t]) / M.
// The three sweeps are row_sweep's (row_sweep.h): the sum in its own order, lane partial sums in ascending trips,
// then the butterfly.
//
// Rows lie at leading dimensions ld_logits / ld_dlogits >= C: columns C .. ld_logits - 1 of the logits are never
// read, columns C .. ld_dlogits - 1 of the gradient receive exact zeros (a GEMM reduces over them).  row_nll may be
// NULL (the plain entries' row_ws holds M floats).
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
// underflowed table entry) is no window column, so a -inf there is never multiplied by it.
template <bool EPS, bool ZL, bool NB>
__global__ __launch_bounds__(256) void ce_reg_rows_kernel(const float* __restrict__ logits, int64_t ld_logits,
                                                          const int64_t* __restrict__ target, int M, int C,
                                                          float inv_m, float eps, float zeta, int codes, float nu,
                                                          int R, const float* __restrict__ w,
                                                          float* __restrict__ row_obj, float* __restrict__ row_nll,
                                                          float* __restrict__ dlogits, int64_t ld_dlogits,
                                                          int* __restrict__ bad) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const float* x = logits + (int64_t)row * ld_logits;
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
    row_sweep(x, C, lane, [&](float v, int) { mx = fmaxf(mx, v); });
    mx = wave_max(mx);
    float s = 0.0f, sh = 0.0f;
    row_sweep(x, C, lane, [&](float v, int) {
        const float d = v - mx;
        s += expf(d);
        if (EPS) sh += d;
    });
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
        if (row_nll) row_nll[row] = ok ? nll : 0.0f;
    }
    if (!dlogits) return;
    float* d = dlogits + (int64_t)row * ld_dlogits;
    const float epsc = eps / (float)C;
    auto unscaled = [&](float v, int col) {
        const float p = expf((v - mx) - logs);
        const float h = (int64_t)col == t ? hot : 0.0f;
        float g = ZL ? fmaf(p, f, -h) : p - h;
        if (EPS) g -= epsc;
        return g;
    };
    row_sweep(x, C, lane, [&](float v, int col) { d[col] = unscaled(v, col) * inv_m; });
    // the window: each lane corrects the one element it owns and has just written itself, so the sweep above carries
    // no per-element test for it
    if (NB && wc >= 0) d[wc] = (unscaled(xw, wc) - nu * wq) * inv_m;
    for (int64_t c = C + lane; c < ld_dlogits; c += 64) d[c] = 0.0f;
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
    hipLaunchKernelGGL(mean2_kernel, dim3(1), dim3(256), 0, st, part_ws, MSE_BLOCKS, inv_n, loss);
    QARIG_CHECK_LAUNCH("mse mean");
    return QARIG_OK;
}

// ---- cross-entropy: every entry fills this and calls ce_launch (contracts: include/qarig.h) ----------------------
struct CeArgs {
    const char* who;         // the calling entry's prefix in its error messages
    const float* logits;
    int64_t ld_logits;
    const int64_t* target;
    int M, C, codes;
    float eps, zeta, nu;     // label_smoothing, z_loss, neighbour_smoothing
    int range;
    const float* weights;
    float* loss;             // pair ? {mean objective, mean nll} : the mean loss
    float* dlogits;
    int64_t ld_dlogits;
    float* row_ws;           // pair ? 2 M floats, the row objectives then the row nlls : M floats
    bool pair;
    int* bad_flag;
    void* stream;
};

// The older entries pass the neutral value of what they do not take (ld = C, 0, codes = C), which every check
// below accepts: the set of arguments each of them refuses is its own.
static int ce_launch(const CeArgs& a) {
    QARIG_CHECK_ARG(a.logits && a.target && a.loss && a.row_ws && a.bad_flag && a.M > 0 && a.C > 0,
                    "%s: bad arguments", a.who);
    QARIG_CHECK_ARG(qarig_dims_ok({a.M, a.C}),
                    "%s: extents must be positive, at most 2^24 each, product at most 2^40", a.who);
    QARIG_CHECK_ARG(a.ld_logits >= a.C && (!a.dlogits || a.ld_dlogits >= a.C) && a.ld_logits <= (1LL << 31) &&
                        a.ld_dlogits <= (1LL << 31),
                    "%s: leading dimensions must be at least C = %d (got %lld, %lld)", a.who, a.C,
                    (long long)a.ld_logits, (long long)a.ld_dlogits);
    QARIG_CHECK_ARG(a.eps >= 0.0f && a.eps < 1.0f, "%s: label_smoothing must lie in [0, 1)", a.who);
    QARIG_CHECK_ARG(a.zeta >= 0.0f && a.zeta < INFINITY, "%s: z_loss must be finite and >= 0", a.who);
    QARIG_CHECK_ARG(a.nu >= 0.0f && a.nu < 1.0f, "%s: neighbour_smoothing must lie in [0, 1)", a.who);
    QARIG_CHECK_ARG(a.eps + a.nu < 1.0f, "%s: label_smoothing + neighbour_smoothing must stay below 1", a.who);
    QARIG_CHECK_ARG(a.codes > 0 && a.codes <= a.C, "%s: codes must lie in [1, C = %d] (got %d)", a.who, a.C, a.codes);
    const bool e = a.eps > 0.0f, z = a.zeta > 0.0f, nb = a.nu > 0.0f;
    if (nb) {       // at neighbour_smoothing = 0 range and weights are not looked at
        QARIG_CHECK_ARG(a.range >= 1 && a.range <= 31, "%s: range must lie in [1, 31] (got %d)", a.who, a.range);
        QARIG_CHECK_ARG(a.weights, "%s: neighbour_smoothing > 0 needs the weight table", a.who);
    }
    static constexpr decltype(&ce_reg_rows_kernel<false, false, false>) kernels[8] = {
        ce_reg_rows_kernel<false, false, false>, ce_reg_rows_kernel<false, false, true>,
        ce_reg_rows_kernel<false, true, false>,  ce_reg_rows_kernel<false, true, true>,
        ce_reg_rows_kernel<true, false, false>,  ce_reg_rows_kernel<true, false, true>,
        ce_reg_rows_kernel<true, true, false>,   ce_reg_rows_kernel<true, true, true>};
    hipStream_t st = (hipStream_t)a.stream;
    const float inv_m = 1.0f / (float)a.M;
    hipLaunchKernelGGL(kernels[4 * e + 2 * z + nb], dim3((a.M + 3) / 4), dim3(256), 0, st, a.logits, a.ld_logits,
                       a.target, a.M, a.C, inv_m, a.eps, a.zeta, a.codes, a.nu, a.range, a.weights, a.row_ws,
                       a.pair ? a.row_ws + a.M : (float*)nullptr, a.dlogits, a.ld_dlogits, a.bad_flag);
    QARIG_CHECK_LAUNCH("cross_entropy rows");
    hipLaunchKernelGGL(mean2_kernel, dim3(a.pair ? 2 : 1), dim3(256), 0, st, a.row_ws, a.M, inv_m, a.loss);
    QARIG_CHECK_LAUNCH("cross_entropy mean");
    return QARIG_OK;
}

extern "C" int qarig_cross_entropy_fused_fwd(const float* logits, int64_t ld_logits, const int64_t* target, int M,
                                             int C, int codes, float label_smoothing, float z_loss,
                                             float neighbour_smoothing, int range, const float* weights, float* loss,
                                             float* dlogits, int64_t ld_dlogits, float* row_ws, int* bad_flag,
                                             void* stream) {
    return ce_launch({"cross_entropy_fused", logits, ld_logits, target, M, C, codes, label_smoothing, z_loss,
                      neighbour_smoothing, range, weights, loss, dlogits, ld_dlogits, row_ws, true, bad_flag, stream});
}

extern "C" int qarig_cross_entropy_ld_fwd(const float* logits, int64_t ld_logits, const int64_t* target, int M, int C,
                                          float* loss, float* dlogits, int64_t ld_dlogits, float* row_ws,
                                          int* bad_flag, void* stream) {
    return ce_launch({"cross_entropy", logits, ld_logits, target, M, C, C, 0.0f, 0.0f, 0.0f, 0, nullptr, loss, dlogits,
                      ld_dlogits, row_ws, false, bad_flag, stream});
}

extern "C" int qarig_cross_entropy_fwd(const float* logits, const int64_t* target, int M, int C,
                                       float* loss, float* dlogits, float* row_ws, int* bad_flag,
                                       void* stream) {
    return qarig_cross_entropy_ld_fwd(logits, C, target, M, C, loss, dlogits, C, row_ws, bad_flag, stream);
}

extern "C" int qarig_cross_entropy_reg_fwd(const float* logits, const int64_t* target, int M, int C,
                                           float label_smoothing, float z_loss, float* loss, float* dlogits,
                                           float* row_ws, int* bad_flag, void* stream) {
    return ce_launch({"cross_entropy_reg", logits, C, target, M, C, C, label_smoothing, z_loss, 0.0f, 0, nullptr, loss,
                      dlogits, C, row_ws, true, bad_flag, stream});
}

extern "C" int qarig_cross_entropy_soft_fwd(const float* logits, const int64_t* target, int M, int C, int codes,
                                            float label_smoothing, float z_loss, float neighbour_smoothing, int range,
                                            const float* weights, float* loss, float* dlogits, float* row_ws,
                                            int* bad_flag, void* stream) {
    return ce_launch({"cross_entropy_soft", logits, C, target, M, C, codes, label_smoothing, z_loss,
                      neighbour_smoothing, range, weights, loss, dlogits, C, row_ws, true, bad_flag, stream});
}
