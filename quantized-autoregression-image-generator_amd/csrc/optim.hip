// Adam step over one flat fp32 buffer (all parameters of a model live in one
// allocation; so do their gradients and moments): one launch per step, and the same
// flat gradient buffer is what the DP all-reduce moves.  Semantics of
// torch.optim.Adam(lr, betas) without weight decay / amsgrad
// (train_quantized_transformer.py:317-320; train_autoencoder.py:133-136).  Additive: a decoupled weight decay of
// the groups a mask selects (torch.optim.AdamW with two parameter groups), an EMA of the parameters and a
// global-norm gradient clip with a skipped-step guard, all from the same launch.
// The update of one element is stated once, in adam_element.h.  Two kernel bodies call it: adam_kernel (one element
// per thread-iteration, any 4-byte alignment: the plain and the EMA entry) and adam_groups_kernel (groups of 8,
// 16-byte accesses: the AdamW and the clip entry).  adam_launch is the host side of all four entries.
#include "adam_element.h"
#include "qarig_common.h"

namespace qarig {

// EMA: the same pass also moves an exponential moving average of the parameters, e <- lerp(e, pn, ema_w),
// one more read and one more write stream on the launch (7 -> 9), no further launch.  The loads stay in this
// order (g, m, v, then p, then ema): the compiler's schedule of the benchmarked launch follows it.
template <bool EMA>
__global__ void adam_kernel(float* __restrict__ p, const float* __restrict__ g,
                            float* __restrict__ m, float* __restrict__ v, float* __restrict__ ema,
                            int64_t n, float beta1, float beta2, float eps, float step_size,
                            float bc2_sqrt, float ema_w, float grad_scale,
                            const float* __restrict__ dev_step, unsigned short* __restrict__ shadow) {
    if (dev_step) {     // captured-graph replay: the per-step scalars live in device memory
        step_size = dev_step[0];
        bc2_sqrt = dev_step[1];
        if (EMA) ema_w = dev_step[2];
    }
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        const float gi = g[i];
        float mi = m[i], vi = v[i];
        const float pi = p[i];
        float ei = EMA ? ema[i] : 0.0f;
        const float pn = adam_element<EMA>(pi, gi, mi, vi, ei, /*decayed*/ false, beta1, beta2, eps, step_size,
                                           bc2_sqrt, ema_w, /*decay*/ 0.0f, grad_scale);
        p[i] = pn;
        m[i] = mi;
        v[i] = vi;
        if (EMA) ema[i] = ei;
        // reduced-precision mode: the bf16 copy the GEMMs read, from the same pass
        if (shadow) shadow[i] = (unsigned short)(pack_bf16x2(pn, 0.0f) & 0xffffu);
    }
}

// AdamW and the clip.  One thread-iteration = one group of 8 elements = one mask byte: two 16-byte loads per input
// stream, all of them ahead of the first store, two 16-byte stores per fp32 output stream and one for the 8 bf16 of
// the shadow.  The last group of an n that is no multiple of 8 goes element by element and touches nothing at or
// behind n.  7 (9 with the EMA) streams of 4 bytes per element as adam_kernel, plus n / 8 mask bytes.
// CLIP: gi = fp32(fp32(g * grad_scale) * coef), norm and coef read from clip_state by every thread; a norm that is
// not finite ends the kernel before it loads or stores anything else (the step is skipped); mask may be NULL
// (nothing decayed).  A template parameter: without it no clip_state read, early return or second multiply is left.
template <bool EMA, bool CLIP>
__global__ void adam_groups_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                   float* __restrict__ v, float* __restrict__ ema,
                                   const unsigned char* __restrict__ mask, int64_t n, float beta1, float beta2,
                                   float eps, float step_size, float bc2_sqrt, float ema_w, float decay,
                                   float grad_scale, const float* __restrict__ dev_step,
                                   unsigned short* __restrict__ shadow, const double* __restrict__ clip_state) {
    float scale = grad_scale;       // the element's scale argument; behind the clip coef, on fp32(g * grad_scale)
    if (CLIP) {
        const double norm = clip_state[0];
        scale = (float)clip_state[1];
        if (!(__builtin_fabs(norm) <= 1.7976931348623157e308)) return;
    }
    if (dev_step) {     // captured-graph replay: always four floats {step_size, bc2_sqrt, ema_w, decay}
        step_size = dev_step[0];
        bc2_sqrt = dev_step[1];
        if (EMA) ema_w = dev_step[2];
        decay = dev_step[3];
    }
    const int64_t full = n >> 3, groups = (n + 7) >> 3;
    for (int64_t gr = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; gr < groups;
         gr += (int64_t)gridDim.x * blockDim.x) {
        const bool decayed = (!CLIP || mask) ? mask[gr] != 0 : false;
        const int64_t base = gr << 3;
        if (gr < full) {
            f32x4 pv[2], gv[2], mv[2], vv[2], ev[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                pv[h] = *(const f32x4*)(p + base + 4 * h);
                gv[h] = *(const f32x4*)(g + base + 4 * h);
                mv[h] = *(const f32x4*)(m + base + 4 * h);
                vv[h] = *(const f32x4*)(v + base + 4 * h);
                if (EMA) ev[h] = *(const f32x4*)(ema + base + 4 * h);
            }
#pragma unroll
            for (int h = 0; h < 2; ++h) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    float mi = mv[h][k], vi = vv[h][k], ei = EMA ? ev[h][k] : 0.0f;
                    pv[h][k] = adam_element<EMA>(pv[h][k], CLIP ? gv[h][k] * grad_scale : gv[h][k], mi, vi, ei,
                                                 decayed, beta1, beta2, eps, step_size, bc2_sqrt, ema_w, decay, scale);
                    mv[h][k] = mi;
                    vv[h][k] = vi;
                    if (EMA) ev[h][k] = ei;
                }
            }
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                *(f32x4*)(p + base + 4 * h) = pv[h];
                *(f32x4*)(m + base + 4 * h) = mv[h];
                *(f32x4*)(v + base + 4 * h) = vv[h];
                if (EMA) *(f32x4*)(ema + base + 4 * h) = ev[h];
            }
            if (shadow) {
                uint4 s;
                s.x = pack_bf16x2(pv[0][0], pv[0][1]);
                s.y = pack_bf16x2(pv[0][2], pv[0][3]);
                s.z = pack_bf16x2(pv[1][0], pv[1][1]);
                s.w = pack_bf16x2(pv[1][2], pv[1][3]);
                *(uint4*)(shadow + base) = s;
            }
        } else {
            for (int64_t i = base; i < n; ++i) {
                float mi = m[i], vi = v[i], ei = EMA ? ema[i] : 0.0f;
                const float pn = adam_element<EMA>(p[i], CLIP ? g[i] * grad_scale : g[i], mi, vi, ei, decayed, beta1,
                                                   beta2, eps, step_size, bc2_sqrt, ema_w, decay, scale);
                p[i] = pn;
                m[i] = mi;
                v[i] = vi;
                if (EMA) ema[i] = ei;
                if (shadow) shadow[i] = (unsigned short)(pack_bf16x2(pn, 0.0f) & 0xffffu);
            }
        }
    }
}

// ---- global-norm gradient clipping (additive: the reference trains without) -------------------------------------
// include/qarig.h QARIG_GRAD_NORM_PARTIALS: the cap of the norm kernel's grid and the size of its partials buffer
static constexpr int GRAD_NORM_PARTIALS = 2048;
static constexpr int GRAD_NORM_BLOCK = 256;

// sum over the workgroup of one fp64 value per thread, in a fixed order: the 64-lane butterfly (offsets 32 ... 1;
// both lanes of a pair add the same two values, so every lane ends with the same bits), then the four waves
// through LDS in wave order, ((w0 + w1) + w2) + w3.  Valid in thread 0.
__device__ __forceinline__ double block_sum_f64(double x, double* lds) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = x;
    __syncthreads();
    return ((lds[0] + lds[1]) + lds[2]) + lds[3];
}

// acc += (double)fp32(g * grad_scale) squared: the product of two equal 24-bit values is exact in fp64
__device__ __forceinline__ void norm_term(double& acc, float g, float grad_scale) {
    const double s = (double)(g * grad_scale);
    acc += s * s;
}

// Stage 1: partials[b] = the sum of squares of the 16-byte vectors j = b * 256 + lane + t * gridDim.x * 256 of g,
// trips t ascending, the four elements of a vector in order, one fp64 accumulator per lane; four trips' loads are
// issued before the first is used.  The lane whose sequence reaches vector floor(n / 4) takes the n % 4 tail
// elements one by one behind its vectors.  Nothing at or behind n is read.
__global__ __launch_bounds__(GRAD_NORM_BLOCK) void grad_sumsq_kernel(const float* __restrict__ g, int64_t n,
                                                                      float grad_scale,
                                                                      double* __restrict__ partials) {
    __shared__ double lds[4];
    const int64_t nvec = n >> 2;
    const int64_t stride = (int64_t)gridDim.x * GRAD_NORM_BLOCK;
    const f32x4* __restrict__ g4 = (const f32x4*)g;
    int64_t j = (int64_t)blockIdx.x * GRAD_NORM_BLOCK + threadIdx.x;
    double acc = 0.0;
    for (; j + 3 * stride < nvec; j += 4 * stride) {
        f32x4 x[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) x[t] = g4[j + t * stride];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
#pragma unroll
            for (int k = 0; k < 4; ++k) norm_term(acc, x[t][k], grad_scale);
        }
    }
    for (; j < nvec; j += stride) {
        const f32x4 x = g4[j];
#pragma unroll
        for (int k = 0; k < 4; ++k) norm_term(acc, x[k], grad_scale);
    }
    if (j == nvec) {
        for (int64_t i = nvec << 2; i < n; ++i) norm_term(acc, g[i], grad_scale);
    }
    const double total = block_sum_f64(acc, lds);
    if (threadIdx.x == 0) partials[blockIdx.x] = total;
}

// Stage 2, one workgroup: thread t adds partials[t], partials[t + 256], ... ascending, then block_sum_f64.
// state = {norm, coef, steps skipped, steps clipped}; the two counts live across steps.
__global__ __launch_bounds__(GRAD_NORM_BLOCK) void grad_clip_coef_kernel(const double* __restrict__ partials,
                                                                          int count, double max_norm,
                                                                          double* __restrict__ state) {
    __shared__ double lds[4];
    double acc = 0.0;
    for (int i = threadIdx.x; i < count; i += GRAD_NORM_BLOCK) acc += partials[i];
    const double sum = block_sum_f64(acc, lds);
    if (threadIdx.x == 0) {
        const double norm = __builtin_sqrt(sum);
        const bool finite = __builtin_fabs(norm) <= 1.7976931348623157e308;      // (false for a NaN)
        double c = max_norm / (norm + 1e-6);
        c = c < 1.0 ? c : 1.0;
        const float coef = finite ? (float)c : 0.0f;
        state[0] = norm;
        state[1] = (double)coef;
        if (!finite) state[2] += 1.0;
        if (finite && coef < 1.0f) state[3] += 1.0;
    }
}

// Exchanges two fp32 buffers in place, as bit patterns (no arithmetic touches the values): 16-byte body where
// both buffers are 16-byte aligned, scalar tail behind it.
__global__ void swap_f32_kernel(unsigned* __restrict__ a, unsigned* __restrict__ b, int64_t nvec, int64_t n) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    uint4* a4 = (uint4*)a;
    uint4* b4 = (uint4*)b;
    for (int64_t i = t; i < nvec; i += stride) {
        const uint4 x = a4[i], y = b4[i];
        a4[i] = y;
        b4[i] = x;
    }
    for (int64_t i = nvec * 4 + t; i < n; i += stride) {
        const unsigned x = a[i], y = b[i];
        a[i] = y;
        b[i] = x;
    }
}

}  // namespace qarig

using namespace qarig;

// The host side of the four Adam entries (include/qarig.h documents their arguments and what they refuse): each
// checks the one pointer that is its own and calls this; `who` prefixes every message.  grouped: adam_groups_kernel,
// whose 16-byte accesses need aligned buffers and an ema and a shadow that do not overlap p, with the clip where
// clip_state is given; otherwise adam_kernel, which takes any 4-byte-aligned view.  The EMA instantiation where ema
// is given; decay is looked at only where there is a mask.  A refused call launches nothing.
static int adam_launch(const char* who, bool grouped, float* p, const float* g, float* m, float* v, float* ema,
                       const unsigned char* mask, int64_t n, float beta1, float beta2, float eps, float step_size,
                       float bc2_sqrt, float ema_w, float decay, float grad_scale, const float* dev_step,
                       void* shadow_bf16, const double* clip_state, void* stream) {
    QARIG_CHECK_ARG(p && g && m && v && n > 0 && n <= (1LL << 40), "%s: bad arguments", who);
    if (grouped) {
        const uintptr_t up = (uintptr_t)p, ue = (uintptr_t)ema, us = (uintptr_t)shadow_bf16;
        QARIG_CHECK_ARG(up % 16 == 0 && (uintptr_t)g % 16 == 0 && (uintptr_t)m % 16 == 0 && (uintptr_t)v % 16 == 0 &&
                            ue % 16 == 0 && us % 16 == 0,
                        "%s: p, g, m, v, ema and shadow_bf16 must be 16-byte aligned", who);
        QARIG_CHECK_ARG((uintptr_t)clip_state % 8 == 0, "%s: clip_state must be 8-byte aligned", who);
        QARIG_CHECK_ARG(!mask || (decay >= 0.0f && decay < 1.0f), "%s: decay must lie in [0, 1)", who);  // (NaN fails)
        const uint64_t bytes = 4 * (uint64_t)n;
        QARIG_CHECK_ARG(!ema || ue + bytes <= up || up + bytes <= ue, "%s: ema overlaps p", who);
        QARIG_CHECK_ARG(!shadow_bf16 || us + bytes / 2 <= up || up + bytes <= us, "%s: shadow_bf16 overlaps p", who);
    }
    int64_t b = ((grouped ? (n + 7) / 8 : n) + 255) / 256;
    if (b > 8192) b = 8192;
    unsigned short* shadow = (unsigned short*)shadow_bf16;
    if (grouped) {
        const auto kernel = clip_state ? (ema ? adam_groups_kernel<true, true> : adam_groups_kernel<false, true>)
                                       : (ema ? adam_groups_kernel<true, false> : adam_groups_kernel<false, false>);
        hipLaunchKernelGGL(kernel, dim3((int)b), dim3(256), 0, (hipStream_t)stream, p, g, m, v, ema, mask, n, beta1,
                           beta2, eps, step_size, bc2_sqrt, ema_w, decay, grad_scale, dev_step, shadow, clip_state);
    } else {
        const auto kernel = ema ? adam_kernel<true> : adam_kernel<false>;
        hipLaunchKernelGGL(kernel, dim3((int)b), dim3(256), 0, (hipStream_t)stream, p, g, m, v, ema, n, beta1, beta2,
                           eps, step_size, bc2_sqrt, ema_w, grad_scale, dev_step, shadow);
    }
    QARIG_CHECK_LAUNCH(who);
    return QARIG_OK;
}

extern "C" int qarig_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float beta1,
                               float beta2, float eps, float step_size, float bc2_sqrt,
                               float grad_scale, const float* dev_step, void* shadow_bf16, void* stream) {
    return adam_launch("adam", false, p, g, m, v, nullptr, nullptr, n, beta1, beta2, eps, step_size, bc2_sqrt, 0.0f,
                       0.0f, grad_scale, dev_step, shadow_bf16, nullptr, stream);
}

// dev_step here holds 3 floats, {step_size, bc2_sqrt, ema_w}
extern "C" int qarig_adam_ema_step(float* p, const float* g, float* m, float* v, float* ema, int64_t n,
                                   float beta1, float beta2, float eps, float step_size, float bc2_sqrt,
                                   float ema_w, float grad_scale, const float* dev_step, void* shadow_bf16,
                                   void* stream) {
    QARIG_CHECK_ARG(ema, "adam_ema: bad arguments");
    return adam_launch("adam_ema", false, p, g, m, v, ema, nullptr, n, beta1, beta2, eps, step_size, bc2_sqrt, ema_w,
                       0.0f, grad_scale, dev_step, shadow_bf16, nullptr, stream);
}

// ema may be NULL; dev_step, when given, is always four floats {step_size, bc2_sqrt, ema_w, decay}, here and below
extern "C" int qarig_adamw_step(float* p, const float* g, float* m, float* v, float* ema,
                                const unsigned char* decay_mask, int64_t n, float beta1, float beta2, float eps,
                                float step_size, float bc2_sqrt, float ema_w, float decay, float grad_scale,
                                const float* dev_step, void* shadow_bf16, void* stream) {
    QARIG_CHECK_ARG(decay_mask, "adamw: bad arguments");
    return adam_launch("adamw", true, p, g, m, v, ema, decay_mask, n, beta1, beta2, eps, step_size, bc2_sqrt, ema_w,
                       decay, grad_scale, dev_step, shadow_bf16, nullptr, stream);
}

// Global gradient norm and clip coefficient (include/qarig.h has the normative arithmetic): two launches, the
// streaming sum of squares into at most GRAD_NORM_PARTIALS fp64 partials, then one workgroup that adds them and
// writes state = {norm, coef, skipped, clipped}.  partials: GRAD_NORM_PARTIALS doubles; state: four doubles.
extern "C" int qarig_grad_clip_coef(const float* g, int64_t n, float grad_scale, double max_norm, double* partials,
                                    double* state, void* stream) {
    QARIG_CHECK_ARG(g && partials && state && n > 0 && n <= (1LL << 40), "grad_clip_coef: bad arguments");
    QARIG_CHECK_ARG((uintptr_t)g % 16 == 0, "grad_clip_coef: g must be 16-byte aligned");
    QARIG_CHECK_ARG((uintptr_t)partials % 8 == 0 && (uintptr_t)state % 8 == 0,
                    "grad_clip_coef: partials and state must be 8-byte aligned");
    QARIG_CHECK_ARG(max_norm > 0.0, "grad_clip_coef: max_norm must be > 0 (inf: guard only)");     // (NaN fails)
    QARIG_CHECK_ARG(grad_scale - grad_scale == 0.0f, "grad_clip_coef: grad_scale must be finite");
    const int64_t per_block = 4 * (int64_t)GRAD_NORM_BLOCK;
    int64_t b = (n + per_block - 1) / per_block;
    if (b > GRAD_NORM_PARTIALS) b = GRAD_NORM_PARTIALS;
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3((int)b), dim3(GRAD_NORM_BLOCK), 0, (hipStream_t)stream, g, n,
                       grad_scale, partials);
    QARIG_CHECK_LAUNCH("grad_clip_coef");
    hipLaunchKernelGGL(grad_clip_coef_kernel, dim3(1), dim3(GRAD_NORM_BLOCK), 0, (hipStream_t)stream,
                       (const double*)partials, (int)b, max_norm, state);
    QARIG_CHECK_LAUNCH("grad_clip_coef");
    return QARIG_OK;
}

// decay_mask may be NULL here (no decay: the host decay is not looked at)
extern "C" int qarig_adam_clip_step(float* p, const float* g, float* m, float* v, float* ema,
                                    const unsigned char* decay_mask, int64_t n, float beta1, float beta2, float eps,
                                    float step_size, float bc2_sqrt, float ema_w, float decay, float grad_scale,
                                    const float* dev_step, void* shadow_bf16, const double* clip_state,
                                    void* stream) {
    QARIG_CHECK_ARG(clip_state, "adam_clip: bad arguments");
    return adam_launch("adam_clip", true, p, g, m, v, ema, decay_mask, n, beta1, beta2, eps, step_size, bc2_sqrt,
                       ema_w, decay, grad_scale, dev_step, shadow_bf16, clip_state, stream);
}

// a <-> b, n floats each, bit-exact.  The buffers must not overlap (refused).
extern "C" int qarig_swap_f32(float* a, float* b, int64_t n, void* stream) {
    QARIG_CHECK_ARG(a && b && n > 0 && n <= (1LL << 40), "swap_f32: bad arguments");
    const uintptr_t ua = (uintptr_t)a, ub = (uintptr_t)b;
    QARIG_CHECK_ARG(ua % 4 == 0 && ub % 4 == 0, "swap_f32: buffers must be 4-byte aligned");
    QARIG_CHECK_ARG(ua + 4 * (uint64_t)n <= ub || ub + 4 * (uint64_t)n <= ua, "swap_f32: buffers overlap");
    const int64_t nvec = (ua % 16 == 0 && ub % 16 == 0) ? n / 4 : 0;
    const int64_t work = nvec > n - 4 * nvec ? nvec : n - 4 * nvec;
    int64_t blocks = (work + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(swap_f32_kernel, dim3((int)blocks), dim3(256), 0, (hipStream_t)stream, (unsigned*)a,
                       (unsigned*)b, nvec, n);
    QARIG_CHECK_LAUNCH("swap_f32");
    return QARIG_OK;
}
