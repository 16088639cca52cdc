// Adam step over one flat fp32 buffer (all parameters of a model live in one
// allocation; so do their gradients and moments): one launch per step, and the same
// flat gradient buffer is what the DP all-reduce moves.  Semantics of
// torch.optim.Adam(lr, betas) without weight decay / amsgrad
// (train_quantized_transformer.py:317-320; train_autoencoder.py:133-136).  Additive: adamw_kernel, the same update
// behind a decoupled weight decay of the groups a mask selects (torch.optim.AdamW with two parameter groups).
#include "qarig_common.h"

namespace qarig {

// EMA: the same pass also moves an exponential moving average of the parameters, e <- lerp(e, pn, ema_w),
// one more read and one more write stream on the launch (7 -> 9), no further launch.  p, m, v and the shadow
// are computed by the very expressions of the plain instantiation.
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
        const float gi = g[i] * grad_scale;
        // exp_avg.lerp_(grad, 1 - beta1), torch's two-branch lerp
        const float w = 1.0f - beta1;
        const float mi = m[i];
        const float mn = w < 0.5f ? mi + w * (gi - mi) : gi - (gi - mi) * (1.0f - w);
        // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
        const float vn = v[i] * beta2 + (1.0f - beta2) * gi * gi;
        const float denom = sqrtf(vn) / bc2_sqrt + eps;
        const float pn = p[i] - step_size * (mn / denom);
        p[i] = pn;
        m[i] = mn;
        v[i] = vn;
        if (EMA) {
            // the two-branch lerp again: ema_w = 1 yields pn, ema_w = 0 keeps e, and e == pn stays, all exactly
            const float ei = ema[i];
            ema[i] = ema_w < 0.5f ? ei + ema_w * (pn - ei) : pn - (pn - ei) * (1.0f - ema_w);
        }
        if (shadow) {       // reduced-precision mode: the bf16 copy the GEMMs read, from the same pass
            typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
            typedef float f32x2_t __attribute__((ext_vector_type(2)));
            const f32x2_t f = {pn, 0.0f};
            shadow[i] = (unsigned short)(__builtin_bit_cast(unsigned, __builtin_convertvector(f, bf16x2_t)) & 0xffffu);
        }
    }
}

// AdamW: decoupled weight decay in front of the same update, on groups of 8 elements.  One element's arithmetic:
// pd = fma(-decay, p, p) where the element is decayed (one rounding; decay = fp32(lr * lambda)), p's own bits
// where it is not, then adam_kernel's expressions with pd in the place of p[i].  Returns the new parameter.
template <bool EMA>
__device__ __forceinline__ float adamw_element(float pi, float graw, float& mi, float& vi, float& ei, bool decayed,
                                               float beta1, float beta2, float eps, float step_size,
                                               float bc2_sqrt, float ema_w, float decay, float grad_scale) {
    const float pd = decayed ? __builtin_fmaf(-decay, pi, pi) : pi;
    const float gi = graw * grad_scale;
    const float w = 1.0f - beta1;
    const float mn = w < 0.5f ? mi + w * (gi - mi) : gi - (gi - mi) * (1.0f - w);
    const float vn = vi * beta2 + (1.0f - beta2) * gi * gi;
    const float denom = sqrtf(vn) / bc2_sqrt + eps;
    const float pn = pd - step_size * (mn / denom);
    mi = mn;
    vi = vn;
    if (EMA) ei = ema_w < 0.5f ? ei + ema_w * (pn - ei) : pn - (pn - ei) * (1.0f - ema_w);
    return pn;
}

// two floats -> two nearest-even bf16 in one dword (low half: a), the conversion of adam_kernel's shadow
__device__ __forceinline__ unsigned pack_bf16x2(float a, float b) {
    typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
    typedef float f32x2_t __attribute__((ext_vector_type(2)));
    const f32x2_t f = {a, b};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(f, bf16x2_t));
}

// One thread-iteration = one group of 8 elements = one mask byte: two 16-byte loads per input stream, all of them
// ahead of the first store, two 16-byte stores per fp32 output stream and one for the 8 bf16 of the shadow.  The
// last group of an n that is no multiple of 8 goes element by element and touches nothing at or behind n.
// 7 (9 with the EMA) streams of 4 bytes per element as adam_kernel, plus n / 8 mask bytes.
template <bool EMA>
__global__ void adamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                             float* __restrict__ v, float* __restrict__ ema,
                             const unsigned char* __restrict__ mask, int64_t n, float beta1, float beta2,
                             float eps, float step_size, float bc2_sqrt, float ema_w, float decay,
                             float grad_scale, const float* __restrict__ dev_step,
                             unsigned short* __restrict__ shadow) {
    if (dev_step) {     // captured-graph replay: always four floats {step_size, bc2_sqrt, ema_w, decay}
        step_size = dev_step[0];
        bc2_sqrt = dev_step[1];
        if (EMA) ema_w = dev_step[2];
        decay = dev_step[3];
    }
    const int64_t full = n >> 3, groups = (n + 7) >> 3;
    for (int64_t gr = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; gr < groups;
         gr += (int64_t)gridDim.x * blockDim.x) {
        const bool decayed = mask[gr] != 0;
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
                    pv[h][k] = adamw_element<EMA>(pv[h][k], gv[h][k], mi, vi, ei, decayed, beta1, beta2, eps,
                                                  step_size, bc2_sqrt, ema_w, decay, grad_scale);
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
                const float pn = adamw_element<EMA>(p[i], g[i], mi, vi, ei, decayed, beta1, beta2, eps, step_size,
                                                    bc2_sqrt, ema_w, decay, grad_scale);
                p[i] = pn;
                m[i] = mi;
                v[i] = vi;
                if (EMA) ema[i] = ei;
                if (shadow) shadow[i] = (unsigned short)(pack_bf16x2(pn, 0.0f) & 0xffffu);
            }
        }
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

// step_size = lr / (1 - beta1^t), bc2_sqrt = sqrt(1 - beta2^t), both computed by the
// host in double as torch does.  grad_scale multiplies g first (1/world after a sum
// all-reduce; 1 otherwise).  dev_step (optional, device, 2 floats {step_size, bc2_sqrt}) overrides
// the two per-step scalars, so that a captured graph of the training step can be replayed while
// the host refreshes them between replays.  shadow_bf16 (optional, n bf16 values): receives the updated
// parameters rounded to nearest-even bf16 -- the operands of the reduced-precision GEMMs -- so that no
// per-weight cast launch follows an optimiser step.
extern "C" int qarig_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float beta1,
                               float beta2, float eps, float step_size, float bc2_sqrt,
                               float grad_scale, const float* dev_step, void* shadow_bf16, void* stream) {
    QARIG_CHECK_ARG(p && g && m && v && n > 0 && n <= (1LL << 40), "adam: bad arguments");
    int64_t b = (n + 255) / 256;
    if (b > 8192) b = 8192;
    hipLaunchKernelGGL(adam_kernel<false>, dim3((int)b), dim3(256), 0, (hipStream_t)stream, p, g, m, v,
                       (float*)nullptr, n, beta1, beta2, eps, step_size, bc2_sqrt, 0.0f, grad_scale, dev_step,
                       (unsigned short*)shadow_bf16);
    QARIG_CHECK_LAUNCH("adam");
    return QARIG_OK;
}

// The same step with an exponential moving average of the parameters kept from the same pass:
// ema <- lerp(ema, p_new, ema_w), n floats, updated in place.  dev_step here holds 3 floats,
// {step_size, bc2_sqrt, ema_w}.  p, m, v and shadow_bf16 come out as qarig_adam_step leaves them.
extern "C" int qarig_adam_ema_step(float* p, const float* g, float* m, float* v, float* ema, int64_t n,
                                   float beta1, float beta2, float eps, float step_size, float bc2_sqrt,
                                   float ema_w, float grad_scale, const float* dev_step, void* shadow_bf16,
                                   void* stream) {
    QARIG_CHECK_ARG(p && g && m && v && ema && n > 0 && n <= (1LL << 40), "adam_ema: bad arguments");
    int64_t b = (n + 255) / 256;
    if (b > 8192) b = 8192;
    hipLaunchKernelGGL(adam_kernel<true>, dim3((int)b), dim3(256), 0, (hipStream_t)stream, p, g, m, v, ema, n,
                       beta1, beta2, eps, step_size, bc2_sqrt, ema_w, grad_scale, dev_step,
                       (unsigned short*)shadow_bf16);
    QARIG_CHECK_LAUNCH("adam_ema");
    return QARIG_OK;
}

// AdamW (include/qarig.h has the normative arithmetic): decay_mask holds one byte per group of 8 elements,
// ceil(n / 8) of them; ema may be NULL (the plain instantiation); dev_step, when given, is always four floats
// {step_size, bc2_sqrt, ema_w, decay} and the host's values of the four are ignored.
extern "C" int qarig_adamw_step(float* p, const float* g, float* m, float* v, float* ema,
                                const unsigned char* decay_mask, int64_t n, float beta1, float beta2, float eps,
                                float step_size, float bc2_sqrt, float ema_w, float decay, float grad_scale,
                                const float* dev_step, void* shadow_bf16, void* stream) {
    QARIG_CHECK_ARG(p && g && m && v && decay_mask && n > 0 && n <= (1LL << 40), "adamw: bad arguments");
    const uintptr_t up = (uintptr_t)p, ue = (uintptr_t)ema, us = (uintptr_t)shadow_bf16;
    QARIG_CHECK_ARG(up % 16 == 0 && (uintptr_t)g % 16 == 0 && (uintptr_t)m % 16 == 0 && (uintptr_t)v % 16 == 0 &&
                        ue % 16 == 0 && us % 16 == 0,
                    "adamw: p, g, m, v, ema and shadow_bf16 must be 16-byte aligned");
    QARIG_CHECK_ARG(decay >= 0.0f && decay < 1.0f, "adamw: decay must lie in [0, 1)");      // (NaN fails both)
    const uint64_t bytes = 4 * (uint64_t)n;
    QARIG_CHECK_ARG(!ema || ue + bytes <= up || up + bytes <= ue, "adamw: ema overlaps p");
    QARIG_CHECK_ARG(!shadow_bf16 || us + bytes / 2 <= up || up + bytes <= us, "adamw: shadow_bf16 overlaps p");
    int64_t b = ((n + 7) / 8 + 255) / 256;
    if (b > 8192) b = 8192;
    if (ema)
        hipLaunchKernelGGL(adamw_kernel<true>, dim3((int)b), dim3(256), 0, (hipStream_t)stream, p, g, m, v, ema,
                           decay_mask, n, beta1, beta2, eps, step_size, bc2_sqrt, ema_w, decay, grad_scale,
                           dev_step, (unsigned short*)shadow_bf16);
    else
        hipLaunchKernelGGL(adamw_kernel<false>, dim3((int)b), dim3(256), 0, (hipStream_t)stream, p, g, m, v,
                           (float*)nullptr, decay_mask, n, beta1, beta2, eps, step_size, bc2_sqrt, 0.0f, decay,
                           grad_scale, dev_step, (unsigned short*)shadow_bf16);
    QARIG_CHECK_LAUNCH("adamw");
    return QARIG_OK;
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
