// The Adam / AdamW update of one element and the shadow's bf16 conversion, in plain C++ for host and device.  Every
// Adam kernel of csrc/optim.hip calls them; tests/test_adamw_host.py and tests/test_grad_clip_host.py compile this
// header for the host alone and hold it, bit for bit, to the NumPy emulations that the tolerances are derived from.
// Needs -ffp-contract=off (the one fused operation is the explicit fma).
//
// The element update, normative: every operation rounds to fp32, in this order.
//   pd    = fma(-decay, p, p) where the element is decayed (one rounding; decay = fp32(lr * lambda)), else p's bits
//   gi    = graw * grad_scale;   w = 1 - beta1
//   mn    = w < 0.5 ? m + w (gi - m) : gi - (gi - m) (1 - w)     exp_avg.lerp_(grad, w), torch's two-branch lerp
//   vn    = v beta2 + (1 - beta2) gi gi                          exp_avg_sq.mul_(beta2).addcmul_(grad, grad, 1 - beta2)
//   denom = sqrt(vn) / bc2_sqrt + eps;   pn = pd - step_size (mn / denom)
//   en    = the same two-branch lerp of e towards pn by ema_w (EMA only): ema_w = 1 yields pn, ema_w = 0 keeps e,
//           and e == pn stays, all exactly
#pragma once
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define QARIG_HD __host__ __device__
#else
#define QARIG_HD
#endif

namespace qarig {

// mi, vi and (EMA) ei are updated in place; returns pn.
template <bool EMA>
QARIG_HD inline float adam_element(float pi, float graw, float& mi, float& vi, float& ei, bool decayed, float beta1,
                                   float beta2, float eps, float step_size, float bc2_sqrt, float ema_w, float decay,
                                   float grad_scale) {
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

// two floats -> two nearest-even bf16 in one dword (low half: a)
QARIG_HD inline unsigned pack_bf16x2(float a, float b) {
    typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
    typedef float f32x2_t __attribute__((ext_vector_type(2)));
    const f32x2_t f = {a, b};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(f, bf16x2_t));
}

}  // namespace qarig
