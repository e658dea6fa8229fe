// The AdamW element update and the clip coefficient, written once: adamw_kernel (optim.hip), adamw_guarded_kernel (health.hip) and
// adamw_ema_kernel (ema.hip) call these two functions and nothing else per element, so that p, m, v and the bf16 shadow are the same
// bits whichever entry point ran the step (tests/test_ema_gpu.py holds the three against each other).
//
// Every fused multiply-add is spelled out and contraction is off inside the two functions: which products of
//     m + (gi - m)(1 - b1),   v b2 + gi gi (1 - b2),   p (1 - lr wd) - update
// the compiler fuses otherwise depends on the code around the expression (a scalar loop and a float4 body fused different ones).
// The forms below are the ones the scalar kernels have always compiled to.
#pragma once
#include "common.h"

// grad_scale * clip_coef: torch.nn.utils.clip_grad_norm_, clip_coef = max_norm / (total_norm + 1e-6), clamped to 1; sq may be NULL
__device__ __forceinline__ float adamw_coef(const double *sq, float max_norm, float grad_scale) {
#pragma clang fp contract(off)
    float coef = grad_scale;
    if (sq && max_norm > 0.f) {
        const float total = (float)sqrt(sq[0]);
        coef *= fminf(max_norm / __builtin_fmaf(total, grad_scale, 1e-6f), 1.0f);
    }
    return coef;
}

// step = lr / bc1, rs2 = rsqrtf(bc2); pi, mi, vi hold the stored values on entry and the new ones on return
__device__ __forceinline__ void adamw_element(float &pi, float g, float &mi, float &vi, float coef, float lr, float b1, float b2,
                                              float eps, float wd, float step, float rs2) {
#pragma clang fp contract(off)
    const float gi = g * coef;
    const float mn = __builtin_fmaf(1.0f - b1, __builtin_fmaf(g, coef, -mi), mi);      // lerp, as torch's exp_avg.lerp_
    const float vn = __builtin_fmaf(1.0f - b2, gi * gi, vi * b2);
    const float update = step * mn / __builtin_fmaf(sqrtf(vn), rs2, eps);
    pi = __builtin_fmaf(__builtin_fmaf(-lr, wd, 1.0f), pi, -update);
    mi = mn;
    vi = vn;
}
