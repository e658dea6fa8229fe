// The per-pixel arithmetic of the dense evaluation, shared by eval_partial_kernel (evalmetrics.hip) and eval_frames_kernel
// (evalframes.hip) so that the two agree bit for bit: the clamp of src/engine_glassrgbd.py:249-252 in that order, the validity
// test of :253 and the ten terms of compute_depth_errors (src/util/metrics.py:198-218), each formed in fp32 with IEEE division.
#pragma once
#include "common.h"

__device__ __forceinline__ float log_rn(float v) { return (float)log((double)v); }        // = correctly rounded logf
__device__ __forceinline__ float log10_rn(float v) { return (float)log10((double)v); }

// engine_glassrgbd.py:249-252, in that order; a NaN fails both comparisons and is caught last
__device__ __forceinline__ float eval_clamp(float p, float dmin, float dmax) {
    if (p < dmin) p = dmin;
    if (p > dmax) p = dmax;
    if (p != p) p = dmin;
    return p;
}

__device__ __forceinline__ bool eval_valid(float g, float dmin, float dmax) { return g > dmin && g < dmax; }      // :253

// t[0] = 1, t[1..3] = threshold hits (0 / 1), then sq, abs_rel, sq_rel, err, err^2, |log10 diff| of one valid pixel
__device__ __forceinline__ void eval_terms(float g, float p, float (&t)[GWD_EVAL_NSUM]) {
    const float thr = fmaxf(__fdiv_rn(g, p), __fdiv_rn(p, g));
    const float diff = g - p, sq = diff * diff;
    const float err = log_rn(p) - log_rn(g);
    t[0] = 1.0f;
    t[1] = thr < 1.25f ? 1.0f : 0.0f;
    t[2] = thr < 1.5625f ? 1.0f : 0.0f;
    t[3] = thr < 1.953125f ? 1.0f : 0.0f;
    t[4] = sq;
    t[5] = __fdiv_rn(fabsf(diff), g);
    t[6] = __fdiv_rn(sq, g);
    t[7] = err;
    t[8] = err * err;
    t[9] = fabsf(log10_rn(p) - log10_rn(g));
}

// The nine measures of engine_glassrgbd.py:204 from the ten sums; n == 0: every measure is NaN, as numpy's mean of an empty array
// (no contraction: the host forms me2 - me * me from two rounded operations, and so does this)
__device__ __forceinline__ void eval_measures(const double (&s)[GWD_EVAL_NSUM], double *m) {
#pragma clang fp contract(off)
    const double n = s[0];
    const double me = s[7] / n, me2 = s[8] / n;
    m[0] = sqrt(me2 - me * me) * 100.0;          // silog
    m[1] = s[5] / n;                             // abs_rel
    m[2] = s[9] / n;                             // log10
    m[3] = sqrt(s[4] / n);                       // rms
    m[4] = s[6] / n;                             // sq_rel
    m[5] = sqrt(me2);                            // log_rms  ((log g - log p)^2 == err^2)
    m[6] = s[1] / n;
    m[7] = s[2] / n;
    m[8] = s[3] / n;
}
