// The least-squares plane w = alpha x + beta y + gamma over the samples of up to 32 sets at once, shared by the planes of the glass
// regions (regions.hip: the network's depth inside a region) and of the sensor fusion (fusion.hip: the sensor's depth on the ring
// around it) so that both fit by the same method, to the same exactness (DESIGN.md sections 23 and 26):
//   * ten moments per set, coordinates RELATIVE to an origin (ox, oy) that no sample lies left of or above, so dx, dy are in
//     [0, 2^14): the six integer moments are exact in int64 (n < 2^28 samples: sum dx^2 < 2^56), and n Sxx - Sx^2 etc. are exact in
//     128 bits.  regions.hip takes the corner (x0, y0) of the region's box; fusion.hip takes (max(x0 - ring, 0), max(y0 - ring, 0)):
//     a ring pixel has a pixel of its region within `ring` columns and rows, so it lies at or right of / below that corner and
//     the argument carries over unchanged;
//   * the four fp64 moments are summed in a fixed order: 64 lanes by the xor butterfly, a wave's rounds in the order it walks its
//     pixels, the four waves as (0 + 1) + (2 + 3), the workgroups ascending - no atomics, so a call repeats its bits;
//   * collinear samples are decided in integers (determinant of the centred second moments == 0), never by a float threshold.
// Every function that rounds switches contraction off for itself: the including file's own setting does not reach in here.
#pragma once
#include "common.h"

constexpr int kFitNI = 6, kFitND = 4;                     // integer / fp64 moments of a partial record
constexpr int kFitRec = kFitNI + kFitND;

__device__ __forceinline__ long long wave_sum_ll(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// One round of a wave: the lanes with `mine` hold a sample (dx, dy, w) of ONE set; every lane of the wave calls (others pass 0, 0,
// 0.0).  pi / pd: the wave's record of that set in LDS.
__device__ __forceinline__ void fit_add_moments(bool mine, long long dx, long long dy, double w, int lane, long long *pi, double *pd) {
#pragma clang fp contract(off)
    const long long vi[kFitNI] = {mine ? 1 : 0, dx, dy, dx * dx, dx * dy, dy * dy};
    const double vd[kFitND] = {w, (double)dx * w, (double)dy * w, w * w};
#pragma unroll
    for (int k = 0; k < kFitNI; ++k) {
        const long long s = wave_sum_ll(vi[k]);
        if (lane == 0) pi[k] += s;
    }
#pragma unroll
    for (int k = 0; k < kFitND; ++k) {
        const double s = wave_sum_d(vd[k]);
        if (lane == 0) pd[k] += s;
    }
}

// the residual of a sample at ABSOLUTE (x, y) against stored coefficients
__device__ __forceinline__ double fit_residual(double w, double ca, double cb, double cg, int x, int y) {
#pragma clang fp contract(off)
    return w - ((ca * (double)x + cb * (double)y) + cg);
}

// the same round for the sum of squared residuals (e = 0.0 in the lanes without a sample), kept in pd[0]
__device__ __forceinline__ void fit_add_residual(double e, int lane, double *pd) {
#pragma clang fp contract(off)
    const double s = wave_sum_d(e * e);
    if (lane == 0) pd[0] += s;
}

// the workgroup's partial record of `sets` sets: the four waves in order; every entry written
__device__ __forceinline__ void fit_store_partial(const long long (*pi)[32][kFitNI], const double (*pd)[32][kFitND], long long *out,
                                                  int sets, int tid, int threads) {
#pragma clang fp contract(off)
    for (int k = tid; k < sets * kFitRec; k += threads) {
        const int r = k / kFitRec, q = k - r * kFitRec;
        if (q < kFitNI) out[k] = (pi[0][r][q] + pi[1][r][q]) + (pi[2][r][q] + pi[3][r][q]);
        else ((double *)out)[k] = (pd[0][r][q - kFitNI] + pd[1][r][q - kFitNI]) + (pd[2][r][q - kFitNI] + pd[3][r][q - kFitNI]);
    }
}

// lane q < kFitRec folds moment q of one set over the nb partial records (`stride` 8-byte values apart), ascending
__device__ __forceinline__ void fit_fold(const long long *part, int nb, int64_t stride, int q, long long *si, double *sd) {
#pragma clang fp contract(off)
    if (q < kFitNI) {
        long long s = 0;
        for (int k = 0; k < nb; ++k) s += part[(int64_t)k * stride + q];
        si[q] = s;
    } else if (q < kFitRec) {
        double s = 0.0;
        for (int k = 0; k < nb; ++k) s += ((const double *)part)[(int64_t)k * stride + q];
        sd[q - kFitNI] = s;
    }
}

typedef unsigned __int128 u128;
__device__ __forceinline__ double to_double(u128 v) {      // two exact halves, one rounding each
    return (double)(unsigned long long)(v >> 64) * 18446744073709551616.0 + (double)(unsigned long long)v;
}
// a * b of two 128-bit values as (high, low) 128-bit halves
__device__ inline void mul128(u128 a, u128 b, u128 &hi, u128 &lo) {
    const u128 mask = ((u128)1 << 64) - 1;
    const u128 a0 = a & mask, a1 = a >> 64, b0 = b & mask, b1 = b >> 64;
    const u128 p00 = a0 * b0, p01 = a0 * b1, p10 = a1 * b0, p11 = a1 * b1;
    const u128 mid = (p00 >> 64) + (p01 & mask) + (p10 & mask);
    lo = (p00 & mask) | (mid << 64);
    hi = p11 + (p01 >> 64) + (p10 >> 64) + (mid >> 64);
}

struct PlaneFit {
    double alpha, beta, gamma, n;                         // gamma in ABSOLUTE coordinates; NaN coefficients with flat
    bool flat;                                            // fewer than 3 samples, or collinear ones
};

// the folded moments of one set, taken relative to (ox, oy) -> its plane
__device__ inline PlaneFit fit_solve(const long long *si, const double *sd, long long ox, long long oy) {
#pragma clang fp contract(off)
    PlaneFit f;
    const long long n = si[0], Sx = si[1], Sy = si[2];
    const double nan = __builtin_nan("");
    bool flat = n < 3;
    u128 Dxx = 0, Dyy = 0;
    __int128 Dxy = 0;
    if (!flat) {                                          // n * Sxx - Sx^2 etc. are exact: coordinates < 2^14, n < 2^28
        Dxx = (u128)n * (u128)si[3] - (u128)Sx * (u128)Sx;
        Dyy = (u128)n * (u128)si[5] - (u128)Sy * (u128)Sy;
        Dxy = (__int128)n * si[4] - (__int128)Sx * Sy;
        const u128 axy = Dxy < 0 ? (u128)(-Dxy) : (u128)Dxy;
        u128 h1, l1, h2, l2;
        mul128(Dxx, Dyy, h1, l1);
        mul128(axy, axy, h2, l2);
        flat = h1 == h2 && l1 == l2;                      // the determinant is never negative (Cauchy-Schwarz): zero = collinear
    }
    f.flat = flat;
    f.n = (double)n;
    if (flat) {
        f.alpha = f.beta = f.gamma = nan;
        return f;
    }
    const double dn = (double)n, dSx = (double)Sx, dSy = (double)Sy, Sw = sd[0];
    const double dxx = to_double(Dxx), dyy = to_double(Dyy), dxy = Dxy < 0 ? -to_double((u128)(-Dxy)) : to_double((u128)Dxy);
    const double dxw = dn * sd[1] - dSx * Sw, dyw = dn * sd[2] - dSy * Sw;
    const double det = dxx * dyy - dxy * dxy;
    const double alpha = (dyy * dxw - dxy * dyw) / det, beta = (dxx * dyw - dxy * dxw) / det;
    const double gamma_rel = (Sw - alpha * dSx - beta * dSy) / dn;
    f.alpha = alpha;
    f.beta = beta;
    f.gamma = gamma_rel - alpha * (double)ox - beta * (double)oy;
    return f;
}
