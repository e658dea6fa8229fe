// Line probe geometry shared by the device kernel (csrc/lineprofile.hip) and a host build (tests/lineprobe_host.cpp): how many
// samples a line gets, where the three probes of a sample lie (on the line, `offset` pixels to either side of it) and which pixel
// a probe reads, as plain scalar functions (tests/line_profile_ref.py states the same in numpy).
//
// Everything is fp64 and every operation is rounded on its own - no contraction: a * b + c stays two roundings, as numpy has it -
// so the host build, the numpy statement and the kernel put every probe into the same pixel bit for bit (division and square root
// are correctly rounded on all three).
#pragma once
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
#if defined(__HIPCC__)
#define LP_HD __host__ __device__ __forceinline__
#else
#include <cmath>
#define LP_HD inline
#endif

struct LpLine {
    double x1, y1, dx, dy;                                // on(t) = (x1 + t dx, y1 + t dy)
    double ox, oy;                                        // a = on + (ox, oy), b = on - (ox, oy): offset * (-dy / L, dx / L)
    int n;                                                // samples 0 .. n at t = k / n; 0: a degenerate line
};

// n: the smallest integer >= 1 with n * n >= L2, limited to max_samples - 1 (2 <= max_samples <= 2048); 0 when L2 is not a positive
// finite number.  The candidate comes from a square root and is corrected against n * n, which is exact (n <= 2047), so the last
// bit of the root changes nothing.
LP_HD int lp_sample_count(double L2, int max_samples) {
    if (!(L2 > 0.0) || L2 > 1.7976931348623157e308) return 0;
    const int cap = max_samples - 1;
    if (L2 >= (double)(cap * cap)) return cap;
    int n = (int)ceil(sqrt(L2));                          // L2 < 2047^2
    while (n > 1 && (double)((n - 1) * (n - 1)) >= L2) --n;
    while ((double)(n * n) < L2) ++n;
    return n < 1 ? 1 : n;
}

LP_HD LpLine lp_line(double x1, double y1, double x2, double y2, double offset, int max_samples) {
    LpLine l;
    l.x1 = x1, l.y1 = y1, l.dx = x2 - x1, l.dy = y2 - y1;
    const double L2 = l.dx * l.dx + l.dy * l.dy;
    l.n = lp_sample_count(L2, max_samples);
    l.ox = l.oy = 0.0;
    if (l.n) {
        const double L = sqrt(L2);
        l.ox = offset * (-l.dy / L);
        l.oy = offset * (l.dx / L);
    }
    return l;
}

LP_HD double lp_t(const LpLine &l, int k) { return (double)k / (double)l.n; }

// probe 0 = on the line, 1 = side a, 2 = side b, of sample k
LP_HD void lp_probe(const LpLine &l, int k, int probe, double &x, double &y) {
    const double t = lp_t(l, k);
    x = l.x1 + t * l.dx;
    y = l.y1 + t * l.dy;
    if (probe == 1) { x = x + l.ox; y = y + l.oy; }
    if (probe == 2) { x = x - l.ox; y = y - l.oy; }
}

// the pixel (floor x, floor y) as iy * pitch + ix, or -1 when it lies outside the fh x fw frame (NaN and infinities are outside);
// the comparisons run on the doubles, so no conversion ever overflows
LP_HD long long lp_pixel(double x, double y, int fh, int fw, int pitch) {
    if (!(x >= 0.0 && x < (double)fw && y >= 0.0 && y < (double)fh)) return -1;
    return (long long)(int)y * pitch + (int)x;
}
