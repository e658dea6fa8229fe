// Render geometry shared by the device kernel (csrc/render.hip) and a host build (tests/rendergeom_host.cpp): how a line's ends are
// quantised, which pixels a row of given width covers, which tiles it can touch and which table entry a score takes, as plain scalar
// functions (tests/render_ref.py states the same in numpy).
//
// Ends live on a 1/16 pixel grid, X = floor(16 x + 0.5) (16 x is exact, so the sum is rounded once however it is contracted), pixel
// (ix, iy) is the point (16 ix + 8, 16 iy + 8), and everything after the quantisation is integer arithmetic that fits int64:
// |X| <= 2^19 + 1, a pixel coordinate < 2^19, so a difference is below 2^20.1, a dot or cross product below 2^41.2, L2 below 2^41.2;
// with h <= 1024 (the widest disc) h^2 L2 < 2^61.2.  No square root is taken anywhere.
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#define RG_HD __host__ __device__ __forceinline__
#else
#define RG_HD inline
#endif

struct RgRow {
    int32_t ax, ay, bx, by;                               // the two ends in 1/16 pixel
};

constexpr double RG_MAX_COORD = 32767.0;                  // a row with a larger |coordinate|, or a non-finite one, is not drawn

// false: the row is not drawn.  The comparisons run on the doubles (NaN and infinities fail them), so no conversion overflows.
RG_HD bool rg_quantise(double x1, double y1, double x2, double y2, RgRow &r) {
    if (!(x1 >= -RG_MAX_COORD && x1 <= RG_MAX_COORD && y1 >= -RG_MAX_COORD && y1 <= RG_MAX_COORD && x2 >= -RG_MAX_COORD &&
          x2 <= RG_MAX_COORD && y2 >= -RG_MAX_COORD && y2 <= RG_MAX_COORD))
        return false;
    r.ax = (int32_t)__builtin_floor(16.0 * x1 + 0.5);
    r.ay = (int32_t)__builtin_floor(16.0 * y1 + 0.5);
    r.bx = (int32_t)__builtin_floor(16.0 * x2 + 0.5);
    r.by = (int32_t)__builtin_floor(16.0 * y2 + 0.5);
    return true;
}

// the point (px, py) (1/16 pixel) lies within r (r2 = r r) of the point (cx, cy); ties are inside
RG_HD bool rg_disc(int32_t cx, int32_t cy, int32_t px, int32_t py, int64_t r2) {
    const int64_t qx = (int64_t)px - cx, qy = (int64_t)py - cy;
    return qx * qx + qy * qy <= r2;
}

// the point lies within h (h2 = h h) of the segment A B: round caps, ties inside, a zero-length row is a disc
RG_HD bool rg_covered(const RgRow &r, int32_t px, int32_t py, int64_t h2) {
    const int64_t dx = (int64_t)r.bx - r.ax, dy = (int64_t)r.by - r.ay;
    const int64_t qx = (int64_t)px - r.ax, qy = (int64_t)py - r.ay;
    const int64_t L2 = dx * dx + dy * dy, t = qx * dx + qy * dy;
    if (t <= 0) return qx * qx + qy * qy <= h2;
    if (t >= L2) return rg_disc(r.bx, r.by, px, py, h2);
    const int64_t cr = qx * dy - qy * dx;                 // |cr| = distance to the line * |d|
    if (cr >= ((int64_t)1 << 31) || cr <= -((int64_t)1 << 31)) return false;      // cr^2 >= 2^62 > h2 L2: exact, and cr cr fits
    return cr * cr <= h2 * L2;
}

// Conservative: false only when NO pixel ix in [x0, x1], iy in [y0, y1] can be covered by the row at half width m (1/16 pixel,
// the larger of the line's half width and the end discs' radius).  A covered pixel lies within m of the segment, hence inside the
// segment's bounding box grown by m, and within m of the infinite line: when the four corners of the rectangle of pixel centres lie
// strictly on one side of the line and each is further than m from it, every point between them is (the signed distance is affine).
RG_HD bool rg_tile_may_touch(const RgRow &r, int32_t x0, int32_t y0, int32_t x1, int32_t y1, int32_t m) {
    const int32_t lx = 16 * x0 + 8, hx = 16 * x1 + 8, ly = 16 * y0 + 8, hy = 16 * y1 + 8;
    const int32_t minx = r.ax < r.bx ? r.ax : r.bx, maxx = r.ax < r.bx ? r.bx : r.ax;
    const int32_t miny = r.ay < r.by ? r.ay : r.by, maxy = r.ay < r.by ? r.by : r.ay;
    if (maxx + m < lx || minx - m > hx || maxy + m < ly || miny - m > hy) return false;
    const int64_t dx = (int64_t)r.bx - r.ax, dy = (int64_t)r.by - r.ay;
    const int64_t lim = (int64_t)m * m * (dx * dx + dy * dy);
    int pos = 0, neg = 0;
    for (int k = 0; k < 4; ++k) {
        const int64_t qx = (int64_t)((k & 1) ? hx : lx) - r.ax, qy = (int64_t)((k & 2) ? hy : ly) - r.ay;
        const int64_t cr = qx * dy - qy * dx;
        const bool big = cr >= ((int64_t)1 << 31) || cr <= -((int64_t)1 << 31);
        if (!big && cr * cr <= lim) return true;          // a corner within m of the line
        pos += cr > 0, neg += cr < 0;
    }
    return pos != 4 && neg != 4;                          // the line passes between the corners
}

// the table entry of a score: clamp(floor((s - lo) k), 0, 255), k = 256 / (hi - lo) formed by the caller; two fp64 operations,
// each rounded on its own (the product is not contracted into the difference: there is nothing to contract it with)
RG_HD int32_t rg_score_index(double s, double lo, double k) {
    const double v = (s - lo) * k;
    if (!(v >= 1.0)) return 0;                            // below the range, and NaN
    if (v >= 255.0) return 255;
    return (int32_t)v;                                    // v >= 1: truncation is the floor
}
