// Host build of gw_depth_amd/csrc/rendergeom.h for tests/test_render.py: the same scalar functions the device kernel calls, driven by
// plain loops.  Built by the test with g++ -ffp-contract=off into a shared object and called through ctypes.
#include "rendergeom.h"

// -> 1 and q[4] = the quantised ends, or 0: the row is not drawn
extern "C" int rg_host_quantise(const double *line, int32_t *q) {
    RgRow r;
    if (!rg_quantise(line[0], line[1], line[2], line[3], r)) return 0;
    q[0] = r.ax, q[1] = r.ay, q[2] = r.bx, q[3] = r.by;
    return 1;
}

// cover[iy * fw + ix] = 1 where pixel (ix, iy) lies within h of the segment q, | 2 where it lies within radius (1/16 pixel) of an end
extern "C" void rg_host_cover(const int32_t *q, int32_t h, int32_t radius, int32_t fh, int32_t fw, uint8_t *cover) {
    const RgRow r{q[0], q[1], q[2], q[3]};
    for (int iy = 0; iy < fh; ++iy)
        for (int ix = 0; ix < fw; ++ix) {
            const int32_t px = 16 * ix + 8, py = 16 * iy + 8;
            const int ends = rg_disc(r.ax, r.ay, px, py, (int64_t)radius * radius) || rg_disc(r.bx, r.by, px, py, (int64_t)radius * radius);
            cover[(int64_t)iy * fw + ix] = (uint8_t)((rg_covered(r, px, py, (int64_t)h * h) ? 1 : 0) | (ends ? 2 : 0));
        }
}

extern "C" int rg_host_tile(const int32_t *q, int32_t x0, int32_t y0, int32_t x1, int32_t y1, int32_t m) {
    return rg_tile_may_touch(RgRow{q[0], q[1], q[2], q[3]}, x0, y0, x1, y1, m) ? 1 : 0;
}

extern "C" int rg_host_score_index(double s, double lo, double k) { return rg_score_index(s, lo, k); }
