// Scene view on the device: a cloud of 32-byte records - a call's own (gwd_point_cloud) or a map's extraction (gwd_scene_extract) -
// projected into up to 16 posed pinhole cameras and z-buffered into depth, label, colour and source-row planes at frame size
// (DESIGN.md section 33).  The semantics are tests/view_ref.py's.
//
// gwd_cloud_view        three launches on the caller's stream; the z-buffer - one 64-bit key per pixel - is the workspace.
//   clear               the empty key (all ones) into every pixel of the z-buffer, 16-byte stores.
//   splat               a grid of (tiles of GWD_VIEW_TILE rows) x V.  A lane takes one row of the cloud into one camera: the position
//                       in the camera (R^T (p - t), fp64, one rounding per operation), the depth test, the projection, the half
//                       sides of its square and the pixel range, clamped to the frame in fp64.  The row's key is float32(Z)'s bits
//                       << 32 | row: positive floats order as their bits do, so a 64-bit unsigned min keeps the nearest point, ties to
//                       the lowest row.  Keys only decrease, so a plain load first skips the atomic when the stored key is already
//                       smaller (a stale value is a larger one: the skip errs towards the atomic).  A rectangle of at most
//                       kOwnArea pixels is walked by its own lane; the larger ones are taken by the whole wave, one after the
//                       other: ballot, the rectangle and the key broadcast by shuffles, the 64 lanes stride over its pixels with
//                       row-contiguous addresses.  The minimum over (depth bits, row) is unique, so the split changes nothing.
//   resolve             a grid over the planes, four pixels per lane: the keys (two 16-byte loads) become depth, index, label and
//                       colour - the second half of the winning row's record, one 16-byte load - stored 16 / 16 / 4 / 12 bytes
//                       wide; a pixel no row reached, the pixels outside a view's (fh, fw) among them, gets the empty values.
// Nothing reads the total or a size on the host, no memset, no thread waits for another; bit-identical from call to call.
#include "common.h"

// tests/view_ref.py rounds after every operation; hipcc would contract a * b + c
#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kRounds = GWD_VIEW_TILE / kThreads;
constexpr int kMaxV = 16;
constexpr int kOwnArea = 16;                              // pixels a lane walks by itself
constexpr int kPlaneBlocks = 4096;                        // clear and resolve: grid-stride above this
constexpr unsigned long long kEmpty = ~0ull;
static_assert(GWD_VIEW_TILE % kThreads == 0, "a tile is whole rounds of the workgroup");

struct ViewArgs {
    const uint4 *cloud;
    const int32_t *total_in, *sizes;                      // &cloud_offsets[n_offsets - 1]
    const double *intrinsics, *poses;
    unsigned long long *zbuf;                             // [V][Fh][Fw]
    float *depth;
    int32_t *index;
    uint8_t *labels, *rgb;
    double dmin, dmax, half_footprint, cap;
    int64_t rows, pixels;                                 // pixels = V * Fh * Fw
    int32_t V, Fh, Fw, keep;
    int32_t ext_h[kMaxV], ext_w[kMaxV];
};

struct Camera {
    double fx, fy, cx, cy, r[9], t[3];
    int fh, fw;
    bool posed;
};

struct Rect {
    int x0, y0, w, h;
};

// ceil(c - h) .. ceil(c + h) - 1 clamped to 0 .. n - 1 in fp64; false: empty (a NaN fails the comparisons)
__device__ __forceinline__ bool axis_range(double c, double h, int n, int &first, int &count) {
    double lo = ceil(c - h), hi = ceil(c + h) - 1.0;
    if (!(lo <= hi)) return false;
    lo = lo > 0.0 ? lo : 0.0;
    hi = hi < (double)(n - 1) ? hi : (double)(n - 1);
    if (!(lo <= hi)) return false;
    first = (int)lo;                                      // 0 .. n - 1 <= 16383
    count = (int)hi - first + 1;
    return true;
}

// max(0.5, min(cap, (half_footprint f) / Z)); false when it is NaN
__device__ __forceinline__ bool half_side(const ViewArgs &a, double f, double Z, double &h) {
    h = (a.half_footprint * f) / Z;
    if (h != h) return false;
    h = h < a.cap ? h : a.cap;
    h = h > 0.5 ? h : 0.5;
    return true;
}

// the rectangle and the key of one row in one camera; false: the row draws nothing
__device__ __forceinline__ bool splat_of(const ViewArgs &a, const Camera &c, int64_t row, Rect &rc, unsigned long long &key) {
    const uint4 r0 = a.cloud[2 * row], r1 = a.cloud[2 * row + 1];
    if (!(r1.w >> 24 & 1u)) return false;
    const unsigned label = r1.z >> 24;
    if ((a.keep == GWD_CLOUD_KEEP_GLASS && label != 1u) || (a.keep == GWD_CLOUD_KEEP_NON_GLASS && label == 1u)) return false;
    const float p[3] = {__uint_as_float(r0.x), __uint_as_float(r0.y), __uint_as_float(r0.z)};
#pragma unroll
    for (int k = 0; k < 3; ++k)
        if (!(fabsf(p[k]) <= 3.40282346638528859812e38f)) return false;      // NaN, Inf
    double X = (double)p[0], Y = (double)p[1], Z = (double)p[2];
    if (c.posed) {
        const double d[3] = {X - c.t[0], Y - c.t[1], Z - c.t[2]};
        X = (c.r[0] * d[0] + c.r[3] * d[1]) + c.r[6] * d[2];
        Y = (c.r[1] * d[0] + c.r[4] * d[1]) + c.r[7] * d[2];
        Z = (c.r[2] * d[0] + c.r[5] * d[1]) + c.r[8] * d[2];
    }
    if (!(Z >= a.dmin && Z <= a.dmax)) return false;      // NaN fails; dmax is finite
    const double u = (c.fx * X) / Z + c.cx, v = (c.fy * Y) / Z + c.cy;
    double hx, hy;
    if (!half_side(a, c.fx, Z, hx) || !half_side(a, c.fy, Z, hy)) return false;
    if (!axis_range(u, hx, c.fw, rc.x0, rc.w) || !axis_range(v, hy, c.fh, rc.y0, rc.h)) return false;
    key = (unsigned long long)__float_as_uint((float)Z) << 32 | (unsigned long long)row;
    return true;
}

__device__ __forceinline__ void draw(unsigned long long *at, unsigned long long key) {
    if (*at > key) atomicMin(at, key);                    // keys only decrease: a smaller one stored already stays
}

__global__ __launch_bounds__(kThreads) void view_clear_kernel(const ViewArgs a) {
    const int64_t step = (int64_t)gridDim.x * kThreads, at = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int64_t pairs = a.pixels / 2;
    ulonglong2 *z2 = (ulonglong2 *)a.zbuf;
    for (int64_t k = at; k < pairs; k += step) z2[k] = make_ulonglong2(kEmpty, kEmpty);
    if (at == 0 && (a.pixels & 1)) a.zbuf[a.pixels - 1] = kEmpty;
}

__global__ __launch_bounds__(kThreads) void view_splat_kernel(const ViewArgs a) {
    const int v = blockIdx.y;
    const int64_t total = min((int64_t)max(*a.total_in, 0), a.rows);
    if ((int64_t)blockIdx.x * GWD_VIEW_TILE >= total) return;                  // uniform: the tiles behind the total
    Camera c;
    c.fx = a.intrinsics[4 * v], c.fy = a.intrinsics[4 * v + 1], c.cx = a.intrinsics[4 * v + 2], c.cy = a.intrinsics[4 * v + 3];
    c.posed = a.poses != nullptr;
    if (c.posed) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = 0; j < 3; ++j) c.r[3 * i + j] = a.poses[12 * v + 4 * i + j];
            c.t[i] = a.poses[12 * v + 4 * i + 3];
        }
    }
    c.fh = frame_side(a.sizes[2 * v], a.ext_h[v]);
    c.fw = frame_side(a.sizes[2 * v + 1], a.ext_w[v]);
    unsigned long long *plane = a.zbuf + (int64_t)v * a.Fh * a.Fw;
    const int lane = threadIdx.x & 63;
#pragma unroll 1
    for (int j = 0; j < kRounds; ++j) {
        const int64_t row = (int64_t)blockIdx.x * GWD_VIEW_TILE + j * kThreads + threadIdx.x;
        Rect rc = {0, 0, 0, 0};
        unsigned long long key = kEmpty;
        const bool ok = row < total && splat_of(a, c, row, rc, key);
        const int area = ok ? rc.w * rc.h : 0;            // at most 66 x 66
        if (area > 0 && area <= kOwnArea) {
            for (int y = rc.y0; y < rc.y0 + rc.h; ++y)
                for (int x = rc.x0; x < rc.x0 + rc.w; ++x) draw(plane + (int64_t)y * a.Fw + x, key);
        }
        // the larger rectangles, one after the other, by all 64 lanes (every lane of the wave is here: no lane has left the loop)
        unsigned long long big = __ballot(area > kOwnArea);
        while (big) {
            const int src = __ffsll(big) - 1;
            big &= big - 1ull;
            const int x0 = __shfl(rc.x0, src, 64), y0 = __shfl(rc.y0, src, 64), w = __shfl(rc.w, src, 64), n = __shfl(area, src, 64);
            const unsigned lo = (unsigned)__shfl((int)(unsigned)key, src, 64), hi = (unsigned)__shfl((int)(unsigned)(key >> 32), src, 64);
            const unsigned long long k = (unsigned long long)hi << 32 | lo;
            for (int i = lane; i < n; i += 64) {
                const int dy = i / w;
                draw(plane + (int64_t)(y0 + dy) * a.Fw + (x0 + (i - dy * w)), k);
            }
        }
    }
}

__global__ __launch_bounds__(kThreads) void view_resolve_kernel(const ViewArgs a) {
    const int64_t step = (int64_t)gridDim.x * kThreads, groups = (a.pixels + 3) / 4;
    for (int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x; g < groups; g += step) {
        const int64_t p = 4 * g;
        const int n = (int)min((int64_t)4, a.pixels - p);
        unsigned long long key[4] = {kEmpty, kEmpty, kEmpty, kEmpty};
        if (n == 4) {
            const ulonglong2 k0 = *(const ulonglong2 *)(a.zbuf + p), k1 = *(const ulonglong2 *)(a.zbuf + p + 2);
            key[0] = k0.x, key[1] = k0.y, key[2] = k1.x, key[3] = k1.y;
        } else {
            for (int k = 0; k < n; ++k) key[k] = a.zbuf[p + k];
        }
        float depth[4];
        int32_t index[4];
        unsigned label[4], rgb[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            depth[k] = 0.0f, index[k] = -1, label[k] = 255u, rgb[k] = 0u;
            const int64_t row = (int64_t)(key[k] & 0xffffffffull);
            if (key[k] != kEmpty && row < a.rows) {       // a key holds a row of the cloud: always inside
                const uint4 r1 = a.cloud[2 * row + 1];
                depth[k] = __uint_as_float((unsigned)(key[k] >> 32));
                index[k] = (int32_t)row;
                label[k] = r1.z >> 24;
                if (r1.w >> 24 & 8u) rgb[k] = r1.z & 0xffffffu;
            }
        }
        if (n == 4) {
            *(float4 *)(a.depth + p) = make_float4(depth[0], depth[1], depth[2], depth[3]);
            *(int4 *)(a.index + p) = make_int4(index[0], index[1], index[2], index[3]);
            *(unsigned *)(a.labels + p) = label[0] | label[1] << 8 | label[2] << 16 | label[3] << 24;
            unsigned *c = (unsigned *)(a.rgb + 3 * p);    // 12 bytes at a multiple of 12
            c[0] = rgb[0] | rgb[1] << 24;
            c[1] = rgb[1] >> 8 | rgb[2] << 16;
            c[2] = rgb[2] >> 16 | rgb[3] << 8;
        } else {
            for (int k = 0; k < n; ++k) {
                a.depth[p + k] = depth[k];
                a.index[p + k] = index[k];
                a.labels[p + k] = (uint8_t)label[k];
                for (int ch = 0; ch < 3; ++ch) a.rgb[3 * (p + k) + ch] = (uint8_t)(rgb[k] >> (8 * ch));
            }
        }
    }
}

int64_t tiles_of(int64_t n) { return (n + GWD_VIEW_TILE - 1) / GWD_VIEW_TILE; }

unsigned plane_blocks(int64_t items) {
    const int64_t blocks = (items + kThreads - 1) / kThreads;
    return (unsigned)(blocks < 1 ? 1 : blocks > kPlaneBlocks ? kPlaneBlocks : blocks);
}

}  // namespace

// bytes of gwd_query_workspace(GWD_WS_VIEW, {V, Fh, Fw}) (optim.hip): the z-buffer, 8 bytes per pixel
int64_t gwd_view_workspace_bytes(int64_t V, int64_t Fh, int64_t Fw) {
    if (V < 1 || V > kMaxV || Fh < 1 || Fw < 1 || Fh > 16384 || Fw > 16384) return -1;
    return (V * Fh * Fw * 8 + 15) / 16 * 16;
}

extern "C" int gwd_cloud_view(const gwd_view_desc *d, void *stream) {
    if (!d || !d->cloud || !d->cloud_offsets || !d->sizes || !d->intrinsics || !d->workspace || !d->view_depth || !d->view_index ||
        !d->view_labels || !d->view_rgb)
        return -1;
    if (d->V < 1 || d->V > kMaxV || d->Fh < 1 || d->Fw < 1 || d->Fh > 16384 || d->Fw > 16384 || d->rows < 1 || d->rows > 2147483647LL ||
        d->n_offsets < 2)
        return -1;
    for (int v = 0; v < d->V; ++v)
        if (d->ext_h[v] < 1 || d->ext_w[v] < 1 || d->ext_h[v] > d->Fh || d->ext_w[v] > d->Fw) return -1;
    if (d->keep != GWD_CLOUD_KEEP_ALL && d->keep != GWD_CLOUD_KEEP_GLASS && d->keep != GWD_CLOUD_KEEP_NON_GLASS) return -2;
    if (d->max_splat < 1 || d->max_splat > GWD_VIEW_MAX_SPLAT) return -2;
    if (!(d->footprint >= 0.0) || !(d->footprint < 1e300)) return -2;                       // NaN, negative, Inf
    if (!(d->min_depth > 0.0) || !(d->min_depth <= d->max_depth) || !(d->max_depth < 1e300)) return -2;
    if (((uintptr_t)d->cloud & 15) || ((uintptr_t)d->cloud_offsets & 3) || ((uintptr_t)d->sizes & 3) || ((uintptr_t)d->intrinsics & 7) ||
        ((uintptr_t)d->poses & 7) || ((uintptr_t)d->workspace & 15) || ((uintptr_t)d->view_depth & 15) || ((uintptr_t)d->view_index & 15) ||
        ((uintptr_t)d->view_labels & 3) || ((uintptr_t)d->view_rgb & 3))
        return -3;
    ViewArgs a;
    a.cloud = (const uint4 *)d->cloud;
    a.total_in = d->cloud_offsets + (d->n_offsets - 1);
    a.sizes = d->sizes; a.intrinsics = d->intrinsics; a.poses = d->poses;
    a.zbuf = (unsigned long long *)d->workspace;
    a.depth = d->view_depth; a.index = d->view_index; a.labels = d->view_labels; a.rgb = d->view_rgb;
    a.dmin = d->min_depth; a.dmax = d->max_depth;
    a.half_footprint = 0.5 * d->footprint;
    a.cap = (double)d->max_splat / 2.0;
    a.rows = d->rows;
    a.V = d->V; a.Fh = d->Fh; a.Fw = d->Fw; a.keep = d->keep;
    a.pixels = (int64_t)d->V * d->Fh * d->Fw;
    for (int v = 0; v < kMaxV; ++v) {
        a.ext_h[v] = v < d->V ? d->ext_h[v] : 0;
        a.ext_w[v] = v < d->V ? d->ext_w[v] : 0;
    }
    const hipStream_t s = (hipStream_t)stream;
    view_clear_kernel<<<plane_blocks(a.pixels / 2), kThreads, 0, s>>>(a);
    GWD_CHECK_LAUNCH();
    view_splat_kernel<<<dim3((unsigned)tiles_of(a.rows), (unsigned)a.V), kThreads, 0, s>>>(a);
    GWD_CHECK_LAUNCH();
    view_resolve_kernel<<<plane_blocks((a.pixels + 3) / 4), kThreads, 0, s>>>(a);
    GWD_CHECK_LAUNCH();
    return 0;
}
