// Point clouds on the device: the dense results of InferenceSession.predict_frames (depth fp32, labels uint8, [B][Fh][Fw], top-left
// aligned frames, sizes on the device) unprojected through pinhole intrinsics and packed - the valid points of every frame, frame
// after frame, in raster order, 32 bytes each.  The semantics are tests/cloud_ref.py's.
//
// gwd_point_cloud       three launches on the caller's stream.  A frame's candidates - the pixels of its stride lattice, numbered
//                       in raster order - are cut into tiles of GWD_CLOUD_TILE; workgroup g takes tile g - block0[b] of frame b,
//                       block0 being the prefix of the frames' tile counts, formed on the host from what it knows of the sizes.
//   count               validity of the tile's candidates -> the tile's count in the workspace (ballot + population count).
//   scan                ONE workgroup: the tile counts become exclusive offsets in place, the total behind them; cloud_offsets.
//   emit                validity again (the planes are in L2; a mask would be a byte written and read per candidate and a second
//                       operand to keep in step), the lane's rank = the tile's offset + the counts of the waves and rounds before
//                       it (LDS) + the set bits below it in its wave's ballot, the record, two 16-byte stores; the rows from the
//                       total to the capacity are zeroed grid-stride by the same workgroups.
// The count per tile, the scan and the rank inside a tile are compact.h's, shared with scene.hip.
// A tile's offset is a function of the counts alone: no workgroup waits for another, no atomic takes part, no memset; repeated calls
// are bit-identical and a frame's rows depend on neither its slot nor its neighbours nor Fh x Fw.
// All geometry is fp64, one rounding per operation (no contraction), one final rounding to fp32.
#include "compact.h"

// tests/cloud_ref.py rounds after every operation; hipcc would contract a * b + c
#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kRounds = GWD_CLOUD_TILE / kThreads;        // candidates per lane
constexpr int kMaxB = 16;
static_assert(GWD_CLOUD_TILE % kThreads == 0, "a tile is whole rounds of the workgroup");

struct CloudArgs {
    const float *depth;
    const uint8_t *labels, *region_map, *source;
    const int32_t *sizes, *region_count;
    const double *intrinsics, *planes, *poses;
    int32_t *ws;                                          // [tiles] counts, then exclusive offsets; [tiles] the total
    uint4 *cloud;
    int32_t *offsets;
    const uint8_t *frame[kMaxB];
    int32_t pitch[kMaxB], ext_h[kMaxB], ext_w[kMaxB], block0[kMaxB + 1];
    double dmin, dmax, edge;
    int64_t plane, capacity;
    int32_t B, Fh, Fw, R, s, normals, keep, edge_on, tiles;
};

struct Frame {
    int b, tile, fh, fw, nw;
    int64_t ncand;
};

// which frame and which of its tiles a workgroup takes; uniform
__device__ __forceinline__ Frame frame_of(const CloudArgs &a, int block) {
    Frame f;
    f.b = 0;
    while (f.b + 1 < a.B && block >= a.block0[f.b + 1]) ++f.b;
    f.tile = block - a.block0[f.b];
    f.fh = frame_side(a.sizes[2 * f.b], a.ext_h[f.b]);
    f.fw = frame_side(a.sizes[2 * f.b + 1], a.ext_w[f.b]);
    f.nw = (f.fw + a.s - 1) / a.s;
    f.ncand = (int64_t)((f.fh + a.s - 1) / a.s) * f.nw;
    return f;
}

__device__ __forceinline__ bool usable(const CloudArgs &a, double z) { return z >= a.dmin && z <= a.dmax; }    // NaN, Inf: false

// candidate c of the frame -> its pixel; false past the last candidate
__device__ __forceinline__ bool candidate(const CloudArgs &a, const Frame &f, int64_t c, int &x, int &y) {
    if (c >= f.ncand) return false;
    const int cy = (int)(c / f.nw);
    y = cy * a.s;
    x = ((int)(c - (int64_t)cy * f.nw)) * a.s;
    return true;
}

__device__ __forceinline__ bool is_point(const CloudArgs &a, const Frame &f, const float *__restrict__ D, const uint8_t *__restrict__ L,
                                         int x, int y) {
    const int64_t at = (int64_t)y * a.Fw + x;
    const double z = (double)D[at];
    if (!usable(a, z)) return false;
    const int lab = L[at];
    if (lab == 255 || (a.keep == GWD_CLOUD_KEEP_GLASS && lab != 1) || (a.keep == GWD_CLOUD_KEEP_NON_GLASS && lab == 1)) return false;
    if (a.edge_on) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int xn = x + (k == 0 ? -a.s : k == 1 ? a.s : 0), yn = y + (k == 2 ? -a.s : k == 3 ? a.s : 0);
            if (xn < 0 || yn < 0 || xn >= f.fw || yn >= f.fh) continue;
            const double zn = (double)D[(int64_t)yn * a.Fw + xn];
            if (usable(a, zn) && !(fabs(zn - z) <= a.edge * fmin(zn, z))) return false;
        }
    }
    return true;
}

struct Cam {
    double fx, fy, cx, cy;
};

__device__ __forceinline__ void unproject(const Cam &c, int x, int y, double z, double (&p)[3]) {
    p[0] = (((double)x - c.cx) * z) / c.fx;
    p[1] = (((double)y - c.cy) * z) / c.fy;
    p[2] = z;
}

// the difference of the unprojected 1-pixel neighbours along one axis: central, else the one-sided one that exists
__device__ __forceinline__ bool axis_difference(const CloudArgs &a, const Frame &f, const float *__restrict__ D, const Cam &c, int x, int y,
                                                int ax, int ay, const double (&p)[3], double (&d)[3]) {
    const int xm = x - ax, ym = y - ay, xp = x + ax, yp = y + ay;
    double zm = 0.0, zp = 0.0;
    bool um = xm >= 0 && ym >= 0, up = xp < f.fw && yp < f.fh;
    if (um) {
        zm = (double)D[(int64_t)ym * a.Fw + xm];
        um = usable(a, zm);
    }
    if (up) {
        zp = (double)D[(int64_t)yp * a.Fw + xp];
        up = usable(a, zp);
    }
    if (!um && !up) return false;
    double lo[3], hi[3];
    if (um) unproject(c, xm, ym, zm, lo);
    if (up) unproject(c, xp, yp, zp, hi);
#pragma unroll
    for (int k = 0; k < 3; ++k) d[k] = (up ? hi[k] : p[k]) - (um ? lo[k] : p[k]);
    return true;
}

__device__ __forceinline__ void rotate(const double *__restrict__ m, const double (&v)[3], double (&o)[3], bool translate) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        o[i] = (m[4 * i] * v[0] + m[4 * i + 1] * v[1]) + m[4 * i + 2] * v[2];
        if (translate) o[i] = o[i] + m[4 * i + 3];
    }
}

// the 32 bytes of the point at pixel (x, y) of frame f.b
__device__ __forceinline__ void record(const CloudArgs &a, const Frame &f, const float *__restrict__ D, const uint8_t *__restrict__ L,
                                       const Cam &c, int x, int y, uint4 &r0, uint4 &r1) {
    const int64_t at = (int64_t)y * a.Fw + x;
    const double z = (double)D[at];
    double p[3], n[3] = {0.0, 0.0, 0.0};
    unproject(c, x, y, z, p);
    const int region = a.region_map ? a.region_map[f.b * a.plane + at] : 0;
    unsigned flags = 1u;
    if (a.normals) {
        bool have = false;
        if (region >= 1 && region <= a.R && region - 1 < a.region_count[f.b]) {
            const double *pl = a.planes + ((int64_t)f.b * a.R + (region - 1)) * 6;
            if (pl[5] == 0.0) {
                const double m[3] = {pl[0] * c.fx, pl[1] * c.fy, (pl[2] + pl[0] * c.cx) + pl[1] * c.cy};
                const double len = sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]);
                if (len > 0.0 && len <= 1.79769313486231570815e308) {
#pragma unroll
                    for (int k = 0; k < 3; ++k) n[k] = -(m[k] / len);
                    have = true;
                    flags |= 4u;
                }
            }
        }
        if (!have) {
            double dx[3], dy[3];
            if (axis_difference(a, f, D, c, x, y, 1, 0, p, dx) && axis_difference(a, f, D, c, x, y, 0, 1, p, dy)) {
                const double v[3] = {dx[1] * dy[2] - dx[2] * dy[1], dx[2] * dy[0] - dx[0] * dy[2], dx[0] * dy[1] - dx[1] * dy[0]};
                const double len = sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
                if (len > 0.0 && len <= 1.79769313486231570815e308) {
#pragma unroll
                    for (int k = 0; k < 3; ++k) n[k] = v[k] / len;
                    if ((n[0] * p[0] + n[1] * p[1]) + n[2] * p[2] > 0.0) {
#pragma unroll
                        for (int k = 0; k < 3; ++k) n[k] = -n[k];
                    }
                    have = true;
                }
            }
        }
        if (have) flags |= 2u;
    }
    if (a.poses) {
        const double *m = a.poses + 12 * f.b;
        double q[3];
        rotate(m, p, q, true);
#pragma unroll
        for (int k = 0; k < 3; ++k) p[k] = q[k];
        if (flags & 2u) {
            rotate(m, n, q, false);
#pragma unroll
            for (int k = 0; k < 3; ++k) n[k] = q[k];
        }
    }
    unsigned rgb = 0u;
    if (a.frame[f.b]) {
        const uint8_t *px = a.frame[f.b] + (int64_t)y * a.pitch[f.b] + 3 * x;
        rgb = px[0] | (unsigned)px[1] << 8 | (unsigned)px[2] << 16;
        flags |= 8u;
    }
    const unsigned src = a.source ? a.source[f.b * a.plane + at] : 0u;
    r0 = make_uint4(__float_as_uint((float)p[0]), __float_as_uint((float)p[1]), __float_as_uint((float)p[2]), __float_as_uint((float)n[0]));
    r1 = make_uint4(__float_as_uint((float)n[1]), __float_as_uint((float)n[2]), rgb | (unsigned)L[at] << 24,
                    (unsigned)region | src << 8 | (unsigned)f.b << 16 | flags << 24);
}

__global__ __launch_bounds__(kThreads) void cloud_count_kernel(const CloudArgs a) {
    __shared__ int part[kWaves];
    const Frame f = frame_of(a, blockIdx.x);
    const float *__restrict__ D = a.depth + f.b * a.plane;
    const uint8_t *__restrict__ L = a.labels + f.b * a.plane;
    int n = 0;                                            // uniform in the wave
#pragma unroll
    for (int j = 0; j < kRounds; ++j) {
        int x, y;
        const bool ok = candidate(a, f, (int64_t)f.tile * GWD_CLOUD_TILE + j * kThreads + threadIdx.x, x, y) && is_point(a, f, D, L, x, y);
        n += __popcll(__ballot(ok));
    }
    tile_sum<kWaves>(n, part, &a.ws[blockIdx.x]);
}

// one workgroup: the tile counts become exclusive offsets in place, the total behind them
__global__ __launch_bounds__(kScanThreads) void cloud_scan_kernel(const CloudArgs a) {
    __shared__ int sums[kScanThreads];
    const int t = threadIdx.x;
    scan_tiles(a.ws, a.tiles, sums);
    if (t <= a.B) a.offsets[t] = a.ws[t < a.B ? a.block0[t] : a.tiles];
}

__global__ __launch_bounds__(kThreads) void cloud_emit_kernel(const CloudArgs a) {
    __shared__ int part[kRounds * kWaves];
    const Frame f = frame_of(a, blockIdx.x);
    const float *__restrict__ D = a.depth + f.b * a.plane;
    const uint8_t *__restrict__ L = a.labels + f.b * a.plane;
    int px[kRounds], py[kRounds];
    TileRank<kRounds, kWaves> points;
#pragma unroll
    for (int j = 0; j < kRounds; ++j) {
        const bool ok = candidate(a, f, (int64_t)f.tile * GWD_CLOUD_TILE + j * kThreads + threadIdx.x, px[j], py[j]) &&
                        is_point(a, f, D, L, px[j], py[j]);
        points.vote(j, ok, part);
    }
    __syncthreads();
    const int64_t base = a.ws[blockIdx.x];
    if (points.any()) {
        Cam c;
        const double *cam = a.intrinsics + 4 * f.b;
        c.fx = cam[0], c.fy = cam[1], c.cx = cam[2], c.cy = cam[3];
        points.finish(part);
#pragma unroll
        for (int j = 0; j < kRounds; ++j) {               // a round's lanes store neighbouring rows
            const int64_t row = base + points.rank(j);
            if (points.keeps(j) && row < a.capacity) {    // the capacity covers the worst case (checked on the host): always true
                uint4 r0, r1;
                record(a, f, D, L, c, px[j], py[j], r0, r1);
                a.cloud[2 * row] = r0;
                a.cloud[2 * row + 1] = r1;
            }
        }
    }
    // the rows behind the last point: zeros, shared out over the whole grid
    const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
    for (int64_t row = (int64_t)a.ws[a.tiles] + (int64_t)blockIdx.x * kThreads + threadIdx.x; row < a.capacity;
         row += (int64_t)gridDim.x * kThreads) {
        a.cloud[2 * row] = zero;
        a.cloud[2 * row + 1] = zero;
    }
}

int64_t lattice(int64_t h, int64_t w, int64_t s) { return ((h + s - 1) / s) * ((w + s - 1) / s); }
int64_t tiles_of(int64_t candidates) { return (candidates + GWD_CLOUD_TILE - 1) / GWD_CLOUD_TILE; }

}  // namespace

// bytes of gwd_query_workspace(GWD_WS_CLOUD, {B, Fh, Fw, stride}) (optim.hip)
int64_t gwd_cloud_workspace_bytes(int64_t B, int64_t Fh, int64_t Fw, int64_t stride) {
    if (B < 1 || B > kMaxB || Fh < 1 || Fw < 1 || Fh > 16384 || Fw > 16384 || stride < 1 || stride > GWD_CLOUD_MAX_STRIDE) return -1;
    return ((B * tiles_of(lattice(Fh, Fw, stride)) + 1) * (int64_t)sizeof(int32_t) + 15) / 16 * 16;
}

extern "C" int gwd_point_cloud(const gwd_cloud_desc *d, void *stream) {
    if (!d || !d->depth || !d->labels || !d->sizes || !d->intrinsics || !d->workspace || !d->cloud || !d->cloud_offsets) return -1;
    if (d->B < 1 || d->B > kMaxB || d->Fh < 1 || d->Fw < 1 || d->Fh > 16384 || d->Fw > 16384) return -1;
    if (d->stride < 1 || d->stride > GWD_CLOUD_MAX_STRIDE || !(d->min_depth <= d->max_depth) || !(d->max_depth < 1e300) ||
        !(d->min_depth > -1e300))
        return -1;
    if (d->keep != GWD_CLOUD_KEEP_ALL && d->keep != GWD_CLOUD_KEEP_GLASS && d->keep != GWD_CLOUD_KEEP_NON_GLASS) return -2;
    if ((d->region_map == nullptr) != (d->region_count == nullptr) || (d->region_map == nullptr) != (d->planes == nullptr)) return -2;
    if (d->region_map && (d->max_regions < 1 || d->max_regions > GWD_REGION_MAX)) return -2;
    if (d->edge != d->edge || d->edge > 1e300) return -2;
    if (((uintptr_t)d->depth & 3) || ((uintptr_t)d->sizes & 3) || ((uintptr_t)d->intrinsics & 7) || ((uintptr_t)d->region_count & 3) ||
        ((uintptr_t)d->planes & 7) || ((uintptr_t)d->poses & 7) || ((uintptr_t)d->workspace & 15) || ((uintptr_t)d->cloud & 15) ||
        ((uintptr_t)d->cloud_offsets & 3))
        return -3;
    CloudArgs a;
    a.depth = d->depth; a.labels = d->labels; a.region_map = d->region_map; a.source = d->source; a.sizes = d->sizes;
    a.region_count = d->region_count; a.intrinsics = d->intrinsics; a.planes = d->planes; a.poses = d->poses;
    a.ws = (int32_t *)d->workspace; a.cloud = (uint4 *)d->cloud; a.offsets = d->cloud_offsets;
    int64_t worst = 0, tiles = 0;
    for (int b = 0; b < kMaxB; ++b) {
        a.frame[b] = nullptr;
        a.pitch[b] = 0;
        a.ext_h[b] = a.ext_w[b] = 0;
        if (b >= d->B) continue;
        if (d->ext_h[b] < 1 || d->ext_w[b] < 1 || d->ext_h[b] > d->Fh || d->ext_w[b] > d->Fw) return -1;
        a.ext_h[b] = d->ext_h[b];
        a.ext_w[b] = d->ext_w[b];
        if (d->has_frames) {
            if (!d->frames.ptr[b] || (d->ext_h[b] > 1 && d->frames.pitch[b] < 3 * d->ext_w[b])) return -1;
            a.frame[b] = (const uint8_t *)d->frames.ptr[b];
            a.pitch[b] = d->frames.pitch[b];
        }
        a.block0[b] = (int32_t)tiles;
        const int64_t n = lattice(a.ext_h[b], a.ext_w[b], d->stride);
        worst += n;
        tiles += tiles_of(n);
    }
    for (int b = d->B; b <= kMaxB; ++b) a.block0[b] = (int32_t)tiles;
    if (d->capacity < worst || d->capacity > 2147483647LL) return -1;      // never a shortened cloud
    a.dmin = d->min_depth; a.dmax = d->max_depth; a.edge = d->edge; a.edge_on = d->edge > 0.0;
    a.plane = (int64_t)d->Fh * d->Fw; a.capacity = d->capacity;
    a.B = d->B; a.Fh = d->Fh; a.Fw = d->Fw; a.R = d->region_map ? d->max_regions : 0; a.s = d->stride; a.normals = d->normals != 0;
    a.keep = d->keep; a.tiles = (int32_t)tiles;
    const hipStream_t s = (hipStream_t)stream;
    cloud_count_kernel<<<(unsigned)tiles, kThreads, 0, s>>>(a);
    GWD_CHECK_LAUNCH();
    cloud_scan_kernel<<<1, kScanThreads, 0, s>>>(a);
    GWD_CHECK_LAUNCH();
    cloud_emit_kernel<<<(unsigned)tiles, kThreads, 0, s>>>(a);
    GWD_CHECK_LAUNCH();
    return 0;
}
