// Sensor depth fusion on the device: the depth plane of an RGB-D camera (uint16 millimetres, 0 = no reading,
// registered to the frame) completed behind glass from what predict_frames and gwd_glass_regions already hold - glass labels,
// connected regions, the network's depth.  Every pane is fitted from the depth the SENSOR measured on its frame - the ring of
// non-glass pixels around the region - and the pane's depth is written over the sensor's; where no pane can be fitted the network's
// depth, scaled to the sensor, fills in.  No host sync, no memset, no floating-point atomics; every phase is its own launch, so a
// kernel boundary is the only thing any thread ever waits for.
//
// gwd_fusion_ring
//   fusion_row_kernel     one byte per frame pixel: bit 7 = a glass pixel within `gap` columns in this row, bits 0..5 = the smallest
//                         region_map value within `ring` columns (63 = none).  A workgroup stages its 256 pixels and a 32-pixel
//                         halo either side in LDS once and every thread walks its window there.
//   fusion_col_kernel     the same two windows down the columns of that plane (Chebyshev windows are separable) -> fusion_ring;
//                         the three integer sums of the scale ride along: a wave reduces, a workgroup adds once (integer
//                         atomics: their order changes no bit).
//   fusion_scale_kernel   s = sum sensor * network / sum network^2 per frame.
// gwd_fusion_planes       the method of gwd_region_planes (planefit.h) over the ring pixels of every kept region, twice: all
//                         samples, then those whose residual against the STORED first coefficients is within trim * rms.
// gwd_fusion_depth        one streaming pass: SENSOR / PLANE / NETWORK per pixel, four pixels per thread where the rows allow
//                         16-byte accesses.
#include "common.h"
#include "depthmm.h"
#include "planefit.h"

namespace {

constexpr int kThreads = 256;                             // columns of a workgroup's tile in the row, column and moment passes
constexpr int kMaxB = 16;
constexpr int kMaxR = GWD_REGION_MAX;
constexpr int kRec = GWD_REGION_RECORD;
constexpr int kMaxRing = GWD_FUSION_MAX_RING;             // the halo of the row pass's tile, and of the column pass's
constexpr int kRows = 16;                                 // rows of a workgroup's tile in the column pass
constexpr int kPlaneBlocks = 64;                          // workgroups per image of the moment passes, at most
constexpr int kPl = GWD_FUSION_PLANE;                     // fp64 fields of a fusion plane
constexpr int kNone = 63;                                 // `no region` in bits 0..5 of the row pass's byte
enum { P_A1 = 0, P_B1, P_G1, P_RMS1, P_N1, P_A, P_B, P_G, P_RMS, P_N, P_STATUS, P_SPARE };
enum { R_X0 = 1, R_Y0 = 2 };                              // fields of a region's record (regions.hip)

__host__ __device__ inline int64_t up16(int64_t v) { return (v + 15) & ~(int64_t)15; }
struct Layout {                                           // byte offsets into the workspace, every one a multiple of 16
    int64_t sums, partial, rowcode, total;
};
Layout layout(int64_t B, int64_t Fh, int64_t Fw) {
    Layout l;
    l.sums = 0;                                           // [16][4] uint64: n, sum sensor * network, sum network^2, spare
    l.partial = kMaxB * 4 * 8;                            // [B][kPlaneBlocks][32][10] 8-byte values
    l.rowcode = l.partial + B * kPlaneBlocks * kMaxR * kFitRec * 8;        // [B][Fh * Fw] uint8
    l.total = l.rowcode + up16(B * Fh * Fw);
    return l;
}

// ------------------------------------------------------------------------------------------------ ring map and scale sums
struct RingArgs {
    const uint8_t *labels, *region_map;
    const uint16_t *sensor_mm, *depth_mm;
    const int32_t *sizes, *region_count;
    uint8_t *rowcode, *ring_map;
    unsigned long long *sums;
    double *scale;
    int64_t plane;
    int32_t B, Fh, Fw, max_regions, ring, gap, lo_mm, hi_mm, align, min_align;
};

// thread = pixel (x, y) of image b.  tile[t] is the pixel x0 - kMaxRing + t of the row; outside the frame: nothing.
__global__ __launch_bounds__(kThreads) void fusion_row_kernel(const RingArgs a) {
    __shared__ uint8_t tile[kThreads + 2 * kMaxRing];
    const int b = blockIdx.z, y = blockIdx.y, x0 = blockIdx.x * kThreads, t = threadIdx.x;
    if (blockIdx.x == 0 && y == 0 && t < 4) a.sums[b * 4 + t] = 0ull;
    const FrameExtent f = frame_extent(a.sizes, b, a.Fh, a.Fw);
    if (y >= f.fh || x0 >= f.fw) return;                  // uniform: the whole workgroup leaves
    const int K = min(max(a.region_count[b], 0), a.max_regions);
    const uint8_t *__restrict__ L = a.labels + b * a.plane + (int64_t)y * a.Fw;
    const uint8_t *__restrict__ M = a.region_map + b * a.plane + (int64_t)y * a.Fw;
    for (int k = t; k < kThreads + 2 * kMaxRing; k += kThreads) {
        const int x = x0 - kMaxRing + k;
        uint8_t code = kNone;
        if (x >= 0 && x < f.fw) {
            const int rank = M[x];
            code = (uint8_t)((rank >= 1 && rank <= K ? rank : kNone) | (L[x] == 1 ? 0x80 : 0));
        }
        tile[k] = code;
    }
    __syncthreads();
    const int x = x0 + t;
    if (x >= f.fw) return;
    int best = kNone, glass = 0;
    for (int d = -a.ring; d <= a.ring; ++d) best = min(best, tile[kMaxRing + t + d] & 0x3f);
    for (int d = -a.gap; d <= a.gap; ++d) glass |= tile[kMaxRing + t + d] & 0x80;
    a.rowcode[b * a.plane + (int64_t)y * a.Fw + x] = (uint8_t)(best | glass);
}

// thread = column x of kRows rows of image b.  col[j][t] is row y0 - ring + j of the thread's OWN column: no thread reads what
// another one wrote, so the tile needs no barrier.  Every lane stays to the end (the wave sums below).
__global__ __launch_bounds__(kThreads) void fusion_col_kernel(const RingArgs a) {
    __shared__ uint8_t col[kRows + 2 * kMaxRing][kThreads];
    __shared__ unsigned long long wsum[3];
    const int b = blockIdx.z, y0 = blockIdx.y * kRows, t = threadIdx.x, lane = t & 63;
    const int x = blockIdx.x * kThreads + t;
    const FrameExtent f = frame_extent(a.sizes, b, a.Fh, a.Fw);
    if (t < 3) wsum[t] = 0ull;
    __syncthreads();
    const int64_t base = b * a.plane;
    const int span = kRows + 2 * a.ring;
    for (int j = 0; j < span; ++j) {
        const int y = y0 - a.ring + j;
        col[j][t] = (y >= 0 && y < f.fh && x < f.fw) ? a.rowcode[base + (int64_t)y * a.Fw + x] : (uint8_t)kNone;
    }
    unsigned long long n = 0, sp = 0, pp = 0;
    for (int i = 0; i < kRows; ++i) {
        const int y = y0 + i;
        if (y >= a.Fh || x >= a.Fw) break;
        const int64_t at = base + (int64_t)y * a.Fw + x;
        uint8_t out = 0;
        if (y < f.fh && x < f.fw) {
            int best = kNone, glass = 0;
            for (int d = -a.ring; d <= a.ring; ++d) best = min(best, col[a.ring + i + d][t] & 0x3f);
            for (int d = -a.gap; d <= a.gap; ++d) glass |= col[a.ring + i + d][t] & 0x80;
            const int s = a.sensor_mm[at];
            const bool clear = a.labels[at] != 1 && !glass;                   // not glass, no glass within `gap`
            const bool valid = s >= a.lo_mm && s <= a.hi_mm;
            if (clear && valid && best != kNone) out = (uint8_t)best;         // best = r + 1 of the smallest rank within `ring`
            if (clear && valid) {
                const int p = a.depth_mm[at];
                if (p >= a.lo_mm && p <= a.hi_mm) {
                    n += 1ull;
                    sp += (unsigned long long)s * (unsigned long long)p;
                    pp += (unsigned long long)p * (unsigned long long)p;
                }
            }
        }
        a.ring_map[at] = out;
    }
    n = (unsigned long long)wave_sum_ll((long long)n);
    sp = (unsigned long long)wave_sum_ll((long long)sp);
    pp = (unsigned long long)wave_sum_ll((long long)pp);
    if (lane == 0 && n) {
        atomicAdd(&wsum[0], n); atomicAdd(&wsum[1], sp); atomicAdd(&wsum[2], pp);
    }
    __syncthreads();
    if (t < 3 && wsum[0]) atomicAdd(a.sums + b * 4 + t, wsum[t]);
}

__global__ __launch_bounds__(64) void fusion_scale_kernel(const RingArgs a) {
    const int b = threadIdx.x;
    if (b >= a.B) return;
    const unsigned long long n = a.sums[b * 4], sp = a.sums[b * 4 + 1], pp = a.sums[b * 4 + 2];
    const bool use = a.align && n >= (unsigned long long)a.min_align && pp > 0ull;
    a.scale[b * 4 + 0] = use ? (double)sp / (double)pp : 1.0;
    a.scale[b * 4 + 1] = (double)n;
    a.scale[b * 4 + 2] = (double)sp;
    a.scale[b * 4 + 3] = (double)pp;
}

// ------------------------------------------------------------------------------------------------ frame planes
struct FitArgs {
    const uint8_t *ring_map;
    const uint16_t *sensor_mm;
    const int32_t *sizes, *region_count;
    const long long *records;
    double *planes;                                       // [B][max_regions][kPl]
    long long *partial;                                   // [B][nb][32][kFitNI int64 | kFitND f64]
    int64_t plane;
    int32_t B, Fh, Fw, max_regions, ring, lo_mm, hi_mm, min_ring, nb;
    double trim, max_rms;
};

// does the second fit run for the region of this row?  (read before and after its solve: a second fit that came out flat has
// status 1 and needs no residual)
__device__ __forceinline__ bool refits(const double *pl, double trim) {
    return trim > 0.0 && pl[P_STATUS] == 0.0 && pl[P_RMS1] > 0.0;
}

// MODE 0: the ten moments of every region's ring samples, coordinates relative to (max(x0 - ring, 0), max(y0 - ring, 0));
// 1: their squared residuals against the first fit; 2: the moments of the samples the trim keeps; 3: those samples' squared
// residuals against the second fit.  The walk is gwd_region_planes': a workgroup owns every 64th row, a wave 64 neighbours of it.
template <int MODE>
__global__ __launch_bounds__(kThreads) void fusion_moments_kernel(const FitArgs a) {
#pragma clang fp contract(off)
    __shared__ long long pi[4][kMaxR][kFitNI];
    __shared__ double pd[4][kMaxR][kFitND];
    __shared__ int ox[kMaxR], oy[kMaxR], act[kMaxR];
    __shared__ double c1[kMaxR][3], c2[kMaxR][3], thr[kMaxR];
    const int b = blockIdx.y, blk = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const FrameExtent f = frame_extent(a.sizes, b, a.Fh, a.Fw);
    const int K = min(max(a.region_count[b], 0), a.max_regions);
    for (int k = threadIdx.x; k < 4 * kMaxR * kFitNI; k += kThreads) (&pi[0][0][0])[k] = 0;
    for (int k = threadIdx.x; k < 4 * kMaxR * kFitND; k += kThreads) (&pd[0][0][0])[k] = 0.0;
    if ((int)threadIdx.x < kMaxR) {
        const int r = threadIdx.x;
        const long long *rec = a.records + ((int64_t)b * a.max_regions + (r < K ? r : 0)) * kRec;
        ox[r] = r < K ? max((int)rec[R_X0] - a.ring, 0) : 0;
        oy[r] = r < K ? max((int)rec[R_Y0] - a.ring, 0) : 0;
        const double *pl = a.planes + ((int64_t)b * a.max_regions + (r < K ? r : 0)) * kPl;
        bool on = r < K;
        if (MODE == 1) on = on && pl[P_STATUS] == 0.0;
        if (MODE >= 2) on = on && refits(pl, a.trim);
        act[r] = on;
        const double tr = a.trim * (on && MODE >= 2 ? pl[P_RMS1] : 0.0);
        thr[r] = tr * tr;
        for (int k = 0; k < 3; ++k) {
            c1[r][k] = on && MODE >= 1 ? pl[P_A1 + k] : 0.0;
            c2[r][k] = on && MODE == 3 ? pl[P_A + k] : 0.0;
        }
    }
    __syncthreads();
    const uint8_t *__restrict__ M = a.ring_map + b * a.plane;
    const uint16_t *__restrict__ D = a.sensor_mm + b * a.plane;
    // row y belongs to workgroup y % kPlaneBlocks whatever the plane's height (min(Fh, kPlaneBlocks) workgroups run, and y < Fh): a
    // frame's sums are then formed in the same order alone and in any batch - a workgroup without rows adds an exact 0
    for (int y = blk; y < f.fh; y += kPlaneBlocks) {
        for (int xt = 0; xt < f.fw; xt += kThreads) {     // uniform bounds: every lane of a wave reaches the ballots
            const int x = xt + threadIdx.x;
            int rank = 0, mm = 1;
            if (x < f.fw) {
                rank = M[(int64_t)y * a.Fw + x];
                mm = D[(int64_t)y * a.Fw + x];
                if (rank > K || mm < a.lo_mm || mm > a.hi_mm || !act[rank ? rank - 1 : 0]) rank = 0;
            }
            double w = rank ? 1000.0 / (double)mm : 0.0;
            if (MODE >= 2 && rank) {                      // the trim: against the STORED first coefficients
                const double e = fit_residual(w, c1[rank - 1][0], c1[rank - 1][1], c1[rank - 1][2], x, y);
                if (!(e * e <= thr[rank - 1])) { rank = 0; w = 0.0; }
            }
            unsigned long long todo = __ballot(rank > 0);
            while (todo) {                                // one round per region present in the wave, in lane order
                const int r = __shfl(rank, __builtin_ctzll(todo), 64);
                const bool mine = rank == r;
                todo &= ~__ballot(mine);
                const double wm = mine ? w : 0.0;
                if (MODE == 1 || MODE == 3) {
                    const double *c = MODE == 1 ? c1[r - 1] : c2[r - 1];
                    fit_add_residual(mine ? fit_residual(wm, c[0], c[1], c[2], x, y) : 0.0, lane, pd[wave][r - 1]);
                } else {
                    const long long dx = mine ? x - ox[r - 1] : 0, dy = mine ? y - oy[r - 1] : 0;
                    fit_add_moments(mine, dx, dy, wm, lane, pi[wave][r - 1], pd[wave][r - 1]);
                }
            }
        }
    }
    __syncthreads();
    fit_store_partial(pi, pd, a.partial + ((int64_t)b * kPlaneBlocks + blk) * kMaxR * kFitRec, kMaxR, threadIdx.x, kThreads);
}

// one wave per (region, image): folds the workgroups' partial records in ascending order, then one thread finishes the mode's
// part of the row
template <int MODE>
__global__ __launch_bounds__(64) void fusion_solve_kernel(const FitArgs a) {
#pragma clang fp contract(off)
    __shared__ long long si[kFitNI];
    __shared__ double sd[kFitND];
    const int r = blockIdx.x, b = blockIdx.y, q = threadIdx.x;
    if (r >= a.max_regions) return;
    const int K = min(max(a.region_count[b], 0), a.max_regions);
    double *pl = a.planes + ((int64_t)b * a.max_regions + r) * kPl;
    if (r >= K) {
        if (MODE == 0 && q < kPl) pl[q] = 0.0;
        return;
    }
    fit_fold(a.partial + (int64_t)b * kPlaneBlocks * kMaxR * kFitRec + r * kFitRec, a.nb, (int64_t)kMaxR * kFitRec, q, si, sd);
    __syncthreads();
    if (q != 0) return;
    const double nan = __builtin_nan("");
    const long long *rec = a.records + ((int64_t)b * a.max_regions + r) * kRec;
    const long long ox = max((int)rec[R_X0] - a.ring, 0), oy = max((int)rec[R_Y0] - a.ring, 0);
    if (MODE == 0) {
        const PlaneFit fit = fit_solve(si, sd, ox, oy);
        pl[P_A1] = fit.alpha; pl[P_B1] = fit.beta; pl[P_G1] = fit.gamma;
        pl[P_RMS1] = nan;
        pl[P_N1] = fit.n;
        pl[P_A] = pl[P_B] = pl[P_G] = pl[P_RMS] = nan;
        pl[P_N] = fit.n;
        pl[P_STATUS] = fit.flat ? 1.0 : 0.0;
        pl[P_SPARE] = 0.0;
    } else if (MODE == 1) {
        if (pl[P_STATUS] == 0.0) pl[P_RMS1] = sqrt(sd[0] / pl[P_N1]);
    } else if (MODE == 2) {
        if (refits(pl, a.trim)) {
            const PlaneFit fit = fit_solve(si, sd, ox, oy);
            pl[P_A] = fit.alpha; pl[P_B] = fit.beta; pl[P_G] = fit.gamma;
            pl[P_N] = fit.n;
            if (fit.flat) pl[P_STATUS] = 1.0;
        } else if (pl[P_STATUS] == 0.0) {                 // no second fit: the first one stands
            pl[P_A] = pl[P_A1]; pl[P_B] = pl[P_B1]; pl[P_G] = pl[P_G1]; pl[P_RMS] = pl[P_RMS1];
        }
    } else {
        if (refits(pl, a.trim)) pl[P_RMS] = sqrt(sd[0] / pl[P_N]);
        if (pl[P_STATUS] == 0.0 && (pl[P_N] < (double)a.min_ring || pl[P_RMS] > a.max_rms)) pl[P_STATUS] = 2.0;
    }
}

// ------------------------------------------------------------------------------------------------ fused depth
struct FuseArgs {
    const uint8_t *labels, *region_map;
    const uint16_t *sensor_mm;
    const float *depth;
    const int32_t *sizes, *region_count;
    const double *planes, *scale;
    float *out;
    uint16_t *out_mm;
    uint8_t *source;
    int64_t plane;
    int32_t B, Fh, Fw, max_regions, lo_mm, hi_mm;
    float dmin, dmax;
};

struct Fused {
    float v;
    unsigned short mm;
    uint8_t src;
};

__device__ __forceinline__ Fused fuse_pixel(int x, int y, bool inside, int label, int rank, int s, float d, int lo_mm, int hi_mm,
                                            double dmin, double dmax, double scale, const double (*coef)[3], const int *fit) {
#pragma clang fp contract(off)
    Fused o = {0.f, 0, 0};
    if (!inside) return o;
    if (label != 1 && s >= lo_mm && s <= hi_mm) {
        o.v = __fdiv_rn((float)s, 1000.0f);
        o.mm = (unsigned short)s;
        o.src = GWD_FUSED_SENSOR;
        return o;
    }
    double z = 0.0;
    if (rank > 0 && rank <= kMaxR && fit[rank - 1]) {
        const double den = (coef[rank - 1][0] * (double)x + coef[rank - 1][1] * (double)y) + coef[rank - 1][2];
        if (den > 0.0) {
            z = 1.0 / den;
            o.src = GWD_FUSED_PLANE;
        }
    }
    if (!o.src) {
        z = (double)d * scale;
        o.src = GWD_FUSED_NETWORK;
    }
    z = z < dmin ? dmin : z;
    z = z > dmax ? dmax : z;
    o.v = (float)z;
    o.mm = to_mm(o.v);
    return o;
}

// thread = V neighbours of row y of image b; V = 4 where Fw is a multiple of 4 and the planes are 16-byte aligned: the fp32 plane
// moves in 16-byte, the uint16 planes in 8-byte, the byte planes in 4-byte accesses
template <int V>
__global__ __launch_bounds__(kThreads) void fusion_depth_kernel(const FuseArgs a) {
    __shared__ double coef[kMaxR][3];
    __shared__ int fit[kMaxR];
    const int b = blockIdx.z, y = blockIdx.y, x = (blockIdx.x * kThreads + threadIdx.x) * V;
    const FrameExtent f = frame_extent(a.sizes, b, a.Fh, a.Fw);
    if ((int)threadIdx.x < kMaxR) {
        const int r = threadIdx.x;
        const int K = min(max(a.region_count[b], 0), a.max_regions);
        const double *pl = a.planes + ((int64_t)b * a.max_regions + (r < a.max_regions ? r : 0)) * kPl;
        fit[r] = r < K && pl[P_STATUS] == 0.0;
        coef[r][0] = pl[P_A]; coef[r][1] = pl[P_B]; coef[r][2] = pl[P_G];
    }
    __syncthreads();
    if (x >= a.Fw) return;                                // V divides Fw: x + V <= Fw
    const int64_t at = b * a.plane + (int64_t)y * a.Fw + x;
    const double scale = a.scale[b * 4], dmin = (double)a.dmin, dmax = (double)a.dmax;
    const bool row = y < f.fh;
    if (V == 4) {
        uchar4 l4 = make_uchar4(0, 0, 0, 0), r4 = l4;
        ushort4 s4 = make_ushort4(0, 0, 0, 0);
        float4 d4 = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row && x < f.fw) {                            // the bytes behind the frame's last column are read, never used
            l4 = *reinterpret_cast<const uchar4 *>(a.labels + at);
            r4 = *reinterpret_cast<const uchar4 *>(a.region_map + at);
            s4 = *reinterpret_cast<const ushort4 *>(a.sensor_mm + at);
            d4 = *reinterpret_cast<const float4 *>(a.depth + at);
        }
        const int l[4] = {l4.x, l4.y, l4.z, l4.w}, r[4] = {r4.x, r4.y, r4.z, r4.w}, s[4] = {s4.x, s4.y, s4.z, s4.w};
        const float d[4] = {d4.x, d4.y, d4.z, d4.w};
        Fused o[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            o[k] = fuse_pixel(x + k, y, row && x + k < f.fw, l[k], r[k], s[k], d[k], a.lo_mm, a.hi_mm, dmin, dmax, scale, coef, fit);
        *reinterpret_cast<float4 *>(a.out + at) = make_float4(o[0].v, o[1].v, o[2].v, o[3].v);
        *reinterpret_cast<ushort4 *>(a.out_mm + at) = make_ushort4(o[0].mm, o[1].mm, o[2].mm, o[3].mm);
        *reinterpret_cast<uchar4 *>(a.source + at) = make_uchar4(o[0].src, o[1].src, o[2].src, o[3].src);
    } else {
        const bool inside = row && x < f.fw;
        const Fused o = fuse_pixel(x, y, inside, inside ? a.labels[at] : 0, inside ? a.region_map[at] : 0, inside ? a.sensor_mm[at] : 0,
                                   inside ? a.depth[at] : 0.f, a.lo_mm, a.hi_mm, dmin, dmax, scale, coef, fit);
        a.out[at] = o.v;
        a.out_mm[at] = o.mm;
        a.source[at] = o.src;
    }
}

bool bad_dims(int32_t B, int32_t Fh, int32_t Fw, int32_t max_regions) {
    return B < 1 || B > kMaxB || Fh < 1 || Fw < 1 || Fh > 16384 || Fw > 16384 || max_regions < 1 || max_regions > kMaxR;
}
bool bad_range(int32_t lo_mm, int32_t hi_mm) { return lo_mm < 1 || hi_mm > 65535 || lo_mm > hi_mm; }

}  // namespace

// bytes of gwd_query_workspace(GWD_WS_FUSION, {B, Fh, Fw}) (optim.hip)
int64_t gwd_fusion_workspace_bytes(int64_t B, int64_t Fh, int64_t Fw) {
    if (B < 1 || B > kMaxB || Fh < 1 || Fw < 1 || Fh > 16384 || Fw > 16384) return -1;
    return layout(B, Fh, Fw).total;
}

extern "C" int gwd_fusion_ring(const uint8_t *labels, const uint16_t *sensor_mm, const uint16_t *depth_mm, const int32_t *sizes,
                               const uint8_t *region_map, const int32_t *region_count, int32_t B, int32_t Fh, int32_t Fw,
                               int32_t max_regions, int32_t ring, int32_t gap, int32_t lo_mm, int32_t hi_mm, int32_t align,
                               int32_t min_align, void *workspace, uint8_t *fusion_ring, double *fusion_scale, void *stream) {
    if (!labels || !sensor_mm || !depth_mm || !sizes || !region_map || !region_count || !workspace || !fusion_ring || !fusion_scale)
        return -1;
    if (bad_dims(B, Fh, Fw, max_regions) || bad_range(lo_mm, hi_mm) || min_align < 0) return -1;
    if (ring < 1 || ring > kMaxRing || gap < 0 || gap >= ring) return -2;
    if (((uintptr_t)workspace & 15) || ((uintptr_t)sensor_mm & 1) || ((uintptr_t)depth_mm & 1) || ((uintptr_t)sizes & 3) ||
        ((uintptr_t)region_count & 3) || ((uintptr_t)fusion_scale & 7))
        return -3;
    const Layout l = layout(B, Fh, Fw);
    char *ws = (char *)workspace;
    RingArgs a;
    a.labels = labels; a.region_map = region_map; a.sensor_mm = sensor_mm; a.depth_mm = depth_mm; a.sizes = sizes;
    a.region_count = region_count; a.rowcode = (uint8_t *)(ws + l.rowcode); a.ring_map = fusion_ring;
    a.sums = (unsigned long long *)(ws + l.sums); a.scale = fusion_scale;
    a.plane = (int64_t)Fh * Fw;
    a.B = B; a.Fh = Fh; a.Fw = Fw; a.max_regions = max_regions; a.ring = ring; a.gap = gap; a.lo_mm = lo_mm; a.hi_mm = hi_mm;
    a.align = align != 0; a.min_align = min_align;
    const hipStream_t s = (hipStream_t)stream;
    fusion_row_kernel<<<dim3((Fw + kThreads - 1) / kThreads, Fh, B), kThreads, 0, s>>>(a);
    GWD_CHECK_LAUNCH();
    fusion_col_kernel<<<dim3((Fw + kThreads - 1) / kThreads, (Fh + kRows - 1) / kRows, B), kThreads, 0, s>>>(a);
    GWD_CHECK_LAUNCH();
    fusion_scale_kernel<<<1, 64, 0, s>>>(a);
    GWD_CHECK_LAUNCH();
    return 0;
}

extern "C" int gwd_fusion_planes(const uint8_t *fusion_ring, const uint16_t *sensor_mm, const int32_t *sizes,
                                 const int32_t *region_count, const int64_t *records, int32_t B, int32_t Fh, int32_t Fw,
                                 int32_t max_regions, int32_t ring, int32_t lo_mm, int32_t hi_mm, double trim, int32_t min_ring,
                                 double max_rms, void *workspace, double *fusion_planes, void *stream) {
    if (!fusion_ring || !sensor_mm || !sizes || !region_count || !records || !workspace || !fusion_planes) return -1;
    if (bad_dims(B, Fh, Fw, max_regions) || bad_range(lo_mm, hi_mm) || min_ring < 0) return -1;
    if (ring < 1 || ring > kMaxRing || !(trim >= 0.0) || !(trim < 1e300) || !(max_rms >= 0.0)) return -2;
    if (((uintptr_t)workspace & 15) || ((uintptr_t)sensor_mm & 1) || ((uintptr_t)sizes & 3) || ((uintptr_t)region_count & 3) ||
        ((uintptr_t)records & 7) || ((uintptr_t)fusion_planes & 7))
        return -3;
    FitArgs a;
    a.ring_map = fusion_ring; a.sensor_mm = sensor_mm; a.sizes = sizes; a.region_count = region_count;
    a.records = (const long long *)records; a.planes = fusion_planes;
    a.partial = (long long *)((char *)workspace + layout(B, Fh, Fw).partial);
    a.plane = (int64_t)Fh * Fw;
    a.B = B; a.Fh = Fh; a.Fw = Fw; a.max_regions = max_regions; a.ring = ring; a.lo_mm = lo_mm; a.hi_mm = hi_mm;
    a.min_ring = min_ring; a.nb = Fh < kPlaneBlocks ? Fh : kPlaneBlocks; a.trim = trim; a.max_rms = max_rms;
    const hipStream_t s = (hipStream_t)stream;
    const dim3 mg(a.nb, B), sg(max_regions, B);
    fusion_moments_kernel<0><<<mg, kThreads, 0, s>>>(a);
    GWD_CHECK_LAUNCH();
    fusion_solve_kernel<0><<<sg, 64, 0, s>>>(a);
    GWD_CHECK_LAUNCH();
    fusion_moments_kernel<1><<<mg, kThreads, 0, s>>>(a);
    GWD_CHECK_LAUNCH();
    fusion_solve_kernel<1><<<sg, 64, 0, s>>>(a);
    GWD_CHECK_LAUNCH();
    fusion_moments_kernel<2><<<mg, kThreads, 0, s>>>(a);
    GWD_CHECK_LAUNCH();
    fusion_solve_kernel<2><<<sg, 64, 0, s>>>(a);
    GWD_CHECK_LAUNCH();
    fusion_moments_kernel<3><<<mg, kThreads, 0, s>>>(a);
    GWD_CHECK_LAUNCH();
    fusion_solve_kernel<3><<<sg, 64, 0, s>>>(a);
    GWD_CHECK_LAUNCH();
    return 0;
}

extern "C" int gwd_fusion_depth(const uint8_t *labels, const uint16_t *sensor_mm, const float *depth, const int32_t *sizes,
                                const uint8_t *region_map, const int32_t *region_count, const double *fusion_planes,
                                const double *fusion_scale, int32_t B, int32_t Fh, int32_t Fw, int32_t max_regions, int32_t lo_mm,
                                int32_t hi_mm, float min_depth, float max_depth, float *depth_fused, uint16_t *depth_fused_mm,
                                uint8_t *fused_source, void *stream) {
    if (!labels || !sensor_mm || !depth || !sizes || !region_map || !region_count || !fusion_planes || !fusion_scale || !depth_fused ||
        !depth_fused_mm || !fused_source)
        return -1;
    if (bad_dims(B, Fh, Fw, max_regions) || bad_range(lo_mm, hi_mm) || !(min_depth < max_depth) || !(min_depth > 0.f)) return -1;
    if (((uintptr_t)sensor_mm & 1) || ((uintptr_t)depth & 3) || ((uintptr_t)sizes & 3) || ((uintptr_t)region_count & 3) ||
        ((uintptr_t)fusion_planes & 7) || ((uintptr_t)fusion_scale & 7) || ((uintptr_t)depth_fused & 3) || ((uintptr_t)depth_fused_mm & 1))
        return -3;
    FuseArgs a;
    a.labels = labels; a.region_map = region_map; a.sensor_mm = sensor_mm; a.depth = depth; a.sizes = sizes;
    a.region_count = region_count; a.planes = fusion_planes; a.scale = fusion_scale; a.out = depth_fused; a.out_mm = depth_fused_mm;
    a.source = fused_source;
    a.plane = (int64_t)Fh * Fw;
    a.B = B; a.Fh = Fh; a.Fw = Fw; a.max_regions = max_regions; a.lo_mm = lo_mm; a.hi_mm = hi_mm; a.dmin = min_depth; a.dmax = max_depth;
    const uintptr_t all = (uintptr_t)labels | (uintptr_t)region_map | (uintptr_t)sensor_mm | (uintptr_t)depth | (uintptr_t)depth_fused |
                          (uintptr_t)depth_fused_mm | (uintptr_t)fused_source;
    const hipStream_t s = (hipStream_t)stream;
    if (Fw % 4 == 0 && !(all & 15))
        fusion_depth_kernel<4><<<dim3((Fw / 4 + kThreads - 1) / kThreads, Fh, B), kThreads, 0, s>>>(a);
    else
        fusion_depth_kernel<1><<<dim3((Fw + kThreads - 1) / kThreads, Fh, B), kThreads, 0, s>>>(a);
    GWD_CHECK_LAUNCH();
    return 0;
}
