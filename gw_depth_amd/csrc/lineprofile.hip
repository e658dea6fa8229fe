// Line profiles on the device: every detected line of InferenceSession.predict_frames (nms_lines / lines, frame pixels) walked
// through the dense results of the same call (labels uint8, depth_mm uint16, region_map uint8, [B][Fh][Fw], top-left aligned frames,
// sizes on the device) - how far away its two ends are, on which side the glass lies, which pane it frames.
// The semantics are tests/line_profile_ref.py's; the scalar geometry is csrc/lineprobe.h, which a CPU test also compiles.
//
// gwd_line_profiles     ONE launch for all B x C rows.  One 64-lane wave per line, four lines per workgroup; lane l takes the samples
//                       l, l + 64, ... in turn.  The work is ragged and a handful of gathers per sample: latency-bound, so there
//                       is no more machinery than that.
//   pass 1              the three probes of every sample: exact counts (in the frame, glass, with depth - three 16-bit fields of one
//                       64-bit word per probe, folded through __shfl_xor), the two 33-bin region histograms of the wave in LDS
//                       (integer adds: their order changes no bit), and the sums of u = t - 1/2 and w = 1000 / mm;
//   pass 2              the centred sums about those means;
//   pass 3              the squared residuals of the fit.
//                       The later passes gather the pixels again (they are in L2) rather than keep up to 32 samples x 3 probes per
//                       lane.  Every fp64 sum is the lane's own samples in order, then the same fixed xor tree: no atomics on
//                       floats, no global atomics, no memset; repeated calls are bit-identical, and a line's record depends on
//                       neither its row nor its neighbours nor the plane size.
// Geometry and fit are fp64 with no contraction (lineprobe.h sets the pragma for this whole file).
#include "common.h"
#include "lineprobe.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;                     // lines per workgroup
constexpr int kBins = GWD_REGION_MAX + 1;                 // bin 0 = in no kept region
constexpr int kMaxB = 16;

struct ProfileArgs {
    const void *lines;
    const int32_t *count, *order, *sizes;
    const uint8_t *labels, *region_map;
    const uint16_t *depth_mm;
    const double *intrinsics;
    int32_t *counts, *kind;
    double *fits, *points;
    int64_t plane;
    double offset;
    int32_t B, C, Fh, Fw, f64, max_samples, lo_mm, hi_mm, hi, lo;
};

// 1 = glass on side a only, 2 = on side b only, 3 = on both, 4 = on neither, 0 = anything else; all in integers
__device__ __forceinline__ int kind_of(int a_in, int a_glass, int b_in, int b_glass, int hi, int lo) {
    const bool ag = a_in > 0 && 1000 * a_glass >= hi * a_in, an = a_in > 0 && 1000 * a_glass <= lo * a_in;
    const bool bg = b_in > 0 && 1000 * b_glass >= hi * b_in, bn = b_in > 0 && 1000 * b_glass <= lo * b_in;
    return ag && bn ? 1 : bg && an ? 2 : ag && bg ? 3 : an && bn ? 4 : 0;
}

__global__ __launch_bounds__(kThreads) void line_profile_kernel(const ProfileArgs a) {
    __shared__ int hist[kWaves][2][kBins];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row = blockIdx.x * kWaves + wave;
    const bool live = row < a.B * a.C;                    // everything below is uniform in a wave; every wave reaches both barriers
    const int b = live ? row / a.C : 0, r = live ? row - b * a.C : 0;
    for (int k = lane; k < 2 * kBins; k += 64) (&hist[wave][0][0])[k] = 0;

    int status = 3, fh = 0, fw = 0;                       // 3: a row from count[b] on
    double ends[4] = {0.0, 0.0, 0.0, 0.0};
    LpLine ln;
    ln.x1 = ln.y1 = ln.dx = ln.dy = ln.ox = ln.oy = 0.0;
    ln.n = 0;
    if (live && r < min(max(a.count[b], 0), a.C)) {
        status = 2;                                       // 2: a degenerate line (or a source row outside the list)
        const int src = a.order ? a.order[(int64_t)b * a.C + r] : r;
        if (src >= 0 && src < a.C) {
            const int64_t at = ((int64_t)b * a.C + src) * 4;
#pragma unroll
            for (int k = 0; k < 4; ++k) ends[k] = a.f64 ? ((const double *)a.lines)[at + k] : (double)((const float *)a.lines)[at + k];
            ln = lp_line(ends[0], ends[1], ends[2], ends[3], a.offset, a.max_samples);
            if (ln.n) status = 0;
        }
        fh = frame_side(a.sizes[2 * b], a.Fh);
        fw = frame_side(a.sizes[2 * b + 1], a.Fw);
    }
    const int S = status == 0 ? ln.n + 1 : 0;
    const uint8_t *__restrict__ L = a.labels + b * a.plane;
    const uint16_t *__restrict__ D = a.depth_mm + b * a.plane;
    const uint8_t *__restrict__ M = a.region_map ? a.region_map + b * a.plane : nullptr;
    __syncthreads();

    // ---- pass 1: counts, histograms, sums of u and w
    unsigned long long cnt[3] = {0ull, 0ull, 0ull};       // in the frame | glass << 16 | with depth << 32 (each <= 2048)
    double su[3] = {0.0, 0.0, 0.0}, sw[3] = {0.0, 0.0, 0.0};
    for (int k = lane; k < S; k += 64) {
        const double u = lp_t(ln, k) - 0.5;
#pragma unroll
        for (int p = 0; p < 3; ++p) {
            double x, y;
            lp_probe(ln, k, p, x, y);
            const long long at = lp_pixel(x, y, fh, fw, a.Fw);
            if (at < 0) continue;
            const int mm = D[at];
            const bool ok = mm >= a.lo_mm && mm <= a.hi_mm;
            cnt[p] += 1ull | (L[at] == 1 ? 1ull << 16 : 0ull) | (ok ? 1ull << 32 : 0ull);
            if (ok) {
                su[p] += u;
                sw[p] += 1000.0 / (double)mm;
            }
            if (p > 0 && M) {
                const int rank = M[at];
                if (rank > 0 && rank < kBins) atomicAdd(&hist[wave][p - 1][rank], 1);
            }
        }
    }
    int n_in[3], n_glass[3], n_depth[3];
    double mu[3], mw[3], dn[3];
    bool fit[3];
#pragma unroll
    for (int p = 0; p < 3; ++p) {
        const unsigned long long c = wave_sum_u64(cnt[p]);
        n_in[p] = (int)(c & 0xffffull), n_glass[p] = (int)((c >> 16) & 0xffffull), n_depth[p] = (int)((c >> 32) & 0xffffull);
        fit[p] = n_depth[p] >= 2;
        dn[p] = (double)n_depth[p];
        const double s1 = wave_sum_d(su[p]), s2 = wave_sum_d(sw[p]);
        mu[p] = fit[p] ? s1 / dn[p] : 0.0;
        mw[p] = fit[p] ? s2 / dn[p] : 0.0;
    }

    // ---- pass 2: centred sums; pass 3: squared residuals.  The same samples, gathered again.
    double slope[3] = {0.0, 0.0, 0.0}, rms[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int pass = 2; pass <= 3; ++pass) {
        double s1[3] = {0.0, 0.0, 0.0}, s2[3] = {0.0, 0.0, 0.0};
        for (int k = lane; k < S; k += 64) {
            const double u = lp_t(ln, k) - 0.5;
#pragma unroll
            for (int p = 0; p < 3; ++p) {
                if (!fit[p]) continue;
                double x, y;
                lp_probe(ln, k, p, x, y);
                const long long at = lp_pixel(x, y, fh, fw, a.Fw);
                if (at < 0) continue;
                const int mm = D[at];
                if (mm < a.lo_mm || mm > a.hi_mm) continue;
                const double cu = u - mu[p], cw = 1000.0 / (double)mm - mw[p];
                if (pass == 2) {
                    s1[p] += cu * cu;
                    s2[p] += cu * cw;
                } else {
                    const double e = cw - slope[p] * cu;
                    s1[p] += e * e;
                }
            }
        }
#pragma unroll
        for (int p = 0; p < 3; ++p) {
            if (!fit[p]) continue;
            if (pass == 2) {
                const double suu = wave_sum_d(s1[p]), suw = wave_sum_d(s2[p]);
                slope[p] = suw / suu;                     // two or more distinct t: suu > 0
            } else {
                rms[p] = sqrt(wave_sum_d(s1[p]) / dn[p]);
            }
        }
    }

    // ---- the pane each side frames: the rank with the most samples, ties to the lower rank
    __syncthreads();
    int region[2];
#pragma unroll
    for (int side = 0; side < 2; ++side) {
        const int c = lane < GWD_REGION_MAX ? hist[wave][side][lane + 1] : 0;
        int key = c > 0 ? (c << 6) | (63 - lane) : 0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) key = max(key, __shfl_xor(key, o, 64));
        region[side] = key ? 63 - (key & 63) : -1;
    }

    if (!live || lane != 0) return;
    const double nan = __builtin_nan("");
    int32_t *oc = a.counts + (int64_t)row * GWD_PROFILE_COUNTS;
    double *of = a.fits + (int64_t)row * 15;
    oc[0] = S;
    double w_end[2] = {nan, nan};
#pragma unroll
    for (int p = 0; p < 3; ++p) {
        oc[1 + 3 * p] = n_in[p], oc[2 + 3 * p] = n_glass[p], oc[3 + 3 * p] = n_depth[p];
        double w0 = 0.0, w1 = 0.0, e = 0.0, st = (double)status;
        if (status == 2) w0 = w1 = e = nan;
        if (status == 0) {
            if (fit[p]) {
                w0 = mw[p] + slope[p] * (-0.5 - mu[p]);
                w1 = mw[p] + slope[p] * (0.5 - mu[p]);
                e = rms[p];
                if (p == 0) w_end[0] = w0, w_end[1] = w1;
            } else {
                w0 = w1 = e = nan;
                st = 1.0;
            }
        }
        of[5 * p + 0] = w0, of[5 * p + 1] = w1, of[5 * p + 2] = e, of[5 * p + 3] = dn[p], of[5 * p + 4] = st;
    }
    oc[10] = region[0], oc[11] = region[1];
    a.kind[row] = status == 0 ? kind_of(n_in[1], n_glass[1], n_in[2], n_glass[2], a.hi, a.lo) : 0;
    if (a.points) {
        const double *cam = a.intrinsics + 4 * b;         // fx, fy, cx, cy
        double *op = a.points + (int64_t)row * 6;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            double X = nan, Y = nan, Z = nan;
            if (w_end[e] > 0.0) {                         // NaN (no fit) compares false
                Z = 1.0 / w_end[e];
                X = (ends[2 * e] - cam[2]) / cam[0] * Z;
                Y = (ends[2 * e + 1] - cam[3]) / cam[1] * Z;
            }
            op[3 * e + 0] = X, op[3 * e + 1] = Y, op[3 * e + 2] = Z;
        }
    }
}

}  // namespace

extern "C" int gwd_line_profiles(const void *lines, int32_t lines_dtype, const int32_t *count, const int32_t *order,
                                 const uint8_t *labels, const uint16_t *depth_mm, const int32_t *sizes, const uint8_t *region_map,
                                 const double *intrinsics, int32_t B, int32_t C, int32_t Fh, int32_t Fw, double offset,
                                 int32_t max_samples, int32_t lo_mm, int32_t hi_mm, int32_t hi, int32_t lo, int32_t *counts,
                                 double *fits, int32_t *kind, double *line_points, void *stream) {
    if (!lines || !count || !labels || !depth_mm || !sizes || !counts || !fits || !kind) return -1;
    if ((intrinsics == nullptr) != (line_points == nullptr)) return -1;
    if (B < 1 || B > kMaxB || C < 1 || Fh < 1 || Fw < 1 || Fh > 16384 || Fw > 16384) return -1;
    if (!(offset > 0.0) || !(offset <= 16384.0) || lo_mm < 1 || hi_mm > 65535 || lo_mm > hi_mm) return -1;
    if (lo < 0 || hi > 1000 || lo >= hi) return -1;
    if ((lines_dtype != GWD_LINES_F32 && lines_dtype != GWD_LINES_F64) || C > GWD_PROFILE_MAX_LINES || max_samples < 2 ||
        max_samples > GWD_PROFILE_MAX_SAMPLES)
        return -2;
    if (((uintptr_t)lines & (lines_dtype == GWD_LINES_F64 ? 7 : 3)) || ((uintptr_t)count & 3) || ((uintptr_t)order & 3) ||
        ((uintptr_t)depth_mm & 1) || ((uintptr_t)sizes & 3) || ((uintptr_t)intrinsics & 7) || ((uintptr_t)counts & 3) ||
        ((uintptr_t)fits & 7) || ((uintptr_t)kind & 3) || ((uintptr_t)line_points & 7))
        return -3;
    ProfileArgs a;
    a.lines = lines; a.count = count; a.order = order; a.sizes = sizes; a.labels = labels; a.region_map = region_map;
    a.depth_mm = depth_mm; a.intrinsics = intrinsics; a.counts = counts; a.kind = kind; a.fits = fits; a.points = line_points;
    a.plane = (int64_t)Fh * Fw;
    a.offset = offset;
    a.B = B; a.C = C; a.Fh = Fh; a.Fw = Fw; a.f64 = lines_dtype == GWD_LINES_F64; a.max_samples = max_samples;
    a.lo_mm = lo_mm; a.hi_mm = hi_mm; a.hi = hi; a.lo = lo;
    line_profile_kernel<<<(B * C + kWaves - 1) / kWaves, kThreads, 0, (hipStream_t)stream>>>(a);
    GWD_CHECK_LAUNCH();
    return 0;
}
