// Structural-AP scoring of the line detector on the device: what the reference does per image on the host between evaluate() and
// its offline scripts, as ONE launch with one workgroup per image (no atomics, no memset, every output element written).
//
//   scores        softmax probability of class 0 (src/engine_glassrgbd.py:287,297)
//   lines         the first two points of each query as (y, x), times (h, w) in fp32 (evaluation/eval_post_online.py:133-134)
//   first trim    cut at the first i > 0 whose line equals line 0 (eval_post_online.py:127-131)
//   NMS           postprocess(lines, scores, diag * t, tol = 0, do_clip = False) (eval_post_online.py:44-91,142) for up to four
//                 t at once, one wave each.  The lines are taken in QUERY order, as the reference passes them - not score order.
//   rescale       kept lines times (128 / h, 128 / w) (eval_post_online.py:174-175)
//   second trim   of the kept lines (evaluation/eval-sAP-glassrgbd.py:55-59)
//   msTPFP        against gt * 128 (evaluation/lcnn/metric.py:194-210) for up to four distance thresholds
//
// Geometry is f64 with no contraction (csrc/linescore.h says why and holds the scalar functions, which a CPU test also compiles).
#include "common.h"
#include "linescore.h"
#pragma clang fp contract(off)

namespace {

constexpr int LS_MAXQ = 1024, LS_MAXG = 1024, LS_MAXT = 4, LS_MAXS = 4;

struct LineScoreArgs {
    const float *logits, *lines, *gt;
    const int32_t *sizes, *gt_count;
    uint8_t *flag;
    double *kept;
    float *score;
    int32_t *gt_seen;
    int64_t cap, slot;
    int32_t Q, ld, G, T, S;
    double nms[LS_MAXT], sap[LS_MAXS];
};

// Dynamic LDS: rec[T][Q][2] f64, then px[Q][4] fp32.  rec holds (start, end) of the NMS until the kept lines are written, then
// (match distance, choice | second-trim bit) of the same line - each record is rewritten only by the thread that owns the line.
__global__ __launch_bounds__(256) void line_score_kernel(const LineScoreArgs a) {
    extern __shared__ __attribute__((aligned(16))) char ls_smem[];
    __shared__ unsigned long long keptmask[LS_MAXT][LS_MAXQ / 64];
    __shared__ double firstline[LS_MAXT][4];
    __shared__ int wmin[4], firstkept[LS_MAXT];
    const int Q = a.Q, ld = a.ld, T = a.T, S = a.S;
    double *rec = (double *)ls_smem;
    float *px = (float *)(ls_smem + (size_t)T * Q * 16);
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t img = a.slot + b;
    const int32_t hi = a.sizes[2 * b], wi = a.sizes[2 * b + 1];
    const float hf = (float)hi, wf = (float)wi;
    const float *L = a.lines + (int64_t)b * Q * ld;

    // scores, pixel lines, first duplicate trim
    int first = Q;
    for (int q = tid; q < Q; q += 256) {
        const float l0 = a.logits[((int64_t)b * Q + q) * 2], l1 = a.logits[((int64_t)b * Q + q) * 2 + 1];
        const float m = fmaxf(l0, l1), e0 = expf(l0 - m), e1 = expf(l1 - m);
        a.score[img * Q + q] = (l0 != l0 || l1 != l1) ? __builtin_nanf("") : __fdiv_rn(e0, e0 + e1);
        const float *src = L + (int64_t)q * ld;
        px[q * 4 + 0] = src[1] * hf;            // pred_lines.reshape(-1, 3, 2).flip(-1): (y, x), engine_glassrgbd.py:288
        px[q * 4 + 1] = src[0] * wf;
        px[q * 4 + 2] = src[3] * hf;
        px[q * 4 + 3] = src[2] * wf;
        bool eq = q > 0;
        for (int k = 0; k < ld; ++k) eq = eq && src[k] == L[k];
        if (eq && q < first) first = q;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) first = min(first, __shfl_xor(first, o, 64));
    if (lane == 0) wmin[wave] = first;
    if (tid < LS_MAXT * (LS_MAXQ / 64)) keptmask[tid >> 4][tid & 15] = 0ull;
    const int ng = max(0, min(a.gt_count[b], a.G));
    if (tid == 0) a.gt_seen[img] = ng;
    __syncthreads();
    const int n = min(min(wmin[0], wmin[1]), min(wmin[2], wmin[3]));

    // NMS: wave t runs threshold t.  Lanes do the pair geometry of line i against the selected lines j < i; the selected pairs
    // that pass the distance test are then walked in order (a ballot, lowest bit first) through the interval update.
    const int t = wave;
    double thr2 = 0.0;
    if (t < T) {
        const double diag = sqrt((double)hi * (double)hi + (double)wi * (double)wi);
        const double thr = diag * a.nms[t];
        thr2 = thr * thr;
    }
    for (int i = 0; i < n; ++i) {
        if (t < T) {
            const double p[2] = {(double)px[i * 4 + 0], (double)px[i * 4 + 1]}, q[2] = {(double)px[i * 4 + 2], (double)px[i * 4 + 3]};
            double start = 0.0, end = 1.0;
            bool done = false;
            for (int base = 0; base < i && !done; base += 64) {
                const int j = base + lane;
                const bool sel = j < i && ((keptmask[t][base >> 6] >> lane) & 1ull);
                double la = 0.0, lb = 0.0;
                bool hit = false;
                if (sel) {
                    const double pj[2] = {(double)px[j * 4 + 0], (double)px[j * 4 + 1]}, qj[2] = {(double)px[j * 4 + 2], (double)px[j * 4 + 3]};
                    const double sj = rec[((size_t)t * Q + j) * 2], ej = rec[((size_t)t * Q + j) * 2 + 1];
                    const double ca[2] = {ls_along(pj[0], qj[0], sj), ls_along(pj[1], qj[1], sj)};
                    const double cb[2] = {ls_along(pj[0], qj[0], ej), ls_along(pj[1], qj[1], ej)};
                    hit = ls_pair(p, q, ca, cb, thr2, la, lb);
                }
                unsigned long long todo = __ballot(hit);
                while (todo != 0ull && !done) {
                    const int src = __ffsll((long long)todo) - 1;
                    todo &= todo - 1ull;
                    done = ls_interval(start, end, shfl_d(la, src), shfl_d(lb, src));
                }
            }
            if (lane == 0) {
                rec[((size_t)t * Q + i) * 2] = start;
                rec[((size_t)t * Q + i) * 2 + 1] = end;
                if (!(start >= end)) keptmask[t][i >> 6] |= 1ull << (i & 63);
            }
        }
        __syncthreads();
    }

    // the first kept line of each threshold, rescaled: what the second trim compares with
    const double sy = 128.0 / (double)hi, sx = 128.0 / (double)wi;
    if (tid < T) {
        int f = -1;
        for (int w = 0; w < (Q + 63) / 64 && f < 0; ++w)
            if (keptmask[tid][w] != 0ull) f = w * 64 + __ffsll((long long)keptmask[tid][w]) - 1;
        for (int k = 0; k < 4; ++k) firstline[tid][k] = 0.0;
        if (f >= 0) {
            const double s = rec[((size_t)tid * Q + f) * 2], e = rec[((size_t)tid * Q + f) * 2 + 1];
            const double y1 = (double)px[f * 4 + 0], x1 = (double)px[f * 4 + 1], y2 = (double)px[f * 4 + 2], x2 = (double)px[f * 4 + 3];
            firstline[tid][0] = ls_along(y1, y2, s) * sy;
            firstline[tid][1] = ls_along(x1, x2, s) * sx;
            firstline[tid][2] = ls_along(y1, y2, e) * sy;
            firstline[tid][3] = ls_along(x1, x2, e) * sx;
        }
        firstkept[tid] = f;
    }
    __syncthreads();

    // kept lines out, match distance and choice of every kept line
    const float *gt = a.gt + (int64_t)b * a.G * 4;
    for (int idx = tid; idx < T * Q; idx += 256) {
        const int tt = idx / Q, i = idx - tt * Q;
        const bool kept = (keptmask[tt][i >> 6] >> (i & 63)) & 1ull;
        double l[4] = {0.0, 0.0, 0.0, 0.0};
        if (kept) {
            double *r = rec + ((size_t)tt * Q + i) * 2;
            const double s = r[0], e = r[1];
            const double y1 = (double)px[i * 4 + 0], x1 = (double)px[i * 4 + 1], y2 = (double)px[i * 4 + 2], x2 = (double)px[i * 4 + 3];
            l[0] = ls_along(y1, y2, s) * sy;
            l[1] = ls_along(x1, x2, s) * sx;
            l[2] = ls_along(y1, y2, e) * sy;
            l[3] = ls_along(x1, x2, e) * sx;
            const bool dup = i != firstkept[tt] && l[0] == firstline[tt][0] && l[1] == firstline[tt][1] && l[2] == firstline[tt][2] &&
                             l[3] == firstline[tt][3];
            double best = __builtin_inf();
            long long choice = 0x3fffffff;                         // no ground truth: matches nothing
            for (int g = 0; g < ng; ++g) {
                const double gl[4] = {(double)gt[g * 4 + 1] * 128.0, (double)gt[g * 4 + 0] * 128.0, (double)gt[g * 4 + 3] * 128.0,
                                      (double)gt[g * 4 + 2] * 128.0};
                const double d = ls_match(l, gl);
                if (g == 0 || d < best) best = d, choice = g;      // np.argmin: the first minimum
            }
            r[0] = best;
            r[1] = __builtin_bit_cast(double, choice | (dup ? (1ll << 32) : 0ll));
        }
        double *out = a.kept + (((int64_t)tt * a.cap + img) * Q + i) * 4;
        for (int k = 0; k < 4; ++k) out[k] = l[k];
    }
    __syncthreads();

    // flags: a kept line is a true positive iff it is close enough and no EARLIER kept line with the same choice was - the hit
    // array of metric.py:201-209 without its serial walk.  Lines from the second trim's cut on are not scored.
    for (int idx = tid; idx < T * Q; idx += 256) {
        const int tt = idx / Q, i = idx - tt * Q;
        const bool kept = (keptmask[tt][i >> 6] >> (i & 63)) & 1ull;
        bool cut = !kept;
        unsigned blocked = 0u;
        double dist = 0.0;
        if (kept) {
            const double *r = rec + (size_t)tt * Q * 2;
            dist = r[i * 2];
            const long long mine = __builtin_bit_cast(long long, r[i * 2 + 1]);
            cut = (mine >> 32) & 1ll;
            for (int w = 0; w <= (i >> 6); ++w) {
                unsigned long long bits = keptmask[tt][w];
                if (w == (i >> 6)) bits &= (1ull << (i & 63)) - 1ull;          // strictly earlier lines
                while (bits != 0ull) {
                    const int k = w * 64 + __ffsll((long long)bits) - 1;
                    bits &= bits - 1ull;
                    const long long other = __builtin_bit_cast(long long, r[k * 2 + 1]);
                    cut = cut || ((other >> 32) & 1ll);
                    if ((int)other == (int)mine) {
                        const double dk = r[k * 2];
                        for (int s = 0; s < S; ++s) blocked |= (dk < a.sap[s] ? 1u : 0u) << s;
                    }
                }
            }
        }
        for (int s = 0; s < S; ++s) {
            const uint8_t f = cut ? 2 : ((dist < a.sap[s] && !((blocked >> s) & 1u)) ? 1 : 0);
            a.flag[(((int64_t)tt * S + s) * a.cap + img) * Q + i] = f;
        }
    }
}

}  // namespace

extern "C" int gwd_line_score(const float *logits, const float *lines, const int32_t *sizes, const float *gt, const int32_t *gt_count,
                              const double *nms_thresholds, int32_t T, const double *sap_thresholds, int32_t S, uint8_t *flag,
                              double *kept_lines, float *score, int32_t *gt_seen, int32_t B, int32_t Q, int32_t ld, int32_t G,
                              int64_t capacity, int64_t slot, void *stream) {
    if (B <= 0 || Q <= 0 || G < 0 || !logits || !lines || !sizes || !gt_count || !nms_thresholds || !sap_thresholds || !flag ||
        !kept_lines || !score || !gt_seen || (G > 0 && !gt))
        return -1;
    if (ld != 4 && ld != 6) return -1;
    if (T < 1 || T > LS_MAXT || S < 1 || S > LS_MAXS) return -1;
    if (slot < 0 || capacity < slot + B) return -1;
    if (Q > LS_MAXQ || G > LS_MAXG) return -2;
    LineScoreArgs a;
    a.logits = logits, a.lines = lines, a.gt = gt, a.sizes = sizes, a.gt_count = gt_count;
    a.flag = flag, a.kept = kept_lines, a.score = score, a.gt_seen = gt_seen;
    a.cap = capacity, a.slot = slot, a.Q = Q, a.ld = ld, a.G = G, a.T = T, a.S = S;
    for (int k = 0; k < LS_MAXT; ++k) a.nms[k] = k < T ? nms_thresholds[k] : 0.0;
    for (int k = 0; k < LS_MAXS; ++k) a.sap[k] = k < S ? sap_thresholds[k] : 0.0;
    const size_t lds = (size_t)T * Q * 16 + (size_t)Q * 16;
    if (lds > 48 * 1024) {
        const hipError_t e = hipFuncSetAttribute((const void *)line_score_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    line_score_kernel<<<B, 256, lds, (hipStream_t)stream>>>(a);
    GWD_CHECK_LAUNCH();
    return 0;
}
