// L-CNN's line NMS over the detector's queries on the device: what every consumer of the reference's line output runs on the host
// first (postprocess, evaluation/eval_post_online.py:44-91, a pure-Python double loop), as ONE launch with one workgroup (one wave)
// per image - no atomics, no memset, every output element written.
//
//   scores        softmax probability of class 0, the expression of line_post_kernel (csrc/postproc.hip) bit for bit
//   points        the first two points of each query as (y, x), times (h, w) in fp32, then f64 (csrc/linescore.hip does the same)
//   trim          cut at the first i > 0 whose ld values all equal query 0's (eval_post_online.py:127-131), per image
//   floor         only score > min_score enters (a NaN score never does); min_score NaN = no floor
//   twin          the surviving queries of image b + twin are candidates of image b as well, mirrored back by hflip_lines' rule
//                 (src/datasets/transforms_depth.py:218-222): end points swapped, x -> w - x in fp32 on the pixel values
//   order         query order (what the reference passes), or the places of a given permutation per image; with a twin the two
//                 lists are concatenated (query order) or merged by score, originals first on ties (given order)
//   NMS           postprocess(candidates, _, diag * t, tol = 0, do_clip = False): the pair geometry of candidate i against the kept
//                 lines runs across the lanes, the hits are walked in kept order through ls_interval
//   output        row r of an image = its r-th kept line (the running count of kept lines is the row)
//
// Geometry is f64 with no contraction (csrc/linescore.h says why and holds the scalar functions).
#include "common.h"
#include "linescore.h"
#pragma clang fp contract(off)

namespace {

constexpr int LN_MAXC = 1024;          // candidates per image: Q, or 2 Q with a twin

struct LineNmsArgs {
    const float *logits, *lines;
    const int32_t *sizes, *order;
    double *out_lines;
    float *out_scores;
    int32_t *out_ids, *out_count;
    double t;
    float min_score;
    int32_t Q, ld, twin;
};

// A "slot" names a query of the image or of its twin: slot = query index, + Q for the twin's - the value nms_ids reports.
// LDS (static, 42 KB): px and sc by slot; cand = the slots that enter, by place; perm = the same in candidate order; keptslot and
// iv = slot and (start, end) of the r-th kept line.  iv's storage holds the score keys of the merge before the NMS starts.
__global__ __launch_bounds__(64) void line_nms_kernel(const LineNmsArgs a) {
    __shared__ __attribute__((aligned(16))) float px[LN_MAXC * 4];
    __shared__ double iv[LN_MAXC * 2];
    __shared__ float sc[LN_MAXC];
    __shared__ uint16_t cand[LN_MAXC], perm[LN_MAXC], keptslot[LN_MAXC];
    const int Q = a.Q, ld = a.ld, twin = a.twin, C = twin ? 2 * Q : Q;
    const int b = blockIdx.x, lane = threadIdx.x;
    const int32_t hi = a.sizes[2 * b], wi = a.sizes[2 * b + 1];
    const float hf = (float)hi, wf = (float)wi;

    // scores, pixel points (the twin's mirrored back), the duplicate trim of either list
    int first0 = Q, first1 = Q;
    for (int s = lane; s < C; s += 64) {
        const int L = s >= Q ? 1 : 0, q = s - L * Q;
        const int64_t at = (int64_t)(b + L * twin) * Q + q;
        const float l0 = a.logits[at * 2], l1 = a.logits[at * 2 + 1];
        const float m = fmaxf(l0, l1), e0 = expf(l0 - m), e1 = expf(l1 - m);
        sc[s] = (l0 != l0 || l1 != l1) ? __builtin_nanf("") : __fdiv_rn(e0, e0 + e1);
        const float *src = a.lines + at * ld, *zero = a.lines + (at - q) * ld;
        const float y1 = src[1] * hf, x1 = src[0] * wf, y2 = src[3] * hf, x2 = src[2] * wf;
        px[s * 4 + 0] = L ? y2 : y1;
        px[s * 4 + 1] = L ? wf - x2 : x1;
        px[s * 4 + 2] = L ? y1 : y2;
        px[s * 4 + 3] = L ? wf - x1 : x2;
        bool eq = q > 0;
        for (int k = 0; k < ld; ++k) eq = eq && src[k] == zero[k];
        if (eq && L == 0) first0 = min(first0, q);
        if (eq && L == 1) first1 = min(first1, q);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        first0 = min(first0, __shfl_xor(first0, o, 64));
        first1 = min(first1, __shfl_xor(first1, o, 64));
    }
    __syncthreads();

    // the candidates by place: a prefix count over the places that enter
    const bool no_floor = a.min_score != a.min_score;
    int n = 0;
    for (int base = 0; base < C; base += 64) {
        const int k = base + lane;
        bool in = false;
        int slot = 0;
        if (k < C) {
            const int L = k >= Q ? 1 : 0, kk = k - L * Q;
            const int q = a.order ? a.order[(int64_t)(b + L * twin) * Q + kk] : kk;          // device data: checked before use
            if (q >= 0 && q < Q && q < (L ? first1 : first0)) {
                slot = L * Q + q;
                in = no_floor || sc[slot] > a.min_score;
            }
        }
        const unsigned long long mask = __ballot(in);
        if (in) cand[n + __popcll(mask & ((1ull << lane) - 1ull))] = (uint16_t)slot;
        n += __popcll(mask);
    }
    __syncthreads();

    // candidate order: the places as they are, or - two lists in a given order - merged by score: candidate i goes to the place
    // given by the number of candidates that beat it (higher key, or equal key and earlier place; the image's own places come
    // first).  A total order, so the ranks are a permutation of 0..n-1 whatever the scores hold.
    const bool merge = a.order != nullptr && twin != 0;
    if (merge) {
        uint32_t *key = (uint32_t *)iv;
        for (int i = lane; i < n; i += 64) key[i] = score_key(sc[cand[i]]);
        __syncthreads();
        for (int i = lane; i < n; i += 64) {
            const uint32_t mine = key[i];
            int rank = 0;
            for (int j = 0; j < n; ++j) {
                const uint32_t k = key[j];
                rank += (k > mine || (k == mine && j < i)) ? 1 : 0;
            }
            perm[rank] = cand[i];
        }
        __syncthreads();
    }
    const uint16_t *P = merge ? perm : cand;

    // NMS: lanes do the pair geometry of candidate i against the kept lines; the pairs that pass the distance test are then walked
    // in kept order (a ballot, lowest bit first) through the interval update.
    const double diag = sqrt((double)hi * (double)hi + (double)wi * (double)wi);
    const double thr = diag * a.t, thr2 = thr * thr;
    int nk = 0;
    for (int i = 0; i < n; ++i) {
        const int slot = P[i];
        const double p[2] = {(double)px[slot * 4 + 0], (double)px[slot * 4 + 1]}, q[2] = {(double)px[slot * 4 + 2], (double)px[slot * 4 + 3]};
        double start = 0.0, end = 1.0;
        bool done = false;
        for (int base = 0; base < nk && !done; base += 64) {
            const int r = base + lane;
            double la = 0.0, lb = 0.0;
            bool hit = false;
            if (r < nk) {
                const int j = keptslot[r];
                const double pj[2] = {(double)px[j * 4 + 0], (double)px[j * 4 + 1]}, qj[2] = {(double)px[j * 4 + 2], (double)px[j * 4 + 3]};
                const double sj = iv[r * 2], ej = iv[r * 2 + 1];
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
        if (!(start >= end)) {                             // the same in every lane
            if (lane == 0) {
                iv[nk * 2] = start;
                iv[nk * 2 + 1] = end;
                keptslot[nk] = (uint16_t)slot;
            }
            ++nk;
        }
        __syncthreads();
    }

    // rows: the kept lines in candidate order, then zeros / 0 / -1
    for (int r = lane; r < C; r += 64) {
        const int64_t at = (int64_t)b * C + r;
        double l[4] = {0.0, 0.0, 0.0, 0.0};
        float s = 0.0f;
        int32_t id = -1;
        if (r < nk) {
            id = keptslot[r];
            s = sc[id];
            const double y1 = (double)px[id * 4 + 0], x1 = (double)px[id * 4 + 1], y2 = (double)px[id * 4 + 2], x2 = (double)px[id * 4 + 3];
            const double st = iv[r * 2], en = iv[r * 2 + 1];
            l[0] = ls_along(x1, x2, st);
            l[1] = ls_along(y1, y2, st);
            l[2] = ls_along(x1, x2, en);
            l[3] = ls_along(y1, y2, en);
        }
        for (int k = 0; k < 4; ++k) a.out_lines[at * 4 + k] = l[k];
        a.out_scores[at] = s;
        a.out_ids[at] = id;
    }
    if (lane == 0) a.out_count[b] = nk;
}

}  // namespace

extern "C" int gwd_line_nms(const float *logits, const float *lines, const int32_t *sizes, const int32_t *order, double t,
                            float min_score, double *nms_lines, float *nms_scores, int32_t *nms_ids, int32_t *nms_count, int32_t B,
                            int32_t Q, int32_t ld, int32_t twin, void *stream) {
    if (B <= 0 || Q <= 0 || !logits || !lines || !sizes || !nms_lines || !nms_scores || !nms_ids || !nms_count) return -1;
    if (ld != 4 && ld != 6) return -1;
    if (twin != 0 && twin != B) return -1;
    if (!(t >= 0.0)) return -1;
    if ((int64_t)Q * (twin ? 2 : 1) > LN_MAXC) return -2;
    LineNmsArgs a;
    a.logits = logits, a.lines = lines, a.sizes = sizes, a.order = order;
    a.out_lines = nms_lines, a.out_scores = nms_scores, a.out_ids = nms_ids, a.out_count = nms_count;
    a.t = t, a.min_score = min_score, a.Q = Q, a.ld = ld, a.twin = twin;
    line_nms_kernel<<<B, 64, 0, (hipStream_t)stream>>>(a);
    GWD_CHECK_LAUNCH();
    return 0;
}
