// Host build of gw_depth_amd/csrc/linescore.h for tests/test_line_score.py: the same scalar functions the device kernel calls, driven
// by a plain serial loop over one image (the sequencing of csrc/linescore.hip without its lanes).  Built by the test with g++
// -ffp-contract=off into a shared object and called through ctypes.
#include <cstdint>
#include <cmath>
#include <vector>

#include "linescore.h"

extern "C" int ls_host_image(const float *lines, int Q, int ld, int h, int w, const float *gt, int G, const double *nms, int T,
                             const double *sap, int S, uint8_t *flag, double *kept_lines, uint8_t *kept) {
    std::vector<double> px((size_t)Q * 4), start(Q), end(Q), dist(Q);
    std::vector<int> choice(Q);
    std::vector<char> dup(Q);
    const float hf = (float)h, wf = (float)w;
    int n = Q;
    for (int q = 0; q < Q; ++q) {
        const float *src = lines + (size_t)q * ld;
        const float y1 = src[1] * hf, x1 = src[0] * wf, y2 = src[3] * hf, x2 = src[2] * wf;        // fp32 products, then f64
        px[q * 4 + 0] = y1, px[q * 4 + 1] = x1, px[q * 4 + 2] = y2, px[q * 4 + 3] = x2;
        bool eq = q > 0;
        for (int k = 0; k < ld; ++k) eq = eq && src[k] == lines[k];
        if (eq && q < n) n = q;
    }
    const double diag = std::sqrt((double)h * (double)h + (double)w * (double)w), sy = 128.0 / (double)h, sx = 128.0 / (double)w;
    for (int t = 0; t < T; ++t) {
        const double thr = diag * nms[t], thr2 = thr * thr;
        uint8_t *kp = kept + (size_t)t * Q;
        double *out = kept_lines + (size_t)t * Q * 4;
        int first = -1;
        for (int i = 0; i < Q; ++i) {
            kp[i] = 0;
            for (int k = 0; k < 4; ++k) out[i * 4 + k] = 0.0;
        }
        for (int i = 0; i < n; ++i) {
            const double p[2] = {px[i * 4], px[i * 4 + 1]}, q[2] = {px[i * 4 + 2], px[i * 4 + 3]};
            double s = 0.0, e = 1.0;
            for (int j = 0; j < i; ++j) {
                if (!kp[j]) continue;
                const double ca[2] = {ls_along(px[j * 4], px[j * 4 + 2], start[j]), ls_along(px[j * 4 + 1], px[j * 4 + 3], start[j])};
                const double cb[2] = {ls_along(px[j * 4], px[j * 4 + 2], end[j]), ls_along(px[j * 4 + 1], px[j * 4 + 3], end[j])};
                double la, lb;
                if (!ls_pair(p, q, ca, cb, thr2, la, lb)) continue;
                if (ls_interval(s, e, la, lb)) break;
            }
            start[i] = s, end[i] = e;
            kp[i] = !(s >= e);
            if (kp[i] && first < 0) first = i;
        }
        for (int i = 0; i < n; ++i) {
            if (!kp[i]) continue;
            double *l = out + i * 4;
            l[0] = ls_along(px[i * 4], px[i * 4 + 2], start[i]) * sy;
            l[1] = ls_along(px[i * 4 + 1], px[i * 4 + 3], start[i]) * sx;
            l[2] = ls_along(px[i * 4], px[i * 4 + 2], end[i]) * sy;
            l[3] = ls_along(px[i * 4 + 1], px[i * 4 + 3], end[i]) * sx;
            const double *f = out + first * 4;
            dup[i] = i != first && l[0] == f[0] && l[1] == f[1] && l[2] == f[2] && l[3] == f[3];
            dist[i] = INFINITY;
            choice[i] = -1;
            for (int g = 0; g < G; ++g) {
                const double gl[4] = {(double)gt[g * 4 + 1] * 128.0, (double)gt[g * 4] * 128.0, (double)gt[g * 4 + 3] * 128.0,
                                      (double)gt[g * 4 + 2] * 128.0};
                const double d = ls_match(l, gl);
                if (g == 0 || d < dist[i]) dist[i] = d, choice[i] = g;
            }
        }
        for (int s = 0; s < S; ++s) {
            uint8_t *fl = flag + ((size_t)t * S + s) * Q;
            bool cut = false;
            for (int i = 0; i < Q; ++i) {
                fl[i] = 2;
                if (i >= n || !kp[i]) continue;
                cut = cut || dup[i];
                if (cut) continue;
                bool blocked = false;
                for (int k = 0; k < i; ++k) blocked = blocked || (kp[k] && choice[k] == choice[i] && dist[k] < sap[s]);
                fl[i] = (dist[i] < sap[s] && !blocked) ? 1 : 0;
            }
        }
    }
    return n;
}
