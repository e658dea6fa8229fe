// Host build of gw_depth_amd/csrc/lineprobe.h for tests/test_line_profiles.py: the same scalar functions the device kernel calls,
// driven by a plain loop over the samples of one line.  Built by the test with g++ -ffp-contract=off into a shared object and
// called through ctypes.
#include "lineprobe.h"

// -> n (0: degenerate); pix[probe * max_samples + k] = the pixel of probe `probe` of sample k as iy * pitch + ix, or -1
extern "C" int lp_host_line(const double *line, double offset, int max_samples, int fh, int fw, int pitch, long long *pix) {
    const LpLine l = lp_line(line[0], line[1], line[2], line[3], offset, max_samples);
    if (!l.n) return 0;
    for (int p = 0; p < 3; ++p)
        for (int k = 0; k <= l.n; ++k) {
            double x, y;
            lp_probe(l, k, p, x, y);
            pix[(long long)p * max_samples + k] = lp_pixel(x, y, fh, fw, pitch);
        }
    return l.n;
}

extern "C" int lp_host_count(double L2, int max_samples) { return lp_sample_count(L2, max_samples); }
