"""Writes tests/golden/glass_regions.npz: the label masks (bit-packed) and uint16 depth planes the glass-region tests run on.

The masks are thresholded gaussian_filter noise; they are committed as data because the filter's last bits may differ between
scipy builds and flip thresholded pixels.  Depth: per 8-connected component a true plane in inverse depth plus seeded noise,
rounded to millimetres (tests/regions_ref.py: plane_depth); on the large mask the largest region is exactly planar before the
rounding, the second has every depth out of range (0 mm) and the third follows a quadratic in x, so that its fitted plane
crosses zero inside the region.

    python tools/make_regions_fixture.py
"""
import os
import sys

import numpy as np
from scipy.ndimage import gaussian_filter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import regions_ref as R  # noqa: E402

SPECS = (("large", 0, 300, 500, 3.0, 0.55), ("small", 1, 37, 53, 1.2, 0.5), ("medium", 2, 64, 70, 1.5, 0.5))


def make_mask(seed, h, w, sigma, thresh):
    f = gaussian_filter(np.random.default_rng(seed).random((h, w)), sigma=sigma)
    f = (f - f.min()) / (f.max() - f.min())
    return f > thresh


def main():
    out = {"names": np.array([s[0] for s in SPECS])}
    for name, seed, h, w, sigma, thresh in SPECS:
        mask = make_mask(seed, h, w, sigma, thresh)
        mm = R.plane_depth(mask, 100 + seed)
        if name == "large":
            lab, anchors, areas = R.components(mask, 8)
            rank = sorted(range(len(areas)), key=lambda k: (-areas[k], anchors[k]))
            ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
            sel = lab == rank[0] + 1                                   # exactly planar in inverse depth
            mm[sel] = np.rint(1000.0 / (0.6 + 4e-4 * (xs[sel] - xs[sel].mean()) - 3e-4 * (ys[sel] - ys[sel].mean()))).astype(np.uint16)
            mm[lab == rank[1] + 1] = 0                                 # no pixel with depth
            sel = lab == rank[2] + 1                                   # 10 m .. 0.2 m along x, quadratic in 1 / z
            t = (xs[sel] - xs[sel].min()) / max(xs[sel].max() - xs[sel].min(), 1.0)
            mm[sel] = np.rint(1000.0 / (0.1 + 4.9 * t * t)).astype(np.uint16)
        lab8, lab4 = R.components(mask, 8), R.components(mask, 4)
        print("%s: %d x %d, %d components 8-connected, %d 4-connected, %d of area >= 100, largest %d"
              % (name, h, w, len(lab8[1]), len(lab4[1]), int((lab8[2] >= 100).sum()), int(lab8[2].max())))
        out[name + "_shape"] = np.array([h, w], np.int32)
        out[name + "_bits"] = np.packbits(mask.ravel())
        out[name + "_mm"] = mm
    path = os.path.join(ROOT, "tests", "golden", "glass_regions.npz")
    np.savez_compressed(path, **out)
    print("%s: %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
