"""Generate tests/golden/frame_metrics.npz with the REAL reference's depth measures and confusion matrix on the CPU.

TEST INFRASTRUCTURE ONLY.  Usage: python tools/make_golden_frame_metrics.py   (needs the reference tree; see oracle/ref_stubs.py).

What runs is the reference's own, unmodified `compute_depth_errors` and `get_confusion_matrix` (src/util/metrics.py:197-218, 37-56),
imported under the stand-ins of oracle/ref_stubs.py.  This file draws three small frames, forms the ground truth the way the data set
does (depth_gt / 1000.0 in fp32 and seg_gt > 0: src/datasets/glassrgbd_norhint.py:273,275), clamps the prediction and takes the valid
pixels as evaluate() does (src/engine_glassrgbd.py:249-253), cuts every region's subset (all / glass / non-glass / eight GT-depth bins)
and hands each subset to those two functions.  Only arrays travel.

Frames (prediction fp32 + uint8 label, GT int32 millimetres + raw uint8 label):
  0   24 x 32  without glass; GT depths up to 7 m, so the bin [8, 10) stays empty; some GT exactly on the edges 1 m, 2 m and 4 m
  1   17 x 23  GT millimetres 0, 1, 10000 and 65535 among the values (all four invalid: g must lie strictly inside (0.001, 10));
               raw labels 0, 1, 128 and 255 (everything above 0 is glass); predicted labels 0, 1 and a few 7 / 255 (not counted)
  2    8 x 16  predictions with NaN, +inf, -inf, negatives, zeros and values beyond 10 m
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")
MIN_D, MAX_D = 1e-3, 10.0
EDGES = (0.5, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 8.0, 10.0)


def draw():
    rng = np.random.default_rng(20)
    frames = []
    # 0: no glass, an empty last bin, GT on bin edges
    h, w = 24, 32
    mm = rng.integers(300, 7000, size=(h, w)).astype(np.int32)
    mm[rng.random((h, w)) < 0.1] = 0
    mm[2, 3:6] = (1000, 2000, 4000)
    pred = (mm / 1000.0 * rng.uniform(0.7, 1.4, size=(h, w))).astype(np.float32)
    pred[mm == 0] = 1.5
    frames.append((pred, (rng.random((h, w)) < 0.2).astype(np.uint8), mm, np.zeros((h, w), np.uint8)))
    # 1: the special millimetre values, raw labels of every kind, predicted labels outside {0, 1}
    h, w = 17, 23
    mm = rng.integers(1, 12000, size=(h, w)).astype(np.int32)
    mm[0, :4] = (0, 1, 10000, 65535)
    mm[5, 5:9] = (9999, 2, 500, 8000)
    raw = rng.choice(np.array([0, 0, 1, 128, 255], np.uint8), size=(h, w))
    pred = rng.uniform(0.0, 11.0, size=(h, w)).astype(np.float32)
    lab = (rng.random((h, w)) < 0.5).astype(np.uint8)
    lab[3, 2:5] = (7, 255, 2)
    frames.append((pred, lab, mm, raw))
    # 2: predictions the clamp has to repair
    h, w = 8, 16
    mm = rng.integers(200, 9500, size=(h, w)).astype(np.int32)
    raw = (rng.random((h, w)) < 0.5).astype(np.uint8) * 255
    pred = rng.uniform(-1.0, 12.0, size=(h, w)).astype(np.float32)
    pred[0, :8] = (np.nan, np.inf, -np.inf, -3.0, 0.0, 1e-3, 10.0, 20.0)
    frames.append((pred, (rng.random((h, w)) < 0.5).astype(np.uint8), mm, raw))
    return frames


def main():
    from oracle import ref_stubs
    ref_stubs.install()
    from util import metrics as ref                       # the reference's src/util/metrics.py

    f32 = np.float32
    out = {"min_depth_eval": np.float64(MIN_D), "max_depth_eval": np.float64(MAX_D), "edges": np.asarray(EDGES, dtype=f32)}
    R = 3 + len(EDGES) - 1
    for i, (pred, lab, mm, raw) in enumerate(draw()):
        gt = mm.astype(f32) / f32(1000.0)                  # glassrgbd_norhint.py:273
        seg = (raw > 0).astype(np.int64)                   # :275
        p = pred.copy()
        with np.errstate(invalid="ignore"):
            p[p < MIN_D] = MIN_D                           # engine_glassrgbd.py:249-252
            p[p > MAX_D] = MAX_D
            p[np.isinf(p)] = MAX_D
            p[np.isnan(p)] = MIN_D
            valid = np.logical_and(gt > MIN_D, gt < MAX_D)  # :253
        e = np.asarray(EDGES, dtype=f32)
        masks = [valid, valid & (seg == 1), valid & (seg == 0)] + [valid & (gt >= e[k]) & (gt < e[k + 1]) for k in range(len(e) - 1)]
        measures = np.full((R, 9), np.nan)
        counts = np.zeros(R, dtype=np.int64)
        for r, m in enumerate(masks):
            counts[r] = int(m.sum())
            if counts[r]:
                measures[r] = [float(v) for v in ref.compute_depth_errors(gt[m], p[m])]
        keep = lab < 2                                     # a predicted label outside the two classes is not counted
        conf = ref.get_confusion_matrix(seg[keep], lab[keep].astype(np.int64), 2)
        out.update({"depth%d" % i: pred, "label%d" % i: lab, "mm%d" % i: mm, "raw%d" % i: raw, "ref_measures%d" % i: measures,
                    "ref_counts%d" % i: counts, "ref_conf%d" % i: conf.astype(np.int64).reshape(-1)})
    os.makedirs(GOLDEN_DIR, exist_ok=True)
    path = os.path.join(GOLDEN_DIR, "frame_metrics.npz")
    np.savez_compressed(path, **out)
    print(path, "%.1f KB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
