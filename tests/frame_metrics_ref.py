"""NumPy restatement of gwd_eval_frames (include/gwdepth.h, csrc/evalframes.hip).  TEST INFRASTRUCTURE ONLY.

Per-pixel terms are formed in fp32 with the kernel's expressions (IEEE division; logarithms through f64, rounded to fp32); every
raw sum is math.fsum of the fp32 terms, i.e. the correctly rounded sum.  The closing arithmetic is oracle/eval_ref.py's.  Pinned
against the reference's own compute_depth_errors / get_confusion_matrix by tests/golden/frame_metrics.npz
(tools/make_golden_frame_metrics.py).
"""
import math
import warnings

import numpy as np

from oracle import eval_ref

NSUM = 10
METRIC_NAMES = eval_ref.METRIC_NAMES
EPS = 2.0 ** -52


def region_names(n_bins):
    return ["all", "glass", "nonglass"] + ["bin%d" % k for k in range(n_bins)]


def frame_pixels(depth, label, mm, raw, min_d=1e-3, max_d=10.0):
    """The kernel's view of one frame: (g fp32, clamped prediction fp32, valid, glass) over its pixels, flat."""
    f32 = np.float32
    dmin, dmax = f32(min_d), f32(max_d)
    g = (np.asarray(mm).astype(np.int64).astype(f32) / f32(1000.0)).reshape(-1)       # glassrgbd_norhint.py:273
    p = np.array(depth, dtype=f32, copy=True).reshape(-1)
    with np.errstate(invalid="ignore"):
        p[p < dmin] = dmin                                                           # engine_glassrgbd.py:249-252, in that order
        p[p > dmax] = dmax
        p[np.isnan(p)] = dmin
        valid = (g > dmin) & (g < dmax)                                              # :253
    glass = np.asarray(raw).reshape(-1) > 0                                          # :275
    return g, p, valid, glass


def pixel_terms(g, p):
    """(n, 10) fp32: 1, three threshold hits, sq, abs_rel, sq_rel, err, err^2, |log10 diff| of valid pixels."""
    f32 = np.float32
    g, p = g.astype(f32), p.astype(f32)
    with np.errstate(all="ignore"):
        thr = np.maximum(g / p, p / g)
        diff = g - p
        sq = diff * diff
        err = np.log(p.astype(np.float64)).astype(f32) - np.log(g.astype(np.float64)).astype(f32)
        l10 = np.abs(np.log10(p.astype(np.float64)).astype(f32) - np.log10(g.astype(np.float64)).astype(f32))
        t = np.stack([np.ones_like(g), (thr < f32(1.25)).astype(f32), (thr < f32(1.5625)).astype(f32),
                      (thr < f32(1.953125)).astype(f32), sq, np.abs(diff) / g, sq / g, err, err * err, l10], axis=1)
    assert t.dtype == f32
    return t


def region_masks(g, valid, glass, edges):
    """[R] boolean masks over the flat pixels: all, glass, non-glass, the bins [e_k, e_k+1)."""
    out = [valid, valid & glass, valid & ~glass]
    e = np.asarray(edges, dtype=np.float32)
    for k in range(max(len(e) - 1, 0)):
        out.append(valid & (g >= e[k]) & (g < e[k + 1]))
    return out


def score_frame(depth, label, mm, raw, min_d=1e-3, max_d=10.0, edges=()):
    """-> dict: sums (R,10) f64 (fsum), abs_sums (R,10) f64 (fsum of |term|: the error bound's scale), conf (4,) int64,
    measures (R,9) f64."""
    g, p, valid, glass = frame_pixels(depth, label, mm, raw, min_d, max_d)
    masks = region_masks(g, valid, glass, edges)
    R = len(masks)
    sums, abs_sums = np.zeros((R, NSUM)), np.zeros((R, NSUM))
    terms = np.zeros((g.size, NSUM), dtype=np.float32)
    terms[valid] = pixel_terms(g[valid], p[valid])
    for r, m in enumerate(masks):
        t = terms[m].astype(np.float64)
        for k in range(NSUM):
            sums[r, k] = math.fsum(t[:, k])
            abs_sums[r, k] = math.fsum(np.abs(t[:, k]))
    lab = np.asarray(label).reshape(-1).astype(np.int64)
    keep = lab < 2
    conf = np.bincount(glass[keep].astype(np.int64) * 2 + lab[keep], minlength=4).astype(np.int64)
    return {"sums": sums, "abs_sums": abs_sums, "conf": conf, "measures": measures_from_sums(sums)}


def measures_from_sums(sums):
    """(..., 10) raw sums -> (..., 9) measures in METRIC_NAMES order, NaN where the count is zero (the kernel's closing step)."""
    s = np.asarray(sums, dtype=np.float64)
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        n = s[..., 0]
        me, me2 = s[..., 7] / n, s[..., 8] / n
        return np.stack([np.sqrt(me2 - me * me) * 100.0, s[..., 5] / n, s[..., 9] / n, np.sqrt(s[..., 4] / n), s[..., 6] / n,
                         np.sqrt(me2), s[..., 1] / n, s[..., 2] / n, s[..., 3] / n], axis=-1)


def running_fold(sums, measures, conf):
    """The kernel's running totals over images in the given order: (R,10) f64 (nine measure sums + the count of images whose region
    is not empty) and the (4,) confusion."""
    sums, measures = np.asarray(sums), np.asarray(measures)
    R = sums.shape[1]
    run = np.zeros((R, NSUM))
    for b in range(sums.shape[0]):
        for r in range(R):
            if sums[b, r, 0] != 0:
                run[r, :9] += measures[b, r]
                run[r, 9] += 1
    return run, np.asarray(conf, dtype=np.int64).reshape(-1, 4).sum(0)


def closing(run, confusion, sums):
    """FrameMetrics.compute()'s dictionary from the running totals, the confusion counts and the per-image raw sums."""
    names = region_names(run.shape[0] - 3)
    out = {}
    conf = np.asarray(confusion, dtype=np.float64).reshape(2, 2)
    if conf.sum() > 0:
        out.update(eval_ref.seg_scores(conf))
    total = np.zeros(run.shape)
    for s in np.asarray(sums):
        total += s
    pix = measures_from_sums(total)
    for r, name in enumerate(names):
        pre = "" if r == 0 else name + "/"
        for k, m in enumerate(METRIC_NAMES):
            if run[r, 9] > 0:
                out[pre + m] = float(run[r, k] / run[r, 9])
            if total[r, 0] > 0:
                out["pixel/" + pre + m] = float(pix[r, k])
    out["n_images"] = {name: int(run[r, 9]) for r, name in enumerate(names)}
    return out


def sum_bound(n_pixels, abs_sum):
    """Worst case of an f64 fold, in any order, of n exactly representable terms: |error| <= n * 2^-52 * sum |term|."""
    return n_pixels * EPS * abs_sum
