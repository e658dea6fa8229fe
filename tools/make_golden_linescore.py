"""Generate tests/golden/line_score.npz with the REAL reference's line NMS and msTPFP on the CPU.

TEST INFRASTRUCTURE ONLY.  Usage: python tools/make_golden_linescore.py   (needs the reference tree; see oracle/ref_stubs.py).

What runs is the reference's own `postprocess` (evaluation/eval_post_online.py:44-91) and `lcnn.metric.msTPFP` / `ap`
(evaluation/lcnn/metric.py), loaded unmodified by file path; docopt, turtle and lcnn.utils (imported, unused on this path) get empty
stand-ins.  This file draws the inputs, does the glue between those functions the way vis_pred_lines (:118-176) and
eval-sAP-glassrgbd.py:55-73 / eval-fscore-glassrgbd.py:35-43 do (those two wrap plotting and file I/O around it and cannot be called),
and stores arrays.  The reference's functions are handed FLOAT64 arrays: that is the pinned precision (csrc/linescore.h).

Images (Q = 100 queries, 6-wide lines):
  0, 1   480 x 640: jittered copies of 8-20 ground-truth lines, near-duplicates, sub-segments, clutter
  2      480 x 640 with a repeat of line 0 at query 70 (the trim)
  3      427 x 569 (odd size)
  4      480 x 640 without ground truth (every kept line is a false positive; msTPFP itself raises on an empty axis)
  5      128 x 128 'exact': small-integer coordinates, axis-parallel lines of power-of-two length, literal duplicates, collinear
         overlaps, a zero-length line; every comparison is exact in any precision.  The queries behind it repeat line 0.
One pair of clutter lines of image 0 shares its logits (equal scores); both are false positives everywhere, so the AP does not depend
on how a sort orders them.

Stability CONDITION on the random images: the discrete results (kept ids, every TP / FP flag) must be unchanged under 8 redraws that
multiply every float64 coordinate by an independent factor in 1 +- 2^-40; a case that fails is drawn again with the next seed.
No random line is shorter than one pixel.
"""
import importlib.util
import os
import sys
import types

import matplotlib                                            # before the reference's modules (they import pyplot at load)
matplotlib.use("Agg")
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")
NMS_T, SAP_T, Q = (0.010, 0.015), (5, 10, 15), 100


def load_reference():
    from oracle.ref_stubs import REF_ROOT
    if not hasattr(np, "float"):
        np.float = float                                     # metric.py:202 (np.bool exists in NumPy 2: left alone)
    for name, attrs in (("docopt", {"docopt": lambda *a, **k: {}}), ("turtle", {"color": None}), ("lcnn", {}),
                        ("lcnn.utils", {"argsort2d": None})):
        if name not in sys.modules:
            m = types.ModuleType(name)
            m.__dict__.update(attrs)
            sys.modules[name] = m
    mods = []
    for name, rel in (("ref_eval_post_online", "evaluation/eval_post_online.py"), ("ref_lcnn_metric", "evaluation/lcnn/metric.py")):
        spec = importlib.util.spec_from_file_location(name, os.path.join(REF_ROOT, rel))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        mods.append(mod)
    return mods


def draw_image(seed, h, w, n_gt, repeat_at=None):
    """Normalised (x1, y1, x2, y2, cx, cy) float32 predictions and ground truth."""
    r = np.random.RandomState(seed)

    def segment():
        while True:
            a, b = r.uniform(0.05, 0.95, 2), r.uniform(0.05, 0.95, 2)
            if np.hypot(*(a - b)) > 0.15:
                return a, b

    gt = [segment() for _ in range(n_gt)]
    lines = []
    for a, b in gt:
        for _ in range(r.randint(2, 5)):                                             # jittered copies: TP candidates and duplicates
            s = r.choice([0.002, 0.004, 0.012, 0.03])
            p, q = a + r.normal(0, s, 2), b + r.normal(0, s, 2)
            lines.append((q, p) if r.rand() < 0.5 else (p, q))
        if r.rand() < 0.7:                                                             # a sub-segment or an overhang: clipping
            u, v = sorted(r.uniform(-0.3, 1.3, 2))
            if v - u > 0.2:
                lines.append((a + (b - a) * u + r.normal(0, 0.001, 2), a + (b - a) * v + r.normal(0, 0.001, 2)))
    if not gt:
        for _ in range(12):
            a, b = segment()
            lines += [(a, b), (a + r.normal(0, 0.003, 2), b + r.normal(0, 0.003, 2))]
    lines = lines[:Q - 10]
    while len(lines) < Q:                                                              # clutter
        lines.append(segment())
    order = r.permutation(Q)
    lines = [lines[i] for i in order]
    arr = np.array([[p[0], p[1], q[0], q[1], (p[0] + q[0]) / 2, (p[1] + q[1]) / 2] for p, q in lines], np.float32)
    arr = np.clip(arr, 0.0, 1.0)
    if repeat_at is not None:
        arr[repeat_at] = arr[0]
    length = np.hypot((arr[:, 2] - arr[:, 0]) * w, (arr[:, 3] - arr[:, 1]) * h)
    assert length.min() >= 1.0, "a random line shorter than one pixel"
    gt_arr = np.array([[a[0], a[1], b[0], b[1]] for a, b in gt], np.float32).reshape(-1, 4)
    logits = (r.normal(0, 2.0, (Q, 2))).astype(np.float32)
    clutter = np.nonzero(order >= Q - 10)[0]                                           # two clutter lines share their logits
    logits[clutter[1]] = logits[clutter[0]]
    return arr, gt_arr, logits, (int(clutter[0]), int(clutter[1]))


def exact_image():
    """128 x 128, pixel coordinates k / 128 with small integers k: (x1, y1, x2, y2) in pixels below."""
    px = [(0, 20, 64, 20),          # line 0 is a line of its own, so the duplicates below are left to the NMS, not to the trim
          (8, 10, 72, 10),          # A: horizontal, length 64
          (8, 10, 72, 10),          # literal duplicate of A: covered
          (40, 10, 104, 10),        # collinear overlap with A: start moves to 0.5
          (24, 10, 40, 10),         # inside A: covered
          (20, 30, 20, 94),         # B: vertical, length 64
          (20, 94, 20, 30),         # B reversed: covered
          (20, 62, 20, 126),        # overlaps B's second half: clipped to (20, 94)-(20, 126)
          (60, 60, 60, 60),         # zero-length line, far from everything: kept
          (60, 60, 60, 60),         # its literal duplicate
          (100, 40, 100, 72),       # C: vertical, length 32
          (101, 40, 101, 72),       # one pixel beside C: within 0.010 * diag = 1.81 px, covered
          (104, 40, 104, 72),       # four pixels beside C: kept
          (8, 100, 72, 100),        # D: one of the ground-truth lines exactly
          (8, 102, 72, 102)]        # two pixels beside D: kept at 0.010 (2 > 1.81), covered at 0.015 (2 < 2.72)
    n = len(px)
    arr = np.zeros((Q, 6), np.float32)
    arr[:n, :4] = np.array(px, np.float32) / 128.0
    arr[:n, 4:] = (arr[:n, :2] + arr[:n, 2:4]) / 2
    arr[n:] = arr[0]                # the queries behind the last real one repeat line 0: the first trim cuts at n
    gt = np.array([(8, 100, 72, 100), (8, 10, 72, 10), (20, 30, 20, 126), (100, 41, 100, 72), (0, 22, 64, 21)], np.float32) / 128.0
    logits = np.random.RandomState(99).normal(0, 2.0, (Q, 2)).astype(np.float32)
    return arr, gt, logits


def to_pixels(lines, h, w):
    """engine_glassrgbd.py:288 and eval_post_online.py:127-136: (y, x) points, the trim, the fp32 scaling; then float64."""
    pts = lines.reshape(-1, 3, 2)[:, :, ::-1].copy()
    n = len(pts)
    for i in range(1, len(pts)):
        if (pts[i] == pts[0]).all():
            n = i
            break
    pts = pts[:n]
    pts[:, :, 0] *= h
    pts[:, :, 1] *= w
    assert pts.dtype == np.float32
    return pts[:, :2].astype(np.float64), n


def chain(post, metric, px, gt128, h, w):
    """The reference's functions on float64 arrays.  Returns per NMS threshold (kept ids, kept lines in 128-space, {s: tp})."""
    diag = (h ** 2 + w ** 2) ** 0.5
    out = []
    for t in NMS_T:
        nlines, _, ids = post.postprocess(px, np.zeros(len(px)), diag * t, 0, False)
        nlines = nlines.reshape(-1, 2, 2).copy()
        nlines[:, :, 0] *= 128 / h
        nlines[:, :, 1] *= 128 / w
        scored = nlines
        for i in range(len(scored)):                                                   # eval-sAP-glassrgbd.py:55-59
            if i > 0 and (scored[i] == scored[0]).all():
                scored = scored[:i]
                break
        tps = {}
        for s in SAP_T:
            if len(gt128) and len(scored):
                tp, fp = metric.msTPFP(scored, gt128, s)
                assert ((tp + fp) == 1).all()
            else:
                tp = np.zeros(len(scored))
            tps[s] = tp
        out.append((np.asarray(ids, np.int64), nlines, len(scored), tps))
    return out


def discrete(res):
    return [(tuple(ids), n, tuple(tuple(tp) for tp in tps.values())) for ids, _, n, tps in res]


def stable(post, metric, px, gt128, h, w, seed):
    base = discrete(chain(post, metric, px, gt128, h, w))
    r = np.random.RandomState(seed)
    for _ in range(8):
        f = lambda a: a * (1.0 + r.choice([-1.0, 1.0], a.shape) * 2.0 ** -40)
        if discrete(chain(post, metric, f(px), f(gt128), h, w)) != base:
            return False
    return True


def main():
    post, metric = load_reference()
    plan = [(480, 640, 14, None), (480, 640, 20, None), (480, 640, 8, 70), (427, 569, 11, None), (480, 640, 0, None)]
    images, seed = [], 1000
    for h, w, n_gt, repeat_at in plan:
        while True:
            seed += 1
            lines, gt, logits, tie = draw_image(seed, h, w, n_gt, repeat_at)
            px, n = to_pixels(lines, h, w)
            gt128 = gt.reshape(-1, 2, 2)[:, :, ::-1].astype(np.float64) * 128.0
            if stable(post, metric, px, gt128, h, w, seed):
                break
            print("seed %d: unstable under the 2^-40 redraws, drawn again" % seed)
        images.append((h, w, lines, gt, logits, px, n, gt128, tie))
    lines, gt, logits = exact_image()
    px, n = to_pixels(lines, 128, 128)
    images.append((128, 128, lines, gt, logits, px, n, gt.reshape(-1, 2, 2)[:, :, ::-1].astype(np.float64) * 128.0, None))

    B, T, S = len(images), len(NMS_T), len(SAP_T)
    G = max(len(im[3]) for im in images)
    out = {"pred_logits": np.stack([im[4] for im in images]), "pred_lines": np.stack([im[2] for im in images]),
           "sizes": np.array([[im[0], im[1]] for im in images], np.int32), "gt_lines": np.zeros((B, G, 4), np.float32),
           "gt_counts": np.array([len(im[3]) for im in images], np.int32), "trim": np.array([im[6] for im in images], np.int32),
           "nms_thresholds": np.array(NMS_T), "sap_thresholds": np.array(SAP_T, np.float64), "tie": np.array(images[0][8], np.int32)}
    out["scores"] = torch.softmax(torch.from_numpy(out["pred_logits"]), -1)[..., 0].numpy()          # engine_glassrgbd.py:287,297
    kept = np.zeros((T, B, Q), bool)
    kept_lines = np.zeros((T, B, Q, 4))
    flag = np.full((T, S, B, Q), 2, np.uint8)
    for b, (h, w, _, gt, _, px, n, gt128, _) in enumerate(images):
        out["gt_lines"][b, :len(gt)] = gt
        for t, (ids, nlines, n_scored, tps) in enumerate(chain(post, metric, px, gt128, h, w)):
            kept[t, b, ids] = True
            kept_lines[t, b, ids] = nlines.reshape(-1, 4)
            for s, st in enumerate(SAP_T):
                flag[t, s, b, ids[:n_scored]] = tps[st].astype(np.uint8)
    out.update(kept=kept, kept_lines=kept_lines, flag=flag)

    # the closing lines of eval-sAP-glassrgbd.py:66-73 (and of the F-score script, which differ in the last call only)
    def f_score(tp, fp):                                                               # eval-fscore-glassrgbd.py:35-43
        rec = np.concatenate(([0.0], tp, [1.0]))
        prec = np.concatenate(([0.0], tp / np.maximum(tp + fp, 1e-9), [0.0]))
        return (2 * prec * rec / (prec + rec + 0.0000000001)).max()

    n_gt = int(out["gt_counts"].sum())
    sap, sf = np.zeros((T, S)), np.zeros((T, S))
    for t in range(T):
        for s in range(S):
            scored = flag[t, s] != 2
            tp_all, fp_all, sc = (flag[t, s] == 1)[scored].astype(np.float64), (flag[t, s] == 0)[scored].astype(np.float64), out["scores"][scored]
            index = np.argsort(-sc)
            tp, fp = np.cumsum(tp_all[index]) / n_gt, np.cumsum(fp_all[index]) / n_gt
            sap[t, s], sf[t, s] = 100 * metric.ap(tp, fp), 100 * f_score(tp, fp)
    out.update(sAP=sap, sF=sf)

    a, b = out["tie"]
    assert out["scores"][0, a] == out["scores"][0, b] and (flag[:, :, 0, a] == flag[:, :, 0, b]).all() and kept[:, 0, a].all()
    for t in range(T):
        print("nms %.3f: kept per image %s, TP/FP/unscored at sAP10 %s, sAP %s sF %s" % (
            NMS_T[t], kept[t].sum(1).tolist(), [int((flag[t, 1] == v).sum()) for v in (1, 0, 2)], sap[t].round(3).tolist(),
            sf[t].round(3).tolist()))
    path = os.path.join(GOLDEN_DIR, "line_score.npz")
    np.savez_compressed(path, **out)
    print(path, "%.1f KB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
