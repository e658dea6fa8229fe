"""NumPy restatement of the reference's line-scoring chain, for use where the reference tree is absent (GPU tests at other sizes, the
host baseline of tools/linescore_bench.py).  Pinned by tests/golden/line_score.npz, which the reference's own functions produced
(tools/make_golden_linescore.py); tests/test_line_score.py holds the two together.

The chain, per image (reference files under evaluation/ unless said otherwise):
  score = softmax(logits)[:, 0]                                  src/engine_glassrgbd.py:287,297
  lines: first two points as (y, x), times (h, w) in fp32          eval_post_online.py:133-136, then float64 (the pinned precision)
  trim at the first i > 0 with lines[i] == lines[0]                eval_post_online.py:127-131
  postprocess(lines, scores, diag * t, 0, False) per t             eval_post_online.py:44-91,142  - in QUERY order
  kept lines times (128 / h, 128 / w)                              eval_post_online.py:174-175
  second trim of the kept lines                                    eval-sAP-glassrgbd.py:55-59
  msTPFP(kept, gt * 128, s) per s                                  lcnn/metric.py:194-210
and over all images: sort by score, cumulative sums over n_gt, ap / f_score (eval-sAP-glassrgbd.py:66-73, lcnn/metric.py:11-21,
eval-fscore-glassrgbd.py:35-43).  Ground truth is the targets' normalised lines times 128 (the reference's scripts read the data
set's own lpos files; that source is not pinned by any reference-held vector).  An image without ground truth scores every kept line
as a false positive (the reference's argmin raises on an empty axis).

Everything after the fp32 scaling is elementwise float64 NumPy: a * b + c is two roundings, as in the reference.
"""
import numpy as np

NMS_THRESHOLDS = (0.010, 0.015)
SAP_THRESHOLDS = (5, 10, 15)


def _pline(x1, y1, x2, y2, x, y):
    px, py = x2 - x1, y2 - y1
    dd = px * px + py * py
    u = ((x - x1) * px + (y - y1) * py) / np.where(dd > 1e-9, dd, 1e-9)           # max(1e-9, float(dd))
    dx, dy = x1 + u * px - x, y1 + u * py - y
    return dx * dx + dy * dy


def _plambda(x1, y1, x2, y2, x, y):
    px, py = x2 - x1, y2 - y1
    dd = px * px + py * py
    return ((x - x1) * px + (y - y1) * py) / np.where(dd > 1e-9, dd, 1e-9)


def nms(lines, threshold):
    """postprocess(lines, _, threshold, tol=0, do_clip=False): lines (n, 2, 2) float64 -> (kept ids, clipped lines (k, 2, 2)).
    The pair geometry of line i against all selected lines is one vector expression; the interval walk is the reference's."""
    lines = np.asarray(lines, np.float64)
    ids, sel = [], np.zeros((0, 2, 2))
    thr2 = threshold * threshold
    for i, (p, q) in enumerate(lines):
        start, end = 0.0, 1.0
        if len(ids):
            a, b = sel[:, 0], sel[:, 1]
            one = np.ones(len(ids))
            P0, P1, Q0, Q1 = p[0] * one, p[1] * one, q[0] * one, q[1] * one
            d_pa, d_pb = _pline(P0, P1, Q0, Q1, a[:, 0], a[:, 1]), _pline(P0, P1, Q0, Q1, b[:, 0], b[:, 1])
            d_ap, d_aq = _pline(a[:, 0], a[:, 1], b[:, 0], b[:, 1], P0, P1), _pline(a[:, 0], a[:, 1], b[:, 0], b[:, 1], Q0, Q1)
            m1 = np.where(d_pb > d_pa, d_pb, d_pa)                                  # Python's max / min on two numbers
            m2 = np.where(d_aq > d_ap, d_aq, d_ap)
            d = np.where(m2 < m1, m2, m1)
            la, lb = _plambda(P0, P1, Q0, Q1, a[:, 0], a[:, 1]), _plambda(P0, P1, Q0, Q1, b[:, 0], b[:, 1])
            la, lb = np.where(la > lb, lb, la), np.where(la > lb, la, lb)
            for j in np.nonzero(~(d > thr2))[0]:
                lo, hi = float(la[j]), float(lb[j])
                if start < lo and hi < end:
                    continue
                if hi < start or lo > end:
                    continue
                if lo <= start and end <= hi:
                    start = 10.0
                    break
                if lo <= start and start <= hi:
                    start = hi
                if lo <= end and end <= hi:
                    end = lo
                if start >= end:
                    break
        if start >= end:
            continue
        ids.append(i)
        sel = np.concatenate([sel, np.array([p + (q - p) * start, p + (q - p) * end])[None]])
    return np.array(ids, np.int64), sel


def first_repeat(lines):
    """The cut of both duplicate trims: the first i > 0 whose line equals line 0, else len(lines)."""
    for i in range(1, len(lines)):
        if (lines[i] == lines[0]).all():
            return i
    return len(lines)


def match(kept, gt128):
    """msTPFP's distance and choice: kept (k, 2, 2), gt128 (G, 2, 2), G > 0."""
    diff = ((kept[:, None, :, None] - gt128[:, None]) ** 2).sum(-1)
    diff = np.minimum(diff[:, :, 0, 0] + diff[:, :, 1, 1], diff[:, :, 0, 1] + diff[:, :, 1, 0])
    return np.min(diff, 1), np.argmin(diff, 1)


def image_chain(lines, size, gt, nms_thresholds=NMS_THRESHOLDS, sap_thresholds=SAP_THRESHOLDS):
    """lines (Q, 4 | 6) float32 normalised (x, y, ...), size (h, w), gt (G, >= 4) float32 normalised.
    Returns kept (T, Q) bool, kept_lines (T, Q, 4) float64 as (y1, x1, y2, x2) in 128-space (zeros where not kept) and
    flag (T, S, Q) uint8: 0 false positive, 1 true positive, 2 not scored."""
    lines = np.asarray(lines, np.float32)
    Q = lines.shape[0]
    h, w = int(size[0]), int(size[1])
    n = first_repeat(lines)
    pts = lines[:, :4].reshape(Q, 2, 2)[:, :, ::-1].copy()                         # (y, x)
    pts[:, :, 0] *= np.float32(h)
    pts[:, :, 1] *= np.float32(w)
    px = pts[:n].astype(np.float64)
    gt = np.asarray(gt, np.float32)
    gt = gt[:, :4] if gt.size else np.zeros((0, 4), np.float32)
    gt128 = gt.reshape(-1, 2, 2)[:, :, ::-1].astype(np.float64) * 128.0
    diag = (h ** 2 + w ** 2) ** 0.5
    T, S = len(nms_thresholds), len(sap_thresholds)
    kept = np.zeros((T, Q), bool)
    kept_lines = np.zeros((T, Q, 4))
    flag = np.full((T, S, Q), 2, np.uint8)
    for t, thr in enumerate(nms_thresholds):
        ids, sel = nms(px, diag * thr)
        sel = sel.copy()
        sel[:, :, 0] *= 128 / h
        sel[:, :, 1] *= 128 / w
        kept[t, ids] = True
        kept_lines[t, ids] = sel.reshape(-1, 4)
        m = first_repeat(sel)
        ids, sel = ids[:m], sel[:m]
        if len(gt128) and len(ids):
            dist, choice = match(sel, gt128)
        else:
            dist, choice = np.full(len(ids), np.inf), np.zeros(len(ids), np.int64)
        for s, st in enumerate(sap_thresholds):
            hit = np.zeros(max(len(gt128), 1), bool)
            for k, i in enumerate(ids):
                if dist[k] < st and not hit[choice[k]]:
                    hit[choice[k]] = True
                    flag[t, s, i] = 1
                else:
                    flag[t, s, i] = 0
    return kept, kept_lines, flag


def _curves(tp, fp):
    """Recall and precision along the ranking, padded with the (0, 0) start and the (1, 0) end both scripts add."""
    rec = np.concatenate(([0.0], tp, [1.0]))
    prec = np.concatenate(([0.0], tp / np.maximum(tp + fp, 1e-9), [0.0]))
    return rec, prec


def ap(tp, fp):
    """lcnn/metric.py:11-21: the area under the precision envelope (every precision raised to the best one at any later rank),
    summed over the ranks where the recall moves."""
    rec, prec = _curves(tp, fp)
    env = np.maximum.accumulate(prec[::-1])[::-1]
    step = np.nonzero(rec[1:] != rec[:-1])[0]
    return np.sum((rec[step + 1] - rec[step]) * env[step + 1])


def f_score(tp, fp):
    """eval-fscore-glassrgbd.py:35-43: the best harmonic mean of precision and recall along the ranking."""
    rec, prec = _curves(tp, fp)
    return np.max(2 * prec * rec / (prec + rec + 1e-10))


def close(sorted_flags, n_gt):
    """eval-sAP-glassrgbd.py:70-73 on one (NMS threshold, sAP threshold) column: flags in descending score order, the unscored
    entries (2) dropped.  Returns (AP, F), both times 100 as the scripts print them."""
    f = np.asarray(sorted_flags)
    f = f[f != 2]
    tp = np.cumsum((f == 1).astype(np.float64)) / n_gt
    fp = np.cumsum((f == 0).astype(np.float64)) / n_gt
    return 100 * float(ap(tp, fp)), 100 * float(f_score(tp, fp))


def key(kind, s, t):
    """'sAP10_nms0_010' for kind 'sAP', s = 10, t = 0.010."""
    return "%s%g_nms%s" % (kind, s, ("%.3f" % t).replace(".", "_"))


def score_all(scores, lines, sizes, gts, nms_thresholds=NMS_THRESHOLDS, sap_thresholds=SAP_THRESHOLDS):
    """The whole chain over a list of images: scores (N, Q), lines (N, Q, ld), sizes (N, 2), gts a list of (G_i, >= 4).
    Equal scores keep image order, then line order (a stable sort; the reference's argsort leaves it open)."""
    out = [image_chain(l, s, g, nms_thresholds, sap_thresholds) for l, s, g in zip(lines, sizes, gts)]
    flag = np.stack([o[2] for o in out], 2)                                        # (T, S, N, Q)
    order = np.argsort(-np.asarray(scores, np.float32).reshape(-1), kind="stable")
    n_gt = sum(len(g) for g in gts)
    stats = {}
    for t, thr in enumerate(nms_thresholds):
        for s, st in enumerate(sap_thresholds):
            a, f = close(flag[t, s].reshape(-1)[order], n_gt)
            stats[key("sAP", st, thr)], stats[key("sF", st, thr)] = a, f
    return stats


def random_case(B, Q, G, seed, size=(480, 640)):
    """Jittered copies of G ground-truth lines (16 hidden ones when G = 0), sub-segments and clutter; no line under a pixel."""
    r = np.random.RandomState(seed)

    def segments(n):
        a, b = r.uniform(0.05, 0.95, (n, 2)), r.uniform(0.05, 0.95, (n, 2))
        short = np.hypot(*(a - b).T) < 0.1
        b[short] = np.clip(a[short] + 0.2, 0, 1)
        return a, b

    lines, gts = np.zeros((B, Q, 6), np.float32), np.zeros((B, G, 4), np.float32)
    for i in range(B):
        ga, gb = segments(max(G, 16))
        pick = r.randint(0, len(ga), Q)
        kind = r.rand(Q)
        u, v = np.where(kind < 0.2, r.uniform(-0.2, 0.4, Q), 0.0)[:, None], np.where(kind < 0.2, r.uniform(0.6, 1.2, Q), 1.0)[:, None]
        a, b = ga[pick] + (gb[pick] - ga[pick]) * u, ga[pick] + (gb[pick] - ga[pick]) * v
        s = r.choice([0.002, 0.004, 0.012, 0.03], Q)[:, None]
        a, b = a + r.normal(0, 1, (Q, 2)) * s, b + r.normal(0, 1, (Q, 2)) * s
        ca, cb = segments(Q)
        clutter = kind > 0.8
        a[clutter], b[clutter] = ca[clutter], cb[clutter]
        lines[i, :, :2], lines[i, :, 2:4], lines[i, :, 4:] = a, b, (a + b) / 2
        if G:
            gts[i, :, :2], gts[i, :, 2:] = ga[:G], gb[:G]
    lines = np.clip(lines, 0, 1)
    logits = r.normal(0, 2, (B, Q, 2)).astype(np.float32)
    sizes = np.tile(np.array(size, np.int32), (B, 1))
    counts = np.full(B, G, np.int32)
    if B > 1 and G > 1:
        counts[1] = G // 2                                                            # padded ground truth: rows behind the count are ignored
    return logits, lines, sizes, gts, counts
