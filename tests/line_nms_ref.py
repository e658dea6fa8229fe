"""NumPy restatement of gwd_line_nms (gw_depth_amd/csrc/linenms.hip): which queries are candidates, in which order, the twin's lists,
and the compacted rows - around tests/line_score_ref.nms, the restated postprocess(lines, _, threshold, tol=0, do_clip=False) of the
reference (evaluation/eval_post_online.py:44-91).  Pinned by tests/golden/line_nms.npz, which the reference's own postprocess
produced (tools/make_golden_linenms.py); used for the shapes the fixture lacks.

Per image b (the twin, if any, is image b + twin of the inputs):
  points      the first two points of a query as (y, x), times (h, w) in fp32 (eval_post_online.py:133-134), then float64
  trim        each list is cut at the first i > 0 whose values all equal query 0's (eval_post_online.py:127-131)
  floor       only score > min_score enters; a NaN score never does
  twin        its points are mirrored back: end points swapped, x -> w - x in fp32 (data.hflip_lines)
  order       None: query order, the twin's list behind the image's.  Given (L, Q): place k holds the query taken k-th; two lists are
              merged by score (descending, a NaN above every number), the image's own first on ties, equal scores of a list by place
  rows        the kept lines in candidate order as (x1, y1, x2, y2), their scores, ids (+ Q for the twin's); then 0 / 0 / -1

The scores are an INPUT here (softmax probability of class 0, fp32): a test hands in the ones the device computed, so that the order
and the floor are decided on the same bits.
"""
import numpy as np

from tests.line_score_ref import nms


def score_key(scores):
    """The kernel's sort key: ascending keys = ascending floats, a NaN above everything."""
    s = np.ascontiguousarray(scores, np.float32)
    u = s.view(np.uint32)
    key = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))
    return np.where(np.isnan(s), np.uint32(0xFFFFFFFF), key).astype(np.uint32)


def score_order(scores):
    """gwd_line_postprocess's `order` of one image: score descending, equal scores by lower index."""
    return np.argsort(-score_key(scores).astype(np.int64), kind="stable").astype(np.int32)


def first_repeat(lines):
    eq = (lines[1:] == lines[0]).all(-1)
    return int(np.argmax(eq)) + 1 if eq.any() else len(lines)


def pixels(lines, size):
    """(Q, ld) normalised (x, y, ...) fp32 -> (Q, 2, 2) fp32 points (y, x) in pixels of size = (h, w)."""
    pts = np.asarray(lines, np.float32)[:, :4].reshape(-1, 2, 2)[:, :, ::-1].copy()
    pts[:, :, 0] *= np.float32(size[0])
    pts[:, :, 1] *= np.float32(size[1])
    return pts


def mirrored(pts, w):
    out = pts[:, ::-1].copy()
    out[:, :, 1] = np.float32(w) - out[:, :, 1]
    return out


def candidates(scores, lines, size, order=None, min_score=None):
    """scores (L, Q), lines (L, Q, ld), order None or (L, Q), L = 1 (the image) or 2 (the image and its twin).
    -> slots (n,) int (query index, + Q for the twin's) in candidate order, points (n, 2, 2) fp32."""
    scores, lines = np.asarray(scores, np.float32), np.asarray(lines, np.float32)
    L, Q = scores.shape
    slots, pts, keys = [], [], []
    for l in range(L):
        p = pixels(lines[l], size)
        if l == 1:
            p = mirrored(p, size[1])
        place = np.arange(Q) if order is None else np.asarray(order[l], np.int64)
        place = place[(place >= 0) & (place < Q)]
        ok = place < first_repeat(lines[l])
        if min_score is not None:
            ok &= scores[l][place] > np.float32(min_score)                           # False for a NaN score
        place = place[ok]
        slots.append(place + l * Q)
        pts.append(p[place])
        keys.append(score_key(scores[l][place]))
    slots, pts, keys = np.concatenate(slots), np.concatenate(pts), np.concatenate(keys)
    if L == 2 and order is not None:
        merge = np.argsort(-keys.astype(np.int64), kind="stable")
        slots, pts = slots[merge], pts[merge]
    return slots, pts


def line_nms(scores, lines, sizes, threshold, order=None, min_score=None, twin=0):
    """The four outputs of ops.line_nms as NumPy arrays: scores (B + twin, Q) fp32, lines (B + twin, Q, ld), sizes (B, 2)."""
    scores, lines = np.asarray(scores, np.float32), np.asarray(lines, np.float32)
    Bs, Q = scores.shape
    B, C = Bs - twin, Q * (2 if twin else 1)
    out_lines, out_scores = np.zeros((B, C, 4)), np.zeros((B, C), np.float32)
    out_ids, out_count = np.full((B, C), -1, np.int32), np.zeros(B, np.int32)
    for b in range(B):
        imgs = [b, b + twin] if twin else [b]
        h, w = int(sizes[b][0]), int(sizes[b][1])
        slots, pts = candidates(scores[imgs], lines[imgs], (h, w), None if order is None else np.asarray(order)[imgs], min_score)
        diag = (h ** 2 + w ** 2) ** 0.5
        ids, sel = nms(pts.astype(np.float64), diag * threshold)
        k = len(ids)
        out_count[b] = k
        out_ids[b, :k] = slots[ids]
        out_scores[b, :k] = scores.reshape(-1)[(np.array(imgs) * Q)[slots[ids] // Q] + slots[ids] % Q] if k else 0
        out_lines[b, :k] = sel[:, :, ::-1].reshape(k, 4)
    return out_lines, out_scores, out_ids, out_count


def random_case(B, Q, seed, size=(480, 640), ld=6, twin=False):
    """tests/line_score_ref.random_case's lines; with twin, B more images that hold the mirrored lines, jittered, with other logits."""
    from tests.line_score_ref import random_case as draw
    logits, lines, sizes, _, _ = draw(B, Q, 0, seed, size)
    if twin:
        r = np.random.RandomState(seed + 1)
        mir = lines.copy()
        mir[..., 0], mir[..., 2], mir[..., 4] = 1 - lines[..., 2], 1 - lines[..., 0], 1 - lines[..., 4]
        mir[..., 1], mir[..., 3] = lines[..., 3], lines[..., 1]
        mir[..., :4] += r.choice([0.001, 0.004, 0.02], (B, Q, 1)) * r.normal(0, 1, (B, Q, 4))
        lines = np.concatenate([lines, np.clip(mir, 0, 1).astype(np.float32)])
        logits = np.concatenate([logits, r.normal(0, 2, (B, Q, 2)).astype(np.float32)])
    return logits, np.ascontiguousarray(lines[:, :, :ld]), sizes
