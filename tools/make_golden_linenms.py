"""Generate tests/golden/line_nms.npz with the REAL reference's line NMS on the CPU.

TEST INFRASTRUCTURE ONLY.  Usage: python tools/make_golden_linenms.py   (needs the reference tree; see oracle/ref_stubs.py).

What runs is the reference's own `postprocess` (evaluation/eval_post_online.py:44-91), loaded unmodified by file path through
tools/make_golden_linescore.load_reference, on FLOAT64 arrays (the pinned precision, csrc/linescore.h).  This file draws the inputs
(make_golden_linescore's draw_image / exact_image), lists the candidates of gwd_line_nms in plain loops - the fp32 scaling and the
duplicate trim as vis_pred_lines does them (:127-136), the score floor, the order, the twin's lines mirrored back by hflip's own
expression (src/datasets/transforms_depth.py, hflip) - and stores arrays.

Cases (Q = 100; every case holds inputs, options and the expected rows):
  query_0010 / query_0015 / score_0010 / score_0015   three images (480 x 640 twice, 427 x 569), query order and score order
  frame_0010     an image scaled to 720 x 1280, a size its input never had (what target_sizes / predict_frames ask for)
  floor_0010     score order with a floor of 0.5
  repeat_0015    a repeat of line 0 at query 70 (the trim), query order
  twin_query_0010 / twin_score_0015   two images and their mirrored twins (ld = 4): lists appended / merged by score
  exact_query_0010 / exact_score_0015  128 x 128 on small integers: literal duplicates, collinear overlaps, a zero-length line
One pair of clutter lines per random image shares its logits (equal scores: the lower index goes first in score order).

Stability CONDITION on the random images: kept ids and count must be unchanged under 8 redraws that multiply every float64
coordinate by an independent factor in 1 +- 2^-40; an image that fails in ANY case it takes part in (its mirrored twin is drawn
from it) is drawn again with the next seed.  This is a condition on the inputs, checked with the reference alone.

Also prints the host time of the reference's postprocess per image (Q = 100), the figure the device kernel is set against.
"""
import importlib.util
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")
Q = 100


def linescore_tool():
    spec = importlib.util.spec_from_file_location("make_golden_linescore", os.path.join(ROOT, "tools", "make_golden_linescore.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def scores_of(logits):
    return torch.softmax(torch.from_numpy(logits), -1)[..., 0].numpy()                  # engine_glassrgbd.py:287,297


def one_list(lines, scores, h, w, order, floor, mirror):
    """[(score, query, points (2, 2) fp32 as (y, x))] of one image's queries, in the order they are taken."""
    pts = lines.reshape(len(lines), -1, 2)[:, :, ::-1].copy()
    n = len(pts)
    for i in range(1, len(pts)):                                                         # eval_post_online.py:127-131
        if (pts[i] == pts[0]).all():
            n = i
            break
    pts[:, :, 0] *= np.float32(h)                                                        # :133-134
    pts[:, :, 1] *= np.float32(w)
    assert pts.dtype == np.float32
    pts = pts[:, :2]
    if mirror:                                                                           # hflip's expression on (x1, y1, x2, y2) pixels
        t = torch.from_numpy(pts[:, :, ::-1].reshape(-1, 4).copy())
        t = t[:, [2, 3, 0, 1]] * torch.as_tensor([-1, 1, -1, 1]) + torch.as_tensor([w, 0, w, 0])
        assert t.dtype == torch.float32
        pts = t.numpy().reshape(-1, 2, 2)[:, :, ::-1].copy()
    places = range(len(pts)) if order == "query" else sorted(range(len(pts)), key=lambda q: -float(scores[q]))
    return [(float(scores[q]), q, pts[q]) for q in places if q < n and (floor is None or scores[q] > np.float32(floor))]


def image_candidates(case, b):
    h, w = (int(v) for v in case["sizes"][b])
    s = case["scores"]
    own = one_list(case["lines"][b], s[b], h, w, case["order"], case["floor"], False)
    cand = [(sc, q, p) for sc, q, p in own]
    if case["twin"]:
        tb = b + case["twin"]
        other = [(sc, q + Q, p) for sc, q, p in one_list(case["lines"][tb], s[tb], h, w, case["order"], case["floor"], True)]
        cand = cand + other
        if case["order"] == "score":
            cand = sorted(cand, key=lambda e: -e[0])                                     # stable: the image's own first on ties
    return cand, h, w


def run_image(post, cand, h, w, t, jitter=None):
    px = np.array([p for _, _, p in cand], np.float64).reshape(-1, 2, 2)
    if jitter is not None:
        px = px * (1.0 + jitter.choice([-1.0, 1.0], px.shape) * 2.0 ** -40)
    diag = (h ** 2 + w ** 2) ** 0.5
    nlines, _, ids = post.postprocess(px, np.zeros(len(px)), diag * t, 0, False)
    ids = np.asarray(ids, np.int64)
    slots = np.array([cand[i][1] for i in ids], np.int64)
    return slots, np.asarray(nlines, np.float64).reshape(-1, 2, 2)[:, :, ::-1].reshape(-1, 4)


def stable(post, case, b, seed):
    cand, h, w = image_candidates(case, b)
    base = run_image(post, cand, h, w, case["t"])[0]
    r = np.random.RandomState(seed)
    for _ in range(8):
        got = run_image(post, cand, h, w, case["t"], r)[0]
        if len(got) != len(base) or (got != base).any():
            return False
    return True


def build_cases(images):
    """images: name -> (lines (Q, 6) fp32, logits (Q, 2) fp32).  Returns name -> case dict (the random ones reference their images)."""
    def case(names, sizes, t, order, floor=None, twin=0, ld=6):
        lines = np.stack([images[n][0][:, :ld] for n in names])
        logits = np.stack([images[n][1] for n in names])
        return {"images": names, "lines": np.ascontiguousarray(lines), "logits": logits, "scores": scores_of(logits),
                "sizes": np.array(sizes, np.int32), "t": t, "order": order, "floor": floor, "twin": twin}

    three, sz3 = ["a", "b", "c"], [(480, 640), (480, 640), (427, 569)]
    return {
        "query_0010": case(three, sz3, 0.010, "query"), "query_0015": case(three, sz3, 0.015, "query"),
        "score_0010": case(three, sz3, 0.010, "score"), "score_0015": case(three, sz3, 0.015, "score"),
        "frame_0010": case(["a"], [(720, 1280)], 0.010, "score"),
        "floor_0010": case(["b"], [(480, 640)], 0.010, "score", floor=0.5),
        "repeat_0015": case(["r"], [(480, 640)], 0.015, "query"),
        "twin_query_0010": case(["a", "c", "am", "cm"], [(480, 640), (427, 569)], 0.010, "query", twin=2, ld=4),
        "twin_score_0015": case(["a", "c", "am", "cm"], [(480, 640), (427, 569)], 0.015, "score", twin=2, ld=4),
        "exact_query_0010": case(["x"], [(128, 128)], 0.010, "query"), "exact_score_0015": case(["x"], [(128, 128)], 0.015, "score"),
    }


def mirror_of(lines, seed):
    """What a detector would say of the mirrored image: the lines mirrored (x -> 1 - x, end points swapped) and jittered - every one: an exact mirror
    image covers its original to the last bit, which no rounding-stable case can hold."""
    r = np.random.RandomState(seed)
    m = lines.copy()
    m[:, 0], m[:, 2], m[:, 4] = 1 - lines[:, 2], 1 - lines[:, 0], 1 - lines[:, 4]
    m[:, 1], m[:, 3] = lines[:, 3], lines[:, 1]
    m[:, :4] += r.choice([0.001, 0.004, 0.02], (len(m), 1)) * r.normal(0, 1, (len(m), 4))
    return np.clip(m, 0, 1).astype(np.float32), r.normal(0, 2.0, (len(m), 2)).astype(np.float32)


def main():
    tool = linescore_tool()
    post = tool.load_reference()[0]
    plan = {"a": (480, 640, 14, None), "b": (480, 640, 20, None), "c": (427, 569, 11, None), "r": (480, 640, 8, 70)}
    seeds = {name: 2001 + 100 * k for k, name in enumerate(plan)}
    x_lines, _, x_logits = tool.exact_image()
    while True:
        images = {"x": (x_lines, x_logits)}
        for name, (h, w, n_gt, repeat_at) in plan.items():
            lines, _, logits, _ = tool.draw_image(seeds[name], h, w, n_gt, repeat_at)
            images[name] = (lines, logits)
            images[name + "m"] = mirror_of(lines, seeds[name] + 50)
        cases = build_cases(images)
        bad = sorted({c["images"][b] for c in cases.values() for b in range(len(c["sizes"]))
                      if c["images"][b] != "x" and not stable(post, c, b, seeds[c["images"][b]])})
        if not bad:
            break
        for name in bad:
            print("image %s seed %d: unstable under the 2^-40 redraws, drawn again" % (name, seeds[name]))
            seeds[name] += 1

    out = {"cases": np.array(sorted(cases))}
    for name, c in cases.items():
        B, C = len(c["sizes"]), Q * (2 if c["twin"] else 1)
        ids, count, nl = np.full((B, C), -1, np.int32), np.zeros(B, np.int32), np.zeros((B, C, 4))
        for b in range(B):
            cand, h, w = image_candidates(c, b)
            slots, kept = run_image(post, cand, h, w, c["t"])
            count[b] = len(slots)
            ids[b, :len(slots)] = slots
            nl[b, :len(slots)] = kept
        pre = name + "/"
        out.update({pre + "logits": c["logits"], pre + "lines": c["lines"], pre + "sizes": c["sizes"], pre + "scores": c["scores"],
                    pre + "t": np.float64(c["t"]), pre + "by_score": np.bool_(c["order"] == "score"),
                    pre + "min_score": np.float32(np.nan if c["floor"] is None else c["floor"]), pre + "twin": np.int32(c["twin"]),
                    pre + "ids": ids, pre + "count": count, pre + "nms_lines": nl})
        print("%-18s kept per image %s of %s candidates" % (name, count.tolist(), [len(image_candidates(c, b)[0]) for b in range(B)]))

    q = cases["query_0010"]
    times = []
    for t in (0.010, 0.015):
        for b in range(3):
            cand, h, w = image_candidates(q, b)
            t0 = time.perf_counter()
            run_image(post, cand, h, w, t)
            times.append((time.perf_counter() - t0) * 1e3)
    print("reference postprocess on this host, Q = 100: median %.1f ms per image and threshold (min %.1f, max %.1f)" % (
        float(np.median(times)), min(times), max(times)))

    path = os.path.join(GOLDEN_DIR, "line_nms.npz")
    np.savez_compressed(path, **out)
    print(path, "%.1f KB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
