"""The seeded cases of the render tests (tests/test_render.py on the CPU, tests/test_render_gpu.py on the device,
tools/make_render_golden.py for the fixture): operands as numpy arrays in the form ops.render_frames takes them, the statement
(tests/render_ref.py) evaluated on them, and the same call through ops.render_frames on a device.  Shapes are the smallest at which
the kernel (64 x 16 pixel tiles, a 256-row list, 16-byte stores) can still go wrong."""
import numpy as np
import torch

from gw_depth_amd import ops
from gw_depth_amd import render as R
from tests import render_ref as P

RAGGED = ((37, 53), (64, 80), (16, 16))                  # 3 * 53 and 3 * 80 bytes per row: every offset from a 16-byte boundary occurs


def scene(seed, sizes, Fh=None, Fw=None):
    """Frames, a depth plane, a label plane and a region map for frames of `sizes`, top-left in (B, Fh, Fw)."""
    rng = np.random.default_rng(seed)
    Fh, Fw = Fh or max(s[0] for s in sizes), Fw or max(s[1] for s in sizes)
    B = len(sizes)
    frames = []
    mm = np.zeros((B, Fh, Fw), np.uint16)
    labels = np.full((B, Fh, Fw), 255, np.uint8)
    rmap = np.zeros((B, Fh, Fw), np.uint8)
    for b, (h, w) in enumerate(sizes):
        y, x = np.mgrid[0:h, 0:w]
        f = np.stack([(5 * x + 3 * y) % 256, (7 * x + b * 40) % 256, (11 * y) % 256], axis=2) + rng.integers(0, 4, (h, w, 3))
        frames.append(np.clip(f, 0, 255).astype(np.uint8))
        d = (40 * x + 90 * y + 300 * b + rng.integers(0, 50, (h, w))) % 9000
        d[rng.random((h, w)) < 0.03] = 0                                              # holes
        d.flat[:6] = (0, 1, 8500, 65535, 50, 150)                                     # the ends of the range, the first ties
        mm[b, :h, :w] = d
        lab = np.zeros((h, w), np.uint8)
        lab[h // 5:h // 5 + h // 2, w // 6:w // 6 + w // 2] = 1
        lab[h - 3:, :4] = 2
        lab[0, w - 2:] = 255
        labels[b, :h, :w] = lab
        m = np.zeros((h, w), np.uint8)
        m[h // 5:h // 5 + h // 2, w // 6:w // 6 + w // 3] = 1                          # a block
        m[0:3, 0:5] = 2                                                               # in the frame's corner: its border is outline
        m[h - 1, w - 1] = 3                                                           # one pixel: its own outline
        m[h // 2, w - 3] = 32                                                         # the last rank
        rmap[b, :h, :w] = m
    return frames, mm, labels, rmap


def ragged():
    """B = 3 ragged frames, P = 3: every layer, every colour mode, rows of every kind, through `order`, count = 0 on the last frame."""
    sizes = np.asarray(RAGGED, np.int32)
    frames, mm, labels, rmap = scene(11, RAGGED)
    C = 40
    rng = np.random.default_rng(12)
    lines = np.zeros((3, C, 4), np.float64)
    for b, (h, w) in enumerate(RAGGED):
        lines[b] = np.round(rng.uniform([-4, -4, -4, -4], [w + 4, h + 4, w + 4, h + 4], (C, 4)) * 32) / 32
    # frame 1 (64 x 80): through the tile corners (64, 16), (64, 32), (64, 48), along tile edges, and the special rows
    lines[1, :12] = [(60.0, 12.0, 68.0, 20.0), (0.0, 16.0, 80.0, 16.0), (64.0, 0.0, 64.0, 64.0), (63.5, 31.5, 64.5, 32.5), (10.0, 47.9, 75.0, 48.1),
                     (-50.0, -50.0, -10.0, -20.0), (500.0, 10.0, 900.0, 30.0), (20.5, 20.5, 20.5, 20.5), (np.nan, 1.0, 5.0, 5.0),
                     (1.0, np.inf, 5.0, 5.0), (40000.0, 1.0, 5.0, 5.0), (3.0, 3.0, 3.0, -32768.0)]
    lines[1, 12] = (-30000.0, 30.0, 30000.0, 34.0)                                    # the longest a row may be: |cr| beyond 2^31 far from it
    lines[0, 0] = (5.0, 10.5, 40.0, 10.5)                                             # the horizontal tie: three rows of pixels
    order = np.stack([rng.permutation(C) for _ in range(3)]).astype(np.int32)
    order[1, 5] = -1                                                                  # a row whose source lies outside the list
    order[1, 6] = C
    scores = rng.uniform(0.9, 1.03, (3, C)).astype(np.float32)
    scores[1, 3], scores[0, 2], scores[0, 4] = np.nan, 0.5, 0.91
    kinds = rng.integers(0, 5, (3, C)).astype(np.int32)
    kinds[0, 1], kinds[0, 2] = 7, -1
    count = np.asarray([C - 5, C + 3, 0], np.int32)
    panels = [{"base": "frame", "tint": 0, "outlines": True, "lines": "score"},
              {"base": ("depth", 0), "lines": "kind", "ends": False, "void": (9, 9, 9)},
              {"base": ("labels", 0), "lines": (250, 10, 20), "tint": 0, "tint_alpha": 256, "tint_color": (1, 2, 3)}]
    return dict(sizes=sizes, panels=panels, frames=frames, planes=[mm], label_planes=[labels], region_map=rmap, lines=lines, count=count,
                order=order, scores=scores, kinds=kinds, options={"min_score": 0.905})


def overflow():
    """600 rows through one 48 x 48 frame: every tile gets more rows than the list holds; black base, two colour modes."""
    rng = np.random.default_rng(21)
    C = 600
    lines = (np.round(rng.uniform(0, 48, (1, C, 4)) * 16) / 16).astype(np.float32)
    scores = rng.uniform(0.92, 1.02, (1, C))                                          # float64 scores
    _, mm, labels, _ = scene(22, ((48, 48),))
    return dict(sizes=np.asarray([(48, 48)], np.int32), panels=[{"base": "black", "lines": "score", "ends": False}, {"base": ("labels", 0), "lines": (255, 255, 255)}],
                frames=None, planes=[], label_planes=[labels], region_map=None, lines=lines, count=np.asarray([C], np.int32), order=None,
                scores=scores, kinds=None, options={"width": 1.0, "end_radius": 1})


def many():
    """C = 2048 short rows on a 33 x 150 frame (three tiles wide, three high), nine chunks of 256."""
    rng = np.random.default_rng(31)
    C = 2048
    a = rng.uniform([0, 0], [150, 33], (1, C, 2))
    lines = np.round(np.concatenate([a, a + rng.uniform(-9, 9, (1, C, 2))], axis=2) * 8) / 8
    frames, mm, _, _ = scene(32, ((33, 150),))
    kinds = rng.integers(0, 5, (1, C)).astype(np.int32)
    return dict(sizes=np.asarray([(33, 150)], np.int32), panels=[{"base": ("depth", 0), "lines": "kind", "range": (100, 6000)}, "frame"],
                frames=frames, planes=[mm], label_planes=[], region_map=None, lines=lines, count=np.asarray([C], np.int32),
                order=np.ascontiguousarray(np.arange(C, dtype=np.int32)[::-1][None]), scores=None, kinds=kinds, options={"width": 0.75, "end_radius": 0})


def wide():
    """Width 16 with end_radius 8 on two frames: a row reaches into tiles its ends are far from."""
    sizes = ((40, 70), (20, 130))
    frames, mm, labels, rmap = scene(41, sizes)
    lines = np.asarray([[(10.0, 10.0, 60.0, 30.0), (35.0, 20.0, 35.0, 20.0), (-20.0, 45.0, 90.0, 38.0)],
                        [(5.0, 5.0, 125.0, 15.0), (64.0, -12.0, 64.0, 40.0), (200.0, 10.0, 140.0, 10.0)]], np.float32)
    return dict(sizes=np.asarray(sizes, np.int32), panels=[{"base": "frame", "lines": (0, 0, 0), "end_color": (255, 0, 0)}, {"base": "black", "ends": True}],
                frames=frames, planes=[], label_planes=[], region_map=None, lines=lines, count=np.asarray([3, 3], np.int32), order=None,
                scores=None, kinds=None, options={"width": 16.0, "end_radius": 8})


CASES = {"ragged": ragged, "overflow": overflow, "many": many, "wide": wide}


def operands(case):
    """-> the positional form of P.render / hip's binding: shape, tables, records, per-frame views, options."""
    B = len(case["sizes"])
    split = lambda v: None if v is None else [v[b] for b in range(B)]
    frames, rmap = split(case["frames"]), split(case["region_map"])
    planes, labels = [split(v) for v in case["planes"]], [split(v) for v in case["label_planes"]]
    opts = R.check_options(**case["options"])
    tables, recs = R.resolve(case["panels"], len(planes), len(labels), frames is not None, rmap is not None, case["lines"] is not None,
                             case["scores"] is not None, case["kinds"] is not None)
    every = (frames or []) + (rmap or []) + [t for v in planes + labels for t in v]
    Fh, Fw = opts["canvas_size"] or (max(t.shape[0] for t in every), max(t.shape[1] for t in every))
    return (B, len(recs), Fh, Fw), tables, recs, frames, planes, labels, rmap, opts


def statement(case):
    shape, tables, recs, frames, planes, labels, rmap, opts = operands(case)
    return P.render(shape, case["sizes"], tables, recs, frames, planes, labels, rmap, case["lines"], case["count"], case["order"],
                    case["scores"], case["kinds"], opts)


def pitched(plane, device, pad=(3, 5)):
    """A (B, h, w) array as B separate views into one larger buffer: another row pitch, another offset per frame, the rest 0xAB-like."""
    t = torch.from_numpy(np.ascontiguousarray(plane))
    B, h, w = t.shape[:3]
    big = torch.full((B, h + pad[0], w + pad[1]) + tuple(t.shape[3:]), 171, dtype=t.dtype).to(device)
    views = []
    for b in range(B):
        oy, ox = (b + 1) % (pad[0] + 1), (2 * b + 1) % (pad[1] + 1)
        big[b, oy:oy + h, ox:ox + w] = t[b].to(device)
        views.append(big[b, oy:oy + h, ox:ox + w])
    return views


def call(case, device="cpu", views=False, **more):
    """ops.render_frames on the case; views=True hands every plane over as pitched per-frame views."""
    dev = torch.device(device)
    T = lambda v: None if v is None else torch.from_numpy(np.ascontiguousarray(v)).to(dev)
    plane = (lambda v: pitched(v, dev)) if views else T
    frames = None if case["frames"] is None else [T(f) for f in case["frames"]]
    if views and frames is not None:
        frames = [pitched(f[None], dev)[0] for f in case["frames"]]
    return ops.render_frames(T(case["sizes"]), case["panels"], frames=frames, planes=[plane(v) for v in case["planes"]],
                             label_planes=[plane(v) for v in case["label_planes"]],
                             region_map=None if case["region_map"] is None else plane(case["region_map"]), lines=T(case["lines"]),
                             count=T(case["count"]), order=T(case["order"]), scores=T(case["scores"]), kinds=T(case["kinds"]),
                             **dict(case["options"], **more))
