"""The statement of gwd_render_frames in numpy: a plain, unoptimised restatement of the rules in
include/gwdepth.h - a loop over frames, panels and rows, whole-frame integer arrays, no tiles, no binning, no list.  The kernel, the
host build of csrc/rendergeom.h and the stand-in library (tests/render_fake.py) are all held to it bit for bit.

It takes what the binding takes (hip.HipLibrary.render_frames): operands per frame, the colour tables of the call, and the panels
as the integer records gw_depth_amd.render.resolve makes.  The colour tables are restated here too (jet_table, voc_palette), so the
product's builders are checked against a second writing of the same rule."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "render.npz")
GOLDEN_LUT = os.path.join(HERE, "golden", "render_lut.npy")
BLACK, FRAME, DEPTH, LABELS = 0, 1, 2, 3
LINES_NONE, LINES_SCORE, LINES_KIND, LINES_FIXED = 0, 1, 2, 3
MAX_COORD = 32767.0
LIST = 256                                                # rows the kernel's LDS list holds (csrc/render.hip: kList)
TILE_W, TILE_H = 64, 16                                   # its tile


def jet_table():
    red = [(0.0, 0.0), (0.35, 0.0), (0.66, 1.0), (0.89, 1.0), (1.0, 0.5)]
    green = [(0.0, 0.0), (0.125, 0.0), (0.375, 1.0), (0.64, 1.0), (0.91, 0.0), (1.0, 0.0)]
    blue = [(0.0, 0.5), (0.11, 1.0), (0.34, 1.0), (0.65, 0.0), (1.0, 0.0)]
    out = np.zeros((256, 3), np.uint8)
    step = 1.0 / 255.0
    for i in range(256):
        x = 1.0 if i == 255 else i * step                 # numpy.linspace(0, 1, 256)
        for ch, seg in enumerate((red, green, blue)):
            if x >= seg[-1][0]:
                v = seg[-1][1]
            else:                                         # numpy.interp: the last knot at or below x, slope times distance plus its value
                j = max(k for k in range(len(seg) - 1) if seg[k][0] <= x)
                (xa, ya), (xb, yb) = seg[j], seg[j + 1]
                v = ((yb - ya) / (xb - xa)) * (x - xa) + ya
            out[i, ch] = int(v * 255.0)                    # truncated, as matplotlib's bytes are
    return out


def voc_palette():
    out = np.zeros((256, 3), np.uint8)
    for i in range(255):                                  # 255 stays black
        for bit in range(24):
            if (i >> bit) & 1:
                out[i, bit % 3] |= 1 << (7 - bit // 3)
    return out


def depth_index(mm, lo_mm, hi_mm):
    span = hi_mm - lo_mm
    return np.clip((2 * 255 * (np.asarray(mm, np.int64) - lo_mm) + span) // (2 * span), 0, 255)


def tint(c, t, a):
    return (np.asarray(c, np.int64) * (256 - a) + np.asarray(t, np.int64) * a + 128) >> 8


def quantise(v):
    """One coordinate (float64) -> 1/16 pixel."""
    return int(np.floor(16.0 * np.float64(v) + 0.5))


def score_index(s, lo, k):
    v = (np.float64(s) - np.float64(lo)) * np.float64(k)
    return int(min(max(np.floor(v), 0.0), 255.0))


def rows_of(b, C, lines, count, order, scores, kinds, opts):
    """The rows of frame b that are drawn, in row order: (r, (ax, ay, bx, by), score index, kind)."""
    out = []
    if lines is None:
        return out
    for r in range(min(max(int(count[b]), 0), C)):
        src = int(order[b, r]) if order is not None else r
        if not 0 <= src < C:
            continue
        v = np.asarray(lines[b, src], np.float64)
        if not (np.isfinite(v).all() and (np.abs(v) <= MAX_COORD).all()):
            continue
        sidx = 0
        if scores is not None:
            s = np.float64(scores[b, src])
            if np.isnan(s) or s < opts["min_score"]:
                continue
            sidx = score_index(s, opts["score_lo"], opts["score_k"])
        kind = 0
        if kinds is not None and 0 <= int(kinds[b, r]) <= 4:
            kind = int(kinds[b, r])
        out.append((r, tuple(quantise(c) for c in v), sidx, kind))
    return out


def covered(px, py, row, h):
    """Pixels (points px, py in 1/16 pixel, int64 arrays) within h of the segment: the rule of the issue, term by term."""
    ax, ay, bx, by = row
    dx, dy = bx - ax, by - ay
    L2 = dx * dx + dy * dy
    qx, qy = px - ax, py - ay
    t = qx * dx + qy * dy
    cr = qx * dy - qy * dx
    near_a = qx * qx + qy * qy <= h * h
    near_b = (px - bx) ** 2 + (py - by) ** 2 <= h * h
    small = np.abs(cr) < 2 ** 31
    mid = small & (np.where(small, cr, 0) ** 2 <= h * h * L2)
    return np.where(t <= 0, near_a, np.where(t >= L2, near_b, mid))


def disc(px, py, cx, cy, r):
    return (px - cx) ** 2 + (py - cy) ** 2 <= r * r


def frame_size(b, sizes, Fh, Fw, operands):
    """(fh, fw) of frame b: sizes clamped to the canvas and to what every operand of the frame covers."""
    fh, fw = min(max(int(sizes[b, 0]), 0), Fh), min(max(int(sizes[b, 1]), 0), Fw)
    for op in operands:
        if op is not None:
            fh, fw = min(fh, op[b].shape[0]), min(fw, op[b].shape[1])
    return fh, fw


def coverage(fh, fw, rows, opts, want_lines=True, want_ends=True):
    """-> first (fh, fw) int32: the index INTO rows of the first row covering the pixel, or -1; dot (fh, fw) bool: an end disc does."""
    py, px = np.meshgrid(16 * np.arange(fh, dtype=np.int64) + 8, 16 * np.arange(fw, dtype=np.int64) + 8, indexing="ij")
    first = np.full((fh, fw), -1, np.int32)
    dot = np.zeros((fh, fw), bool)
    R = 16 * opts["end_radius"]
    for k, (_, row, _, _) in enumerate(rows):
        if want_lines:
            first[(first < 0) & covered(px, py, row, opts["width8"])] = k
        if want_ends and R > 0:
            dot |= disc(px, py, row[0], row[1], R) | disc(px, py, row[2], row[3], R)
    return first, dot


def outline(rmap, fh, fw):
    """The rank whose colour an outline pixel takes, else 0."""
    m = np.asarray(rmap[:fh, :fw], np.int32)
    pad = np.full((fh + 2, fw + 2), -1, np.int32)          # outside the frame: another value than any rank
    pad[1:-1, 1:-1] = m
    edge = (pad[:-2, 1:-1] != m) | (pad[2:, 1:-1] != m) | (pad[1:-1, :-2] != m) | (pad[1:-1, 2:] != m)
    return np.where((m > 0) & edge, m, 0)


def render(shape, sizes, tables, panels, frames=None, planes=(), label_planes=(), region_map=None, lines=None, count=None, order=None,
           scores=None, kinds=None, opts=None):
    """shape (B, P, Fh, Fw); frames: B arrays (h, w, 3); planes / label_planes: lists of B-lists of 2-D arrays; region_map: a B-list.
    -> canvas (B, P, Fh, Fw, 3) uint8."""
    B, P, Fh, Fw = shape
    canvas = np.zeros((B, P, Fh, Fw, 3), np.uint8)
    want_lines = any(p["lines"] != LINES_NONE for p in panels)
    want_ends = any(p["ends"] for p in panels)
    C = 0 if lines is None else lines.shape[1]
    for b in range(B):
        fh, fw = frame_size(b, sizes, Fh, Fw, [frames, region_map] + list(planes) + list(label_planes))
        if fh == 0 or fw == 0:
            continue
        rows = rows_of(b, C, lines, count, order, scores, kinds, opts) if (want_lines or want_ends) else []
        first, dot = coverage(fh, fw, rows, opts, want_lines, want_ends) if rows else (np.full((fh, fw), -1, np.int32), np.zeros((fh, fw), bool))
        ring = outline(region_map[b], fh, fw) if region_map is not None and any(p["outlines"] for p in panels) else None
        sidx = np.asarray([r[2] for r in rows] + [0], np.int64)
        kind = np.asarray([r[3] for r in rows] + [0], np.int64)
        for k, p in enumerate(panels):
            c = np.zeros((fh, fw, 3), np.int64)
            if p["base"] == FRAME:
                c[:] = frames[b][:fh, :fw]
            elif p["base"] == DEPTH:
                mm = np.asarray(planes[p["plane"]][b][:fh, :fw], np.int64)
                c[:] = tables[p["table"]][depth_index(mm, p["lo_mm"], p["hi_mm"])]
                c[mm == 0] = p["void"]
            elif p["base"] == LABELS:
                c[:] = tables[p["table"]][np.asarray(label_planes[p["plane"]][b][:fh, :fw], np.int64)]
            if p["tint"] >= 0:
                glass = np.asarray(label_planes[p["tint"]][b][:fh, :fw]) == 1
                c[glass] = tint(c[glass], p["tint_rgb"], p["tint_alpha"])
            if p["outlines"]:
                c[ring > 0] = tables[p["region_table"]][ring[ring > 0] - 1]
            if p["lines"] != LINES_NONE:
                on = first >= 0
                if p["lines"] == LINES_SCORE:
                    c[on] = tables[p["line_table"]][sidx[first[on]]]
                elif p["lines"] == LINES_KIND:
                    c[on] = tables[p["line_table"]][kind[first[on]]]
                else:
                    c[on] = p["line_rgb"]
            if p["ends"]:
                c[dot] = p["end_rgb"]
            canvas[b, k, :fh, :fw] = c
    return canvas


def rows_through_tiles(fh, fw, rows, opts):
    """How many drawn rows cover at least one pixel of each kernel tile: (tiles_y, tiles_x) int - what its LDS list must take."""
    py, px = np.meshgrid(16 * np.arange(fh, dtype=np.int64) + 8, 16 * np.arange(fw, dtype=np.int64) + 8, indexing="ij")
    ty, tx = (fh + TILE_H - 1) // TILE_H, (fw + TILE_W - 1) // TILE_W
    n = np.zeros((ty, tx), np.int64)
    for _, row, _, _ in rows:
        hit = covered(px, py, row, opts["width8"])
        for j in range(ty):
            for i in range(tx):
                n[j, i] += bool(hit[j * TILE_H:(j + 1) * TILE_H, i * TILE_W:(i + 1) * TILE_W].any())
    return n


def load_golden():
    return dict(np.load(GOLDEN, allow_pickle=False))
