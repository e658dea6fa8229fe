"""Rendering of predict_frames' results: the host side of gwd_render_frames (ops.render_frames, InferenceSession(render=...)).

* the colour tables: matplotlib's `jet` rebuilt from its segment data (jet_table), the PASCAL-VOC palette by its bit rule
  (voc_palette; its first 21 entries are the reference's COLORS, src/util/commons.py:13-17), the region colours and the colours of
  profile_kind;
* the panel and call options, checked and brought into the integers the kernel takes (resolve) - an unknown key raises TypeError,
  as InferenceSession(regions=...) does;
* save_panels: ONE device-to-host copy of a canvas, every frame cropped to its size, PNGs written with Pillow from a small thread
  pool (the encoding is the slow part of saving, not the rendering: DESIGN.md section 27).

What a panel is, layer over layer, is stated in include/gwdepth.h (gwd_render_frames) and in numpy in tests/render_ref.py."""
import functools
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

BLACK, FRAME, DEPTH, LABELS = 0, 1, 2, 3                  # GWD_RENDER_*: a panel's base
LINES_NONE, LINES_SCORE, LINES_KIND, LINES_FIXED = 0, 1, 2, 3
MAX_PANELS, MAX_PLANES, MAX_TABLES, MAX_WIDTH8, MAX_END_RADIUS = 8, 4, 16, 128, 64

PANEL_KEYS = ("base", "table", "range", "void", "tint", "tint_alpha", "tint_color", "outlines", "region_colors", "lines", "score_table",
              "kind_colors", "ends", "end_color")
RENDER_OPTIONS = ("width", "end_radius", "min_score", "score_range", "canvas_size")
END_COLOR = (0x33, 0xFF, 0xFF)                            # the reference's end markers, '#33FFFF' (evaluation/eval_post_online.py)
TINT_COLOR, TINT_ALPHA = (0, 255, 0), 102                 # 40 % green over the glass
KIND_COLORS = ((160, 160, 160), (255, 128, 0), (0, 128, 255), (255, 0, 255), (255, 255, 0))      # profile_kind 0 .. 4
DEPTH_RANGE = (0, 8500)                                   # millimetres over the table: the reference's alpha = 0.03 per mm, rounded half up
SCORE_RANGE = (0.92, 1.02)                                # the reference's norm for line scores

# matplotlib's `jet` (its public segment data: x, y0, y1 per channel)
_JET = {"red": ((0.0, 0, 0), (0.35, 0, 0), (0.66, 1, 1), (0.89, 1, 1), (1.0, 0.5, 0.5)),
        "green": ((0.0, 0, 0), (0.125, 0, 0), (0.375, 1, 1), (0.64, 1, 1), (0.91, 0, 0), (1.0, 0, 0)),
        "blue": ((0.0, 0.5, 0.5), (0.11, 1, 1), (0.34, 1, 1), (0.65, 0, 0), (1.0, 0, 0))}


def _frozen(t):
    t.setflags(write=False)                               # the builders are cached: what they return is shared
    return t


@functools.lru_cache(maxsize=None)
def jet_table():
    """(256, 3) uint8 (read-only): matplotlib's `jet` as its bytes come out - the segments interpolated over linspace(0, 1, 256), times
    255, TRUNCATED."""
    x = np.linspace(0.0, 1.0, 256)
    cols = []
    for ch in ("red", "green", "blue"):
        seg = np.asarray(_JET[ch], dtype=np.float64)
        cols.append(np.interp(x, seg[:, 0], seg[:, 1]))
    return _frozen((np.stack(cols, axis=1) * 255.0).astype(np.uint8))


@functools.lru_cache(maxsize=None)
def voc_palette():
    """(256, 3) uint8 (read-only): the PASCAL-VOC bit rule (bit k of the index feeds bit 7 - k // 3 of channel k % 3); 255 is black."""
    pal = np.zeros((256, 3), dtype=np.uint8)
    for i in range(255):
        c = i
        for j in range(8):
            for ch in range(3):
                pal[i, ch] |= ((c >> ch) & 1) << (7 - j)
            c >>= 3
    return _frozen(pal)


def _bitrev5(v):
    return int("{:05b}".format(v)[::-1], 2)


@functools.lru_cache(maxsize=None)
def region_colors():
    """(256, 3) uint8 (read-only): rank r - 1 takes jet at 8 * bitrev5(r - 1) + 4 - neighbouring ranks lie far apart on it."""
    out = np.zeros((256, 3), dtype=np.uint8)
    out[:32] = jet_table()[[8 * _bitrev5(k) + 4 for k in range(32)]]
    return _frozen(out)


@functools.lru_cache(maxsize=None)
def kind_colors():
    out = np.zeros((256, 3), dtype=np.uint8)
    out[:5] = KIND_COLORS
    return _frozen(out)


def _table(value, name, rows=256):
    t = np.asarray(value)
    if t.dtype != np.uint8 or t.ndim != 2 or t.shape[1] != 3 or not rows <= t.shape[0] <= 256:
        raise ValueError("render: %s must be a uint8 (%s, 3) table, got %s %s" % (name, rows if rows == 256 else "%d..256" % rows, t.dtype, t.shape))
    out = np.zeros((256, 3), dtype=np.uint8)
    out[:t.shape[0]] = t
    return out


def _rgb(value, name):
    try:
        c = tuple(int(v) for v in value)
    except TypeError:
        c = ()
    if len(c) != 3 or any(not 0 <= v <= 255 for v in c) or any(int(v) != v for v in value):
        raise ValueError("render: %s must be three integers 0..255, got %r" % (name, value))
    return c


def check_options(width=2.0, end_radius=2, min_score=None, score_range=SCORE_RANGE, canvas_size=None):
    """The options of one call -> dict(width8, end_radius, min_score, score_lo, score_k, canvas_size)."""
    if not 0.0 < float(width) <= 16.0 or int(np.floor(8.0 * float(width) + 0.5)) < 1:
        raise ValueError("render: 0 < width <= 16 pixels (at least 1/16), got %r" % (width,))
    if int(end_radius) != end_radius or not 0 <= int(end_radius) <= MAX_END_RADIUS:
        raise ValueError("render: end_radius is an integer 0..%d pixels, got %r" % (MAX_END_RADIUS, end_radius))
    lo, hi = (float(v) for v in score_range)
    if not (np.isfinite(lo) and np.isfinite(hi) and lo < hi) or not np.isfinite(256.0 / (hi - lo)):
        raise ValueError("render: score_range must be finite with lo < hi, got %r" % (score_range,))
    if min_score is not None and np.isnan(float(min_score)):
        raise ValueError("render: min_score must not be NaN")
    if canvas_size is not None:
        canvas_size = tuple(int(v) for v in canvas_size)
        if len(canvas_size) != 2 or not all(1 <= v <= 16384 for v in canvas_size):
            raise ValueError("render: canvas_size = (Fh, Fw), sides 1..16384, got %r" % (canvas_size,))
    return dict(width8=int(np.floor(8.0 * float(width) + 0.5)), end_radius=int(end_radius),
                min_score=float("-inf") if min_score is None else float(min_score), score_lo=lo, score_k=256.0 / (hi - lo),
                canvas_size=canvas_size)


def check_panels(panels):
    """Panels as the caller writes them -> a list of dicts with every PANEL_KEYS entry; TypeError on an unknown key."""
    if isinstance(panels, dict) or not isinstance(panels, (list, tuple)) or not 1 <= len(panels) <= MAX_PANELS:
        raise ValueError("render: panels is a list of 1..%d panels" % MAX_PANELS)
    out = []
    for k, p in enumerate(panels):
        if isinstance(p, (str, tuple)):
            p = {"base": p}
        if not isinstance(p, dict):
            raise TypeError("render: panel %d must be a dict (or just its base), got %r" % (k, p))
        if set(p) - set(PANEL_KEYS):
            raise TypeError("render: panel %d: unknown key(s) %s (known: %s)" % (k, sorted(set(p) - set(PANEL_KEYS)), ", ".join(PANEL_KEYS)))
        base = p.get("base", "black")
        if isinstance(base, str) and base in ("depth", "labels"):
            base = (base, 0)
        if base not in ("black", "frame") and not (isinstance(base, tuple) and len(base) == 2 and base[0] in ("depth", "labels")
                                                   and isinstance(base[1], int) and 0 <= base[1] < MAX_PLANES):
            raise ValueError("render: panel %d: base is 'black', 'frame', ('depth', i) or ('labels', i), got %r" % (k, base))
        lo, hi = (int(v) for v in p.get("range", DEPTH_RANGE))
        if not 0 <= lo < hi <= 65535:
            raise ValueError("render: panel %d: range = (lo_mm, hi_mm) with 0 <= lo < hi <= 65535, got %r" % (k, p.get("range")))
        tint = p.get("tint")
        if tint is not None and (not isinstance(tint, int) or isinstance(tint, bool) or not 0 <= tint < MAX_PLANES):
            raise ValueError("render: panel %d: tint is None or the index of a label plane, got %r" % (k, tint))
        alpha = p.get("tint_alpha", TINT_ALPHA)
        if int(alpha) != alpha or not 0 <= int(alpha) <= 256:
            raise ValueError("render: panel %d: tint_alpha is an integer 0..256, got %r" % (k, alpha))
        lines = p.get("lines")
        if lines is not None and lines not in ("score", "kind"):
            lines = _rgb(lines, "panel %d: lines ('score', 'kind' or a colour)" % k)
        is_labels = base not in ("black", "frame") and base[0] == "labels"
        out.append(dict(
            base=base, table=_table(p["table"], "table") if p.get("table") is not None else (voc_palette() if is_labels else jet_table()),
            range=(lo, hi), void=_rgb(p.get("void", (0, 0, 0)), "void"), tint=tint, tint_alpha=int(alpha),
            tint_color=_rgb(p.get("tint_color", TINT_COLOR), "tint_color"), outlines=bool(p.get("outlines", False)),
            region_colors=_table(p["region_colors"], "region_colors", 1) if p.get("region_colors") is not None else region_colors(),
            lines=lines, score_table=_table(p["score_table"], "score_table") if p.get("score_table") is not None else jet_table(),
            kind_colors=_table(p["kind_colors"], "kind_colors", 5) if p.get("kind_colors") is not None else kind_colors(),
            ends=bool(p.get("ends", lines is not None)), end_color=_rgb(p.get("end_color", END_COLOR), "end_color")))
    return out


def resolve(panels, n_planes, n_label_planes, has_frames, has_region_map, has_lines, has_scores, has_kinds):
    """Checked panels against the operands of a call -> (tables (T, 256, 3) uint8, records): per panel the integers of
    gwd_render_panel, every table named by its index in `tables` (equal tables are stored once)."""
    tables, index = [], {}

    def slot(t):
        key = t.tobytes()
        if key not in index:
            index[key] = len(tables)
            tables.append(t)
        return index[key]

    recs = []
    for k, p in enumerate(check_panels(panels)):
        r = dict(base=BLACK, plane=0, table=0, lo_mm=p["range"][0], hi_mm=p["range"][1], void=p["void"], tint=-1, tint_alpha=p["tint_alpha"],
                 tint_rgb=p["tint_color"], outlines=0, region_table=0, lines=LINES_NONE, line_table=0, line_rgb=(0, 0, 0), ends=0,
                 end_rgb=p["end_color"])
        base = p["base"]
        if base == "frame":
            if not has_frames:
                raise ValueError("render: panel %d shows the frame, but no frames were passed" % k)
            r["base"] = FRAME
        elif base != "black":
            have = n_planes if base[0] == "depth" else n_label_planes
            if base[1] >= have:
                raise ValueError("render: panel %d names %s plane %d of %d" % (k, base[0], base[1], have))
            r.update(base=DEPTH if base[0] == "depth" else LABELS, plane=base[1], table=slot(p["table"]))
        if p["tint"] is not None:
            if p["tint"] >= n_label_planes:
                raise ValueError("render: panel %d tints by label plane %d of %d" % (k, p["tint"], n_label_planes))
            r["tint"] = p["tint"]
        if p["outlines"]:
            if not has_region_map:
                raise ValueError("render: panel %d draws region outlines, but no region_map was passed" % k)
            r.update(outlines=1, region_table=slot(p["region_colors"]))
        if p["lines"] is not None or p["ends"]:
            if not has_lines:
                raise ValueError("render: panel %d draws lines, but no lines were passed" % k)
            r["ends"] = int(p["ends"])
        if p["lines"] == "score":
            if not has_scores:
                raise ValueError("render: panel %d colours lines by score, but no scores were passed" % k)
            r.update(lines=LINES_SCORE, line_table=slot(p["score_table"]))
        elif p["lines"] == "kind":
            if not has_kinds:
                raise ValueError("render: panel %d colours lines by kind, but no kinds were passed" % k)
            r.update(lines=LINES_KIND, line_table=slot(p["kind_colors"]))
        elif p["lines"] is not None:
            r.update(lines=LINES_FIXED, line_rgb=p["lines"])
        recs.append(r)
    if not tables:
        tables.append(np.zeros((256, 3), dtype=np.uint8))
    if len(tables) > MAX_TABLES:
        raise ValueError("render: at most %d distinct colour tables per call, got %d" % (MAX_TABLES, len(tables)))
    return np.stack(tables), recs


# ---------------------------------------------------------------------------------------------------------------------- saving
def save_panels(canvas, sizes, paths, layout="row", suffixes=None, workers=4):
    """canvas (B, P, Fh, Fw, 3) uint8 (device or host), sizes: B (fh, fw) pairs (a tensor or a nested sequence), paths: B file names.
    layout="row": paths[b] gets frame b's P panels side by side; "files": one file per panel, the panel's suffix (suffixes: P
    strings, default "_0", "_1", ...) set before the extension of paths[b].  ONE device-to-host copy of the canvas; every frame is
    cropped to its size; PNG encoding runs in `workers` threads.  -> the files written, frame by frame."""
    from PIL import Image
    if layout not in ("row", "files"):
        raise ValueError("save_panels: layout is 'row' or 'files', got %r" % (layout,))
    host = canvas.cpu().numpy() if hasattr(canvas, "cpu") else np.asarray(canvas)
    if host.ndim != 5 or host.shape[4] != 3 or host.dtype != np.uint8:
        raise ValueError("save_panels: canvas must be uint8 (B, P, Fh, Fw, 3), got %s %s" % (host.dtype, host.shape))
    B, P = host.shape[:2]
    sizes = np.asarray(sizes.cpu() if hasattr(sizes, "cpu") else sizes).reshape(-1, 2)
    if len(sizes) != B or len(paths) != B:
        raise ValueError("save_panels: %d frames, %d sizes, %d paths" % (B, len(sizes), len(paths)))
    suffixes = ["_%d" % p for p in range(P)] if suffixes is None else list(suffixes)
    if layout == "files" and len(suffixes) != P:
        raise ValueError("save_panels: %d panels, %d suffixes" % (P, len(suffixes)))
    jobs = []
    for b in range(B):
        fh, fw = (int(min(max(v, 0), lim)) for v, lim in zip(sizes[b], host.shape[2:4]))
        if fh == 0 or fw == 0:
            raise ValueError("save_panels: frame %d is empty" % b)
        crop = host[b, :, :fh, :fw]
        if layout == "row":
            jobs.append((np.concatenate(list(crop), axis=1), str(paths[b])))
        else:
            stem, ext = os.path.splitext(str(paths[b]))
            jobs += [(crop[p], stem + suffixes[p] + (ext or ".png")) for p in range(P)]

    def write(job):
        Image.fromarray(np.ascontiguousarray(job[0]), "RGB").save(job[1], format="PNG")
        return job[1]

    with ThreadPoolExecutor(max_workers=max(1, int(workers))) as pool:
        return list(pool.map(write, jobs))
