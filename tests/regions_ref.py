"""The numpy / scipy restatement of csrc/regions.hip (include/gwdepth.h: gwd_glass_regions, gwd_region_planes, gwd_depth_planar):
scipy.ndimage.label per frame, the ranking rule, the integer records, the plane fit by numpy.linalg.lstsq on centred columns in
fp64 and the planar depth - plus the hand-built masks the GPU tests run on and the loader of tests/golden/glass_regions.npz."""
import math
import os

import numpy as np
from scipy import ndimage

FIELDS = ("area", "x0", "y0", "x1", "y1", "anchor", "sum_x", "sum_y", "n_depth", "sum_mm", "min_mm", "max_mm")
STRUCTURE = {8: np.ones((3, 3), dtype=bool), 4: np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], dtype=bool)}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "glass_regions.npz")


def components(mask, connectivity):
    """-> (lab int32 (h, w): 0 = background, k = 1.. in ascending order of the component's anchor; anchors, areas)."""
    lab, n = ndimage.label(mask, structure=STRUCTURE[connectivity])
    if n == 0:
        return lab.astype(np.int32), np.zeros(0, np.int64), np.zeros(0, np.int64)
    flat = lab.ravel()
    idx = np.nonzero(flat)[0]
    anchors = np.full(n + 1, flat.size, dtype=np.int64)
    np.minimum.at(anchors, flat[idx], idx)
    order = np.argsort(anchors[1:], kind="stable")
    remap = np.zeros(n + 1, dtype=np.int32)
    remap[order + 1] = np.arange(1, n + 1)
    out = remap[lab]
    return out, anchors[1:][order], np.bincount(out.ravel(), minlength=n + 1)[1:].astype(np.int64)


def glass_regions(labels, depth_mm, sizes, max_regions=32, min_area=100, connectivity=8, lo_mm=1, hi_mm=10000, max_candidates=8192):
    """labels uint8 / depth_mm uint16 (B, Fh, Fw), sizes (B, 2) -> region_map, region_count, region_total, regions as the kernels give them."""
    B, Fh, Fw = labels.shape
    rmap = np.zeros((B, Fh, Fw), np.uint8)
    count, total = np.zeros(B, np.int32), np.zeros(B, np.int32)
    rec = np.zeros((B, max_regions, len(FIELDS)), np.int64)
    for b in range(B):
        fh, fw = (int(v) for v in sizes[b])
        lab, anchors, areas = components(labels[b, :fh, :fw] == 1, connectivity)
        total[b] = len(anchors)
        cand = np.nonzero(areas >= min_area)[0]
        if len(cand) > max_candidates:
            count[b] = -1
            continue
        kept = sorted(cand, key=lambda k: (-areas[k], anchors[k]))[:max_regions]
        count[b] = len(kept)
        mm = depth_mm[b, :fh, :fw].astype(np.int64)
        for r, k in enumerate(kept):
            ys, xs = np.nonzero(lab == k + 1)
            rmap[b, ys, xs] = r + 1
            m = mm[ys, xs]
            m = m[(m >= lo_mm) & (m <= hi_mm)]
            rec[b, r] = (len(xs), xs.min(), ys.min(), xs.max(), ys.max(), anchors[k], xs.sum(), ys.sum(), len(m), m.sum(),
                         m.min() if len(m) else 0, m.max() if len(m) else 0)
    return {"region_map": rmap, "region_count": count, "region_total": total, "regions": rec}


def region_pixels(region_map, depth_mm, r, lo_mm=1, hi_mm=10000):
    """(x, y, w) of the pixels with depth of rank r in one image, raster order; w = 1000 / mm in fp64."""
    ys, xs = np.nonzero(region_map == r + 1)
    m = depth_mm[ys, xs].astype(np.int64)
    ok = (m >= lo_mm) & (m <= hi_mm)
    return xs[ok].astype(np.int64), ys[ok].astype(np.int64), 1000.0 / m[ok].astype(np.float64)


def collinear(x, y):
    """Exact: the determinant of the centred second moments, scaled by n^2, in Python integers."""
    n, sx, sy = len(x), int(x.sum()), int(y.sum())
    sxx, sxy, syy = int((x * x).sum()), int((x * y).sum()), int((y * y).sum())
    return (n * sxx - sx * sx) * (n * syy - sy * sy) - (n * sxy - sx * sy) ** 2 == 0


def fit_plane(x, y, w):
    """numpy.linalg.lstsq on centred columns -> (alpha, beta, gamma, rms, n, status) in absolute frame coordinates."""
    n = len(x)
    if n < 3 or collinear(x, y):
        return (np.nan, np.nan, np.nan, np.nan, float(n), 1.0)
    mx, my, mw = x.mean(), y.mean(), w.mean()
    A = np.stack([x - mx, y - my], 1)
    (alpha, beta), *_ = np.linalg.lstsq(A, w - mw, rcond=None)
    gamma = mw - alpha * mx - beta * my
    res = (w - mw) - A @ np.array([alpha, beta])
    return (alpha, beta, gamma, math.sqrt(float(res @ res) / n), float(n), 0.0)


def normal_cond(x, y):
    """cond of the centred 2 x 2 normal matrix: the kappa of the tests' bound."""
    A = np.stack([x - x.mean(), y - y.mean()], 1).astype(np.float64)
    return float(np.linalg.cond(A.T @ A))


def fit_from_moments(x, y, w, summer):
    """The kernel's route - ten moments relative to the box corner, the centred 2 x 2 system, gamma from the means, shifted back -
    with the summation left to `summer` (math.fsum, or a naive loop in any order)."""
    x0, y0 = int(x.min()), int(y.min())
    dx, dy = (x - x0).astype(np.float64), (y - y0).astype(np.float64)
    n = float(len(x))
    Sx, Sy, Sxx, Sxy, Syy = (float(int(v.sum())) for v in ((x - x0), (y - y0), (x - x0) ** 2, (x - x0) * (y - y0), (y - y0) ** 2))
    Sw, Sxw, Syw = summer(w), summer(dx * w), summer(dy * w)
    dxx, dyy, dxy = n * Sxx - Sx * Sx, n * Syy - Sy * Sy, n * Sxy - Sx * Sy
    dxw, dyw = n * Sxw - Sx * Sw, n * Syw - Sy * Sw
    det = dxx * dyy - dxy * dxy
    alpha, beta = (dyy * dxw - dxy * dyw) / det, (dxx * dyw - dxy * dxw) / det
    gamma = (Sw - alpha * Sx - beta * Sy) / n - alpha * x0 - beta * y0
    return alpha, beta, gamma


def region_planes(region_map, depth_mm, region_count, max_regions, lo_mm=1, hi_mm=10000):
    B = region_map.shape[0]
    planes = np.zeros((B, max_regions, 6), np.float64)
    for b in range(B):
        for r in range(max(int(region_count[b]), 0)):
            planes[b, r] = fit_plane(*region_pixels(region_map[b], depth_mm[b], r, lo_mm, hi_mm))
    return planes


def to_mm(d):
    """gwd_dense_postprocess's conversion: rint(fp32 metres * 1000) in fp32, saturated to uint16."""
    mm = np.rint(d.astype(np.float32) * np.float32(1000.0))
    return np.clip(mm, 0, 65535).astype(np.uint16)


def plane_denominator(planes_b, region_map_b):
    """alpha x + beta y + gamma in fp64 at every pixel of a kept region of status 0 (NaN elsewhere), as the kernel rounds it."""
    h, w = region_map_b.shape
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    den = np.full((h, w), np.nan)
    for r in range(planes_b.shape[0]):
        if planes_b[r, 5] == 0.0:
            sel = region_map_b == r + 1
            den[sel] = ((planes_b[r, 0] * xs + planes_b[r, 1] * ys) + planes_b[r, 2])[sel]
    return den


def depth_planar(region_map, depth_mm, depth, sizes, region_count, planes, min_depth=1e-3, max_depth=10.0):
    """-> (depth_planar fp32, depth_planar_mm uint16, rewritten bool, z fp64 before the rounding to fp32)."""
    B, Fh, Fw = region_map.shape
    base = (depth_mm.astype(np.float32) / np.float32(1000.0)) if depth is None else depth
    out, out_mm = np.zeros((B, Fh, Fw), np.float32), np.zeros((B, Fh, Fw), np.uint16)
    hit, z64 = np.zeros((B, Fh, Fw), bool), np.zeros((B, Fh, Fw), np.float64)
    lo, hi = float(np.float32(min_depth)), float(np.float32(max_depth))
    for b in range(B):
        fh, fw = (int(v) for v in sizes[b])
        out[b, :fh, :fw], out_mm[b, :fh, :fw] = base[b, :fh, :fw], depth_mm[b, :fh, :fw]
        if region_count[b] <= 0:
            continue
        live = planes[b].copy()
        live[int(region_count[b]):, 5] = 1.0
        den = plane_denominator(live, region_map[b])
        sel = den > 0.0
        with np.errstate(divide="ignore", invalid="ignore"):
            z = np.clip(1.0 / den, lo, hi)
        out[b][sel] = z[sel].astype(np.float32)
        out_mm[b][sel] = to_mm(out[b][sel])
        hit[b], z64[b][sel] = sel, z[sel]
    return out, out_mm, hit, z64


# ---------------------------------------------------------------------------------------------------- inputs
def hand_masks(h, w):
    """The masks union-find goes wrong on, h x w each (h, w >= 16): name -> bool array."""
    out = {}
    m = np.zeros((h, w), bool)                                 # a one-pixel-wide spiral: long parent chains
    y = x = 0
    dy, dx = 0, 1
    m[0, 0] = True
    moved = True
    while moved:                                               # walk on while two cells ahead are free, else turn right once
        moved = False
        for _ in range(2):
            ny, nx, ay, ax = y + dy, x + dx, y + 2 * dy, x + 2 * dx
            if 0 <= ny < h and 0 <= nx < w and not m[ny, nx] and not (0 <= ay < h and 0 <= ax < w and m[ay, ax]):
                y, x, moved = ny, nx, True
                m[y, x] = True
                break
            dy, dx = dx, -dy
    out["spiral"] = m
    m = np.zeros((h, w), bool)                                 # a comb whose teeth join in the last row only
    m[:, ::2] = True
    m[h - 1, :] = True
    out["comb"] = m
    m = np.zeros((h, w), bool)                                 # a U: two columns that meet in the last row
    m[:, 1] = m[:, w - 2] = True
    m[h - 1, 1:w - 1] = True
    out["u"] = m
    yy, xx = np.mgrid[0:h, 0:w]
    out["checkerboard"] = (yy + xx) % 2 == 0                   # one component 8-connected, ceil(h w / 2) of them 4-connected
    out["full"] = np.ones((h, w), bool)
    out["empty"] = np.zeros((h, w), bool)
    m = np.zeros((h, w), bool)
    m[0, 0] = m[0, w - 1] = m[h - 1, 0] = m[h - 1, w - 1] = True
    out["corners"] = m
    m = np.zeros((h, w), bool)                                 # a ring around a hole
    m[2:h - 2, 2:w - 2] = True
    m[5:h - 5, 5:w - 5] = False
    out["ring"] = m
    m = np.zeros((h, w), bool)                                 # two regions of equal area: the anchor breaks the tie
    m[1:5, w - 7:w - 1] = True
    m[h - 6:h - 2, 2:8] = True
    out["twins"] = m
    m = np.zeros((h, w), bool)                                 # a diagonal line: 8-connected, collinear (status 1)
    k = np.arange(min(h, w) - 2)
    m[k + 1, k + 1] = True
    out["diagonal"] = m
    return out


def plane_depth(mask, seed, connectivity=8, noise=2e-3):
    """uint16 millimetres for a mask: per component a plane in inverse depth plus seeded noise, rounded; 2500 elsewhere."""
    rng = np.random.default_rng(seed)
    h, w = mask.shape
    lab, anchors, _ = components(mask, connectivity)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    mm = np.full((h, w), 2500, np.uint16)
    for k in range(len(anchors)):
        sel = lab == k + 1
        w0 = rng.uniform(0.3, 1.0)
        a, b = rng.uniform(-1, 1, 2) * 0.3 * w0 / max(h, w)
        inv = w0 + a * (xs - xs[sel].mean()) + b * (ys - ys[sel].mean()) + rng.normal(0.0, noise * w0, (h, w))
        mm[sel] = np.clip(np.rint(1000.0 / np.maximum(inv[sel], 1e-2)), 1, 65535).astype(np.uint16)
    return mm


def load_golden():
    """-> [(name, mask bool (h, w), depth_mm uint16 (h, w))] of tests/golden/glass_regions.npz (tools/make_regions_fixture.py)."""
    z = np.load(GOLDEN)
    out = []
    for name in [str(n) for n in z["names"]]:
        h, w = (int(v) for v in z[name + "_shape"])
        out.append((name, np.unpackbits(z[name + "_bits"])[:h * w].reshape(h, w).astype(bool), z[name + "_mm"]))
    return out


def batch_of(items, Fh=None, Fw=None, fill_label=255, fill_mm=0, rng=None):
    """[(mask, mm)] -> labels uint8, depth_mm uint16 (B, Fh, Fw), sizes int32 (B, 2); outside a frame fill_label / fill_mm, or
    random bytes with rng."""
    Fh = Fh or max(m.shape[0] for m, _ in items)
    Fw = Fw or max(m.shape[1] for m, _ in items)
    B = len(items)
    if rng is None:
        labels = np.full((B, Fh, Fw), fill_label, np.uint8)
        depth = np.full((B, Fh, Fw), fill_mm, np.uint16)
    else:
        labels = rng.integers(0, 256, (B, Fh, Fw), dtype=np.uint8)
        depth = rng.integers(0, 65536, (B, Fh, Fw), dtype=np.uint16)
    sizes = np.zeros((B, 2), np.int32)
    for b, (m, mm) in enumerate(items):
        h, w = m.shape
        labels[b, :h, :w] = m.astype(np.uint8)
        depth[b, :h, :w] = mm
        sizes[b] = (h, w)
    return labels, depth, sizes
