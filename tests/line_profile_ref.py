"""The numpy fp64 statement of csrc/lineprofile.hip (include/gwdepth.h: gwd_line_profiles): every detected
line walked through the dense results - sample count, three probes per sample, exact counts, the affine fit of inverse depth along
the line, the glass sides, the framed panes and the 3-D end points.  The reference project has no such step, so this file IS the
definition; the kernel follows it.  Every operation below is one fp64 operation rounded on its own (numpy fuses nothing).

Also here: the bound the tests hold the fits to, the kernel's summation order restated (to show the bound does not depend on the
order), and the generator / loader of tests/golden/line_profiles.npz (`python -m tests.line_profile_ref` rewrites it)."""
import math
import os

import numpy as np

COUNT_FIELDS = ("samples", "on_in", "on_glass", "on_depth", "a_in", "a_glass", "a_depth", "b_in", "b_glass", "b_depth",
                "region_a", "region_b")
FIT_FIELDS = ("w0", "w1", "rms", "n_used", "status")
PROBES = ("on", "a", "b")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "line_profiles.npz")
MAX_RANK = 32
MIN_GRID_DISTANCE = 1e-9


# ---------------------------------------------------------------------------------------------------- geometry
def sample_count(L2, max_samples=2048):
    """n: the smallest integer >= 1 with n * n >= L2, limited to max_samples - 1; 0 for a degenerate line (L2 not a positive
    finite number).  The candidate comes from a square root and is corrected against n * n, which is exact."""
    L2 = float(L2)
    if not (L2 > 0.0) or math.isinf(L2):
        return 0
    cap = int(max_samples) - 1
    if L2 >= float(cap * cap):
        return cap
    n = int(math.ceil(math.sqrt(L2)))
    while n > 1 and float((n - 1) * (n - 1)) >= L2:
        n -= 1
    while float(n * n) < L2:
        n += 1
    return max(n, 1)


def probes(line, offset=3.0, max_samples=2048):
    """-> (n, t (S,), xy (3, S, 2)): the on / a / b positions of the S = n + 1 samples; n = 0: a degenerate line, nothing else."""
    x1, y1, x2, y2 = (np.float64(v) for v in line)
    with np.errstate(all="ignore"):
        dx, dy = x2 - x1, y2 - y1
        L2 = dx * dx + dy * dy
    n = sample_count(L2, max_samples)
    if n == 0:
        return 0, np.zeros(0), np.zeros((3, 0, 2))
    L = np.sqrt(L2)
    ox, oy = np.float64(offset) * (-dy / L), np.float64(offset) * (dx / L)
    t = np.arange(n + 1, dtype=np.float64) / np.float64(n)
    px, py = x1 + t * dx, y1 + t * dy
    return n, t, np.stack([np.stack([px, py], -1), np.stack([px + ox, py + oy], -1), np.stack([px - ox, py - oy], -1)])


def pixels(xy, fh, fw):
    """-> (inside bool (...), ix, iy int64 (...)): the pixel (floor x, floor y) of every probe, 0 where it is outside the frame."""
    x, y = xy[..., 0], xy[..., 1]
    with np.errstate(invalid="ignore"):
        inside = (x >= 0.0) & (x < float(fw)) & (y >= 0.0) & (y < float(fh))
    ix = np.where(inside, np.floor(np.where(inside, x, 0.0)), 0).astype(np.int64)
    iy = np.where(inside, np.floor(np.where(inside, y, 0.0)), 0).astype(np.int64)
    return inside, ix, iy


def grid_distance(line, offset=3.0, max_samples=2048):
    """The smallest distance of any probe coordinate of the line to an integer (a pixel boundary); inf for a degenerate line."""
    n, _, xy = probes(line, offset, max_samples)
    if n == 0 or not np.isfinite(xy).all():
        return math.inf
    return float(np.abs(xy - np.rint(xy)).min())


def exact_line(line, offset):
    """Axis-aligned, coordinates and offset multiples of 1/8 below 2^20: L, the unit normal and every coordinate ACROSS the line are
    exact; along the line only t = k / n and t dx are rounded, each once and correctly, the same on every implementation."""
    v = np.asarray(line, np.float64)
    eighth = bool((v * 8 == np.rint(v * 8)).all() and offset * 8 == round(offset * 8) and np.abs(v).max() < 2 ** 20)
    return eighth and (v[0] == v[2] or v[1] == v[3])


# ---------------------------------------------------------------------------------------------------- sums
def numpy_sum(v):
    return float(np.sum(v)) if len(v) else 0.0


def kernel_sum(v, k):
    """The kernel's order: lane l adds the values of its samples l, l + 64, ... in turn (a sample without depth adds 0.0), then
    the 64 lane sums fold through the xor tree 32, 16, ... 1.  v: the values of the used samples, k: their sample numbers."""
    lanes = [0.0] * 64
    for value, sample in sorted(zip(v.tolist(), k.tolist()), key=lambda p: p[1]):
        lanes[sample % 64] += value
    o = 32
    while o:
        lanes = [lanes[i] + lanes[i ^ o] for i in range(64)]
        o >>= 1
    return lanes[0]


def fit_line(t, w, k=None, summer=None):
    """Centred two-pass least squares of w over u = t - 0.5 -> (w0, w1, rms, n_used, status): the fit at t = 0 and t = 1."""
    n = len(t)
    if n < 2:
        return (np.nan, np.nan, np.nan, float(n), 1.0)
    s = numpy_sum if summer is None else (lambda v: summer(v, k))
    u = t - 0.5
    dn = np.float64(n)
    mu, mw = np.float64(s(u)) / dn, np.float64(s(w)) / dn
    cu, cw = u - mu, w - mw
    suu, suw = np.float64(s(cu * cu)), np.float64(s(cu * cw))
    slope = suw / suu
    e = cw - slope * cu
    rms = np.sqrt(np.float64(s(e * e)) / dn)
    return (float(mw + slope * (np.float64(-0.5) - mu)), float(mw + slope * (np.float64(0.5) - mu)), float(rms), float(n), 0.0)


def fit_bound(t, w):
    """max |w0 or w1 of one evaluation of fit_line - another's| when only the ORDER of the sums differs:
    (n + 8) 2^-52 max |w| (1 + 2 kappa), kappa = sqrt(n / Suu) - a fit from a short run of samples is extrapolated to the ends."""
    n = len(t)
    suu = float(((t - t.mean()) ** 2).sum())
    return (n + 8.0) * 2.0 ** -52 * float(np.abs(w).max()) * (1.0 + 2.0 * math.sqrt(n / suu))


# ---------------------------------------------------------------------------------------------------- the whole step
def line_samples(line, labels_b, depth_b, size_b, region_b=None, offset=3.0, max_samples=2048, lo_mm=1, hi_mm=10000):
    """One line in one image -> None (degenerate) or dict(n, t, inside, label, mm, rank, depth): (3, S) arrays per probe."""
    fh, fw = (int(v) for v in size_b)
    fh, fw = min(max(fh, 0), labels_b.shape[0]), min(max(fw, 0), labels_b.shape[1])
    n, t, xy = probes(line, offset, max_samples)
    if n == 0:
        return None
    inside, ix, iy = pixels(xy, fh, fw)
    label = np.where(inside, labels_b[iy, ix], 0).astype(np.int64)
    mm = np.where(inside, depth_b[iy, ix], 0).astype(np.int64)
    rank = np.zeros_like(mm) if region_b is None else np.where(inside, region_b[iy, ix], 0).astype(np.int64)
    rank[rank > MAX_RANK] = 0
    return {"n": n, "t": t, "inside": inside, "label": label, "mm": mm, "rank": rank, "depth": inside & (mm >= lo_mm) & (mm <= hi_mm)}


def side_state(n_in, n_glass, hi, lo):
    """-> (has glass, has none), in integers."""
    return n_in > 0 and 1000 * n_glass >= hi * n_in, n_in > 0 and 1000 * n_glass <= lo * n_in


def kind_of(a, b):
    """1 = glass on side a only, 2 = on side b only, 3 = on both, 4 = on neither, 0 = anything else."""
    (ag, an), (bg, bn) = a, b
    return 1 if ag and bn else 2 if bg and an else 3 if ag and bg else 4 if an and bn else 0


def framed_region(rank):
    """The rank (0-based) that holds the most samples, ties to the lower rank; -1 when none lies in a kept region."""
    hist = np.bincount(rank, minlength=MAX_RANK + 1)[1:]
    return int(np.argmax(hist)) if hist.max() > 0 else -1


def line_profiles(lines, count, labels, depth_mm, sizes, order=None, region_map=None, intrinsics=None, offset=3.0, max_samples=2048,
                  lo_mm=1, hi_mm=10000, hi=700, lo=300, summer=None):
    """-> dict(profile_counts (B,C,12) int32, profile_fits (B,C,3,5) float64, profile_kind (B,C) int32[, line_points (B,C,2,3)])."""
    lines = np.asarray(lines)
    B, C = lines.shape[:2]
    counts = np.zeros((B, C, 12), np.int32)
    counts[..., 10:] = -1
    fits = np.zeros((B, C, 3, 5), np.float64)
    fits[..., 4] = 3.0
    kind = np.zeros((B, C), np.int32)
    points = np.full((B, C, 2, 3), np.nan)
    for b in range(B):
        for r in range(min(max(int(count[b]), 0), C)):
            src = r if order is None else int(order[b, r])
            line = lines[b, src].astype(np.float64) if 0 <= src < C else np.zeros(4)
            s = line_samples(line, labels[b], depth_mm[b], sizes[b], None if region_map is None else region_map[b], offset, max_samples,
                             lo_mm, hi_mm)
            if s is None:
                fits[b, r] = (np.nan, np.nan, np.nan, 0.0, 2.0)
                continue
            k = np.arange(s["n"] + 1)
            row = [s["n"] + 1]
            for p in range(3):
                row += [int(s["inside"][p].sum()), int((s["inside"][p] & (s["label"][p] == 1)).sum()), int(s["depth"][p].sum())]
                use = s["depth"][p]
                fits[b, r, p] = fit_line(s["t"][use], 1000.0 / s["mm"][p][use].astype(np.float64), k[use], summer)
            counts[b, r, :10] = row
            if region_map is not None:
                counts[b, r, 10:] = framed_region(s["rank"][1]), framed_region(s["rank"][2])
            kind[b, r] = kind_of(side_state(row[4], row[5], hi, lo), side_state(row[7], row[8], hi, lo))
            if intrinsics is not None and fits[b, r, 0, 4] == 0.0:
                fx, fy, cx, cy = (np.float64(v) for v in intrinsics[b])
                for e, (x, y) in enumerate((line[:2], line[2:])):
                    w = np.float64(fits[b, r, 0, e])
                    if w > 0.0:
                        z = np.float64(1.0) / w
                        points[b, r, e] = ((x - cx) / fx * z, (y - cy) / fy * z, z)
    out = {"profile_counts": counts, "profile_fits": fits, "profile_kind": kind}
    if intrinsics is not None:
        out["line_points"] = points
    return out


def check_fits(got, want, lines, count, labels, depth_mm, sizes, order=None, offset=3.0, max_samples=2048, lo_mm=1, hi_mm=10000,
               intrinsics=None, got_points=None, want_points=None):
    """Another evaluation's profile_fits against this file's: n_used, status and the NaN placement exact, w0 / w1 within
    fit_bound, rms within twice that, the end points within the bound that error in w leaves.  -> the worst error / bound seen."""
    assert np.array_equal(got[..., 3:], want[..., 3:]), "n_used / status differ"
    assert np.array_equal(np.isnan(got), np.isnan(want)), "NaN placement differs"
    if want_points is not None:
        assert np.array_equal(np.isnan(got_points), np.isnan(want_points)), "NaN placement of line_points differs"
    worst = 0.0
    B, C = want.shape[:2]
    for b in range(B):
        for r in range(min(max(int(count[b]), 0), C)):
            src = r if order is None else int(order[b, r])
            line = np.asarray(lines[b, src], np.float64)
            s = line_samples(line, labels[b], depth_mm[b], sizes[b], None, offset, max_samples, lo_mm, hi_mm)
            for p in range(3):
                if want[b, r, p, 4] != 0.0:
                    continue
                use = s["depth"][p]
                bound = fit_bound(s["t"][use], 1000.0 / s["mm"][p][use].astype(np.float64))
                err = np.abs(got[b, r, p, :3] - want[b, r, p, :3]) / (bound, bound, 2.0 * bound)
                worst = max(worst, float(err.max()))
                assert err.max() <= 1.0, (b, r, PROBES[p], got[b, r, p], want[b, r, p], bound)
                if p == 0 and want_points is not None:
                    fx, fy, cx, cy = intrinsics[b]
                    for e, (x, y) in enumerate((line[:2], line[2:])):
                        w = want[b, r, 0, e]
                        if not w > 0.0:
                            continue
                        assert w > 2.0 * bound, "the fixture keeps every end point's w away from 0"
                        ray = np.abs(np.array([(x - cx) / fx, (y - cy) / fy, 1.0]))
                        pb = ray * (bound / (w * (w - bound))) + 2.0 ** -50 * np.abs(want_points[b, r, e])      # dz = dw / (w w'), a few roundings
                        perr = np.abs(got_points[b, r, e] - want_points[b, r, e])
                        worst = max(worst, float((perr / pb).max()))
                        assert (perr <= pb).all(), (b, r, e, got_points[b, r, e], want_points[b, r, e], pb)
    return worst


# ---------------------------------------------------------------------------------------------------- scenes
def plane_mm(h, w, alpha, beta, gamma):
    """uint16 millimetres of the plane w = alpha x + beta y + gamma (1 / m) sampled at the pixel centres (x + 0.5, y + 0.5)."""
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    inv = alpha * (xs + 0.5) + beta * (ys + 0.5) + gamma
    return np.clip(np.rint(1000.0 / inv), 1, 65535).astype(np.uint16)


def mm_rounding(w_max):
    """|1000 / rint(1000 / w) - w| <= this for 0 < w <= w_max: with mm = 1000 / w + rho, |rho| <= 1/2, the difference is
    w (rho w / 1000) / (1 + rho w / 1000)."""
    return 0.5 * w_max * w_max / 1000.0 / (1.0 - 0.5 * w_max / 1000.0)


def endpoint_gain(t, at):
    """sum |c_i| of the linear map samples -> fit at `at` (the fit reproduces affine data exactly, so an error of at most e in
    every sample moves the fit at `at` by at most this times e)."""
    u = t - t.mean()
    return float(np.abs(1.0 / len(t) + (at - t.mean()) * u / (u * u).sum()).sum())


def make_inputs(seed=20):
    """The fixture's inputs: three frames in one (3, 40, 56) plane, 70 line slots each, counts (70, 5, 0)."""
    rng = np.random.default_rng(seed)
    Fh, Fw, C, offset = 40, 56, 70, 3.0
    sizes = np.array([(40, 56), (37, 53), (17, 9)], np.int32)
    labels = rng.integers(0, 256, (3, Fh, Fw), dtype=np.uint8)          # what lies outside a frame (and all of frame 2) is noise
    depth = rng.integers(0, 65536, (3, Fh, Fw), dtype=np.uint16)
    rmap = rng.integers(0, 256, (3, Fh, Fw), dtype=np.uint8)
    # frame 0: a planar background, a pane (rank 0) whose depth steps along its edge, a second pane (rank 1), holes
    labels[0], rmap[0] = 0, 0
    depth[0] = plane_mm(40, 56, 0.004, -0.003, 0.5)
    labels[0, 8:30, 10:40], rmap[0, 8:30, 10:40] = 1, 1
    depth[0, 8:30, 10:40] = plane_mm(40, 56, -0.002, 0.005, 0.9)[8:30, 10:40]
    labels[0, 32:38, 44:54], rmap[0, 32:38, 44:54] = 1, 2
    labels[0, 2:5, 2:6] = 1                                             # glass in no kept region
    depth[0, 12:15, 20:26], depth[0, 20:24, 5:9] = 0, 40000             # holes: no value, and beyond hi_mm
    depth[0, 3, 30:50] = 10001
    # frame 1 (37 x 53): glass and a region, no pixel with valid depth
    labels[1, :37, :53], rmap[1, :37, :53] = 0, 0
    labels[1, 5:20, 5:45], rmap[1, 5:20, 5:45] = 1, 7
    depth[1, :37, :53] = np.where(rng.random((37, 53)) < 0.5, 0, 20000).astype(np.uint16)
    lines = np.zeros((3, C, 4), np.float64)
    fixed = [
        (10.0, 8.0, 40.0, 8.0), (40.0, 8.0, 40.0, 30.0), (40.0, 30.0, 10.0, 30.0), (10.0, 30.0, 10.0, 8.0),      # pane 0's border, on grid lines
        (40.0, 8.0, 10.0, 8.0), (10.0, 8.0, 10.0, 30.0),                                                         # ... two of them reversed
        (44.0, 32.0, 54.0, 32.0), (54.0, 38.0, 44.0, 38.0),                                                      # pane 1
        (0.0, 0.0, 56.0, 0.0), (0.0, 40.0, 56.0, 40.0), (56.0, 0.0, 56.0, 40.0), (0.0, 0.0, 0.0, 40.0),          # the frame's own border
        (-7.5, 20.125, 63.25, 20.125), (25.625, -9.0, 25.625, 49.5),                                             # through both borders, eighths
        (5.0, 5.0, 5.0, 5.0), (12.5, 7.25, 12.5, 7.25),                                                          # zero length
        (20.0, 10.125, 20.5, 10.125), (30.25, 12.0, 30.25, 12.75),                                               # shorter than a pixel
        (-20.0, -5.0, -3.5, -5.0), (70.0, 3.0, 70.0, 30.0), (3.0, 45.0, 50.0, 45.0),                             # wholly outside
        (2.0, 3.5, 52.0, 3.5), (3.125, 2.0, 3.125, 38.0),                                                        # axis-aligned inside, through holes
        (float("nan"), 1.0, 2.0, 3.0), (1.0, 2.0, float("inf"), 3.0),                                            # not a line at all
    ]
    general = []
    span = [(-8.0, 64.0, -8.0, 48.0)] * 12 + [(1.0, 55.0, 1.0, 39.0)] * 12                                        # crossing borders; inside
    long_ones = [(0.3, 0.4, 55.6, 39.7), (55.2, 0.7, 0.6, 39.1), (-30.1, -20.3, 90.7, 71.9), (0.2, 20.3, 55.9, 21.1)]
    for x0, x1, y0, y1 in span:
        general.append((rng.uniform(x0, x1), rng.uniform(y0, y1), rng.uniform(x0, x1), rng.uniform(y0, y1)))
    general += [tuple(v + rng.uniform(-0.05, 0.05) for v in ln) for ln in long_ones]
    general.append((general[13][0], general[13][1], general[13][0] + 0.31, general[13][1] - 0.27))              # shorter than a pixel
    kept = [g for g in general if grid_distance(g, offset) >= MIN_GRID_DISTANCE and grid_distance(g, offset, 16) >= MIN_GRID_DISTANCE]
    assert len(kept) == len(general), "a random line came within 1e-9 px of a pixel boundary: change the seed"
    rows = fixed + kept
    rows += [(x2, y2, x1, y1) for x1, y1, x2, y2 in kept[:C - len(rows)]]                                        # duplicates reversed
    assert len(rows) == C, len(rows)
    lines[0] = rows
    lines[1, :5] = [(5.0, 5.0, 45.0, 5.0), (45.0, 20.0, 5.0, 20.0), kept[0], (-4.0, 10.5, 60.0, 10.5), (52.875, 0.0, 52.875, 37.0)]
    lines[1, 5:] = rng.uniform(-5, 60, (C - 5, 4))                      # rows from count on: never read
    lines[2] = rng.uniform(-5, 60, (C, 4))
    count = np.array([C, 5, 0], np.int32)
    intrinsics = np.array([(60.0, 62.0, 28.0, 20.0), (50.0, 50.0, 26.5, 18.5), (10.0, 10.0, 4.5, 8.5)], np.float64)
    return {"lines": lines, "count": count, "labels": labels, "depth_mm": depth, "sizes": sizes, "region_map": rmap,
            "intrinsics": intrinsics, "offset": np.float64(offset)}


def make_fixture(path=GOLDEN):
    z = make_inputs()
    for cap in (2048, 16):
        out = line_profiles(z["lines"], z["count"], z["labels"], z["depth_mm"], z["sizes"], None, z["region_map"], z["intrinsics"],
                            float(z["offset"]), cap)
        z.update({"%s_%d" % (k, cap): v for k, v in out.items()})
    np.savez_compressed(path, **z)
    return z


def load_golden(path=GOLDEN):
    """The fixture, with the condition on its inputs asserted: every processed line is exact (axis-aligned in eighths), degenerate,
    or keeps every probe at least 1e-9 px away from a pixel boundary - for both sample caps."""
    z = dict(np.load(path))
    offset = float(z["offset"])
    closest = math.inf
    for b in range(len(z["count"])):
        for r in range(int(z["count"][b])):
            line = z["lines"][b, r]
            if not np.isfinite(line).all() or exact_line(line, offset):
                continue
            closest = min(closest, grid_distance(line, offset, 2048), grid_distance(line, offset, 16))
    assert closest >= MIN_GRID_DISTANCE, closest
    z["closest"] = closest
    return z


if __name__ == "__main__":
    made = make_fixture()
    print("wrote %s (%d bytes); closest probe to a pixel boundary %.3g px" % (GOLDEN, os.path.getsize(GOLDEN), load_golden()["closest"]))
