"""The numpy / scipy restatement of csrc/fusion.hip (include/gwdepth.h: gwd_fusion_ring, gwd_fusion_planes, gwd_fusion_depth), stage
by stage as DESIGN.md section 26 defines them: the ring map from separable running minima / maxima, the frame plane of every kept
region by numpy.linalg.lstsq on centred columns (tests/regions_ref.py), the trim against STORED first coefficients, the scale from
exact Python integers and the fused depth - plus the seeded inputs the tests run on.  Every function takes `first=` where the GPU
tests hand in the kernel's own first-pass coefficients, so that the trim decision is compared bit for bit."""
import numpy as np

from tests import regions_ref as R

SENSOR, PLANE, NETWORK = 1, 2, 3
PLANE_FIELDS = ("alpha1", "beta1", "gamma1", "rms1", "n1", "alpha", "beta", "gamma", "rms", "n_used", "status", "spare")


def _window(a, radius, op, fill):
    """op over the Chebyshev window of `radius` in a 2-D array, separably: rows, then columns; outside the array `fill`."""
    h, w = a.shape
    p = np.full((h, w + 2 * radius), fill, a.dtype)
    p[:, radius:radius + w] = a
    rows = op.reduce(np.stack([p[:, d:d + w] for d in range(2 * radius + 1)]), axis=0)
    q = np.full((h + 2 * radius, w), fill, a.dtype)
    q[radius:radius + h] = rows
    return op.reduce(np.stack([q[d:d + h] for d in range(2 * radius + 1)]), axis=0)


def ring_map(labels, sensor_mm, region_map, K, ring=6, gap=1, lo_mm=1, hi_mm=10000):
    """One FRAME (the arrays cut to (fh, fw)) -> (ring uint8: r + 1 on the ring of rank r, near_glass bool)."""
    rank = region_map.astype(np.uint8).copy()
    rank[(rank < 1) | (rank > K)] = 255                                # 0 -> 255: the minimum then skips `no region`
    best = _window(rank, ring, np.minimum, 255)
    near = _window((labels == 1).astype(np.uint8), gap, np.maximum, 0).astype(bool)
    valid = (sensor_mm >= lo_mm) & (sensor_mm <= hi_mm)
    take = (labels != 1) & valid & ~near & (best != 255)
    return np.where(take, best, 0).astype(np.uint8), near


def ring_samples(ring, sensor_mm, r):
    """(x, y, w) of the ring pixels of rank r in one frame, raster order; w = 1000 / mm in fp64."""
    ys, xs = np.nonzero(ring == r + 1)
    return xs.astype(np.int64), ys.astype(np.int64), 1000.0 / sensor_mm[ys, xs].astype(np.float64)


def residual(x, y, w, a, b, g):
    """w - ((a x + b y) + g), every operation rounded on its own (numpy does not contract)."""
    return w - ((a * x.astype(np.float64) + b * y.astype(np.float64)) + g)


def trim_keep(x, y, w, first, trim):
    """The samples a second fit keeps, against stored first coefficients (alpha1, beta1, gamma1, rms1); -> (keep bool, e^2, thr)."""
    e = residual(x, y, w, first[0], first[1], first[2])
    t = trim * first[3]
    return e * e <= t * t, e * e, t * t


def fit_region(x, y, w, trim=2.5, min_ring=50, max_rms=None, first=None):
    """-> the 12 fields of a fusion plane.  first=(alpha1, beta1, gamma1, rms1): decide the trim with these stored values."""
    nan = np.nan
    a1, b1, g1, rms1, n1, st1 = R.fit_plane(x, y, w)
    row = [a1, b1, g1, rms1, n1, nan, nan, nan, nan, n1, st1, 0.0]
    if st1:
        return np.array(row)
    stored = (a1, b1, g1, rms1) if first is None else tuple(float(v) for v in first)
    if trim > 0 and stored[3] > 0:
        keep, _, _ = trim_keep(x, y, w, stored, trim)
        a, b, g, rms, n, st = R.fit_plane(x[keep], y[keep], w[keep])
        row[5:11] = [a, b, g, rms, n, st]
    else:
        row[5:9] = row[0:4]
    if row[10] == 0.0 and (row[9] < min_ring or (max_rms is not None and row[8] > max_rms)):
        row[10] = 2.0
    return np.array(row)


def scale_sums(labels, sensor_mm, depth_mm, near, lo_mm=1, hi_mm=10000):
    """One frame -> (n, sum sensor * network, sum network^2) as Python integers."""
    s, p = sensor_mm.astype(np.int64), depth_mm.astype(np.int64)
    ok = (labels != 1) & ~near & (s >= lo_mm) & (s <= hi_mm) & (p >= lo_mm) & (p <= hi_mm)
    return int(ok.sum()), sum(int(v) for v in (s[ok] * p[ok])), sum(int(v) for v in (p[ok] * p[ok]))


def scale_of(n, sp, pp, align=True, min_align=1000):
    """The fp64 quotient of the two integers, each converted to fp64 first (as the kernel forms it)."""
    return float(sp) / float(pp) if align and n >= min_align and pp > 0 else 1.0


def fused_depth(labels, sensor_mm, depth, region_map, K, planes, s, lo_mm=1, hi_mm=10000, min_depth=1e-3, max_depth=10.0):
    """One frame -> (depth_fused fp32, depth_fused_mm uint16, fused_source uint8, z fp64 before the rounding of PLANE / NETWORK)."""
    h, w = labels.shape
    lo, hi = float(np.float32(min_depth)), float(np.float32(max_depth))
    out, out_mm, src = np.zeros((h, w), np.float32), np.zeros((h, w), np.uint16), np.full((h, w), NETWORK, np.uint8)
    z = np.clip(depth.astype(np.float64) * float(s), lo, hi)
    live = np.zeros((planes.shape[0], 6))
    live[:, :3], live[:, 5] = planes[:, 5:8], 1.0
    live[:K, 5] = (planes[:K, 10] != 0.0).astype(np.float64)
    den = R.plane_denominator(live, np.where(region_map <= K, region_map, 0))
    on_plane = den > 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        z[on_plane] = np.clip(1.0 / den[on_plane], lo, hi)
    src[on_plane] = PLANE
    out[:] = z.astype(np.float32)
    out_mm[:] = R.to_mm(out)
    sens = (labels != 1) & (sensor_mm >= lo_mm) & (sensor_mm <= hi_mm)
    out[sens] = sensor_mm[sens].astype(np.float32) / np.float32(1000.0)
    out_mm[sens] = sensor_mm[sens]
    src[sens] = SENSOR
    z[sens] = 0.0
    return out, out_mm, src, z


def sensor_fusion(sensor_mm, labels, depth, depth_mm, sizes, region_map, region_count, max_regions, ring=6, gap=1, trim=2.5,
                  min_ring=50, max_rms=None, align=True, min_align=1000, lo_mm=1, hi_mm=10000, min_depth=1e-3, max_depth=10.0,
                  first=None, use_planes=None, use_scale=None):
    """The whole operation on a batch -> dict of FUSION_KEYS plus "z" (fp64 before rounding).  first: (B, R, >= 4) stored first
    fits for the trim decision; use_planes / use_scale: evaluate the fused depth with these (the kernel's own) values."""
    B, Fh, Fw = labels.shape
    out = {"depth_fused": np.zeros((B, Fh, Fw), np.float32), "depth_fused_mm": np.zeros((B, Fh, Fw), np.uint16),
           "fused_source": np.zeros((B, Fh, Fw), np.uint8), "fusion_ring": np.zeros((B, Fh, Fw), np.uint8),
           "fusion_planes": np.zeros((B, max_regions, 12)), "fusion_scale": np.zeros((B, 4)), "z": np.zeros((B, Fh, Fw))}
    for b in range(B):
        fh, fw = (int(v) for v in sizes[b])
        cut = (b, slice(0, fh), slice(0, fw))
        K = min(max(int(region_count[b]), 0), max_regions)
        ring_b, near = ring_map(labels[cut], sensor_mm[cut], region_map[cut], K, ring, gap, lo_mm, hi_mm)
        out["fusion_ring"][cut] = ring_b
        for r in range(K):
            out["fusion_planes"][b, r] = fit_region(*ring_samples(ring_b, sensor_mm[cut], r), trim=trim, min_ring=min_ring,
                                                    max_rms=max_rms, first=None if first is None else first[b, r, :4])
        n, sp, pp = scale_sums(labels[cut], sensor_mm[cut], depth_mm[cut], near, lo_mm, hi_mm)
        out["fusion_scale"][b] = (scale_of(n, sp, pp, align, min_align), n, sp, pp)
        planes = out["fusion_planes"][b] if use_planes is None else use_planes[b]
        s = out["fusion_scale"][b, 0] if use_scale is None else use_scale[b, 0]
        d, mm, src, z = fused_depth(labels[cut], sensor_mm[cut], depth[cut], region_map[cut], K, planes, s, lo_mm, hi_mm, min_depth, max_depth)
        out["depth_fused"][cut], out["depth_fused_mm"][cut], out["fused_source"][cut], out["z"][cut] = d, mm, src, z
    return out


# ---------------------------------------------------------------------------------------------------- inputs
def sensor_for(mask, seed, holes=0.03, outliers=0.05, ring=6):
    """A seeded sensor plane (uint16 mm) and network depth (fp32 m, uint16 mm) for a glass mask: the scene is a slanted wall in
    inverse depth; inside the glass the sensor reads a wall 1.6 times farther; `outliers` of the pixels within `ring` of the
    glass read twice the depth, `holes` of all pixels read 0; the network's depth is the scene times 1.1 with 1 % noise."""
    rng = np.random.default_rng(seed)
    h, w = mask.shape
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    inv = 0.6 + 0.15 * xs / max(w, 1) - 0.1 * ys / max(h, 1)
    true_mm = 1000.0 / inv
    sensor = np.where(mask, 1.6 * true_mm, true_mm)
    near = _window(mask.astype(np.uint8), ring, np.maximum, 0).astype(bool) & ~mask
    sensor = np.where(near & (rng.random((h, w)) < outliers), 2.0 * sensor, sensor)
    sensor = np.where(rng.random((h, w)) < holes, 0.0, sensor)
    sensor_mm = np.clip(np.rint(sensor), 0, 65535).astype(np.uint16)
    depth = (true_mm / 1000.0 * 1.1 * (1.0 + 0.01 * rng.standard_normal((h, w)))).astype(np.float32)
    return sensor_mm, depth, R.to_mm(depth)


def batch_of(items, Fh=None, Fw=None, rng=None):
    """[(mask, sensor_mm, depth, depth_mm)] -> labels, sensor, depth, depth_mm (B, Fh, Fw), sizes; outside a frame label 255 and
    zeros, or random bytes in every plane with rng."""
    Fh = Fh or max(i[0].shape[0] for i in items)
    Fw = Fw or max(i[0].shape[1] for i in items)
    B = len(items)
    if rng is None:
        labels = np.full((B, Fh, Fw), 255, np.uint8)
        sensor, depth_mm = np.zeros((B, Fh, Fw), np.uint16), np.zeros((B, Fh, Fw), np.uint16)
        depth = np.zeros((B, Fh, Fw), np.float32)
    else:
        labels = rng.integers(0, 256, (B, Fh, Fw), dtype=np.uint8)
        sensor = rng.integers(0, 65536, (B, Fh, Fw), dtype=np.uint16)
        depth_mm = rng.integers(0, 65536, (B, Fh, Fw), dtype=np.uint16)
        depth = rng.integers(0, 2 ** 31, (B, Fh, Fw), dtype=np.int64).astype(np.uint32).view(np.float32)
    sizes = np.zeros((B, 2), np.int32)
    for b, (m, s, d, dmm) in enumerate(items):
        h, w = m.shape
        labels[b, :h, :w], sensor[b, :h, :w], depth[b, :h, :w], depth_mm[b, :h, :w] = m.astype(np.uint8), s, d, dmm
        sizes[b] = (h, w)
    return labels, sensor, depth, depth_mm, sizes


def masks_for(h, w):
    """The masks the ring passes go wrong on, h x w each (h >= 20, w >= 40): name -> bool array."""
    out = {}
    m = np.zeros((h, w), bool)                                 # touches all four borders: a cross
    m[h // 2 - 3:h // 2 + 3, :] = True
    m[:, w // 2 - 3:w // 2 + 3] = True
    out["cross"] = m
    out["full"] = np.ones((h, w), bool)                        # no ring: status 1, NETWORK everywhere
    m = np.zeros((h, w), bool)                                 # two panes 5 columns apart: closer than 2 ring for ring >= 3
    m[4:h - 6, 5:w // 2 - 2] = True
    m[8:h - 4, w // 2 + 3:w - 4] = True
    out["pair"] = m
    m = np.zeros((h, w), bool)                                 # one pane in the middle, far from the borders at ring 6
    m[h // 4:3 * h // 4, w // 4:3 * w // 4] = True
    out["pane"] = m
    out["empty"] = np.zeros((h, w), bool)
    return out


# ---------------------------------------------------------------------------------------------------- the recovery scene
def recovery_scene(seed=5, h=120, w=160):
    """Two panes on known 3-D planes in a room (pinhole fx = fy = 140, centre of the frame): -> dict(mask, truth (m, fp64: the
    panes where there is glass, the room elsewhere), sensor_mm (the wall behind the panes inside the glass, the truth quantised to
    millimetres elsewhere, 5 % of the pixels within 6 of the glass at twice the depth, 3 % holes), depth / depth_mm (the network:
    the truth times 1.15 with 2 % noise - unscaled it is off by the factor)."""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    fx = fy = 140.0
    u, v = (xs - w / 2) / fx, (ys - h / 2) / fy
    plane_inv = lambda n, d: (n[0] * u + n[1] * v + n[2]) / d          # 1 / Z of the plane n . P = d along every pixel's ray
    wall = 1.0 / plane_inv((0.1, 0.0, 1.0), 4.0)
    mask = np.zeros((h, w), bool)
    truth = wall.copy()
    for (y0, y1, x0, x1), n, d in (((20, 95, 15, 70), (0.35, 0.05, 1.0), 2.0), ((30, 100, 95, 150), (-0.3, 0.1, 1.0), 2.6)):
        mask[y0:y1, x0:x1] = True
        truth[y0:y1, x0:x1] = (1.0 / plane_inv(n, d))[y0:y1, x0:x1]
    room = wall.copy()                                         # what surrounds a pane lies ON the pane's plane: its frame
    for (y0, y1, x0, x1), n, d in (((20, 95, 15, 70), (0.35, 0.05, 1.0), 2.0), ((30, 100, 95, 150), (-0.3, 0.1, 1.0), 2.6)):
        fy0, fy1, fx0, fx1 = y0 - 8, y1 + 8, x0 - 8, x1 + 8
        room[fy0:fy1, fx0:fx1] = (1.0 / plane_inv(n, d))[fy0:fy1, fx0:fx1]
    truth[~mask] = room[~mask]
    sensor = np.where(mask, wall, room) * 1000.0
    near = _window(mask.astype(np.uint8), 6, np.maximum, 0).astype(bool) & ~mask
    sensor = np.where(near & (rng.random((h, w)) < 0.05), 2.0 * sensor, sensor)
    sensor = np.where(rng.random((h, w)) < 0.03, 0.0, sensor)
    depth = (truth * 1.15 * (1.0 + 0.02 * rng.standard_normal((h, w)))).astype(np.float32)
    return dict(mask=mask, truth=truth, sensor_mm=np.clip(np.rint(sensor), 0, 65535).astype(np.uint16), depth=depth,
                depth_mm=R.to_mm(depth))


def fit_from_moments(x, y, w, summer, ox, oy):
    """The kernel's route (csrc/planefit.h) - ten moments relative to the origin (ox, oy) = (max(x0 - ring, 0), max(y0 - ring, 0)) of
    the region's box, the centred 2 x 2 system, gamma from the means, shifted back - with the summation left to `summer`."""
    dx, dy = (x - ox).astype(np.float64), (y - oy).astype(np.float64)
    assert (x >= ox).all() and (y >= oy).all()                 # the exactness argument: relative coordinates never negative
    n = float(len(x))
    Sx, Sy, Sxx, Sxy, Syy = (float(int(v.sum())) for v in ((x - ox), (y - oy), (x - ox) ** 2, (x - ox) * (y - oy), (y - oy) ** 2))
    Sw, Sxw, Syw = summer(w), summer(dx * w), summer(dy * w)
    dxx, dyy, dxy = n * Sxx - Sx * Sx, n * Syy - Sy * Sy, n * Sxy - Sx * Sy
    dxw, dyw = n * Sxw - Sx * Sw, n * Syw - Sy * Sw
    det = dxx * dyy - dxy * dxy
    alpha, beta = (dyy * dxw - dxy * dyw) / det, (dxx * dyw - dxy * dxw) / det
    gamma = (Sw - alpha * Sx - beta * Sy) / n - alpha * ox - beta * oy
    return alpha, beta, gamma


# ---------------------------------------------------------------------------------------------------- the GPU test's inputs
SHAPES = ((37, 53), (64, 70), (65, 129), (40, 300))           # (40, 300): wider than a 256-column tile, taller than 16 rows, + halo at ring 6
WIDE = ((20, 1284), (20, 301))                                # a second workgroup along x of the fused pass: 4 pixels per thread (1024 columns), 1 (256)
RINGS = ((1, 0), (6, 0), (6, 5), (32, 0), (32, 31))           # (ring, gap)


def hand_case(h, w):
    """cross, full, pair, pane, empty at h x w as one batch with a seeded sensor each -> (labels, sensor, depth, depth_mm, sizes)."""
    masks = masks_for(h, w)
    return batch_of([(masks[n],) + sensor_for(masks[n], 20 + k) for k, n in enumerate(masks)])


def golden_case(name):
    """One 300 x 500 mask of tests/golden/glass_regions.npz with a seeded sensor plane; the network's millimetres are the fixture's."""
    at = [g[0] for g in R.load_golden()].index(name)
    _, mask, mm = R.load_golden()[at]
    sensor, depth, _ = sensor_for(mask, 40 + at)
    depth = (mm.astype(np.float32) / np.float32(1000.0)) * np.float32(1.03125)
    return batch_of([(mask, sensor, depth, mm)])


def regions_of(labels, depth_mm, sizes, **kw):
    """The oracle's glass regions for a case (what ops.glass_regions gives on the device) -> region_map, region_count, regions."""
    out = R.glass_regions(labels, depth_mm, sizes, kw.get("max_regions", 32), kw.get("min_area", 1), 8, 1, 10000, kw.get("max_candidates", 8192))
    return out["region_map"], out["region_count"], out["regions"]
