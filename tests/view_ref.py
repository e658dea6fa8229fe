"""The statement of the scene view (csrc/view.hip, ops.cloud_view, cloud.SceneMap.view) in numpy: a cloud of
32-byte records z-buffered into posed pinhole cameras, plain loops, fp64 with every operation rounded on its own and in the order
written here, one rounding to float32 for the depth.  The kernels, the stand-in library (tests/view_fake.py) and the fixture
tests/golden/scene_view.npz are held to this file."""
import numpy as np

from tests.cloud_ref import HAS_COLOUR, KEEP, POINT, RECORD

EMPTY = np.uint64(0xffffffffffffffff)
MAX_VIEWS = 16
MAX_SPLAT = 64
KEYS = ("view_depth", "view_labels", "view_index", "view_rgb")


def axis_range(c, h, n):
    """The pixels of one axis a splat of half side h around c covers in a frame of n pixels: ceil(c - h) .. ceil(c + h) - 1, clamped
    in fp64 to 0 .. n - 1 -> (first, last) as integers, or None for an empty range; a NaN fails the comparisons."""
    with np.errstate(all="ignore"):
        lo, hi = np.ceil(c - h), np.ceil(c + h) - np.float64(1.0)
    if not lo <= hi:
        return None
    lo = lo if lo > 0.0 else np.float64(0.0)
    hi = hi if hi < np.float64(n - 1) else np.float64(n - 1)
    if not lo <= hi:
        return None
    return int(lo), int(hi)


def half_side(half_footprint, f, Z, cap):
    """max(0.5, min(cap, (half_footprint f) / Z)); None when it is NaN."""
    with np.errstate(all="ignore"):
        h = (half_footprint * f) / Z
    if h != h:
        return None
    h = h if h < cap else cap
    return h if h > 0.5 else np.float64(0.5)


def camera_position(p, pose):
    """World position p (three float32) in the camera of pose = rows [R | t] camera-to-world: R^T (p - t)."""
    p = [np.float64(c) for c in p]
    if pose is None:
        return p
    with np.errstate(all="ignore"):
        d = [p[k] - pose[k, 3] for k in range(3)]
        return [(pose[0, i] * d[0] + pose[1, i] * d[1]) + pose[2, i] * d[2] for i in range(3)]


def splat(row, pose, cam, fh, fw, min_depth, max_depth, footprint, max_splat, keep):
    """One record in one camera -> (depth bits, (x0, x1, y0, y1)) or None."""
    if not int(row["flags"]) & POINT or not np.isfinite(row["xyz"]).all():
        return None
    label = int(row["label"])
    if (keep == "glass" and label != 1) or (keep == "non_glass" and label == 1):
        return None
    X, Y, Z = camera_position(row["xyz"], pose)
    if not (np.isfinite(Z) and min_depth <= Z <= max_depth):
        return None
    fx, fy, cx, cy = (np.float64(c) for c in cam)
    with np.errstate(all="ignore"):
        u, v = (fx * X) / Z + cx, (fy * Y) / Z + cy
        half = np.float64(0.5) * np.float64(footprint)
    cap = np.float64(max_splat) / np.float64(2.0)
    hx, hy = half_side(half, fx, Z, cap), half_side(half, fy, Z, cap)
    if hx is None or hy is None:
        return None
    xs, ys = axis_range(u, hx, fw), axis_range(v, hy, fh)
    if xs is None or ys is None:
        return None
    with np.errstate(over="ignore"):
        bits = int(np.float32(Z).view(np.uint32))
    return bits, xs + ys


def cloud_view(cloud, cloud_offsets, intrinsics, sizes, poses, Fh, Fw, min_depth=1e-3, max_depth=10.0, footprint=0.0, max_splat=32,
               keep="all", ext=None):
    """-> dict(view_depth (V, Fh, Fw) float32, view_labels (V, Fh, Fw) uint8, view_index (V, Fh, Fw) int32, view_rgb (V, Fh, Fw, 3)
    uint8).  ext: None or V pairs the sizes are clamped to (what the host knows of them), next to the plane."""
    intrinsics, sizes = np.asarray(intrinsics, dtype=np.float64), np.asarray(sizes)
    V = len(intrinsics)
    assert keep in KEEP and 1 <= V <= MAX_VIEWS and 1 <= max_splat <= MAX_SPLAT and footprint >= 0.0
    assert 0.0 < min_depth <= max_depth < np.inf and sizes.shape == (V, 2) and intrinsics.shape == (V, 4)
    poses = None if poses is None else np.asarray(poses, dtype=np.float64)
    rows = np.ascontiguousarray(cloud).view(RECORD).ravel()
    total = min(max(int(cloud_offsets[-1]), 0), len(rows))
    zbuf = np.full((V, Fh, Fw), EMPTY, dtype=np.uint64)
    for v in range(V):
        eh, ew = (Fh, Fw) if ext is None else (min(int(ext[v][0]), Fh), min(int(ext[v][1]), Fw))
        fh, fw = min(max(int(sizes[v, 0]), 0), eh), min(max(int(sizes[v, 1]), 0), ew)
        for r in range(total):
            hit = splat(rows[r], None if poses is None else poses[v], intrinsics[v], fh, fw, np.float64(min_depth), np.float64(max_depth),
                        footprint, max_splat, keep)
            if hit is None:
                continue
            bits, (x0, x1, y0, y1) = hit
            key = np.uint64(bits << 32 | r)
            window = zbuf[v, y0:y1 + 1, x0:x1 + 1]
            np.minimum(window, key, out=window)           # a pixel keeps the smallest key drawn on it
    return resolve(zbuf, rows)


def resolve(zbuf, rows):
    """The four planes of a z-buffer of keys."""
    V, Fh, Fw = zbuf.shape
    hit = zbuf != EMPTY
    index = np.where(hit, (zbuf & np.uint64(0xffffffff)).astype(np.int64), -1).astype(np.int32)
    depth = np.where(hit, (zbuf >> np.uint64(32)).astype(np.uint32), 0).astype(np.uint32).view(np.float32)
    labels = np.full((V, Fh, Fw), 255, dtype=np.uint8)
    rgb = np.zeros((V, Fh, Fw, 3), dtype=np.uint8)
    for v, y, x in zip(*np.nonzero(hit)):
        row = rows[index[v, y, x]]
        labels[v, y, x] = row["label"]
        if int(row["flags"]) & HAS_COLOUR:
            rgb[v, y, x] = row["rgb"]
    return {"view_depth": depth, "view_labels": labels, "view_index": index, "view_rgb": rgb}
