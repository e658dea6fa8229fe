"""The statement of ops.point_cloud (csrc/cloud.hip) in numpy: fp64 throughout, every operation rounded on its
own and in the order written here, one rounding to float32 at the end.  The kernel, the stand-in library and the fixture
tests/golden/point_cloud.npz are held to this file."""
import numpy as np

RECORD = np.dtype([("xyz", "<f4", 3), ("normal", "<f4", 3), ("rgb", "u1", 3), ("label", "u1"), ("region", "u1"), ("source", "u1"),
                   ("frame", "u1"), ("flags", "u1")])
assert RECORD.itemsize == 32
POINT, HAS_NORMAL, PANE_NORMAL, HAS_COLOUR = 1, 2, 4, 8
KEEP = ("all", "glass", "non_glass")


def capacity(B, Fh, Fw, stride):
    """The default capacity: B planes of the stride lattice."""
    return B * -(-Fh // stride) * -(-Fw // stride)


def usable(z, min_depth, max_depth):
    """A depth that is finite and in range (z: fp64)."""
    with np.errstate(invalid="ignore"):
        return np.isfinite(z) & (z >= min_depth) & (z <= max_depth)


def unproject(x, y, z, cam):
    """Camera-frame positions (..., 3) of pixels (x, y) at depth z; cam = (fx, fy, cx, cy)."""
    fx, fy, cx, cy = (float(v) for v in cam)
    with np.errstate(all="ignore"):
        X, Y, Z = np.broadcast_arrays(((x - cx) * z) / fx, ((y - cy) * z) / fy, z)
    return np.stack([X, Y, Z], axis=-1)


def pane_normal(plane, cam):
    """The camera-facing unit normal of a pane from its plane in inverse depth (alpha, beta, gamma, ...), or None."""
    fx, fy, cx, cy = (float(v) for v in cam)
    alpha, beta, gamma = (float(v) for v in plane[:3])
    with np.errstate(all="ignore"):
        m = np.array([alpha * fx, beta * fy, (gamma + alpha * cx) + beta * cy], dtype=np.float64)
        length = np.sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2])
    if not (np.isfinite(length) and length > 0.0):
        return None
    return -(m / length)


def _axis_difference(P, ok, axis):
    """Per pixel the difference of the positions of its 1-pixel neighbours along `axis`: central where both are usable, else the
    one-sided one that exists; -> (difference (h, w, 3), exists (h, w))."""
    h, w = ok.shape
    pad = [(0, 0), (0, 0)]
    pad[axis] = (1, 1)
    okp = np.pad(ok, pad, constant_values=False)
    Pp = np.pad(P, pad + [(0, 0)], constant_values=0.0)
    sl = lambda k: (slice(k, k + h), slice(None)) if axis == 0 else (slice(None), slice(k, k + w))
    um, up = okp[sl(0)], okp[sl(2)]
    hi = np.where(up[..., None], Pp[sl(2)], P)
    lo = np.where(um[..., None], Pp[sl(0)], P)
    with np.errstate(all="ignore"):
        return hi - lo, um | up


def frame_normals(P, ok):
    """The difference normals of one frame: P (h, w, 3) camera positions, ok (h, w) usable depth -> (normals, has)."""
    dx, ex = _axis_difference(P, ok, 1)
    dy, ey = _axis_difference(P, ok, 0)
    with np.errstate(all="ignore"):
        v = np.stack([dx[..., 1] * dy[..., 2] - dx[..., 2] * dy[..., 1],
                      dx[..., 2] * dy[..., 0] - dx[..., 0] * dy[..., 2],
                      dx[..., 0] * dy[..., 1] - dx[..., 1] * dy[..., 0]], axis=-1)
        length = np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])
        has = ex & ey & np.isfinite(length) & (length > 0.0)
        n = v / np.where(has, length, 1.0)[..., None]
        flip = (n[..., 0] * P[..., 0] + n[..., 1] * P[..., 1]) + n[..., 2] * P[..., 2] > 0.0
    n = np.where(flip[..., None], -n, n)
    return np.where(has[..., None], n, 0.0), has


def rotate(M, v, translate):
    """Rows [R | t] (3, 4) applied to vectors (n, 3)."""
    out = np.empty_like(v)
    with np.errstate(all="ignore"):
        for i in range(3):
            out[:, i] = (M[i, 0] * v[:, 0] + M[i, 1] * v[:, 1]) + M[i, 2] * v[:, 2]
            if translate:
                out[:, i] = out[:, i] + M[i, 3]
    return out


def frame_points(b, depth, labels, size, cam, frame=None, region_map=None, region_count=0, planes=None, source=None, pose=None, stride=1,
                 min_depth=1e-3, max_depth=10.0, edge=None, normals=True, keep="all"):
    """The records of one frame, in raster order: depth / labels / region_map / source are the frame's PLANES (any size >= the frame)."""
    assert keep in KEEP and 1 <= stride <= 16
    fh, fw = int(size[0]), int(size[1])
    s = int(stride)
    z = depth[:fh, :fw].astype(np.float64)
    lab = labels[:fh, :fw]
    ok = usable(z, min_depth, max_depth)
    valid = ok & (lab != 255)
    if keep == "glass":
        valid &= lab == 1
    elif keep == "non_glass":
        valid &= lab != 1
    lattice = np.zeros((fh, fw), dtype=bool)
    lattice[::s, ::s] = True
    valid &= lattice
    if edge is not None:
        e = float(edge)
        for dy, dx in ((0, -s), (0, s), (-s, 0), (s, 0)):
            zn = np.full((fh, fw), np.nan)
            y0, y1, x0, x1 = max(0, -dy), min(fh, fh - dy), max(0, -dx), min(fw, fw - dx)
            if y1 > y0 and x1 > x0:
                zn[y0:y1, x0:x1] = z[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
            with np.errstate(invalid="ignore"):
                valid &= ~(usable(zn, min_depth, max_depth) & ~(np.abs(zn - z) <= e * np.minimum(zn, z)))
    ys, xs = np.nonzero(valid)                            # raster order
    out = np.zeros(len(ys), dtype=RECORD)
    if len(ys) == 0:
        return out
    yy, xx = np.meshgrid(np.arange(fh, dtype=np.float64), np.arange(fw, dtype=np.float64), indexing="ij")
    P = unproject(xx, yy, z, cam)
    pos = P[ys, xs]
    flags = np.full(len(ys), POINT, dtype=np.uint8)
    nrm, has = np.zeros((len(ys), 3), dtype=np.float64), np.zeros(len(ys), dtype=bool)
    region = region_map[:fh, :fw][ys, xs] if region_map is not None else np.zeros(len(ys), dtype=np.uint8)
    if normals:
        n_all, has_all = frame_normals(P, ok)
        nrm, has = n_all[ys, xs].copy(), has_all[ys, xs].copy()
        if region_map is not None:
            for r in range(min(max(int(region_count), 0), planes.shape[0])):
                if planes[r, 5] != 0.0:
                    continue
                n = pane_normal(planes[r], cam)
                if n is None:
                    continue
                sel = region == r + 1
                nrm[sel], has[sel] = n, True
                flags[sel] |= PANE_NORMAL
        flags[has] |= HAS_NORMAL
    if pose is not None:
        M = np.asarray(pose, dtype=np.float64)
        pos = rotate(M, pos, True)
        nrm[has] = rotate(M, nrm[has], False)            # decided in the camera frame, then rotated
    with np.errstate(all="ignore"):
        out["xyz"], out["normal"] = pos.astype(np.float32), nrm.astype(np.float32)
    if frame is not None:
        out["rgb"] = frame[ys, xs]
        flags |= HAS_COLOUR
    out["label"], out["region"], out["frame"], out["flags"] = lab[ys, xs], region, b, flags
    if source is not None:
        out["source"] = source[:fh, :fw][ys, xs]
    return out


def point_cloud(depth, labels, sizes, intrinsics, frames=None, region_map=None, region_count=None, planes=None, source=None, poses=None,
                stride=1, min_depth=1e-3, max_depth=10.0, edge=None, normals=True, keep="all", capacity_rows=None):
    """-> dict(cloud (capacity, 32) uint8, cloud_offsets (B + 1,) int32): the frames in order of b, every row behind the total zero."""
    B, Fh, Fw = depth.shape
    rows = capacity(B, Fh, Fw, stride) if capacity_rows is None else int(capacity_rows)
    parts = [frame_points(b, depth[b], labels[b], sizes[b], intrinsics[b], None if frames is None else frames[b],
                          None if region_map is None else region_map[b], 0 if region_count is None else region_count[b],
                          None if planes is None else planes[b], None if source is None else source[b],
                          None if poses is None else poses[b], stride, min_depth, max_depth, edge, normals, keep) for b in range(B)]
    offsets = np.zeros(B + 1, dtype=np.int32)
    offsets[1:] = np.cumsum([len(p) for p in parts])
    if offsets[B] > rows:
        raise ValueError("point_cloud: %d points do not fit a capacity of %d rows" % (offsets[B], rows))
    cloud = np.zeros(rows, dtype=RECORD)
    cloud[:offsets[B]] = np.concatenate(parts)
    return {"cloud": cloud.view(np.uint8).reshape(rows, 32), "cloud_offsets": offsets}
