"""The seeded scene behind tests/golden/point_cloud.npz and the option grid both point-cloud tests walk.  Three frames in one
(3, 61, 53) plane, noise outside them:

frame 0  61 x 53 = 3233 candidates at stride 1: three full tiles' worth is 3072, so four tiles with a ragged last one.  A tilted plane
         left of x = 30 and a farther one right of it (the depth step the edge rule cuts); rows 0 .. 19 are clean (tile 0 is all
         points); rows 20 .. 37 carry NaN, +-Inf, 0, depths out of range, label 255, a vertical 1-pixel strip (no x neighbour) and a
         horizontal one (no y neighbour); rows 38 .. 57 hold no point at all (tile 2 is empty), one kind of invalid per band; rows
         58 .. 60 are points again.  Pane 1 (rank 0, status 0, the plane its depths were made from), pane 2 (rank 1, status 1), and a
         patch of region value 3 with region_count = 2.
frame 1  17 x 33: one slanted pane over the whole frame with holes.
frame 2  1 x 1: one non-glass pixel."""
import itertools
import os

import numpy as np

from tests import cloud_ref as C

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "point_cloud.npz")
SIZES = ((61, 53), (17, 33), (1, 1))
PLANE = (61, 53)
MIN_DEPTH, MAX_DEPTH = 0.25, 8.0
# the inverse-depth planes w = alpha x + beta y + gamma (1 / m) the scene is made from
W_LEFT = (0.002, 0.001, 0.5)
W_RIGHT = (-0.0005, 0.0015, 0.22)
W_SMALL = (0.004, -0.003, 0.6)
INPUT_KEYS = ("depth", "labels", "sizes", "intrinsics", "region_map", "region_count", "planes", "source", "poses")


def inverse_depth(coef, h, w):
    y, x = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    return (1.0 / ((coef[0] * x + coef[1] * y) + coef[2])).astype(np.float32)


def rotation(axis, angle):
    axis = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def scene():
    rng = np.random.default_rng(28)
    Fh, Fw = PLANE
    depth = rng.uniform(-1.0, 12.0, (3, Fh, Fw)).astype(np.float32)            # noise: some of it a usable depth
    labels = rng.integers(0, 256, (3, Fh, Fw), dtype=np.uint8)
    region_map = rng.integers(0, 6, (3, Fh, Fw), dtype=np.uint8)
    source = rng.integers(0, 4, (3, Fh, Fw), dtype=np.uint8)

    # ---- frame 0
    h, w = SIZES[0]
    d = inverse_depth(W_LEFT, h, w)
    d[:, 30:] = inverse_depth(W_RIGHT, h, w)[:, 30:]
    lab = rng.integers(0, 3, (h, w), dtype=np.uint8) * np.uint8(2)             # 0, 2, 4: not glass
    rmap = np.zeros((h, w), dtype=np.uint8)
    for value, (y0, y1, x0, x1) in ((1, (2, 16, 5, 26)), (2, (2, 11, 35, 46)), (3, (12, 19, 35, 46))):
        rmap[y0:y1, x0:x1] = value
        lab[y0:y1, x0:x1] = 1
    lab[58:, 20:40] = 1                                                         # glass in no region
    # rows 20 .. 37: the single offenders
    d[20, 3], d[20, 9], d[21, 4], d[21, 40], d[22, 7], d[22, 44] = np.nan, np.inf, -np.inf, 0.0, 20.0, 1e-4
    d[23, 45:50] = np.float32(MAX_DEPTH) * np.float32(1.0000001)
    lab[20, 15:18], lab[36, 50:53] = 255, 255
    d[24:31, 10:15] = np.nan
    d[24:31, 12] = inverse_depth(W_LEFT, h, w)[24:31, 12]                       # a vertical strip one pixel wide
    d[32:35, 33:45] = np.inf
    d[33, 35:43] = inverse_depth(W_RIGHT, h, w)[33, 35:43]                      # a horizontal strip one pixel high
    d[29:32, 48:53] = 0.0                                                       # a hole on the right border
    d[35:38, 0:4] = -1.0                                                        # and one on the left
    # rows 38 .. 57: no point, one kind of invalid per band
    d[38:42], d[42:46], d[46:50], d[50:52] = np.nan, np.inf, 0.0, 9.5
    lab[52:58] = 255
    depth[0, :h, :w], labels[0, :h, :w], region_map[0, :h, :w] = d, lab, rmap
    source[0, :h, :w] = np.where(lab == 1, 2, 1)

    # ---- frame 1
    h, w = SIZES[1]
    d = inverse_depth(W_SMALL, h, w)
    d[3, 4], d[9, 20:23], d[16, 0] = np.nan, 0.0, np.inf
    lab = np.ones((h, w), dtype=np.uint8)
    lab[:, 28:] = 0
    lab[5, 5] = 255
    depth[1, :h, :w], labels[1, :h, :w] = d, lab
    region_map[1, :h, :w] = (lab == 1).astype(np.uint8)
    source[1, :h, :w] = 3

    # ---- frame 2
    depth[2, 0, 0], labels[2, 0, 0], region_map[2, 0, 0], source[2, 0, 0] = 1.5, 0, 0, 1

    nan = np.nan
    planes = np.zeros((3, 4, 6), dtype=np.float64)
    planes[0, 0] = W_LEFT + (0.0, 294.0, 0.0)
    planes[0, 1] = (nan, nan, nan, nan, 2.0, 1.0)
    planes[0, 2] = W_RIGHT + (0.0, 77.0, 0.0)                                  # beyond region_count: never used
    planes[1, 0] = W_SMALL + (0.0, 400.0, 0.0)
    frames = [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in SIZES]
    poses = np.stack([np.concatenate([rotation(ax, an), np.asarray(t, dtype=np.float64)[:, None]], axis=1)
                      for ax, an, t in (((1, 2, 3), 0.7, (0.5, -1.0, 2.0)), ((0, 1, 0), -1.1, (3.0, 0.0, 0.25)), ((1, 0, 0), 0.2, (0.0, 0.0, 0.0)))])
    return dict(depth=depth, labels=labels, sizes=np.asarray(SIZES, dtype=np.int32),
                intrinsics=np.array([(60.5, 61.25, 26.3, 30.1), (40.0, 39.5, 16.0, 8.5), (10.0, 10.0, 0.5, 0.5)], dtype=np.float64),
                region_map=region_map, region_count=np.array([2, 1, 0], dtype=np.int32), planes=planes, source=source, poses=poses,
                frames=frames)


def arrays(sc):
    out = {k: sc[k] for k in INPUT_KEYS}
    out.update({"frame%d" % b: f for b, f in enumerate(sc["frames"])})
    return out


def load_golden():
    gold = dict(np.load(GOLDEN))
    gold["frames"] = [gold.pop("frame%d" % b) for b in range(len(SIZES))]
    return gold


# stride x edge x keep x (frames, poses, normals): 3 x 2 x 3 x 8 = 144 calls
GRID = [dict(stride=s, edge=e, keep=k, frames=f, poses=p, normals=n)
        for s, e, k, (f, p, n) in itertools.product((1, 2, 3), (None, 0.05), C.KEEP, itertools.product((False, True), repeat=3))]
RECORDED = (dict(stride=1, edge=None, keep="all", frames=True, poses=True, normals=True),
            dict(stride=3, edge=0.05, keep="glass", frames=False, poses=False, normals=True))


def config_id(cfg):
    return "s%d-e%s-%s-%s" % (cfg["stride"], cfg["edge"], cfg["keep"],
                              "".join(c for c, on in zip("fpn", (cfg["frames"], cfg["poses"], cfg["normals"])) if on) or "bare")


def statement(sc, cfg, **kw):
    """The statement's cloud of the scene under one configuration of the grid."""
    return C.point_cloud(sc["depth"], sc["labels"], sc["sizes"], sc["intrinsics"], frames=sc["frames"] if cfg["frames"] else None,
                         region_map=sc["region_map"], region_count=sc["region_count"], planes=sc["planes"], source=sc["source"],
                         poses=sc["poses"] if cfg["poses"] else None, stride=cfg["stride"], min_depth=MIN_DEPTH, max_depth=MAX_DEPTH,
                         edge=cfg["edge"], normals=cfg["normals"], keep=cfg["keep"], **kw)
