"""The inputs both scene-view tests walk: the clouds and the four-part map of the point-cloud fixture with the cameras they were
made from, the arithmetic edges as named cases with results written out by hand, and the small shapes at which the kernels can still
go wrong."""
import os

import numpy as np

from tests import cloud_cases as CK
from tests import cloud_ref as C
from tests import scene_cases as SK
from tests import scene_ref as S
from tests import view_ref as W

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scene_view.npz")
VOXELS = (0.05, 0.25)
MAP_SPLAT = 8
DEPTHS = dict(min_depth=CK.MIN_DEPTH, max_depth=CK.MAX_DEPTH)
# a rotation whose transpose differs from itself (a quarter turn about z) with a translation; rows [R | t], camera-to-world
TURN = [[0.0, -1.0, 0.0, 1.0], [1.0, 0.0, 0.0, 2.0], [0.0, 0.0, 1.0, 3.0]]
IDENTITY = [[1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0]]
UNIT_CAM = (1.0, 1.0, 0.0, 0.0)                           # u = X / Z, v = Y / Z


def same(a, b, what=""):
    for k in W.KEYS:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, (what, k, a[k].shape, b[k].shape, a[k].dtype, b[k].dtype)
        if a[k].tobytes() != b[k].tobytes():
            bad = np.argwhere(a[k].view(np.uint32 if a[k].dtype == np.float32 else a[k].dtype) !=
                              b[k].view(np.uint32 if b[k].dtype == np.float32 else b[k].dtype))
            raise AssertionError("%s: %s differs at %d places, first %s" % (what, k, len(bad), bad[:5].tolist()))


_CACHE = {}


def fixture_cameras():
    """-> (intrinsics (4, 4), poses (4, 3, 4), sizes (4, 2)): the fixture's three cameras and the first again, moved by RESHOT."""
    gold = CK.load_golden()
    poses = np.concatenate([gold["poses"], gold["poses"][:1]])
    poses[3, :, 3] += SK.RESHOT
    return (np.concatenate([gold["intrinsics"], gold["intrinsics"][:1]]), poses,
            np.concatenate([gold["sizes"], gold["sizes"][:1]]).astype(np.int32))


def fixture_map(voxel):
    """The statement's extraction of the fixture's four-part map (tests/scene_cases.py)."""
    if ("map", voxel) not in _CACHE:
        _CACHE["map", voxel] = S.merge(SK.fixture_clouds()[1], voxel, SK.FIXTURE_MAX_VOXELS)
    return _CACHE["map", voxel]


def fixture_map_view(voxel):
    """The statement's view of that map from the four cameras, footprint = voxel, at most MAP_SPLAT pixels.  Made once."""
    if ("view", voxel) not in _CACHE:
        ext = fixture_map(voxel)
        cams, poses, sizes = fixture_cameras()
        _CACHE["view", voxel] = W.cloud_view(ext["cloud"], ext["cloud_offsets"], cams, sizes, poses, *CK.PLANE, footprint=voxel,
                                             max_splat=MAP_SPLAT, **DEPTHS)
    return _CACHE["view", voxel]


def fixture_whole_view():
    """The statement's view of the 4702-row fixture cloud from the four cameras, one pixel per row.  Made once."""
    if "whole" not in _CACHE:
        whole, _ = SK.fixture_clouds()
        cams, poses, sizes = fixture_cameras()
        _CACHE["whole"] = W.cloud_view(whole[0], whole[1], cams, sizes, poses, *CK.PLANE, **DEPTHS)
    return _CACHE["whole"]


def golden_id(voxel):
    return "v%s" % voxel


def load_golden():
    return dict(np.load(GOLDEN))


# ---- the arithmetic edges.  Every case: points (tests/scene_cases.rows), the cameras (default: one, UNIT_CAM, no pose, the whole
# 8 x 8 plane), the options, and `want`: the covered pixels as (view, x, y, row, depth), written out by hand; every other pixel is
# empty.  All numbers are exact in float32 and fp64: powers of two and small integers.
P = lambda x, y, z, **kw: dict(xyz=(x, y, z), **kw)
SQUARE = lambda v, xs, ys, row, depth: [(v, x, y, row, depth) for y in ys for x in xs]
EDGE_PLANE = (8, 8)
EDGES = {
    # u = 3, hx = 1: u - hx = 2 is an integer, pixel 2 is in; u + hx = 4 is out.  v = 2: rows 1 and 2
    "integer_edge": dict(points=[P(3.0, 2.0, 1.0)], options=dict(footprint=2.0), want=SQUARE(0, (2, 3), (1, 2), 0, 1.0)),
    # footprint 0 is the half-open unit square [u - 0.5, u + 0.5): u = 2.5 covers 2 <= x < 3, v = 3.25 covers 2.75 <= y < 3.75
    "half_pixel": dict(points=[P(2.5, 3.25, 1.0), P(5.5, 6.5, 1.0)], want=[(0, 2, 3, 0, 1.0), (0, 5, 6, 1, 1.0)]),
    # Z = p_z - t_z.  View 0: 0.5 and 4 lie ON the bounds and are kept.  View 1, t_z = 2^-54: 0.5 - 2^-54 is the fp64 below 0.5 - out;
    # 4 - 2^-54 rounds to 4 - in.  View 2, t_z = -2^-50: 0.5 + 2^-50 - in, at u = 1 / Z just below 2: still pixel 2; 4 + 2^-50 - out
    "depth_bounds": dict(points=[P(1.0, 0.5, 0.5), P(12.0, 8.0, 4.0)], cams=[UNIT_CAM] * 3,
                         poses=[IDENTITY, [r[:3] + [t] for r, t in zip(IDENTITY, (0.0, 0.0, 2.0 ** -54))],
                                [r[:3] + [t] for r, t in zip(IDENTITY, (0.0, 0.0, -2.0 ** -50))]],
                         options=dict(min_depth=0.5, max_depth=4.0),
                         want=[(0, 2, 1, 0, 0.5), (0, 3, 2, 1, 4.0), (1, 3, 2, 1, 4.0), (2, 2, 1, 0, 0.5)]),
    # nothing but the last row is drawn: Z = 0, Z < 0, NaN, Inf, no flag 1 (one of them with other flags)
    "undrawn": dict(points=[P(0.0, 0.0, 0.0), P(1.0, 1.0, -1.0), P(np.nan, 1.0, 1.0), P(1.0, np.nan, 1.0), P(1.0, 1.0, np.nan),
                            P(np.inf, 1.0, 1.0), P(1.0, -np.inf, 1.0), P(1.0, 1.0, np.inf), P(2.0, 2.0, 1.0, flags=0),
                            P(2.0, 2.0, 1.0, flags=2 | 8), P(6.0, 10.0, 2.0)],
                    want=[(0, 3, 5, 10, 2.0)]),
    # the total is 1: row 1 carries flag 1 and lies behind it
    "behind_total": dict(points=[P(1.0, 1.0, 1.0), P(2.0, 2.0, 1.0)], total=1, want=[(0, 1, 1, 0, 1.0)]),
    # Z = p_z + 1024: 1025 + 2^-23 (row 0) and 1025 (row 1) differ in fp64 and share the float32 1025: the lower row wins
    "same_float32": dict(points=[P(0.0, 0.0, 1.0 + 2.0 ** -23), P(0.0, 0.0, 1.0)],
                         poses=[[r[:3] + [t] for r, t in zip(IDENTITY, (0.0, 0.0, -1024.0))]], options=dict(max_depth=2048.0),
                         want=[(0, 0, 0, 0, 1025.0)]),
    # the nearer row wins whatever the order of the rows
    "nearer_wins": dict(points=[P(4.0, 4.0, 2.0), P(2.0, 2.0, 1.0), P(3.0, 1.0, 1.0), P(6.0, 2.0, 2.0)],
                        want=[(0, 2, 2, 1, 1.0), (0, 3, 1, 2, 1.0)]),
    # a footprint of 100 m: the cap.  max_splat 4: hx = 2, ceil(2) .. ceil(6) - 1; max_splat 3: hx = 1.5, ceil(2.5) .. ceil(5.5) - 1
    "cap_even": dict(points=[P(4.0, 4.0, 1.0)], options=dict(footprint=100.0, max_splat=4), want=SQUARE(0, (2, 3, 4, 5), (2, 3, 4, 5), 0, 1.0)),
    "cap_odd": dict(points=[P(4.0, 4.0, 1.0)], options=dict(footprint=100.0, max_splat=3), want=SQUARE(0, (3, 4, 5), (3, 4, 5), 0, 1.0)),
    # hx = 1: left -1 .. 0, top -1 .. 0, right 7 .. 8, bottom 7 .. 8, each cut to the plane; two squares wholly outside
    "clipped": dict(points=[P(0.0, 4.0, 1.0), P(4.0, 0.0, 1.0), P(7.5, 4.0, 1.0), P(4.0, 7.5, 1.0), P(-3.0, 4.0, 1.0), P(4.0, 20.0, 1.0)],
                    options=dict(footprint=2.0),
                    want=SQUARE(0, (0,), (3, 4), 0, 1.0) + SQUARE(0, (3, 4), (0,), 1, 1.0) + SQUARE(0, (7,), (3, 4), 2, 1.0) +
                    SQUARE(0, (3, 4), (7,), 3, 1.0)),
    "keep_glass": dict(points=[P(1.0, 1.0, 1.0), P(2.0, 1.0, 1.0, label=1), P(3.0, 1.0, 1.0, label=2), P(4.0, 1.0, 1.0, label=255)],
                       options=dict(keep="glass"), want=[(0, 2, 1, 1, 1.0)]),
    "keep_non_glass": dict(points=[P(1.0, 1.0, 1.0), P(2.0, 1.0, 1.0, label=1), P(3.0, 1.0, 1.0, label=2), P(4.0, 1.0, 1.0, label=255)],
                           options=dict(keep="non_glass"), want=[(0, 1, 1, 0, 1.0), (0, 3, 1, 2, 1.0), (0, 4, 1, 3, 1.0)]),
    # colour bytes without flag 8 are not a colour
    "no_colour": dict(points=[P(1.0, 1.0, 1.0, rgb=(9, 8, 7), flags=1), P(2.0, 1.0, 1.0, rgb=(1, 2, 3))],
                      want=[(0, 1, 1, 0, 1.0), (0, 2, 1, 1, 1.0)], rgb={0: (0, 0, 0), 1: (1, 2, 3)}),
    # label 255 is a label: the pixel is covered, its index and depth say so
    "label_255": dict(points=[P(1.0, 2.0, 1.0, label=255, rgb=(5, 6, 7))], want=[(0, 1, 2, 0, 1.0)]),
    # R^T (p - t): d = (-2, 3, 1) -> (X, Y, Z) = (d1, -d0, d2) = (3, 2, 1); R itself would give (-3, -2, 1), off the plane
    "turned": dict(points=[P(-1.0, 5.0, 4.0)], poses=[TURN], want=[(0, 3, 2, 0, 1.0)]),
    # a 4 x 4 view in the 8 x 8 plane: (5, 5) lies in the plane and outside the view; the square 3 .. 4 around (3.5, 3.5) is cut to 3
    "small_view": dict(points=[P(5.0, 5.0, 1.0), P(3.5, 3.5, 1.0)], sizes=[(4, 4)], options=dict(footprint=2.0), want=[(0, 3, 3, 1, 1.0)]),
    # sizes says 100 x 100, the host knows 4 x 4: clamped
    "ext_clamp": dict(points=[P(5.0, 5.0, 1.0), P(3.5, 3.5, 1.0)], sizes=[(100, 100)], ext=[(4, 4)], options=dict(footprint=2.0),
                      want=[(0, 3, 3, 1, 1.0)]),
}


def edge_inputs(case):
    """-> dict(cloud, cloud_offsets, intrinsics, sizes, poses, plane, ext, options) of an edge case, numpy."""
    pts = SK.rows(case["points"])
    cloud, offsets = SK.as_cloud(pts, capacity=max(len(pts), 1) + 3)
    if "total" in case:
        offsets = np.array([0, case["total"]], dtype=np.int32)
    cams = np.asarray(case.get("cams", [UNIT_CAM]), dtype=np.float64)
    V = len(cams)
    return dict(cloud=cloud, cloud_offsets=offsets, intrinsics=cams, sizes=np.asarray(case.get("sizes", [EDGE_PLANE] * V), dtype=np.int32),
                poses=None if "poses" not in case else np.asarray(case["poses"], dtype=np.float64), plane=EDGE_PLANE, ext=case.get("ext"),
                options=dict(case.get("options", {})))


def edge_expected(case):
    """The hand-written planes of an edge case."""
    inp = edge_inputs(case)
    V, (Fh, Fw) = len(inp["intrinsics"]), EDGE_PLANE
    rec = inp["cloud"].view(C.RECORD).ravel()
    out = {"view_depth": np.zeros((V, Fh, Fw), np.float32), "view_labels": np.full((V, Fh, Fw), 255, np.uint8),
           "view_index": np.full((V, Fh, Fw), -1, np.int32), "view_rgb": np.zeros((V, Fh, Fw, 3), np.uint8)}
    for v, x, y, row, depth in case["want"]:
        assert float(np.float32(depth)) == depth and out["view_index"][v, y, x] == -1, "an expectation written twice, or not a float32"
        out["view_depth"][v, y, x], out["view_index"][v, y, x], out["view_labels"][v, y, x] = depth, row, rec["label"][row]
        out["view_rgb"][v, y, x] = case["rgb"][row] if "rgb" in case else (rec["rgb"][row] if rec["flags"][row] & C.HAS_COLOUR else 0)
    return out


def statement(inp, **more):
    """The statement applied to a dict of edge_inputs' shape."""
    return W.cloud_view(inp["cloud"], inp["cloud_offsets"], inp["intrinsics"], inp["sizes"], inp["poses"], *inp["plane"], ext=inp.get("ext"),
                        **dict(inp["options"], **more))


def all_edges_in_one_cloud():
    """The points of every edge case that looks through the one default camera, in ONE cloud (they land on each other: this cloud is
    held to the statement, not to hand-written planes) -> (inputs without options, the distinct option sets of those cases)."""
    names = [n for n, c in EDGES.items() if not {"cams", "poses", "sizes", "ext", "total"} & set(c)]
    pts = SK.rows([p for n in names for p in EDGES[n]["points"]])
    cloud, offsets = SK.as_cloud(pts, capacity=len(pts) + 5)
    options = []
    for n in names:
        if EDGES[n].get("options", {}) not in options:
            options.append(EDGES[n].get("options", {}))
    return dict(cloud=cloud, cloud_offsets=offsets, intrinsics=np.asarray([UNIT_CAM], dtype=np.float64), sizes=np.asarray([EDGE_PLANE], np.int32),
                poses=None, plane=EDGE_PLANE, ext=None, options={}), options


# ---- the small shapes at which the kernels can still go wrong
def on_one_pixel(n=5003, mixed=False, seed=7):
    """n rows that all project onto pixel (1, 2) of a 3 x 4 plane: at one depth, or at one of five."""
    rng = np.random.default_rng(seed)
    z = rng.choice(np.array([0.5, 1.0, 1.0 + 2.0 ** -23, 2.0, 4.0], dtype=np.float32), n) if mixed else np.full(n, 2.0, np.float32)
    rec = np.zeros(n, dtype=C.RECORD)
    rec["xyz"] = np.stack([z * np.float32(2.0), z, z], axis=1)          # u = 2 v = 1 exactly
    rec["rgb"], rec["label"], rec["flags"] = rng.integers(0, 256, (n, 3)), rng.integers(0, 3, n), C.POINT | C.HAS_COLOUR
    cloud, offsets = SK.as_cloud(rec, capacity=n + 17)
    return dict(cloud=cloud, cloud_offsets=offsets, intrinsics=np.asarray([UNIT_CAM], dtype=np.float64), sizes=np.asarray([(3, 4)], np.int32),
                poses=None, plane=(3, 4), ext=None, options={})


def splats(n=300, plane=(96, 128), near=1.0, far=0.0, footprint=0.5, max_splat=64, seed=11, spread=20.0):
    """n rows in front of a camera of fx = fy = 100 over a plane of 96 x 128, some of them up to `spread` pixels past a border.  A share `near` of them
    lies at 0.2 .. 0.6 m, where a footprint of 0.5 m is 83 .. 250 pixels: all at the cap, many cut by a border; the share `far` lies
    at 6 .. 9 m, where it is below one pixel."""
    rng = np.random.default_rng(seed)
    Fh, Fw = plane
    kind = rng.random(n)
    z = np.where(kind < near, rng.uniform(0.2, 0.6, n), np.where(kind < near + far, rng.uniform(6.0, 9.0, n), rng.uniform(1.0, 3.0, n)))
    u, v = rng.uniform(-spread, Fw + spread, n), rng.uniform(-spread, Fh + spread, n)
    rec = np.zeros(n, dtype=C.RECORD)
    rec["xyz"] = np.stack([(u - Fw / 2.0) * z / 100.0, (v - Fh / 2.0) * z / 100.0, z], axis=1)
    rec["rgb"], rec["label"], rec["flags"] = rng.integers(0, 256, (n, 3)), rng.integers(0, 2, n), C.POINT | C.HAS_COLOUR
    cloud, offsets = SK.as_cloud(rec, capacity=n + 9)
    return dict(cloud=cloud, cloud_offsets=offsets, intrinsics=np.asarray([(100.0, 100.0, Fw / 2.0, Fh / 2.0)], dtype=np.float64),
                sizes=np.asarray([plane], np.int32), poses=None, plane=plane, ext=None,
                options=dict(footprint=footprint, max_splat=max_splat, min_depth=0.1, max_depth=10.0))


def sixteen_cameras():
    """Frame 1's cloud (555 rows) seen by sixteen cameras around its own, on a plane of 17 x 33 -> inputs."""
    gold = CK.load_golden()
    cloud, offsets = SK.fixture_clouds()[1][1]
    rng = np.random.default_rng(16)
    poses = np.repeat(gold["poses"][1:2], 16, axis=0)
    poses[1:, :, 3] += rng.uniform(-0.05, 0.05, (15, 3))
    cams = np.repeat(gold["intrinsics"][1:2], 16, axis=0)
    cams[1:, :2] *= rng.uniform(0.8, 1.25, (15, 2))
    sizes = np.asarray([(17 - k % 3, 33 - k % 5) for k in range(16)], np.int32)
    return dict(cloud=cloud, cloud_offsets=offsets, intrinsics=cams, sizes=sizes, poses=poses, plane=(17, 33), ext=None,
                options=dict(footprint=0.02, max_splat=6, **DEPTHS))
