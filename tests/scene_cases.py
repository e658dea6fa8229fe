"""The inputs both scene-map tests walk: the clouds of the point-cloud fixture (tests/golden/point_cloud.npz through tests/cloud_ref.py:
three posed frames and the first again from a camera moved a little, 4702 points), the arithmetic edges as named cases with hand-computed results, and the small shapes at which the
kernels can still go wrong."""
import os

import numpy as np

from tests import cloud_cases as K
from tests import cloud_ref as C
from tests import scene_ref as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scene_map.npz")
VOXELS = (0.02, 0.05, 0.25)
FIXTURE_MAX_VOXELS = 5000                                 # above the 4702 points of the fixture
RESHOT = (0.013, -0.007, 0.021)                           # metres
ORIGIN = (0.0, 0.0, 0.0)
F32 = lambda v: float(np.float32(v))


def rows(points):
    """Records from dicts: xyz (required), normal, rgb, label, flags (default 1, + 2 with a normal, + 8 with rgb)."""
    out = np.zeros(len(points), dtype=C.RECORD)
    for rec, p in zip(out, points):
        rec["xyz"] = p["xyz"]
        flags = C.POINT
        if "normal" in p:
            rec["normal"], flags = p["normal"], flags | C.HAS_NORMAL
        if "rgb" in p:
            rec["rgb"], flags = p["rgb"], flags | C.HAS_COLOUR
        rec["label"], rec["region"], rec["source"], rec["frame"] = p.get("label", 0), p.get("region", 7), p.get("source", 3), p.get("frame", 2)
        rec["flags"] = p.get("flags", flags)
    return out


def as_cloud(records, capacity=None):
    """-> (cloud (capacity, 32) uint8 with the records in front, cloud_offsets [0, n])."""
    n = len(records)
    cloud = np.zeros(n if capacity is None else capacity, dtype=C.RECORD)
    cloud[:n] = records
    return cloud.view(np.uint8).reshape(-1, 32), np.array([0, n], dtype=np.int32)


_FIXTURE = {}


def fixture_clouds():
    """-> (whole, parts): the fixture's cloud with frames, poses and normals at stride 1, frame by frame as (cloud, offsets) pairs -
    the three frames lie apart, so frame 0 comes a second time, from a camera moved by RESHOT: a fourth cloud over the voxels of the
    first - and all four as one pair.  Made once."""
    if not _FIXTURE:
        gold = K.load_golden()
        cfg = dict(stride=1, edge=None, keep="all", frames=True, poses=True, normals=True)
        out = K.statement(gold, cfg)
        off = out["cloud_offsets"]
        rec = out["cloud"].view(C.RECORD).ravel()
        moved = dict(gold, poses=gold["poses"].copy())
        moved["poses"][0, :, 3] += RESHOT
        again = K.statement(moved, cfg)
        parts = [rec[off[b]:off[b + 1]] for b in range(len(off) - 1)] + [again["cloud"].view(C.RECORD).ravel()[:again["cloud_offsets"][1]]]
        _FIXTURE["parts"] = [as_cloud(p) for p in parts]
        _FIXTURE["whole"] = as_cloud(np.concatenate(parts))
    return _FIXTURE["whole"], _FIXTURE["parts"]


def golden_id(voxel, split):
    return "v%s-%s" % (voxel, "split" if split else "whole")


def load_golden():
    return dict(np.load(GOLDEN))


# ---- the arithmetic edges: name -> dict(voxel, origin, points, extract options, expected rows / stats / state), by hand.
# A single point at p whose offset in its voxel is a whole number q of 65536ths comes back at i * voxel + (q + 0.5) / 65536 * voxel:
# with voxel = 0.5 that is p + 2^-18.
E = 2.0 ** -18
HALF = 0x3f3504f3                                         # float32(1 / sqrt 2)
EDGES = {
    # floor, not truncation: -0.25 and 0.25 lie in the voxels -1 and 0 of x; truncation would put both into 0
    "negative": dict(voxel=0.5, points=[dict(xyz=(-0.25, -0.75, 0.25)), dict(xyz=(0.25, -0.75, 0.25))],
                     want=[dict(xyz=(-0.25 + E, -0.75 + E, 0.25 + E)), dict(xyz=(0.25 + E, -0.75 + E, 0.25 + E))], stats=[(1, 0, 0, 0)] * 2),
    # exactly on a face: the voxel that begins there, offset 0
    "face": dict(voxel=0.5, points=[dict(xyz=(0.5, 1.0, -0.5))], want=[dict(xyz=(0.5 + E, 1.0 + E, -0.5 + E))], stats=[(1, 0, 0, 0)]),
    # t = (0.5, -0.5, 1.5): indices (0, -1, 1), offsets one half
    "origin": dict(voxel=0.5, origin=(0.25, -1.0, 10.0), points=[dict(xyz=(0.5, -1.25, 10.75))],
                   want=[dict(xyz=(0.5 + E, -1.25 + E, 10.75 + E))], stats=[(1, 0, 0, 0)]),
    # float32(0.1) / 0.03 = 3.33333338...: index 3 (-4 for -0.1), offsets 21845 and 43690; (3 + 21845.5 / 65536) * 0.03 in exact
    # rationals rounds to the float32 0x3dccccd7
    "voxel_0.03": dict(voxel=0.03, points=[dict(xyz=(F32(0.1), F32(-0.1), F32(0.1)))], want=[dict(xyz_bits=(0x3dccccd7, 0xbdccccd7, 0x3dccccd7))],
                       stats=[(1, 0, 0, 0)]),
    # indices -2^20 and 2^20 - 1 are kept, one beyond is dropped; at 2^20 a float32 step is 1/8 and 1/16: the half offsets round away
    "index_range": dict(voxel=1.0, points=[dict(xyz=(-1048576.0, 0.5, 0.5)), dict(xyz=(1048575.5, 0.5, 0.5)), dict(xyz=(1048576.0, 0.5, 0.5)),
                                           dict(xyz=(-1048576.5, 0.5, 0.5)), dict(xyz=(0.5, 0.5, -3e6)), dict(xyz=(0.5, 3e38, 0.5))],
                        want=[dict(xyz=(-1048576.0, 0.5 + 2.0 ** -17, 0.5 + 2.0 ** -17)), dict(xyz=(1048575.5, 0.5 + 2.0 ** -17, 0.5 + 2.0 ** -17))],
                        stats=[(1, 0, 0, 0)] * 2, dropped=4),
    # NaN, Inf, rows without flag 1 (one of them with other flags set): dropped and counted
    "dropped": dict(voxel=0.5, points=[dict(xyz=(np.nan, 0.25, 0.25)), dict(xyz=(0.25, np.inf, 0.25)), dict(xyz=(0.25, 0.25, -np.inf)),
                                       dict(xyz=(0.25, 0.25, 0.25), flags=0), dict(xyz=(0.25, 0.25, 0.25), flags=2 | 8),
                                       dict(xyz=(0.25, 0.25, 0.25), label=1)],
                    want=[dict(xyz=(0.25 + E, 0.25 + E, 0.25 + E), label=1)], stats=[(1, 1, 0, 0)], dropped=5),
    "empty": dict(voxel=0.5, points=[], want=[], stats=[]),
    # 2 n_glass == n is glass, one less is not; a label that is neither 0 nor 1 counts as not glass
    "label_tie": dict(voxel=0.5, points=[dict(xyz=(0.25, 0.25, 0.25), label=1), dict(xyz=(0.25, 0.25, 0.25), label=0),
                                         dict(xyz=(0.75, 0.25, 0.25), label=1), dict(xyz=(0.75, 0.25, 0.25), label=2),
                                         dict(xyz=(0.75, 0.25, 0.25), label=0)],
                      want=[dict(xyz=(0.25 + E, 0.25 + E, 0.25 + E), label=1), dict(xyz=(0.75 + E, 0.25 + E, 0.25 + E), label=0)],
                      stats=[(2, 1, 0, 0), (3, 1, 0, 0)]),
    # means 10.5, 11 and 0.5: halves round up; the third row has no colour and does not count
    "rgb_half": dict(voxel=0.5, points=[dict(xyz=(0.25, 0.25, 0.25), rgb=(10, 11, 0)), dict(xyz=(0.25, 0.25, 0.25), rgb=(11, 11, 1)),
                                        dict(xyz=(0.25, 0.25, 0.25))],
                     want=[dict(xyz=(0.25 + E, 0.25 + E, 0.25 + E), rgb=(11, 11, 1))], stats=[(3, 0, 0, 0)]),
    # +z and -z cancel: no normal, no flag 2; x and y add up to (32767, 32767, 0): (1, 1, 0) / sqrt 2
    "normals": dict(voxel=0.5, points=[dict(xyz=(0.25, 0.25, 0.25), normal=(0, 0, 1)), dict(xyz=(0.25, 0.25, 0.25), normal=(0, 0, -1)),
                                       dict(xyz=(0.75, 0.25, 0.25), normal=(1, 0, 0)), dict(xyz=(0.75, 0.25, 0.25), normal=(0, 1, 0)),
                                       dict(xyz=(0.75, 0.25, 0.25), normal=(np.nan, 0, 0)), dict(xyz=(0.75, 0.25, 0.25), normal=(0, 0, 3.0))],
                    want=[dict(xyz=(0.25 + E, 0.25 + E, 0.25 + E)), dict(xyz=(0.75 + E, 0.25 + E, 0.25 + E), normal_bits=(HALF, HALF, 0))],
                    stats=[(2, 0, 0, 0), (4, 0, 0, 0)]),
    # the mean of offsets 0 and one half is one quarter: 0.125 + 2^-18
    "min_obs": dict(voxel=0.5, points=[dict(xyz=(0.0, 0.25, 0.25)), dict(xyz=(0.75, 0.25, 0.25), label=1), dict(xyz=(0.25, 0.25, 0.25))],
                    options=dict(min_obs=2), want=[dict(xyz=(0.125 + E, 0.25 + E, 0.25 + E))], stats=[(2, 0, 0, 0)]),
    "keep_glass": dict(voxel=0.5, points=[dict(xyz=(0.25, 0.25, 0.25)), dict(xyz=(0.75, 0.25, 0.25), label=1), dict(xyz=(1.25, 0.25, 0.25))],
                       options=dict(keep="glass"), want=[dict(xyz=(0.75 + E, 0.25 + E, 0.25 + E), label=1)], stats=[(1, 1, 0, 0)]),
    "keep_non_glass": dict(voxel=0.5, points=[dict(xyz=(0.25, 0.25, 0.25)), dict(xyz=(0.75, 0.25, 0.25), label=1), dict(xyz=(1.25, 0.25, 0.25))],
                           options=dict(keep="non_glass"),
                           want=[dict(xyz=(0.25 + E, 0.25 + E, 0.25 + E)), dict(xyz=(1.25 + E, 0.25 + E, 0.25 + E))], stats=[(1, 0, 0, 0)] * 2),
}
EDGE_MAX_VOXELS = 8


def edge_expected(case):
    """The hand-computed extraction of an edge case as the three arrays."""
    rec = np.zeros(EDGE_MAX_VOXELS, dtype=C.RECORD)
    stats = np.zeros((EDGE_MAX_VOXELS, 4), dtype=np.int32)
    for k, (w, st) in enumerate(zip(case["want"], case["stats"])):
        flags = C.POINT | S.MERGED
        if "xyz_bits" in w:
            rec["xyz"][k] = np.array(w["xyz_bits"], dtype=np.uint32).view(np.float32)
        else:
            assert all(float(np.float32(v)) == v for v in w["xyz"]), "an expectation that float32 does not hold"
            rec["xyz"][k] = w["xyz"]
        if "normal_bits" in w:
            rec["normal"][k], flags = np.array(w["normal_bits"], dtype=np.uint32).view(np.float32), flags | C.HAS_NORMAL
        if "rgb" in w:
            rec["rgb"][k], flags = w["rgb"], flags | C.HAS_COLOUR
        rec["label"][k], rec["flags"][k] = w.get("label", 0), flags
        stats[k] = st
    return {"cloud": rec.view(np.uint8).reshape(-1, 32), "cloud_offsets": np.array([0, len(case["want"])], dtype=np.int32), "voxel_stats": stats}


def edge_cloud(case):
    return as_cloud(rows(case["points"]), capacity=max(len(case["points"]), 1) + 3)


def all_edges_in_one_cloud():
    """The points of every edge case with voxel 0.5, the default origin and the default options in ONE cloud, each case moved by a
    whole number of 64 m along y into cells of its own (the offsets in the voxels stay; the float32 results do not, so this cloud is
    held to the statement, not to the hand-computed rows) -> (cloud, offsets)."""
    pts = []
    for k, name in enumerate(n for n, c in EDGES.items() if c["voxel"] == 0.5 and "origin" not in c and "options" not in c):
        for p in EDGES[name]["points"]:
            x, y, z = p["xyz"]
            pts.append(dict(p, xyz=(x, y + 64.0 * (k + 1), z)))
    return as_cloud(rows(pts), capacity=len(pts) + 5)


def distinct_voxels(n, voxel=0.1, seed=3):
    """n points in n different voxels scattered over a few metres, shuffled -> records."""
    rng = np.random.default_rng(seed)
    cells = rng.permutation(40 ** 3)[:n]
    idx = np.stack([cells % 40, cells // 40 % 40, cells // 1600], axis=1) - 20
    pts = (idx + rng.uniform(0.1, 0.9, (n, 3))) * voxel
    return rows([dict(xyz=tuple(p), normal=(0.0, 0.6, -0.8), rgb=tuple(rng.integers(0, 256, 3)), label=int(k % 3 == 0)) for k, p in enumerate(pts)])


def contended(n, cells, voxel=0.25, seed=5):
    """n points spread over `cells` neighbouring voxels along x, with normals, colours and labels -> records."""
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(0.0, voxel, (n, 3))
    xyz[:, 0] += voxel * rng.integers(0, cells, n)
    nrm = rng.normal(size=(n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    rgb = rng.integers(0, 256, (n, 3))
    out = np.zeros(n, dtype=C.RECORD)
    out["xyz"], out["normal"], out["rgb"], out["label"] = xyz, nrm, rgb, rng.integers(0, 2, n)
    out["flags"] = C.POINT | C.HAS_NORMAL | C.HAS_COLOUR
    out["flags"][rng.random(n) < 0.1] = C.POINT           # some without normal and colour
    return out
