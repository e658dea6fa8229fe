"""CPU: the statement of ops.point_cloud (tests/cloud_ref.py) against hand-computed points, the fixture tests/golden/point_cloud.npz
against the statement and the conditions that keep the device test from passing vacuously, the ABI of gwd_point_cloud (header,
binding, descriptor layout, refusals before any launch), ops.point_cloud and InferenceSession(cloud=) through the stand-in library
(tests/cloud_fake.py), and the PLY round trip of gw_depth_amd.cloud."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest
import torch

from gw_depth_amd import cloud as PC
from gw_depth_amd import data, hip, infer, ops
from gw_depth_amd.infer import CLOUD_KEYS, FUSION_KEYS, PROFILE_KEYS, REGION_KEYS, RENDER_KEYS, RESULT_KEYS, InferenceSession
from tests import cloud_cases as K
from tests import cloud_ref as C
from tests.cloud_fake import CloudFakeDevice
from tests.test_frames_post import BUDGET, FramesFakeDevice, TinyModel, frames_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = K.load_golden()


def records(out):
    """The points of a statement's / a call's cloud as a structured array."""
    cloud = out["cloud"].numpy() if torch.is_tensor(out["cloud"]) else out["cloud"]
    total = int(out["cloud_offsets"][-1])
    return np.ascontiguousarray(cloud).view(C.RECORD).ravel()[:total]


# ------------------------------------------------------------------------------------------------------------------ the statement
def test_fronto_parallel_plane_by_hand():
    depth, labels = np.full((1, 5, 7), 2.0, np.float32), np.zeros((1, 5, 7), np.uint8)
    cam = np.array([[100.0, 110.0, 3.0, 2.0]])
    out = C.point_cloud(depth, labels, np.array([[5, 7]], np.int32), cam)
    rec = records(out)
    assert out["cloud_offsets"].tolist() == [0, 35] and out["cloud"].shape == (35, 32) and (rec["flags"] == C.POINT | C.HAS_NORMAL).all()
    assert (rec["normal"] == np.array([0, 0, -1], np.float32)).all()                  # border pixels included: one-sided differences
    y, x = 3, 5
    want = np.array([(x - 3.0) * 2.0 / 100.0, (y - 2.0) * 2.0 / 110.0, 2.0]).astype(np.float32)
    assert rec["xyz"][y * 7 + x].tobytes() == want.tobytes() and (rec["frame"] == 0).all() and not rec["rgb"].any()
    # stride 3 of a 5 x 7 frame: rows 0, 3 and columns 0, 3, 6, in raster order
    out = C.point_cloud(depth, labels, np.array([[5, 7]], np.int32), cam, stride=3)
    assert out["cloud_offsets"].tolist() == [0, 6] and out["cloud"].shape == (C.capacity(1, 5, 7, 3), 32) == (6, 32)
    assert np.allclose(records(out)["xyz"][:, 0], np.array([-3, 0, 3, -3, 0, 3]) * 2.0 / 100.0)
    # normals off: zeros, bit 1 clear; a smaller frame in the same plane: the plane beyond it never takes part
    off = records(C.point_cloud(depth, labels, np.array([[2, 3]], np.int32), cam, normals=False))
    assert len(off) == 6 and (off["flags"] == C.POINT).all() and not off["normal"].any()


def test_validity_rules_by_hand():
    depth = np.array([[[1.0, 1.0, 1.0, 1.04, 2.0, np.nan, np.inf, 0.0, 9.0, 1.0]]], np.float32)
    labels = np.array([[[0, 1, 255, 0, 0, 0, 0, 0, 0, 2]]], np.uint8)
    sizes, cam = np.array([[1, 10]], np.int32), np.array([[10.0, 10.0, 0.0, 0.0]])
    xs = lambda **kw: np.rint(records(C.point_cloud(depth, labels, sizes, cam, min_depth=0.5, max_depth=8.0, **kw))["xyz"][:, 0] * 10 /
                              records(C.point_cloud(depth, labels, sizes, cam, min_depth=0.5, max_depth=8.0, **kw))["xyz"][:, 2]).astype(int).tolist()
    assert xs() == [0, 1, 3, 4, 9]                                                   # 255, NaN, Inf, 0 and out of range are no points
    assert xs(keep="glass") == [1] and xs(keep="non_glass") == [0, 3, 4, 9]
    # edge: 1.04 against 1.0 is within 5 %, against 2.0 not; a neighbour without a usable depth, or outside the frame, does not count;
    # the pixel of label 255 has a usable depth and counts as a neighbour
    assert xs(edge=0.05) == [0, 1, 9] and xs(edge=0.03) == [0, 1, 9] and xs(edge=1.0) == [0, 1, 3, 4, 9]
    # lattice neighbours are 3 apart at stride 3: 1.0 | 1.04 | inf | 1.0
    assert xs(stride=3) == [0, 3, 9] and xs(edge=0.05, stride=3) == [0, 3, 9] and xs(edge=0.03, stride=3) == [9]
    one = records(C.point_cloud(depth, labels, sizes, cam, min_depth=0.5, max_depth=8.0))
    assert not one["normal"].any() and (one["flags"] == C.POINT).all()               # a strip one pixel high: no y neighbour


def test_pane_normal_of_a_fitted_known_plane():
    """Exact inverse depths of the 3-D plane n . P = d, fitted by least squares: the pane's normal is -n to 1e-12."""
    n = np.array([0.3, -0.2, 0.933]) / np.linalg.norm([0.3, -0.2, 0.933])
    d, cam = 2.5, (80.0, 82.0, 15.5, 11.25)
    fx, fy, cx, cy = cam
    y, x = np.meshgrid(np.arange(24.0), np.arange(32.0), indexing="ij")
    w = (n[0] * (x - cx) / fx + n[1] * (y - cy) / fy + n[2]) / d                      # 1 / Z on the plane
    coef = np.linalg.lstsq(np.stack([x.ravel(), y.ravel(), np.ones(x.size)], axis=1), w.ravel(), rcond=None)[0]
    got = C.pane_normal(np.concatenate([coef, [0.0, x.size, 0.0]]), cam)
    assert np.abs(got + n).max() <= 1e-12 and abs(np.linalg.norm(got) - 1.0) <= 1e-15
    # through the whole statement: pane pixels take it (flag 4), the others their differences, which agree with it to rounding
    depth, labels = (1.0 / w).astype(np.float32)[None], np.zeros((1, 24, 32), np.uint8)
    rmap = np.zeros((1, 24, 32), np.uint8)
    rmap[0, 4:12, 6:20] = 1
    rmap[0, 15:20, 6:20] = 2
    planes = np.zeros((1, 2, 6))
    planes[0, 0, :3] = coef
    planes[0, 1] = (np.nan, np.nan, np.nan, np.nan, 2, 1)
    for count, panes in ((2, 8 * 14), (0, 0)):
        rec = records(C.point_cloud(depth, labels, np.array([[24, 32]], np.int32), np.array([cam]), region_map=rmap,
                                    region_count=np.array([count], np.int32), planes=planes))
        pane = (rec["flags"] & C.PANE_NORMAL) != 0
        assert pane.sum() == panes and (rec["region"][pane] == 1).all() and (rec["flags"] & C.HAS_NORMAL).all()
        assert (rec["normal"][pane] == (-n).astype(np.float32)).all() and np.abs(rec["normal"] + n).max() < 1e-4
        assert (rec["region"] == rmap.ravel()).all()
    assert C.pane_normal(np.zeros(6), cam) is None                                    # no plane: the pixel falls back to its differences


def test_identity_pose_and_quarter_turn():
    sc = GOLD
    base = dict(K.RECORDED[0], poses=False)
    plain = records(K.statement(sc, base))
    eye = np.tile(np.eye(3, 4), (3, 1, 1))
    same = records(C.point_cloud(sc["depth"], sc["labels"], sc["sizes"], sc["intrinsics"], frames=sc["frames"], region_map=sc["region_map"],
                                 region_count=sc["region_count"], planes=sc["planes"], source=sc["source"], poses=eye,
                                 min_depth=K.MIN_DEPTH, max_depth=K.MAX_DEPTH))
    for f in C.RECORD.names:                                                          # x + 0 = x, 1 x = x: every bit but the sign of a zero
        assert np.array_equal(plain[f], same[f]), f
    turn = np.tile(np.array([[0.0, -1.0, 0.0, 1.0], [1.0, 0.0, 0.0, 2.0], [0.0, 0.0, 1.0, 3.0]]), (3, 1, 1))      # 90 degrees about z, then t
    moved = records(C.point_cloud(sc["depth"], sc["labels"], sc["sizes"], sc["intrinsics"], poses=turn, min_depth=K.MIN_DEPTH,
                                  max_depth=K.MAX_DEPTH, region_map=sc["region_map"], region_count=sc["region_count"], planes=sc["planes"]))
    still = records(C.point_cloud(sc["depth"], sc["labels"], sc["sizes"], sc["intrinsics"], min_depth=K.MIN_DEPTH, max_depth=K.MAX_DEPTH,
                                  region_map=sc["region_map"], region_count=sc["region_count"], planes=sc["planes"]))
    assert np.abs(moved["xyz"] - (still["xyz"][:, [1, 0, 2]] * [-1, 1, 1] + [1, 2, 3])).max() < 1e-6
    assert np.array_equal(moved["normal"], still["normal"][:, [1, 0, 2]] * np.array([-1, 1, 1], np.float32))      # exact: a signed permutation
    assert np.array_equal(moved["flags"], still["flags"])


# ------------------------------------------------------------------------------------------------------------------ the fixture
def test_fixture_is_what_the_statement_gives_and_covers_the_cases():
    sc = K.scene()
    for k, v in K.arrays(sc).items():
        g = GOLD["frames"][int(k[5:])] if k.startswith("frame") else GOLD[k]
        assert g.dtype == v.dtype and g.tobytes() == v.tobytes(), k
    for cfg in K.RECORDED:
        out = K.statement(sc, cfg)
        for k in CLOUD_KEYS:
            assert GOLD["%s.%s" % (K.config_id(cfg), k)].tobytes() == out[k].tobytes(), (cfg, k)
    assert os.path.getsize(K.GOLDEN) < 1 << 20 and len(K.GRID) == 144 and len({K.config_id(c) for c in K.GRID}) == 144
    # frame 0 spans at least three tiles with a ragged last one
    T = hip.CLOUD_TILE
    (fh, fw), (h1, w1), (h2, w2) = (tuple(s) for s in GOLD["sizes"])
    assert fh * fw > 2 * T and (fh * fw) % T != 0 and (h1, w1) == (17, 33) and (h2, w2) == (1, 1)
    assert fh % 3 and fw % 3 and tuple(GOLD["depth"].shape) == (3, fh, fw)
    # at stride 1 a third of its candidates are points, a tenth are not, a whole tile is empty and a whole tile is full
    out = K.statement(sc, dict(stride=1, edge=None, keep="all", frames=False, poses=False, normals=True))
    n0 = int(out["cloud_offsets"][1])
    assert 3 * n0 >= fh * fw and 10 * (fh * fw - n0) >= fh * fw
    d, lab = GOLD["depth"][0].astype(np.float64), GOLD["labels"][0]
    point = (C.usable(d, K.MIN_DEPTH, K.MAX_DEPTH) & (lab != 255)).ravel()
    assert point.sum() == n0
    per_tile = [int(point[t * T:(t + 1) * T].sum()) for t in range(-(-fh * fw // T))]
    assert 0 in per_tile[:-1] and T in per_tile and 0 < per_tile[-1] < (fh * fw) % T + 1
    assert int(K.statement(sc, dict(K.RECORDED[0], keep="glass"))["cloud_offsets"][3] - K.statement(sc, dict(K.RECORDED[0], keep="glass"))["cloud_offsets"][2]) == 0
    # what the scene holds
    f0 = GOLD["depth"][0]
    assert np.isnan(f0).any() and np.isposinf(f0).any() and np.isneginf(f0).any() and (f0 == 0).any() and (f0 > K.MAX_DEPTH).any() \
        and ((f0 > 0) & (f0 < K.MIN_DEPTH)).any() and (lab == 255).any()
    assert GOLD["planes"][0, 0, 5] == 0 and GOLD["planes"][0, 1, 5] == 1 and (GOLD["region_map"][0] == 3).any() and GOLD["region_count"][0] == 2
    rec = records(out)
    f = rec[rec["frame"] == 0]
    assert ((f["flags"] & C.PANE_NORMAL) != 0).sum() == 14 * 21 and (f["region"][(f["flags"] & C.PANE_NORMAL) != 0] == 1).all()
    assert ((f["flags"] & C.HAS_NORMAL) == 0).sum() == 7 + 8                           # the two 1-pixel strips
    assert ((f["region"] == 2) & ((f["flags"] & C.HAS_NORMAL) != 0) & ((f["flags"] & C.PANE_NORMAL) == 0)).any()      # status 1: differences
    assert ((f["region"] == 3) & ((f["flags"] & C.PANE_NORMAL) == 0)).any()
    edge = K.statement(sc, dict(stride=1, edge=0.05, keep="all", frames=False, poses=False, normals=True))
    assert 0 < int(edge["cloud_offsets"][1]) < n0                                      # the depth step loses its flying pixels
    assert (rec[rec["frame"] == 2]["flags"] == C.POINT).all() and (rec["frame"] == 2).sum() == 1
    # every row behind the total is zero, the offsets are the exclusive prefix
    assert not out["cloud"][out["cloud_offsets"][3]:].any() and out["cloud"].shape[0] == 3 * fh * fw
    assert np.array_equal(np.bincount(rec["frame"], minlength=3), np.diff(out["cloud_offsets"]))


# ------------------------------------------------------------------------------------------------------------------ the ABI
def test_header_binding_and_makefile_agree(tmp_path):
    header = open(os.path.join(ROOT, "include", "gwdepth.h")).read()
    for name, value in (("GWD_CLOUD_TILE", hip.CLOUD_TILE), ("GWD_CLOUD_RECORD", hip.CLOUD_RECORD), ("GWD_CLOUD_MAX_STRIDE", hip.CLOUD_MAX_STRIDE),
                        ("GWD_CLOUD_KEEP_ALL", hip.CLOUD_KEEP["all"]), ("GWD_CLOUD_KEEP_GLASS", hip.CLOUD_KEEP["glass"]),
                        ("GWD_CLOUD_KEEP_NON_GLASS", hip.CLOUD_KEEP["non_glass"])):
        assert "#define %s %d" % (name, value) in header, name
    assert "GWD_WS_CLOUD = %d" % hip.WS_CLOUD in header and hip.WS_CLOUD == 7
    assert "#define GWD_VERSION 10" in header and "gwd_point_cloud" in hip.ENTRY_POINTS
    assert tuple(hip.CLOUD_KEEP) == C.KEEP and hip.CLOUD_RECORD == C.RECORD.itemsize == PC.RECORD_BYTES == PC.RECORD_DTYPE.itemsize
    assert (C.POINT, C.HAS_NORMAL, C.PANE_NORMAL, C.HAS_COLOUR) == (PC.FLAG_POINT, PC.FLAG_NORMAL, PC.FLAG_PANE_NORMAL, PC.FLAG_COLOUR) \
        == tuple(ops.CLOUD_FLAGS.values())
    assert [PC.RECORD_DTYPE.fields[n][1] for n in PC.FLOAT_FIELDS + PC.BYTE_FIELDS] == list(range(0, 24, 4)) + list(range(24, 32))
    assert [C.RECORD.fields[n][1] for n in C.RECORD.names] == [0, 12, 24, 27, 28, 29, 30, 31]
    assert "cloud.hip" in open(os.path.join(ROOT, "gw_depth_amd", "csrc", "Makefile")).read()
    assert infer.CLOUD_KEYS == ops.CLOUD_KEYS == ("cloud", "cloud_offsets")
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include "gwdepth.h"\n'
                   'long layout(int k) { switch (k) { case 0: return sizeof(gwd_cloud_desc); case 1: return offsetof(gwd_cloud_desc, min_depth);\n'
                   'case 2: return offsetof(gwd_cloud_desc, capacity); case 3: return offsetof(gwd_cloud_desc, B);\n'
                   'case 4: return offsetof(gwd_cloud_desc, has_frames); case 5: return offsetof(gwd_cloud_desc, ext_h);\n'
                   'case 6: return offsetof(gwd_cloud_desc, ext_w); case 7: return offsetof(gwd_cloud_desc, frames); default: return -1; } }\n')
    out = str(tmp_path / "liblayout.so")
    subprocess.check_call(["gcc", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"), str(src), "-o", out])
    layout = ctypes.CDLL(out).layout
    layout.restype = ctypes.c_long
    D = hip.CloudDesc
    assert [layout(k) for k in range(8)] == [ctypes.sizeof(D), D.min_depth.offset, D.capacity.offset, D.B.offset, D.has_frames.offset,
                                             D.ext_h.offset, D.ext_w.offset, D.frames.offset]


def test_workspace_query_and_refusals_before_any_launch():
    """Every call below must return before the launch: this host has no device to launch on."""
    lib = hip.HipLibrary()
    assert lib.version() == 10
    T = hip.CLOUD_TILE
    assert lib.workspace_bytes(hip.WS_CLOUD, 8, 720, 1280, 1) == (8 * (720 * 1280 // T) + 1) * 4 + 12
    assert lib.workspace_bytes(hip.WS_CLOUD, 3, 61, 53, 3) == 16 and lib.workspace_bytes(hip.WS_CLOUD, 3, 61, 53, 1) == (3 * 4 + 1) * 4 + 12
    for dims in ((0, 8, 8, 1), (17, 8, 8, 1), (1, 0, 8, 1), (1, 8, 16385, 1), (1, 8, 8, 0), (1, 8, 8, 17), (1, 8, 8)):
        with pytest.raises(ValueError):
            lib.workspace_bytes(hip.WS_CLOUD, *dims)
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(buf, ctypes.c_void_p).value
    p += (-p) % 16

    def call(edit=None, **kw):
        d = hip.CloudDesc()
        for n in ("depth", "labels", "sizes", "intrinsics", "region_map", "region_count", "planes", "source", "poses", "workspace", "cloud",
                  "cloud_offsets"):
            setattr(d, n, p)
        d.min_depth, d.max_depth, d.edge, d.capacity = 0.1, 10.0, 0.05, 2 * 64
        d.B, d.Fh, d.Fw, d.max_regions, d.stride, d.normals, d.keep, d.has_frames = 2, 8, 8, 4, 1, 1, 0, 1
        for b in range(2):
            d.ext_h[b] = d.ext_w[b] = 8
            d.frames.ptr[b], d.frames.pitch[b] = p, 24
        for k, v in kw.items():
            setattr(d, k, v)
        if edit:
            edit(d)
        return lib.lib.gwd_point_cloud(ctypes.byref(d), None)

    assert lib.lib.gwd_point_cloud(None, None) == -1
    for k in ("depth", "labels", "sizes", "intrinsics", "workspace", "cloud", "cloud_offsets"):
        assert call(**{k: None}) == -1, k
    assert call(B=0) == -1 and call(B=17) == -1 and call(Fh=0) == -1 and call(Fw=16385) == -1 and call(stride=0) == -1 and call(stride=17) == -1
    assert call(min_depth=math.nan) == -1 and call(max_depth=math.inf) == -1 and call(min_depth=11.0) == -1
    assert call(capacity=127) == -1 and call(capacity=2 ** 31) == -1                  # never a shortened cloud
    assert call(capacity=31, stride=2) == -1 and call(capacity=17, stride=3) == -1    # 2 x 4 x 4 and 2 x 3 x 3 would do
    assert call(capacity=95, edit=lambda d: d.ext_h.__setitem__(1, 4)) == -1          # 64 + 32 would do
    assert call(edit=lambda d: d.ext_h.__setitem__(1, 0)) == -1 and call(edit=lambda d: d.ext_w.__setitem__(0, 9)) == -1
    assert call(edit=lambda d: d.frames.ptr.__setitem__(1, None)) == -1 and call(edit=lambda d: d.frames.pitch.__setitem__(0, 23)) == -1
    assert call(keep=3) == -2 and call(keep=-1) == -2 and call(edge=math.nan) == -2 and call(edge=math.inf) == -2
    assert call(planes=None) == -2 and call(region_map=None) == -2 and call(region_count=None) == -2
    assert call(max_regions=0) == -2 and call(max_regions=33) == -2
    assert call(depth=p + 2) == -3 and call(sizes=p + 2) == -3 and call(intrinsics=p + 4) == -3 and call(planes=p + 4) == -3
    assert call(poses=p + 4) == -3 and call(workspace=p + 8) == -3 and call(cloud=p + 8) == -3 and call(cloud_offsets=p + 2) == -3
    assert call(cloud=p + 8, B=0) == -1


# ------------------------------------------------------------------------------------------------------------------ host logic
@pytest.fixture
def fake(monkeypatch):
    lib = CloudFakeDevice()
    upload = data.upload_tables

    def counted(host, device):
        lib.calls["upload_tables"] += 1
        return upload(host, device)

    monkeypatch.setattr(data, "upload_tables", counted)
    hip.set_library(lib)
    yield lib
    hip.set_library(None)


def scene_call(cfg, **kw):
    T = lambda v: None if v is None else torch.from_numpy(np.ascontiguousarray(v))
    return ops.point_cloud(T(GOLD["depth"]), T(GOLD["labels"]), T(GOLD["sizes"]), T(GOLD["intrinsics"]),
                           frames=[T(f) for f in GOLD["frames"]] if cfg["frames"] else None, region_map=T(GOLD["region_map"]),
                           region_count=T(GOLD["region_count"]), planes=T(GOLD["planes"]), source=T(GOLD["source"]),
                           poses=T(GOLD["poses"]) if cfg["poses"] else None, stride=cfg["stride"], min_depth=K.MIN_DEPTH,
                           max_depth=K.MAX_DEPTH, edge=cfg["edge"], normals=cfg["normals"], keep=cfg["keep"], **kw)


@pytest.mark.parametrize("cfg", K.RECORDED, ids=K.config_id)
def test_point_cloud_gives_the_fixture(fake, cfg):
    out = scene_call(cfg)
    assert tuple(out) == CLOUD_KEYS and out["cloud"].dtype == torch.uint8 and out["cloud_offsets"].dtype == torch.int32
    for k in CLOUD_KEYS:
        want = GOLD["%s.%s" % (K.config_id(cfg), k)]
        assert tuple(out[k].shape) == want.shape and out[k].numpy().tobytes() == want.tobytes(), k
    rec = fake.cloud_calls[-1]
    assert rec["capacity"] == C.capacity(3, 61, 53, cfg["stride"]) and rec["after"] == (0, 0, 0, 0)
    assert rec["frame_sizes"] == (list(K.SIZES) if cfg["frames"] else None)           # a frame's image bounds it
    # with the sizes known on the host the capacity may be exact, and the points are the same
    rows = sum(-(-h // cfg["stride"]) * -(-w // cfg["stride"]) for h, w in K.SIZES)
    exact = scene_call(cfg, frame_sizes=K.SIZES, capacity=rows)
    with pytest.raises(ValueError, match="never shortened"):
        scene_call(cfg, frame_sizes=K.SIZES, capacity=rows - 1)
    assert exact["cloud"].shape[0] == rows == ops.cloud_capacity(3, 61, 53, cfg["stride"], K.SIZES)
    assert torch.equal(exact["cloud"], out["cloud"][:rows]) and torch.equal(exact["cloud_offsets"], out["cloud_offsets"])


def test_point_cloud_validates_before_any_launch(fake):
    T = lambda v: torch.from_numpy(np.ascontiguousarray(v))
    depth, labels, sizes, cam = T(GOLD["depth"]), T(GOLD["labels"]), T(GOLD["sizes"]), T(GOLD["intrinsics"])
    rmap, cnt, planes, poses = T(GOLD["region_map"]), T(GOLD["region_count"]), T(GOLD["planes"]), T(GOLD["poses"])
    for kw in ({"stride": 0}, {"stride": 17}, {"min_depth": 0.0}, {"min_depth": 2.0, "max_depth": 1.0}, {"max_depth": math.inf}, {"edge": 0.0},
               {"edge": -1.0}, {"edge": math.nan}, {"edge": math.inf}, {"keep": "mirrors"}, {"capacity": 3 * 61 * 53 - 1}, {"capacity": 2 ** 31},
               {"capacity": 3233 + 561, "frame_sizes": K.SIZES}, {"frame_sizes": K.SIZES[:2]}, {"frame_sizes": [(0, 5)] * 3},
               {"capacity": 3 * 21 * 18 - 1, "stride": 3}):
        with pytest.raises(ValueError):
            ops.point_cloud(depth, labels, sizes, cam, **kw)
    for kw in ({"stride": 1.5}, {"normals": 1}, {"capacity": 1e4 + 0.5}):
        with pytest.raises(TypeError):
            ops.point_cloud(depth, labels, sizes, cam, **kw)
    for args in ((depth.double(), labels, sizes, cam), (depth, labels.int(), sizes, cam), (depth, labels, sizes.long(), cam),
                 (depth, labels, sizes, cam.float()), (depth.numpy(), labels, sizes, cam)):
        with pytest.raises(TypeError):
            ops.point_cloud(*args)
    for args in ((depth[0], labels[0], sizes, cam), (depth, labels[:, :60], sizes, cam), (depth, labels, sizes[:2], cam), (depth, labels, sizes, cam[:, :3]),
                 (depth[:, :0], labels[:, :0], sizes, cam)):
        with pytest.raises(ValueError):
            ops.point_cloud(*args)
    with pytest.raises(ValueError):
        ops.point_cloud(depth.expand(3, 61, 53)[:1].expand(17, 61, 53), labels[:1].expand(17, 61, 53), sizes[:1].expand(17, 2), cam[:1].expand(17, 4))
    for kw in ({"region_map": rmap}, {"planes": planes, "region_count": cnt}, {"region_map": rmap, "region_count": cnt[:2], "planes": planes},
               {"region_map": rmap, "region_count": cnt, "planes": planes[:, :, :5]}, {"region_map": rmap[:, :60], "region_count": cnt, "planes": planes},
               {"poses": poses[:, :, :3]}, {"poses": poses[:2]}, {"source": rmap[:2]}, {"frames": [T(f) for f in GOLD["frames"][:2]]},
               {"frames": [T(f)[:, :, :2] for f in GOLD["frames"]]}):
        with pytest.raises(ValueError):
            ops.point_cloud(depth, labels, sizes, cam, **kw)
    for kw in ({"poses": poses.float()}, {"source": rmap.int()}, {"region_map": rmap.int(), "region_count": cnt, "planes": planes},
               {"frames": [T(f).float() for f in GOLD["frames"]]}):
        with pytest.raises(TypeError):
            ops.point_cloud(depth, labels, sizes, cam, **kw)
    assert fake.cloud_calls == []
    # what is allowed: a larger capacity (zeros behind the points), a frame that covers less than sizes says: clipped to it
    big = ops.point_cloud(depth, labels, sizes, cam, capacity=3 * 61 * 53 + 100, min_depth=K.MIN_DEPTH, max_depth=K.MAX_DEPTH)
    total = int(big["cloud_offsets"][3])
    assert big["cloud"].shape[0] == 3 * 61 * 53 + 100 and not big["cloud"][total:].any() and big["cloud"][:total, 31].all()
    cut = [T(GOLD["frames"][0])[:30, :20], T(GOLD["frames"][1]), T(GOLD["frames"][2])]
    small = ops.point_cloud(depth, labels, sizes, cam, frames=cut, min_depth=K.MIN_DEPTH, max_depth=K.MAX_DEPTH)
    assert fake.cloud_calls[-1]["frame_sizes"] == [(30, 20), (17, 33), (1, 1)] and 0 < int(small["cloud_offsets"][1]) <= 30 * 20
    tight = ops.point_cloud(depth, labels, sizes, cam, frames=cut, capacity=30 * 20 + 17 * 33 + 1, min_depth=K.MIN_DEPTH, max_depth=K.MAX_DEPTH)
    assert torch.equal(tight["cloud"], small["cloud"][:30 * 20 + 17 * 33 + 1]) and torch.equal(tight["cloud_offsets"], small["cloud_offsets"])


def test_default_session_issues_todays_launches_and_keys(fake):
    sess = InferenceSession(TinyModel(), compute_dtype=torch.float32, graph=False)
    assert sess.cloud is None
    res = sess.predict_frames(frames_of(3), size=48, max_size=64)
    assert fake.calls == dict(BUDGET, gather2d_batch=0) and fake.cloud_calls == [] and fake.render_calls == [] and fake.region_calls == []
    assert sorted(res) == sorted(RESULT_KEYS + ("net_sizes",))
    hip.set_library(FramesFakeDevice())                                                 # the stand-in without the new call: not needed
    old = InferenceSession(TinyModel(), compute_dtype=torch.float32, graph=False, cloud=None).predict_frames(frames_of(3), size=48, max_size=64)
    for k in res:
        assert torch.equal(res[k], old[k]), k
    with pytest.raises(ValueError, match="line_profiles="):
        sess.predict_frames(frames_of(3), size=48, max_size=64, intrinsics=[(50.0, 50.0, 30.0, 20.0)] * 3)
    with pytest.raises(ValueError, match="cloud="):
        sess.predict_frames(frames_of(3), size=48, max_size=64, poses=[np.eye(3, 4)] * 3)


def session_cloud(res, frames, depth, cam, poses=None, **options):
    """The statement on the session's own outputs."""
    n = lambda k: res[k].numpy() if k in res else None
    return C.point_cloud(res[depth].numpy(), n("labels"), n("sizes"), np.asarray(cam, np.float64), frames=[f.numpy() for f in frames],
                         region_map=n("region_map") if "planes" in res else None, region_count=n("region_count") if "planes" in res else None,
                         planes=n("planes"), source=n("fused_source"), poses=None if poses is None else np.asarray(poses, np.float64),
                         capacity_rows=res["cloud"].shape[0], **options)


def cams(frames):
    return [(60.0, 61.0, w / 2.0, h / 2.0) for h, w in (f.shape[:2] for f in frames)]


def test_plain_session_makes_its_cloud_from_depth(fake):
    sess = InferenceSession(TinyModel(), compute_dtype=torch.float32, graph=False, cloud=True, max_depth=5.0)
    assert sess.cloud == dict(depth="auto", planar=False, options=dict(stride=1, min_depth=1e-3, max_depth=5.0, edge=None, normals=True, keep="all"))
    frames = frames_of(3)
    res = sess.predict_frames(frames, size=48, max_size=64, intrinsics=cams(frames))
    assert fake.calls == dict(BUDGET, gather2d_batch=0)                                # the launches before it are the same
    assert sorted(res) == sorted(RESULT_KEYS + ("net_sizes",) + CLOUD_KEYS)
    assert len(fake.cloud_calls) == 1
    rec = fake.cloud_calls[0]
    assert rec["depth"] is res["depth"] and rec["frames"] and not rec["region_map"] and not rec["source"] and not rec["poses"]
    assert rec["frame_sizes"] == [tuple(f.shape[:2]) for f in frames] and rec["capacity"] == sum(f.shape[0] * f.shape[1] for f in frames)
    assert (rec["stride"], rec["min_depth"], rec["max_depth"], rec["edge"], rec["normals"], rec["keep"]) == (1, 1e-3, 5.0, None, True, "all")
    want = session_cloud(res, frames, "depth", cams(frames), max_depth=5.0)
    for k in CLOUD_KEYS:
        assert res[k].numpy().tobytes() == want[k].tobytes(), k
    got = PC.fields(res["cloud"])
    assert int(res["cloud_offsets"][3]) > 0 and (got["flags"][:int(res["cloud_offsets"][3])] & C.HAS_COLOUR).all()
    # a call without intrinsics returns what it returns today
    bare = sess.predict_frames(frames, size=48, max_size=64)
    assert sorted(bare) == sorted(RESULT_KEYS + ("net_sizes",)) and len(fake.cloud_calls) == 1
    for k in bare:
        assert torch.equal(bare[k], res[k]), k
    with pytest.raises(ValueError, match="intrinsics"):
        sess.predict_frames(frames, size=48, max_size=64, intrinsics=cams(frames)[:2])
    with pytest.raises(ValueError, match="intrinsics"):
        sess.predict_frames(frames, size=48, max_size=64, poses=[np.eye(3, 4)] * 3)
    with pytest.raises(ValueError, match="poses"):
        sess.predict_frames(frames, size=48, max_size=64, intrinsics=cams(frames), poses=[np.eye(4)] * 3)
    with pytest.raises(ValueError, match="sensor_depth"):
        sess.predict_frames(frames, size=48, max_size=64, intrinsics=cams(frames), sensor_depth=[torch.zeros(f.shape[:2], dtype=torch.uint16) for f in frames])


def test_session_with_everything_runs_the_cloud_behind_fusion_and_profiles_and_before_render(fake):
    sess = InferenceSession(TinyModel(), compute_dtype=torch.float32, graph=False, line_nms=0.01, regions={"min_area": 4, "max_regions": 8},
                            line_profiles=True, fusion=True, render=True, cloud={"stride": 2, "edge": 0.1, "keep": "glass"})
    frames = frames_of(3)
    sensor = [torch.full(tuple(f.shape[:2]), 1500, dtype=torch.uint16) for f in frames]
    turn = [[[0.0, -1.0, 0.0, 1.0], [1.0, 0.0, 0.0, 2.0], [0.0, 0.0, 1.0, 3.0]]] * 3
    res = sess.predict_frames(frames, size=48, max_size=64, sensor_depth=sensor, intrinsics=cams(frames), poses=turn)
    assert sorted(res) == sorted(RESULT_KEYS + ("net_sizes",) + infer.NMS_KEYS + REGION_KEYS + PROFILE_KEYS + FUSION_KEYS + CLOUD_KEYS + RENDER_KEYS)
    rec = fake.cloud_calls[-1]
    assert rec["after"] == (3, 1, 3, 0) and fake.render_calls[-1]["after"] == (3, 1, 3) and len(fake.render_calls) == 1
    assert rec["depth"] is res["depth_fused"] and rec["region_map"] and rec["source"] and rec["poses"] and rec["frames"]
    assert (rec["stride"], rec["edge"], rec["keep"]) == (2, 0.1, "glass")
    want = session_cloud(res, frames, "depth_fused", cams(frames), poses=turn, stride=2, edge=0.1, keep="glass", min_depth=1e-3, max_depth=10.0)
    for k in CLOUD_KEYS:
        assert res[k].numpy().tobytes() == want[k].tobytes(), k
    # the call did not fuse: "auto" falls to the planar depth, and there is no source
    res = sess.predict_frames(frames, size=48, max_size=64, intrinsics=cams(frames))
    rec = fake.cloud_calls[-1]
    assert rec["depth"] is res["depth_planar"] and rec["region_map"] and not rec["source"] and not rec["poses"]
    # every other key is what a session without cloud= returns
    plain = InferenceSession(TinyModel(), compute_dtype=torch.float32, graph=False, line_nms=0.01, regions={"min_area": 4, "max_regions": 8},
                             line_profiles=True, fusion=True, render=True).predict_frames(frames, size=48, max_size=64, intrinsics=cams(frames))
    assert sorted(plain) == sorted(set(res) - set(CLOUD_KEYS))
    for k in plain:
        assert torch.equal(plain[k], res[k], ) or (res[k].dtype.is_floating_point and np.array_equal(plain[k].numpy(), res[k].numpy(), equal_nan=True)), k


@pytest.mark.parametrize("kw,depth,want", [
    (dict(), "auto", "depth"),
    (dict(regions={"min_area": 4}), "auto", "depth_planar"),
    (dict(regions={"min_area": 4, "planar": False}), "auto", "depth"),
    (dict(regions={"min_area": 4}, fusion=True), "auto", "depth_planar"),               # fusion=, but the call passes no sensor plane
    (dict(regions={"min_area": 4}, fusion=True), "depth", "depth"),
    (dict(regions={"min_area": 4}), "depth_planar", "depth_planar"),
], ids=["plain", "regions", "regions-no-planar", "fusion-unfused", "named-depth", "named-planar"])
def test_auto_depth_choice(fake, kw, depth, want):
    sess = InferenceSession(TinyModel(), compute_dtype=torch.float32, graph=False, cloud={"depth": depth}, **kw)
    frames = frames_of(2)
    res = sess.predict_frames(frames, size=48, max_size=64, intrinsics=cams(frames))
    rec = fake.cloud_calls[-1]
    assert rec["depth"] is res[want] and rec["region_map"] == ("planes" in res)


def test_fused_depth_by_name_and_by_auto(fake):
    frames = frames_of(2)
    sensor = [torch.full(tuple(f.shape[:2]), 1500, dtype=torch.uint16) for f in frames]
    for depth in ("auto", "depth_fused"):
        sess = InferenceSession(TinyModel(), compute_dtype=torch.float32, graph=False, regions={"min_area": 4}, fusion=True, cloud={"depth": depth})
        res = sess.predict_frames(frames, size=48, max_size=64, intrinsics=cams(frames), sensor_depth=sensor)
        assert fake.cloud_calls[-1]["depth"] is res["depth_fused"] and fake.cloud_calls[-1]["source"]
    with pytest.raises(ValueError, match="sensor_depth"):                               # named, and the call did not fuse
        sess.predict_frames(frames, size=48, max_size=64, intrinsics=cams(frames))


def test_session_options_are_validated():
    mk = lambda **kw: InferenceSession(TinyModel(), compute_dtype=torch.float32, graph=False, **kw)
    for bad, exc in ((False, TypeError), (3, TypeError), ({"colour": 3}, TypeError), ({"capacity": 100}, TypeError), ({"stride": 0}, ValueError),
                     ({"stride": 17}, ValueError), ({"edge": 0}, ValueError), ({"keep": "walls"}, ValueError), ({"normals": "yes"}, TypeError),
                     ({"depth": "depth_mm"}, ValueError), ({"depth": "depth_planar"}, ValueError), ({"depth": "depth_fused"}, ValueError),
                     ({"min_depth": 0.0}, ValueError)):
        with pytest.raises(exc):
            mk(cloud=bad)
    with pytest.raises(ValueError, match="depth_planar"):
        mk(regions={"planar": False}, cloud={"depth": "depth_planar"})
    with pytest.raises(ValueError, match="depth_fused"):
        mk(regions=True, cloud={"depth": "depth_fused"})
    assert mk(regions=True, fusion=True, cloud={"depth": "depth_fused", "min_depth": 0.5}).cloud["options"]["min_depth"] == 0.5


# ------------------------------------------------------------------------------------------------------------------ fields and PLY
def test_fields_are_views_of_the_cloud():
    cfg = K.RECORDED[0]
    cloud = torch.from_numpy(GOLD["%s.cloud" % K.config_id(cfg)].copy())
    rec = cloud.numpy().view(C.RECORD).ravel()
    f = PC.fields(cloud)
    assert sorted(f) == sorted(("xyz", "normal", "rgb", "label", "region", "source", "frame", "flags"))
    for k in f:
        assert f[k].dtype == (torch.float32 if k in ("xyz", "normal") else torch.uint8) and np.array_equal(f[k].numpy(), rec[k], equal_nan=True), k
        assert f[k].untyped_storage().data_ptr() == cloud.untyped_storage().data_ptr(), k
    f["xyz"][5, 1] = 42.0
    f["flags"][7] = 0
    assert cloud.numpy().view(C.RECORD).ravel()["xyz"][5, 1] == 42.0 and cloud[7, 31] == 0
    empty = PC.fields(torch.zeros((0, 32), dtype=torch.uint8))
    assert tuple(empty["xyz"].shape) == (0, 3) and tuple(empty["flags"].shape) == (0,)
    for bad in (cloud[:, :31], cloud.int(), cloud.numpy()):
        with pytest.raises(TypeError):
            PC.fields(bad)


@pytest.mark.parametrize("frame", [None, 0, 1, 2])
def test_ply_round_trip(tmp_path, frame):
    cfg = K.RECORDED[0]
    cloud = torch.from_numpy(GOLD["%s.cloud" % K.config_id(cfg)])
    off = torch.from_numpy(GOLD["%s.cloud_offsets" % K.config_id(cfg)])
    path = str(tmp_path / "cloud.ply")
    n = PC.save_ply(path, cloud, off, frame=frame)
    lo, hi = (0, int(off[3])) if frame is None else (int(off[frame]), int(off[frame + 1]))
    assert n == hi - lo
    back = PC.load_ply(path)
    assert back.dtype == torch.uint8 and back.numpy().tobytes() == cloud[lo:hi].numpy().tobytes()
    # the header, line by line, as any PLY reader takes it
    blob = open(path, "rb").read()
    head, body = blob.split(b"end_header\n", 1)
    lines = head.decode("ascii").splitlines()
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    elements = [ln.split() for ln in lines if ln.startswith("element")]
    props = [ln.split() for ln in lines if ln.startswith("property")]
    assert elements == [["element", "vertex", str(n)]] and all(len(p) == 3 for p in props)
    assert [p[2] for p in props] == list(PC.FLOAT_FIELDS + PC.BYTE_FIELDS) and [p[1] for p in props] == ["float"] * 6 + ["uchar"] * 8
    assert set(ln.split()[0] for ln in lines[2:]) <= {"comment", "element", "property"}
    assert len(body) == 32 * n == sum({"float": 4, "uchar": 1}[p[1]] for p in props) * n
    rec = np.frombuffer(body, dtype=PC.RECORD_DTYPE)
    want = cloud[lo:hi].numpy().view(C.RECORD).ravel()
    assert np.array_equal(rec["x"], want["xyz"][:, 0]) and np.array_equal(rec["nz"], want["normal"][:, 2]) and np.array_equal(rec["flags"], want["flags"])
    assert np.array_equal(rec["blue"], want["rgb"][:, 2])


def test_ply_refuses_what_it_did_not_write(tmp_path):
    cloud, off = torch.zeros((4, 32), dtype=torch.uint8), [0, 2, 3]
    for bad in ([0, 5], [1, 2], [0, 3, 2], [0]):
        with pytest.raises(ValueError):
            PC.save_ply(str(tmp_path / "x.ply"), cloud, bad)
    with pytest.raises(ValueError):
        PC.save_ply(str(tmp_path / "x.ply"), cloud, off, frame=2)
    path = str(tmp_path / "x.ply")
    assert PC.save_ply(path, cloud, off) == 3
    blob = open(path, "rb").read()
    for edit in (blob[:-1], blob.replace(b"property uchar flags\n", b""), blob.replace(b"binary_little_endian", b"binary_big_endian"), b"nothing"):
        open(path, "wb").write(edit)
        with pytest.raises(ValueError):
            PC.load_ply(path)
