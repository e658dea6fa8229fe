"""CPU: the statement of the scene view (tests/view_ref.py) against an independent vectorised np.lexsort formulation, against the round
trip through ops.point_cloud's statement, against results written out by hand and against the fixture tests/golden/scene_view.npz;
the ABI of gwd_cloud_view (header, binding, descriptor layout, refusals before any launch); ops.cloud_view, cloud.SceneMap.view and
InferenceSession(scene_view=) through the stand-in library (tests/view_fake.py).

One thing is decided here and not in the issue that asked for this: the rule - pixels ceil(u - hx) .. ceil(u + hx) - 1, that is
u - hx <= x < u + hx - and the edge "u - hx exactly an integer: that pixel is in, the pixel at u + hx is out" put a footprint-0 point
at u = x + 0.5 on pixel x.  The same text also says such a tie goes to x + 1; both cannot hold, and the rule as written is what the
statement, the kernels and the case "half_pixel" below follow."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest
import torch

from gw_depth_amd import cloud as PC
from gw_depth_amd import data, hip, infer, ops
from gw_depth_amd.infer import CLOUD_KEYS, RESULT_KEYS, SCENE_VIEW_KEYS, InferenceSession
from tests import cloud_cases as CK
from tests import cloud_ref as C
from tests import scene_cases as SK
from tests import scene_ref as S
from tests import view_cases as K
from tests import view_ref as W
from tests.test_frames_post import BUDGET, TinyModel, frames_of
from tests.view_fake import ViewFakeDevice

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def lexsort_view(cloud, cloud_offsets, intrinsics, sizes, poses, Fh, Fw, min_depth=1e-3, max_depth=10.0, footprint=0.0, max_splat=32,
                 keep="all"):
    """The second formulation: every row of a view at once in array arithmetic, the rectangles expanded into (pixel, key) pairs,
    np.lexsort over them, the first pair of every pixel."""
    rec = np.ascontiguousarray(cloud).view(C.RECORD).ravel()
    total = min(max(int(cloud_offsets[-1]), 0), len(rec))
    live = rec[:total]
    ok = ((live["flags"] & 1) != 0) & np.isfinite(live["xyz"]).all(1)
    ok &= {"all": np.ones(total, bool), "glass": live["label"] == 1, "non_glass": live["label"] != 1}[keep]
    V = len(intrinsics)
    depth, index = np.zeros((V, Fh * Fw), np.float32), np.full((V, Fh * Fw), -1, np.int32)
    labels, rgb = np.full((V, Fh * Fw), 255, np.uint8), np.zeros((V, Fh * Fw, 3), np.uint8)
    with np.errstate(all="ignore"):
        for v in range(V):
            fx, fy, cx, cy = intrinsics[v]
            fh, fw = min(max(int(sizes[v][0]), 0), Fh), min(max(int(sizes[v][1]), 0), Fw)
            p = live["xyz"].astype(np.float64)
            if poses is not None:
                R, d = poses[v][:, :3], p - poses[v][:, 3]
                p = np.stack([(R[0, i] * d[:, 0] + R[1, i] * d[:, 1]) + R[2, i] * d[:, 2] for i in range(3)], axis=1)
            X, Y, Z = p.T
            sel = ok & np.isfinite(Z) & (Z >= min_depth) & (Z <= max_depth)
            u, w = (fx * X) / Z + cx, (fy * Y) / Z + cy
            half, cap = 0.5 * footprint, max_splat / 2.0
            hx, hy = (half * fx) / Z, (half * fy) / Z
            sel &= ~np.isnan(hx) & ~np.isnan(hy)
            hx, hy = np.maximum(0.5, np.minimum(cap, hx)), np.maximum(0.5, np.minimum(cap, hy))
            x0, x1, y0, y1 = np.ceil(u - hx), np.ceil(u + hx) - 1.0, np.ceil(w - hy), np.ceil(w + hy) - 1.0
            sel &= (x0 <= x1) & (y0 <= y1)
            x0, x1, y0, y1 = np.maximum(x0, 0.0), np.minimum(x1, fw - 1.0), np.maximum(y0, 0.0), np.minimum(y1, fh - 1.0)
            sel &= (x0 <= x1) & (y0 <= y1)
            rows = np.nonzero(sel)[0]
            if len(rows) == 0:
                continue
            x0, y0 = x0[rows].astype(np.int64), y0[rows].astype(np.int64)
            nx, ny = x1[rows].astype(np.int64) - x0 + 1, y1[rows].astype(np.int64) - y0 + 1
            count = nx * ny
            who = np.repeat(np.arange(len(rows)), count)
            local = np.arange(count.sum()) - np.repeat(np.cumsum(count) - count, count)
            pixel = (y0[who] + local // nx[who]) * Fw + x0[who] + local % nx[who]
            bits = Z[rows].astype(np.float32).view(np.uint32).astype(np.uint64)
            key = (bits << np.uint64(32) | rows.astype(np.uint64))[who]
            order = np.lexsort((key, pixel))
            pixel, key = pixel[order], key[order]
            first = np.r_[True, pixel[1:] != pixel[:-1]]
            pixel, key = pixel[first], key[first]
            winner = (key & np.uint64(0xffffffff)).astype(np.int64)
            depth[v, pixel] = (key >> np.uint64(32)).astype(np.uint32).view(np.float32)
            index[v, pixel], labels[v, pixel] = winner, live["label"][winner]
            rgb[v, pixel] = np.where(((live["flags"][winner] & 8) != 0)[:, None], live["rgb"][winner], 0)
    return {"view_depth": depth.reshape(V, Fh, Fw), "view_labels": labels.reshape(V, Fh, Fw), "view_index": index.reshape(V, Fh, Fw),
            "view_rgb": rgb.reshape(V, Fh, Fw, 3)}


# ------------------------------------------------------------------------------------------------------------------ the statement
def test_statement_equals_the_lexsort_formulation():
    whole, parts = SK.fixture_clouds()
    cams, poses, sizes = K.fixture_cameras()
    assert int(whole[1][-1]) == 4702 > 4 * hip.VIEW_TILE and 4702 % hip.VIEW_TILE != 0
    K.same(K.fixture_whole_view(), lexsort_view(whole[0], whole[1], cams, sizes, poses, *CK.PLANE, **K.DEPTHS), "whole")
    for voxel in K.VOXELS:
        ext = K.fixture_map(voxel)
        K.same(K.fixture_map_view(voxel), lexsort_view(ext["cloud"], ext["cloud_offsets"], cams, sizes, poses, *CK.PLANE, footprint=voxel,
                                                       max_splat=K.MAP_SPLAT, **K.DEPTHS), "map %s" % voxel)
    for opt in (dict(keep="glass", footprint=0.1), dict(keep="non_glass", footprint=0.03, max_splat=5), dict(footprint=0.2, max_splat=64)):
        one = W.cloud_view(*parts[1], cams, sizes, None, *CK.PLANE, **opt)      # no poses: frame 1's cloud as if in every camera's frame
        K.same(one, lexsort_view(*parts[1], cams, sizes, None, *CK.PLANE, **opt), "frame 1 %r" % (opt,))
    for inp in (K.splats(), K.splats(near=0.3, far=0.4, seed=12), K.sixteen_cameras(), K.on_one_pixel(mixed=True)):
        K.same(K.statement(inp), lexsort_view(inp["cloud"], inp["cloud_offsets"], inp["intrinsics"], inp["sizes"], inp["poses"], *inp["plane"],
                                              **inp["options"]), "shapes")


@pytest.mark.parametrize("b", range(3))
def test_round_trip_a_frames_cloud_comes_back_on_its_own_pixels(b):
    """A frame's cloud (stride 1, poses) seen from that frame's own pose and intrinsics at footprint 0: every point on exactly its own
    pixel, as many covered pixels as rows, view_depth within 1.4e-7 relative of the frame's depth (one pose there and back in fp64 and
    two roundings to float32: 2^-23 = 1.2e-7)."""
    gold = CK.load_golden()
    cloud, offsets = SK.fixture_clouds()[1][b]
    n = int(offsets[1])
    assert n == (2073, 555, 1)[b]
    fh, fw = CK.SIZES[b]
    out = W.cloud_view(cloud, offsets, gold["intrinsics"][b:b + 1], gold["sizes"][b:b + 1], gold["poses"][b:b + 1], fh, fw, **K.DEPTHS)
    hit = out["view_index"][0] >= 0
    assert int(hit.sum()) == n
    # the cloud is in raster order: the covered pixels, in raster order, carry the rows 0 .. n - 1
    assert np.array_equal(out["view_index"][0][hit], np.arange(n))
    want = gold["depth"][b, :fh, :fw]
    lab = gold["labels"][b, :fh, :fw]
    assert np.array_equal(hit, C.usable(want.astype(np.float64), CK.MIN_DEPTH, CK.MAX_DEPTH) & (lab != 255))
    assert np.abs(out["view_depth"][0][hit].astype(np.float64) / want[hit].astype(np.float64) - 1.0).max() <= 1.4e-7
    assert np.array_equal(out["view_labels"][0][hit], lab[hit]) and (out["view_labels"][0][~hit] == 255).all()
    assert np.array_equal(out["view_rgb"][0][hit], gold["frames"][b][hit]) and not out["view_rgb"][0][~hit].any()
    assert not out["view_depth"][0][~hit].any()


@pytest.mark.parametrize("voxel", K.VOXELS)
def test_fixture_map_view_is_the_recorded_one(voxel):
    gold = K.load_golden()
    out = K.fixture_map_view(voxel)
    K.same(out, {k: gold["%s.%s" % (K.golden_id(voxel), k)] for k in W.KEYS}, "golden %s" % voxel)
    hit = out["view_index"] >= 0
    kept = int(K.fixture_map(voxel)["cloud_offsets"][1])
    assert out["view_index"].max() < kept and hit[0].sum() > 1000 and hit[3].sum() > 1000 and hit[2].sum() == 1
    assert not hit[1, 17:].any() and not hit[1, :, 33:].any() and not hit[2, 1:].any() and not hit[2, :, 1:].any()      # outside (fh, fw)
    assert set(np.unique(out["view_labels"][hit])) == {0, 1}
    # a map of 0.25 m seen at 8 pixels per voxel at most fills its views more than one of 0.05 m does
    assert voxel == 0.05 or hit[0].sum() > (K.fixture_map_view(0.05)["view_index"][0] >= 0).sum()


@pytest.mark.parametrize("name", list(K.EDGES))
def test_arithmetic_edges_by_hand(name):
    case = K.EDGES[name]
    inp = K.edge_inputs(case)
    want = K.edge_expected(case)
    K.same(K.statement(inp), want, name)
    if inp["ext"] is None:
        K.same(lexsort_view(inp["cloud"], inp["cloud_offsets"], inp["intrinsics"], inp["sizes"], inp["poses"], *inp["plane"], **inp["options"]),
               want, name + " (lexsort)")


def test_all_edges_in_one_cloud_is_not_empty():
    inp, options = K.all_edges_in_one_cloud()
    assert int(inp["cloud_offsets"][1]) >= 25 and len(options) >= 5
    covered = [int((K.statement(inp, **opt)["view_index"] >= 0).sum()) for opt in options]
    assert min(covered) >= 1 and len(set(covered)) > 1


# ------------------------------------------------------------------------------------------------------------------ the ABI
def test_header_binding_and_makefile_agree(tmp_path):
    header = open(os.path.join(ROOT, "include", "gwdepth.h")).read()
    for name, value in (("GWD_VIEW_TILE", hip.VIEW_TILE), ("GWD_VIEW_MAX_SPLAT", hip.VIEW_MAX_SPLAT)):
        assert "#define %s %d" % (name, value) in header, name
    assert "GWD_WS_VIEW = %d" % hip.WS_VIEW in header and hip.WS_VIEW == 9 and "#define GWD_VERSION 10" in header
    assert "gwd_cloud_view" in hip.ENTRY_POINTS and len(hip.ENTRY_POINTS) == len(set(hip.ENTRY_POINTS))
    assert "int gwd_cloud_view(const gwd_view_desc *desc, void *stream);" in header
    assert hip.VIEW_MAX_SPLAT == W.MAX_SPLAT and hip.VIEW_MAX_VIEWS == W.MAX_VIEWS and ops.VIEW_KEYS == W.KEYS
    assert SCENE_VIEW_KEYS == ("scene_depth", "scene_labels", "scene_index", "scene_rgb", "scene_cloud", "scene_cloud_offsets", "scene_stats")
    assert "view.hip" in open(os.path.join(ROOT, "gw_depth_amd", "csrc", "Makefile")).read()
    fields = [n for n, _ in hip.ViewDesc._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include "gwdepth.h"\nlong layout(int k) { switch (k) { case 0: return sizeof(gwd_view_desc);\n' +
                   "".join("case %d: return offsetof(gwd_view_desc, %s);\n" % (k + 1, n) for k, n in enumerate(fields)) +
                   "default: return -1; } }\n")
    out = str(tmp_path / "liblayout.so")
    subprocess.check_call(["gcc", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"), str(src), "-o", out])
    layout = ctypes.CDLL(out).layout
    layout.restype = ctypes.c_long
    D = hip.ViewDesc
    assert [layout(k) for k in range(len(fields) + 1)] == [ctypes.sizeof(D)] + [getattr(D, n).offset for n in fields]
    assert len(fields) == 22


def test_workspace_query_and_refusals_before_any_launch():
    """Every call below must return before the launch: this host has no device to launch on."""
    lib = hip.HipLibrary()
    assert lib.version() == 10
    assert lib.workspace_bytes(hip.WS_VIEW, 4, 61, 53) == 4 * 61 * 53 * 8            # the z-buffer: 8 bytes per pixel
    assert lib.workspace_bytes(hip.WS_VIEW, 1, 1, 1) == 16 and lib.workspace_bytes(hip.WS_VIEW, 3, 3, 7) == 512
    assert lib.workspace_bytes(hip.WS_VIEW, 16, 16384, 16384) == 16 * 16384 * 16384 * 8
    for dims in ((0, 8, 8), (17, 8, 8), (1, 0, 8), (1, 8, 0), (1, 16385, 8), (1, 8, 16385), (1, 8), (1, 8, 8, 8)):
        with pytest.raises(ValueError):
            lib.workspace_bytes(hip.WS_VIEW, *dims)
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(buf, ctypes.c_void_p).value
    p += (-p) % 16
    pointers = ("cloud", "cloud_offsets", "sizes", "intrinsics", "poses", "workspace", "view_depth", "view_index", "view_labels", "view_rgb")

    def call(**kw):
        d = hip.ViewDesc()
        for n in pointers:
            setattr(d, n, p)
        d.min_depth, d.max_depth, d.footprint, d.rows = 1e-3, 10.0, 0.05, 8
        d.n_offsets, d.V, d.Fh, d.Fw, d.max_splat, d.keep = 2, 2, 8, 8, 32, 0
        for v in range(2):
            d.ext_h[v] = d.ext_w[v] = 8
        for k, v in kw.items():
            if k in ("ext_h", "ext_w"):
                getattr(d, k)[1] = v
            else:
                setattr(d, k, v)
        return lib.lib.gwd_cloud_view(ctypes.byref(d), None)

    assert lib.lib.gwd_cloud_view(None, None) == -1
    for n in pointers:
        if n != "poses":                                  # poses may be absent: that call would be launched
            assert call(**{n: None}) == -1, n
    for kw in (dict(V=0), dict(V=17), dict(Fh=0), dict(Fw=0), dict(Fh=16385), dict(Fw=16385), dict(rows=0), dict(rows=2 ** 31), dict(n_offsets=1),
               dict(n_offsets=0), dict(ext_h=0), dict(ext_w=0), dict(ext_h=9), dict(ext_w=9)):
        assert call(**kw) == -1, kw
    for kw in (dict(keep=3), dict(keep=-1), dict(max_splat=0), dict(max_splat=65), dict(footprint=math.nan), dict(footprint=-1e-9),
               dict(footprint=math.inf), dict(min_depth=0.0), dict(min_depth=-1.0), dict(min_depth=math.nan), dict(max_depth=math.nan),
               dict(max_depth=math.inf), dict(min_depth=11.0)):
        assert call(**kw) == -2, kw
    for kw in (dict(cloud=p + 8), dict(cloud_offsets=p + 2), dict(sizes=p + 2), dict(intrinsics=p + 4), dict(poses=p + 4), dict(workspace=p + 8),
               dict(view_depth=p + 8), dict(view_index=p + 8), dict(view_labels=p + 2), dict(view_rgb=p + 2)):
        assert call(**kw) == -3, kw
    assert call(V=0, keep=3, cloud=p + 8) == -1 and call(keep=3, cloud=p + 8) == -2      # the order of the file


# ------------------------------------------------------------------------------------------------------------------ host logic
@pytest.fixture
def fake(monkeypatch):
    lib = ViewFakeDevice()
    upload = data.upload_tables

    def counted(host, device):
        lib.calls["upload_tables"] += 1
        return upload(host, device)

    monkeypatch.setattr(data, "upload_tables", counted)
    hip.set_library(lib)
    yield lib
    hip.set_library(None)


T = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a))
N = lambda res: {k: v.numpy() for k, v in res.items()}


def test_cloud_view_through_the_stand_in(fake):
    for name in ("integer_edge", "depth_bounds", "turned", "small_view", "keep_glass"):
        inp = K.edge_inputs(K.EDGES[name])
        res = ops.cloud_view(T(inp["cloud"]), T(inp["cloud_offsets"]), inp["intrinsics"].tolist(), inp["sizes"].tolist(),
                             poses=None if inp["poses"] is None else inp["poses"].tolist(), plane=inp["plane"], **inp["options"])
        assert tuple(res) == ops.VIEW_KEYS
        assert [t.dtype for t in res.values()] == [torch.float32, torch.uint8, torch.int32, torch.uint8]
        K.same(N(res), K.edge_expected(K.EDGES[name]), name)
    # sizes as a tensor next to the cloud: plane is needed, view_sizes is what the host knows
    inp = K.edge_inputs(K.EDGES["ext_clamp"])
    args = (T(inp["cloud"]), T(inp["cloud_offsets"]), T(inp["intrinsics"]), T(inp["sizes"]))
    with pytest.raises(ValueError, match="plane"):
        ops.cloud_view(*args, footprint=2.0)
    res = ops.cloud_view(*args, plane=inp["plane"], view_sizes=inp["ext"], footprint=2.0)
    K.same(N(res), K.edge_expected(K.EDGES["ext_clamp"]), "ext_clamp")
    assert fake.view_calls[-1]["ext"] == [(4, 4)] and fake.view_calls[-1]["plane"] == (8, 8)
    # plane defaults to the largest fh and fw
    cams, poses, sizes = K.fixture_cameras()
    whole = SK.fixture_clouds()[0]
    res = ops.cloud_view(T(whole[0]), T(whole[1]), cams, sizes.tolist(), poses=poses, **K.DEPTHS)
    assert res["view_depth"].shape == (4,) + CK.PLANE
    K.same(N(res), K.fixture_whole_view(), "whole")
    again = ops.cloud_view(T(whole[0]), T(whole[1]), cams, sizes.tolist(), poses=poses, **K.DEPTHS)
    assert again["view_depth"].data_ptr() != res["view_depth"].data_ptr()             # fresh tensors
    # a cloud of no rows: the one-row stand-in, empty planes
    n = len(fake.view_calls)
    res = ops.cloud_view(torch.zeros((0, 32), dtype=torch.uint8), torch.zeros(2, dtype=torch.int32), [K.UNIT_CAM], [(3, 5)])
    assert fake.view_calls[n]["rows"] == 1 and res["view_depth"].shape == (1, 3, 5)
    assert not res["view_depth"].any() and (res["view_index"] == -1).all() and (res["view_labels"] == 255).all() and not res["view_rgb"].any()
    assert ops.check_view_options() == dict(min_depth=1e-3, max_depth=10.0, footprint=0.0, max_splat=32, keep="all")


def test_argument_errors_raise_before_anything_is_launched(fake):
    cloud, off = (T(a) for a in SK.fixture_clouds()[0])
    cams, sizes = [K.UNIT_CAM], [(8, 8)]
    for kw in (dict(min_depth=0.0), dict(min_depth=-1.0), dict(min_depth=2.0, max_depth=1.0), dict(max_depth=math.inf), dict(min_depth=math.nan),
               dict(footprint=-0.1), dict(footprint=math.nan), dict(footprint=math.inf), dict(max_splat=0), dict(max_splat=65), dict(keep="mirrors")):
        with pytest.raises(ValueError):
            ops.cloud_view(cloud, off, cams, sizes, **kw)
    for kw in (dict(max_splat=2.5), dict(max_splat=True), dict(footprint="0.1"), dict(min_depth=None), dict(stride=2)):
        with pytest.raises(TypeError):
            ops.cloud_view(cloud, off, cams, sizes, **kw)
    for c, o in ((cloud.int(), off), (cloud[:, :31], off), (cloud.numpy(), off), (cloud, off.long()), (cloud, off.tolist())):
        with pytest.raises(TypeError):
            ops.cloud_view(c, o, cams, sizes)
    for a in ((cloud, off[:1], cams, sizes), (cloud, off.view(1, 2), cams, sizes), (cloud, off, [K.UNIT_CAM[:3]], sizes), (cloud, off, [K.UNIT_CAM] * 17, sizes * 17),
              (cloud, off, cams, sizes * 2), (cloud, off, cams, [(0, 8)]), (cloud, off, cams, [(8, 8, 8)])):
        with pytest.raises(ValueError):
            ops.cloud_view(*a)
    for kw in (dict(poses=[K.IDENTITY] * 2), dict(plane=(0, 8)), dict(plane=(8, 16385)), dict(plane=(8,))):
        with pytest.raises(ValueError):
            ops.cloud_view(cloud, off, cams, sizes, **kw)
    with pytest.raises(TypeError):
        ops.cloud_view(cloud, off, cams, torch.tensor(sizes, dtype=torch.int64), plane=(8, 8))
    m = PC.SceneMap(0.1, 10, device="cpu")
    n = len(fake.scene_calls)
    for kw, err in ((dict(min_obs=0), ValueError), (dict(keep="x"), ValueError), (dict(footprint=-1.0), ValueError), (dict(max_splat=99), ValueError),
                    (dict(stride=2), TypeError), (dict(min_obs="2"), TypeError)):
        with pytest.raises(err):
            m.view(cams, sizes, **kw)
    assert fake.view_calls == [] and len(fake.scene_calls) == n
    # the binding's own checks
    new = lambda shape, dt: torch.zeros(shape, dtype=dt)
    good = dict(cloud=cloud, cloud_offsets=off, sizes=new((1, 2), torch.int32), intrinsics=new((1, 4), torch.float64), poses=None, view_sizes=None,
                min_depth=1e-3, max_depth=10.0, footprint=0.0, max_splat=32, keep="all", workspace=new((512,), torch.uint8),
                view_depth=new((1, 8, 8), torch.float32), view_index=new((1, 8, 8), torch.int32), view_labels=new((1, 8, 8), torch.uint8),
                view_rgb=new((1, 8, 8, 3), torch.uint8))
    assert hip.HipLibrary.view_desc(**good).rows == cloud.shape[0]
    for kw in (dict(view_depth=new((1, 8, 8), torch.float64)), dict(view_index=new((1, 8, 8), torch.int64)), dict(intrinsics=new((1, 4), torch.float32)),
               dict(sizes=new((1, 2), torch.int64)), dict(cloud=cloud.int())):
        with pytest.raises(TypeError):
            hip.HipLibrary.view_desc(**dict(good, **kw))
    for kw in (dict(view_index=new((1, 8, 9), torch.int32)), dict(view_rgb=new((1, 8, 8, 4), torch.uint8)), dict(sizes=new((2, 2), torch.int32)),
               dict(poses=new((2, 3, 4), torch.float64)), dict(view_labels=new((1, 8, 16), torch.uint8)[:, :, ::2]), dict(max_splat=0), dict(keep="x"),
               dict(footprint=-1.0), dict(min_depth=0.0), dict(view_sizes=[(0, 8)]), dict(view_sizes=[(8, 8)] * 2), dict(cloud=cloud[:0]),
               dict(workspace=None)):
        with pytest.raises(ValueError):
            hip.HipLibrary.view_desc(**dict(good, **kw))
    with pytest.raises(ValueError, match="workspace"):
        fake.cloud_view(**dict(good, workspace=new((511,), torch.uint8)))


def test_scene_map_view_through_the_stand_in(fake):
    _, parts = SK.fixture_clouds()
    cams, poses, sizes = K.fixture_cameras()
    m = PC.SceneMap(0.05, SK.FIXTURE_MAX_VOXELS, device="cpu")
    for part in parts:
        m.integrate(T(part[0]), T(part[1]))
    before, n = m.state(), len(fake.scene_calls)
    res = m.view(cams, sizes.tolist(), poses=poses, max_splat=K.MAP_SPLAT, **K.DEPTHS)
    assert tuple(res) == ops.VIEW_KEYS + PC.SCENE_KEYS
    assert [c["what"] for c in fake.scene_calls[n:]] == ["extract"] and m.state() == before          # the map is unchanged
    assert fake.view_calls[-1]["footprint"] == 0.05 and fake.view_calls[-1]["rows"] == SK.FIXTURE_MAX_VOXELS
    got = N(res)
    K.same(got, K.fixture_map_view(0.05), "map view")
    ext = K.fixture_map(0.05)
    for k in PC.SCENE_KEYS:
        assert got[k].tobytes() == ext[k].tobytes(), k
    # view_index leads into voxel_stats
    hit = got["view_index"] >= 0
    assert (got["voxel_stats"][got["view_index"][hit], 0] >= 1).all()
    # min_obs and keep choose the voxels; footprint and the bounds are the view's
    res = m.view(cams, sizes.tolist(), poses=poses, min_obs=2, keep="glass", footprint=0.1, max_splat=5, **K.DEPTHS)
    ext = S.merge(parts, 0.05, SK.FIXTURE_MAX_VOXELS, min_obs=2, keep="glass")
    K.same(N(res), W.cloud_view(ext["cloud"], ext["cloud_offsets"], cams, sizes, poses, *CK.PLANE, footprint=0.1, max_splat=5, **K.DEPTHS), "filtered")
    assert fake.view_calls[-1]["keep"] == "all" and fake.scene_calls[-1]["keep"] == "glass"
    # an overflowed map: empty planes, never a partial picture
    small = PC.SceneMap(0.1, 63, slots=64, device="cpu")
    small.integrate(*(T(a) for a in SK.as_cloud(SK.distinct_voxels(64))))
    res = small.view([K.UNIT_CAM], [(8, 8)], max_depth=100.0)
    assert (res["view_index"] == -1).all() and not res["view_depth"].any() and res["cloud_offsets"].tolist() == [0, 0]


# ------------------------------------------------------------------------------------------------------------------ the session
POSES = [K.TURN, [[1.0, 0.0, 0.0, 0.5], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0]], [[1.0, 0.0, 0.0, 0.0], [0.0, 0.0, -1.0, 0.0], [0.0, 1.0, 0.0, 0.25]]]
SCENE = dict(voxel=0.25, max_voxels=4096, origin=(0.0, 0.5, 0.0))


def cams_of(frames):
    return [(60.0, 61.0, w / 2.0, h / 2.0) for h, w in (f.shape[:2] for f in frames)]


def test_sessions_without_scene_view_record_the_calls_they_record_today(fake):
    frames = frames_of(3)
    sess = InferenceSession(TinyModel(), compute_dtype=torch.float32, graph=False, cloud=True)
    res = sess.predict_frames(frames, size=48, max_size=64, intrinsics=cams_of(frames), poses=POSES)
    assert fake.calls == dict(BUDGET, gather2d_batch=0) and len(fake.cloud_calls) == 1 and fake.scene_calls == [] and fake.view_calls == []
    assert sorted(res) == sorted(RESULT_KEYS + ("net_sizes",) + CLOUD_KEYS)
    sess = InferenceSession(TinyModel(), compute_dtype=torch.float32, graph=False, cloud={"stride": 2}, scene=dict(SCENE))
    assert sess.scene_view is None
    for _ in range(2):
        res = sess.predict_frames(frames, size=48, max_size=64, intrinsics=cams_of(frames), poses=POSES)
        assert sorted(res) == sorted(RESULT_KEYS + ("net_sizes",) + CLOUD_KEYS)
    assert fake.view_calls == [] and [c["what"] for c in fake.scene_calls] == ["reset", "integrate", "integrate"] and len(fake.cloud_calls) == 3


def test_session_views_the_map_before_it_integrates(fake):
    sess = InferenceSession(TinyModel(), compute_dtype=torch.float32, graph=False, cloud={"stride": 2}, scene=dict(SCENE),
                            scene_view=dict(max_splat=8))
    assert sess.scene_view == dict(min_obs=1, keep="all", footprint=None, max_splat=8)
    plain = InferenceSession(TinyModel(), compute_dtype=torch.float32, graph=False, cloud={"stride": 2})
    frames = frames_of(3)
    sizes = [f.shape[:2] for f in frames]
    ref = S.SceneMap(SCENE["voxel"], SCENE["max_voxels"], SCENE["origin"])
    for k in range(2):
        res = sess.predict_frames(frames, size=48, max_size=64, intrinsics=cams_of(frames), poses=POSES)
        assert sorted(res) == sorted(RESULT_KEYS + ("net_sizes",) + CLOUD_KEYS + SCENE_VIEW_KEYS)
        plane = tuple(res["depth"].shape[1:])
        call = fake.view_calls[-1]
        assert call["plane"] == plane and call["ext"] == [tuple(s) for s in sizes] and call["footprint"] == 0.25 and call["max_splat"] == 8
        assert (call["min_depth"], call["max_depth"]) == (sess.min_depth, sess.max_depth) and call["rows"] == SCENE["max_voxels"]
        assert call["after"] == (2 * k + 1, 2 * k + 2)    # (`plain` calls point_cloud too) behind this call's cloud and the extraction, before its integration
        ext = ref.extract()
        want = W.cloud_view(ext["cloud"], ext["cloud_offsets"], np.asarray(cams_of(frames)), np.asarray(sizes, np.int32),
                            np.asarray(POSES), *plane, min_depth=sess.min_depth, max_depth=sess.max_depth, footprint=0.25, max_splat=8)
        got = {src: res[key].numpy() for key, src in zip(SCENE_VIEW_KEYS, W.KEYS + ("cloud", "cloud_offsets", "voxel_stats"))}
        K.same(got, dict(want, **ext), "call %d" % k)
        for key in PC.SCENE_KEYS:
            assert got[key].tobytes() == ext[key].tobytes(), key
        covered = int((got["view_index"] >= 0).sum())
        assert covered == 0 if k == 0 else covered > 100  # the first call looks at an empty map
        ref.integrate(res["cloud"].numpy(), res["cloud_offsets"].numpy())
        base = plain.predict_frames(frames, size=48, max_size=64, intrinsics=cams_of(frames), poses=POSES)
        for key in base:
            assert torch.equal(base[key], res[key]), key
    assert [c["what"] for c in fake.scene_calls] == ["reset", "extract", "integrate", "extract", "integrate"]
    assert sess.scene.check()["serial"] == 2
    # a call without intrinsics returns what it returns today and looks at nothing
    n = len(fake.view_calls)
    bare = sess.predict_frames(frames, size=48, max_size=64)
    assert sorted(bare) == sorted(RESULT_KEYS + ("net_sizes",)) and len(fake.view_calls) == n and len(fake.scene_calls) == 5


def test_session_scene_view_options_are_validated(fake):
    mk = lambda **kw: InferenceSession(TinyModel(), compute_dtype=torch.float32, graph=False, **kw)
    with pytest.raises(ValueError, match="scene="):
        mk(scene_view=True)
    with pytest.raises(ValueError, match="scene="):
        mk(cloud=True, scene_view=dict(min_obs=2))
    n = len(fake.scene_calls)
    for view, err in ((1, TypeError), ("all", TypeError), (dict(voxel=0.1), TypeError), (dict(min_depth=0.5), TypeError), (dict(min_obs=0), ValueError),
                      (dict(min_obs=1.5), TypeError), (dict(keep="panes"), ValueError), (dict(footprint=-0.5), ValueError),
                      (dict(max_splat=0), ValueError), (dict(max_splat=65), ValueError), (dict(max_splat=2.5), TypeError)):
        with pytest.raises(err):
            mk(cloud=True, scene=dict(SCENE), scene_view=view)
    assert fake.view_calls == [] and all(c["what"] == "reset" for c in fake.scene_calls[n:])
    sess = mk(cloud=True, scene=dict(SCENE), scene_view=True)
    assert sess.scene_view == dict(min_obs=1, keep="all", footprint=None, max_splat=32)
    sess = mk(cloud=True, scene=dict(SCENE), scene_view=dict(min_obs=3, keep="glass", footprint=0.0, max_splat=64))
    assert sess.scene_view == dict(min_obs=3, keep="glass", footprint=0.0, max_splat=64)
    assert infer._SCENE_OPTIONS == ("voxel", "max_voxels", "origin", "slots") and infer._SCENE_VIEW_OPTIONS == ("min_obs", "keep", "footprint", "max_splat")
