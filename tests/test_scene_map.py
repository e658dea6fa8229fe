"""CPU: the statement of the scene map (tests/scene_ref.py) against an independent np.unique / np.add.at formulation, against
hand-computed edge cases and against the fixture tests/golden/scene_map.npz; the ABI of gwd_scene_* (header, binding, descriptor
layout, refusals before any launch); cloud.SceneMap, ops.scene_merge and InferenceSession(scene=) through the stand-in library
(tests/scene_fake.py); the PLY round trip of an extracted map."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest
import torch

from gw_depth_amd import cloud as PC
from gw_depth_amd import data, hip, infer, ops
from gw_depth_amd.infer import CLOUD_KEYS, RENDER_KEYS, RESULT_KEYS, InferenceSession
from tests import cloud_ref as C
from tests import scene_cases as K
from tests import scene_ref as S
from tests.scene_fake import SceneFakeDevice
from tests.test_frames_post import BUDGET, TinyModel, frames_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("cloud", "cloud_offsets", "voxel_stats")


def same(a, b, what=""):
    for k in KEYS:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), (what, k)


def unique_merge(clouds, voxel, max_voxels, origin=(0.0, 0.0, 0.0), min_obs=1, keep="all"):
    """The second formulation: every call's rows in one array, np.unique over the keys, np.add.at for the sums, array arithmetic for
    the records.  No overflow rule (the inputs here stay below max_voxels)."""
    recs = np.concatenate([np.ascontiguousarray(c).view(C.RECORD).ravel()[:int(o[-1])] for c, o in clouds])
    serial = np.concatenate([np.full(int(o[-1]), k, dtype=np.int64) for k, (c, o) in enumerate(clouds)])
    with np.errstate(all="ignore"):
        t = (recs["xyz"].astype(np.float64) - np.asarray(origin, dtype=np.float64)) / np.float64(voxel)
        i = np.floor(t)
        ok = ((recs["flags"] & 1) != 0) & np.isfinite(recs["xyz"]).all(1) & ((i >= -2 ** 20) & (i < 2 ** 20)).all(1)
    recs, serial, t, i = recs[ok], serial[ok], t[ok], i[ok]
    q = np.floor((t - i) * 65536.0).astype(np.int64)
    idx = i.astype(np.int64)
    key = (idx[:, 0] + 2 ** 20) | (idx[:, 1] + 2 ** 20) << 21 | (idx[:, 2] + 2 ** 20) << 42
    uniq, first, inverse = np.unique(key, return_index=True, return_inverse=True)
    rank = np.empty(len(uniq), dtype=np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(len(uniq))          # rows are in (serial, row) order: first index = birth
    g = rank[inverse.ravel()]
    V = len(uniq)
    index = np.zeros((V, 3), dtype=np.int64)
    index[g] = idx
    n = np.bincount(g, minlength=V).astype(np.int64)
    sum_q = np.zeros((V, 3), dtype=np.int64)
    np.add.at(sum_q, g, q)
    with np.errstate(invalid="ignore"):
        has_n = ((recs["flags"] & 2) != 0) & (np.abs(recs["normal"]) <= 2.0).all(1)
    has_c = (recs["flags"] & 8) != 0
    n_normal, n_colour = np.bincount(g[has_n], minlength=V), np.bincount(g[has_c], minlength=V)
    sum_n, sum_rgb = np.zeros((V, 3), dtype=np.int64), np.zeros((V, 3), dtype=np.int64)
    np.add.at(sum_n, g[has_n], np.rint(recs["normal"][has_n].astype(np.float64) * 32767.0).astype(np.int64))
    np.add.at(sum_rgb, g[has_c], recs["rgb"][has_c].astype(np.int64))
    n_glass = np.bincount(g[recs["label"] == 1], minlength=V)
    first_seen, last_seen = np.full(V, 2 ** 40), np.full(V, -1)
    np.minimum.at(first_seen, g, serial)
    np.maximum.at(last_seen, g, serial)
    label = (2 * n_glass >= n).astype(np.uint8)
    sel = (n >= min_obs) & {"all": np.ones(V, bool), "glass": label == 1, "non_glass": label != 1}[keep]
    out = np.zeros(max_voxels, dtype=C.RECORD)
    stats = np.zeros((max_voxels, 4), dtype=np.int32)
    kept = int(sel.sum())
    o = out[:kept]
    o["xyz"] = (((index[sel] + (sum_q[sel] / n[sel, None].astype(np.float64) + 0.5) / 65536.0) * np.float64(voxel))
                + np.asarray(origin, dtype=np.float64)).astype(np.float32)
    s = sum_n[sel].astype(np.float64)
    length = np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2])
    with_normal = (n_normal[sel] > 0) & (sum_n[sel] != 0).any(1)
    o["normal"][with_normal] = (s[with_normal] / length[with_normal, None]).astype(np.float32)
    with_colour = n_colour[sel] > 0
    nc = np.maximum(n_colour[sel], 1)[:, None]
    o["rgb"][with_colour] = ((2 * sum_rgb[sel] + nc) // (2 * nc))[with_colour]
    o["label"] = label[sel]
    o["flags"] = 1 | 16 | np.where(with_normal, 2, 0) | np.where(with_colour, 8, 0)
    stats[:kept] = np.stack([n[sel], n_glass[sel], first_seen[sel], last_seen[sel]], axis=1)
    return {"cloud": out.view(np.uint8).reshape(max_voxels, 32), "cloud_offsets": np.array([0, kept], dtype=np.int32), "voxel_stats": stats}


# ------------------------------------------------------------------------------------------------------------------ the statement
@pytest.mark.parametrize("voxel", K.VOXELS)
def test_statement_equals_the_unique_formulation_and_the_fixture(voxel):
    whole, parts = K.fixture_clouds()
    total = int(whole[1][-1])
    assert total > 2 * hip.SCENE_TILE and total % hip.SCENE_TILE != 0
    gold = K.load_golden()
    for split in (False, True):
        clouds = parts if split else [whole]
        res = S.merge(clouds, voxel, K.FIXTURE_MAX_VOXELS)
        same(res, unique_merge(clouds, voxel, K.FIXTURE_MAX_VOXELS), (voxel, split))
        kept = int(res["cloud_offsets"][1])
        gid = K.golden_id(voxel, split)
        assert gold[gid + ".cloud"].shape == (kept, 32) and gold[gid + ".cloud"].tobytes() == res["cloud"][:kept].tobytes()
        assert gold[gid + ".voxel_stats"].tobytes() == res["voxel_stats"][:kept].tobytes()
        assert not res["cloud"][kept:].any() and not res["voxel_stats"][kept:].any()
        for opt in (dict(min_obs=2), dict(keep="glass"), dict(keep="non_glass", min_obs=3)):
            same(S.merge(clouds, voxel, K.FIXTURE_MAX_VOXELS, **opt), unique_merge(clouds, voxel, K.FIXTURE_MAX_VOXELS, **opt), (voxel, split, opt))
    # the fixture merges: fewer voxels than points at the two larger sizes, voxels seen from more than one frame, both labels
    res = S.merge(parts, voxel, K.FIXTURE_MAX_VOXELS)
    kept = int(res["cloud_offsets"][1])
    st = res["voxel_stats"][:kept]
    assert st[:, 0].sum() == total and (voxel == 0.02 or kept < total)
    rec = res["cloud"].view(C.RECORD).ravel()[:kept]
    assert set(rec["label"]) == {0, 1} and (rec["flags"] & 16).all() and (voxel == 0.02 or (st[:, 3] > st[:, 2]).any())


@pytest.mark.parametrize("voxel", K.VOXELS)
def test_a_then_b_is_a_and_b_at_once(voxel):
    whole, parts = K.fixture_clouds()
    one, three = S.merge([whole], voxel, K.FIXTURE_MAX_VOXELS), S.merge(parts, voxel, K.FIXTURE_MAX_VOXELS)
    assert one["cloud"].tobytes() == three["cloud"].tobytes() and np.array_equal(one["cloud_offsets"], three["cloud_offsets"])
    assert np.array_equal(one["voxel_stats"][:, :2], three["voxel_stats"][:, :2])
    assert not one["voxel_stats"][:, 2:].any() and three["voxel_stats"][:, 3].max() == 3


def test_a_row_permutation_changes_the_order_only():
    whole, _ = K.fixture_clouds()
    total = int(whole[1][-1])
    rec = whole[0].view(C.RECORD).ravel()[:total]
    shuffled = K.as_cloud(rec[np.random.default_rng(1).permutation(total)])
    a, b = S.merge([whole], 0.05, K.FIXTURE_MAX_VOXELS), S.merge([shuffled], 0.05, K.FIXTURE_MAX_VOXELS)
    kept = int(a["cloud_offsets"][1])
    assert kept == int(b["cloud_offsets"][1]) and a["cloud"].tobytes() != b["cloud"].tobytes()
    rows = lambda r: sorted(bytes(c) + bytes(s) for c, s in zip(r["cloud"][:kept], r["voxel_stats"][:kept]))
    assert rows(a) == rows(b)


@pytest.mark.parametrize("name", list(K.EDGES))
def test_arithmetic_edges_by_hand(name):
    case = K.EDGES[name]
    m = S.SceneMap(case["voxel"], K.EDGE_MAX_VOXELS, case.get("origin", K.ORIGIN))
    cloud, offsets = K.edge_cloud(case)
    m.integrate(cloud, offsets)
    same(m.extract(**case.get("options", {})), K.edge_expected(case), name)
    n = len(case["points"])
    assert m.state() == dict(serial=1, count=m.state()["count"], points=n - case.get("dropped", 0), dropped=case.get("dropped", 0), status=0)
    if "options" not in case:
        assert m.state()["count"] == len(case["want"])


def test_overflow_is_an_empty_map_never_a_truncated_one():
    rec = K.distinct_voxels(64)
    m = S.SceneMap(0.1, 63)
    m.integrate(*K.as_cloud(rec[:63]))
    assert m.state() == dict(serial=1, count=63, points=63, dropped=0, status=0) and int(m.extract()["cloud_offsets"][1]) == 63
    m.integrate(*K.as_cloud(rec[:63]))                    # the same voxels again: still fine
    assert m.state()["count"] == 63 and m.state()["status"] == 0 and (m.extract()["voxel_stats"][:, 0] == 2).all()
    m.integrate(*K.as_cloud(rec[63:]))
    assert m.state() == dict(serial=3, count=63, points=126, dropped=0, status=1)
    out = m.extract()
    assert not out["cloud"].any() and not out["voxel_stats"].any() and out["cloud_offsets"].tolist() == [0, 0]
    m.integrate(*K.as_cloud(rec[:1]))
    assert m.state()["serial"] == 4 and m.state()["status"] == 1
    m.reset()
    m.integrate(*K.as_cloud(rec[:63]))
    assert m.state() == dict(serial=1, count=63, points=63, dropped=0, status=0)


# ------------------------------------------------------------------------------------------------------------------ the ABI
def test_header_binding_and_makefile_agree(tmp_path):
    header = open(os.path.join(ROOT, "include", "gwdepth.h")).read()
    for name, value in (("GWD_SCENE_TILE", hip.SCENE_TILE), ("GWD_SCENE_VOXEL_BYTES", hip.SCENE_VOXEL_BYTES),
                        ("GWD_SCENE_MAX_VOXELS", hip.SCENE_MAX_VOXELS), ("GWD_SCENE_FLAG_MERGED", hip.SCENE_FLAG_MERGED)):
        assert "#define %s %d" % (name, value) in header, name
    assert "GWD_WS_SCENE = %d" % hip.WS_SCENE in header and hip.WS_SCENE == 8 and "#define GWD_VERSION 10" in header
    assert {"gwd_scene_reset", "gwd_scene_integrate", "gwd_scene_extract"} <= set(hip.ENTRY_POINTS)
    assert PC.FLAG_MERGED == S.MERGED == 16 and hip.SCENE_MAX_VOXELS == S.MAX_VOXELS and hip.SCENE_STATE == S.STATE_KEYS
    assert PC.SCENE_KEYS == ops.SCENE_KEYS == KEYS
    assert "scene.hip" in open(os.path.join(ROOT, "gw_depth_amd", "csrc", "Makefile")).read()
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include "gwdepth.h"\n'
                   'long layout(int k) { switch (k) { case 0: return sizeof(gwd_scene_desc); case 1: return offsetof(gwd_scene_desc, state);\n'
                   'case 2: return offsetof(gwd_scene_desc, voxel); case 3: return offsetof(gwd_scene_desc, origin);\n'
                   'case 4: return offsetof(gwd_scene_desc, max_voxels); case 5: return offsetof(gwd_scene_desc, slots); default: return -1; } }\n')
    out = str(tmp_path / "liblayout.so")
    subprocess.check_call(["gcc", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"), str(src), "-o", out])
    layout = ctypes.CDLL(out).layout
    layout.restype = ctypes.c_long
    D = hip.SceneDesc
    assert [layout(k) for k in range(6)] == [ctypes.sizeof(D), D.state.offset, D.voxel.offset, D.origin.offset, D.max_voxels.offset, D.slots.offset]


def test_workspace_query_and_refusals_before_any_launch():
    """Every call below must return before the launch: this host has no device to launch on."""
    lib = hip.HipLibrary()
    assert lib.version() == 10
    # integrate: a header, a slot per row, the tiles' births (+ 1) and drops; extract: the tiles' counts + 1
    assert lib.workspace_bytes(hip.WS_SCENE, 2629, 63) == 32 + 10528 + 16 + 16
    assert lib.workspace_bytes(hip.WS_SCENE, 1, 1 << 27) == ((1 << 17) + 1) * 4 + 12
    for dims in ((0, 8), (2 ** 31, 8), (8, 0), (8, (1 << 27) + 1), (8,), (8, 8, 8)):
        with pytest.raises(ValueError):
            lib.workspace_bytes(hip.WS_SCENE, *dims)
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(buf, ctypes.c_void_p).value
    p += (-p) % 16

    def desc(**kw):
        d = hip.SceneDesc()
        d.keys = d.marks = d.ranks = d.voxels = d.state = p
        d.voxel, d.max_voxels, d.slots = 0.05, 63, 64
        for k, v in kw.items():
            if k == "origin":
                d.origin[0] = v
            else:
                setattr(d, k, v)
        return d

    L = lib.lib
    calls = (lambda d: L.gwd_scene_reset(ctypes.byref(d), None),
             lambda d: L.gwd_scene_integrate(ctypes.byref(d), p, p, 8, 2, p, None),
             lambda d: L.gwd_scene_extract(ctypes.byref(d), 1, 0, p, p, p, p, None))
    assert L.gwd_scene_reset(None, None) == -1 and L.gwd_scene_integrate(None, p, p, 8, 2, p, None) == -1
    assert L.gwd_scene_extract(None, 1, 0, p, p, p, p, None) == -1
    for call in calls:
        for k in ("keys", "marks", "ranks", "voxels", "state"):
            assert call(desc(**{k: None})) == -1, k
        for kw in (dict(max_voxels=0), dict(max_voxels=(1 << 27) + 1, slots=1 << 28), dict(slots=63), dict(slots=96), dict(slots=32), dict(slots=1 << 29, max_voxels=1 << 27)):
            assert call(desc(**kw)) == -1, kw
        for kw in (dict(voxel=0.0), dict(voxel=-1.0), dict(voxel=math.nan), dict(voxel=math.inf), dict(origin=math.nan), dict(origin=-math.inf)):
            assert call(desc(**kw)) == -2, kw
        for kw in (dict(keys=p + 4), dict(marks=p + 4), dict(ranks=p + 2), dict(voxels=p + 8), dict(state=p + 4)):
            assert call(desc(**kw)) == -3, kw
    d = desc()
    integrate = lambda cloud=p, off=p, rows=8, n=2, ws=p: L.gwd_scene_integrate(ctypes.byref(d), cloud, off, rows, n, ws, None)
    assert integrate(cloud=None) == -1 and integrate(off=None) == -1 and integrate(ws=None) == -1 and integrate(rows=0) == -1
    assert integrate(rows=2 ** 31) == -1 and integrate(n=1) == -1
    assert integrate(cloud=p + 8) == -3 and integrate(off=p + 2) == -3 and integrate(ws=p + 8) == -3
    extract = lambda min_obs=1, keep=0, ws=p, cloud=p, off=p, st=p: L.gwd_scene_extract(ctypes.byref(d), min_obs, keep, ws, cloud, off, st, None)
    assert extract(ws=None) == -1 and extract(cloud=None) == -1 and extract(off=None) == -1 and extract(st=None) == -1 and extract(min_obs=0) == -1
    assert extract(keep=3) == -2 and extract(keep=-1) == -2
    assert extract(ws=p + 8) == -3 and extract(cloud=p + 8) == -3 and extract(off=p + 2) == -3 and extract(st=p + 8) == -3


# ------------------------------------------------------------------------------------------------------------------ host logic
@pytest.fixture
def fake(monkeypatch):
    lib = SceneFakeDevice()
    upload = data.upload_tables

    def counted(host, device):
        lib.calls["upload_tables"] += 1
        return upload(host, device)

    monkeypatch.setattr(data, "upload_tables", counted)
    hip.set_library(lib)
    yield lib
    hip.set_library(None)


T = lambda pair: tuple(torch.from_numpy(np.ascontiguousarray(a)) for a in pair)
N = lambda res: {k: v.numpy() for k, v in res.items()}


def test_scene_map_object_through_the_stand_in(fake):
    whole, parts = K.fixture_clouds()
    m = PC.SceneMap(0.05, K.FIXTURE_MAX_VOXELS, device="cpu")
    assert (m.voxel, m.max_voxels, m.origin, m.slots) == (0.05, 5000, (0.0, 0.0, 0.0), 16384)
    assert [c["what"] for c in fake.scene_calls] == ["reset"] and m.state() == dict(serial=0, count=0, points=0, dropped=0, status=0)
    for part in parts:
        assert m.integrate(*T(part)) is m
    res = m.extract()
    assert tuple(res) == PC.SCENE_KEYS and [t.dtype for t in res.values()] == [torch.uint8, torch.int32, torch.int32]
    same(N(res), S.merge(parts, 0.05, K.FIXTURE_MAX_VOXELS), "three calls")
    assert m.check() == dict(serial=4, count=2650, points=4702, dropped=0, status=0)
    again = m.extract(min_obs=2, keep="non_glass")
    assert again["cloud"].data_ptr() != res["cloud"].data_ptr()                       # fresh tensors
    same(N(again), S.merge(parts, 0.05, K.FIXTURE_MAX_VOXELS, min_obs=2, keep="non_glass"))
    # an extraction is a cloud: it can be integrated into a coarser map
    coarse = PC.SceneMap(0.25, 500, origin=(0.5, 0.0, -1.0), slots=512, device="cpu").integrate(res["cloud"], res["cloud_offsets"])
    same(N(coarse.extract()), S.merge([(res["cloud"].numpy(), res["cloud_offsets"].numpy())], 0.25, 500, (0.5, 0.0, -1.0)))
    # a cloud of no rows still counts as a call
    m.integrate(torch.zeros((0, 32), dtype=torch.uint8), torch.zeros(2, dtype=torch.int32))
    assert m.state()["serial"] == 5 and fake.scene_calls[-1]["rows"] == 1
    assert m.reset() is m and m.state()["serial"] == 0 and int(m.extract()["cloud_offsets"][1]) == 0
    # overflow
    small = PC.SceneMap(0.1, 63, slots=64, device="cpu")
    small.integrate(*T(K.as_cloud(K.distinct_voxels(64))))
    with pytest.raises(RuntimeError, match="max_voxels = 63"):
        small.check()
    assert not small.extract()["cloud"].any()


def test_scene_merge_is_the_one_shot_form(fake):
    whole, _ = K.fixture_clouds()
    res = ops.scene_merge(*T(whole), 0.25, max_voxels=300, origin=(0.1, 0.2, 0.3), min_obs=2, keep="glass")
    assert tuple(res) == ops.SCENE_KEYS and [c["what"] for c in fake.scene_calls] == ["reset", "integrate", "extract"]
    same(N(res), S.merge([whole], 0.25, 300, (0.1, 0.2, 0.3), min_obs=2, keep="glass"))
    res = ops.scene_merge(*T(whole), 0.05)                                              # max_voxels: the cloud's rows
    assert res["cloud"].shape[0] == whole[0].shape[0]
    same(N(res), S.merge([whole], 0.05, whole[0].shape[0]))
    assert ops.check_scene_options(0.5, 10) == dict(voxel=0.5, max_voxels=10, origin=(0.0, 0.0, 0.0), slots=32, min_obs=1, keep="all")


def test_argument_errors_raise_before_anything_is_launched(fake):
    cloud, off = T(K.fixture_clouds()[0])
    mk = lambda *a, **kw: PC.SceneMap(*a, device="cpu", **kw)
    for a, kw in (((0.0, 10), {}), ((-0.1, 10), {}), ((math.nan, 10), {}), ((math.inf, 10), {}), ((0.1, 0), {}), ((0.1, (1 << 27) + 1), {}),
                  ((0.1, 10), dict(origin=(0.0, 0.0))), ((0.1, 10), dict(origin=(0.0, math.nan, 0.0))), ((0.1, 10), dict(origin=(0.0, math.inf, 0.0))),
                  ((0.1, 10), dict(slots=8)), ((0.1, 10), dict(slots=24)), ((0.1, 16), dict(slots=16)), ((0.1, 10), dict(slots=1 << 29))):
        with pytest.raises(ValueError):
            mk(*a, **kw)
        with pytest.raises(ValueError):
            ops.scene_merge(cloud, off, a[0], a[1], **kw)
    for a, kw in ((("0.1", 10), {}), ((True, 10), {}), ((0.1, 10.5), {}), ((0.1, True), {}), ((0.1, 10), dict(origin=5)), ((0.1, 10), dict(slots=16.0))):
        with pytest.raises(TypeError):
            mk(*a, **kw)
    for kw in (dict(min_obs=0), dict(min_obs=2 ** 31), dict(keep="mirrors")):
        with pytest.raises(ValueError):
            ops.scene_merge(cloud, off, 0.1, **kw)
    with pytest.raises(TypeError):
        ops.scene_merge(cloud, off, 0.1, min_obs=1.5)
    for c, o in ((cloud.int(), off), (cloud[:, :31], off), (cloud.numpy(), off), (cloud, off.long()), (cloud, off.tolist())):
        with pytest.raises(TypeError):
            ops.scene_merge(c, o, 0.1)
    for c, o in ((cloud, off[:1]), (cloud, off.view(1, 2))):
        with pytest.raises(ValueError):
            ops.scene_merge(c, o, 0.1)
    assert fake.scene_calls == []
    m = mk(0.1, 10)
    n = len(fake.scene_calls)
    for c, o, err in ((cloud.int(), off, TypeError), (cloud, off.long(), TypeError), (cloud, off[:1], ValueError)):
        with pytest.raises(err):
            m.integrate(c, o)
    for kw, err in ((dict(min_obs=0), ValueError), (dict(keep="x"), ValueError), (dict(min_obs="2"), TypeError)):
        with pytest.raises(err):
            m.extract(**kw)
    assert len(fake.scene_calls) == n
    # the binding's own checks
    t = m._tensors
    for bad in ((t[0].int(), t[1], t[2], t[3], t[4]), (t[0], t[1], t[2].long(), t[3], t[4])):
        with pytest.raises(TypeError):
            hip.HipLibrary.scene_desc(*bad, 0.1, (0, 0, 0))
    for bad, voxel in (((t[0][:8], t[1], t[2], t[3], t[4]), 0.1), ((t[0], t[1], t[2], t[3][:, :64], t[4]), 0.1), ((t[0], t[1], t[2], t[3], t[4][:5]), 0.1),
                       (t, 0.0), (t, math.nan)):
        with pytest.raises(ValueError):
            hip.HipLibrary.scene_desc(*bad, voxel, (0, 0, 0))


# ------------------------------------------------------------------------------------------------------------------ the session
def cams(frames):
    return [(60.0, 61.0, w / 2.0, h / 2.0) for h, w in (f.shape[:2] for f in frames)]


TURN = [[[0.0, -1.0, 0.0, 1.0], [1.0, 0.0, 0.0, 2.0], [0.0, 0.0, 1.0, 3.0]], [[1.0, 0.0, 0.0, 0.5], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0]],
        [[1.0, 0.0, 0.0, 0.0], [0.0, 0.0, -1.0, 0.0], [0.0, 1.0, 0.0, 0.25]]]


def test_sessions_without_scene_record_the_calls_they_record_today(fake):
    sess = InferenceSession(TinyModel(), compute_dtype=torch.float32, graph=False, cloud=True)
    assert sess.scene is None
    frames = frames_of(3)
    res = sess.predict_frames(frames, size=48, max_size=64, intrinsics=cams(frames), poses=TURN)
    assert fake.calls == dict(BUDGET, gather2d_batch=0) and len(fake.cloud_calls) == 1 and fake.scene_calls == [] and fake.maps == {}
    assert sorted(res) == sorted(RESULT_KEYS + ("net_sizes",) + CLOUD_KEYS)
    res = sess.predict_frames(frames, size=48, max_size=64, intrinsics=cams(frames))   # no poses: fine without scene=
    assert fake.scene_calls == []


def test_session_integrates_behind_the_cloud_and_before_render(fake):
    sess = InferenceSession(TinyModel(), compute_dtype=torch.float32, graph=False, cloud={"stride": 2}, render=True,
                            scene=dict(voxel=0.25, max_voxels=4096, origin=(0.0, 0.5, 0.0)))
    assert isinstance(sess.scene, PC.SceneMap) and (sess.scene.voxel, sess.scene.max_voxels, sess.scene.origin) == (0.25, 4096, (0.0, 0.5, 0.0))
    plain = InferenceSession(TinyModel(), compute_dtype=torch.float32, graph=False, cloud={"stride": 2}, render=True)
    frames = frames_of(3)
    ref = S.SceneMap(0.25, 4096, (0.0, 0.5, 0.0))
    for k in range(2):
        res = sess.predict_frames(frames, size=48, max_size=64, intrinsics=cams(frames), poses=TURN)
        assert sorted(res) == sorted(RESULT_KEYS + ("net_sizes",) + CLOUD_KEYS + RENDER_KEYS)       # the keys do not change
        rec = fake.scene_calls[-1]
        assert rec["what"] == "integrate" and rec["cloud"] is res["cloud"] and rec["after"] == (2 * k + 1, 2 * k)
        assert fake.render_calls[-1]["after"] is not None and len(fake.render_calls) == 2 * k + 1
        ref.integrate(res["cloud"].numpy(), res["cloud_offsets"].numpy())
        base = plain.predict_frames(frames, size=48, max_size=64, intrinsics=cams(frames), poses=TURN)
        for key in base:
            assert torch.equal(base[key], res[key]), key
    assert [c["what"] for c in fake.scene_calls] == ["reset", "integrate", "integrate"]
    got = N(sess.scene.extract())
    same(got, ref.extract(), "session")
    assert sess.scene.check()["serial"] == 2 and (got["voxel_stats"][:int(got["cloud_offsets"][1]), 3] == 1).all()
    # a call without intrinsics returns what it returns today and leaves the map alone
    bare = sess.predict_frames(frames, size=48, max_size=64)
    assert sorted(bare) == sorted(RESULT_KEYS + ("net_sizes",) + RENDER_KEYS) and len(fake.scene_calls) == 4
    with pytest.raises(ValueError, match="share no world"):
        sess.predict_frames(frames, size=48, max_size=64, intrinsics=cams(frames))
    assert len(fake.scene_calls) == 4 and len(fake.cloud_calls) == 4
    # a map of one's own, shared by two sessions
    shared = PC.SceneMap(0.5, 100, device="cpu")
    a = InferenceSession(TinyModel(), compute_dtype=torch.float32, graph=False, cloud=True, scene=shared)
    assert a.scene is shared


def test_session_scene_options_are_validated(fake):
    mk = lambda **kw: InferenceSession(TinyModel(), compute_dtype=torch.float32, graph=False, **kw)
    with pytest.raises(ValueError, match="cloud="):
        mk(scene=dict(voxel=0.1, max_voxels=10))
    with pytest.raises(ValueError, match="cloud="):
        mk(scene=PC.SceneMap(0.1, 10, device="cpu"))
    n = len(fake.scene_calls)
    for scene, err in ((True, TypeError), (0.05, TypeError), (dict(voxel=0.1), TypeError), (dict(max_voxels=10), TypeError),
                       (dict(voxel=0.1, max_voxels=10, min_obs=2), TypeError), (dict(voxel=0.0, max_voxels=10), ValueError),
                       (dict(voxel=0.1, max_voxels=0), ValueError), (dict(voxel=0.1, max_voxels=10, slots=10), ValueError),
                       (dict(voxel=0.1, max_voxels=10, origin=(0, 0)), ValueError)):
        with pytest.raises(err):
            mk(cloud=True, scene=scene)
    assert len(fake.scene_calls) == n
    assert infer._SCENE_OPTIONS == ("voxel", "max_voxels", "origin", "slots")


# ------------------------------------------------------------------------------------------------------------------ PLY
def test_ply_round_trip_of_an_extracted_map(fake, tmp_path):
    _, parts = K.fixture_clouds()
    m = PC.SceneMap(0.25, 300, device="cpu")
    for part in parts:
        m.integrate(*T(part))
    res = m.extract(min_obs=2)
    kept = int(res["cloud_offsets"][1])
    path = str(tmp_path / "map.ply")
    assert m.save_ply(path, min_obs=2) == kept and 0 < kept < 300
    back = PC.load_ply(path)
    assert back.shape == (kept, 32) and torch.equal(back, res["cloud"][:kept])
    assert PC.save_ply(path, res["cloud"], res["cloud_offsets"]) == kept and torch.equal(PC.load_ply(path), back)
    f = PC.fields(back)
    assert (f["flags"] & PC.FLAG_MERGED).all() and not f["frame"].any() and not f["region"].any() and not f["source"].any()
