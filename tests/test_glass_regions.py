"""CPU: the restatement of the glass-region kernels (tests/regions_ref.py) against scipy.ndimage.label and a hand-written case, the
bound the GPU test holds the plane fit to, and the host logic of ops.glass_regions / InferenceSession(regions=...) /
evaluate_frames(planar=...) through a stand-in library (tests/regions_fake.py)."""
import math
import os
import re

import numpy as np
import pytest
import torch
from scipy import ndimage

from gw_depth_amd import data, hip, ops
from gw_depth_amd.evaluate import evaluate_frames
from gw_depth_amd.infer import REGION_KEYS, RESULT_KEYS, InferenceSession
from tests import regions_ref as R
from tests.regions_fake import RegionsFakeDevice
from tests.test_frames_post import BUDGET, TinyModel, frames_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = R.load_golden()


# ------------------------------------------------------------------------------------------------------------------ the oracle
@pytest.mark.parametrize("connectivity", [8, 4])
@pytest.mark.parametrize("name,mask,mm", GOLDEN, ids=[g[0] for g in GOLDEN])
def test_partition_equals_scipy_label(name, mask, mm, connectivity):
    lab, anchors, areas = R.components(mask, connectivity)
    want, n = ndimage.label(mask, structure=R.STRUCTURE[connectivity])
    assert len(anchors) == n and (lab > 0).tolist() == mask.tolist()
    pairs = np.unique(np.stack([lab.ravel(), want.ravel()]), axis=1)
    assert pairs.shape[1] == n + 1                              # a bijection between the two labellings (background included)
    flat = lab.ravel()
    for k in range(n):                                          # numbered by anchor = smallest raster index, ascending
        assert anchors[k] == np.nonzero(flat == k + 1)[0][0] and areas[k] == int((flat == k + 1).sum())
    assert (np.diff(anchors) > 0).all()


def test_fixture_component_counts():
    counts = {name: [len(R.components(mask, c)[1]) for c in (8, 4)] for name, mask, _ in GOLDEN}
    assert counts == {"large": [293, 298], "small": [17, 18], "medium": [11, 13]}
    _, _, areas = R.components(GOLDEN[0][1], 8)
    assert int((areas >= 100).sum()) == 104 and int(areas.max()) == 1506 and len(areas) - len(set(areas.tolist())) >= 100


def test_ranking_and_records_by_hand():
    rows = ["11.....2",
            "11.....2",
            ".......2",
            "..3.....",
            ".3.3....",
            "........",
            "44444...",
            ".......5"]
    mask = np.array([[c != "." for c in r] for r in rows])
    mm = (np.arange(64, dtype=np.uint16).reshape(8, 8) + 1) * 100
    mm[0, 0], mm[1, 1] = 0, 20000                               # out of range on either side
    labels, depth, sizes = R.batch_of([(mask, mm)])
    out = R.glass_regions(labels, depth, sizes, max_regions=3, min_area=3, connectivity=8)
    # areas: 1 -> 4, 2 -> 3, 3 -> 3 (joined diagonally), 4 -> 5, 5 -> 1; kept: 4 (5), 1 (4), then 2 before 3 by its anchor 7 < 26
    assert out["region_total"].tolist() == [5] and out["region_count"].tolist() == [3]
    rec = {f: out["regions"][0, :, k].tolist() for k, f in enumerate(R.FIELDS)}
    assert rec["area"] == [5, 4, 3] and rec["anchor"] == [48, 0, 7]
    assert (rec["x0"], rec["y0"], rec["x1"], rec["y1"]) == ([0, 0, 7], [6, 0, 0], [4, 1, 7], [6, 1, 2])
    assert rec["sum_x"] == [10, 2, 21] and rec["sum_y"] == [30, 2, 3]
    assert rec["n_depth"] == [5, 2, 3] and rec["sum_mm"] == [4900 + 5000 + 5100 + 5200 + 5300, 200 + 900, 800 + 1600 + 2400]
    assert rec["min_mm"] == [4900, 200, 800] and rec["max_mm"] == [5300, 900, 2400]
    want = np.zeros((8, 8), np.uint8)
    want[6, :5], want[:2, :2], want[:3, 7] = 1, 2, 3
    assert np.array_equal(out["region_map"][0], want)
    four = R.glass_regions(labels, depth, sizes, max_regions=8, min_area=1, connectivity=4)          # region 3 falls apart
    assert four["region_total"].tolist() == [7] and four["regions"][0, :, 0].tolist() == [5, 4, 3, 1, 1, 1, 1, 0]
    assert four["regions"][0, 3:7, 5].tolist() == [26, 33, 35, 63]                                  # equal areas in anchor order
    refused = R.glass_regions(labels, depth, sizes, max_regions=3, min_area=1, connectivity=4, max_candidates=6)
    assert refused["region_count"].tolist() == [-1] and not refused["region_map"].any() and not refused["regions"].any()
    planes = R.region_planes(out["region_map"], depth, out["region_count"], 3)
    assert planes[0, :, 5].tolist() == [1.0, 1.0, 1.0] and planes[0, :, 4].tolist() == [5.0, 2.0, 3.0]  # a row, two pixels, a column


def fit_bound(x, y, w):
    """max |fit - oracle's fit| over a region's pixels: (n + 64 kappa) 2^-52 max |w|."""
    return (len(x) + 64.0 * R.normal_cond(x, y)) * 2.0 ** -52 * float(np.abs(w).max())


def naive_reversed(v):
    s = 0.0
    for t in v[::-1].tolist():
        s += t
    return s


@pytest.mark.parametrize("name,mask,mm", GOLDEN, ids=[g[0] for g in GOLDEN])
def test_moment_route_stays_inside_the_bound_whatever_the_summation(name, mask, mm):
    """The kernel's route to the plane (bbox-relative moments, centred 2 x 2 system) summed exactly (math.fsum) and summed naively
    in reversed raster order, against numpy.linalg.lstsq on centred columns: both inside the bound the GPU test uses."""
    labels, depth, sizes = R.batch_of([(mask, mm)])
    out = R.glass_regions(labels, depth, sizes, 32, 1, 8)
    worst = 0.0
    for r in range(int(out["region_count"][0])):
        x, y, w = R.region_pixels(out["region_map"][0], depth[0], r)
        a, b, c, rms, n, status = R.fit_plane(x, y, w)
        if status:
            continue
        bound = fit_bound(x, y, w)
        for summer in (math.fsum, naive_reversed):
            a2, b2, c2 = R.fit_from_moments(x, y, w, summer)
            err = float(np.abs((a2 * x + b2 * y + c2) - (a * x + b * y + c)).max())
            worst = max(worst, err / bound)
            assert err <= bound, (name, r, summer.__name__, err, bound)
    print("%s: worst error / bound %.3g" % (name, worst))


def test_fixture_specials_and_millimetre_boundaries():
    """On the large mask: rank 0 is planar up to the millimetre rounding, rank 1 has no pixel with depth (status 1), the plane of rank
    2 is not positive everywhere inside the region; and no rewritten pixel of any fixture lies within 1e-9 mm of a millimetre
    rounding boundary, so the GPU test compares every millimetre."""
    for name, mask, mm in GOLDEN:
        labels, depth, sizes = R.batch_of([(mask, mm)])
        out = R.glass_regions(labels, depth, sizes, 32, 100 if name == "large" else 1, 8)
        planes = R.region_planes(out["region_map"], depth, out["region_count"], 32)
        _, _, hit, z = R.depth_planar(out["region_map"], depth, None, sizes, out["region_count"], planes)
        frac = np.abs((z[hit] * 1000.0) % 1.0 - 0.5)
        assert hit.any() and float(frac.min()) > 1e-9, (name, float(frac.min()))
        if name == "large":
            assert planes[0, 0, 5] == 0.0 and planes[0, 0, 3] < 2e-4 and planes[0, 0, 3] < 0.2 * planes[0, 3, 3]
            assert out["regions"][0, 1, 8] == 0 and planes[0, 1, 5] == 1.0 and np.isnan(planes[0, 1, :4]).all()
            den = R.plane_denominator(planes[0], out["region_map"][0])
            assert planes[0, 2, 5] == 0.0 and (den[out["region_map"][0] == 3] <= 0.0).any() and (den[out["region_map"][0] == 3] > 0.0).any()


# ------------------------------------------------------------------------------------------------------------------ host logic
@pytest.fixture
def fake(monkeypatch):
    lib = RegionsFakeDevice()
    upload = data.upload_tables

    def counted(host, device):
        lib.calls["upload_tables"] += 1
        return upload(host, device)

    monkeypatch.setattr(data, "upload_tables", counted)
    hip.set_library(lib)
    yield lib
    hip.set_library(None)


def operands(seed=0):
    name, mask, mm = GOLDEN[1]
    labels, depth, sizes = R.batch_of([(mask, mm), (GOLDEN[2][1][:30, :40], GOLDEN[2][2][:30, :40])], rng=np.random.default_rng(seed))
    return torch.from_numpy(labels), torch.from_numpy(depth), torch.from_numpy(sizes)


def test_glass_regions_validates_before_any_launch(fake):
    labels, depth, sizes = operands()
    for kw in ({"connectivity": 6}, {"max_regions": 0}, {"max_regions": 33}, {"min_area": 0}, {"max_candidates": 0},
               {"min_depth": 2.0, "max_depth": 1.0}, {"min_depth": 0.0}):
        with pytest.raises(ValueError):
            ops.glass_regions(labels, depth, sizes, **kw)
    with pytest.raises(TypeError):
        ops.glass_regions(labels.int(), depth, sizes)
    with pytest.raises(TypeError):
        ops.glass_regions(labels, depth.int(), sizes)
    with pytest.raises(TypeError):
        ops.glass_regions(labels, depth, sizes.long())
    with pytest.raises(TypeError):
        ops.glass_regions(labels, depth, sizes, depth=depth)
    with pytest.raises(ValueError):
        ops.glass_regions(labels, depth[:, :-1], sizes)
    with pytest.raises(ValueError):
        ops.glass_regions(labels[0], depth[0], sizes)
    with pytest.raises(ValueError):
        ops.glass_regions(labels[:1].expand(17, -1, -1), depth[:1].expand(17, -1, -1), sizes[:1].expand(17, -1))
    assert fake.region_calls == []


def test_glass_regions_keys_calls_and_values(fake):
    labels, depth, sizes = operands()
    res = ops.glass_regions(labels, depth, sizes, min_area=5)
    assert tuple(res) == REGION_KEYS == ops.region_keys() and [c[0] for c in fake.region_calls] == ["glass_regions", "region_planes", "depth_planar"]
    assert fake.region_calls[0][1] == dict(max_regions=32, min_area=5, connectivity=8, max_candidates=hip.REGION_CANDIDATES, lo_mm=1, hi_mm=10000)
    assert fake.region_calls[2][1] == {"from_depth": False}
    assert res["regions"].shape == (2, 32, 12) and res["regions"].dtype == torch.int64 and res["planes"].shape == (2, 32, 6)
    assert res["region_map"].dtype == torch.uint8 and res["depth_planar"].dtype == torch.float32 and res["depth_planar_mm"].dtype == torch.uint16
    want = R.glass_regions(labels.numpy(), depth.numpy(), sizes.numpy(), 32, 5, 8)
    assert np.array_equal(res["region_map"].numpy(), want["region_map"]) and int(res["region_count"][0]) > 1
    assert not res["region_map"][1, 30:].any() and not res["region_map"][1, :, 40:].any()          # random bytes outside the frame stay out
    fake.region_calls.clear()
    res = ops.glass_regions(labels, depth, sizes, planes=False, planar=False, connectivity=4, max_regions=4, max_candidates=7)
    assert tuple(res) == REGION_KEYS[:4] == ops.region_keys(False, False) and [c[0] for c in fake.region_calls] == ["glass_regions"]
    assert fake.region_calls[0][1]["max_candidates"] == 7 and res["regions"].shape == (2, 4, 12)
    res = ops.glass_regions(labels, depth, sizes, planar=False)
    assert tuple(res) == REGION_KEYS[:5]
    res = ops.glass_regions(labels, depth, sizes, depth=depth.float() / 1000, min_depth=0.5, max_depth=2.0)
    assert fake.region_calls[-1] == ("depth_planar", {"from_depth": True}) and fake.range == (500, 2000)


def test_mm_range():
    assert ops.region_mm_range(1e-3, 10.0) == (1, 10000) and ops.region_mm_range(0.0015, 0.5) == (2, 500)
    assert ops.region_mm_range(1e-6, 100.0) == (1, 65535)


def test_default_session_issues_todays_launches_and_keys(fake):
    sess = InferenceSession(TinyModel(), compute_dtype=torch.float32, graph=False)
    assert sess.regions is None
    res = sess.predict_frames(frames_of(3), size=48, max_size=64)
    assert fake.calls == dict(BUDGET, gather2d_batch=0) and fake.region_calls == []
    assert sorted(res) == sorted(RESULT_KEYS + ("net_sizes",))


def test_session_with_regions_adds_the_region_keys(fake):
    sess = InferenceSession(TinyModel(), compute_dtype=torch.float32, graph=False, regions={"min_area": 4, "max_regions": 8}, max_depth=5.0)
    assert sess.regions == dict(max_regions=8, min_area=4, connectivity=8, min_depth=1e-3, max_depth=5.0, planes=True, planar=True,
                                max_candidates=hip.REGION_CANDIDATES)
    frames = frames_of(3)
    res = sess.predict_frames(frames, size=48, max_size=64)
    assert fake.calls == dict(BUDGET, gather2d_batch=0)         # the launches before it are the same
    assert [c[0] for c in fake.region_calls] == ["glass_regions", "region_planes", "depth_planar"]
    assert fake.region_calls[2][1] == {"from_depth": True} and fake.range == (1, 5000)
    assert sorted(res) == sorted(RESULT_KEYS + ("net_sizes",) + REGION_KEYS)
    want = R.glass_regions(res["labels"].numpy(), res["depth_mm"].numpy(), res["sizes"].numpy(), 8, 4, 8, 1, 5000)
    for k in ("region_map", "region_count", "region_total", "regions"):
        assert np.array_equal(res[k].numpy(), want[k]), k
    plain = ~(res["region_map"] > 0)
    assert torch.equal(res["depth_planar"][plain], res["depth"][plain])
    assert InferenceSession(TinyModel(), compute_dtype=torch.float32, graph=False, regions=True).regions["max_regions"] == 32
    for bad, exc in ((False, TypeError), (3, TypeError), ({"area": 3}, TypeError), ({"connectivity": 5}, ValueError), ({"max_regions": 64}, ValueError)):
        with pytest.raises(exc):
            InferenceSession(TinyModel(), compute_dtype=torch.float32, graph=False, regions=bad)


def test_evaluate_frames_planar_needs_a_session_with_regions(fake):
    sess = InferenceSession(TinyModel(), compute_dtype=torch.float32, graph=False)
    with pytest.raises(ValueError, match="regions="):
        evaluate_frames(sess, [], planar=True)
    sess = InferenceSession(TinyModel(), compute_dtype=torch.float32, graph=False, regions={"planar": False})
    with pytest.raises(ValueError, match="regions="):
        evaluate_frames(sess, [], planar=True)


def test_header_binding_and_makefile_agree():
    header = open(os.path.join(ROOT, "include", "gwdepth.h")).read()
    for name, value in (("GWD_REGION_MAX", hip.REGION_MAX), ("GWD_REGION_RECORD", hip.REGION_RECORD), ("GWD_REGION_CANDIDATES", hip.REGION_CANDIDATES)):
        assert "#define %s %d" % (name, value) in header
    assert re.search(r"GWD_WS_REGIONS\s*=\s*%d\b" % hip.WS_REGIONS, header) and hip.WS_REGIONS == 5
    assert len(R.FIELDS) == hip.REGION_RECORD and R.FIELDS == ops.REGION_FIELDS
    assert "regions.hip" in open(os.path.join(ROOT, "gw_depth_amd", "csrc", "Makefile")).read()
    for name in ("gwd_glass_regions", "gwd_region_planes", "gwd_depth_planar"):
        assert name in hip.ENTRY_POINTS


def test_workspace_query():
    import ctypes
    if not os.path.exists(hip.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(hip.LIB_PATH)
    lib.gwd_query_workspace.restype = ctypes.c_int64
    lib.gwd_query_workspace.argtypes = [ctypes.c_int32, ctypes.POINTER(ctypes.c_int64), ctypes.c_int32]
    q = lambda *d: lib.gwd_query_workspace(hip.WS_REGIONS, (ctypes.c_int64 * len(d))(*d), len(d))
    fixed = lambda B: 128 + B * 32 * 4 + B * 32 * 12 * 8 + B * 64 * 32 * 10 * 8
    assert q(1, 64, 70, 8) == fixed(1) + 32 + 2 * 64 * 70 * 4
    assert q(8, 720, 1280, 8192) == fixed(8) + 8 * 8192 * 4 + 2 * 8 * 720 * 1280 * 4
    assert q(17, 8, 8, 8) == -1 and q(1, 8, 16385, 8) == -1 and q(1, 8, 8, 0) == -1 and q(1, 8, 8) == -1
    assert lib.gwd_query_workspace(7, (ctypes.c_int64 * 3)(1, 2, 3), 3) == -1
