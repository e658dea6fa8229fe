"""CPU: the restatement of the sensor-fusion kernels (tests/fusion_ref.py) against scipy.ndimage filters, numpy.linalg.lstsq and a
hand-written case; the conditions the GPU test's exact comparisons rest on (no sample at the trim threshold, no pixel at a millimetre
boundary); a recovery test on a synthetic scene; and the host logic of ops.sensor_fusion / InferenceSession(fusion=...) /
evaluate_frames(fused=...) through a stand-in library (tests/fusion_fake.py)."""
import math
import os
import re

import numpy as np
import pytest
import torch
from scipy import ndimage

from gw_depth_amd import data, hip, ops
from gw_depth_amd.evaluate import evaluate_frames
from gw_depth_amd.infer import FUSION_KEYS, REGION_KEYS, RESULT_KEYS, InferenceSession
from tests import fusion_ref as F
from tests import regions_ref as R
from tests.fusion_fake import FusionFakeDevice
from tests.test_frames_post import BUDGET, TinyModel, frames_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------------ the oracle
def scipy_ring(labels, sensor_mm, region_map, K, ring, gap, lo=1, hi=10000):
    rank = np.where((region_map >= 1) & (region_map <= K), region_map, 255).astype(np.uint8)
    best = ndimage.minimum_filter(rank, size=2 * ring + 1, mode="constant", cval=255)
    near = ndimage.maximum_filter((labels == 1).astype(np.uint8), size=2 * gap + 1, mode="constant", cval=0) > 0
    take = (labels != 1) & (sensor_mm >= lo) & (sensor_mm <= hi) & ~near & (best != 255)
    return np.where(take, best, 0).astype(np.uint8)


@pytest.mark.parametrize("ring,gap", F.RINGS)
@pytest.mark.parametrize("hw", F.SHAPES[:2], ids=lambda s: "%dx%d" % s)
def test_ring_map_equals_scipy_filters(hw, ring, gap):
    labels, sensor, depth, depth_mm, sizes = F.hand_case(*hw)
    rmap, count, _ = F.regions_of(labels, depth_mm, sizes)
    for b in range(labels.shape[0]):
        got, _ = F.ring_map(labels[b], sensor[b], rmap[b], int(count[b]), ring, gap)
        assert np.array_equal(got, scipy_ring(labels[b], sensor[b], rmap[b], int(count[b]), ring, gap)), b


def test_ring_map_by_hand():
    """8 x 8, ring 2, gap 1: region 1 (rank 0) top-left, region 2 (rank 1) a single pixel at (6, 5); `g` is glass in NO kept region
    (it has a gap around it but no ring of its own), `0` a hole of the sensor.  Written out: the ring keeps off the gap, takes the
    smaller rank where both regions are within 2, and skips the hole."""
    glass = ["11......",
             "11......",
             "........",
             "........",
             "........",
             "......2.",
             "........",
             "g......."]
    holes = ["........",
             "........",
             "...0....",
             "........",
             "........",
             "........",
             "........",
             "........"]
    want = ["...1....",
            "...1....",
            "...0....",
            "11112222",
            "....2...",
            "....2...",
            "....2...",
            "....2222"]
    labels = np.array([[c != "." for c in r] for r in glass], np.uint8)
    rmap = np.array([[int(c) if c in "12" else 0 for c in r] for r in glass], np.uint8)
    sensor = np.where(np.array([[c == "0" for c in r] for r in holes]), 0, 2000).astype(np.uint16)
    got, near = F.ring_map(labels, sensor, rmap, 2, ring=2, gap=1)
    assert ["".join("." if v == 0 else str(v) for v in row) for row in got] == [r.replace("0", ".") for r in want]
    assert near[6, 1] and near[7, 1] and not near[5, 0] and got[5, 0] == 0 and got[6, 0] == 0
    one, _ = F.ring_map(labels, sensor, rmap, 1, ring=2, gap=1)      # rank 1 no longer kept: its ring is gone, its gap stays
    assert not (one == 2).any() and one[4, 4] == 0 and one[3, 3] == 1 and one[5, 5] == 0
    assert np.array_equal(got, scipy_ring(labels, sensor, rmap, 2, 2, 1))


def fit_bound(x, y, w):
    """max |fit - oracle's fit| over the samples: (n + 64 kappa) 2^-52 max |w|."""
    return (len(x) + 64.0 * R.normal_cond(x, y)) * 2.0 ** -52 * float(np.abs(w).max())


def naive_reversed(v):
    s = 0.0
    for t in v[::-1].tolist():
        s += t
    return s


def each_ring(case, ring=6, gap=1, **kw):
    """(b, r, x, y, w, record) of every kept region with a ring in a case."""
    labels, sensor, depth, depth_mm, sizes = case
    rmap, count, rec = F.regions_of(labels, depth_mm, sizes, **kw)
    for b, (fh, fw) in enumerate(sizes.tolist()):
        ring_b, _ = F.ring_map(labels[b, :fh, :fw], sensor[b, :fh, :fw], rmap[b, :fh, :fw], int(count[b]), ring, gap)
        for r in range(max(int(count[b]), 0)):
            yield (b, r) + F.ring_samples(ring_b, sensor[b, :fh, :fw], r) + (rec[b, r],)


@pytest.mark.parametrize("case", ["hand", "small", "large"])
def test_moment_route_stays_inside_the_bound_whatever_the_summation(case):
    """The kernel's route to the frame plane (moments relative to the box corner moved out by the ring, centred 2 x 2 system) summed
    exactly (math.fsum) and naively in reversed raster order, against numpy.linalg.lstsq on centred columns: inside the bound the
    GPU test uses.  The relative coordinates are never negative (asserted in fit_from_moments)."""
    worst, seen = 0.0, 0
    kw = {"min_area": 100} if case == "large" else {}
    for b, r, x, y, w, rec in each_ring(F.hand_case(64, 70) if case == "hand" else F.golden_case(case), **kw):
        a, bb, c, rms, n, status = R.fit_plane(x, y, w)
        if status:
            continue
        bound = fit_bound(x, y, w)
        ox, oy = max(int(rec[1]) - 6, 0), max(int(rec[2]) - 6, 0)
        for summer in (math.fsum, naive_reversed):
            a2, b2, c2 = F.fit_from_moments(x, y, w, summer, ox, oy)
            err = float(np.abs((a2 * x + b2 * y + c2) - (a * x + bb * y + c)).max())
            worst, seen = max(worst, err / bound), seen + 1
            assert err <= bound, (case, b, r, summer.__name__, err, bound)
    assert seen >= 4
    print("%s: %d fits, worst error / bound %.3g" % (case, seen, worst))


def all_cases():
    for hw in F.SHAPES:
        for ring, gap in F.RINGS:
            yield "%dx%d ring %d gap %d" % (hw + (ring, gap)), F.hand_case(*hw), dict(ring=ring, gap=gap), {}
    for hw in F.WIDE:
        yield "%dx%d" % hw, F.hand_case(*hw), {}, {}
    for name in ("small", "medium", "large"):
        yield name, F.golden_case(name), {}, ({"min_area": 100} if name == "large" else {})


def test_fixtures_put_nothing_on_a_decision_boundary():
    """What the GPU test's exact comparisons rest on, with the oracle's coefficients: no ring sample of any case lies within 1e-12
    (relative) of the trim threshold, and no PLANE / NETWORK pixel within 1e-9 mm of a millimetre rounding boundary."""
    trimmed = planes = 0
    for name, case, opt, kw in all_cases():
        labels, sensor, depth, depth_mm, sizes = case
        rmap, count, rec = F.regions_of(labels, depth_mm, sizes, **kw)
        out = F.sensor_fusion(sensor, labels, depth, depth_mm, sizes, rmap, count, 32, **opt)
        for b, (fh, fw) in enumerate(sizes.tolist()):
            for r in range(max(int(count[b]), 0)):
                row = out["fusion_planes"][b, r]
                if row[10] == 1.0 and np.isnan(row[0]) or not row[3] > 0:
                    continue
                x, y, w = F.ring_samples(out["fusion_ring"][b, :fh, :fw], sensor[b, :fh, :fw], r)
                keep, e2, thr = F.trim_keep(x, y, w, row[:4], 2.5)
                assert float(np.abs(e2 - thr).min()) > 1e-12 * thr, (name, b, r)
                trimmed += int((~keep).sum())
                planes += 1
        rewritten = out["fused_source"] >= F.PLANE
        frac = np.abs((out["z"][rewritten] * 1000.0) % 1.0 - 0.5)
        assert float(frac.min()) > 1e-9, (name, float(frac.min()))
    assert planes > 60 and trimmed > 100


def test_full_frame_region_has_no_ring_and_falls_back_to_the_network():
    labels, sensor, depth, depth_mm, sizes = F.hand_case(37, 53)
    rmap, count, rec = F.regions_of(labels, depth_mm, sizes)
    out = F.sensor_fusion(sensor, labels, depth, depth_mm, sizes, rmap, count, 32)
    full = list(F.masks_for(37, 53)).index("full")
    assert count[full] == 1 and not out["fusion_ring"][full].any()
    assert out["fusion_planes"][full, 0, 10] == 1.0 and out["fusion_planes"][full, 0, 4] == 0 and np.isnan(out["fusion_planes"][full, 0, :4]).all()
    assert (out["fused_source"][full] == F.NETWORK).all() and out["fusion_scale"][full].tolist() == [1.0, 0.0, 0.0, 0.0]
    pair = list(F.masks_for(37, 53)).index("pair")                  # both ranks within `ring` of the columns between the panes: the smaller wins
    between = out["fusion_ring"][pair, 10:30, 53 // 2 - 1:53 // 2 + 2]
    assert count[pair] == 2 and (between[between > 0] == 1).all() and (out["fusion_ring"][pair] == 2).any()


def test_recovery_on_a_synthetic_scene():
    """Two panes on known 3-D planes, the sensor reading the wall behind them inside the glass and the true frame (millimetre
    quantisation, 5 % outliers at twice the depth on the ring, 3 % holes) around it.  On the glass the oracle's fused depth is closer
    to the truth than the sensor's and than the unscaled network's.  Measured on this fixture: worst |fused - truth| on glass
    4.5e-5 m (mean 1.7e-5 m) with trim = 2.5, against 3.1 m (mean 1.5 m) for the sensor and 0.69 m (mean 0.38 m) for the unscaled
    network; the bar is twice the measured worst error (the factor covers another valid summation order).  Without the trim the
    outliers tilt the planes: the worst error is 9.2e-2 m."""
    s = F.recovery_scene()
    mask = s["mask"]
    labels, sensor, depth, depth_mm, sizes = F.batch_of([(mask, s["sensor_mm"], s["depth"], s["depth_mm"])])
    rmap, count, rec = F.regions_of(labels, depth_mm, sizes, min_area=100)
    assert count[0] == 2
    err = {}
    for trim in (2.5, 0.0):
        out = F.sensor_fusion(sensor, labels, depth, depth_mm, sizes, rmap, count, 32, trim=trim)
        assert out["fusion_planes"][0, :2, 10].tolist() == [0.0, 0.0] and (out["fused_source"][0][mask] == F.PLANE).all()
        err[trim] = np.abs(out["depth_fused"][0].astype(np.float64) - s["truth"])[mask]
    sensor_err = np.abs(sensor[0][mask] / 1000.0 - s["truth"][mask])
    network_err = np.abs(depth[0][mask].astype(np.float64) - s["truth"][mask])
    print("glass: fused worst %.3g mean %.3g | trim=0 worst %.3g | sensor worst %.3g mean %.3g | network worst %.3g mean %.3g"
          % (err[2.5].max(), err[2.5].mean(), err[0.0].max(), sensor_err.max(), sensor_err.mean(), network_err.max(), network_err.mean()))
    assert err[2.5].mean() < sensor_err.mean() and err[2.5].mean() < network_err.mean()
    assert err[2.5].max() < sensor_err.max() and err[2.5].max() < network_err.max()
    assert err[2.5].max() <= 2 * MEASURED_WORST
    assert err[0.0].max() > err[2.5].max() and err[0.0].mean() > err[2.5].mean()
    scale = out["fusion_scale"][0]
    assert abs(scale[0] - 1 / 1.15) < 2e-2 and scale[1] >= 1000          # 1.15 times too large; the outliers near the glass pull the scale up a little


MEASURED_WORST = 4.5e-5


# ------------------------------------------------------------------------------------------------------------------ host logic
@pytest.fixture
def fake(monkeypatch):
    lib = FusionFakeDevice()
    upload = data.upload_tables

    def counted(host, device):
        lib.calls["upload_tables"] += 1
        return upload(host, device)

    monkeypatch.setattr(data, "upload_tables", counted)
    hip.set_library(lib)
    yield lib
    hip.set_library(None)


def operands():
    labels, sensor, depth, depth_mm, sizes = F.hand_case(37, 53)
    rmap, count, rec = F.regions_of(labels, depth_mm, sizes)
    t = torch.from_numpy
    return dict(sensor_mm=t(sensor), labels=t(labels), depth=t(depth), depth_mm=t(depth_mm), sizes=t(sizes), region_map=t(rmap),
                region_count=t(count), regions=t(rec))


def test_check_fusion_options():
    assert ops.check_fusion_options() == dict(ring=6, gap=1, trim=2.5, min_ring=50, max_rms=None, align=True, min_align=1000,
                                              min_depth=1e-3, max_depth=10.0)
    assert ops.check_fusion_options(ring=32, gap=31, trim=0, max_rms=0.5)["max_rms"] == 0.5
    assert ops.fusion_keys() == FUSION_KEYS == ops.FUSION_KEYS
    for kw, name in (({"ring": 0}, "ring"), ({"ring": 33}, "ring"), ({"gap": -1}, "gap"), ({"gap": 6}, "gap"), ({"ring": 3, "gap": 3}, "gap"),
                     ({"trim": -1.0}, "trim"), ({"trim": float("nan")}, "trim"), ({"trim": float("inf")}, "trim"), ({"min_ring": -1}, "min_ring"),
                     ({"max_rms": -0.1}, "max_rms"), ({"max_rms": float("nan")}, "max_rms"), ({"min_align": -1}, "min_align"),
                     ({"min_depth": 0.0}, "min_depth"), ({"min_depth": 2.0, "max_depth": 1.0}, "max_depth"),
                     ({"min_depth": 0.0101, "max_depth": 0.0109}, "millimetre")):
        with pytest.raises(ValueError, match=name):
            ops.check_fusion_options(**kw)
    for kw, name in (({"ring": 2.5}, "ring"), ({"gap": 0.5}, "gap"), ({"min_ring": 1.5}, "min_ring"), ({"min_align": 0.5}, "min_align"),
                     ({"align": 1}, "align"), ({"ring": True}, "ring")):
        with pytest.raises(TypeError, match=name):
            ops.check_fusion_options(**kw)


def test_sensor_fusion_validates_before_any_launch(fake):
    good = operands()
    wrong = {"sensor_mm": torch.int16, "labels": torch.int32, "depth": torch.float64, "depth_mm": torch.int32, "sizes": torch.int64,
             "region_map": torch.int32, "region_count": torch.int64, "regions": torch.int32}
    for name, dt in wrong.items():
        with pytest.raises(TypeError, match=name):
            ops.sensor_fusion(**dict(good, **{name: good[name].to(dt)}))
        with pytest.raises(TypeError, match=name):
            ops.sensor_fusion(**dict(good, **{name: good[name].numpy()}))
    for name in ("sensor_mm", "depth", "depth_mm", "region_map"):
        with pytest.raises(ValueError, match=name):
            ops.sensor_fusion(**dict(good, **{name: good[name][:, :, :-1]}))
    for name, bad in (("labels", good["labels"][0]), ("sizes", good["sizes"][:, :1]), ("region_count", good["region_count"][:-1]),
                      ("regions", good["regions"][:, :, :-1]), ("regions", good["regions"][:-1]), ("regions", good["regions"][:, :0])):
        with pytest.raises(ValueError, match=name):
            ops.sensor_fusion(**dict(good, **{name: bad}))
    with pytest.raises(ValueError, match="at most"):
        ops.sensor_fusion(**{k: v[:1].expand(17, *v.shape[1:]) for k, v in good.items()})
    with pytest.raises(ValueError, match="ring"):
        ops.sensor_fusion(**good, ring=40)
    assert fake.fusion_calls == []


def test_sensor_fusion_keys_calls_and_values(fake):
    good = operands()
    res = ops.sensor_fusion(**good)
    assert tuple(res) == FUSION_KEYS and [c[0] for c in fake.fusion_calls] == ["fusion_ring", "fusion_planes", "fusion_depth"]
    assert fake.fusion_calls[0][1] == dict(max_regions=32, ring=6, gap=1, lo_mm=1, hi_mm=10000, align=True, min_align=1000)
    assert fake.fusion_calls[1][1] == dict(ring=6, trim=2.5, min_ring=50, max_rms=None)
    B, Fh, Fw = good["labels"].shape
    for k, dt, shape in (("depth_fused", torch.float32, (B, Fh, Fw)), ("depth_fused_mm", torch.uint16, (B, Fh, Fw)),
                         ("fused_source", torch.uint8, (B, Fh, Fw)), ("fusion_ring", torch.uint8, (B, Fh, Fw)),
                         ("fusion_planes", torch.float64, (B, 32, 12)), ("fusion_scale", torch.float64, (B, 4))):
        assert res[k].dtype == dt and tuple(res[k].shape) == shape, k
    n = {k: v.numpy() for k, v in good.items()}
    want = F.sensor_fusion(n["sensor_mm"], n["labels"], n["depth"], n["depth_mm"], n["sizes"], n["region_map"], n["region_count"], 32)
    for k in FUSION_KEYS:
        assert np.array_equal(res[k].numpy(), want[k], equal_nan=True), k
    fake.fusion_calls.clear()
    ops.sensor_fusion(**good, ring=3, gap=0, trim=0, min_ring=5, max_rms=0.25, align=False, min_align=7, min_depth=0.5, max_depth=2.0)
    assert fake.fusion_calls[0][1] == dict(max_regions=32, ring=3, gap=0, lo_mm=500, hi_mm=2000, align=False, min_align=7)
    assert fake.fusion_calls[1][1] == dict(ring=3, trim=0.0, min_ring=5, max_rms=0.25)
    assert fake.fusion_calls[2][1] == dict(lo_mm=500, hi_mm=2000, min_depth=0.5, max_depth=2.0)


def sensor_planes(frames, value=1800):
    return [torch.full((int(f.shape[0]), int(f.shape[1])), value, dtype=torch.uint16) for f in frames]


def test_session_without_fusion_issues_todays_launches_and_keys(fake):
    sess = InferenceSession(TinyModel(), compute_dtype=torch.float32, graph=False, regions={"min_area": 4})
    assert sess.fusion is None
    frames = frames_of(3)
    res = sess.predict_frames(frames, size=48, max_size=64)
    assert fake.calls == dict(BUDGET, gather2d_batch=0) and fake.fusion_calls == []
    assert [c[0] for c in fake.region_calls] == ["glass_regions", "region_planes", "depth_planar"]
    assert sorted(res) == sorted(RESULT_KEYS + ("net_sizes",) + REGION_KEYS)
    with pytest.raises(ValueError, match="fusion="):
        sess.predict_frames(frames, size=48, max_size=64, sensor_depth=sensor_planes(frames))
    plain = InferenceSession(TinyModel(), compute_dtype=torch.float32, graph=False)
    fake.region_calls.clear()
    assert sorted(plain.predict_frames(frames, size=48, max_size=64)) == sorted(RESULT_KEYS + ("net_sizes",))
    assert fake.region_calls == [] and fake.fusion_calls == []


def test_session_with_fusion_adds_the_fusion_keys(fake):
    sess = InferenceSession(TinyModel(), compute_dtype=torch.float32, graph=False, regions={"min_area": 4, "max_regions": 8},
                            fusion={"ring": 4, "min_ring": 10}, max_depth=5.0)
    assert sess.fusion == dict(ring=4, gap=1, trim=2.5, min_ring=10, max_rms=None, align=True, min_align=1000, min_depth=1e-3, max_depth=5.0)
    frames = frames_of(3)
    res = sess.predict_frames(frames, size=48, max_size=64)             # no sensor plane in this call: the keys of a session without fusion=
    assert sorted(res) == sorted(RESULT_KEYS + ("net_sizes",) + REGION_KEYS) and fake.fusion_calls == []
    assert fake.calls == dict(BUDGET, gather2d_batch=0)
    launches = dict(fake.calls)
    fake.region_calls.clear()
    planes = sensor_planes(frames)
    res = sess.predict_frames(frames, size=48, max_size=64, sensor_depth=planes)
    assert {k: fake.calls[k] - launches[k] for k in launches} == dict(BUDGET, gather2d_batch=0)      # the launches before it are the same
    assert [c[0] for c in fake.region_calls] == ["glass_regions", "region_planes", "depth_planar"]
    assert [c[0] for c in fake.fusion_calls] == ["fusion_ring", "fusion_planes", "fusion_depth"]
    assert fake.fusion_calls[0][1] == dict(max_regions=8, ring=4, gap=1, lo_mm=1, hi_mm=5000, align=True, min_align=1000)
    assert sorted(res) == sorted(RESULT_KEYS + ("net_sizes",) + REGION_KEYS + FUSION_KEYS)
    n = {k: res[k].numpy() for k in ("labels", "depth", "depth_mm", "sizes", "region_map", "region_count")}
    Fh, Fw = n["labels"].shape[1:]
    packed = np.zeros((3, Fh, Fw), np.uint16)
    for b, p in enumerate(planes):
        packed[b, :p.shape[0], :p.shape[1]] = p.numpy()
    want = F.sensor_fusion(packed, n["labels"], n["depth"], n["depth_mm"], n["sizes"], n["region_map"], n["region_count"], 8, ring=4,
                           min_ring=10, hi_mm=5000, max_depth=5.0)
    for k in FUSION_KEYS:
        assert np.array_equal(res[k].numpy(), want[k], equal_nan=True), k
    one = sess.predict_frames(frames, size=48, max_size=64, sensor_depth=torch.from_numpy(packed))     # one (B, Fh, Fw) tensor
    for k in FUSION_KEYS:
        assert np.array_equal(one[k].numpy(), want[k], equal_nan=True), k
    assert InferenceSession(TinyModel(), compute_dtype=torch.float32, graph=False, regions=True, fusion=True).fusion["ring"] == 6


def test_session_rejects_bad_fusion_arguments(fake):
    new = lambda **kw: InferenceSession(TinyModel(), compute_dtype=torch.float32, graph=False, **kw)
    with pytest.raises(ValueError, match="regions="):
        new(fusion=True)
    for bad, exc in ((False, TypeError), (3, TypeError), ({"rings": 3}, TypeError), ({"ring": 0}, ValueError), ({"gap": 9}, ValueError),
                     ({"align": 2}, TypeError)):
        with pytest.raises(exc):
            new(regions=True, fusion=bad)
    sess = new(regions=True, fusion=True)
    frames = frames_of(3)
    planes = sensor_planes(frames)
    h, w = planes[1].shape
    for bad in (planes[:2], planes[:1] + [planes[1][:, :-1]] + planes[2:], planes[:1] + [planes[1].int()] + planes[2:],
                planes[:1] + [planes[1].numpy()] + planes[2:]):
        with pytest.raises(ValueError, match="sensor_depth" + ("" if len(bad) == 2 else r"\[1\].*frame 1")):
            sess.predict_frames(frames, size=48, max_size=64, sensor_depth=bad)
    with pytest.raises(ValueError, match="sensor_depth"):
        sess.predict_frames(frames, size=48, max_size=64, sensor_depth=torch.zeros((3, 4, 4), dtype=torch.uint16))
    assert fake.fusion_calls == []


def test_evaluate_frames_fused_needs_a_session_with_fusion_and_a_sensor(fake):
    plain = InferenceSession(TinyModel(), compute_dtype=torch.float32, graph=False, regions=True)
    with pytest.raises(ValueError, match="fusion="):
        evaluate_frames(plain, [], fused=True, sensor=lambda idx: [])
    sess = InferenceSession(TinyModel(), compute_dtype=torch.float32, graph=False, regions=True, fusion=True)
    with pytest.raises(ValueError, match="sensor"):
        evaluate_frames(sess, [], fused=True)
    with pytest.raises(ValueError, match="sensor"):
        evaluate_frames(sess, [], sensor=lambda idx: [])
    with pytest.raises(ValueError, match="planar"):
        evaluate_frames(sess, [], fused=True, planar=True, sensor=lambda idx: [])


def test_header_binding_and_makefile_agree():
    header = open(os.path.join(ROOT, "include", "gwdepth.h")).read()
    for name, value in (("GWD_FUSION_MAX_RING", hip.FUSION_MAX_RING), ("GWD_FUSION_PLANE", hip.FUSION_PLANE), ("GWD_FUSED_SENSOR", hip.FUSED_SENSOR),
                        ("GWD_FUSED_PLANE", hip.FUSED_PLANE), ("GWD_FUSED_NETWORK", hip.FUSED_NETWORK), ("GWD_VERSION", 10)):
        assert re.search(r"#define %s %d\b" % (name, value), header), name
    assert re.search(r"GWD_WS_FUSION\s*=\s*%d\b" % hip.WS_FUSION, header) and hip.WS_FUSION == 6
    assert (F.SENSOR, F.PLANE, F.NETWORK) == (hip.FUSED_SENSOR, hip.FUSED_PLANE, hip.FUSED_NETWORK)
    assert len(F.PLANE_FIELDS) == hip.FUSION_PLANE and F.PLANE_FIELDS == ops.FUSION_PLANE_FIELDS
    make = open(os.path.join(ROOT, "gw_depth_amd", "csrc", "Makefile")).read()
    # regions.o and fusion.o follow planefit.h through the dependencies the compiler writes: the flags ask for them, the Makefile
    # reads them, and both sources include the header
    assert "fusion.hip" in make and re.search(r"^CXXFLAGS\b.*-MMD", make, re.M) and re.search(r"^-include \$\(OBJS:\.o=\.d\)", make, re.M)
    assert '#include "planefit.h"' in open(os.path.join(ROOT, "gw_depth_amd", "csrc", "fusion.hip")).read()
    for name in ("gwd_fusion_ring", "gwd_fusion_planes", "gwd_fusion_depth"):
        assert name in hip.ENTRY_POINTS and name in header
    regions = open(os.path.join(ROOT, "gw_depth_amd", "csrc", "regions.hip")).read()     # the fit is written once, in the header
    assert '#include "planefit.h"' in regions and "mul128" not in regions


def test_workspace_query():
    import ctypes
    if not os.path.exists(hip.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(hip.LIB_PATH)
    lib.gwd_query_workspace.restype = ctypes.c_int64
    lib.gwd_query_workspace.argtypes = [ctypes.c_int32, ctypes.POINTER(ctypes.c_int64), ctypes.c_int32]
    q = lambda *d: lib.gwd_query_workspace(hip.WS_FUSION, (ctypes.c_int64 * len(d))(*d), len(d))
    fixed = lambda B: 16 * 4 * 8 + B * 64 * 32 * 10 * 8
    assert q(1, 64, 70) == fixed(1) + 64 * 70 and q(3, 37, 53) == fixed(3) + 3 * 37 * 53 + 5
    assert q(8, 720, 1280) == fixed(8) + 8 * 720 * 1280
    assert q(17, 8, 8) == -1 and q(1, 8, 16385) == -1 and q(1, 0, 8) == -1 and q(1, 8) == -1 and q(1, 8, 8, 8) == -1
