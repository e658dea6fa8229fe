"""CPU: line profiles (gwd_line_profiles, ops.line_profiles, InferenceSession(line_profiles=...)) - everything that needs no GPU.

  * gw_depth_amd/csrc/lineprobe.h - the scalar geometry the device kernel calls - compiled for the host with g++ -ffp-contract=off
    (tests/lineprobe_host.cpp) against the numpy statement tests/line_profile_ref.py: sample count and every probe's pixel, bit for bit;
  * known answers from the statement alone: a planar scene, a rectangular pane, a reversed line;
  * tests/golden/line_profiles.npz is what the statement gives, covers the cases, and the kernel's summation order stays inside the
    bound the GPU test holds the fits to;
  * header, binding and Makefile agree; the entry point refuses bad arguments before any launch (there is no GPU here);
  * ops.line_profiles and the session's plumbing over a stand-in library (tests/line_profile_fake.py)."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from gw_depth_amd import data, hip, infer, ops
from gw_depth_amd.infer import NMS_KEYS, PROFILE_KEYS, REGION_KEYS, RESULT_KEYS, InferenceSession
from tests import line_profile_ref as P
from tests.line_profile_fake import LineProfileFakeDevice
from tests.test_frames_post import BUDGET, FramesFakeDevice, TinyModel, frames_of

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = P.load_golden()
CAPS = (2048, 16)


def gold_inputs():
    return tuple(GOLD[k] for k in ("lines", "count", "labels", "depth_mm", "sizes"))


# ------------------------------------------------------------------------------------------------------------------ host geometry
@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("lineprobe") / "liblineprobe_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-I",
                           os.path.join(ROOT, "gw_depth_amd", "csrc"), os.path.join(HERE, "lineprobe_host.cpp"), "-o", out])
    lib = ctypes.CDLL(out)
    lib.lp_host_line.argtypes = [ctypes.POINTER(ctypes.c_double), ctypes.c_double] + [ctypes.c_int] * 4 + [ctypes.POINTER(ctypes.c_longlong)]
    lib.lp_host_count.argtypes = [ctypes.c_double, ctypes.c_int]
    return lib


def host_pixels(lib, line, offset, cap, fh, fw, pitch):
    buf = (ctypes.c_longlong * (3 * cap))()
    n = lib.lp_host_line((ctypes.c_double * 4)(*[float(v) for v in line]), offset, cap, fh, fw, pitch, buf)
    return n, np.frombuffer(buf, dtype=np.int64).reshape(3, cap)[:, :n + 1 if n else 0]


@pytest.mark.parametrize("cap", CAPS)
def test_host_build_reproduces_count_and_every_pixel(host_lib, cap):
    lines, count, labels, _, sizes = gold_inputs()
    offset, pitch = float(GOLD["offset"]), labels.shape[2]
    probes = 0
    for b in range(len(count)):
        fh, fw = (int(v) for v in sizes[b])
        for r in range(int(count[b])):
            n, _, xy = P.probes(lines[b, r], offset, cap)
            got_n, got = host_pixels(host_lib, lines[b, r], offset, cap, fh, fw, pitch)
            assert got_n == n, (b, r)
            inside, ix, iy = P.pixels(xy, fh, fw)
            assert np.array_equal(got, np.where(inside, iy * pitch + ix, -1)), (b, r)
            probes += got.size
    assert probes > (4000 if cap == 2048 else 2500)


def test_sample_count_does_not_depend_on_the_roots_last_bit(host_lib):
    cases = [0.0, -1.0, math.nan, math.inf, 5e-324, 1e-30, 0.5, 1.0, math.nextafter(1.0, 2.0), 2.0, 4.0, math.nextafter(4.0, 0.0),
             math.nextafter(4.0, 5.0), 2046.0 ** 2, math.nextafter(2046.0 ** 2, math.inf), 2047.0 ** 2, 1e300]
    cases += [float(k * k) for k in range(1, 300)] + [math.nextafter(float(k * k), math.inf) for k in range(1, 300)]
    for L2 in cases:
        for cap in (2, 16, 2048):
            n = P.sample_count(L2, cap)
            assert host_lib.lp_host_count(L2, cap) == n, (L2, cap)
            if n:
                assert 1 <= n <= cap - 1 and (n == cap - 1 or n * n >= L2) and (n == 1 or (n - 1) * (n - 1) < L2), (L2, cap, n)
    assert P.sample_count(4.0) == 2 and P.sample_count(math.nextafter(4.0, 5.0)) == 3 and P.sample_count(1e300) == 2047


# ------------------------------------------------------------------------------------------------------------------ known answers
def test_planar_scene_gives_the_plane_at_the_end_points():
    """Pixel (i, j) holds rint(1000 / plane(i + 1/2, j + 1/2)).  A sample's value differs from the plane at its probe by at most
    e = (|alpha| + |beta|) / 2 (the probe lies within half a pixel of that centre in x and in y) + mm_rounding(w_max) (the whole
    millimetre).  Along the line the plane is affine in t and the fit reproduces affine data, so the fit at an end is off by at most
    e * sum |c_i|, c = the weights of the linear map samples -> fit there (endpoint_gain); 1e-12 covers the fp64 roundings."""
    alpha, beta, gamma = 0.004, -0.003, 0.5
    h, w = 40, 56
    mm = P.plane_mm(h, w, alpha, beta, gamma)[None]
    labels, sizes = np.zeros((1, h, w), np.uint8), np.array([(h, w)], np.int32)
    lines = np.array([[(5.3, 4.1, 50.2, 33.7), (50.0, 6.0, 7.0, 35.5), (10.0, 20.5, 45.0, 20.5), (28.5, 5.0, 28.5, 36.0), (20.1, 20.2, 23.4, 18.9)]])
    out = P.line_profiles(lines, np.array([5], np.int32), labels, mm, sizes)
    w_max = 1000.0 / float(mm.min())
    e = 0.5 * (abs(alpha) + abs(beta)) + P.mm_rounding(w_max)
    worst = 0.0
    for r, line in enumerate(lines[0]):
        n, t, xy = P.probes(line)
        for p in range(3):
            assert out["profile_fits"][0, r, p, 4] == 0.0 and out["profile_fits"][0, r, p, 3] == n + 1      # every probe is inside
            for end, at in ((0, 0.0), (1, 1.0)):
                x, y = xy[p, 0 if end == 0 else n]
                want = alpha * x + beta * y + gamma
                bound = e * P.endpoint_gain(t, at) + 1e-12
                err = abs(out["profile_fits"][0, r, p, end] - want)
                worst = max(worst, err / bound)
                assert err <= bound, (r, p, end, err, bound)
            assert out["profile_fits"][0, r, p, 2] <= e + 1e-12                                             # the residual's rms too
    print("planar scene: worst error / bound %.3g (e = %.3g 1/m)" % (worst, e))
    assert out["profile_kind"][0].tolist() == [4] * 5 and (out["profile_counts"][0, :, 10:] == -1).all()


def pane_scene():
    h, w = 48, 64
    labels = np.zeros((1, h, w), np.uint8)
    labels[0, 12:36, 16:50] = 1
    rmap = labels.copy() * 3                                                                                # the pane is rank 2
    mm = np.full((1, h, w), 2000, np.uint16)
    mm[0, 12:36, 16:50] = 3000
    border = [(16.0, 12.0, 50.0, 12.0), (50.0, 12.0, 50.0, 36.0), (50.0, 36.0, 16.0, 36.0), (16.0, 36.0, 16.0, 12.0)]      # clockwise on the screen
    return labels, mm, rmap, np.array([(h, w)], np.int32), border


def test_rectangle_pane_borders_have_the_glass_on_the_inner_side():
    labels, mm, rmap, sizes, border = pane_scene()
    lines = np.array([border + [(x2, y2, x1, y1) for x1, y1, x2, y2 in border]])
    out = P.line_profiles(lines, np.array([8], np.int32), labels, mm, sizes, region_map=rmap)
    c = {f: out["profile_counts"][0, :, k] for k, f in enumerate(P.COUNT_FIELDS)}
    # walking clockwise (y down) the inside is on the side of (-dy, dx): side a; the reversed walk has it on side b
    assert out["profile_kind"][0].tolist() == [1] * 4 + [2] * 4
    assert c["region_a"].tolist() == [2] * 4 + [-1] * 4 and c["region_b"].tolist() == [-1] * 4 + [2] * 4
    assert c["samples"].tolist() == [35, 25, 35, 25] * 2 and (c["a_in"] == c["samples"]).all() and (c["b_in"] == c["samples"]).all()
    assert (c["a_glass"][:4] >= c["samples"][:4] - 1).all() and not c["b_glass"][:4].any()                   # the far end's pixel lies past the pane
    # two metres outside, exactly: the outer side's fit is flat; the inner side is three metres but for its one sample past the pane
    fits = out["profile_fits"][0]
    assert np.allclose(fits[:4, 2, :2], 0.5, rtol=0, atol=1e-15) and (fits[:4, 2, 2] <= 1e-15).all()
    assert (fits[:4, 1, :2] > 0.32).all() and (fits[:4, 1, :2] < 0.36).all() and (fits[:4, 1, 2] > 0.01).all()


def test_a_reversed_line_swaps_a_and_b():
    """Axis-aligned lines in eighths (every probe coordinate across the line is exact; along it, sample k of the reversed line is
    sample n - k of the line up to the rounding of t dx, which the 1/8 grid of the ends keeps clear of every pixel boundary but the
    integers themselves) and the fixture's general lines with their reversed duplicates."""
    labels, mm, rmap, sizes, border = pane_scene()
    rows = [(16.125, 12.0, 49.875, 12.0), (50.0, 11.625, 50.0, 36.375), (3.5, 30.25, 60.5, 30.25)]
    lines = np.array([rows + [(x2, y2, x1, y1) for x1, y1, x2, y2 in rows]])
    out = P.line_profiles(lines, np.array([6], np.int32), labels, mm, sizes, region_map=rmap)
    swap = [0, 1, 2, 3, 7, 8, 9, 4, 5, 6, 11, 10]
    other = {0: 0, 1: 2, 2: 1, 3: 3, 4: 4}
    for k in range(3):
        assert out["profile_counts"][0, k].tolist() == out["profile_counts"][0, 3 + k][swap].tolist(), k
        assert other[int(out["profile_kind"][0, k])] == int(out["profile_kind"][0, 3 + k])
    assert out["profile_kind"][0, :3].tolist() == [1, 1, 0]
    # the fixture's general-position pairs: counts swap exactly there too (no probe within 1e-9 px of a boundary), w0 <-> w1 closely
    lines, count, labels, mm, sizes = gold_inputs()
    counts, fits, kind = (GOLD[k + "_2048"] for k in ("profile_counts", "profile_fits", "profile_kind"))
    pairs = [(r, q) for r in range(70) for q in range(r + 1, 70) if np.array_equal(lines[0, r], lines[0, q][[2, 3, 0, 1]]) and np.isfinite(lines[0, r]).all()]
    assert len(pairs) >= 16
    for r, q in pairs:
        if counts[0, r, 0] == 0:
            continue
        if not P.exact_line(lines[0, r], 3.0):
            assert sorted(counts[0, r, 1:4].tolist()) == sorted(counts[0, q, 1:4].tolist())
        assert other[int(kind[0, r])] == int(kind[0, q]), (r, q)
        assert counts[0, r, 10] == counts[0, q, 11] and counts[0, r, 11] == counts[0, q, 10]


# ------------------------------------------------------------------------------------------------------------------ the fixture
def test_fixture_is_what_the_statement_gives_and_covers_the_cases():
    assert os.path.getsize(P.GOLDEN) < 100 * 1024 and GOLD["closest"] >= P.MIN_GRID_DISTANCE
    made = P.make_inputs()
    for k, v in made.items():
        assert np.array_equal(GOLD[k], v, equal_nan=True), k
    assert GOLD["labels"].shape == (3, 40, 56) and GOLD["sizes"].tolist() == [[40, 56], [37, 53], [17, 9]]
    assert GOLD["lines"].shape == (3, 70, 4) and GOLD["count"].tolist() == [70, 5, 0]
    for cap in CAPS:
        out = P.line_profiles(*gold_inputs(), None, GOLD["region_map"], GOLD["intrinsics"], float(GOLD["offset"]), cap)
        for k, v in out.items():
            assert np.array_equal(GOLD["%s_%d" % (k, cap)], v, equal_nan=True), (k, cap)
        counts, fits, kind = out["profile_counts"], out["profile_fits"], out["profile_kind"]
        assert set(fits[..., 4].ravel().tolist()) == {0.0, 1.0, 2.0, 3.0} and set(kind[0].tolist()) == {0, 1, 2, 3, 4}
        assert (fits[1, 5:, :, 4] == 3).all() and (fits[2, :, :, 4] == 3).all() and (fits[1, :5, :, 4] == 1).all()     # frame 1: no valid depth
        assert not counts[2, :, :10].any() and (counts[2, :, 10:] == -1).all() and not kind[2].any() and not fits[2, :, :, :4].any()
        assert int(counts[0, :, 0].max()) == (154 if cap == 2048 else 16) and (cap == 2048 or int((counts[0, :, 0] == 16).sum()) > 30)
        assert set(np.unique(counts[0, :, 10:]).tolist()) == {-1, 0, 1} and 6 in counts[1, :5, 10].tolist()
        deg = fits[0, :, 0, 4] == 2
        assert int(deg.sum()) == 4 and not counts[0, deg, :10].any() and np.isnan(fits[0, deg, :, :3]).all()
        pts = out["line_points"]
        assert np.isnan(pts[1:]).all() and int(np.isfinite(pts[0]).all(-1).sum()) > 80
        on = fits[0, :, 0]
        ok = on[:, 4] == 0
        assert (on[ok, :2] > 0).all()                                                # every fitted end has w > 0: the NaN placement is decided


@pytest.mark.parametrize("cap", CAPS)
def test_kernel_summation_order_stays_inside_the_bound(cap):
    """The statement evaluated with the kernel's order of every sum (lane-strided, then the xor tree) against the stored results
    (numpy's pairwise sums): inside the bound the GPU test uses, integers equal."""
    lines, count, labels, mm, sizes = gold_inputs()
    out = P.line_profiles(lines, count, labels, mm, sizes, None, GOLD["region_map"], GOLD["intrinsics"], float(GOLD["offset"]), cap,
                          summer=P.kernel_sum)
    assert np.array_equal(out["profile_counts"], GOLD["profile_counts_%d" % cap]) and np.array_equal(out["profile_kind"], GOLD["profile_kind_%d" % cap])
    worst = P.check_fits(out["profile_fits"], GOLD["profile_fits_%d" % cap], lines, count, labels, mm, sizes, max_samples=cap,
                         intrinsics=GOLD["intrinsics"], got_points=out["line_points"], want_points=GOLD["line_points_%d" % cap])
    print("max_samples %d: worst error / bound %.3g" % (cap, worst))


# ------------------------------------------------------------------------------------------------------------------ the ABI
def test_header_binding_and_makefile_agree():
    header = open(os.path.join(ROOT, "include", "gwdepth.h")).read()
    for name, value in (("GWD_PROFILE_MAX_LINES", hip.PROFILE_MAX_LINES), ("GWD_PROFILE_MAX_SAMPLES", hip.PROFILE_MAX_SAMPLES),
                        ("GWD_PROFILE_COUNTS", hip.PROFILE_COUNTS), ("GWD_LINES_F32", 0), ("GWD_LINES_F64", 1)):
        assert "#define %s %d" % (name, value) in header
    assert "#define GWD_VERSION 10" in header and "gwd_line_profiles" in hip.ENTRY_POINTS
    assert "lineprofile.hip" in open(os.path.join(ROOT, "gw_depth_amd", "csrc", "Makefile")).read()
    assert ops.PROFILE_COUNT_FIELDS == P.COUNT_FIELDS and len(P.COUNT_FIELDS) == hip.PROFILE_COUNTS
    assert ops.PROFILE_FIT_FIELDS == P.FIT_FIELDS and ops.PROFILE_PROBES == P.PROBES
    assert infer.PROFILE_KEYS == ops.PROFILE_KEYS == ("profile_counts", "profile_fits", "profile_kind", "line_points")
    probe = open(os.path.join(ROOT, "gw_depth_amd", "csrc", "lineprobe.h")).read()
    assert "#pragma clang fp contract(off)" in probe and re.search(r'#include "lineprobe\.h"', open(os.path.join(ROOT, "gw_depth_amd", "csrc", "lineprofile.hip")).read())


def test_entry_point_refuses_before_any_launch():
    """Every call below must return before the launch: this host has no device to launch on."""
    lib = hip.HipLibrary()
    assert lib.version() == 10
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(buf, ctypes.c_void_p)
    off = lambda k: ctypes.c_void_p(p.value + k)

    def call(lines=p, dtype=1, count=p, order=None, labels=p, mm=p, sizes=p, rmap=None, cam=None, B=1, C=4, Fh=8, Fw=8, offset=3.0, cap=2048,
             lo_mm=1, hi_mm=10000, hi=700, lo=300, counts=p, fits=p, kind=p, pts=None):
        return lib.lib.gwd_line_profiles(lines, dtype, count, order, labels, mm, sizes, rmap, cam, B, C, Fh, Fw, offset, cap, lo_mm, hi_mm, hi,
                                         lo, counts, fits, kind, pts, None)

    for k in ("lines", "count", "labels", "mm", "sizes", "counts", "fits", "kind"):
        assert call(**{k: None}) == -1, k
    assert call(cam=p) == -1 and call(pts=p) == -1                                   # intrinsics and line_points: both or neither
    assert call(B=0) == -1 and call(B=17) == -1 and call(C=0) == -1 and call(Fh=0) == -1 and call(Fw=16385) == -1
    assert call(offset=0.0) == -1 and call(offset=-1.0) == -1 and call(offset=math.nan) == -1 and call(offset=math.inf) == -1
    assert call(lo_mm=0) == -1 and call(hi_mm=65536) == -1 and call(lo_mm=5, hi_mm=4) == -1
    assert call(hi=1001) == -1 and call(lo=-1) == -1 and call(hi=300, lo=300) == -1
    assert call(dtype=2) == -2 and call(dtype=-1) == -2 and call(C=2049) == -2 and call(cap=1) == -2 and call(cap=2049) == -2
    assert call(lines=off(4)) == -3 and call(lines=off(2), dtype=0) == -3 and call(count=off(2)) == -3 and call(order=off(1)) == -3
    assert call(mm=off(1)) == -3 and call(fits=off(4)) == -3 and call(kind=off(2)) == -3 and call(cam=off(4), pts=p) == -3
    assert call(lines=off(4), dtype=0, B=0) == -1


# ------------------------------------------------------------------------------------------------------------------ host logic
@pytest.fixture
def fake(monkeypatch):
    lib = LineProfileFakeDevice()
    upload = data.upload_tables

    def counted(host, device):
        lib.calls["upload_tables"] += 1
        return upload(host, device)

    monkeypatch.setattr(data, "upload_tables", counted)
    hip.set_library(lib)
    yield lib
    hip.set_library(None)


def operands():
    return tuple(torch.from_numpy(v) for v in gold_inputs())


def test_line_profiles_validates_before_any_launch(fake):
    lines, count, labels, mm, sizes = operands()
    for kw in ({"offset": 0.0}, {"offset": -3.0}, {"offset": float("nan")}, {"max_samples": 1}, {"max_samples": 2049}, {"max_samples": 7.5},
               {"hi": 300, "lo": 300}, {"hi": 1001}, {"lo": -1}, {"min_depth": 2.0, "max_depth": 1.0}, {"min_depth": 0.0}):
        with pytest.raises(ValueError):
            ops.line_profiles(lines, count, labels, mm, sizes, **kw)
    for bad in ((lines.half(), count, labels, mm, sizes), (lines, count.long(), labels, mm, sizes), (lines, count, labels.int(), mm, sizes),
                (lines, count, labels, mm.int(), sizes), (lines, count, labels, mm, sizes.long())):
        with pytest.raises(TypeError):
            ops.line_profiles(*bad)
    with pytest.raises(TypeError):
        ops.line_profiles(lines, count, labels, mm, sizes, order=torch.zeros(3, 70, dtype=torch.int64))
    with pytest.raises(TypeError):
        ops.line_profiles(lines, count, labels, mm, sizes, intrinsics=torch.zeros(3, 4))
    with pytest.raises(TypeError):
        ops.line_profiles(lines, count, labels, mm, sizes, region_map=torch.zeros(3, 40, 56, dtype=torch.int32))
    for bad in ((lines[:2], count, labels, mm, sizes), (lines[..., :3], count, labels, mm, sizes), (lines, count[:2], labels, mm, sizes),
                (lines, count, labels, mm[:, :-1], sizes), (lines, count, labels[0], mm[0], sizes), (lines[:, :0], count, labels, mm, sizes)):
        with pytest.raises(ValueError):
            ops.line_profiles(*bad)
    with pytest.raises(ValueError):
        ops.line_profiles(lines, count, labels, mm, sizes, order=torch.zeros(3, 69, dtype=torch.int32))
    with pytest.raises(ValueError):
        ops.line_profiles(lines, count, labels, mm, sizes, intrinsics=torch.zeros(3, 3, dtype=torch.float64))
    with pytest.raises(ValueError):
        ops.line_profiles(torch.zeros(1, 2049, 4), count[:1], labels[:1], mm[:1], sizes[:1])
    with pytest.raises(ValueError):
        ops.line_profiles(lines[:1].expand(17, -1, -1), count[:1].expand(17), labels[:1].expand(17, -1, -1), mm[:1].expand(17, -1, -1), sizes[:1].expand(17, -1))
    assert fake.profile_calls == []


def test_line_profiles_keys_call_and_values(fake):
    lines, count, labels, mm, sizes = operands()
    rmap, cam = torch.from_numpy(GOLD["region_map"]), torch.from_numpy(GOLD["intrinsics"])
    res = ops.line_profiles(lines, count, labels, mm, sizes)
    assert tuple(res) == PROFILE_KEYS[:3] == ops.profile_keys()
    assert fake.profile_calls[-1] == dict(rows=(3, 70), dtype=torch.float64, order=False, region_map=False, intrinsics=False, offset=3.0,
                                          max_samples=2048, lo_mm=1, hi_mm=10000, hi=700, lo=300, after=0)
    assert res["profile_counts"].shape == (3, 70, 12) and res["profile_counts"].dtype == torch.int32
    assert res["profile_fits"].shape == (3, 70, 3, 5) and res["profile_fits"].dtype == torch.float64
    assert res["profile_kind"].shape == (3, 70) and res["profile_kind"].dtype == torch.int32
    assert np.array_equal(res["profile_counts"].numpy()[..., :10], GOLD["profile_counts_2048"][..., :10])
    assert (res["profile_counts"][..., 10:] == -1).all()                             # no map: no pane
    res = ops.line_profiles(lines, count, labels, mm, sizes, region_map=rmap, intrinsics=cam, max_samples=16, min_depth=0.5, max_depth=2.0,
                            offset=2.5, hi=800, lo=100)
    assert tuple(res) == PROFILE_KEYS == ops.profile_keys(True) and res["line_points"].shape == (3, 70, 2, 3)
    assert fake.profile_calls[-1] == dict(rows=(3, 70), dtype=torch.float64, order=False, region_map=True, intrinsics=True, offset=2.5,
                                          max_samples=16, lo_mm=500, hi_mm=2000, hi=800, lo=100, after=0)
    res = ops.line_profiles(lines, count, labels, mm, sizes, region_map=rmap, intrinsics=cam, max_samples=16)
    for k in PROFILE_KEYS:
        assert np.array_equal(res[k].numpy(), GOLD["%s_16" % k], equal_nan=True), k
    # float32 lines go down as they are; the order path names the rows
    order = torch.arange(69, -1, -1, dtype=torch.int32).repeat(3, 1)
    res = ops.line_profiles(lines.float(), count, labels, mm, sizes, order=order)
    assert fake.profile_calls[-1]["dtype"] == torch.float32 and fake.profile_calls[-1]["order"]
    want = P.line_profiles(lines.float().numpy()[:, ::-1], count.numpy(), labels.numpy(), mm.numpy(), sizes.numpy())
    assert np.array_equal(res["profile_counts"].numpy(), want["profile_counts"])


def test_default_session_issues_todays_launches_and_keys(fake):
    sess = InferenceSession(TinyModel(), compute_dtype=torch.float32, graph=False)
    assert sess.line_profiles is None
    res = sess.predict_frames(frames_of(3), size=48, max_size=64)
    assert fake.calls == dict(BUDGET, gather2d_batch=0) and fake.region_calls == [] and fake.profile_calls == [] and fake.nms_calls == []
    assert sorted(res) == sorted(RESULT_KEYS + ("net_sizes",))
    hip.set_library(FramesFakeDevice())                                              # the stand-in without the new call: not needed
    old = InferenceSession(TinyModel(), compute_dtype=torch.float32, graph=False, line_profiles=None).predict_frames(frames_of(3), size=48, max_size=64)
    for k in res:
        assert torch.equal(res[k], old[k]), k
    with pytest.raises(ValueError, match="line_profiles="):
        sess.predict_frames(frames_of(3), size=48, max_size=64, intrinsics=[(50.0, 50.0, 30.0, 20.0)] * 3)


def check_session_profiles(res, sess, rows, order=None, cam=None):
    lines, cnt = rows
    want = P.line_profiles(lines.numpy(), cnt.numpy(), res["labels"].numpy(), res["depth_mm"].numpy(), res["sizes"].numpy(),
                           None if order is None else order.numpy(), res["region_map"].numpy() if "region_map" in res else None,
                           None if cam is None else np.asarray(cam, np.float64), sess.line_profiles["offset"], sess.line_profiles["max_samples"],
                           *ops.region_mm_range(sess.line_profiles["min_depth"], sess.line_profiles["max_depth"]),
                           sess.line_profiles["hi"], sess.line_profiles["lo"])
    for k, v in want.items():
        assert np.array_equal(res[k].numpy(), v, equal_nan=True), k
    return want


@pytest.mark.parametrize("ensemble", [False, True], ids=["plain", "ensemble"])
def test_session_without_nms_profiles_the_lines_above_the_threshold(fake, ensemble):
    sess = InferenceSession(TinyModel(), compute_dtype=torch.float32, graph=False, line_profiles=True, score_thresh=0.45, max_depth=5.0)
    assert sess.line_profiles == dict(offset=3.0, max_samples=2048, min_depth=1e-3, max_depth=5.0, hi=700, lo=300)
    frames = frames_of(3)
    res = sess.predict_frames(frames, size=48, max_size=64, ensemble=ensemble)
    assert fake.calls == dict(BUDGET, gather2d_batch=0) and fake.region_calls == [] and fake.nms_calls == []
    assert sorted(res) == sorted(RESULT_KEYS + ("net_sizes",) + PROFILE_KEYS[:3])
    Q = TinyModel.Q
    assert fake.profile_calls == [dict(rows=(3, Q), dtype=torch.float32, order=True, region_map=False, intrinsics=False, offset=3.0,
                                       max_samples=2048, lo_mm=1, hi_mm=5000, hi=700, lo=300, after=0)]
    assert 0 < int(res["count"].min()) and int(res["count"].max()) < Q                # some rows are processed, some are not
    want = check_session_profiles(res, sess, (res["lines"], res["count"]), order=res["order"])
    k = int(res["count"][0])
    assert (want["profile_fits"][0, :k, 0, 4] == 0).all() and (want["profile_fits"][0, k:, :, 4] == 3).all()


@pytest.mark.parametrize("ensemble", [False, True], ids=["plain", "ensemble"])
def test_session_with_nms_and_regions_profiles_the_survivors(fake, ensemble):
    sess = InferenceSession(TinyModel(), compute_dtype=torch.float32, graph=False, line_nms=0.01, regions={"min_area": 4, "max_regions": 8},
                            line_profiles={"offset": 2.0, "max_samples": 64, "hi": 600})
    assert sess.line_profiles == dict(offset=2.0, max_samples=64, min_depth=1e-3, max_depth=10.0, hi=600, lo=300)
    frames = frames_of(3)
    cam = [(60.0, 61.0, w / 2.0, h / 2.0) for h, w in (f.shape[:2] for f in frames)]
    res = sess.predict_frames(frames, size=48, max_size=64, ensemble=ensemble, intrinsics=cam)
    assert fake.calls == dict(BUDGET, gather2d_batch=0)                              # the launches before it are the same
    assert sorted(res) == sorted(RESULT_KEYS + ("net_sizes",) + NMS_KEYS + REGION_KEYS + PROFILE_KEYS)
    C = TinyModel.Q * (2 if ensemble else 1)                                          # the twin's candidates are rows too
    assert fake.profile_calls == [dict(rows=(3, C), dtype=torch.float64, order=False, region_map=True, intrinsics=True, offset=2.0,
                                       max_samples=64, lo_mm=1, hi_mm=10000, hi=600, lo=300, after=3)]      # behind the three region calls
    assert res["line_points"].shape == (3, C, 2, 3) and res["profile_counts"].shape == (3, C, 12)
    want = check_session_profiles(res, sess, (res["nms_lines"], res["nms_count"]), cam=cam)
    assert np.isfinite(want["line_points"][0, 0]).all() and int(want["profile_counts"][..., 0].max()) >= 8
    plain = InferenceSession(TinyModel(), compute_dtype=torch.float32, graph=False, line_nms=0.01, regions={"min_area": 4, "max_regions": 8})
    base = plain.predict_frames(frames, size=48, max_size=64, ensemble=ensemble)
    assert sorted(base) == sorted(set(res) - set(PROFILE_KEYS))
    for k in base:
        assert torch.equal(base[k], res[k]), k
    with pytest.raises(ValueError, match="line_profiles="):
        plain.predict_frames(frames, size=48, max_size=64, intrinsics=cam)
    with pytest.raises(ValueError, match="intrinsics"):
        sess.predict_frames(frames, size=48, max_size=64, intrinsics=cam[:2])


def test_session_options_are_validated():
    for bad, exc in ((False, TypeError), (3, TypeError), ({"sides": 3}, TypeError), ({"offset": 0}, ValueError), ({"max_samples": 4096}, ValueError),
                     ({"hi": 200, "lo": 300}, ValueError)):
        with pytest.raises(exc):
            InferenceSession(TinyModel(), compute_dtype=torch.float32, graph=False, line_profiles=bad)
