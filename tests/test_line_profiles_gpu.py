"""GPU: gwd_line_profiles (csrc/lineprofile.hip) through ops.line_profiles against its statement (tests/line_profile_ref.py).

Integers (profile_counts, profile_kind, n_used, status) and the placement of every NaN are compared exactly; every call is made twice
with bit-identical results, the floats included.  w0 / w1 of a fit stay within (n + 8) 2^-52 max |w| (1 + 2 sqrt(n / Suu)) of the
statement's (the two differ in the order of their sums only; DESIGN.md section 25 derives it), rms within twice that, an end point
within what that error in w leaves of it (line_profile_ref.check_fits)."""
import ctypes

import numpy as np
import pytest
import torch

from gw_depth_amd import hip, ops
from tests import line_profile_ref as P

pytestmark = pytest.mark.gpu

GOLD = P.load_golden()
INPUTS = ("lines", "count", "labels", "depth_mm", "sizes")


def run(lines, count, labels, depth_mm, sizes, order=None, region_map=None, intrinsics=None, **kw):
    """ops.line_profiles twice on the device -> numpy dict; the two calls agree in every bit."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    args = [dev(a) for a in (lines, count, labels, depth_mm, sizes)]
    opt = dict(order=dev(order), region_map=dev(region_map), intrinsics=dev(intrinsics), **kw)
    torch.cuda.set_sync_debug_mode("error")                     # nothing in the call waits for the device
    try:
        one = ops.line_profiles(*args, **opt)
        two = ops.line_profiles(*args, **opt)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    out = {}
    for k in one:
        a, b = one[k].cpu().numpy(), two[k].cpu().numpy()
        assert a.tobytes() == b.tobytes(), "%s differs between two calls" % k
        out[k] = a
    return out


def check(out, want, lines, count, labels, depth_mm, sizes, order=None, intrinsics=None, **kw):
    """-> worst error / bound."""
    for k in ("profile_counts", "profile_kind"):
        assert np.array_equal(out[k], want[k]), (k, np.argwhere(out[k] != want[k])[:5].tolist())
    return P.check_fits(out["profile_fits"], want["profile_fits"], lines, count, labels, depth_mm, sizes, order=order, intrinsics=intrinsics,
                        got_points=out.get("line_points"), want_points=want.get("line_points"), **kw)


@pytest.mark.parametrize("cap", [2048, 16])
def test_fixture(cap):
    """tests/golden/line_profiles.npz: three frames of different sizes in one plane (noise outside them), counts (70, 5, 0); lines
    inside, across every border, outside, degenerate, shorter than a pixel, on grid lines, long diagonals, reversed duplicates;
    a planar scene with a depth step along a pane, holes, a frame with no valid depth; the sample cap hit (16) and not (2048)."""
    inputs = [GOLD[k] for k in INPUTS]
    out = run(*inputs, region_map=GOLD["region_map"], intrinsics=GOLD["intrinsics"], offset=float(GOLD["offset"]), max_samples=cap)
    want = {k: GOLD["%s_%d" % (k, cap)] for k in ops.PROFILE_KEYS}
    worst = check(out, want, *inputs, intrinsics=GOLD["intrinsics"], max_samples=cap)
    print("fixture, max_samples %d: worst fit error / bound %.3g" % (cap, worst))
    assert out["profile_fits"][2].tobytes() == want["profile_fits"][2].tobytes() and np.isnan(out["line_points"][1:]).all()


def test_same_line_same_record_in_another_row_slot_and_plane():
    """Frame 0 of the fixture in slot 0 of its (3, 40, 56) plane, and in slot 1 of a (2, 64, 70) plane of noise with its rows in
    reversed order (through `order`, and gathered by hand): every record is the same, bit for bit."""
    lines, count, labels, mm, sizes = (GOLD[k] for k in INPUTS)
    base = run(lines, count, labels, mm, sizes, region_map=GOLD["region_map"], intrinsics=GOLD["intrinsics"])
    rng = np.random.default_rng(5)
    C = lines.shape[1]
    big = [rng.integers(0, 256, (2, 64, 70), dtype=np.uint8), rng.integers(0, 65536, (2, 64, 70), dtype=np.uint16),
           rng.integers(0, 256, (2, 64, 70), dtype=np.uint8)]
    for dst, src in zip(big, (labels, mm, GOLD["region_map"])):
        dst[1, :40, :56] = src[0]
    lines2 = np.stack([rng.uniform(-5, 60, (C, 4)), lines[0][::-1]])
    count2, sizes2 = np.array([C // 2, C], np.int32), np.array([(64, 70), (40, 56)], np.int32)
    cam2 = np.stack([GOLD["intrinsics"][1], GOLD["intrinsics"][0]])
    moved = run(lines2, count2, big[0], big[1], sizes2, region_map=big[2], intrinsics=cam2)
    order = np.stack([np.arange(C, dtype=np.int32), np.arange(C - 1, -1, -1, dtype=np.int32)])
    lines3 = np.stack([lines2[0], lines[0]])
    ordered = run(lines3, count2, big[0], big[1], sizes2, order=order, region_map=big[2], intrinsics=cam2)
    for k in base:
        assert moved[k][1][::-1].tobytes() == base[k][0].tobytes(), k
        assert ordered[k].tobytes() == moved[k].tobytes(), k                # the order path equals gathering the lines first
    assert (moved["profile_fits"][0, C // 2:, :, 4] == 3).all() and (moved["profile_fits"][0, :C // 2, :, 4] != 3).all()


def test_float32_and_float64_lines_of_the_same_values_agree():
    lines, count, labels, mm, sizes = (GOLD[k] for k in INPUTS)
    l32 = lines.astype(np.float32)
    a = run(l32, count, labels, mm, sizes, region_map=GOLD["region_map"], intrinsics=GOLD["intrinsics"])
    b = run(l32.astype(np.float64), count, labels, mm, sizes, region_map=GOLD["region_map"], intrinsics=GOLD["intrinsics"])
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    want = P.line_profiles(l32, count, labels, mm, sizes)                   # rounding the ends to fp32 moves probes: compared with its own statement
    assert np.array_equal(a["profile_counts"][..., :10], want["profile_counts"][..., :10])


def test_glass_regions_then_line_profiles_name_the_pane():
    """A 64 x 48 frame with two panes (and a second, smaller frame): every border line of a pane names that pane's rank on its glass
    side, and -1 or the other pane outside."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    h, w = 48, 64
    labels = np.zeros((2, h, w), np.uint8)
    boxes = [(6, 8, 40, 30), (6, 33, 30, 55)]                              # y0, x0, y1, x1: 34 x 22 = 748 and 24 x 22 = 528 pixels: ranks 0, 1
    for y0, x0, y1, x1 in boxes:
        labels[0, y0:y1, x0:x1] = 1
    labels[1, 5:25, 5:30] = 1
    mm = np.full((2, h, w), 2500, np.uint16)
    mm[0, 6:40, 8:30], mm[0, 6:30, 33:55] = 3100, 3300
    sizes = np.array([(h, w), (30, 40)], np.int32)
    dev = [torch.from_numpy(a).cuda() for a in (labels, mm, sizes)]
    reg = ops.glass_regions(*dev, min_area=50)
    rows = []
    for y0, x0, y1, x1 in boxes:                                            # clockwise on the screen: the glass on side a
        rows += [(x0, y0, x1, y0), (x1, y0, x1, y1), (x1, y1, x0, y1), (x0, y1, x0, y0)]
    lines = np.zeros((2, 8, 4), np.float64)
    lines[0] = rows
    lines[1, :4] = [(5, 5, 30, 5), (30, 5, 30, 25), (30, 25, 5, 25), (5, 25, 5, 5)]
    count = torch.tensor([8, 4], dtype=torch.int32, device="cuda")
    res = ops.line_profiles(torch.from_numpy(lines).cuda(), count, *dev, region_map=reg["region_map"], offset=4.0)
    torch.cuda.synchronize()
    assert reg["region_count"].tolist() == [2, 1]
    c = res["profile_counts"].cpu().numpy()
    # the panes are 3 px apart and the probes 4 px from the line: the two facing borders see the other pane on their outer side
    assert c[0, :, 10].tolist() == [0] * 4 + [1] * 4 and c[1, :4, 10].tolist() == [0] * 4
    assert c[0, :4, 11].tolist() == [-1, 1, -1, -1] and c[0, 4:, 11].tolist() == [-1, -1, -1, 0] and (c[1, :, 11] == -1).all()
    kind = res["profile_kind"].cpu().numpy()
    assert kind[0, [0, 2, 3, 4, 5, 6]].tolist() == [1] * 6 and kind[0, 7] == 3 and kind[1].tolist() == [1, 1, 1, 1, 0, 0, 0, 0]
    want = P.line_profiles(lines, [8, 4], labels, mm, sizes, region_map=reg["region_map"].cpu().numpy(), offset=4.0)
    assert np.array_equal(c, want["profile_counts"]) and np.array_equal(kind, want["profile_kind"])


def test_status_returns_launch_nothing():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    lib = hip.library()
    B, C, Fh, Fw = 1, 4, 8, 16
    lines = torch.tensor([[(1.0, 1.0, 14.0, 6.0)] * C], dtype=torch.float64, device="cuda")
    count = torch.tensor([2], dtype=torch.int32, device="cuda")
    labels = torch.ones((B, Fh, Fw), dtype=torch.uint8, device="cuda")
    mm = torch.full((B, Fh, Fw), 1000, dtype=torch.uint16, device="cuda")
    sizes = torch.tensor([[Fh, Fw]], dtype=torch.int32, device="cuda")
    counts = torch.full((B, C, 12), 77, dtype=torch.int32, device="cuda")
    fits = torch.full((B, C, 3, 5), 77.0, dtype=torch.float64, device="cuda")
    kind = torch.full((B, C), 77, dtype=torch.int32, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)

    def call(lines_p=p(lines), dtype=1, B=B, C=C, offset=3.0, cap=2048, hi=700, lo=300, fits_p=p(fits), cam=None, pts=None):
        return lib.lib.gwd_line_profiles(lines_p, dtype, p(count), None, p(labels), p(mm), p(sizes), None, cam, B, C, Fh, Fw, offset, cap, 1, 10000,
                                         hi, lo, p(counts), fits_p, p(kind), pts, stream)

    assert call(lines_p=None) == -1 and call(B=0) == -1 and call(B=17) == -1 and call(C=0) == -1 and call(offset=0.0) == -1
    assert call(hi=300, lo=300) == -1 and call(cam=p(fits)) == -1
    assert call(dtype=2) == -2 and call(C=2049) == -2 and call(cap=1) == -2 and call(cap=2049) == -2
    assert call(lines_p=p(lines, 4)) == -3 and call(fits_p=p(fits, 4)) == -3
    torch.cuda.synchronize()
    for t in (counts, fits, kind):
        assert (t == 77).all()
    assert call() == 0                                                      # ... and the same call with good arguments runs
    torch.cuda.synchronize()
    assert counts[0, :, 0].tolist() == [15, 15, 0, 0] and kind[0].tolist() == [3, 3, 0, 0] and fits[0, :, 0, 4].tolist() == [0, 0, 3, 3]
    assert float((fits[0, :2, :, :2] - 1.0).abs().max()) < 1e-12 and float(fits[0, :2, :, 2].max()) < 1e-12


# ------------------------------------------------------------------------------------------------------------------ end to end
def test_session_end_to_end():
    """Two synthetic frames (96 x 128 and 90 x 120) through InferenceSession(line_nms, regions, line_profiles).predict_frames: the
    profile keys equal ops.line_profiles applied to the returned tensors (bit for bit) and agree with the statement; every other key
    is bit-equal to a session without the option; without line_nms the rows are the lines above the threshold, through `order`."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gw_depth_amd.infer import NMS_KEYS, PROFILE_KEYS, REGION_KEYS, RESULT_KEYS, InferenceSession
    from tests.golden_check import build
    _, model, _ = build(device="cuda")
    g = torch.Generator().manual_seed(4)
    frames = []
    for h, w in ((96, 128), (90, 120)):
        low = torch.rand(1, 3, 6, 8, generator=g)
        frames.append((torch.nn.functional.interpolate(low, size=(h, w), mode="bicubic", align_corners=False)[0].clamp(0, 1) * 255)
                      .permute(1, 2, 0).to(torch.uint8).contiguous())
    cam = torch.tensor([(100.0, 100.0, 64.0, 48.0), (95.0, 96.0, 60.0, 45.0)], dtype=torch.float64)
    kw = dict(compute_dtype=torch.float32, graph=False, line_nms=0.01, line_nms_min_score=0.0, regions={"min_area": 20}, score_thresh=0.0)
    plain = InferenceSession(model, **kw)
    sess = InferenceSession(model, line_profiles={"max_samples": 256}, **kw)
    base = plain.predict_frames(frames, size=96, max_size=128, copy=True)
    res = sess.predict_frames(frames, size=96, max_size=128, copy=True, intrinsics=cam)
    assert sorted(base) == sorted(RESULT_KEYS + ("net_sizes",) + NMS_KEYS + REGION_KEYS)
    assert sorted(res) == sorted(RESULT_KEYS + ("net_sizes",) + NMS_KEYS + REGION_KEYS + PROFILE_KEYS)
    for k in base:
        assert torch.equal(base[k], res[k]), k
    again = ops.line_profiles(res["nms_lines"], res["nms_count"], res["labels"], res["depth_mm"], res["sizes"], region_map=res["region_map"],
                              intrinsics=cam.cuda(), max_samples=256, min_depth=sess.min_depth, max_depth=sess.max_depth)
    host = {k: v.cpu().numpy() for k, v in res.items()}
    for k in PROFILE_KEYS:
        assert again[k].cpu().numpy().tobytes() == host[k].tobytes(), k
    assert int(host["nms_count"].min()) >= 1
    lo, hi = ops.region_mm_range(sess.min_depth, sess.max_depth)
    want = P.line_profiles(host["nms_lines"], host["nms_count"], host["labels"], host["depth_mm"], host["sizes"], None, host["region_map"],
                           cam.numpy(), 3.0, 256, lo, hi)
    counts_equal = np.array_equal(host["profile_counts"], want["profile_counts"]) and np.array_equal(host["profile_kind"], want["profile_kind"])
    print("end to end: %s survivors, %d samples at most, integers %s the statement's"
          % (host["nms_count"].tolist(), int(host["profile_counts"][..., 0].max()), "equal" if counts_equal else "differ from"))
    assert counts_equal
    worst = P.check_fits(host["profile_fits"], want["profile_fits"], host["nms_lines"], host["nms_count"], host["labels"], host["depth_mm"],
                         host["sizes"], max_samples=256, lo_mm=lo, hi_mm=hi)
    print("end to end: worst fit error / bound %.3g" % worst)
    # without line_nms: the rows above score_thresh, through `order`
    sess2 = InferenceSession(model, compute_dtype=torch.float32, graph=False, score_thresh=0.0, line_profiles=True)
    res2 = sess2.predict_frames(frames, size=96, max_size=128, copy=True)
    assert sorted(res2) == sorted(RESULT_KEYS + ("net_sizes",) + PROFILE_KEYS[:3])
    again = ops.line_profiles(res2["lines"], res2["count"], res2["labels"], res2["depth_mm"], res2["sizes"], order=res2["order"],
                              min_depth=sess2.min_depth, max_depth=sess2.max_depth)
    for k in PROFILE_KEYS[:3]:
        assert again[k].cpu().numpy().tobytes() == res2[k].cpu().numpy().tobytes(), k
    assert int(res2["count"].min()) >= 1 and int((res2["profile_fits"][..., 0, 4] == 0).sum()) >= 1
