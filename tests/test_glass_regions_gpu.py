"""GPU: gwd_glass_regions / gwd_region_planes / gwd_depth_planar (csrc/regions.hip) through ops.glass_regions against their
restatement (tests/regions_ref.py).

Integers (region_map, region_count, region_total, the records, n_used, status) are compared exactly, for both connectivities, and
every call is made twice with bit-identical results, the floats included.  A fitted plane, evaluated at all of its region's pixels
with depth, stays within (n + 64 kappa) 2^-52 max |w| of the oracle's (numpy.linalg.lstsq on centred columns; kappa = cond of the
centred normal matrix), rms within sqrt(n) times that.  The planar depth is compared with the oracle evaluated
with the kernel's OWN coefficients, so it does not depend on the fit's rounding: the fp32 value equals the correctly rounded fp64
value and the millimetres are equal; pixels whose fp64 value lies within 1e-9 mm of a rounding boundary may be left out (at most
0.1 % of the rewritten pixels) - tests/test_glass_regions.py confirms on the CPU that the fixtures put no pixel there, and with the
kernel's coefficients none has been seen either.  Pixels that are not rewritten are bit-equal to the input depth."""
import ctypes

import numpy as np
import pytest
import torch

from gw_depth_amd import hip, ops
from tests import regions_ref as R

pytestmark = pytest.mark.gpu

GOLDEN = {name: (mask, mm) for name, mask, mm in R.load_golden()}


def run(labels, depth_mm, sizes, depth=None, **kw):
    """ops.glass_regions twice on the device -> numpy dict; the two calls agree in every bit."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    dev = [torch.from_numpy(a).cuda() for a in (labels, depth_mm, sizes)]
    d = None if depth is None else torch.from_numpy(depth).cuda()
    torch.cuda.set_sync_debug_mode("error")                     # nothing in the call waits for the device
    try:
        one = ops.glass_regions(*dev, depth=d, **kw)
        two = ops.glass_regions(*dev, depth=d, **kw)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    out = {}
    for k in one:
        a, b = one[k].cpu().numpy(), two[k].cpu().numpy()
        assert a.tobytes() == b.tobytes(), "%s differs between two calls" % k
        out[k] = a
    return out


def check_integers(out, labels, depth_mm, sizes, max_regions=32, min_area=100, connectivity=8, max_candidates=8192, lo=1, hi=10000, **_):
    want = R.glass_regions(labels, depth_mm, sizes, max_regions, min_area, connectivity, lo, hi, max_candidates)
    for k in ("region_total", "region_count", "regions", "region_map"):
        assert np.array_equal(out[k], want[k]), (k, connectivity, np.argwhere(out[k] != want[k])[:5].tolist())
    return want


def check_planes(out, depth_mm, lo=1, hi=10000):
    """-> worst error / bound seen."""
    worst = 0.0
    B = out["planes"].shape[0]
    for b in range(B):
        K = max(int(out["region_count"][b]), 0)
        assert not out["planes"][b, K:].any()
        for r in range(K):
            x, y, w = R.region_pixels(out["region_map"][b], depth_mm[b], r, lo, hi)
            want = R.fit_plane(x, y, w)
            got = out["planes"][b, r]
            assert got[5] == want[5] and got[4] == want[4] == out["regions"][b, r, 8], (b, r, got, want)
            if want[5]:
                assert np.isnan(got[:4]).all()
                continue
            bound = (len(x) + 64.0 * R.normal_cond(x, y)) * 2.0 ** -52 * float(np.abs(w).max())
            err = float(np.abs(((got[0] * x + got[1] * y) + got[2]) - ((want[0] * x + want[1] * y) + want[2])).max())
            rms_err = abs(got[3] - want[3])
            worst = max(worst, err / bound, rms_err / (bound * np.sqrt(len(x))))
            assert err <= bound, (b, r, len(x), err, bound)
            assert rms_err <= bound * np.sqrt(len(x)), (b, r, len(x), got[3], want[3], bound)
    return worst


def check_planar(out, depth_mm, sizes, depth=None, min_depth=1e-3, max_depth=10.0):
    """-> number of rewritten pixels."""
    want, want_mm, hit, z = R.depth_planar(out["region_map"], depth_mm, depth, sizes, out["region_count"], out["planes"], min_depth, max_depth)
    assert out["depth_planar"].tobytes() == want.tobytes()      # rewritten: the correctly rounded fp64 value; the rest: the input's bits; 0 outside
    near = hit & (np.abs((z * 1000.0) % 1.0 - 0.5) <= 1e-9)
    assert int(near.sum()) <= 1e-3 * int(hit.sum())
    assert np.array_equal(out["depth_planar_mm"][~near], want_mm[~near])
    base = depth if depth is not None else depth_mm.astype(np.float32) / np.float32(1000.0)
    for b, (fh, fw) in enumerate(sizes):
        keep = ~hit[b, :fh, :fw]
        assert out["depth_planar"][b, :fh, :fw][keep].tobytes() == base[b, :fh, :fw][keep].tobytes()
        assert np.array_equal(out["depth_planar_mm"][b, :fh, :fw][keep], depth_mm[b, :fh, :fw][keep])
        assert not out["depth_planar"][b, fh:].any() and not out["depth_planar"][b, :, fw:].any()
        assert not out["depth_planar_mm"][b, fh:].any() and not out["depth_planar_mm"][b, :, fw:].any()
    return int(hit.sum())


def check_all(labels, depth_mm, sizes, depth=None, **kw):
    out = run(labels, depth_mm, sizes, depth=depth, **kw)
    lo, hi = ops.region_mm_range(kw.get("min_depth", 1e-3), kw.get("max_depth", 10.0))
    check_integers(out, labels, depth_mm, sizes, lo=lo, hi=hi, **kw)
    worst = check_planes(out, depth_mm, lo, hi)
    n = check_planar(out, depth_mm, sizes, depth, kw.get("min_depth", 1e-3), kw.get("max_depth", 10.0))
    print("regions kept %s of %s, %d pixels rewritten, worst plane error / bound %.3g"
          % (out["region_count"].tolist(), out["region_total"].tolist(), n, worst))
    return out


def hand_batch(h, w):
    masks = R.hand_masks(h, w)
    names = list(masks)
    return names, R.batch_of([(masks[n], R.plane_depth(masks[n], 7 + k)) for k, n in enumerate(names)])


@pytest.mark.parametrize("connectivity", [8, 4])
@pytest.mark.parametrize("hw", [(37, 53), (64, 70), (65, 129)], ids=lambda s: "%dx%d" % s)
def test_hand_built_masks(hw, connectivity):
    """Spiral, comb, U, checkerboard, full, empty, corners, ring, twins and diagonal as one batch of ten frames; the sizes put the
    shapes across the 64-pixel segments of a wave (70, 129), the 16-row chunks of the record pass and the 64 row-workgroups of
    the moment pass (65)."""
    names, (labels, depth_mm, sizes) = hand_batch(*hw)
    out = check_all(labels, depth_mm, sizes, min_area=1, connectivity=connectivity)
    at = {n: k for k, n in enumerate(names)}
    h, w = hw
    assert out["region_total"][at["checkerboard"]] == (1 if connectivity == 8 else (h * w + 1) // 2)
    assert out["region_total"][at["empty"]] == 0 and out["region_count"][at["empty"]] == 0 and not out["region_map"][at["empty"]].any()
    assert out["regions"][at["full"], 0, :6].tolist() == [h * w, 0, 0, w - 1, h - 1, 0]
    assert out["regions"][at["corners"], :4, 5].tolist() == [0, w - 1, (h - 1) * w, h * w - 1]
    assert out["regions"][at["twins"], :2, 0].tolist() == [24, 24] and out["regions"][at["twins"], 0, 5] < out["regions"][at["twins"], 1, 5]
    for n in ("spiral", "comb", "u", "ring"):
        assert out["region_total"][at[n]] == 1, n
    if connectivity == 8:
        assert out["region_total"][at["diagonal"]] == 1 and out["planes"][at["diagonal"], 0, 5] == 1.0      # collinear
        assert out["planes"][at["diagonal"], 0, 4] == min(h, w) - 2


@pytest.mark.parametrize("connectivity", [8, 4])
@pytest.mark.parametrize("outside", ["ones", "random"])
def test_ragged_batch_outside_never_leaks_in(outside, connectivity):
    """Three frames of different sizes in one 64 x 70 plane; what lies outside a frame is label 1 (it would join the frame's glass
    at its edges) or random bytes."""
    items = [GOLDEN["small"], GOLDEN["medium"], (R.hand_masks(50, 33)["ring"], R.plane_depth(R.hand_masks(50, 33)["ring"], 3))]
    if outside == "ones":
        labels, depth_mm, sizes = R.batch_of(items, fill_label=1, fill_mm=1500)
    else:
        labels, depth_mm, sizes = R.batch_of(items, rng=np.random.default_rng(11))
    out = check_all(labels, depth_mm, sizes, min_area=1, connectivity=connectivity)
    for b, (fh, fw) in enumerate(sizes):
        assert not out["region_map"][b, fh:].any() and not out["region_map"][b, :, fw:].any()


def test_a_frame_alone_and_in_the_batch():
    """The small fixture alone (its own 37 x 53 plane), in slot 0 and in slot 2 of a 64 x 70 batch: the integers are equal, every fit
    inside the bound."""
    small, medium = GOLDEN["small"], GOLDEN["medium"]
    alone = check_all(*R.batch_of([small]), min_area=1)
    first = check_all(*R.batch_of([small, medium, medium]), min_area=1)
    third = check_all(*R.batch_of([medium, medium, small]), min_area=1)
    h, w = small[0].shape
    for got, slot in ((first, 0), (third, 2)):
        for k in ("region_count", "region_total", "regions"):
            assert np.array_equal(got[k][slot], alone[k][0]), k
        assert np.array_equal(got["region_map"][slot, :h, :w], alone["region_map"][0])
        assert np.array_equal(got["planes"][slot, :, 4:], alone["planes"][0, :, 4:])


@pytest.mark.parametrize("connectivity", [8, 4])
@pytest.mark.parametrize("max_regions,min_area", [(32, 100), (4, 1)])
def test_large_fixture(max_regions, min_area, connectivity):
    """300 x 500: 104 components of 100 pixels or more (the 32 largest are kept), 120 components share an area (the tie-break), one
    region exactly planar, one without depth, one whose plane is not positive everywhere inside it."""
    labels, depth_mm, sizes = R.batch_of([GOLDEN["large"]])
    depth = (depth_mm.astype(np.float32) / np.float32(1000.0)) * np.float32(1.03125)      # a depth plane of its own: copied where nothing is rewritten
    out = check_all(labels, depth_mm, sizes, depth=depth, max_regions=max_regions, min_area=min_area, connectivity=connectivity)
    assert out["region_count"][0] == max_regions and out["region_total"][0] == (293 if connectivity == 8 else 298)
    if connectivity == 8:
        assert out["regions"][0, 1, 8] == 0 and out["planes"][0, 1, 5] == 1.0
        den = R.plane_denominator(out["planes"][0], out["region_map"][0])
        assert (den[out["region_map"][0] == 3] <= 0.0).any()


def test_too_many_candidates_refuses_that_image_alone():
    h, w = 37, 53
    masks = R.hand_masks(h, w)
    items = [(masks[n], R.plane_depth(masks[n], 5 + k)) for k, n in enumerate(("twins", "checkerboard", "ring"))]
    labels, depth_mm, sizes = R.batch_of(items)
    out = check_all(labels, depth_mm, sizes, min_area=1, connectivity=4, max_candidates=8, max_regions=8)
    assert out["region_count"].tolist() == [2, -1, 1] and out["region_total"].tolist() == [2, (h * w + 1) // 2, 1]
    assert not out["region_map"][1].any() and not out["regions"][1].any() and not out["planes"][1].any()
    assert out["depth_planar"][1].tobytes() == (depth_mm[1].astype(np.float32) / np.float32(1000.0)).tobytes()


def test_depth_range_and_clamp():
    """min_depth / max_depth decide which pixels have depth (millimetres 1200 .. 2600 here) and clamp the rewritten depth."""
    labels, depth_mm, sizes = R.batch_of([GOLDEN["medium"]])
    check_all(labels, depth_mm, sizes, min_area=20, min_depth=1.2, max_depth=2.6)


def test_status_returns_launch_nothing():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    lib = hip.library()
    B, Fh, Fw = 1, 8, 16
    labels = torch.ones((B, Fh, Fw), dtype=torch.uint8, device="cuda")
    mm = torch.full((B, Fh, Fw), 1000, dtype=torch.uint16, device="cuda")
    sizes = torch.tensor([[Fh, Fw]], dtype=torch.int32, device="cuda")
    ws = torch.zeros(lib.workspace_bytes(hip.WS_REGIONS, B, Fh, Fw, 64) + 16, dtype=torch.uint8, device="cuda")
    rmap = torch.full((B, Fh, Fw), 77, dtype=torch.uint8, device="cuda")
    count = torch.full((B,), 77, dtype=torch.int32, device="cuda")
    total = torch.full((B,), 77, dtype=torch.int32, device="cuda")
    rec = torch.full((B, 4, 12), 77, dtype=torch.int64, device="cuda")
    planes = torch.full((B, 4, 6), 77.0, dtype=torch.float64, device="cuda")
    dp = torch.full((B, Fh, Fw), 77.0, dtype=torch.float32, device="cuda")
    dpm = torch.full((B, Fh, Fw), 77, dtype=torch.uint16, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)

    def regions(labels_p=p(labels), B=B, R=4, area=1, conn=8, cand=64, lo=1, hi=10000, ws_p=p(ws), rec_p=p(rec), mm_p=p(mm)):
        return lib.lib.gwd_glass_regions(labels_p, mm_p, p(sizes), B, Fh, Fw, R, area, conn, cand, lo, hi, ws_p, p(rmap), p(count), p(total),
                                         rec_p, stream)

    assert regions(labels_p=None) == -1 and regions(B=0) == -1 and regions(B=17) == -1 and regions(R=0) == -1 and regions(R=33) == -1
    assert regions(area=0) == -1 and regions(cand=0) == -1 and regions(lo=0) == -1 and regions(hi=70000) == -1 and regions(lo=9, hi=8) == -1
    assert regions(conn=6) == -2
    assert regions(ws_p=p(ws, 8)) == -3 and regions(rec_p=p(rec, 4)) == -3 and regions(mm_p=p(mm, 1)) == -3

    def fit(R=4, lo=1, hi=10000, ws_p=p(ws), planes_p=p(planes), map_p=p(rmap)):
        return lib.lib.gwd_region_planes(map_p, p(mm), p(sizes), p(count), p(rec), B, Fh, Fw, R, lo, hi, ws_p, planes_p, stream)

    assert fit(map_p=None) == -1 and fit(R=40) == -1 and fit(lo=0) == -1 and fit(ws_p=p(ws, 4)) == -3 and fit(planes_p=p(planes, 4)) == -3

    def planar(dmin=1e-3, dmax=10.0, out_p=p(dp), planes_p=p(planes), depth_p=None):
        return lib.lib.gwd_depth_planar(p(rmap), p(mm), depth_p, p(sizes), p(count), planes_p, B, Fh, Fw, 4, dmin, dmax, out_p, p(dpm), stream)

    assert planar(planes_p=None) == -1 and planar(dmin=2.0, dmax=1.0) == -1 and planar(dmin=0.0) == -1 and planar(dmin=float("nan")) == -1
    assert planar(out_p=p(dp, 2)) == -3 and planar(depth_p=p(dp, 1)) == -3
    torch.cuda.synchronize()
    for t in (rmap, count, total, rec, planes, dp, dpm):
        assert (t == 77).all()
    assert regions() == 0 and fit() == 0 and planar() == 0      # ... and the same calls with good arguments run
    torch.cuda.synchronize()
    assert count.tolist() == [1] and rec[0, 0, 0] == Fh * Fw and (rmap == 1).all() and planes[0, 0, 5] == 0.0
    assert abs(float(planes[0, 0, 2]) - 1.0) < 1e-12 and (dpm == 1000).all()


# ------------------------------------------------------------------------------------------------------------------ end to end
class MemorySource:
    """What evaluate_frames needs of a source, over frames held in memory."""

    def __init__(self, frames, gt):
        self.rgb, self.gt = frames, gt

    def __len__(self):
        return len(self.rgb)

    def frames(self, idx):
        return [(self.rgb[i],) + self.gt[i] for i in idx]

    def name(self, i):
        return "frame%d" % i


def test_session_and_evaluate_frames_end_to_end():
    """Two synthetic frames (96 x 128 and 90 x 120) through InferenceSession(regions=True).predict_frames: REGION_KEYS agree with
    the oracle applied to the session's own labels / depth_mm / depth; a session without regions= returns the keys it always did
    and the same dense results; evaluate_frames(planar=True) runs, and against a ground truth whose glass is the predicted glass
    its non-glass rows equal those of planar=False bit for bit."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gw_depth_amd.evaluate import FrameMetrics, evaluate_frames
    from gw_depth_amd.infer import REGION_KEYS, RESULT_KEYS, InferenceSession
    from tests.golden_check import build
    _, model, _ = build(device="cuda")
    g = torch.Generator().manual_seed(4)
    frames = []
    for h, w in ((96, 128), (90, 120)):                          # smooth colour fields: the predicted glass comes in regions, not in specks
        low = torch.rand(1, 3, 6, 8, generator=g)
        frames.append((torch.nn.functional.interpolate(low, size=(h, w), mode="bicubic", align_corners=False)[0].clamp(0, 1) * 255)
                      .permute(1, 2, 0).to(torch.uint8).contiguous())
    plain = InferenceSession(model, compute_dtype=torch.float32, graph=False)
    sess = InferenceSession(model, compute_dtype=torch.float32, graph=False, regions={"min_area": 20})
    base = plain.predict_frames(frames, size=96, max_size=128, copy=True)
    assert sorted(base) == sorted(RESULT_KEYS + ("net_sizes",))
    res = sess.predict_frames(frames, size=96, max_size=128, copy=True)
    assert sorted(res) == sorted(RESULT_KEYS + ("net_sizes",) + REGION_KEYS)
    for k in base:
        assert torch.equal(base[k], res[k]), k
    out = {k: res[k].cpu().numpy() for k in REGION_KEYS}
    labels, depth_mm, depth, sizes = (res[k].cpu().numpy() for k in ("labels", "depth_mm", "depth", "sizes"))
    assert sizes.tolist() == [[96, 128], [90, 120]]
    check_integers(out, labels, depth_mm, sizes, min_area=20)
    worst = check_planes(out, depth_mm)
    n = check_planar(out, depth_mm, sizes, depth)
    print("end to end: kept %s of %s, %d pixels rewritten, worst plane error / bound %.3g"
          % (out["region_count"].tolist(), out["region_total"].tolist(), n, worst))
    gt = [((res["depth_mm"][b, :h, :w].to(torch.int32) + 150).contiguous(), (res["labels"][b, :h, :w] == 1).to(torch.uint8).contiguous())
          for b, (h, w) in enumerate(sizes.tolist())]
    source = MemorySource(frames, gt)
    rows = {}
    for planar in (False, True):
        fm = FrameMetrics("cuda", sess.min_depth, sess.max_depth, capacity_images=2)
        evaluate_frames(sess, source, batch=2, size=96, max_size=128, metrics=fm, planar=planar)
        rows[planar] = fm.per_image()
    assert rows[False]["sums"][:, 2].tobytes() == rows[True]["sums"][:, 2].tobytes()               # region 2 = non-glass
    assert rows[False]["measures"][:, 2].tobytes() == rows[True]["measures"][:, 2].tobytes()
    assert np.array_equal(rows[False]["confusion"], rows[True]["confusion"])
    if n:
        assert rows[False]["sums"][:, 1].tobytes() != rows[True]["sums"][:, 1].tobytes()           # the glass rows see the planes
    with pytest.raises(ValueError):
        evaluate_frames(plain, source, batch=2, size=96, max_size=128, planar=True)
