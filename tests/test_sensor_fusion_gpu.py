"""GPU: gwd_fusion_ring / gwd_fusion_planes / gwd_fusion_depth (csrc/fusion.hip) through ops.sensor_fusion against their restatement
(tests/fusion_ref.py), fed the device's own glass regions.

Every call is made twice under torch.cuda.set_sync_debug_mode("error") with bit-identical results, the floats included.  Integers
(fusion_ring, fused_source, n1, n_used, status, the three sums of the scale) are compared exactly; the trimmed sample set is the
oracle's evaluated with the kernel's OWN stored first coefficients and rms1, so the decision is bit-reproducible
(tests/test_sensor_fusion.py shows that with the oracle's coefficients no sample of these inputs lies within 1e-12 of the threshold).
Both fits, evaluated at all of their samples, stay within (n + 64 kappa) 2^-52 max |w| of numpy.linalg.lstsq on centred columns over
the same samples, rms within sqrt(n) times that.  The scale equals the fp64 quotient of the two integers.
depth_fused is compared bit for bit with the oracle evaluated with the kernel's own coefficients and scale; SENSOR pixels are the
input millimetres; depth_fused_mm is equal except where the fp64 value lies within 1e-9 mm of a rounding boundary (at most 0.1 % of
the PLANE + NETWORK pixels).

The tiles the shapes are chosen against: the row pass and the moment passes own 256 columns of one row per workgroup (the row pass
stages them with a 32-column halo either side), the column pass 256 columns x 16 rows with `ring` rows of halo above and below, the
fused pass (no halo) 1024 columns of a row where the width is a multiple of 4 and 256 otherwise; a wave is 64 neighbours of a row.
At ring 1 and 6, 40 x 300 is wider than the row and moment tiles plus both halos (256 + 2 ring <= 268) and taller than the column tile
plus its halos (16 + 2 ring <= 28); at ring 32 it is not (320 columns, 80 rows): there the windows reach across the whole frame and
every tile edge lies inside a window instead.  300 is wider than the fused pass's 256-column tile only in the variant it does not
take, so 20 x 1284 (a multiple of 4, above 1024) and 20 x 301 (not one, above 256) give either variant a second workgroup along x:
the index (blockIdx.x * 256 + threadIdx.x) * V with blockIdx.x > 0, the tail x >= Fw in the last workgroup and the 16-byte accesses
across a workgroup edge are compared with the oracle bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

from gw_depth_amd import hip, ops
from tests import fusion_ref as F
from tests import regions_ref as R

pytestmark = pytest.mark.gpu

FIELDS = ("sensor_mm", "labels", "depth", "depth_mm", "sizes")


def run(case, regions_kw=None, garbage=None, **opt):
    """The device's glass regions of a case, then ops.sensor_fusion twice -> (fusion results, region results) as numpy dicts.
    garbage: a numpy Generator - the region map is overwritten OUTSIDE every frame with random bytes, every rank 1 .. 32 among them."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    labels, sensor, depth, depth_mm, sizes = case
    dev = {k: torch.from_numpy(v).cuda() for k, v in zip(FIELDS, (sensor, labels, depth, depth_mm, sizes))}
    reg = ops.glass_regions(dev["labels"], dev["depth_mm"], dev["sizes"], depth=dev["depth"], **dict({"min_area": 1}, **(regions_kw or {})))
    if garbage is not None:
        rmap = reg["region_map"].cpu().numpy()
        noise = np.where(garbage.random(rmap.shape) < 0.5, garbage.integers(1, 33, rmap.shape), garbage.integers(0, 256, rmap.shape)).astype(np.uint8)
        for b, (fh, fw) in enumerate(sizes.tolist()):
            noise[b, :fh, :fw] = rmap[b, :fh, :fw]
        assert (noise != rmap).any()
        reg = dict(reg, region_map=torch.from_numpy(noise).cuda())
    args = dict(dev, region_map=reg["region_map"], region_count=reg["region_count"], regions=reg["regions"])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")                     # nothing in the call waits for the device
    try:
        one = ops.sensor_fusion(**args, **opt)
        two = ops.sensor_fusion(**args, **opt)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    out = {}
    for k in one:
        a, b = one[k].cpu().numpy(), two[k].cpu().numpy()
        assert a.tobytes() == b.tobytes(), "%s differs between two calls" % k
        out[k] = a
    assert tuple(out) == ops.FUSION_KEYS
    return out, {k: v.cpu().numpy() for k, v in reg.items()}


def fit_bound(x, y, w):
    return (len(x) + 64.0 * R.normal_cond(x, y)) * 2.0 ** -52 * float(np.abs(w).max())


def check_fit(got, x, y, w, where):
    """got = (alpha, beta, gamma, rms) of the kernel over the samples (x, y, w) -> error / bound."""
    want = R.fit_plane(x, y, w)
    assert want[5] == 0.0, where
    bound = fit_bound(x, y, w)
    err = float(np.abs(((got[0] * x + got[1] * y) + got[2]) - ((want[0] * x + want[1] * y) + want[2])).max())
    assert err <= bound, where + (len(x), err, bound)
    assert abs(got[3] - want[3]) <= bound * np.sqrt(len(x)), where + (len(x), got[3], want[3], bound)
    return max(err / bound, abs(got[3] - want[3]) / (bound * np.sqrt(len(x))))


def check(out, reg, case, ring=6, gap=1, trim=2.5, min_ring=50, max_rms=None, align=True, min_align=1000, min_depth=1e-3, max_depth=10.0):
    """-> (fits checked, worst error / bound, pixels by source)."""
    labels, sensor, depth, depth_mm, sizes = case
    lo, hi = ops.region_mm_range(min_depth, max_depth)
    Rmax = reg["regions"].shape[1]
    planes, scale = out["fusion_planes"], out["fusion_scale"]
    want = F.sensor_fusion(sensor, labels, depth, depth_mm, sizes, reg["region_map"], reg["region_count"], Rmax, ring=ring, gap=gap,
                           trim=trim, min_ring=min_ring, max_rms=max_rms, align=align, min_align=min_align, lo_mm=lo, hi_mm=hi,
                           min_depth=min_depth, max_depth=max_depth, first=planes, use_planes=planes, use_scale=scale)
    # ---- exact
    for k in ("fusion_ring", "fused_source"):
        assert np.array_equal(out[k], want[k]), (k, np.argwhere(out[k] != want[k])[:5].tolist())
    for f in (4, 9, 10, 11):
        assert np.array_equal(planes[:, :, f], want["fusion_planes"][:, :, f]), (F.PLANE_FIELDS[f], planes[:, :, f], want["fusion_planes"][:, :, f])
    assert np.array_equal(scale[:, 1:], want["fusion_scale"][:, 1:]), (scale, want["fusion_scale"])
    for b in range(len(sizes)):
        n, sp, pp = scale[b, 1:]
        assert scale[b, 0] == (sp / pp if align and n >= min_align and pp > 0 else 1.0)      # the fp64 quotient of the two integers
    # ---- the two fits of every kept region, over the samples the kernel's own stored first fit keeps
    fits, worst = 0, 0.0
    for b, (fh, fw) in enumerate(sizes.tolist()):
        K = max(int(reg["region_count"][b]), 0)
        assert not planes[b, K:].any()
        for r in range(K):
            row = planes[b, r]
            x, y, w = F.ring_samples(out["fusion_ring"][b, :fh, :fw], sensor[b, :fh, :fw], r)
            assert row[4] == len(x)
            if R.fit_plane(x, y, w)[5]:
                assert row[10] == 1.0 and np.isnan(row[:4]).all() and np.isnan(row[5:9]).all() and row[9] == len(x)
                continue
            worst = max(worst, check_fit(row[:4], x, y, w, (b, r, "first")))
            fits += 1
            if trim > 0 and row[3] > 0:
                keep, _, _ = F.trim_keep(x, y, w, row[:4], trim)
                assert row[9] == int(keep.sum())
                if R.fit_plane(x[keep], y[keep], w[keep])[5]:
                    assert row[10] == 1.0 and np.isnan(row[5:9]).all()
                    continue
                worst = max(worst, check_fit(row[5:9], x[keep], y[keep], w[keep], (b, r, "second")))
                fits += 1
            else:
                assert row[5:9].tobytes() == row[:4].tobytes() and row[9] == row[4]
            rejected = row[9] < min_ring or (max_rms is not None and row[8] > max_rms)
            assert row[10] == (2.0 if rejected else 0.0)
    # ---- the fused depth, with the kernel's own coefficients and scale
    assert out["depth_fused"].tobytes() == want["depth_fused"].tobytes()
    src = out["fused_source"]
    rewritten = src >= F.PLANE
    near = rewritten & (np.abs((want["z"] * 1000.0) % 1.0 - 0.5) <= 1e-9)
    assert int(near.sum()) <= 1e-3 * int(rewritten.sum())
    assert np.array_equal(out["depth_fused_mm"][~near], want["depth_fused_mm"][~near])
    assert np.array_equal(out["depth_fused_mm"][src == F.SENSOR], sensor[src == F.SENSOR])
    for b, (fh, fw) in enumerate(sizes.tolist()):
        assert (src[b, :fh, :fw] > 0).all()
        for k in ("depth_fused", "depth_fused_mm", "fused_source", "fusion_ring"):
            assert not out[k][b, fh:].any() and not out[k][b, :, fw:].any(), k
    by_source = [int((src == v).sum()) for v in (F.SENSOR, F.PLANE, F.NETWORK)]
    return fits, worst, by_source


def check_all(case, regions_kw=None, garbage=None, **opt):
    out, reg = run(case, regions_kw, garbage, **opt)
    fits, worst, by_source = check(out, reg, case, **opt)
    print("kept %s, %d fits, worst error / bound %.3g, sensor / plane / network pixels %s, status %s"
          % (reg["region_count"].tolist(), fits, worst, by_source, sorted(set(out["fusion_planes"][:, :, 10].ravel().tolist()))))
    return out, reg


@pytest.mark.parametrize("ring,gap", F.RINGS, ids=lambda v: str(v))
@pytest.mark.parametrize("hw", F.SHAPES, ids=lambda s: "%dx%d" % s)
def test_hand_built_masks(hw, ring, gap):
    """A cross touching all four borders, a region that fills the frame (no ring: status 1, NETWORK everywhere), two panes closer
    than 2 ring (the smaller rank wins between them), one pane, no glass - as one batch of five frames, at a row shorter than a wave
    (53), across wave and tile edges (70, 129, 300) and across the 16-row tiles of the column pass (37 .. 65)."""
    out, reg = check_all(F.hand_case(*hw), ring=ring, gap=gap)
    names = list(F.masks_for(*hw))
    full, pair, empty, cross = (names.index(n) for n in ("full", "pair", "empty", "cross"))
    assert reg["region_count"][full] == 1 and not out["fusion_ring"][full].any() and out["fusion_planes"][full, 0, 10] == 1.0
    assert out["fusion_planes"][full, 0, 4] == 0 and (out["fused_source"][full] == F.NETWORK).all() and out["fusion_scale"][full, 0] == 1.0
    assert reg["region_count"][empty] == 0 and not out["fusion_ring"][empty].any() and not (out["fused_source"][empty] == F.PLANE).any()
    assert reg["region_count"][pair] == 2 and reg["regions"][cross, 0, 1:5].tolist() == [0, 0, hw[1] - 1, hw[0] - 1]
    if ring >= 6 and gap == 0:
        between = out["fusion_ring"][pair, 10:30, hw[1] // 2 - 1:hw[1] // 2 + 2]
        assert (between[between > 0] == 1).all() and (ring > 6 or (out["fusion_ring"][pair] == 2).any())
    if ring == 6 and gap == 0 and hw[0] >= 64:
        assert out["fusion_planes"][names.index("pane"), 0, 10] == 0.0 and (out["fused_source"][names.index("pane")] == F.PLANE).any()


@pytest.mark.parametrize("hw", F.WIDE, ids=lambda s: "%dx%d" % s)
def test_fused_pass_beyond_one_workgroup(hw):
    """The five hand-built masks at 20 x 1284 (four pixels per thread: 1024 columns per workgroup, the second one ends in the tail
    x >= Fw) and at 20 x 301 (one pixel per thread: 256 columns per workgroup): every output against the oracle as everywhere else,
    depth_fused bit for bit, with PLANE and NETWORK pixels on both sides of the workgroup edge."""
    out, reg = check_all(F.hand_case(*hw))
    edge = 1024 if hw[1] % 4 == 0 else 256
    src = out["fused_source"]
    for side in (src[:, :, :edge], src[:, :, edge:]):
        assert all((side == v).any() for v in (F.SENSOR, F.PLANE, F.NETWORK))


@pytest.mark.parametrize("name,opt", [("small", {}), ("medium", {"trim": 0.0}), ("medium", {"max_rms": 2e-3, "min_ring": 200}),
                                      ("large", {}), ("large", {"ring": 32, "gap": 3, "align": False})],
                         ids=["small", "medium-trim0", "medium-rejects", "large", "large-ring32"])
def test_golden_masks(name, opt):
    """The 300 x 500 masks of tests/golden/glass_regions.npz with a seeded sensor plane: the wall behind the panes inside the glass, 5 %
    outliers at twice the depth near it, 3 % holes.  The large one keeps 32 of 104 regions, many of them closer than 2 ring."""
    out, reg = check_all(F.golden_case(name), {"min_area": 100} if name == "large" else None, **opt)
    status = out["fusion_planes"][:, :, 10]
    K = int(reg["region_count"][0])
    if name == "large":
        assert K == 32 and (status[0, :K] == 0.0).any()
    if opt.get("min_ring") == 200:
        assert (status[0, :K] == 2.0).any()
    if opt.get("align") is False:
        assert out["fusion_scale"][0, 0] == 1.0 and out["fusion_scale"][0, 1] > 1000


@pytest.mark.parametrize("value", [0, 65535])
def test_a_sensor_without_a_valid_reading(value):
    """All zeros / all 65535 (outside 1 .. 10000 mm): no ring, no scale, every region status 1, every pixel from the network."""
    labels, sensor, depth, depth_mm, sizes = F.hand_case(64, 70)
    sensor = np.full_like(sensor, value)
    out, reg = check_all((labels, sensor, depth, depth_mm, sizes))
    assert not out["fusion_ring"].any() and (out["fusion_scale"] == [[1.0, 0.0, 0.0, 0.0]]).all()
    for b, K in enumerate(reg["region_count"].tolist()):
        assert (out["fusion_planes"][b, :K, 10] == 1.0).all() and (out["fused_source"][b] == F.NETWORK).all()
        assert out["depth_fused"][b].tobytes() == np.clip(depth[b], np.float32(1e-3), np.float32(10.0)).tobytes()


def ragged_items():
    masks = {hw: F.masks_for(*hw) for hw in ((37, 53), (50, 33), (64, 70))}
    picks = (((37, 53), "pair"), ((50, 33), "pane"), ((64, 70), "cross"))
    return [(masks[hw][n],) + F.sensor_for(masks[hw][n], 60 + k) for k, (hw, n) in enumerate(picks)]


def test_ragged_batch_outside_never_leaks_in():
    """Three frames of different sizes in one 64 x 70 plane, random bytes outside the frames in all five planes - labels, sensor,
    depth, depth_mm and the region map itself (overwritten behind glass_regions, half of the bytes ranks of kept regions): the
    results equal those of the same frames with a quiet outside."""
    noisy = F.batch_of(ragged_items(), rng=np.random.default_rng(11))
    quiet = F.batch_of(ragged_items())
    a, _ = check_all(noisy, garbage=np.random.default_rng(12), ring=6, gap=1, min_ring=20)
    b, _ = check_all(quiet, ring=6, gap=1, min_ring=20)
    for k in ops.FUSION_KEYS:
        assert a[k].tobytes() == b[k].tobytes(), k


def test_a_frame_alone_and_in_the_batch():
    """A frame alone (its own 37 x 53 plane: the scalar fused pass), in slot 0 and in slot 2 of a 64 x 72 batch (the 4-pixel fused
    pass): every per-frame result is identical, the floats included - no result depends on the plane or on the neighbours."""
    items = ragged_items()
    alone, _ = check_all(F.batch_of([items[0]]), min_ring=20)
    first, _ = check_all(F.batch_of([items[0], items[2], items[1]], Fw=72), min_ring=20)
    third, _ = check_all(F.batch_of([items[1], items[2], items[0]], Fw=72), min_ring=20)
    h, w = items[0][0].shape
    assert (alone["fusion_planes"][0, :2, 10] == 0.0).all()
    for got, slot in ((first, 0), (third, 2)):
        for k in ("fusion_planes", "fusion_scale"):
            assert got[k][slot].tobytes() == alone[k][0].tobytes(), k
        for k in ("depth_fused", "depth_fused_mm", "fused_source", "fusion_ring"):
            assert got[k][slot, :h, :w].tobytes() == alone[k][0].tobytes(), k


def test_a_refused_image_has_no_planes():
    """max_candidates = 1: the frame with two panes is refused (region_count -1) - no ring, no planes, its glass from the network, its
    scale still measured; its neighbours are untouched."""
    items = ragged_items()
    out, reg = check_all(F.batch_of([items[1], items[0], items[2]]), {"max_candidates": 1}, min_ring=20, min_align=100)
    assert reg["region_count"].tolist() == [1, -1, 1]
    assert not out["fusion_planes"][1].any() and not out["fusion_ring"][1].any() and not (out["fused_source"][1] == F.PLANE).any()
    assert out["fusion_scale"][1, 1] >= 100 and out["fusion_scale"][1, 0] != 1.0
    assert (out["fused_source"][0] == F.PLANE).any() and (out["fused_source"][2] == F.PLANE).any()


def test_status_returns_launch_nothing():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    lib = hip.library()
    B, Fh, Fw, Rm = 1, 8, 16, 4
    cu = lambda shape, dt, v: torch.full(shape, v, dtype=dt, device="cuda")
    labels = cu((B, Fh, Fw), torch.uint8, 0)
    labels[:, 2:6, 4:12] = 1
    rmap = (labels == 1).to(torch.uint8)
    sensor, mm = cu((B, Fh, Fw), torch.uint16, 2000), cu((B, Fh, Fw), torch.uint16, 1000)
    depth = cu((B, Fh, Fw), torch.float32, 1.0)
    sizes = torch.tensor([[Fh, Fw]], dtype=torch.int32, device="cuda")
    count = cu((B,), torch.int32, 1)
    rec = torch.zeros((B, Rm, 12), dtype=torch.int64, device="cuda")
    rec[0, 0, :5] = torch.tensor([32, 4, 2, 11, 5])
    ws = torch.zeros(lib.workspace_bytes(hip.WS_FUSION, B, Fh, Fw) + 16, dtype=torch.uint8, device="cuda")
    ring = cu((B, Fh, Fw), torch.uint8, 77)
    scale = cu((B, 4), torch.float64, 77.0)
    planes = cu((B, Rm, 12), torch.float64, 77.0)
    fused, fused_mm, source = cu((B, Fh, Fw), torch.float32, 77.0), cu((B, Fh, Fw), torch.uint16, 77), cu((B, Fh, Fw), torch.uint8, 77)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    c_double = ctypes.c_double

    def do_ring(labels_p=p(labels), B=B, R=Rm, ring_w=2, gap=1, lo=1, hi=10000, min_align=0, ws_p=p(ws), scale_p=p(scale), mm_p=p(mm)):
        return lib.lib.gwd_fusion_ring(labels_p, p(sensor), mm_p, p(sizes), p(rmap), p(count), B, Fh, Fw, R, ring_w, gap, lo, hi, 1, min_align,
                                       ws_p, p(ring), scale_p, stream)

    assert do_ring(labels_p=None) == -1 and do_ring(B=0) == -1 and do_ring(B=17) == -1 and do_ring(R=0) == -1 and do_ring(R=33) == -1
    assert do_ring(lo=0) == -1 and do_ring(hi=70000) == -1 and do_ring(lo=9, hi=8) == -1 and do_ring(min_align=-1) == -1
    assert do_ring(ring_w=0) == -2 and do_ring(ring_w=33) == -2 and do_ring(gap=-1) == -2 and do_ring(gap=2) == -2
    assert do_ring(ws_p=p(ws, 8)) == -3 and do_ring(scale_p=p(scale, 4)) == -3 and do_ring(mm_p=p(mm, 1)) == -3

    def do_planes(ring_p=p(ring), R=Rm, ring_w=2, lo=1, hi=10000, trim=2.5, min_ring=3, max_rms=float("inf"), ws_p=p(ws), planes_p=p(planes)):
        return lib.lib.gwd_fusion_planes(ring_p, p(sensor), p(sizes), p(count), p(rec), B, Fh, Fw, R, ring_w, lo, hi, c_double(trim), min_ring,
                                         c_double(max_rms), ws_p, planes_p, stream)

    assert do_planes(ring_p=None) == -1 and do_planes(R=40) == -1 and do_planes(lo=0) == -1 and do_planes(min_ring=-1) == -1
    assert do_planes(ring_w=0) == -2 and do_planes(trim=-1.0) == -2 and do_planes(trim=float("nan")) == -2 and do_planes(max_rms=-1.0) == -2
    assert do_planes(max_rms=float("nan")) == -2 and do_planes(ws_p=p(ws, 4)) == -3 and do_planes(planes_p=p(planes, 4)) == -3

    def do_depth(dmin=1e-3, dmax=10.0, lo=1, hi=10000, out_p=p(fused), planes_p=p(planes), depth_p=p(depth)):
        return lib.lib.gwd_fusion_depth(p(labels), p(sensor), depth_p, p(sizes), p(rmap), p(count), planes_p, p(scale), B, Fh, Fw, Rm, lo, hi,
                                        dmin, dmax, out_p, p(fused_mm), p(source), stream)

    assert do_depth(planes_p=None) == -1 and do_depth(depth_p=None) == -1 and do_depth(dmin=2.0, dmax=1.0) == -1 and do_depth(dmin=0.0) == -1
    assert do_depth(dmin=float("nan")) == -1 and do_depth(hi=70000) == -1 and do_depth(out_p=p(fused, 2)) == -3 and do_depth(depth_p=p(depth, 1)) == -3
    torch.cuda.synchronize()
    for t in (ring, scale, planes, fused, fused_mm, source):
        assert (t == 77).all()
    assert do_ring() == 0 and do_planes() == 0 and do_depth() == 0          # ... and the same calls with good arguments run
    torch.cuda.synchronize()
    assert scale[0].tolist() == [2.0, 68.0, 68 * 2000.0 * 1000.0, 68 * 1e6]             # 8 x 16 less the glass and the gap around it
    assert int((ring == 1).sum()) == 36 and int((ring == 0).sum()) == 128 - 36 and planes[0, 0, 10] == 0.0
    assert planes[0, 0, 4] == 36 and abs(float(planes[0, 0, 2]) - 0.5) < 1e-12 and planes[0, 0, 3] == 0.0 and planes[0, 0, 9] == 36
    assert (source[labels == 0] == 1).all() and (source[labels == 1] == 2).all() and (fused_mm == 2000).all()


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
    """Two synthetic frames (96 x 128 and 90 x 120) through InferenceSession(regions=..., fusion=...).predict_frames(sensor_depth=):
    FUSION_KEYS equal ops.sensor_fusion on the call's own outputs and pass the checks above; a session without fusion= returns
    exactly the keys and values it always did, and so does a call without sensor_depth; evaluate_frames(fused=True, sensor=) equals
    FrameMetrics fed depth_fused by hand."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gw_depth_amd.evaluate import FrameMetrics, evaluate_frames
    from gw_depth_amd.infer import FUSION_KEYS, REGION_KEYS, RESULT_KEYS, InferenceSession
    from tests.golden_check import build
    _, model, _ = build(device="cuda")
    g = torch.Generator().manual_seed(4)
    frames = []
    for h, w in ((96, 128), (90, 120)):                          # smooth colour fields: the predicted glass comes in regions, not in specks
        low = torch.rand(1, 3, 6, 8, generator=g)
        frames.append((torch.nn.functional.interpolate(low, size=(h, w), mode="bicubic", align_corners=False)[0].clamp(0, 1) * 255)
                      .permute(1, 2, 0).to(torch.uint8).contiguous())
    regions = {"min_area": 20}
    fusion = {"ring": 4, "min_ring": 20, "min_align": 100}
    plain = InferenceSession(model, compute_dtype=torch.float32, graph=False, regions=regions)
    sess = InferenceSession(model, compute_dtype=torch.float32, graph=False, regions=regions, fusion=fusion)
    base = plain.predict_frames(frames, size=96, max_size=128, copy=True)
    assert sorted(base) == sorted(RESULT_KEYS + ("net_sizes",) + REGION_KEYS)
    sizes = base["sizes"].cpu().numpy().tolist()
    rng = np.random.default_rng(9)
    planes = []
    for b, (h, w) in enumerate(sizes):                           # the sensor: the network's depth / 1.2, twice as far behind the glass, 3 % holes
        mm = base["depth_mm"][b, :h, :w].cpu().numpy().astype(np.float64) / 1.2
        mm = np.where(base["labels"][b, :h, :w].cpu().numpy() == 1, 2.0 * mm, mm)
        mm = np.where(rng.random((h, w)) < 0.03, 0.0, mm)
        planes.append(torch.from_numpy(np.clip(np.rint(mm), 0, 65535).astype(np.uint16)))
    quiet = sess.predict_frames(frames, size=96, max_size=128, copy=True)
    assert sorted(quiet) == sorted(base)
    for k in base:
        assert base[k].cpu().numpy().tobytes() == quiet[k].cpu().numpy().tobytes(), k
    res = sess.predict_frames(frames, size=96, max_size=128, copy=True, sensor_depth=[planes[0], planes[1].cuda()])
    assert sorted(res) == sorted(RESULT_KEYS + ("net_sizes",) + REGION_KEYS + FUSION_KEYS)
    for k in base:
        assert base[k].cpu().numpy().tobytes() == res[k].cpu().numpy().tobytes(), k
    packed = torch.zeros((2, 96, 128), dtype=torch.uint16)
    for b, (h, w) in enumerate(sizes):
        packed[b, :h, :w] = planes[b]
    direct = ops.sensor_fusion(packed.cuda(), res["labels"], res["depth"], res["depth_mm"], res["sizes"], res["region_map"],
                               res["region_count"], res["regions"], min_depth=sess.min_depth, max_depth=sess.max_depth, **fusion)
    for k in FUSION_KEYS:
        assert res[k].cpu().numpy().tobytes() == direct[k].cpu().numpy().tobytes(), k
    case = (res["labels"].cpu().numpy(), packed.numpy(), res["depth"].cpu().numpy(), res["depth_mm"].cpu().numpy(), res["sizes"].cpu().numpy())
    reg = {k: res[k].cpu().numpy() for k in ("region_map", "region_count", "regions")}
    fits, worst, by_source = check({k: res[k].cpu().numpy() for k in FUSION_KEYS}, reg, case, min_depth=sess.min_depth, max_depth=sess.max_depth,
                                   **fusion)
    print("end to end: kept %s, %d fits, worst error / bound %.3g, sensor / plane / network pixels %s"
          % (reg["region_count"].tolist(), fits, worst, by_source))
    with pytest.raises(ValueError, match="fusion="):
        plain.predict_frames(frames, size=96, max_size=128, sensor_depth=planes)
    with pytest.raises(ValueError, match="frame 1"):
        sess.predict_frames(frames, size=96, max_size=128, sensor_depth=[planes[0], planes[0]])
    gt = [((res["depth_mm"][b, :h, :w].to(torch.int32) + 150).contiguous(), (res["labels"][b, :h, :w] == 1).to(torch.uint8).contiguous())
          for b, (h, w) in enumerate(sizes)]
    source = MemorySource(frames, gt)
    auto = FrameMetrics("cuda", sess.min_depth, sess.max_depth, capacity_images=2)
    evaluate_frames(sess, source, batch=2, size=96, max_size=128, metrics=auto, fused=True, sensor=lambda idx: [planes[i] for i in idx])
    hand = FrameMetrics("cuda", sess.min_depth, sess.max_depth, capacity_images=2)
    hand.update(dict(res, depth=res["depth_fused"]), gt, ids=[0, 1])
    depth_only = FrameMetrics("cuda", sess.min_depth, sess.max_depth, capacity_images=2)
    depth_only.update(res, gt, ids=[0, 1])
    a, h_, d = auto.per_image(), hand.per_image(), depth_only.per_image()
    for k in ("sums", "measures", "confusion"):
        assert np.asarray(a[k]).tobytes() == np.asarray(h_[k]).tobytes(), k
    assert np.asarray(a["sums"]).tobytes() != np.asarray(d["sums"]).tobytes()                # ... and it is the fused depth that was scored
    with pytest.raises(ValueError, match="fusion="):
        evaluate_frames(plain, source, batch=2, size=96, max_size=128, fused=True, sensor=lambda idx: [planes[i] for i in idx])
