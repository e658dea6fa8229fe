"""GPU: gwd_point_cloud (csrc/cloud.hip) through ops.point_cloud against its statement (tests/cloud_ref.py).

cloud_offsets, the zero tail, every uint8 field, the flags and x y z are compared exactly: a position is a handful of fp64 + - * /
in a fixed order, correctly rounded on both sides, then one rounding to float32.  Every component of a normal stays within 2^-23 of
the statement's - one float32 unit at magnitude <= 1: an fp64 sqrt or divide that differs in its last place may push a component
across one float32 rounding boundary, nothing more - and whether a normal is zero is exact.  Every call is made twice under
torch.cuda.set_sync_debug_mode("error"); the two results agree in every byte."""
import numpy as np
import pytest
import torch

from gw_depth_amd import hip, ops
from tests import cloud_cases as K
from tests import cloud_ref as C

pytestmark = pytest.mark.gpu

GOLD = K.load_golden()
NORMAL_BOUND = 2.0 ** -23


def run(depth, labels, sizes, intrinsics, frames=None, region_map=None, region_count=None, planes=None, source=None, poses=None, **kw):
    """ops.point_cloud twice on the device -> numpy dict; the two calls agree in every byte."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    args = [dev(a) for a in (depth, labels, sizes, intrinsics)]
    opt = dict(frames=None if frames is None else [dev(f) for f in frames], region_map=dev(region_map), region_count=dev(region_count),
               planes=dev(planes), source=dev(source), poses=dev(poses), **kw)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")                     # nothing in the call waits for the device
    try:
        one = ops.point_cloud(*args, **opt)
        two = ops.point_cloud(*args, **opt)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    out = {}
    for k in ops.CLOUD_KEYS:
        a, b = one[k].cpu().numpy(), two[k].cpu().numpy()
        assert a.tobytes() == b.tobytes(), "%s differs between two calls" % k
        out[k] = a
    return out


def check(out, want, what=""):
    """Exact but for the normals, which stay within NORMAL_BOUND per component -> (components that differ at all, components)."""
    assert np.array_equal(out["cloud_offsets"], want["cloud_offsets"]), (what, out["cloud_offsets"], want["cloud_offsets"])
    assert out["cloud"].shape == want["cloud"].shape, what
    total = int(want["cloud_offsets"][-1])
    assert not out["cloud"][total:].any(), "%s: the tail is not zero" % what
    got, ref = out["cloud"].view(C.RECORD).ravel()[:total], want["cloud"].view(C.RECORD).ravel()[:total]
    for f in ("rgb", "label", "region", "source", "frame", "flags"):
        assert np.array_equal(got[f], ref[f]), (what, f, np.argwhere(got[f] != ref[f])[:5].tolist())
    assert got["xyz"].tobytes() == ref["xyz"].tobytes(), (what, "xyz", np.argwhere(got["xyz"].view(np.uint32) != ref["xyz"].view(np.uint32))[:5].tolist())
    assert np.array_equal(got["normal"] == 0, ref["normal"] == 0), (what, "a normal's zeros")
    assert np.array_equal((got["normal"] != 0).any(1), (got["flags"] & C.HAS_NORMAL) != 0), (what, "flag 2 and the normal disagree")
    err = np.abs(got["normal"].astype(np.float64) - ref["normal"].astype(np.float64))
    assert total == 0 or err.max() <= NORMAL_BOUND, (what, "normal", float(err.max()))
    return int((got["normal"].view(np.uint32) != ref["normal"].view(np.uint32)).sum()), 3 * total


def scene_run(cfg, **kw):
    return run(GOLD["depth"], GOLD["labels"], GOLD["sizes"], GOLD["intrinsics"], frames=GOLD["frames"] if cfg["frames"] else None,
               region_map=GOLD["region_map"], region_count=GOLD["region_count"], planes=GOLD["planes"], source=GOLD["source"],
               poses=GOLD["poses"] if cfg["poses"] else None, stride=cfg["stride"], min_depth=K.MIN_DEPTH, max_depth=K.MAX_DEPTH,
               edge=cfg["edge"], normals=cfg["normals"], keep=cfg["keep"], **kw)


@pytest.mark.parametrize("stride", [1, 2, 3])
def test_fixture(stride):
    """tests/golden/point_cloud.npz (tests/cloud_cases.py describes the scene) at one stride, for edge None and 0.05, the three values
    of keep, with and without frames, poses and normals: 48 configurations, each against the statement."""
    T = hip.CLOUD_TILE
    fh, fw = (int(v) for v in GOLD["sizes"][0])
    assert fh * fw > 2 * T and (fh * fw) % T != 0 and fh % 3 and fw % 3              # a changed tile size cannot empty the case
    differ = comps = n = 0
    for cfg in K.GRID:
        if cfg["stride"] != stride:
            continue
        d, c = check(scene_run(cfg), K.statement(GOLD, cfg), K.config_id(cfg))
        differ, comps, n = differ + d, comps + c, n + 1
    assert n == 48
    print("stride %d: %d of %d normal components differ from the statement's at all (bound 2^-23 each)" % (stride, differ, comps))


def test_recorded_results_and_capacities():
    """The clouds stored in the fixture; a capacity above the default (zeros behind the points) and the exact one for sizes known on
    the host: the same points."""
    for cfg in K.RECORDED:
        want = {k: GOLD["%s.%s" % (K.config_id(cfg), k)] for k in ops.CLOUD_KEYS}
        out = scene_run(cfg)
        check(out, want, K.config_id(cfg))
        rows = sum(-(-h // cfg["stride"]) * -(-w // cfg["stride"]) for h, w in K.SIZES)
        for cap, sizes in ((want["cloud"].shape[0] + 1000, None), (rows, K.SIZES)):
            other = scene_run(cfg, capacity=cap, frame_sizes=sizes)
            assert other["cloud"].shape[0] == cap and np.array_equal(other["cloud_offsets"], out["cloud_offsets"])
            total = int(out["cloud_offsets"][-1])
            assert other["cloud"][:total].tobytes() == out["cloud"][:total].tobytes() and not other["cloud"][total:].any()


def test_same_frame_same_rows_in_another_slot_and_plane():
    """Frame 0 of the fixture in slot 0 of its own plane, and in slot 1 of a (2, 70, 64) plane of noise behind a frame of noise: its
    rows are the same in every byte but `frame`, at another offset."""
    cfg = dict(stride=1, edge=0.05, keep="all", frames=True, poses=True, normals=True)
    base = scene_run(cfg)
    rng = np.random.default_rng(7)
    h, w = K.SIZES[0]
    depth = rng.uniform(0.0, 9.0, (2, 70, 64)).astype(np.float32)
    planes8 = [rng.integers(0, 256, (2, 70, 64), dtype=np.uint8) for _ in range(3)]           # labels, region_map, source
    depth[1, :h, :w] = GOLD["depth"][0]
    for dst, key in zip(planes8, ("labels", "region_map", "source")):
        dst[1, :h, :w] = GOLD[key][0]
    pick = lambda a: np.stack([a[1], a[0]])
    frames = [rng.integers(0, 256, (70, 64, 3), dtype=np.uint8), GOLD["frames"][0]]
    moved = run(depth, planes8[0], np.array([(70, 64), (h, w)], np.int32), pick(GOLD["intrinsics"]), frames=frames, region_map=planes8[1],
                region_count=pick(GOLD["region_count"]), planes=pick(GOLD["planes"]), source=planes8[2], poses=pick(GOLD["poses"]),
                stride=1, min_depth=K.MIN_DEPTH, max_depth=K.MAX_DEPTH, edge=0.05)
    n = int(base["cloud_offsets"][1])
    lo, hi = (int(v) for v in moved["cloud_offsets"][1:])
    assert hi - lo == n and lo > 0 and n > hip.CLOUD_TILE
    a, b = base["cloud"][:n].copy(), moved["cloud"][lo:hi].copy()
    assert (a[:, 30] == 0).all() and (b[:, 30] == 1).all()
    a[:, 30] = b[:, 30] = 0
    assert a.tobytes() == b.tobytes()


def test_scan_thread_owns_two_tiles():
    """More tiles than the scan workgroup has threads: 513 + 514 tiles, so a scan thread owns two, the frame boundary (block 513)
    falls inside one thread's pair, thread 513 owns a single tile and the threads above it none."""
    T = hip.CLOUD_TILE
    sizes = [(749, 700), (750, 701)]
    per_frame = [-(-h * w // T) for h, w in sizes]
    tiles = sum(per_frame)
    assert tiles > 1024 and tiles % 2 == 1 and per_frame[0] % 2 == 1          # a changed tile size cannot empty the case
    rng = np.random.default_rng(513)
    depth = rng.uniform(0.5, 7.5, (2, 750, 701)).astype(np.float32)
    depth[rng.random(depth.shape) < 0.3] = 0.0
    labels = rng.integers(0, 256, depth.shape, dtype=np.uint8)
    cam = np.array([(600.0, 610.0, 350.0, 374.0), (590.0, 585.0, 352.5, 371.0)], np.float64)
    kw = dict(stride=1, min_depth=K.MIN_DEPTH, max_depth=K.MAX_DEPTH, normals=True)
    want = C.point_cloud(depth, labels, np.array(sizes, np.int32), cam, **kw)
    out = run(depth, labels, np.array(sizes, np.int32), cam, frame_sizes=sizes, **kw)
    total = int(want["cloud_offsets"][-1])
    assert 0.6 * 749 * 700 < int(want["cloud_offsets"][1]) < 749 * 700 and total < out["cloud"].shape[0]
    differ, comps = check(out, want, "1027 tiles")
    print("1027 tiles: %d points, %d of %d normal components differ at all" % (total, differ, comps))


def test_session_end_to_end():
    """Two synthetic frames through InferenceSession(regions, fusion, cloud).predict_frames(sensor_depth, intrinsics, poses): the cloud
    equals ops.point_cloud applied to the returned tensors (bit for bit) and the statement under the bounds above; every other key
    is bit-equal to a session without cloud=."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gw_depth_amd.infer import CLOUD_KEYS, FUSION_KEYS, REGION_KEYS, RESULT_KEYS, InferenceSession
    from tests.golden_check import build
    _, model, _ = build(device="cuda")
    g = torch.Generator().manual_seed(4)
    frames, sensor = [], []
    for h, w in ((96, 128), (90, 120)):
        low = torch.rand(1, 3, 6, 8, generator=g)
        frames.append((torch.nn.functional.interpolate(low, size=(h, w), mode="bicubic", align_corners=False)[0].clamp(0, 1) * 255)
                      .permute(1, 2, 0).to(torch.uint8).contiguous())
        s = torch.randint(800, 4000, (h, w), generator=g, dtype=torch.int32)
        s[torch.rand(h, w, generator=g) < 0.1] = 0
        sensor.append(s.to(torch.uint16))
    cam = torch.tensor([(100.0, 100.0, 64.0, 48.0), (95.0, 96.0, 60.0, 45.0)], dtype=torch.float64)
    poses = torch.from_numpy(np.stack([K.scene()["poses"][0], K.scene()["poses"][1]]))
    kw = dict(compute_dtype=torch.float32, graph=False, regions={"min_area": 20}, fusion={"min_ring": 10})
    opt = dict(stride=2, edge=0.5)
    plain = InferenceSession(model, **kw)
    sess = InferenceSession(model, cloud=opt, **kw)
    base = plain.predict_frames(frames, size=96, max_size=128, copy=True, sensor_depth=sensor)
    res = sess.predict_frames(frames, size=96, max_size=128, copy=True, sensor_depth=sensor, intrinsics=cam, poses=poses)
    assert sorted(base) == sorted(RESULT_KEYS + ("net_sizes",) + REGION_KEYS + FUSION_KEYS)
    assert sorted(res) == sorted(RESULT_KEYS + ("net_sizes",) + REGION_KEYS + FUSION_KEYS + CLOUD_KEYS)
    for k in base:
        assert base[k].cpu().numpy().tobytes() == res[k].cpu().numpy().tobytes(), k
    dev_frames = [f.cuda() for f in frames]
    again = ops.point_cloud(res["depth_fused"], res["labels"], res["sizes"], cam.cuda(), frames=dev_frames, region_map=res["region_map"],
                            region_count=res["region_count"], planes=res["planes"], source=res["fused_source"], poses=poses.cuda(),
                            min_depth=sess.min_depth, max_depth=sess.max_depth, frame_sizes=[tuple(f.shape[:2]) for f in frames],
                            capacity=res["cloud"].shape[0], **opt)
    host = {k: v.cpu().numpy() for k, v in res.items()}
    for k in CLOUD_KEYS:
        assert again[k].cpu().numpy().tobytes() == host[k].tobytes(), k
    want = C.point_cloud(host["depth_fused"], host["labels"], host["sizes"], cam.numpy(), frames=[f.numpy() for f in frames],
                         region_map=host["region_map"], region_count=host["region_count"], planes=host["planes"], source=host["fused_source"],
                         poses=poses.numpy(), min_depth=sess.min_depth, max_depth=sess.max_depth, capacity_rows=host["cloud"].shape[0], **opt)
    differ, comps = check({k: host[k] for k in CLOUD_KEYS}, want, "session")
    print("session: %d points, %d of %d normal components differ at all" % (int(host["cloud_offsets"][-1]), differ, comps))
    assert host["cloud"].shape[0] == 48 * 64 + 45 * 60 and int(host["cloud_offsets"][-1]) > 0
