"""GPU: gwd_scene_reset / gwd_scene_integrate / gwd_scene_extract (csrc/scene.hip) through cloud.SceneMap against their statement
(tests/scene_ref.py).  The input clouds are made on the host (tests/cloud_ref.py, tests/scene_cases.py): nothing here leans on
gwd_point_cloud but the session test.

cloud_offsets, voxel_stats, the zero tails, every uint8 field, the flags and x y z are compared exactly: the accumulators are integers,
a position is a handful of fp64 + * / in a fixed order, correctly rounded on both sides, then one rounding to float32.  Every component
of a normal stays within 2^-23 of the statement's - one float32 unit at magnitude <= 1: an fp64 sqrt or divide that differs in its
last place may push a component across one float32 rounding boundary, nothing more (the bound of tests/test_point_cloud_gpu.py) - and
whether a normal is zero is exact.  Every sequence of calls is made twice, on two fresh maps, under
torch.cuda.set_sync_debug_mode("error"); the two results agree in every byte."""
import numpy as np
import pytest
import torch

from gw_depth_amd import cloud as PC
from gw_depth_amd import hip
from tests import cloud_ref as C
from tests import scene_cases as K
from tests import scene_ref as S

pytestmark = pytest.mark.gpu

NORMAL_BOUND = 2.0 ** -23
KEYS = PC.SCENE_KEYS


def device_pairs(clouds):
    return [tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in pair) for pair in clouds]


def run(clouds, voxel, max_voxels, origin=K.ORIGIN, slots=None, options=({},), then=None):
    """Twice: a fresh map, the clouds integrated in order, one extraction per entry of `options` -> (list of numpy dicts, state,
    map); the two runs agree in every byte.  then(map): more calls on the second map, still with no sync allowed."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    pairs = device_pairs(clouds)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")               # nothing in these calls waits for the device
    try:
        runs = []
        for _ in range(2):
            m = PC.SceneMap(voxel, max_voxels, origin=origin, slots=slots)
            for cloud, offsets in pairs:
                m.integrate(cloud, offsets)
            runs.append([m.extract(**opt) for opt in options])
        extra = then(m) if then is not None else None
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    out = []
    for one, two in zip(*runs):
        host = {}
        for k in KEYS:
            a, b = one[k].cpu().numpy(), two[k].cpu().numpy()
            assert a.tobytes() == b.tobytes(), "%s differs between two runs" % k
            host[k] = a
        out.append(host)
    return out, m.state(), m, extra


def check(out, want, what=""):
    """Exact but for the normals, which stay within NORMAL_BOUND per component -> (components that differ at all, components)."""
    assert np.array_equal(out["cloud_offsets"], want["cloud_offsets"]), (what, out["cloud_offsets"], want["cloud_offsets"])
    assert out["cloud"].shape == want["cloud"].shape and out["voxel_stats"].shape == want["voxel_stats"].shape, what
    kept = int(want["cloud_offsets"][1])
    assert not out["cloud"][kept:].any() and not out["voxel_stats"][kept:].any(), "%s: a tail is not zero" % what
    assert np.array_equal(out["voxel_stats"], want["voxel_stats"]), (what, "voxel_stats", np.argwhere(out["voxel_stats"] != want["voxel_stats"])[:5].tolist())
    got, ref = out["cloud"].view(C.RECORD).ravel()[:kept], want["cloud"].view(C.RECORD).ravel()[:kept]
    for f in ("rgb", "label", "region", "source", "frame", "flags"):
        assert np.array_equal(got[f], ref[f]), (what, f, np.argwhere(got[f] != ref[f])[:5].tolist())
    assert got["xyz"].tobytes() == ref["xyz"].tobytes(), (what, "xyz", np.argwhere(got["xyz"].view(np.uint32) != ref["xyz"].view(np.uint32))[:5].tolist())
    assert np.array_equal(got["normal"] == 0, ref["normal"] == 0), (what, "a normal's zeros")
    err = np.abs(got["normal"].astype(np.float64) - ref["normal"].astype(np.float64))
    assert kept == 0 or err.max() <= NORMAL_BOUND, (what, "normal", float(err.max()))
    return int((got["normal"].view(np.uint32) != ref["normal"].view(np.uint32)).sum()), 3 * kept


def padded(gold, gid, max_voxels):
    """A recorded extraction with its zero tail back."""
    kept = gold[gid + ".cloud"].shape[0]
    cloud, stats = np.zeros((max_voxels, 32), np.uint8), np.zeros((max_voxels, 4), np.int32)
    cloud[:kept], stats[:kept] = gold[gid + ".cloud"], gold[gid + ".voxel_stats"]
    return {"cloud": cloud, "cloud_offsets": np.array([0, kept], np.int32), "voxel_stats": stats}


@pytest.mark.parametrize("voxel", K.VOXELS)
def test_fixture(voxel):
    """tests/golden/scene_map.npz - the statement's maps of the point-cloud fixture (four clouds, the last over the voxels of the
    first) - in one call and in four."""
    whole, parts = K.fixture_clouds()
    total = int(whole[1][-1])
    assert total > 2 * hip.SCENE_TILE and total % hip.SCENE_TILE != 0                # a changed tile size cannot empty the case
    assert all(int(o[-1]) % hip.SCENE_TILE for _, o in parts)
    gold = K.load_golden()
    for split in (False, True):
        (out,), state, _, _ = run(parts if split else [whole], voxel, K.FIXTURE_MAX_VOXELS)
        want = padded(gold, K.golden_id(voxel, split), K.FIXTURE_MAX_VOXELS)
        differ, comps = check(out, want, K.golden_id(voxel, split))
        assert state == dict(serial=4 if split else 1, count=int(want["cloud_offsets"][1]), points=total, dropped=0, status=0)
        print("%s: %d voxels, %d of %d normal components differ from the statement's at all (bound 2^-23 each)"
              % (K.golden_id(voxel, split), state["count"], differ, comps))


def test_nearly_full_table_and_overflow():
    """63 voxels in a table of 64 slots: long probe chains that wrap around, whatever the hash.  A 64th voxel: status 1, an empty
    extraction - and the call returns."""
    rec = K.distinct_voxels(64)
    first, last = K.as_cloud(rec[:63], capacity=70), K.as_cloud(rec[63:])
    (out,), state, _, _ = run([first, first], 0.1, 63, slots=64)
    check(out, S.merge([first, first], 0.1, 63), "63 of 64")
    assert state == dict(serial=2, count=63, points=126, dropped=0, status=0) and int(out["cloud_offsets"][1]) == 63
    (out,), state, m, _ = run([first, last, first], 0.1, 63, slots=64)
    assert state == dict(serial=3, count=63, points=63, dropped=0, status=1)
    assert not out["cloud"].any() and not out["voxel_stats"].any() and out["cloud_offsets"].tolist() == [0, 0]
    with pytest.raises(RuntimeError, match="max_voxels = 63"):
        m.check()
    # more voxels in ONE call than the table has slots: every probe ends, status 1
    (out,), state, _, _ = run([K.as_cloud(K.distinct_voxels(300, seed=4))], 0.1, 63, slots=64)
    assert state["status"] == 1 and state["count"] == 0 and state["serial"] == 1 and out["cloud_offsets"].tolist() == [0, 0]
    # reset() opens the map again
    m.reset().integrate(*device_pairs([first])[0])
    assert m.state() == dict(serial=1, count=63, points=63, dropped=0, status=0)


@pytest.mark.parametrize("cells", [1, 2])
def test_contention(cells):
    """About 5000 rows into one voxel, and into two neighbours: same-address atomics against exact sums."""
    cloud = K.as_cloud(K.contended(5003, cells), capacity=5100)
    (out,), state, _, _ = run([cloud], 0.25, 16)
    want = S.merge([cloud], 0.25, 16)
    check(out, want, "%d cells" % cells)
    assert int(out["cloud_offsets"][1]) == cells and out["voxel_stats"][:cells, 0].sum() == 5003 and state["points"] == 5003


def test_scan_thread_owns_two_tiles():
    """More tiles than a scan workgroup has threads, in the cloud's rows (the integrate scan) and in max_voxels (the extract scan):
    a scan thread owns two tiles.  5003 voxels are born in the first tiles, every later tile counts zero, and the second call has no
    births at all."""
    rows = max_voxels = 1024 * 1024 + 4097
    tiles = -(-rows // hip.SCENE_TILE)
    assert tiles > 1024                                   # a changed tile size cannot empty the case
    cloud = K.as_cloud(K.distinct_voxels(5003), capacity=rows)
    options = ({}, dict(min_obs=2))
    ref = S.SceneMap(0.1, max_voxels).integrate(*cloud).integrate(*cloud)
    outs, state, _, _ = run([cloud, cloud], 0.1, max_voxels, options=options)
    for out, opt in zip(outs, options):
        check(out, ref.extract(**opt), "1029 tiles %r" % (opt,))
    assert int(outs[0]["cloud_offsets"][1]) == int(outs[1]["cloud_offsets"][1]) == 5003
    assert state == ref.state() == dict(serial=2, count=5003, points=10006, dropped=0, status=0)


@pytest.mark.parametrize("name", list(K.EDGES))
def test_arithmetic_edges_by_hand(name):
    case = K.EDGES[name]
    (out,), state, _, _ = run([K.edge_cloud(case)], case["voxel"], K.EDGE_MAX_VOXELS, origin=case.get("origin", K.ORIGIN),
                              options=(case.get("options", {}),))
    check(out, K.edge_expected(case), name)
    assert (state["points"], state["dropped"], state["status"], state["serial"]) == (len(case["points"]) - case.get("dropped", 0), case.get("dropped", 0), 0, 1)


def test_all_edges_in_one_cloud():
    cloud = K.all_edges_in_one_cloud()
    assert int(cloud[1][1]) >= 20
    ref = S.SceneMap(0.5, 64).integrate(*cloud)
    options = ({}, dict(min_obs=2), dict(keep="glass"), dict(keep="non_glass"))
    outs, state, _, _ = run([cloud], 0.5, 64, options=options)
    for out, opt in zip(outs, options):
        check(out, ref.extract(**opt), "edges %r" % (opt,))
    assert state == ref.state() and state["dropped"] == 5


def test_reset_extract_twice_and_filters():
    """reset() and the same input: the bytes of a fresh map; extract twice with no integrate in between: the same bytes; min_obs and
    keep against the statement."""
    _, parts = K.fixture_clouds()
    ref = S.SceneMap(0.25, 300, (0.1, -0.2, 0.3))
    for part in parts:
        ref.integrate(*part)
    options = ({}, {}, dict(min_obs=2), dict(min_obs=40, keep="glass"), dict(keep="non_glass"))
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    junk, on_device = device_pairs([K.as_cloud(K.distinct_voxels(64))])[0], device_pairs(parts)

    def then(m):                                          # on the second map: junk, reset, the same input again
        m.integrate(*junk)
        m.reset()
        for pair in on_device:
            m.integrate(*pair)
        return m.extract()

    outs, state, _, again = run(parts, 0.25, 300, origin=(0.1, -0.2, 0.3), options=options, then=then)
    for out, opt in zip(outs, options):
        check(out, ref.extract(**opt), "filters %r" % (opt,))
    assert 0 < int(outs[3]["cloud_offsets"][1]) < int(outs[2]["cloud_offsets"][1]) < int(outs[0]["cloud_offsets"][1])
    for k in KEYS:
        assert outs[0][k].tobytes() == outs[1][k].tobytes(), k
        assert again[k].cpu().numpy().tobytes() == outs[0][k].tobytes(), k
    assert state == ref.state()


def test_session_end_to_end():
    """Two synthetic frames through InferenceSession(cloud, scene).predict_frames(intrinsics, poses), twice, the second time from
    cameras moved a little: the map equals the statement applied to the two returned clouds; the returned keys are those of a
    session without scene=."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gw_depth_amd.infer import CLOUD_KEYS, RESULT_KEYS, InferenceSession
    from tests import cloud_cases
    from tests.golden_check import build
    _, model, _ = build(device="cuda")
    g = torch.Generator().manual_seed(4)
    frames = []
    for h, w in ((96, 128), (90, 120)):
        low = torch.rand(1, 3, 6, 8, generator=g)
        frames.append((torch.nn.functional.interpolate(low, size=(h, w), mode="bicubic", align_corners=False)[0].clamp(0, 1) * 255)
                      .permute(1, 2, 0).to(torch.uint8).contiguous())
    cam = torch.tensor([(100.0, 100.0, 64.0, 48.0), (95.0, 96.0, 60.0, 45.0)], dtype=torch.float64)
    poses = torch.from_numpy(cloud_cases.scene()["poses"][:2].copy())
    moved = poses.clone()
    moved[:, :, 3] += torch.tensor([0.02, -0.01, 0.03], dtype=torch.float64)
    scene = dict(voxel=0.1, max_voxels=1 << 14, origin=(0.0, 0.0, 0.5))
    sess = InferenceSession(model, compute_dtype=torch.float32, graph=False, cloud=dict(stride=2), scene=scene)
    ref = S.SceneMap(**scene)
    for p in (poses, moved):
        res = sess.predict_frames(frames, size=96, max_size=128, copy=True, intrinsics=cam, poses=p)
        assert sorted(res) == sorted(RESULT_KEYS + ("net_sizes",) + CLOUD_KEYS)
        ref.integrate(res["cloud"].cpu().numpy(), res["cloud_offsets"].cpu().numpy())
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        one, two = sess.scene.extract(), sess.scene.extract(min_obs=2)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    differ, comps = check({k: v.cpu().numpy() for k, v in one.items()}, ref.extract(), "session")
    check({k: v.cpu().numpy() for k, v in two.items()}, ref.extract(min_obs=2), "session, min_obs 2")
    state = sess.scene.check()
    assert state == ref.state() and state["serial"] == 2 and 0 < state["count"] < state["points"]
    assert (one["voxel_stats"][:state["count"], 3] > one["voxel_stats"][:state["count"], 2]).any()      # voxels seen by both calls
    print("session: %d points in %d voxels, %d of %d normal components differ at all" % (state["points"], state["count"], differ, comps))
