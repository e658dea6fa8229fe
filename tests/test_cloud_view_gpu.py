"""GPU: gwd_cloud_view (csrc/view.hip) through ops.cloud_view, cloud.SceneMap.view and InferenceSession(scene_view=) against its
statement (tests/view_ref.py).  The input clouds are made on the host (tests/view_cases.py).

Every comparison is exact - every byte of all four planes: the rule is IEEE fp64 + - * /, ceil and one rounding to float32, correctly
rounded on both sides, and the winner of a pixel is the minimum of unique 64-bit keys.  Every case runs twice into fresh outputs under
torch.cuda.set_sync_debug_mode("error"); the two runs agree in every byte."""
import numpy as np
import pytest
import torch

from gw_depth_amd import cloud as PC
from gw_depth_amd import hip, ops
from tests import cloud_cases as CK
from tests import scene_cases as SK
from tests import scene_ref as S
from tests import view_cases as K
from tests import view_ref as W

pytestmark = pytest.mark.gpu


def run(inp, **more):
    """ops.cloud_view of a dict of view_cases.edge_inputs' shape, twice -> numpy planes; sizes go over as a device tensor, with the
    plane and what the host knows (ext)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    dev = lambda a, dt=None: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dt)
    args = (dev(inp["cloud"]), dev(inp["cloud_offsets"]), dev(inp["intrinsics"]), dev(inp["sizes"], torch.int32))
    kw = dict(poses=dev(inp["poses"]), plane=inp["plane"], view_sizes=inp.get("ext"), **dict(inp["options"], **more))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")               # nothing in these calls waits for the device
    try:
        one, two = ops.cloud_view(*args, **kw), ops.cloud_view(*args, **kw)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    out = {}
    for k in ops.VIEW_KEYS:
        assert one[k].data_ptr() != two[k].data_ptr()
        a, b = one[k].cpu().numpy(), two[k].cpu().numpy()
        assert a.tobytes() == b.tobytes(), "%s differs between two runs" % k
        out[k] = a
    return out


def test_fixture_cloud_from_four_cameras():
    """4702 rows - more than four tiles, no multiple of one - into V = 4 cameras on a plane of 61 x 53, one pixel per row; then a
    total below the rows, and a total of 0."""
    whole, _ = SK.fixture_clouds()
    cams, poses, sizes = K.fixture_cameras()
    total = int(whole[1][-1])
    assert total > 4 * hip.VIEW_TILE and total % hip.VIEW_TILE != 0 and whole[0].shape[0] == total
    inp = dict(cloud=whole[0], cloud_offsets=whole[1], intrinsics=cams, sizes=sizes, poses=poses, plane=CK.PLANE, options=dict(K.DEPTHS))
    K.same(run(inp), K.fixture_whole_view(), "whole")
    part = dict(inp, cloud_offsets=np.array([0, 1500, 3000], dtype=np.int32))
    K.same(run(part, footprint=0.04, max_splat=7), K.statement(part, footprint=0.04, max_splat=7), "a total below the rows")
    none = dict(inp, cloud_offsets=np.array([0, 0], dtype=np.int32))
    out = run(none)
    K.same(out, K.statement(none), "a total of 0")
    assert (out["view_index"] == -1).all() and not out["view_depth"].any() and (out["view_labels"] == 255).all() and not out["view_rgb"].any()


def test_one_camera_and_sixteen():
    inp = K.sixteen_cameras()
    K.same(run(inp), K.statement(inp), "V = 16")
    one = dict(inp, intrinsics=inp["intrinsics"][5:6], sizes=inp["sizes"][5:6], poses=inp["poses"][5:6])
    K.same(run(one), K.statement(one), "V = 1")
    bare = dict(one, poses=None)                          # the cloud taken as the camera's own
    K.same(run(bare, max_depth=100.0), K.statement(bare, max_depth=100.0), "no poses")


def test_a_cloud_of_no_rows():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    res = ops.cloud_view(torch.zeros((0, 32), dtype=torch.uint8, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda"),
                         [K.UNIT_CAM] * 2, [(3, 5), (2, 2)])
    assert res["view_depth"].shape == (2, 3, 5) and not res["view_depth"].any() and (res["view_index"] == -1).all()
    assert (res["view_labels"] == 255).all() and not res["view_rgb"].any()


@pytest.mark.parametrize("name", list(K.EDGES))
def test_arithmetic_edges_by_hand(name):
    case = K.EDGES[name]
    K.same(run(K.edge_inputs(case)), K.edge_expected(case), name)


def test_all_edges_in_one_cloud():
    inp, options = K.all_edges_in_one_cloud()
    assert int(inp["cloud_offsets"][1]) >= 25 and len(options) >= 5
    for opt in options:
        K.same(run(inp, **opt), K.statement(inp, **opt), "edges %r" % (opt,))


@pytest.mark.parametrize("mixed", [False, True])
def test_5003_rows_on_one_pixel(mixed):
    """Same-address 64-bit min: at equal depths row 0 wins, at mixed depths the lowest row of the nearest."""
    inp = K.on_one_pixel(5003, mixed)
    out = run(inp)
    K.same(out, K.statement(inp), "one pixel")
    assert int((out["view_index"] >= 0).sum()) == 1 and (mixed or out["view_index"][0, 1, 2] == 0)


def test_capped_splats_wave_cooperative():
    """300 rows, every one at max_splat = 64 on a plane of 96 x 128, many cut by a border: the path of the whole wave; then one-pixel
    and capped splats in the same waves; then the cap at its other parity with the largest rectangles a lane walks alone."""
    inp = K.splats(300)
    want = K.statement(inp)
    assert int((want["view_index"] >= 0).sum()) == 96 * 128 and len(np.unique(want["view_index"])) >= 10
    K.same(run(inp), want, "capped")
    mix = K.splats(300, near=0.3, far=0.4, seed=12)
    K.same(run(mix), K.statement(mix), "mixed")
    for kw in (dict(max_splat=63), dict(max_splat=4), dict(max_splat=5), dict(footprint=0.0)):      # areas 16 and 25: either side of the split
        K.same(run(mix, **kw), K.statement(mix, **kw), "mixed %r" % (kw,))


@pytest.mark.parametrize("plane", [(1, 1), (3, 70)])
def test_planes_that_are_no_multiple_of_a_vector_store(plane):
    inp = K.splats(40, plane=plane, near=0.2, far=0.3, seed=plane[1], spread=2.0)
    inp["options"].update(footprint=0.02, max_splat=9)
    want = K.statement(inp)
    assert (want["view_index"] >= 0).any()
    K.same(run(inp), want, "plane %r" % (plane,))
    three = dict(inp, intrinsics=np.repeat(inp["intrinsics"], 3, 0), sizes=np.asarray([plane, (1, 1), plane], np.int32))      # 3 planes: an odd total
    K.same(run(three), K.statement(three), "three planes %r" % (plane,))


@pytest.mark.parametrize("voxel", K.VOXELS)
def test_scene_map_view_of_the_fixture_map(voxel):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _, parts = SK.fixture_clouds()
    cams, poses, sizes = K.fixture_cameras()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    m = PC.SceneMap(voxel, SK.FIXTURE_MAX_VOXELS)
    for cloud, offsets in parts:
        m.integrate(dev(cloud), dev(offsets))
    d_cams, d_poses, d_sizes = dev(cams), dev(poses), dev(sizes)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        runs = [m.view(d_cams, d_sizes, poses=d_poses, plane=CK.PLANE, view_sizes=sizes.tolist(), max_splat=K.MAP_SPLAT, **K.DEPTHS) for _ in range(2)]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert tuple(runs[0]) == ops.VIEW_KEYS + PC.SCENE_KEYS
    host = [{k: v.cpu().numpy() for k, v in r.items()} for r in runs]
    for k in host[0]:
        assert host[0][k].tobytes() == host[1][k].tobytes(), k
    # the recorded view is the statement's view of the STATEMENT's map; the device's map agrees with it in positions, labels and colours
    # (tests/test_scene_map_gpu.py), which is all a view reads
    K.same(host[0], K.fixture_map_view(voxel), "map view %s" % voxel)
    ext = K.fixture_map(voxel)
    assert np.array_equal(host[0]["cloud_offsets"], ext["cloud_offsets"]) and np.array_equal(host[0]["voxel_stats"], ext["voxel_stats"])
    assert m.check()["serial"] == 4


def test_session_end_to_end():
    """Two synthetic frames through InferenceSession(cloud, scene, scene_view).predict_frames(intrinsics, poses) twice, the second time
    from cameras moved a little: the first call sees an empty map, the second the statement's view of the first call's extraction; the
    other keys are those of a session without scene_view=."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gw_depth_amd.infer import CLOUD_KEYS, RESULT_KEYS, SCENE_VIEW_KEYS, InferenceSession
    from tests.golden_check import build
    _, model, _ = build(device="cuda")
    g = torch.Generator().manual_seed(4)
    frames = []
    for h, w in ((96, 128), (90, 120)):
        low = torch.rand(1, 3, 6, 8, generator=g)
        frames.append((torch.nn.functional.interpolate(low, size=(h, w), mode="bicubic", align_corners=False)[0].clamp(0, 1) * 255)
                      .permute(1, 2, 0).to(torch.uint8).contiguous())
    cam = torch.tensor([(100.0, 100.0, 64.0, 48.0), (95.0, 96.0, 60.0, 45.0)], dtype=torch.float64)
    poses = torch.from_numpy(CK.scene()["poses"][:2].copy())
    moved = poses.clone()
    moved[:, :, 3] += torch.tensor([0.02, -0.01, 0.03], dtype=torch.float64)
    scene = dict(voxel=0.1, max_voxels=1 << 14, origin=(0.0, 0.0, 0.5))
    sess = InferenceSession(model, compute_dtype=torch.float32, graph=False, cloud=dict(stride=2), scene=scene, scene_view=dict(max_splat=16))
    seen = []
    for p in (poses, moved):
        res = sess.predict_frames(frames, size=96, max_size=128, copy=True, intrinsics=cam, poses=p)
        assert sorted(res) == sorted(RESULT_KEYS + ("net_sizes",) + CLOUD_KEYS + SCENE_VIEW_KEYS)
        seen.append({k: v.cpu().numpy() for k, v in res.items() if k in SCENE_VIEW_KEYS + ("depth",)})
    first, second = seen
    assert (first["scene_index"] == -1).all() and not first["scene_depth"].any() and (first["scene_labels"] == 255).all()
    assert first["scene_cloud_offsets"].tolist() == [0, 0] and first["scene_depth"].shape == first["depth"].shape == (2, 96, 128)
    # the device's own extraction, seen by the statement
    want = W.cloud_view(second["scene_cloud"], second["scene_cloud_offsets"], cam.numpy(), np.asarray([(96, 128), (90, 120)], np.int32),
                        moved.numpy(), 96, 128, min_depth=sess.min_depth, max_depth=sess.max_depth, footprint=0.1, max_splat=16)
    K.same({src: second[k] for k, src in zip(SCENE_VIEW_KEYS, W.KEYS)}, want, "session")
    covered = int((second["scene_index"] >= 0).sum())
    assert covered > 1000 and 0 < int(second["scene_cloud_offsets"][1]) <= sess.scene.check()["count"]
    assert not (second["scene_index"][1, 90:] >= 0).any() and not (second["scene_index"][1, :, 120:] >= 0).any()
    print("session: %d voxels cover %d of %d pixels" % (int(second["scene_cloud_offsets"][1]), covered, 96 * 128 + 90 * 120))
