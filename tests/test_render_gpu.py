"""GPU: gwd_render_frames against its numpy statement (tests/render_ref.py), torch.equal everywhere - the kernel is integer
arithmetic, so there is no tolerance to choose.  The cases are tests/render_cases.py's (their statement canvases are the fixture
tests/golden/render.npz, which tests/test_render.py holds to the statement on the CPU):

  ragged     B = 3 frames of 37 x 53, 64 x 80 and 16 x 16 in one call, P = 3: 3 * 53 and 3 * 80 bytes per row put row starts on all 16
             offsets from a 16-byte boundary (head and tail of the stores); rows through tile corners, wholly outside, zero-length,
             non-finite, out of range, through `order`, count = 0; every layer and colour mode;
  overflow   600 rows through one 48 x 48 frame: more than the tile's list holds;
  many       C = 2048;
  wide       width 16 with end_radius 8."""
import numpy as np
import pytest
import torch

from gw_depth_amd import ops
from tests import render_cases as K
from tests import render_ref as P

pytestmark = pytest.mark.gpu
GOLD = P.load_golden()
CASES = {name: make() for name, make in K.CASES.items()}


def want(name):
    return torch.from_numpy(GOLD["%s.canvas" % name])


def differing(got, ref):
    bad = (got != ref).any(-1)
    return "%d pixels differ, first at (b, p, y, x) = %s" % (int(bad.sum()), bad.nonzero()[:3].tolist())


@pytest.mark.parametrize("views", [False, True], ids=["tensors", "views"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_kernel_equals_the_statement(name, views):
    """Planes as one tensor each, and as per-frame views of another row pitch and offset into buffers filled with 0xAB."""
    got = K.call(CASES[name], "cuda", views=views).cpu()
    ref = want(name)
    assert got.dtype == torch.uint8 and got.shape == ref.shape
    assert torch.equal(got, ref), differing(got, ref)


def row_starts(B, Pn, Fh, Fw):
    return {(((b * Pn + p) * Fh + y) * Fw + x0) * 3 % 16 for b in range(B) for p in range(Pn) for y in range(Fh) for x0 in range(0, Fw, P.TILE_W)}


def test_row_starts_fall_on_every_alignment():
    """The three ragged frames share a canvas 80 wide, 240 = 15 * 16 bytes per row: every one of its rows starts on a 16-byte boundary
    and only the body of the stores runs.  Head and tail run where the canvas is 53 wide (frame 0 alone, below) and 133 wide (the
    larger canvas, below): 159 and 399 bytes per row walk through all 16 offsets."""
    assert row_starts(*want("ragged").shape[:4]) == {0}
    assert row_starts(1, 3, 37, 53) == set(range(16)) and row_starts(3, 3, 70, 133) == set(range(16))


def test_every_byte_is_written_and_two_calls_agree():
    """A canvas pre-filled with 0xAB comes out as the statement's, 0 outside the frames: the launch writes every byte, there is no
    memset to rely on.  A second call into a fresh tensor gives the same bytes."""
    case = CASES["ragged"]
    ref = want("ragged")
    canvas = torch.full(tuple(ref.shape), 0xAB, dtype=torch.uint8, device="cuda")
    assert K.call(case, "cuda", out=canvas) is canvas
    first = canvas.cpu()
    beyond = 0
    for b, (fh, fw) in enumerate(case["sizes"]):
        outside = torch.ones(ref.shape[2:4], dtype=torch.bool)
        outside[:fh, :fw] = False
        beyond += int(outside.sum())
        assert not first[b][:, outside].any()
    assert beyond > 7000                                                              # 37 x 53 and 16 x 16 in a 64 x 80 canvas
    again = K.call(case, "cuda")
    assert again.data_ptr() != canvas.data_ptr()
    assert torch.equal(first, ref) and torch.equal(again.cpu(), ref)                  # bit-identical from call to call


def test_larger_canvas_is_zero_outside_and_unchanged_inside():
    case = CASES["ragged"]
    filled = torch.full((3, 3, 70, 133, 3), 0xAB, dtype=torch.uint8, device="cuda")
    got = K.call(case, "cuda", canvas_size=(70, 133), out=filled).cpu()                           # a third tile column, a ragged last tile row
    ref = want("ragged")
    assert torch.equal(got[:, :, :64, :80], ref) and not got[:, :, 64:].any() and not got[:, :, :, 80:].any()


def test_a_frames_panels_depend_on_neither_its_slot_nor_its_neighbours():
    """Frame 1 of the ragged case alone, and as the last of three with other neighbours, draws the same pixels."""
    case = CASES["ragged"]
    ref = want("ragged")
    pick = lambda v, idx: None if v is None else (np.ascontiguousarray(v[idx]) if isinstance(v, np.ndarray) else [v[i] for i in idx])

    def sub(idx):
        idx = list(idx)
        return dict(case, sizes=pick(case["sizes"], idx), frames=pick(case["frames"], idx), planes=[pick(v, idx) for v in case["planes"]],
                    label_planes=[pick(v, idx) for v in case["label_planes"]], region_map=pick(case["region_map"], idx),
                    lines=pick(case["lines"], idx), count=pick(case["count"], idx), order=pick(case["order"], idx),
                    scores=pick(case["scores"], idx), kinds=pick(case["kinds"], idx))

    alone = K.call(sub([1]), "cuda").cpu()
    assert torch.equal(alone[0], ref[1])
    narrow = K.call(sub([0]), "cuda", canvas_size=(37, 53)).cpu()                                            # its own canvas, 37 x 53: rows start on every alignment
    assert tuple(narrow.shape) == (1, 3, 37, 53, 3) and torch.equal(narrow[0], ref[0, :, :37, :53]), differing(narrow[0], ref[0, :, :37, :53])
    moved = K.call(sub([2, 0, 1]), "cuda").cpu()
    assert torch.equal(moved[2], ref[1]) and torch.equal(moved[0], ref[2]) and torch.equal(moved[1], ref[0])


def test_session_renders_what_render_frames_gives_on_its_outputs():
    """predict_frames(render=True) over the tiny model of the GPU session tests: canvas equals ops.render_frames on the call's own
    outputs and the statement on their host copies; without render= the result dict is what it was."""
    from gw_depth_amd.infer import NMS_KEYS, REGION_KEYS, RENDER_KEYS, RESULT_KEYS, InferenceSession
    from tests.golden_check import build
    _, model, _ = build(device="cuda")
    g = torch.Generator().manual_seed(4)
    frames = []
    for h, w in ((96, 128), (90, 120)):
        low = torch.rand(1, 3, 6, 8, generator=g)
        frames.append((torch.nn.functional.interpolate(low, size=(h, w), mode="bicubic", align_corners=False)[0].clamp(0, 1) * 255)
                      .permute(1, 2, 0).to(torch.uint8).contiguous())
    kw = dict(compute_dtype=torch.float32, graph=False, regions={"min_area": 20}, line_nms=0.01, score_thresh=0.0)
    base = InferenceSession(model, **kw).predict_frames(frames, size=96, max_size=128, copy=True)
    res = InferenceSession(model, render={"score_range": (0.0, 1.0)}, **kw).predict_frames(frames, size=96, max_size=128, copy=True)
    assert sorted(base) == sorted(RESULT_KEYS + ("net_sizes",) + REGION_KEYS + NMS_KEYS) and sorted(res) == sorted(tuple(base) + RENDER_KEYS)
    for k in base:
        assert base[k].cpu().numpy().tobytes() == res[k].cpu().numpy().tobytes(), k
    panels = [{"base": "frame", "tint": 0, "outlines": True, "lines": "score"}, ("depth", 0), ("labels", 0)]
    on_dev = [f.cuda() for f in frames]
    direct = ops.render_frames(res["sizes"], panels, frames=on_dev, planes=res["depth_mm"], label_planes=res["labels"], region_map=res["region_map"],
                               lines=res["nms_lines"], count=res["nms_count"], scores=res["nms_scores"], score_range=(0.0, 1.0))
    assert tuple(res["canvas"].shape) == (2, 3, 96, 128, 3) and torch.equal(res["canvas"], direct)
    host = {k: v.cpu().numpy() for k, v in res.items()}
    case = dict(sizes=host["sizes"], panels=panels, frames=[f.numpy() for f in frames], planes=[host["depth_mm"]], label_planes=[host["labels"]],
                region_map=host["region_map"], lines=host["nms_lines"], count=host["nms_count"], order=None, scores=host["nms_scores"], kinds=None,
                options={"score_range": (0.0, 1.0)})
    ref = torch.from_numpy(K.statement(case))
    assert torch.equal(res["canvas"].cpu(), ref), differing(res["canvas"].cpu(), ref)
    assert int(host["nms_count"].min()) > 0 and (ref[:, 0, :90, :120] != torch.stack([f[:90, :120] for f in frames])).any()      # lines were drawn
