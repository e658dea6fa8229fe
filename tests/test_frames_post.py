"""CPU: the fp64 restatement of gwd_dense_postprocess_resized (tests/frames_ref.py) against F.interpolate and the plain
post-processing, the inputs of the GPU kernel test (how many labels their margins leave undecided), and the host logic of
InferenceSession.predict_frames over a stand-in library: launch and upload counts, limits, keys, shapes, sizes."""
import pytest
import torch
import torch.nn.functional as F

from gw_depth_amd import data, hip
from gw_depth_amd.infer import RESULT_KEYS, InferenceSession
from tests import frames_ref as R
from tests.fake_device import FakeDevice

PAIRS = [((12, 20), (31, 47)), ((12, 20), (7, 11)), ((18, 32), (720, 1280)), ((9, 13), (17, 40)), ((12, 20), (20, 11)), ((12, 20), (5, 30)),
         ((12, 20), (12, 20)), ((1, 1), (3, 5)), ((5, 1), (2, 4))]


@pytest.mark.parametrize("src,dst", PAIRS, ids=["%dx%d-%dx%d" % (s + d) for s, d in PAIRS])
def test_restatement_equals_interpolate(src, dst):
    x = torch.randn(2, 3, *src, dtype=torch.float64, generator=torch.Generator().manual_seed(src[0] * 100 + dst[1]))
    want = F.interpolate(x, size=dst, mode="bilinear", align_corners=False)
    got = R.resize(x, *dst)
    assert got.shape == want.shape and float((got - want).abs().max()) <= 1e-12


def test_zero_weight_taps_stay_out():
    x = torch.tensor([[1.0, float("nan")], [float("inf"), 4.0]], dtype=torch.float64)
    assert torch.equal(R.resize(x, 2, 2).isnan(), x.isnan()) and float(R.resize(x, 2, 2)[0, 0]) == 1.0     # identity: every lambda is 0
    up = R.resize(x, 4, 4)
    assert float(up[0, 0]) == 1.0 and bool(up[0, 1].isnan())          # the corner is its pixel alone, the next one blends the NaN in


def test_twin_of_a_ragged_image_mirrors_inside_w():
    """The twin holds the image mirrored inside its un-padded width w (the rest of the row is padding): the ensemble of an image
    and its own mirror image is the image."""
    depth, seg, sizes, frames, out_hw = R.inputs(5, "up_vec", twin=False)
    B, H, W = depth.shape
    twin_d, twin_s = depth.clone(), seg.clone()
    for b, (h, w) in enumerate(sizes):
        twin_d[b, :h, :w] = depth[b, :h, :w].flip(-1)
        twin_s[b, :, :h, :w] = seg[b, :, :h, :w].flip(-1)
    assert sizes[1][1] < W and not torch.equal(twin_d[1, :9, :13], depth[1, :9].flip(-1)[:, :13])      # not the mirror inside W
    one = R.dense_resized(depth, seg, sizes, frames, out_hw, R.MIN_D, R.MAX_D)
    two = R.dense_resized(torch.cat([depth, twin_d]), torch.cat([seg, twin_s]), sizes, frames, out_hw, R.MIN_D, R.MAX_D, twin=B)
    assert torch.equal(one[0], two[0]) and torch.equal(one[1], two[1]) and torch.equal(one[2], two[2])
    assert torch.equal(two[3], 2 * one[3])                                                             # the logits are summed
    assert bool(torch.isfinite(one[0]).all()) and int(one[2][1, :17, :40].max()) <= 1                  # no padding was read


@pytest.mark.parametrize("shape", ["up_vec", "src16_vec"])
def test_identity_equals_the_plain_postprocessing(shape):
    depth, seg, sizes, _, _ = R.inputs(6, shape, twin=False)
    depth[:, 2, 3], depth[:, 4, 5], depth[:, 6, 7] = float("nan"), float("inf"), float("-inf")
    seg[:, 0, 1, 1], seg[:, 1, 1, 2], seg[:, :, 1, 3], seg[:, :, 3, 4] = float("nan"), float("nan"), float("nan"), 0.5
    B, H, W = depth.shape
    got = R.dense_resized(depth, seg, sizes, sizes, (H, W), R.MIN_D, R.MAX_D)
    want = R.dense_plain(depth, seg, sizes, R.MIN_D, R.MAX_D)
    assert all(torch.equal(a, b) for a, b in zip(got[:3], want))
    assert float(got[0][0, 2, 3]) == R.MIN_D and float(got[0][0, 4, 5]) == R.MAX_D and float(got[0][0, 6, 7]) == R.MIN_D
    assert [int(v) for v in got[2][0, 1, 1:4]] == [0, 1, 0] and int(got[2][0, 3, 4]) == 0


@pytest.mark.parametrize("twin", [False, True], ids=["single", "twin"])
@pytest.mark.parametrize("shape", sorted(R.SHAPES))
@pytest.mark.parametrize("seed", R.SEEDS)
def test_margins_decide_the_labels_of_the_kernel_test(seed, shape, twin):
    depth, seg, sizes, frames, out_hw = R.inputs(seed, shape, twin)
    _, _, label, margin = R.dense_resized(depth, seg, sizes, frames, out_hw, R.MIN_D, R.MAX_D, twin=len(sizes) if twin else 0)
    tol = R.label_tolerance(seg, sizes, twin)
    inside = label != 255
    close = int(((margin <= tol) & inside).sum())
    print("seed %d %s %s: %d of %d pixels within %.2e" % (seed, shape, "twin" if twin else "single", close, int(inside.sum()), tol))
    assert int(inside.sum()) == sum(fh * fw for fh, fw in frames) and close <= 0.01 * int(inside.sum())


# ---------------------------------------------------------------------------------------------------- predict_frames, host logic
BUDGET = {"resample_u8_pass_batch": 2, "gather2d_batch": 1, "collate": 1, "dense_postprocess_resized": 1, "dense_postprocess": 1,
          "line_postprocess": 1, "upload_tables": 1}


class FramesFakeDevice(FakeDevice):
    """The stand-in with the grouped augmentation entry points as loops over its single calls, the three post-processing entry
    points from their restatements, and a count of every call."""

    def __init__(self):
        self.calls = {k: 0 for k in BUDGET}
        self.twin = None

    def resample_u8_pass_batch(self, jobs, axis, C, tables):
        self.calls["resample_u8_pass_batch"] += 1
        assert 0 < len(jobs) <= hip.AUGMENT_BATCH
        for src, dst, row_stride, bounds_off, kk_off, ksize, base0, step0, base1, step1 in jobs:
            n_out = dst.shape[1] if axis == 1 else dst.shape[0]
            bounds = tables[bounds_off:bounds_off + 2 * n_out].view(n_out, 2)
            kk = tables[kk_off:kk_off + n_out * ksize].view(n_out, ksize)
            self.resample_u8_pass(src, dst, bounds, kk, axis, row_stride, base0, step0, base1, step1)

    def gather2d_batch(self, jobs, tables):
        self.calls["gather2d_batch"] += 1
        assert 0 < len(jobs) <= hip.GATHER_BATCH
        for src, dst, row_stride_bytes, ytab_off, xtab_off, oh, ow, elem_bytes in jobs:
            self.gather2d(src, dst, tables[ytab_off:ytab_off + oh], tables[xtab_off:xtab_off + ow], row_stride_bytes, elem_bytes)

    def collate(self, samples, H, W, mean, std, images, mask, depth, seg):
        self.calls["collate"] += 1
        assert depth is None and seg is None                            # frames alone: the stand-in's collate wants both
        B = len(samples)
        super().collate(samples, H, W, mean, std, images, mask, torch.empty(B, H, W), torch.empty(B, H, W, dtype=torch.int64))

    def dense_postprocess(self, depth, seg, seg_strides, sizes, depth_out, depth_mm, label, B, H, W, dmin, dmax):
        self.calls["dense_postprocess"] += 1
        d, mm, lab = R.dense_plain(depth, seg, None if sizes is None else sizes.tolist(), dmin, dmax)
        depth_out.copy_(d)
        label.copy_(lab)
        if depth_mm is not None:
            depth_mm.copy_(mm)

    def dense_postprocess_resized(self, depth, seg, seg_strides, sizes, frame_sizes, twin, depth_out, depth_mm, label, B, H, W, Fh, Fw,
                                  dmin, dmax):
        self.calls["dense_postprocess_resized"] += 1
        self.twin = twin
        d, mm, lab, _ = R.dense_resized(depth, seg, None if sizes is None else sizes.tolist(), frame_sizes.tolist(), (Fh, Fw), dmin, dmax, twin)
        depth_out.copy_(d)
        label.copy_(lab)
        if depth_mm is not None:
            depth_mm.copy_(mm)

    def line_postprocess(self, logits, lines, sizes, scores, lines_px, order, count, B, Q, ld, thresh):
        self.calls["line_postprocess"] += 1
        s = torch.softmax(logits, -1)[..., 0]
        scores.copy_(s)
        h, w = sizes[:, 0].float(), sizes[:, 1].float()
        lines_px.copy_(lines[..., :4] * torch.stack([w, h, w, h], 1)[:, None, :])
        order.copy_(torch.argsort(s, dim=-1, descending=True, stable=True))
        count.copy_((s > thresh).sum(-1))


class TinyModel(torch.nn.Module):
    """What a session needs of a model: parameters, compute_dtype, and the output dict of a forward."""
    Q = 5

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.tensor([0.3, -0.2, 0.4]))
        self.compute_dtype = torch.float32

    def forward(self, samples, taps=None):
        x = samples.tensors.float()
        B = x.shape[0]
        d = (x * self.w.view(1, 3, 1, 1)).sum(1, keepdim=True) + 2.0
        q = torch.linspace(0.1, 0.9, self.Q * 4).view(1, self.Q, 4).expand(B, -1, -1)
        return {"pred_depth": [d * 0.5, d], "pred_seg": x[:, :2] - x[:, 1:], "pred_lines": q.contiguous(),
                "pred_logits": torch.stack([q[..., 0], q[..., 1].flip(1)], -1).contiguous()}


@pytest.fixture
def fake(monkeypatch):
    lib = FramesFakeDevice()
    upload = data.upload_tables

    def counted(host, device):
        lib.calls["upload_tables"] += 1
        assert host.dtype == torch.int32 and host.dim() == 1
        return upload(host, device)

    monkeypatch.setattr(data, "upload_tables", counted)
    hip.set_library(lib)
    yield lib
    hip.set_library(None)


def frames_of(n, seed=0, same=False):
    g = torch.Generator().manual_seed(seed)
    shapes = [(72, 128), (60, 45), (50, 100), (96, 54), (40, 110), (64, 64), (110, 41), (48, 96)]
    return [torch.randint(0, 256, (*(shapes[0] if same else shapes[i % len(shapes)]), 3), dtype=torch.uint8, generator=g) for i in range(n)]


@pytest.mark.parametrize("ensemble", [False, True], ids=["plain", "ensemble"])
@pytest.mark.parametrize("B", [1, 3, 8])
def test_predict_frames_launches_keys_shapes_sizes(fake, B, ensemble):
    sess = InferenceSession(TinyModel(), compute_dtype=torch.float32, graph=False)
    frames = frames_of(B)
    res = sess.predict_frames(frames, size=48, max_size=64, ensemble=ensemble)
    # one size-changing resize: two grouped resample launches, no gather (every frame is resized), one collate, one resized
    # post-processing, one table upload - whatever B is; the forward's own post-processing is predict()'s
    assert fake.calls == dict(BUDGET, gather2d_batch=0), fake.calls
    assert fake.twin == (B if ensemble else 0)
    assert sorted(res) == sorted(RESULT_KEYS + ("net_sizes",))
    fs = [tuple(f.shape[:2]) for f in frames]
    Fh, Fw = max(s[0] for s in fs), max(s[1] for s in fs)
    assert res["depth"].shape == (B, Fh, Fw) and res["depth"].dtype == torch.float32
    assert res["depth_mm"].shape == (B, Fh, Fw) and res["depth_mm"].dtype == torch.uint16
    assert res["labels"].shape == (B, Fh, Fw) and res["labels"].dtype == torch.uint8
    Q = TinyModel.Q
    assert res["scores"].shape == (B, Q) and res["lines"].shape == (B, Q, 4) and res["order"].shape == (B, Q) and res["count"].shape == (B,)
    assert res["sizes"].dtype == torch.int32 and res["sizes"].tolist() == [list(s) for s in fs]
    assert res["net_sizes"].dtype == torch.int32
    assert res["net_sizes"].tolist() == [list(data.resized_shape(w, h, 48, 64)) for h, w in fs]
    for b, (h, w) in enumerate(fs):
        lab = res["labels"][b]
        assert int(lab[:h, :w].max()) <= 1 and bool((lab[h:] == 255).all()) and bool((lab[:, w:] == 255).all())
        assert float(res["depth"][b, :h, :w].min()) >= sess.min_depth and bool((res["depth"][b, h:] == 0).all())
    # the lines are in frame pixels
    q = torch.linspace(0.1, 0.9, Q * 4).view(Q, 4)
    for b, (h, w) in enumerate(fs):
        assert torch.allclose(res["lines"][b], q * torch.tensor([w, h, w, h], dtype=torch.float32))


def test_predict_frames_gathers_only_frames_that_need_no_resize(fake):
    sess = InferenceSession(TinyModel(), compute_dtype=torch.float32, graph=False)
    frames = [torch.randint(0, 256, (48, 64, 3), dtype=torch.uint8), torch.randint(0, 256, (60, 90, 3), dtype=torch.uint8)]
    assert data.resized_shape(64, 48, 48, 64) == (48, 64)                  # frame 0 is at network size already
    res = sess.predict_frames(frames, size=48, max_size=64)
    assert fake.calls["gather2d_batch"] == 0 and fake.calls["resample_u8_pass_batch"] == 2        # used where it is
    assert res["net_sizes"].tolist()[0] == [48, 64]
    for k in fake.calls:
        fake.calls[k] = 0
    sess.predict_frames(frames, size=48, max_size=64, ensemble=True)       # its mirror image has no resize to ride in: one gather
    assert fake.calls == BUDGET, fake.calls


def test_predict_frames_ensemble_of_a_mirror_symmetric_model_changes_nothing(fake):
    """TinyModel is pointwise, so the prediction of the mirrored frame is the mirrored prediction up to the resize's rounding
    of the mirrored read: the ensemble moves the depth by no more than that."""
    sess = InferenceSession(TinyModel(), compute_dtype=torch.float32, graph=False)
    frames = frames_of(2, seed=3)
    one = sess.predict_frames(frames, size=48, max_size=64)
    two = sess.predict_frames(frames, size=48, max_size=64, ensemble=True)
    assert torch.equal(one["sizes"], two["sizes"]) and torch.equal(one["net_sizes"], two["net_sizes"])
    assert torch.allclose(one["lines"], two["lines"])
    step = 0.9 / 255 / min(data.STD)                                         # one uint8 step in every channel, through Normalize and sum |w| = 0.9
    assert float((one["depth"] - two["depth"]).abs().max()) <= step


def test_predict_frames_limits(fake):
    sess = InferenceSession(TinyModel(), compute_dtype=torch.float32, graph=False)
    small = lambda n: [torch.zeros((8, 8, 3), dtype=torch.uint8)] * n
    with pytest.raises(ValueError):
        sess.predict_frames([])
    with pytest.raises(ValueError):
        sess.predict_frames(small(hip.AUGMENT_BATCH + 1), size=8, max_size=8)
    with pytest.raises(ValueError):
        sess.predict_frames(small(hip.AUGMENT_BATCH // 2 + 1), size=8, max_size=8, ensemble=True)
    with pytest.raises(ValueError):
        sess.predict_frames([torch.zeros((8, 8, 3))], size=8, max_size=8)                       # not uint8
    with pytest.raises(ValueError):
        sess.predict_frames([torch.zeros((3, 8, 8), dtype=torch.uint8)], size=8, max_size=8)     # not (h, w, 3)
    with pytest.raises(ValueError):
        sess.predict_frames([torch.zeros((2, 16386, 3), dtype=torch.uint8)], size=2, max_size=None)
    assert sum(fake.calls.values()) == 0
    assert sess.predict_frames(small(hip.AUGMENT_BATCH), size=8, max_size=8)["depth"].shape == (hip.AUGMENT_BATCH, 8, 8)
    assert sess.predict_frames(small(hip.AUGMENT_BATCH // 2), size=8, max_size=8, ensemble=True)["depth"].shape[0] == hip.AUGMENT_BATCH // 2
