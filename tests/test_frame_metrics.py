"""Frame-size metrics on the CPU: the restatement (tests/frame_metrics_ref.py) against the reference's own functions
(tests/golden/frame_metrics.npz, tools/make_golden_frame_metrics.py), and the host logic of FrameMetrics / evaluate_frames /
FrameStore.record_gt over a stand-in for gwd_eval_frames.  The kernel itself: tests/test_frame_metrics_gpu.py.

Tolerances against the fixture: the three accuracies, the pixel counts and the confusion counts are exact; the other measures are
fp32 means in the reference against f64 sums here, 2e-6 relative - the bar of tests/test_eval_metrics.py for the same arithmetic."""
import os
import pickle
import re

import numpy as np
import pytest
import torch

from gw_depth_amd import dataset, decode, hip
from gw_depth_amd.evaluate import METRIC_NAMES, SEG_LABELS, FrameMetrics, evaluate_frames
from oracle import eval_ref
from tests import frame_metrics_ref as F
from tests.fake_device import FakeDevice

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "frame_metrics.npz")


class FrameFakeDevice(FakeDevice):
    """tests/fake_device.py plus gwd_eval_frames, restated through tests/frame_metrics_ref.py; it counts its launches."""
    launches = 0

    def eval_frames(self, depth, label, gt, dmin, dmax, bin_edges, workspace, offset, sums, measures, conf, running, confusion):
        type(self).launches += 1
        R = running.shape[0]
        assert R == 3 + max(len(bin_edges) - 1, 0) and workspace.numel() >= hip.EVAL_FRAMES_WS_BYTES
        for b, (dmm, lab) in enumerate(gt):
            h, w = dmm.shape
            mm = dmm.numpy() if dmm.element_size() == 4 else dmm.view(torch.int16).numpy().view(np.uint16)
            rec = F.score_frame(depth[b, :h, :w].numpy(), label[b, :h, :w].numpy(), mm, lab.numpy(), dmin, dmax, bin_edges)
            sums[offset + b] = torch.from_numpy(rec["sums"])
            measures[offset + b] = torch.from_numpy(rec["measures"])
            conf[offset + b] = torch.from_numpy(rec["conf"])
            for r in range(R):
                if rec["sums"][r, 0] != 0:
                    running[r, :9] += measures[offset + b, r]
                    running[r, 9] += 1
            confusion += conf[offset + b]
        return 0


@pytest.fixture()
def fake():
    FrameFakeDevice.launches = 0
    hip.set_library(FrameFakeDevice())
    yield FrameFakeDevice
    hip.set_library(None)


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLDEN))


def gold_frames(gold):
    return [(gold["depth%d" % i], gold["label%d" % i], gold["mm%d" % i], gold["raw%d" % i]) for i in range(3)]


def as_call(frames, width=4):
    """(result dict, gt list) of one predict_frames-shaped call over numpy frames: padding outside a frame holds 0 / 255."""
    Fh, Fw = max(f[0].shape[0] for f in frames), max(f[0].shape[1] for f in frames)
    depth = torch.zeros(len(frames), Fh, Fw)
    labels = torch.full((len(frames), Fh, Fw), 255, dtype=torch.uint8)
    gt = []
    for b, (p, l, mm, raw) in enumerate(frames):
        h, w = p.shape
        depth[b, :h, :w] = torch.from_numpy(p)
        labels[b, :h, :w] = torch.from_numpy(l)
        dmm = torch.from_numpy(mm.astype(np.uint16)).view(torch.uint16) if width == 2 else torch.from_numpy(mm.astype(np.int32))
        gt.append((dmm, torch.from_numpy(raw)))
    return {"depth": depth, "labels": labels}, gt


def many_frames(n, seed=0):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        h, w = int(rng.integers(2, 9)), int(rng.integers(2, 12))
        mm = rng.integers(0, 11000, size=(h, w)).astype(np.int32)
        if i == 3:
            mm[:] = 0                                                   # an image without a valid pixel
        pred = rng.uniform(-0.5, 11.0, size=(h, w)).astype(np.float32)
        raw = (rng.random((h, w)) < (0.0 if i == 1 else 0.5)).astype(np.uint8) * 255
        out.append((pred, (rng.random((h, w)) < 0.5).astype(np.uint8), mm, raw))
    return out


EDGES = (0.5, 2.0, 4.0, 10.0)


# ---------------------------------------------------------------------------------------------- restatement against the reference
def test_restatement_matches_the_reference_fixture(gold):
    edges = tuple(float(e) for e in gold["edges"])
    assert os.path.getsize(GOLDEN) < 100 * 1024 and len(edges) == 9
    seen_empty = False
    for i, frame in enumerate(gold_frames(gold)):
        assert frame[0].shape[0] <= 24 and frame[0].shape[1] <= 32
        rec = F.score_frame(*frame, float(gold["min_depth_eval"]), float(gold["max_depth_eval"]), edges)
        ref = gold["ref_measures%d" % i]
        np.testing.assert_array_equal(rec["sums"][:, 0], gold["ref_counts%d" % i])
        np.testing.assert_array_equal(rec["conf"], gold["ref_conf%d" % i])
        assert (np.isnan(rec["measures"]) == np.isnan(ref)).all()
        np.testing.assert_array_equal(rec["measures"][:, 6:], ref[:, 6:])                       # d1, d2, d3: bit-exact
        np.testing.assert_allclose(rec["measures"][:, :6], ref[:, :6], rtol=2e-6, atol=0, equal_nan=True)
        seen_empty |= bool((rec["sums"][:, 0] == 0).any())
        assert rec["sums"][0, 0] == rec["sums"][1, 0] + rec["sums"][2, 0] and rec["sums"][3:, 0].sum() <= rec["sums"][0, 0]
    assert seen_empty
    assert (gold["raw0"] == 0).all() and {0, 1, 10000, 65535} <= set(gold["mm1"].reshape(-1).tolist())
    assert np.isnan(gold["depth2"]).any() and np.isposinf(gold["depth2"]).any() and np.isneginf(gold["depth2"]).any() and (gold["depth2"] < 0).any()


def test_restatement_region_zero_is_the_pinned_oracle(gold):
    """Region "all" of the restatement against oracle/eval_ref.depth_errors (pinned by the reference's evaluate())."""
    for frame in gold_frames(gold):
        rec = F.score_frame(*frame, 1e-3, 10.0)
        g = frame[2].astype(np.float32) / np.float32(1000.0)
        p, valid = eval_ref.clamp_and_mask(frame[0], g, 1e-3, 10.0)
        ref = np.asarray(eval_ref.depth_errors(g[valid], p[valid]), dtype=np.float64)
        np.testing.assert_array_equal(rec["measures"][0, 6:], ref[6:])
        np.testing.assert_allclose(rec["measures"][0, :6], ref[:6], rtol=2e-6)


# ---------------------------------------------------------------------------------------------- FrameMetrics host logic
def test_compute_keys_and_closing_arithmetic(fake, gold):
    edges = tuple(float(e) for e in gold["edges"])
    frames = gold_frames(gold)
    fm = FrameMetrics("cpu", depth_bins=edges)
    for width in (4, 2):                                               # one launch per call, both GT widths: the same records
        fm.reset()
        before = fake.launches
        fm.update(*as_call(frames, width))
        assert fake.launches == before + 1
        rec = fm.per_image()
        assert rec["ids"].tolist() == [0, 1, 2] and rec["sums"].shape == (3, 11, 10) and rec["measures"].shape == (3, 11, 9)
        out = fm.compute()
        want = F.closing(*F.running_fold(rec["sums"], rec["measures"], rec["confusion"]), rec["sums"])
        np.testing.assert_equal(out, want)                             # (NaN-aware, otherwise exact)
    regions = ["glass", "nonglass"] + ["bin%d" % k for k in range(8)]
    for m in METRIC_NAMES:
        assert m in out and "pixel/" + m in out and "glass/" + m in out and "pixel/bin0/" + m in out
    counts = np.stack([gold["ref_counts%d" % i] for i in range(3)])
    assert counts[0, 1] == 0 and counts[0, 10] == 0                                  # frame 0: no glass, nothing in [8, 10) m
    assert out["n_images"] == dict(zip(["all"] + regions, (counts > 0).sum(0).tolist())) and out["n_images"]["glass"] == 2
    assert set(SEG_LABELS + ["Pixel accuracy", "Mean accuracy", "Mean IU"]) <= set(out)
    # region "all": the mean over images of the reference's own per-image measures; the segmentation scores from its confusion
    ref_mean = np.mean([gold["ref_measures%d" % i][0] for i in range(3)], axis=0)
    for k, m in enumerate(METRIC_NAMES):
        assert out[m] == pytest.approx(ref_mean[k], rel=2e-6)
    seg = eval_ref.seg_scores(sum(gold["ref_conf%d" % i] for i in range(3)).reshape(2, 2).astype(np.float64))
    for k, v in seg.items():
        assert out[k] == pytest.approx(v, rel=1e-12)
    # pixel-weighted: all valid pixels of the three frames as one set
    total = rec["sums"].sum(0)
    np.testing.assert_allclose([out["pixel/" + m] for m in METRIC_NAMES], F.measures_from_sums(total)[0], rtol=1e-12)
    np.testing.assert_array_equal(fm.running.numpy()[:, 9], (counts > 0).sum(0))


def test_worst_orders_by_value_and_skips_nan(fake):
    frames = many_frames(6, seed=4)
    fm = FrameMetrics("cpu", depth_bins=EDGES)
    fm.update(*as_call(frames), ids=[10, 11, 12, 13, 14, 15])
    rec = fm.per_image()
    rms = rec["measures"][:, 0, 3]
    assert np.isnan(rms[3])
    want = sorted([(10 + i, float(v)) for i, v in enumerate(rms) if not np.isnan(v)], key=lambda t: (-t[1], t[0]))
    assert fm.worst(3) == want[:3] and fm.worst(100) == want and len(want) == 5 and fm.worst(0) == []
    glass = rec["measures"][:, 1, 1]
    got = fm.worst(10, key="abs_rel", region="glass")
    assert [i for i, _ in got] == [10 + int(i) for i in np.lexsort((np.arange(6), -glass)) if not np.isnan(glass[i])]
    assert 11 not in [i for i, _ in got]                               # image 1 has no glass
    with pytest.raises(ValueError):
        fm.worst(1, key="nope")
    with pytest.raises(ValueError):
        fm.worst(1, region="bin9")


def test_merge_of_any_split_equals_the_single_pass_bit_for_bit(fake):
    frames = many_frames(13, seed=9)
    single = FrameMetrics("cpu", depth_bins=EDGES)
    for at in range(0, 13, 5):
        single.update(*as_call(frames[at:at + 5]), ids=range(at, min(at + 5, 13)))
    want = single.compute()
    run_dev = single.running.numpy().copy()
    rec = single.per_image()
    run_host, _ = F.running_fold(rec["sums"], rec["measures"], rec["confusion"])
    np.testing.assert_array_equal(run_dev, run_host)                   # ids ascending: the device's totals are compute()'s
    splits = [[[0, 1, 2, 3, 4, 5, 6], [7, 8, 9, 10, 11, 12]], [[12, 3, 7], [0, 11, 5, 1], [2], [10, 9, 8, 6, 4]],
              [list(range(0, 13, 2)), list(range(1, 13, 2))], [[k] for k in reversed(range(13))]]
    for split in splits:
        states = []
        for part in split:
            fm = FrameMetrics("cpu", depth_bins=EDGES, capacity_images=16)
            for at in range(0, len(part), 3):
                ids = part[at:at + 3]
                fm.update(*as_call([frames[i] for i in ids]), ids=ids)
            states.append(pickle.loads(pickle.dumps(fm.state())))          # a state travels between ranks
        merged = FrameMetrics.merge(states)
        got = merged.compute()
        np.testing.assert_equal(got, want)                             # bit for bit (NaN-aware)
        assert list(got) == list(want)
        assert merged.worst(4) == single.worst(4) and merged.images_seen == 13
        assert sorted(merged.per_image()["ids"].tolist()) == list(range(13))
        with pytest.raises(RuntimeError):
            merged.update(*as_call(frames[:1]))
    again = FrameMetrics.merge([FrameMetrics.merge(states[:5]).state(), FrameMetrics.merge(states[5:]).state()])
    np.testing.assert_equal(again.compute(), want)


def test_merge_refuses_duplicate_ids_and_mixed_settings(fake):
    frames = many_frames(4, seed=2)
    a, b = FrameMetrics("cpu", depth_bins=EDGES), FrameMetrics("cpu", depth_bins=EDGES)
    a.update(*as_call(frames[:2]), ids=[0, 1])
    b.update(*as_call(frames[2:]), ids=[1, 2])
    with pytest.raises(ValueError, match="twice"):
        FrameMetrics.merge([a.state(), b.state()])
    c = FrameMetrics("cpu")
    c.update(*as_call(frames[2:]), ids=[5, 6])
    with pytest.raises(ValueError, match="different"):
        FrameMetrics.merge([a.state(), c.state()])
    with pytest.raises(ValueError):
        FrameMetrics.merge([])


def test_capacity_overflow_raises_before_anything_is_launched(fake):
    frames = many_frames(5, seed=3)
    fm = FrameMetrics("cpu", capacity_images=4)
    fm.update(*as_call(frames[:3]))
    with pytest.raises(RuntimeError, match="capacity"):
        fm.update(*as_call(frames[3:]))
    assert fake.launches == 1 and fm.images_seen == 3
    fm.update(*as_call(frames[3:4]))
    assert fm.images_seen == 4 and fm.per_image()["ids"].tolist() == [0, 1, 2, 3]


def test_shape_and_dtype_refusals(fake):
    frames = many_frames(3, seed=6)
    fm = FrameMetrics("cpu")
    res, gt = as_call(frames)
    bad = [
        (dict(res, depth=res["depth"].double()), gt, None, ValueError),
        (dict(res, labels=res["labels"].long()), gt, None, ValueError),
        (dict(res, labels=res["labels"][:, :-1]), gt, None, ValueError),
        (res, gt[:2], None, ValueError),
        (res, gt, [0, 1], ValueError),
        (res, [(gt[0][0].float(), gt[0][1])] + gt[1:], None, TypeError),
        (res, [(gt[0][0].long(), gt[0][1])] + gt[1:], None, TypeError),
        (res, [(gt[0][0], gt[0][1].long())] + gt[1:], None, TypeError),
        (res, [(gt[0][0], gt[0][1][:-1])] + gt[1:], None, ValueError),
        (res, [(gt[0][0].to(torch.int16), gt[0][1])] + gt[1:], None, TypeError),                # two widths in one call
        (res, [(torch.zeros(99, 3, dtype=torch.int32), torch.zeros(99, 3, dtype=torch.uint8))] + gt[1:], None, ValueError),
        ({"depth": torch.zeros(3, 40, 40), "labels": torch.zeros(3, 40, 40, dtype=torch.uint8)}, gt, None, ValueError),   # not these frames
    ]
    for r, g, ids, exc in bad:
        with pytest.raises(exc):
            fm.update(r, g, ids=ids)
    big = as_call(many_frames(17, seed=1))
    with pytest.raises(ValueError):
        fm.update(*big)
    assert fake.launches == 0 and fm.images_seen == 0
    for bins in ([1.0], [3.0, 2.0], list(range(11)), [0.0, float("nan")]):
        with pytest.raises(ValueError):
            FrameMetrics("cpu", depth_bins=bins)
    with pytest.raises(ValueError):
        FrameMetrics("cpu", capacity_images=0)


# ---------------------------------------------------------------------------------------------- record_gt, evaluate_frames
def cpu_store(frames, where="device"):
    """A FrameStore over records built by hand in host memory (the layout of decode.plane_layout)."""
    sizes = [f[0].shape for f in frames]
    offsets, total = dataset._batch_layout(sizes)
    arena = torch.zeros(total, dtype=torch.uint8)
    view = arena.numpy()
    rng = np.random.default_rng(0)
    for o, (h, w), f in zip(offsets, sizes, frames):
        o_r, o_d, o_l, _ = decode.plane_layout(h, w)
        view[o + o_r:o + o_r + 3 * h * w] = rng.integers(0, 256, size=3 * h * w)
        view[o + o_d:o + o_d + 2 * h * w] = f[2].astype("<u2").reshape(-1).view(np.uint8)
        view[o + o_l:o + o_l + h * w] = f[3].reshape(-1)
    n = len(frames)
    return dataset.FrameStore(arena, offsets, [tuple(s) for s in sizes], [None] * n, list(range(n)), ["img%02d" % i for i in range(n)], "cpu", where)


def test_record_gt_returns_views_of_the_records():
    frames = [f for f in many_frames(5, seed=8)]
    for f in frames:
        f[2][0, 0] = 65535
    store = cpu_store(frames)
    got = store.record_gt([4, 0, 2])
    for (dmm, lab), i in zip(got, [4, 0, 2]):
        assert dmm.dtype == torch.uint16 and lab.dtype == torch.uint8 and dmm.shape == lab.shape == frames[i][0].shape
        assert dmm.untyped_storage().data_ptr() == store.arena.untyped_storage().data_ptr()
        assert (dmm.data_ptr() - store.arena.data_ptr()) % 256 == 0
        rgb = store.record_rgb([i])[0]
        assert rgb.shape == frames[i][0].shape + (3,) and rgb.data_ptr() == store.arena.data_ptr() + store.offsets[i]
        np.testing.assert_array_equal(dmm.view(torch.int16).numpy().view(np.uint16), frames[i][2].astype(np.uint16))
        np.testing.assert_array_equal(lab.numpy(), frames[i][3])
    with pytest.raises(IndexError):
        store.record_gt([5])
    with pytest.raises(ValueError):
        store.record_gt([])
    with pytest.raises(ValueError, match="where='device'"):
        cpu_store(frames, where="pinned").record_gt([0])


class CannedSession:
    """predict_frames that returns canned predictions for the frames it is handed (found by their first RGB bytes)."""
    min_depth, max_depth = 1e-3, 10.0

    def __init__(self, frames, store):
        self.frames, self.calls = frames, []
        self.keys = {bytes(store.arena[o:o + 6].tolist()): i for i, o in enumerate(store.offsets)}

    def _device(self):
        return torch.device("cpu")

    def predict_frames(self, rgb, size=1024, max_size=1024, ensemble=False, pad_to=None, copy=False):
        idx = [self.keys[bytes(f.reshape(-1)[:6].tolist())] for f in rgb]
        self.calls.append((idx, ensemble, size, max_size, pad_to))
        return as_call([self.frames[i] for i in idx])[0]


class WidenFake(FrameFakeDevice):
    widens = 0

    def widen_u16_batch(self, jobs):
        type(self).widens += 1
        for src, dst in jobs:
            dst.copy_(torch.from_numpy(src.numpy().view("<u2").astype(np.int32)))


def test_evaluate_frames_walks_the_source_in_batches():
    frames = many_frames(7, seed=12)
    hip.set_library(WidenFake())
    try:
        WidenFake.launches = 0
        for where in ("device", "pinned"):
            WidenFake.widens = 0
            store = cpu_store(frames, where)
            sess = CannedSession(frames, store)
            before = WidenFake.launches
            out = evaluate_frames(sess, store, batch=3, ensemble=True, size=96, max_size=128, depth_bins=EDGES)
            assert [c[0] for c in sess.calls] == [[0, 1, 2], [3, 4, 5], [6]] and all(c[1:] == (True, 96, 128, None) for c in sess.calls)
            assert WidenFake.launches == before + 3
            assert out["names"] == {i: "img%02d" % i for i in range(7)}
            single = FrameMetrics("cpu", depth_bins=EDGES)
            single.update(*as_call(frames))
            want = single.compute()
            np.testing.assert_equal({k: v for k, v in out.items() if k != "names"}, want)
            assert WidenFake.widens == (0 if where == "device" else 3)             # records in place: no widen launch
        fm = FrameMetrics("cpu", depth_bins=EDGES)
        out = evaluate_frames(CannedSession(frames, store), store, indices=[5, 2], batch=8, metrics=fm)
        assert fm.per_image()["ids"].tolist() == [5, 2] and out["n_images"]["all"] == 2 and sorted(out["names"]) == [2, 5]
        for batch, ensemble in ((9, True), (17, False), (0, False)):
            with pytest.raises(ValueError):
                evaluate_frames(CannedSession(frames, store), store, batch=batch, ensemble=ensemble)
    finally:
        hip.set_library(None)


def test_header_binding_and_kernel_constants_agree():
    header = open(os.path.join(ROOT, "include", "gwdepth.h")).read()
    assert "#define GWD_VERSION 10" in header and "gwd_eval_frames" in hip.ENTRY_POINTS
    ws = re.search(r"#define GWD_EVAL_FRAMES_WS_BYTES \(([^)]*)\)", header).group(1)
    assert eval(ws) == hip.EVAL_FRAMES_WS_BYTES
    assert "#define GWD_EVAL_FRAMES_BATCH %d" % hip.EVAL_FRAMES_BATCH in header
    assert "#define GWD_EVAL_FRAMES_MAX_BINS %d" % hip.EVAL_FRAMES_MAX_BINS in header
    import ctypes
    assert ctypes.sizeof(hip.FrameEvalJob) == 24
