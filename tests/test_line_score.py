"""CPU: line scoring (structural AP / F after L-CNN's line NMS) against tests/golden/line_score.npz.

The fixture holds what the reference's OWN postprocess / msTPFP / ap returned on float64 arrays (tools/make_golden_linescore.py): the
kept ids, the clipped lines in the 128 x 128 space, a flag per (NMS threshold, sAP threshold, image, query) and the AP / F values.
  * the NumPy restatement tests/line_score_ref.py equals it: ids and flags identical, lines within 1e-9 px, AP / F within 1e-12;
  * gw_depth_amd/csrc/linescore.h - the scalar geometry the device kernel calls - compiled for the host with g++ and driven by the
    serial loop of tests/linescore_host.cpp reproduces ids, lines and flags (a sequencing bug shows here without a GPU);
  * LineMetrics.compute() closes the fixture's flags to the fixture's AP / F;
  * evaluate() without args.line_ap returns exactly the keys it returned before the feature.
Bounds: the lines are ~20 f64 operations on coordinates below 1e3, an error near 1e-13; 1e-9 is 1e4 times that.  AP / F are sums of
at most a few hundred f64 terms in [0, 100]: 1e-12 leaves two decimal orders above their rounding.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from gw_depth_amd import hip
from gw_depth_amd.evaluate import METRIC_NAMES, SEG_LABELS, LineMetrics, evaluate
from tests import line_score_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "line_score.npz")
LINE_TOL, STAT_TOL = 1e-9, 1e-12


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLDEN))


def gts(gold):
    return [gold["gt_lines"][b, :gold["gt_counts"][b]] for b in range(len(gold["sizes"]))]


def check_stats(stats, gold):
    for t, thr in enumerate(gold["nms_thresholds"]):
        for s, st in enumerate(gold["sap_thresholds"]):
            for kind in ("sAP", "sF"):
                k = R.key(kind, st, thr)
                print("%-16s %.12f fixture %.12f" % (k, stats[k], gold[kind][t, s]))
                assert abs(stats[k] - float(gold[kind][t, s])) <= STAT_TOL, k


def test_fixture_covers_the_cases(gold):
    """Suppression, clipping and all three outcomes occur; the trims, the odd size, the image without ground truth and the tie are in."""
    kept, flag, B = gold["kept"], gold["flag"], len(gold["sizes"])
    assert gold["pred_lines"].shape == (B, 100, 6) and B >= 6
    assert [tuple(s) for s in gold["sizes"]].count((480, 640)) >= 3 and (427, 569) in [tuple(s) for s in gold["sizes"]]
    assert (gold["gt_counts"] == 0).any() and sorted(gold["trim"])[:2] == [15, 70]
    for t in range(kept.shape[0]):
        assert all((flag[t] == v).any() for v in (0, 1, 2))
        assert (~kept[t, :, :15]).any()                                              # something inside the trimmed range is suppressed
    lines = gold["pred_lines"][:, :, :4].reshape(B, 100, 2, 2)[..., ::-1] * (128.0 / 1.0)
    full = np.abs(gold["kept_lines"][0].reshape(B, 100, 2, 2) - lines.astype(np.float64)).reshape(B, 100, 4).max(-1)
    assert ((full > 1e-3) & kept[0]).any()                                           # a kept line that is not the query's whole line
    a, b = gold["tie"]
    assert gold["scores"][0, a] == gold["scores"][0, b] and (flag[:, :, 0, a] == flag[:, :, 0, b]).all()
    assert os.path.getsize(GOLDEN) < 100 * 1024


def test_restatement_equals_the_reference(gold):
    for b, (lines, size, gt) in enumerate(zip(gold["pred_lines"], gold["sizes"], gts(gold))):
        kept, kept_lines, flag = R.image_chain(lines, size, gt, gold["nms_thresholds"], gold["sap_thresholds"])
        assert (kept == gold["kept"][:, b]).all(), b
        assert (flag == gold["flag"][:, :, b]).all(), b
        scale = np.array([size[0], size[1], size[0], size[1]]) / 128.0                # the bound is in pixels of the image
        err = float(np.abs((kept_lines - gold["kept_lines"][:, b]) * scale).max())
        print("image %d: clipped lines off by %.3g px" % (b, err))
        assert err <= LINE_TOL
    check_stats(R.score_all(gold["scores"], gold["pred_lines"], gold["sizes"], gts(gold), gold["nms_thresholds"], gold["sap_thresholds"]),
                gold)


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("linescore") / "liblinescore_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-I",
                           os.path.join(ROOT, "gw_depth_amd", "csrc"), os.path.join(HERE, "linescore_host.cpp"), "-o", out])
    lib = ctypes.CDLL(out)
    vp = ctypes.c_void_p
    lib.ls_host_image.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, ctypes.c_int, vp, ctypes.c_int, vp,
                                  ctypes.c_int, vp, vp, vp]
    lib.ls_host_image.restype = ctypes.c_int
    return lib


def host_image(lib, lines, size, gt, nms, sap):
    lines, gt = np.ascontiguousarray(lines, np.float32), np.ascontiguousarray(gt, np.float32).reshape(-1, 4)
    nms, sap = np.ascontiguousarray(nms, np.float64), np.ascontiguousarray(sap, np.float64)
    Q, ld = lines.shape
    T, S = len(nms), len(sap)
    flag, kept_lines, kept = np.empty((T, S, Q), np.uint8), np.empty((T, Q, 4), np.float64), np.empty((T, Q), np.uint8)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    n = lib.ls_host_image(p(lines), Q, ld, int(size[0]), int(size[1]), p(gt), len(gt), p(nms), T, p(sap), S, p(flag), p(kept_lines), p(kept))
    return n, kept.astype(bool), kept_lines, flag


def test_kernel_header_on_the_host_equals_the_reference(gold, host_lib):
    for b, (lines, size, gt) in enumerate(zip(gold["pred_lines"], gold["sizes"], gts(gold))):
        n, kept, kept_lines, flag = host_image(host_lib, lines, size, gt, gold["nms_thresholds"], gold["sap_thresholds"])
        assert n == int(gold["trim"][b])
        assert (kept == gold["kept"][:, b]).all(), b
        assert (flag == gold["flag"][:, :, b]).all(), b
        scale = np.array([size[0], size[1], size[0], size[1]]) / 128.0
        err = float(np.abs((kept_lines - gold["kept_lines"][:, b]) * scale).max())
        print("image %d: clipped lines off by %.3g px" % (b, err))
        assert err <= LINE_TOL


def test_kernel_header_handles_a_zero_length_line_without_nan(host_lib):
    lines = np.array([[0.5, 0.5, 0.5, 0.5], [0.5, 0.5, 0.5, 0.5 + 1e-4], [0.2, 0.2, 0.8, 0.2]], np.float32)
    _, kept, kept_lines, flag = host_image(host_lib, lines, (480, 640), np.zeros((0, 4)), [0.01], [5])
    want = R.image_chain(lines, (480, 640), np.zeros((0, 4)), [0.01], [5])
    assert np.isfinite(kept_lines).all() and (kept == want[0]).all() and (flag == want[2]).all()
    assert np.abs(kept_lines - want[1]).max() <= LINE_TOL


def loaded(gold, device="cpu"):
    """A LineMetrics whose buffers hold the fixture's flags, as if update() had written them."""
    B, Q = gold["scores"].shape
    lm = LineMetrics(device, gold["nms_thresholds"], gold["sap_thresholds"], capacity_images=B + 3)
    lm._reserve(B, Q)
    lm._flag.fill_(7)
    lm._score.fill_(9.0)                                                             # unused slots must not reach compute()
    lm._gt_seen.fill_(1000)
    lm._flag[:, :, :B] = torch.from_numpy(gold["flag"])
    lm._score[:B] = torch.from_numpy(gold["scores"])
    lm._gt_seen[:B] = torch.from_numpy(gold["gt_counts"])
    lm.images_seen = B
    return lm


def test_line_metrics_closing_arithmetic(gold):
    stats = loaded(gold).compute()
    check_stats(stats, gold)
    assert stats["n_gt"] == int(gold["gt_counts"].sum())
    assert sorted(stats) == sorted(["n_gt"] + [R.key(k, s, t) for k in ("sAP", "sF") for s in (5, 10, 15) for t in (0.010, 0.015)])
    assert "sAP10_nms0_010" in stats


def test_line_metrics_growth_keeps_what_was_written(gold):
    lm = loaded(gold)
    B, Q = gold["scores"].shape
    lm._reserve(4 * B, Q)                                                            # beyond the capacity: new buffers, old slots copied
    assert lm.capacity >= 4 * B and lm._flag.shape[2] == lm.capacity
    check_stats(lm.compute(), gold)
    with pytest.raises(ValueError):
        lm._reserve(4 * B, Q + 1)
    assert LineMetrics("cpu").compute() == {}


class HostLineDevice:
    """Stands in for the device library on the CPU: line_score through the host build of csrc/linescore.h, so the host logic of
    LineMetrics (slots, growth, the sort, the copy) and of evaluate() runs end to end without a GPU.  The product never does this."""
    is_fake = True

    def __init__(self, lib):
        self.lib, self.calls = lib, 0

    def line_score(self, logits, lines, sizes, gt, gt_count, nms_thresholds, sap_thresholds, flag, kept_lines, score, gt_seen, slot):
        self.calls += 1
        for b in range(lines.shape[0]):
            n_gt = int(gt_count[b])
            _, _, kl, fl = host_image(self.lib, lines[b].numpy(), sizes[b].tolist(), gt[b, :n_gt].numpy(), nms_thresholds, sap_thresholds)
            flag[:, :, slot + b] = torch.from_numpy(fl)
            kept_lines[:, slot + b] = torch.from_numpy(kl)
            score[slot + b] = torch.softmax(logits[b], -1)[:, 0]
            gt_seen[slot + b] = n_gt


@pytest.fixture()
def host_device(host_lib):
    dev = HostLineDevice(host_lib)
    hip.set_library(dev)
    yield dev
    hip.set_library(None)


def fixture_batches(gold, splits):
    t = lambda k: torch.from_numpy(gold[k])
    lo = 0
    for n in splits:
        yield [t(k)[lo:lo + n] for k in ("pred_logits", "pred_lines", "sizes", "gt_lines", "gt_counts")]
        lo += n


@pytest.mark.parametrize("splits,capacity", [((6,), 256), ((1, 3, 2), 1)])
def test_line_metrics_host_logic_in_batches(gold, host_device, splits, capacity):
    lm = LineMetrics("cpu", gold["nms_thresholds"], gold["sap_thresholds"], capacity_images=capacity)
    for batch in fixture_batches(gold, splits):
        lm.update(*batch)
    assert host_device.calls == len(splits) and lm.images_seen == 6
    check_stats(lm.compute(), gold)
    assert np.abs(lm.kept_lines().numpy() - gold["kept_lines"]).max() <= LINE_TOL * 128 / 640


def test_evaluate_with_line_ap_feeds_line_metrics(gold, host_device):
    """evaluate(line_ap) over canned outputs: sizes from the batch tensor, targets padded into one tensor, stats merged.  Batches of
    one size each, because the size evaluate() passes on is the batch tensor's (H, W)."""
    from gw_depth_amd.model import NestedTensor
    order = [0, 1, 2, 4, 3, 5]                                                       # 480 x 640 four times, then the two other sizes
    groups = [[0, 1], [2, 4], [3], [5]]

    class Canned(torch.nn.Module):
        k = 0

        def forward(self, samples, reflc_mat=None, img_name=None):
            ids = groups[self.k]
            self.k += 1
            return {"pred_logits": torch.from_numpy(gold["pred_logits"][ids]), "pred_lines": torch.from_numpy(gold["pred_lines"][ids])}

    loader = []
    for ids in groups:
        h, w = (int(v) for v in gold["sizes"][ids[0]])
        blank = NestedTensor(torch.zeros(len(ids), 3, h, w), torch.zeros(len(ids), h, w, dtype=torch.bool))
        targets = [{"lines": torch.from_numpy(gold["gt_lines"][i, :gold["gt_counts"][i]])} for i in ids]
        loader.append((blank, blank, blank, targets, ["img\n"]))
    args = type("A", (), dict(with_line=True, with_dense=False, line_ap=True))()
    stats = evaluate(Canned(), (None,) * 4, None, loader, None, "cpu", None, args)
    assert stats["n_gt"] == int(gold["gt_counts"].sum()) and host_device.calls == len(groups)
    # the images arrive in another order than the fixture's: the flags are the same set, the tie order may differ, and the fixture's
    # one pair of equal scores has equal flags - so AP / F are the fixture's
    assert order != sorted(order)
    check_stats(stats, gold)


def test_line_metrics_needs_the_device(gold):
    hip.set_library(None)
    lm = LineMetrics("cpu")
    z = torch.zeros
    with pytest.raises(hip.HipUnavailable):
        lm.update(z(1, 4, 2), z(1, 4, 6), z(1, 2, dtype=torch.int32), z(1, 1, 4), z(1, dtype=torch.int32))


def test_evaluate_without_line_ap_is_unchanged():
    """The keys of today, with and without the new flag where --with_line is off; the save_dense / save_line refusal stands."""
    from tests.fake_device import FakeDevice
    from tests.test_eval_metrics import GOLDEN as DENSE, _Canned, _loader, _tensors
    dense = dict(np.load(DENSE))
    hip.set_library(FakeDevice())
    try:
        pred, gt, seg, tgt = _tensors(dense)
        want = sorted(SEG_LABELS + ["Pixel accuracy", "Mean accuracy", "Mean IU"] + METRIC_NAMES)
        for extra in ({}, {"line_ap": False}, {"line_ap": True}):
            args = type("A", (), dict(with_line=False, with_dense=True, min_depth_eval=1e-3, max_depth_eval=10.0, **extra))()
            stats = evaluate(_Canned(pred, seg, 1), (None,) * 4, None, _loader(gt, tgt, 1), None, "cpu", None, args)
            assert sorted(stats) == want
        for kw in ({"save_dense": True}, {"save_line": True}):
            with pytest.raises(NotImplementedError):
                evaluate(_Canned(pred, seg, 1), (None,) * 4, None, [], None, "cpu", None, args, **kw)
    finally:
        hip.set_library(None)
