"""gwd_eval_frames (csrc/evalframes.hip) on the device against tests/frame_metrics_ref.py, and evaluate_frames end to end.

Tolerances.  The kernel's count, the three threshold sums and the confusion counts are integers: exact.  Every other raw sum is an
f64 fold, in some fixed order, of fp32 terms that the restatement sums correctly rounded (math.fsum): an f64 fold of N exactly
representable terms errs by at most N * 2^-52 * sum |term| whatever its order, and that is the bound, computed per entry from the
region's pixel count and the restatement's sum of |term|.  The measures are compared with the closing arithmetic applied to the
kernel's OWN sums on the host (two correctly rounded operations either side: 1e-12 relative), the running totals with the same
sequential f64 adds (bit for bit).  Every figure is printed before it is asserted."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from gw_depth_amd import hip
from gw_depth_amd.evaluate import DenseMetrics
from tests import frame_metrics_ref as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "frame_metrics.npz")
EDGES = (0.5, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 8.0, 10.0)           # eight bins; the data below leaves [8, 10) empty
MIN_D, MAX_D = 1e-3, 10.0
GUARD, SENT = 16, -777.0


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    hip.set_library(None)
    lib = hip.library()
    assert not getattr(lib, "is_fake", False)
    return lib


@pytest.fixture(scope="module")
def workspace(lib):
    """ONE workspace for every call of this module: the tickets are zeroed here once and must come back to zero by themselves."""
    return torch.zeros(hip.EVAL_FRAMES_WS_BYTES, dtype=torch.uint8, device="cuda")


def make_frame(h, w, seed, glass=0.4, max_mm=7000):
    """(prediction fp32, predicted label uint8, GT millimetres int32, raw GT label uint8) with holes, special millimetre values,
    GT exactly on bin edges, predictions the clamp repairs and predicted labels outside {0, 1}."""
    rng = np.random.default_rng(seed)
    mm = rng.integers(300, max_mm, size=(h, w)).astype(np.int32)
    mm[rng.random((h, w)) < 0.1] = 0
    pred = (mm / 1000.0 * rng.uniform(0.6, 1.6, size=(h, w))).astype(np.float32)
    pred[mm == 0] = 2.0
    flat_mm, flat_p = mm.reshape(-1), pred.reshape(-1)
    special_mm = (0, 1, 10000, 65535, 1000, 2000, 500, 4000)
    special_p = (np.nan, np.inf, -np.inf, -2.0, 0.0, 20.0)
    for k, v in enumerate(special_mm[:max(min(len(special_mm), flat_mm.size - 1), 0)]):
        flat_mm[(k * 5 + 1) % flat_mm.size] = v
    for k, v in enumerate(special_p[:max(min(len(special_p), flat_p.size - 1), 0)]):
        flat_p[(k * 7 + 2) % flat_p.size] = v
    raw = (rng.random((h, w)) < glass).astype(np.uint8) * rng.choice(np.array([1, 128, 255], np.uint8), size=(h, w))
    lab = (rng.random((h, w)) < 0.5).astype(np.uint8)
    if lab.size > 4:
        lab.reshape(-1)[3] = 255
        lab.reshape(-1)[4] = 7
    return pred, lab, mm, raw


_REF = {}


def ref_of(key, frame, edges):
    """The restatement's record of a frame, computed once per (frame, edges) and shared."""
    k = (key, tuple(edges))
    if k not in _REF:
        _REF[k] = F.score_frame(*frame, MIN_D, MAX_D, edges)
    return _REF[k]


def guarded(shape, dtype, device="cuda"):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), SENT, dtype=dtype, device=device)
    return buf, buf[GUARD:GUARD + n].view(*shape)


def run(lib, workspace, frames, edges=(), width=4, Fh=None, Fw=None, offset=0, N=None, running=None, confusion=None, seed=0):
    """One gwd_eval_frames call over `frames`, planes of Fh x Fw (default: the largest frame) with garbage outside every frame:
    random depth with NaN, labels 0 / 1.  Outputs sit between guards; the records outside [offset, offset + B) hold a sentinel."""
    B = len(frames)
    Fh = Fh or max(f[0].shape[0] for f in frames)
    Fw = Fw or max(f[0].shape[1] for f in frames)
    N = N or offset + B
    R = 3 + max(len(edges) - 1, 0)
    rng = np.random.default_rng(1000 + seed)
    depth = rng.uniform(0.5, 9.0, size=(B, Fh, Fw)).astype(np.float32)
    depth[:, ::3, ::5] = np.nan
    label = (rng.random((B, Fh, Fw)) < 0.5).astype(np.uint8)
    gt = []
    for b, (p, l, mm, raw) in enumerate(frames):
        h, w = min(p.shape[0], Fh), min(p.shape[1], Fw)                  # (a frame larger than the planes: a refusal case)
        depth[b, :h, :w] = p[:h, :w]
        label[b, :h, :w] = l[:h, :w]
        dmm = torch.from_numpy(mm.astype(np.uint16)) if width == 2 else torch.from_numpy(mm)
        assert width == 4 or int(mm.max()) <= 65535
        gt.append((dmm.cuda(), torch.from_numpy(raw).cuda()))
    bufs = {"sums": guarded((N, R, 10), torch.float64), "measures": guarded((N, R, 9), torch.float64),
            "conf": guarded((N, 4), torch.int64), "running": guarded((R, 10), torch.float64), "confusion": guarded((4,), torch.int64)}
    bufs["running"][1].copy_(torch.zeros(R, 10, dtype=torch.float64) if running is None else torch.from_numpy(running))
    bufs["confusion"][1].copy_(torch.zeros(4, dtype=torch.int64) if confusion is None else torch.from_numpy(confusion))
    rc = lib.eval_frames(torch.from_numpy(depth).cuda(), torch.from_numpy(label).cuda(), gt, MIN_D, MAX_D, edges, workspace, offset,
                         *(bufs[k][1] for k in ("sums", "measures", "conf", "running", "confusion")))
    torch.cuda.synchronize()
    out = {"rc": rc}
    for k, (buf, view) in bufs.items():
        host = buf.cpu().numpy()
        assert (host[:GUARD] == SENT).all() and (host[-GUARD:] == SENT).all(), "guard beside %s overwritten" % k
        out[k] = view.cpu().numpy()
    if rc == 0:
        for k in ("sums", "measures", "conf"):
            assert (out[k][:offset] == SENT).all() and (out[k][offset + B:] == SENT).all(), "%s: a record outside the call was written" % k
            out[k] = out[k][offset:offset + B]
        assert int(workspace[:128].view(torch.int32).abs().sum()) == 0, "the tickets did not return to zero"
    return out


def check_record(got_sums, got_measures, got_conf, ref, what):
    """One image's record against the restatement, entry by entry, with the derived bound."""
    s, rs, ra = got_sums, ref["sums"], ref["abs_sums"]
    np.testing.assert_array_equal(s[:, :4], rs[:, :4], err_msg="%s: count / threshold sums" % (what,))
    np.testing.assert_array_equal(got_conf, ref["conf"], err_msg="%s: confusion" % (what,))
    bound = F.sum_bound(rs[:, :1], ra[:, 4:])
    err = np.abs(s[:, 4:] - rs[:, 4:])
    worst = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    print("%s: pixels %s  max |sum - fsum| / bound = %.3g" % (what, rs[:, 0].astype(int).tolist(), worst))
    assert (err <= bound).all(), (what, err, bound)
    assert s[0, 0] == s[1, 0] + s[2, 0]
    want = F.measures_from_sums(s)
    assert (np.isnan(got_measures) == np.isnan(want)).all(), what
    assert np.isnan(got_measures[s[:, 0] == 0]).all() and not np.isnan(got_measures[s[:, 0] > 0][:, 1:]).any(), what
    np.testing.assert_allclose(got_measures, want, rtol=1e-12, atol=0, equal_nan=True, err_msg=str(what))


def check_call(out, frames, keys, edges, what, running0=None, confusion0=None):
    assert out["rc"] == 0
    for b, (frame, key) in enumerate(zip(frames, keys)):
        check_record(out["sums"][b], out["measures"][b], out["conf"][b], ref_of(key, frame, edges), (what, key))
    run_ref, conf_ref = F.running_fold(out["sums"], out["measures"], out["conf"])
    np.testing.assert_array_equal(out["running"], run_ref + (0 if running0 is None else running0))
    np.testing.assert_array_equal(out["confusion"], conf_ref + (0 if confusion0 is None else confusion0))


SMALL = [(1, 1), (1, 7), (3, 5), (8, 16)] + [(3, w) for w in range(17, 24)]


@pytest.mark.parametrize("width", [2, 4])
@pytest.mark.parametrize("edges", [(), EDGES], ids=["bins0", "bins8"])
def test_small_frames_and_row_tails(lib, workspace, width, edges):
    """1 x 1, 1 x 7, 3 x 5, 8 x 16 and rows of 17..23 pixels in one call of eleven frames, both GT widths, no bins and eight bins
    (GT exactly on an edge, an empty bin)."""
    frames = [make_frame(h, w, seed=10 + i) for i, (h, w) in enumerate(SMALL)]
    out = run(lib, workspace, frames, edges, width)
    check_call(out, frames, ["small%d" % i for i in range(len(SMALL))], edges, "small w%d" % width)
    if edges:
        assert (out["sums"][:, -1, 0] == 0).all() and np.isnan(out["measures"][:, -1]).all()      # [8, 10) m: nothing there
        assert out["running"][-1, 9] == 0
        one = out["sums"][3]                                                                       # 8 x 16 holds GT 1000, 2000, 4000
        assert one[3:, 0].sum() <= one[0, 0] and one[4, 0] > 0 and one[5, 0] > 0 and one[7, 0] > 0


MIXED = [(8, 16), (24, 32), (5, 9), (40, 64), (1, 1), (17, 23), (33, 40), (64, 104), (2, 8), (7, 3), (16, 16), (3, 19), (31, 33),
         (48, 8), (9, 57), (12, 24)]


@pytest.mark.parametrize("edges", [(), EDGES], ids=["bins0", "bins8"])
def test_sixteen_mixed_frames_at_an_offset_twice(lib, workspace, edges):
    """One 16-frame call of mixed sizes with garbage around every frame, written at image offset 3 of 24 records on top of non-zero
    running totals; a second run gives the same bits."""
    frames = [make_frame(h, w, seed=40 + i) for i, (h, w) in enumerate(MIXED)]
    R = 3 + max(len(edges) - 1, 0)
    run0 = np.arange(R * 10, dtype=np.float64).reshape(R, 10) * 0.25
    conf0 = np.array([5, 6, 7, 8], dtype=np.int64)
    a = run(lib, workspace, frames, edges, 4, offset=3, N=24, running=run0, confusion=conf0)
    keys = ["mixed%d" % i for i in range(16)]
    assert a["rc"] == 0
    for b in range(16):
        check_record(a["sums"][b], a["measures"][b], a["conf"][b], ref_of(keys[b], frames[b], edges), ("mixed", b))
    want = run0.copy()
    for b in range(16):                                     # the kernel's order: image by image on top of what was there
        for r in range(R):
            if a["sums"][b, r, 0] != 0:
                want[r, :9] += a["measures"][b, r]
                want[r, 9] += 1
    np.testing.assert_array_equal(a["running"], want)
    np.testing.assert_array_equal(a["confusion"], conf0 + a["conf"].sum(0))
    b2 = run(lib, workspace, frames, edges, 4, offset=3, N=24, running=run0, confusion=conf0)
    for k in ("sums", "measures", "conf", "running", "confusion"):
        assert a[k].tobytes() == b2[k].tobytes(), k


@pytest.mark.parametrize("width", [2, 4])
@pytest.mark.parametrize("shape", [(300, 500), (720, 1280)], ids=["300x500", "720x1280"])
def test_large_frames_fold_over_workgroups(lib, workspace, shape, width):
    """300 x 500: 74 workgroups per slice, element-wise path (500 is no multiple of 8).  720 x 1280: the partition at its cap of 256,
    16-byte path."""
    frame = make_frame(*shape, seed=77)
    out = run(lib, workspace, [frame], EDGES, width)
    check_call(out, [frame], ["large%dx%d" % shape], EDGES, "large w%d" % width)


def test_record_does_not_depend_on_slot_neighbours_or_plane_size(lib, workspace):
    """A frame alone, in slot 11 of a mixed call, and under larger planes - of a width that keeps the 16-byte path and of one that
    forces the element-wise path - gives the same bits; so do the two GT widths."""
    probes = {"8x16": make_frame(8, 16, seed=90), "3x19": make_frame(3, 19, seed=91), "64x104": make_frame(64, 104, seed=92),
              "300x504": make_frame(300, 504, seed=93)}
    others = [make_frame(h, w, seed=40 + i) for i, (h, w) in enumerate(MIXED)]
    for name, frame in probes.items():
        alone = run(lib, workspace, [frame], EDGES, 4)
        check_record(alone["sums"][0], alone["measures"][0], alone["conf"][0], ref_of(name, frame, EDGES), ("alone", name))
        variants = {"narrow GT": run(lib, workspace, [frame], EDGES, 2)}
        h, w = frame[0].shape
        for Fw in (w + 8, w + 11):
            variants["planes %d x %d" % (h + 6, Fw)] = run(lib, workspace, [frame], EDGES, 4, Fh=h + 6, Fw=Fw)
        mixed = others[:11] + [frame] + others[12:15]
        m = run(lib, workspace, mixed, EDGES, 4, offset=2, seed=5)
        variants["slot 11"] = {k: m[k][11:12] for k in ("sums", "measures", "conf")}
        for what, v in variants.items():
            for k in ("sums", "measures", "conf"):
                assert v[k][0].tobytes() == alone[k][0].tobytes(), (name, what, k)


def test_equal_size_frames_agree_with_dense_metrics(lib, workspace):
    """Three 24 x 32 frames: DenseMetrics.update, fed one-hot logits of the labels and the converted GT, counts the same pixels;
    its measures are f64 folds of the same fp32 terms in another order, so each lies inside the derived bound of the other."""
    frames = []
    for i in range(3):
        p, l, mm, raw = make_frame(24, 32, seed=120 + i)
        frames.append((p, (l == 1).astype(np.uint8), mm, raw))                      # predicted labels 0 / 1 only
    out = run(lib, workspace, frames, (), 4)
    assert out["rc"] == 0
    pred = torch.from_numpy(np.stack([f[0] for f in frames])).cuda()
    # the converted GT is formed on the host with an IEEE division (gwd_collate's value); a device-side `/ 1000.0` may multiply by the reciprocal
    gt = torch.from_numpy(np.stack([f[2].astype(np.float32) / np.float32(1000.0) for f in frames])).cuda()
    lab = torch.from_numpy(np.stack([f[1] for f in frames])).cuda().long()
    logits = torch.nn.functional.one_hot(lab, 2).permute(0, 3, 1, 2).float().contiguous()
    seg_gt = (torch.from_numpy(np.stack([f[3] for f in frames])).cuda() > 0).long()
    dm = DenseMetrics("cuda", MIN_D, MAX_D)
    dense = dm.update(pred.unsqueeze(1), gt.unsqueeze(1), logits, seg_gt.unsqueeze(1)).cpu().numpy()
    np.testing.assert_array_equal(dm.confusion.cpu().numpy(), out["confusion"])
    assert float(dm.running[9]) == 3 and (out["running"][0, 9] == 3)
    for b, frame in enumerate(frames):
        ref = ref_of("dense%d" % b, frame, ())
        n, ra = ref["sums"][0, 0], ref["abs_sums"][0]
        got = out["measures"][b, 0]
        np.testing.assert_array_equal(got[6:], dense[b, 6:])                        # d1, d2, d3: the same integers over the same count
        bound = 2 * F.sum_bound(n, ra) / n                                          # two folds, each within the bound of fsum
        slack = 1 + 1e-12                                                           # the closing divisions and square roots
        for k, col in ((1, 5), (2, 9), (4, 6)):                                     # abs_rel, log10, sq_rel: sum / n
            print("frame %d %s: |delta| %.3g bound %.3g" % (b, F.METRIC_NAMES[k], abs(got[k] - dense[b, k]), bound[col]))
            assert abs(got[k] - dense[b, k]) <= bound[col] * slack + 1e-12 * abs(got[k])
        for k, col in ((3, 4), (5, 8)):                                             # rms, log_rms: sqrt(sum / n)
            assert abs(got[k] ** 2 - dense[b, k] ** 2) <= bound[col] * slack + 4e-12 * got[k] ** 2
        me = ref["sums"][0, 7] / n                                                  # silog: 100 sqrt(me2 - me^2)
        var_bound = bound[8] + 2 * abs(me) * bound[7] + bound[7] ** 2
        assert abs((got[0] / 100) ** 2 - (dense[b, 0] / 100) ** 2) <= var_bound * slack + 1e-12 * (ref["abs_sums"][0, 8] / n + me * me)


def test_fixture_frames_against_the_reference(lib, workspace):
    """The three frames of tests/golden/frame_metrics.npz, scored by the reference's own compute_depth_errors / get_confusion_matrix:
    accuracies and confusion exact, the other measures 2e-6 (fp32 means there, f64 sums here)."""
    g = dict(np.load(GOLDEN))
    frames = [(g["depth%d" % i], g["label%d" % i], g["mm%d" % i], g["raw%d" % i]) for i in range(3)]
    edges = tuple(float(e) for e in g["edges"])
    for width in (2, 4):
        out = run(lib, workspace, frames, edges, width)
        assert out["rc"] == 0
        for i in range(3):
            ref = g["ref_measures%d" % i]
            np.testing.assert_array_equal(out["sums"][i][:, 0], g["ref_counts%d" % i])
            np.testing.assert_array_equal(out["conf"][i], g["ref_conf%d" % i])
            assert (np.isnan(out["measures"][i]) == np.isnan(ref)).all()
            np.testing.assert_array_equal(out["measures"][i][:, 6:], ref[:, 6:])
            np.testing.assert_allclose(out["measures"][i][:, :6], ref[:, :6], rtol=2e-6, atol=0, equal_nan=True)


def test_bad_arguments_return_their_codes_and_launch_nothing(lib, workspace):
    frame = make_frame(8, 16, seed=3)
    f2 = make_frame(9, 16, seed=4)

    def untouched(out):
        for k in ("sums", "measures", "conf"):
            assert (out[k] == SENT).all(), k
        assert (out["running"] == 0).all() and (out["confusion"] == 0).all()

    out = run(lib, workspace, [frame], tuple(reversed(EDGES)), 4)                   # descending edges
    assert out["rc"] == -1
    untouched(out)
    out = run(lib, workspace, [frame], (1.0, float("nan"), 3.0), 4)
    assert out["rc"] == -1
    untouched(out)
    out = run(lib, workspace, [frame], tuple(float(k) for k in range(10)), 4)        # nine bins
    assert out["rc"] == -1
    untouched(out)
    out = run(lib, workspace, [frame] * 17, (), 4)
    assert out["rc"] == -1
    untouched(out)
    out = run(lib, workspace, [frame, f2], (), 4, Fh=8, Fw=16)                       # a frame larger than the planes
    assert out["rc"] == -1
    untouched(out)
    # raw calls: GT element widths 1 and 8, min >= max, a misaligned int32 plane
    depth = torch.zeros(1, 8, 16, device="cuda")
    label = torch.zeros(1, 8, 16, dtype=torch.uint8, device="cuda")
    mm = torch.zeros(8 * 16 + 4, dtype=torch.int32, device="cuda")
    raw = torch.zeros(8, 16, dtype=torch.uint8, device="cuda")
    sums = torch.full((1, 3, 10), SENT, dtype=torch.float64, device="cuda")
    meas = torch.full((1, 3, 9), SENT, dtype=torch.float64, device="cuda")
    conf = torch.full((1, 4), int(SENT), dtype=torch.int64, device="cuda")
    running = torch.zeros(3, 10, dtype=torch.float64, device="cuda")
    confusion = torch.zeros(4, dtype=torch.int64, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def raw_call(gt_ptr, gt_bytes, dmin, dmax):
        job = (hip.FrameEvalJob * 1)()
        job[0].gt_depth_mm, job[0].gt_label, job[0].fh, job[0].fw = gt_ptr, raw.data_ptr(), 8, 16
        return lib.lib.gwd_eval_frames(job, 1, depth.data_ptr(), label.data_ptr(), 8, 16, gt_bytes, dmin, dmax, None, 0,
                                       workspace.data_ptr(), 0, sums.data_ptr(), meas.data_ptr(), conf.data_ptr(), running.data_ptr(),
                                       confusion.data_ptr(), stream)

    assert raw_call(mm.data_ptr(), 1, MIN_D, MAX_D) == -2 and raw_call(mm.data_ptr(), 8, MIN_D, MAX_D) == -2
    assert raw_call(mm.data_ptr(), 4, 10.0, 10.0) == -1 and raw_call(mm.data_ptr(), 4, float("nan"), 10.0) == -1
    assert raw_call(mm.data_ptr() + 2, 4, MIN_D, MAX_D) == -3 and raw_call(mm.data_ptr() + 1, 2, MIN_D, MAX_D) == -3
    assert raw_call(None, 4, MIN_D, MAX_D) == -1
    torch.cuda.synchronize()
    assert (sums == SENT).all() and (meas == SENT).all() and (conf == int(SENT)).all() and not running.any() and not confusion.any()
    assert raw_call(mm.data_ptr(), 4, MIN_D, MAX_D) == 0                            # ... and the same call with good arguments runs
    torch.cuda.synchronize()
    assert not (sums == SENT).any() and int(conf.sum()) == 8 * 16


# ------------------------------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def dataset_dir(tmp_path_factory):
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_synth_dataset", os.path.join(ROOT, "tools", "make_synth_dataset.py"))
    synth = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(synth)
    d = str(tmp_path_factory.mktemp("synth_frame_eval"))
    synth.write_dataset(d, 4, [(96, 128), (90, 120)], seed=0)
    return d


def test_evaluate_frames_end_to_end(dataset_dir):
    """Four synthetic samples (96 x 128 and 90 x 120) through evaluate_frames with det_fill_ weights, ensemble off and on, from a
    device-resident store (record_gt), a pinned store and a stream, under set_sync_debug_mode("error") around every update:
    tests/frame_eval_child.py, a fresh process because the decode pool starts before the GPU is initialised."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "frame_eval_child.py"), dataset_dir], timeout=600,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout[-6000:])
    assert r.returncode == 0, "tests/frame_eval_child.py ended with status %d:\n%s" % (r.returncode, r.stdout[-3000:])
    assert r.stdout.rstrip().endswith("ok")
