"""The end-to-end half of tests/test_frame_metrics_gpu.py, run as a fresh process: the decode pool has to start before this process
initialises the GPU.  usage: python tests/frame_eval_child.py DATASET_DIR   (exit status 0 = every check held)

Four synthetic samples go through evaluate_frames (det_fill_ weights, fp32, no graph) with the ensemble off and on.  What it returns
is compared with the same frames pushed through predict_frames(copy=True) and scored on the host by tests/frame_metrics_ref.py from
arrays this script decodes itself: integer sums and confusion exact, the other raw sums inside N * 2^-52 * sum |term|, the closing
dictionary from the kernel's own records bit for bit."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np

from gw_depth_amd import decode
from tests.dataset_child import decode_directly, index_of, live_children

EDGES = (0.0, 1.0, 2.0, 4.0, 10.0)
SIZE, MAX_SIZE = 96, 128


def main(root):
    index = index_of(root)
    pool = decode.DecodePool(index, workers=2)
    import torch
    from gw_depth_amd import dataset, hip
    from gw_depth_amd.evaluate import METRIC_NAMES, FrameMetrics, evaluate_frames
    from gw_depth_amd.infer import InferenceSession
    from tests import frame_metrics_ref as F
    from tests.golden_check import build
    assert not torch.cuda.is_initialized(), "the pool must be up before the GPU is"
    assert not getattr(hip.library(), "is_fake", False)
    direct = decode_directly(index)
    n = len(index)
    assert n == 4 and {d[0].shape[:2] for d in direct} == {(96, 128), (90, 120)}
    _, model, _ = build(device="cuda")
    sess = InferenceSession(model, compute_dtype=torch.float32, graph=False)
    sources = {"store-device": dataset.FrameStore.build(index, pool, device="cuda", where="device"),
               "store-pinned": dataset.FrameStore.build(index, pool, device="cuda", where="pinned"),
               "stream": dataset.StreamSource(index, pool, device="cuda")}
    gt16 = sources["store-device"].record_gt(range(n))
    for i, (dmm, lab) in enumerate(gt16):                   # record_gt: views of the arena holding the decoded planes
        assert dmm.dtype == torch.uint16 and lab.dtype == torch.uint8 and dmm.untyped_storage().data_ptr() == sources["store-device"].arena.untyped_storage().data_ptr()
        assert np.array_equal(dmm.cpu().numpy().astype(np.int32), direct[i][1]) and np.array_equal(lab.cpu().numpy(), direct[i][2])

    # every update runs with host syncs forbidden
    plain_update = FrameMetrics.update

    def strict_update(self, *a, **k):
        torch.cuda.set_sync_debug_mode("error")
        try:
            return plain_update(self, *a, **k)
        finally:
            torch.cuda.set_sync_debug_mode("default")

    FrameMetrics.update = strict_update
    for ensemble in (False, True):
        # the host's own scoring of predict_frames(copy=True) on the directly decoded ground truth
        want = []
        for at in range(0, n, 2):
            frames = [torch.from_numpy(direct[i][0].copy()).cuda() for i in range(at, at + 2)]
            res = sess.predict_frames(frames, size=SIZE, max_size=MAX_SIZE, ensemble=ensemble, copy=True)
            depth, labels = res["depth"].cpu().numpy(), res["labels"].cpu().numpy()
            for k, i in enumerate(range(at, at + 2)):
                h, w = direct[i][1].shape
                want.append(F.score_frame(depth[k, :h, :w], labels[k, :h, :w], direct[i][1], direct[i][2], sess.min_depth, sess.max_depth, EDGES))
        results = {}
        for name, source in sources.items():
            fm = FrameMetrics("cuda", sess.min_depth, sess.max_depth, depth_bins=EDGES, capacity_images=n)
            out = evaluate_frames(sess, source, batch=2, ensemble=ensemble, size=SIZE, max_size=MAX_SIZE, depth_bins=EDGES, metrics=fm)
            rec = fm.per_image()
            assert rec["ids"].tolist() == list(range(n)) and out["names"] == {i: index.name(i) for i in range(n)}
            for i in range(n):
                ref = want[i]
                np.testing.assert_array_equal(rec["sums"][i][:, :4], ref["sums"][:, :4], err_msg="%s image %d" % (name, i))
                np.testing.assert_array_equal(rec["confusion"][i], ref["conf"])
                bound = F.sum_bound(ref["sums"][:, :1], ref["abs_sums"][:, 4:])
                err = np.abs(rec["sums"][i][:, 4:] - ref["sums"][:, 4:])
                print("ensemble=%s %s image %d: valid pixels %d, glass %d, max |sum - fsum| / bound %.3g"
                      % (ensemble, name, i, ref["sums"][0, 0], ref["sums"][1, 0], float((err / np.maximum(bound, 1e-300)).max())))
                assert (err <= bound).all(), (name, i, err, bound)
                np.testing.assert_allclose(rec["measures"][i], F.measures_from_sums(rec["sums"][i]), rtol=1e-12, atol=0, equal_nan=True)
            run, conf = F.running_fold(rec["sums"], rec["measures"], rec["confusion"])
            np.testing.assert_array_equal(fm.running.cpu().numpy(), run)               # the device's totals: the same adds in the same order
            np.testing.assert_array_equal(fm.confusion.cpu().numpy(), conf)
            closed = F.closing(run, conf, rec["sums"])
            for k, v in closed.items():
                assert out[k] == v or (k != "n_images" and abs(out[k] - v) <= 1e-12 * abs(v)), (name, k, out[k], v)
            assert set(out) == set(closed) | {"names"}
            assert all(m in out and np.isfinite(out[m]) for m in METRIC_NAMES) and "Mean IU" in out and out["n_images"]["all"] == n
            worst = fm.worst(2)
            assert len(worst) == 2 and worst[0][1] >= worst[1][1] and worst[0][1] == np.nanmax(rec["measures"][:, 0, 3])
            results[name] = rec
        for name in ("store-pinned", "stream"):                                         # the 16-bit planes in place == the widened int32 planes
            for k in ("sums", "measures", "confusion"):
                assert results[name][k].tobytes() == results["store-device"][k].tobytes(), (name, k)
        print("ensemble=%s: %s" % (ensemble, {k: out[k] for k in ("rms", "glass/rms", "nonglass/rms", "Mean IU", "n_images")}))
    FrameMetrics.update = plain_update
    torch.cuda.synchronize()
    pool.close()
    assert live_children() == [], live_children()


if __name__ == "__main__":
    main(sys.argv[1])
    print("ok")
