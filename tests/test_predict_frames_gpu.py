"""GPU: InferenceSession.predict_frames - uint8 frames in, results at frame size out - against the same steps done by hand: the
frames through DeviceAugment.apply_batch + device_collate, that batch through the session (the raw outputs of the very graph
predict_frames replays), tests/frames_ref.py on those raw outputs, ops.line_postprocess for the lines.

Allowed difference.  The two routes replay one graph on bit-equal inputs, so bit equality is the expectation; what is allowed is
the kernel's bound (tests/test_frames_post_gpu.py: K 2^-24 max_depth on the depth, the margin rule on the labels) plus the
session's own reproducibility bar as tests/test_infer_session.py::bar_for measures it (a relative norm: it is turned into an
absolute figure with the largest value it can apply to - max_depth for the depth, the largest |logit| for the margins, the frame
diagonal for lines in pixels).  Every measured figure is printed before it is asserted."""
import pytest
import torch

from gw_depth_amd import data, hip, ops
from gw_depth_amd.infer import RESULT_KEYS, InferenceSession
from gw_depth_amd.model import NestedTensor
from tests import frames_ref as R
from tests.golden_check import build
from tests.test_infer_session import bar_for, captured, plain, sync_debug_mode_works

pytestmark = pytest.mark.gpu
SIZE, MAX_SIZE = 96, 128
MIN_D, MAX_D, THRESH = 1e-3, 10.0, 0.6
SHAPES = [(72, 110), (100, 60)]          # network sizes (84, 128) and (128, 77): they differ in height and in width
_S = {}


def frames_of(seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, generator=g) for h, w in SHAPES]


@pytest.fixture()
def state():
    """One model, one graph session and one measured bar for the whole module."""
    hip.set_library(None)
    if not _S:
        cfg, model, crits = build(device="cuda")
        _S["model"] = model
        _S["sess"] = InferenceSession(model, compute_dtype=torch.bfloat16, graph=True, min_depth=MIN_D, max_depth=MAX_D, score_thresh=THRESH)
        batch = by_hand(frames_of(11), False)
        img, msk = batch["images"], batch["pad_mask"]
        _S["bar"] = bar_for(model, torch.bfloat16, img, msk, plain(model, torch.bfloat16, img, msk))
    return _S


def by_hand(frames, ensemble):
    aug = data.DeviceAugment(train=False, test_size=SIZE, max_size=MAX_SIZE)
    dev_frames = [f.cuda() for f in frames]
    params = [aug.params(f.shape[1], f.shape[0]) for f in frames]
    if ensemble:
        dev_frames, params = dev_frames * 2, params + [dict(p, flip="h") for p in params]
    out = data.DeviceAugment.apply_batch([(f, None, None) for f in dev_frames], [torch.zeros((0, 4))] * len(dev_frames), params)
    return data.device_collate([o[:3] for o in out], device="cuda", dtype=torch.bfloat16)


def expected(sess, frames, ensemble):
    batch = by_hand(frames, ensemble)
    raw = sess(NestedTensor(batch["images"], batch["pad_mask"]))
    torch.cuda.synchronize()
    B = len(frames)
    fs = [tuple(f.shape[:2]) for f in frames]
    ns = [data.resized_shape(w, h, SIZE, MAX_SIZE) for h, w in fs]
    assert len({n[0] for n in ns}) == B and len({n[1] for n in ns}) == B
    depth, seg = raw["pred_depth"][-1].float().cpu(), raw["pred_seg"].float().cpu()
    out_hw = (max(s[0] for s in fs), max(s[1] for s in fs))
    d, mm, lab, margin = R.dense_resized(depth, seg, ns, fs, out_hw, MIN_D, MAX_D, twin=B if ensemble else 0)
    fsz = torch.tensor(fs * (2 if ensemble else 1), dtype=torch.int32, device="cuda")
    scores, lines, order, count = (t[:B].clone() for t in ops.line_postprocess(raw["pred_logits"], raw["pred_lines"], fsz, THRESH))
    top = max(float(seg[i, :, :ns[i % B][0], :ns[i % B][1]].abs().max()) for i in range(seg.shape[0]))
    return {"depth": d, "label": lab, "margin": margin, "top": top, "scores": scores, "lines": lines, "order": order, "count": count,
            "sizes": fs, "net_sizes": ns, "out_hw": out_hw}


def check(res, want, bar, ensemble):
    B = len(want["sizes"])
    assert sorted(res) == sorted(RESULT_KEYS + ("net_sizes",))
    assert res["sizes"].tolist() == [list(s) for s in want["sizes"]] and res["net_sizes"].tolist() == [list(s) for s in want["net_sizes"]]
    assert res["depth"].shape == (B, *want["out_hw"]) and res["depth_mm"].dtype == torch.uint16 and res["labels"].dtype == torch.uint8
    got_d, got_lab = res["depth"].cpu(), res["labels"].cpu().to(torch.int64)
    err, allowed = float((got_d.double() - want["depth"]).abs().max()), R.K * R.U * MAX_D + bar * MAX_D
    print("depth: largest difference %.3e (allowed %.3e)" % (err, allowed))
    assert err <= allowed
    assert torch.equal(res["depth_mm"].cpu().to(torch.int64), torch.round(got_d * 1000.0).clamp(max=65535.0).to(torch.int64))
    inside = want["label"] != 255
    tol = (2 * R.K * R.U + 2 * bar) * want["top"] * (2 if ensemble else 1)
    decided = inside & (want["margin"] > tol)
    print("labels: %d of %d pixels excused (margin <= %.2e)" % (int((inside & ~decided).sum()), int(inside.sum()), tol))
    assert int((inside & ~decided).sum()) <= 0.01 * int(inside.sum())
    assert torch.equal(got_lab[decided], want["label"][decided]) and bool((got_lab[~inside] == 255).all()) and bool((got_d[~inside] == 0).all())
    diag = max((h * h + w * w) ** 0.5 for h, w in want["sizes"])
    d_scores, d_lines = float((res["scores"] - want["scores"]).abs().max()), float((res["lines"] - want["lines"]).abs().max())
    print("scores: %.3e (allowed %.3e)  lines: %.3e px (allowed %.3e)" % (d_scores, bar, d_lines, bar * diag))
    assert res["scores"].shape == want["scores"].shape and d_scores <= bar and d_lines <= bar * diag
    assert res["order"].shape == want["order"].shape and res["count"].shape == (B,)
    if d_scores == 0:
        assert torch.equal(res["order"], want["order"]) and torch.equal(res["count"], want["count"])


@pytest.mark.parametrize("ensemble", [False, True], ids=["plain", "ensemble"])
def test_predict_frames_equals_the_steps_by_hand(state, ensemble):
    sess, bar = state["sess"], state["bar"]
    frames = frames_of(11)
    res = sess.predict_frames(frames, size=SIZE, max_size=MAX_SIZE, ensemble=ensemble, copy=True)
    torch.cuda.synchronize()
    assert captured(sess), "capture was refused"
    want = expected(sess, frames, ensemble)
    check(res, want, bar, ensemble)
    # frames already on the device give the same results
    dev = sess.predict_frames([f.cuda() for f in frames], size=SIZE, max_size=MAX_SIZE, ensemble=ensemble, copy=True)
    torch.cuda.synchronize()
    check(dev, want, bar, ensemble)
    assert torch.equal(dev["sizes"], res["sizes"]) and torch.equal(dev["net_sizes"], res["net_sizes"])


def test_replay_fresh_dense_results_copy_and_no_host_sync(state):
    sess, bar = state["sess"], state["bar"]
    first_frames, other_frames = frames_of(11), frames_of(12)
    first = sess.predict_frames(first_frames, size=SIZE, max_size=MAX_SIZE)
    kept = sess.predict_frames(first_frames, size=SIZE, max_size=MAX_SIZE, copy=True)
    torch.cuda.synchronize()
    n_graphs = len(sess._graphs)
    snap = {k: v.clone() for k, v in first.items()}
    second = sess.predict_frames(other_frames, size=SIZE, max_size=MAX_SIZE, copy=True)     # other frames, the same sizes: a replay
    torch.cuda.synchronize()
    assert len(sess._graphs) == n_graphs and captured(sess), "capture was refused"
    check(second, expected(sess, other_frames, False), bar, False)
    # the dense results (and the sizes) of the first call are fresh tensors: the second call did not touch them
    for k in ("depth", "depth_mm", "labels", "sizes", "net_sizes"):
        assert first[k].data_ptr() != second[k].data_ptr() and torch.equal(first[k].view(torch.uint8), snap[k].view(torch.uint8)), k
    assert not torch.equal(first["depth"], second["depth"])
    # the line results are the graph's static tensors unless copy=True: the next call writes through the views of the first
    third = sess.predict_frames(other_frames, size=SIZE, max_size=MAX_SIZE)
    torch.cuda.synchronize()
    assert first["lines"].data_ptr() == third["lines"].data_ptr() and torch.equal(first["lines"], third["lines"])
    for k in ("scores", "lines", "order", "count"):
        assert kept[k].data_ptr() != third[k].data_ptr() and second[k].data_ptr() != third[k].data_ptr() and torch.equal(kept[k], snap[k]), k
    # no host sync in a warmed call: host frames (pinned, non-blocking), device frames, and the ensemble
    sess.predict_frames(first_frames, size=SIZE, max_size=MAX_SIZE, ensemble=True)
    dev_frames = [f.cuda() for f in first_frames]
    torch.cuda.synchronize()

    def calls():
        sess.predict_frames(first_frames, size=SIZE, max_size=MAX_SIZE)
        sess.predict_frames(dev_frames, size=SIZE, max_size=MAX_SIZE, copy=True)
        return sess.predict_frames(dev_frames, size=SIZE, max_size=MAX_SIZE, ensemble=True)

    if sync_debug_mode_works():
        torch.cuda.set_sync_debug_mode("error")
        try:
            calls()
        finally:
            torch.cuda.set_sync_debug_mode("default")
    else:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            calls()
        names = [e.name for e in prof.events()]
        assert not any("StreamSynchronize" in n or "DtoH" in n or "EventSynchronize" in n for n in names), sorted(set(names))
    torch.cuda.synchronize()


def test_predict_and_call_are_unchanged_by_the_new_path(state):
    """The same batch through predict() and __call__ of the session that served predict_frames and of a session that never did."""
    sess, bar, model = state["sess"], state["bar"], state["model"]
    sess.predict_frames(frames_of(11), size=SIZE, max_size=MAX_SIZE)
    batch = by_hand(frames_of(11), False)
    nt = NestedTensor(batch["images"], batch["pad_mask"])
    fresh = InferenceSession(model, compute_dtype=torch.bfloat16, graph=True, min_depth=MIN_D, max_depth=MAX_D, score_thresh=THRESH)
    a, b = fresh.predict(nt, copy=True), sess.predict(nt, copy=True)
    ra, rb = fresh(nt)["pred_depth"][-1].float().clone(), sess(nt)["pred_depth"][-1].float().clone()
    torch.cuda.synchronize()
    assert sorted(a) == sorted(b) == sorted(RESULT_KEYS) and captured(fresh) and captured(sess)
    assert torch.equal(a["sizes"], b["sizes"]) and a["depth"].shape == b["depth"].shape == (2, 128, 128)
    d = max(float((a["depth"] - b["depth"]).abs().max()) / MAX_D, float((ra - rb).abs().max()) / max(float(ra.abs().max()), 1e-12),
            float((a["scores"] - b["scores"]).abs().max()))
    print("predict / __call__, fresh session against the one that ran predict_frames: %.3e (bar %.1e)" % (d, bar))
    assert d <= bar
