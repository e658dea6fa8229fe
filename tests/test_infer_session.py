"""GPU: infer.InferenceSession - frozen weight copies, graph replay, device post-processing - against the plain
`model.eval(); model(NestedTensor(...))` forward on the same weights and inputs.

Bars.  fp32: 2e-5 by rel(), the bar of test_hip_graph_step_equals_eager_step ("same kernels, another launch route").  bf16: the
test measures how reproducible the plain bf16 forward is (`spread` = the largest rel() between two plain forwards of the same
input) and allows max(4 * spread, 2e-5): four times because one pair samples the spread poorly, 2e-5 as the floor.  Bit equality
is the expectation; every measured figure is printed before it is asserted."""
import warnings

import pytest
import torch

from gw_depth_amd import graphs, hip
from gw_depth_amd.infer import RESULT_KEYS, InferenceSession
from gw_depth_amd.model import NestedTensor
from gw_depth_amd.synth import synth_batch
from tests.golden_check import build, rel, to_device

pytestmark = pytest.mark.gpu
FP32_BAR = 2e-5
_MODEL = {}


@pytest.fixture()
def built():
    """One model for the tests that leave its weights alone."""
    hip.set_library(None)
    if not _MODEL:
        _MODEL["m"] = build(device="cuda")
    return _MODEL["m"]


def flatten(out):
    flat = {"pred_logits": out["pred_logits"], "pred_lines": out["pred_lines"], "pred_seg": out["pred_seg"]}
    for i, d in enumerate(out["pred_depth"]):
        flat["pred_depth_%d" % i] = d
    for i, a in enumerate(out.get("aux_outputs", [])):
        flat["aux%d_logits" % i], flat["aux%d_lines" % i] = a["pred_logits"], a["pred_lines"]
    return {k: v.detach().float().clone() for k, v in flat.items()}


def plain(model, dtype, img, msk):
    """The parent's inference path."""
    model.compute_dtype = dtype
    model.eval()
    with torch.no_grad():
        out = flatten(model(NestedTensor(img, msk)))
    torch.cuda.synchronize()
    return out


def worst(a, b):
    assert sorted(a) == sorted(b)
    return max(rel(a[k], b[k]) for k in b)


def bar_for(model, dtype, img, msk, ref):
    if dtype == torch.float32:
        return FP32_BAR
    spread = worst(plain(model, dtype, img, msk), ref)
    print("plain bf16 forward, run-to-run spread %.3e" % spread)
    assert spread <= 1e-3, "the plain bf16 forward is not reproducible on this input: a finding, pick another seed"
    return max(4 * spread, 2e-5)


def inputs(B, H, W, seed, sizes=None):
    b = synth_batch(B, H, W, seed=seed, sizes=sizes)
    return b["images"].cuda(), b["pad_mask"].cuda()


def captured(sess):
    return sess._graphs and all(e["graph"] is not None for e in sess._graphs.values())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", [(2, 96, 128), (1, 480, 640)])
def test_session_equals_plain_forward(built, shape, dtype):
    cfg, model, crits = built
    img, msk = inputs(*shape, seed=71)
    ref = plain(model, dtype, img, msk)
    bar = bar_for(model, dtype, img, msk, ref)
    eager = InferenceSession(model, compute_dtype=dtype, graph=False)
    for call in range(2):
        d = worst(flatten(eager(NestedTensor(img, msk))), ref)
        print("eager session call %d: %.3e (bar %.1e)" % (call, d, bar))
        assert d <= bar
    graph = InferenceSession(model, compute_dtype=dtype, graph=True)
    for call in range(3):                                              # the capturing call and two replays
        d = worst(flatten(graph(NestedTensor(img, msk))), ref)
        print("graph session call %d: %.3e (bar %.1e)" % (call, d, bar))
        assert d <= bar
    assert captured(graph), "capture was refused"
    assert model.compute_dtype == dtype and graph.eval() is graph
    with pytest.raises(RuntimeError):
        graph.train()


def test_replay_hygiene_second_shape_and_eviction(built, monkeypatch):
    cfg, model, crits = built
    dtype = torch.bfloat16
    eager = InferenceSession(model, compute_dtype=dtype, graph=False)
    graph = InferenceSession(model, compute_dtype=dtype, graph=True)
    img0, msk0 = inputs(2, 96, 128, seed=81)
    bar = bar_for(model, dtype, img0, msk0, plain(model, dtype, img0, msk0))
    for seed in (81, 82, 83):                                          # three images through one signature
        img, msk = inputs(2, 96, 128, seed=seed)
        d = worst(flatten(graph(NestedTensor(img, msk))), flatten(eager(NestedTensor(img, msk))))
        print("seed %d: replay vs eager session %.3e" % (seed, d))
        assert d <= bar
    assert list(graph.graphs) == [(2, 96, 128)] and captured(graph), "capture was refused"
    img1, msk1 = inputs(1, 96, 128, seed=84)                           # a second shape gets a second graph
    assert worst(flatten(graph(img1)), flatten(eager(img1))) <= bar
    assert list(graph.graphs) == [(2, 96, 128), (1, 96, 128)] and captured(graph), "capture was refused"
    first = graph._graphs[(2, 96, 128)]["graph"]
    assert worst(flatten(graph(NestedTensor(img0, msk0))), flatten(eager(NestedTensor(img0, msk0)))) <= bar
    assert graph._graphs[(2, 96, 128)]["graph"] is first                # going back replays the first
    assert list(graph.graphs) == [(1, 96, 128), (2, 96, 128)]
    monkeypatch.setattr(graphs, "MAX_GRAPHS", 2)                       # the bound, made small: a third signature evicts the oldest
    img2, msk2 = inputs(3, 96, 128, seed=85)
    assert worst(flatten(graph(NestedTensor(img2, msk2))), flatten(eager(NestedTensor(img2, msk2)))) <= bar
    assert list(graph.graphs) == [(2, 96, 128), (3, 96, 128)] and captured(graph), "capture was refused"
    assert worst(flatten(graph(img1)), flatten(eager(img1))) <= bar    # evicted: captured again, right results
    assert list(graph.graphs) == [(3, 96, 128), (1, 96, 128)] and captured(graph), "capture was refused"


def test_capture_refused_when_a_memset_is_seen(built, monkeypatch):
    cfg, model, crits = built
    img, msk = inputs(2, 96, 128, seed=91)
    ref = plain(model, torch.float32, img, msk)
    sess = InferenceSession(model, compute_dtype=torch.float32, graph=True)
    monkeypatch.setattr(sess, "_count_memsets", lambda st: (sess._pass(st), 3)[1])
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        out = flatten(sess(NestedTensor(img, msk)))
        again = flatten(sess(NestedTensor(img, msk)))
    assert any("capture refused" in str(x.message) for x in w)
    assert all(e["graph"] is None for e in sess._graphs.values()) and not sess.graphs[(2, 96, 128)]["captured"]
    assert worst(out, ref) <= FP32_BAR and worst(again, ref) <= FP32_BAR


def kernels_named(fn, part):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if part in e.name)


def test_frozen_weights_and_refresh_after_a_train_step():
    from gw_depth_amd.engine import TrainStep
    hip.set_library(None)
    cfg, model, crits = build(device="cuda")
    dtype = torch.bfloat16
    img, msk = inputs(2, 96, 128, seed=95)
    model.compute_dtype = dtype
    model.eval()

    def plain_call():
        with torch.no_grad():
            model(NestedTensor(img, msk))
    n_plain = kernels_named(plain_call, "weight_prep")
    first = InferenceSession(model, compute_dtype=dtype, graph=False)
    first(NestedTensor(img, msk))
    n_sess = kernels_named(lambda: first(NestedTensor(img, msk)), "weight_prep")
    print("weight_prep launches: plain forward %d, second call of the session %d" % (n_plain, n_sess))
    assert n_plain >= 1 and n_sess == 0

    step = TrainStep(model, crits, cfg, compute_dtype=dtype)           # moves every parameter into its flat buffer
    with pytest.raises(RuntimeError, match="moved"):
        first.refresh()
    eager = InferenceSession(model, compute_dtype=dtype, graph=False)  # built AFTER the TrainStep
    graph = InferenceSession(model, compute_dtype=dtype, graph=True)
    before = flatten(eager(NestedTensor(img, msk)))
    assert worst(flatten(graph(NestedTensor(img, msk))), before) <= 2e-5 and captured(graph), "capture was refused"
    b = to_device(synth_batch(2, 96, 128, seed=96), "cuda")
    step(b)
    torch.cuda.synchronize()
    stale = worst(flatten(eager(NestedTensor(img, msk))), before)
    print("after the step, before refresh(): %.3e from the old result (biases and norms are read in place, weight copies are frozen)" % stale)
    eager.refresh()
    graph.refresh()
    ref = plain(model, dtype, img, msk)                                # the updated weights, through the optimizer's bf16 shadow
    bar = bar_for(model, dtype, img, msk, ref)
    moved = worst(before, ref)
    print("the step moved the outputs by %.3e" % moved)
    assert moved > bar
    for name, sess in (("eager", eager), ("graph", graph)):
        d = worst(flatten(sess(NestedTensor(img, msk))), ref)
        print("%s session after refresh(): %.3e (bar %.1e)" % (name, d, bar))
        assert d <= bar
    assert len(graph._graphs) == 1 and captured(graph)                 # still the graph captured BEFORE the step


def torch_post(raw, sizes, min_d, max_d, thresh):
    d = raw["pred_depth"][-1].float()
    B, _, H, W = d.shape
    d = d.reshape(B, H, W)
    ys, xs = torch.arange(H, device=d.device)[None, :, None], torch.arange(W, device=d.device)[None, None, :]
    inside = (ys < sizes[:, 0, None, None]) & (xs < sizes[:, 1, None, None])
    depth = torch.where(torch.isnan(d), torch.full_like(d, min_d), d.clamp(min_d, max_d))
    mm = torch.round(depth * 1000.0).clamp(max=65535.0)
    lab = raw["pred_seg"].float().argmax(1)
    zero = torch.zeros_like(depth)
    scores = torch.softmax(raw["pred_logits"].float(), -1)[..., 0]
    h, w = sizes[:, 0].float(), sizes[:, 1].float()
    lines = raw["pred_lines"].float()[..., :4] * torch.stack([w, h, w, h], 1)[:, None, :]
    return {"depth": torch.where(inside, depth, zero), "depth_mm": torch.where(inside, mm, zero).to(torch.int32),
            "labels": torch.where(inside, lab, torch.full_like(lab, 255)).to(torch.int32), "scores": scores, "lines": lines,
            "inside": inside}


def sync_debug_mode_works():
    torch.cuda.set_sync_debug_mode("error")
    try:
        torch.ones(2, device="cuda").sum().item()
        return False
    except RuntimeError:
        return True
    finally:
        torch.cuda.set_sync_debug_mode("default")


def test_predict_ragged_batch(built):
    cfg, model, crits = built
    b = synth_batch(2, 96, 128, seed=101, sizes=[(96, 128), (80, 104)])
    ragged = [b["images"][0].cuda(), b["images"][1, :, :80, :104].contiguous().cuda()]     # two image sizes, padded by the session
    sess = InferenceSession(model, compute_dtype=torch.bfloat16, graph=True, min_depth=1e-3, max_depth=10.0, score_thresh=0.6)
    res = sess.predict(ragged)
    assert sorted(res) == sorted(RESULT_KEYS)
    res = {k: v.clone() for k, v in res.items()}
    raw = sess(ragged)                                                 # the same graph, the same static raw outputs
    assert captured(sess), "capture was refused"
    sizes = torch.tensor([[96, 128], [80, 104]], dtype=torch.int32, device="cuda")
    assert res["sizes"].dtype == torch.int32 and torch.equal(res["sizes"], sizes)
    want = torch_post(raw, sizes, 1e-3, 10.0, 0.6)
    assert torch.equal(res["depth"], want["depth"])
    assert res["depth_mm"].dtype == torch.uint16 and torch.equal(res["depth_mm"].to(torch.int32), want["depth_mm"])
    assert res["labels"].dtype == torch.uint8 and torch.equal(res["labels"].to(torch.int32), want["labels"])
    pad = ~want["inside"]
    assert bool(pad[1].any()) and not bool(pad[0].any())
    assert bool((res["depth"][pad] == 0).all()) and bool((res["labels"][pad] == 255).all()) and bool((res["depth_mm"].to(torch.int32)[pad] == 0).all())
    assert float((res["scores"] - want["scores"]).abs().max()) <= 2e-5
    assert torch.equal(res["lines"], want["lines"])
    assert torch.equal(res["order"].long(), torch.argsort(res["scores"], dim=-1, descending=True, stable=True))
    assert torch.equal(res["count"].long(), (res["scores"] > 0.6).sum(-1))
    # target_sizes: the lines in another frame, everything else as before
    tgt = torch.tensor([[480, 640], [400, 520]])
    scaled = sess.predict(ragged, target_sizes=tgt, copy=True)
    tw = torch_post(raw, tgt.cuda().int(), 1e-3, 10.0, 0.6)
    assert torch.equal(scaled["lines"], tw["lines"]) and torch.equal(scaled["depth"], res["depth"]) and torch.equal(scaled["sizes"], sizes)
    # lifetime: copy=True survives the next call, copy=False is the graph's static memory
    other = [t.flip(-1).contiguous() for t in ragged]
    kept = sess.predict(ragged, copy=True)
    live = sess.predict(ragged)
    assert torch.equal(kept["depth"], res["depth"]) and torch.equal(live["depth"], res["depth"])
    new = sess.predict(other)
    assert torch.equal(kept["depth"], res["depth"]) and torch.equal(kept["lines"], res["lines"])
    assert new["depth"] is live["depth"] and not torch.equal(live["depth"], res["depth"])
    # no host sync inside a replayed predict
    torch.cuda.synchronize()
    if sync_debug_mode_works():
        torch.cuda.set_sync_debug_mode("error")
        try:
            sess.predict(ragged)
            sess(ragged)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    else:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            sess.predict(ragged)
        names = [e.name for e in prof.events()]
        assert not any("StreamSynchronize" in n or "DtoH" in n or "EventSynchronize" in n for n in names), sorted(set(names))
    torch.cuda.synchronize()
    assert torch.equal(sess.predict(ragged)["depth"], res["depth"])


def test_evaluate_accepts_a_session(built):
    from gw_depth_amd.evaluate import evaluate
    cfg, model, crits = built
    dtype = torch.bfloat16
    loader = []
    for seed, sizes in ((111, [(96, 128), (80, 104)]), (112, None), (113, [(64, 128), (96, 96)])):
        b = synth_batch(2, 96, 128, seed=seed, n_lines=[3, 4], sizes=sizes)
        loader.append((NestedTensor(b["images"], b["pad_mask"]), NestedTensor(b["depth"], b["pad_mask"]),
                       NestedTensor(b["seg"], b["pad_mask"]), b["targets"], ["synthetic\n"]))
    args = type("A", (), {"with_line": True, "with_dense": True, "min_depth_eval": 1e-3, "max_depth_eval": 10.0})()
    img, msk = loader[0][0].tensors.cuda(), loader[0][0].mask.cuda()
    bar = bar_for(model, dtype, img, msk, plain(model, dtype, img, msk))
    model.compute_dtype = dtype
    want = evaluate(model, crits, None, loader, None, "cuda", None, args)
    sess = InferenceSession(model, compute_dtype=dtype, graph=True)
    got = evaluate(sess, crits, None, loader, None, "cuda", None, args)
    assert captured(sess), "capture was refused"
    assert sorted(got) == sorted(want) and {"silog", "rms", "d1", "Mean IU", "loss"} <= set(got)
    for k in want:
        print("%-24s module %.9g session %.9g" % (k, want[k], got[k]))
        assert abs(got[k] - want[k]) <= bar * max(1.0, abs(want[k])), k


def test_c5_predict_960x1280_batch32_bf16_graph(built):
    """The design of test_c5_inference_960x1280_batch32_bf16 (images 0..3 repeated: every image bit-equal to its twin, finite,
    depth within [0, 10]) through predict() of a graph session."""
    cfg, model, crits = built
    B = 32
    b = synth_batch(4, 960, 1280, seed=53)
    img = b["images"].cuda().repeat(B // 4, 1, 1, 1)
    msk = b["pad_mask"].cuda().repeat(B // 4, 1, 1)
    sess = InferenceSession(model, compute_dtype=torch.bfloat16, graph=True)
    res = sess.predict(NestedTensor(img, msk))
    torch.cuda.synchronize()
    assert captured(sess), "capture was refused"
    assert res["depth"].shape == (B, 960, 1280) and res["depth_mm"].shape == (B, 960, 1280) and res["labels"].shape == (B, 960, 1280)
    assert bool(torch.isfinite(res["depth"]).all()) and bool(torch.isfinite(res["scores"]).all()) and bool(torch.isfinite(res["lines"]).all())
    assert float(res["depth"].min()) >= 0.0 and float(res["depth"].max()) <= 10.0
    assert int(res["labels"].max()) <= 1 and torch.equal(res["sizes"], torch.tensor([[960, 1280]] * B, dtype=torch.int32, device="cuda"))
    for k in ("depth", "depth_mm", "labels", "scores", "lines", "order", "count"):
        v = res[k].to(torch.int32) if res[k].dtype == torch.uint16 else res[k]
        for i in range(4, B):
            assert torch.equal(v[i], v[i % 4]), (k, i)
