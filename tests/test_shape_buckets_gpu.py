"""Shape buckets on the device: device_collate(pad_to=...) is the unpadded collate plus more of the same padding, a stream of
distinct raw batch shapes collated to buckets replays a handful of captured steps where the raw stream captures every batch, a
bucketed batch steps through its graph as it does eagerly, and capture_after defers the capture.  fp32, B = 2."""
import pytest
import torch

from gw_depth_amd import hip
from gw_depth_amd.data import bucket_shape, device_collate
from tests.golden_check import build, rel, to_device

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def real_library():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    hip.set_library(None)
    assert not getattr(hip.library(), "is_fake", False)
    yield


def _frames():
    g = torch.Generator().manual_seed(7)
    out = []
    for h, w in ((90, 120), (70, 101)):
        out.append((torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8), torch.randint(0, 9000, (h, w), generator=g, dtype=torch.int32),
                    torch.randint(0, 2, (h, w), generator=g, dtype=torch.uint8)))
    return out


def test_collate_pad_to_is_the_unpadded_collate_plus_padding():
    frames = _frames()
    raw = device_collate(frames)
    got = device_collate(frames, pad_to=32)
    torch.cuda.synchronize()
    assert tuple(raw["images"].shape) == (2, 3, 90, 120) and tuple(got["images"].shape) == (2, 3, 96, 128)
    assert tuple(got["pad_mask"].shape) == (2, 96, 128) and tuple(got["depth"].shape) == (2, 1, 96, 128) and tuple(got["seg"].shape) == (2, 1, 96, 128)
    for key, fill in (("images", 0.0), ("pad_mask", True), ("depth", 0.0), ("seg", 0)):
        want = torch.full(got[key].shape, fill, dtype=raw[key].dtype, device="cuda")
        want[..., :90, :120] = raw[key]
        assert torch.equal(got[key], want), key
    same = device_collate(frames, pad_to=(96, 128))                   # an explicit size
    assert all(torch.equal(same[k], got[k]) for k in got)
    with pytest.raises(ValueError):
        device_collate(frames, pad_to=(96, 119))


# item sizes of six batches: six distinct raw (H, W), four inside the bucket 96 x 128 and two inside 128 x 160 (step 32)
STREAM = [((88, 120), (72, 104)), ((96, 128), (80, 96)), ((80, 112), (72, 96)), ((72, 104), (64, 128)),
          ((104, 152), (128, 136)), ((112, 160), (104, 136))]


def _run_stream(bucketed):
    from gw_depth_amd.engine import TrainStep
    from gw_depth_amd.synth import synth_batch
    cfg, model, crits = build(device="cuda")
    step = TrainStep(model, crits, cfg, compute_dtype=torch.float32, graph=True, max_graphs=4)
    losses = []
    for i, sizes in enumerate(STREAM):
        h, w = max(s[0] for s in sizes), max(s[1] for s in sizes)
        H, W = bucket_shape(h, w, 32) if bucketed else (h, w)
        b = to_device(synth_batch(2, H, W, seed=70 + i, n_lines=[3 + i % 3, 5], sizes=list(sizes)), "cuda")
        _, total, _ = step(b)
        losses.append(float(total))                     # now: a replayed step returns its entry's static loss tensor
    step.flush()
    torch.cuda.synchronize()
    return step, losses


def test_bucketed_stream_replays_two_captures_where_the_raw_stream_captures_six():
    raws = {(max(s[0] for s in sizes), max(s[1] for s in sizes)) for sizes in STREAM}
    assert len(raws) == 6 and sorted(bucket_shape(h, w, 32) for h, w in raws) == [(96, 128)] * 4 + [(128, 160)] * 2
    step, losses = _run_stream(True)
    st = step.graph_stats()
    assert (st["captures"], st["replays"], st["evictions"], st["eager_steps"], st["refused"], st["host_matcher_steps"]) == (2, 6, 0, 0, 0, 0), st
    assert len(step._graphs) == 2 and all(e["graph"] is not None for e in step._graphs.values()), "capture was refused"
    assert all(torch.isfinite(torch.tensor(losses)))
    step, losses = _run_stream(False)
    st = step.graph_stats()
    assert (st["captures"], st["replays"], st["evictions"]) == (6, 6, 2), st
    assert len(step._graphs) == 4 and all(e["graph"] is not None for e in step._graphs.values())
    assert all(torch.isfinite(torch.tensor(losses)))


def test_bucketed_batch_graph_step_equals_eager_step():
    """Every image of the batch has padding on both sides of the bucket: step 1 through the captured graph == the eager step on
    the same tensors, within the bars of test_hip_graph_step_equals_eager_step."""
    from gw_depth_amd.engine import TrainStep
    from gw_depth_amd.synth import synth_batch
    b = to_device(synth_batch(2, 96, 128, seed=81, n_lines=[4, 6], sizes=[(90, 120), (70, 101)]), "cuda")
    assert bool(b["pad_mask"][:, -1, :].all()) and bool(b["pad_mask"][:, :, -1].all())
    res = []
    for graph in (False, True):
        cfg, model, crits = build(device="cuda")
        step = TrainStep(model, crits, cfg, compute_dtype=torch.float32, graph=graph, max_graphs=16)
        out, total, terms = step(b)
        torch.cuda.synchronize()
        if graph:
            assert step.graph_stats()["replays"] == 1 and all(e["graph"] is not None for e in step._graphs.values()), "capture was refused"
        res.append((float(total), {k: float(v) for k, v in terms.items()}, step.flat_g.clone(), out["pred_depth"][-1].clone()))
    (l0, t0, g0, d0), (l1, t1, g1, d1) = res
    print("loss %r %r  depth rel %.3e  flat_g rel %.3e" % (l0, l1, rel(d1, d0), rel(g1, g0)))
    assert abs(l0 - l1) <= 2e-5 * abs(l0)
    for k in t0:
        assert abs(t0[k] - t1[k]) <= 2e-5 * max(1.0, abs(t0[k])), k
    assert rel(d1, d0) < 2e-5
    assert rel(g1, g0) < 1e-3


def test_capture_after_two_runs_the_first_sight_eagerly():
    from gw_depth_amd.engine import TrainStep
    from gw_depth_amd.synth import synth_batch
    b = to_device(synth_batch(2, 96, 128, seed=83, n_lines=[2, 3]), "cuda")
    cfg, model, crits = build(device="cuda")
    step = TrainStep(model, crits, cfg, compute_dtype=torch.float32, graph=True, capture_after=2)
    step(b)
    st = step.graph_stats()
    assert (st["eager_steps"], st["captures"], st["replays"]) == (1, 0, 0) and not step._graphs, st
    step(b)
    step.flush()
    torch.cuda.synchronize()
    st = step.graph_stats()
    assert (st["eager_steps"], st["captures"], st["replays"]) == (1, 1, 1), st
    assert len(step._graphs) == 1 and all(e["graph"] is not None for e in step._graphs.values()), "capture was refused"
