"""CPU: gw_depth_amd/graphs.py - the verdict on a warmed-up pass, the session's cache - and the two entry points of TrainStep's one
forward/backward body over tests/fake_device.py.  The cache policy itself (graphs.GraphCache) is in tests/test_shape_buckets.py, the
capture in tests/test_graphs_gpu.py."""
import subprocess
import sys
import warnings

import pytest
import torch

from gw_depth_amd import graphs, hip
from gw_depth_amd.engine import TrainStep, static_batch
from gw_depth_amd.infer import InferenceSession
from gw_depth_amd.synth import synth_batch
from tests.fake_device import FakeDevice
from tests.golden_check import build

MISMATCH = "The AccumulateGrad node's stream does not match the stream of the node that produced the incoming gradient."


@pytest.fixture()
def fake():
    hip.set_library(FakeDevice())
    yield
    hip.set_library(None)


def _caught(*texts):
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        for t in texts:
            warnings.warn(t)
    return caught


def test_verdict_clean_pass_is_captured():
    assert graphs.refusal(0) is None
    assert graphs.refusal(0, [], "forward") is None
    assert graphs.refusal(0, _caught("something else entirely")) is None        # other warnings do not refuse


def test_verdict_each_reason_alone():
    r = graphs.refusal(0, _caught("noise", MISMATCH))
    assert "AccumulateGrad nodes would be captured on a forked stream" in r and "another stream is still alive" in r
    r = graphs.refusal(-1)
    assert r == "the capture audit (torch.profiler runtime-call trace) is not available on this host"
    r = graphs.refusal(3)
    assert r.startswith("3 hipMemsetAsync call(s) in the step (") and "memset nodes do not replay correctly" in r


def test_verdict_precedence():
    forked = graphs.refusal(0, _caught(MISMATCH))
    assert graphs.refusal(-1, _caught(MISMATCH)) == forked                      # the stream mismatch goes before the missing audit
    assert graphs.refusal(5, _caught(MISMATCH)) == forked                       # ... and before the memsets
    assert "hipMemsetAsync" not in forked and "audit" not in forked
    assert graphs.refusal(-1, ()) == graphs.refusal(-1, _caught("noise"))       # a caller that records nothing: rule one never holds
    assert "audit" in graphs.refusal(-1) and "hipMemsetAsync" not in graphs.refusal(-1)     # -1 is "no audit", not "memsets"


def test_verdict_names_the_pass():
    assert "2 hipMemsetAsync call(s) in the forward (" in graphs.refusal(2, (), "forward")
    assert "2 hipMemsetAsync call(s) in the step (" in graphs.refusal(2, (), "step")
    assert "in the step" in graphs.refusal(2)


def test_module_imports_alone():
    """No cycle with engine or infer, and no GPU needed: a fresh interpreter imports graphs first."""
    code = "import gw_depth_amd.graphs as g, sys; assert g.GraphCache().bound() == g.MAX_GRAPHS; import gw_depth_amd.engine, gw_depth_amd.infer"
    subprocess.run([sys.executable, "-c", code], check=True)


def test_session_over_the_fake_device_holds_a_graph_cache(fake):
    cfg, model, crits = build()
    sess = InferenceSession(model, compute_dtype=torch.float32, graph=True)
    assert isinstance(sess._cache, graphs.GraphCache) and sess._cache.entries is sess._graphs
    assert sess._cache.capture_after == 1 and sess._cache.bound() == graphs.MAX_GRAPHS
    b = synth_batch(1, 96, 128, seed=3)
    out = sess(b["images"])                                                     # a CPU call: eager, on the caller's stream
    assert out["pred_logits"].shape[0] == 1
    assert not sess._graphs and not sess.graphs and not sess._cache.seen and not any(sess._cache.stats.values())


def _one_step(seed=5):
    cfg, model, crits = build(dropout=0.0)
    step = TrainStep(model, crits, cfg, compute_dtype=torch.float32)
    step.device_matcher = True                                                  # both entry points on the packed criterion
    torch.manual_seed(seed)
    return step


def test_both_entry_points_run_the_same_pass(fake):
    """forward_backward(batch) and _sync_free_fb(static_batch(batch)) at 1 x 96 x 128 on two identical models: the same total, the
    same 17 terms, the same flat_g, bit for bit; the second returns its total and terms detached."""
    batch = synth_batch(1, 96, 128, seed=11)
    a = _one_step()
    out_a, total_a, terms_a = a.forward_backward(batch)
    assert a.graph_stats()["host_matcher_steps"] == 0, "forward_backward took the host matcher"
    b = _one_step()
    st = static_batch(batch)
    assert sorted(st) == ["depth", "images", "packed", "pad_mask", "seg"]
    assert all(st[k].data_ptr() != batch[k].data_ptr() and torch.equal(st[k], batch[k]) for k in ("images", "pad_mask", "depth", "seg"))
    assert st["packed"].B == 1 and st["packed"].cap == 64
    out_b, total_b, terms_b = b._sync_free_fb(st)
    assert total_a.requires_grad and not total_b.requires_grad and not any(v.requires_grad for v in terms_b.values())
    assert torch.equal(total_a.detach(), total_b)
    assert len(terms_a) == 17 and sorted(terms_a) == sorted(terms_b)
    for k in terms_a:
        assert torch.equal(terms_a[k].detach(), terms_b[k]), k
    assert float(a.flat_g.abs().sum()) > 0
    assert torch.equal(a.flat_g.view(torch.int32), b.flat_g.view(torch.int32))
    assert torch.equal(out_a["pred_logits"], out_b["pred_logits"])
