"""The device matcher beyond 64 targets per image: gwd_lsap up to 1024 targets and with more targets than queries against scipy, the
fused set criterion on such a batch against SetCriterion.forward with the host matcher, and whole steps with more than 64 targets,
more targets than queries and no target at all replayed from a captured graph against the eager host-matcher step."""
import functools

import numpy as np
import pytest
import torch

from gw_depth_amd import hip
from tests.golden_check import build, rel, to_device

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def real_library():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    hip.set_library(None)
    assert not getattr(hip.library(), "is_fake", False)
    yield


def test_limit_constant():
    assert hip.LSAP_MAX_TARGETS == 1024


LSAP_CASES = [(100, (65, 100, 0)),         # above 64, T = Q, an empty image
              (20, (33, 20, 7)),           # T > Q
              (300, (128, 1, 300)),        # several column passes
              (1024, (200, 1024))]         # the limits
PAD = 5                                     # padding columns behind the last image
LAYERS = 2


@functools.lru_cache(maxsize=None)
def _lsap_problem(Q, sizes):
    """Seeded fp32 costs (LAYERS, B, Q, sum + PAD) and scipy's optimum per (layer, image): (query of every target or Q, f64 cost sum)."""
    from scipy.optimize import linear_sum_assignment
    g = torch.Generator().manual_seed(1000 + Q)
    B, sumT = len(sizes), sum(sizes) + PAD
    cost = torch.rand(LAYERS, B, Q, sumT, generator=g) * 5 - 1
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    want = {}
    for l in range(LAYERS):
        for b in range(B):
            c = cost[l, b, :, off[b]:off[b + 1]].double().numpy()
            qi, ti = linear_sum_assignment(c)
            qot = np.full(sizes[b], Q, dtype=np.int64)
            qot[ti] = qi
            want[(l, b)] = (qot, float(c[qi, ti].sum()))
    return cost, off, want


@pytest.mark.parametrize("Q,sizes", LSAP_CASES, ids=["Q%d_%s" % (q, "-".join(map(str, s))) for q, s in LSAP_CASES])
def test_wide_lsap_is_optimal(Q, sizes):
    cost, off, want = _lsap_problem(Q, sizes)
    sumT = cost.shape[-1]
    out = torch.full((LAYERS, sumT), -1, dtype=torch.int32, device="cuda")
    hip.library().lsap(cost.cuda(), torch.as_tensor(off, device="cuda"), out, max(sizes))
    torch.cuda.synchronize()
    out = out.cpu().numpy().astype(np.int64)
    identical = True
    for l in range(LAYERS):
        assert (out[l, off[-1]:] == Q).all(), "padding columns hold the dummy query"
        for b, T in enumerate(sizes):
            got = out[l, off[b]:off[b + 1]]
            wq, wsum = want[(l, b)]
            assert ((got >= 0) & (got <= Q)).all()
            t_m = np.nonzero(got < Q)[0]
            q_m = got[t_m]
            assert len(t_m) == min(Q, T) and len(set(q_m.tolist())) == len(q_m), (l, b, "a valid matching of min(Q, T) pairs")
            assert (got[np.setdiff1d(np.arange(T), t_m)] == Q).all()                # surplus targets hold Q
            c = cost[l, b, :, off[b]:off[b + 1]].double().numpy()
            gsum = float(c[q_m, t_m].sum())
            assert abs(gsum - wsum) <= 1e-12 * abs(wsum), (l, b, gsum, wsum)
            identical &= bool((got == wq).all())
    assert identical, "optimal, but not scipy's assignment (expected identical on these seeds)"


def _criterion_problem(sizes, L_=3, Q=100):
    from gw_depth_amd.criteria import HungarianMatcherLine, SetCriterion
    torch.manual_seed(23)
    crit = SetCriterion(1, {}, 0.1, ["lines_labels", "lines"], HungarianMatcherLine(1.0, 5.0)).cuda()
    targets = [{"labels": torch.zeros(n, dtype=torch.int64, device="cuda"), "lines": torch.rand(n, 6, device="cuda")} for n in sizes]
    return crit, targets, torch.randn(L_, len(sizes), Q, 2, device="cuda"), torch.rand(L_, len(sizes), Q, 6, device="cuda")


def test_fused_set_criterion_with_more_targets_than_queries_equals_the_host_matcher():
    """n_lines = [120, 5] on 100 queries: _SetLossFn (match cost, device LSAP, set losses and their backward) == SetCriterion.forward,
    which matches with scipy on the host; the 20 surplus targets of image 0 carry neither a label nor an L1 term."""
    from gw_depth_amd.criteria import pack_targets
    sizes = [120, 5]
    crit, targets, logits0, lines0 = _criterion_problem(sizes)
    L_, Q = logits0.shape[0], logits0.shape[2]
    packed = pack_targets(targets, "cuda")
    res = {}
    for mode in ("device", "host"):
        lg, ln = logits0.clone().requires_grad_(True), lines0.clone().requires_grad_(True)
        outs = {"pred_logits": lg[0], "pred_lines": ln[0], "aux_outputs": [{"pred_logits": lg[i], "pred_lines": ln[i]} for i in range(1, L_)]}
        losses = crit.forward_packed(outs, packed) if mode == "device" else crit(outs, targets)
        total = sum(v * (1.0 + 0.1 * i) for i, (k, v) in enumerate(sorted(losses.items())))
        total.backward()
        torch.cuda.synchronize()
        res[mode] = ({k: float(v) for k, v in losses.items()}, lg.grad.clone(), ln.grad.clone())
    qot = crit.last_query_of_target.cpu()
    assert int((qot[:, :120] < Q).sum()) == L_ * Q and int((qot[:, 120:125] < Q).sum()) == L_ * 5 and bool((qot[:, 125:] == Q).all())
    a, b = res["device"], res["host"]
    assert set(a[0]) == set(b[0]) and len(a[0]) == 2 * L_
    print({k: (a[0][k], b[0][k]) for k in a[0]}, rel(a[1], b[1]), rel(a[2], b[2]))
    for k in a[0]:
        assert abs(a[0][k] - b[0][k]) <= 2e-5 * max(1.0, abs(b[0][k])), (k, a[0][k], b[0][k])
    assert rel(a[1], b[1]) < 1e-5 and rel(a[2], b[2]) < 1e-5


def test_torch_formulation_masks_surplus_targets(monkeypatch):
    """forward_packed with FUSED_SETLOSS off (the A/B path of the fused node) on the same batch: same terms and gradients."""
    from gw_depth_amd.criteria import pack_targets
    crit, targets, logits0, lines0 = _criterion_problem([120, 5])
    L_ = logits0.shape[0]
    packed = pack_targets(targets, "cuda")
    res = {}
    for fused in (True, False):
        monkeypatch.setattr("gw_depth_amd.criteria.FUSED_SETLOSS", fused)
        lg, ln = logits0.clone().requires_grad_(True), lines0.clone().requires_grad_(True)
        outs = {"pred_logits": lg[0], "pred_lines": ln[0], "aux_outputs": [{"pred_logits": lg[i], "pred_lines": ln[i]} for i in range(1, L_)]}
        losses = crit.forward_packed(outs, packed)
        sum(v * (1.0 + 0.1 * i) for i, (k, v) in enumerate(sorted(losses.items()))).backward()
        torch.cuda.synchronize()
        res[fused] = ({k: float(v) for k, v in losses.items()}, lg.grad.clone(), ln.grad.clone())
    a, b = res[True], res[False]
    for k in a[0]:
        assert abs(a[0][k] - b[0][k]) <= 1e-5 * max(1.0, abs(b[0][k])), (k, a[0][k], b[0][k])
    assert rel(a[1], b[1]) < 1e-5 and rel(a[2], b[2]) < 1e-5


@pytest.mark.parametrize("n_lines", [[70, 3], [120, 5], [0, 0]], ids=["70-3", "120-5", "0-0"])
def test_wide_and_empty_batches_replay_and_equal_the_host_matcher_step(n_lines):
    """More than 64 targets in an image, more targets than queries, and no target at all: the graph-mode step captures and replays
    (no host matcher) and equals the eager step with the host matcher, within the bars of
    test_device_matcher_step_equals_host_matcher_step."""
    from gw_depth_amd.engine import TrainStep
    from gw_depth_amd.synth import synth_batch
    b = to_device(synth_batch(2, 96, 128, seed=91, n_lines=n_lines), "cuda")
    res = []
    for graph in (False, True):
        cfg, model, crits = build(device="cuda")
        step = TrainStep(model, crits, cfg, compute_dtype=torch.float32, graph=graph)
        step.device_matcher = graph
        out, total, terms = step(b)
        torch.cuda.synchronize()
        st = step.graph_stats()
        if graph:
            assert step._graphs and all(e["graph"] is not None for e in step._graphs.values()), "capture was refused"
            assert (st["replays"], st["host_matcher_steps"], st["eager_steps"]) == (1, 0, 0), st
        else:
            assert st["host_matcher_steps"] == 1
        res.append((float(total), {k: float(v) for k, v in terms.items()}, step.flat_p.clone()))
    (l0, t0, p0), (l1, t1, p1) = res
    print("loss %r %r  params rel %.3e  worst term %.3e" % (l0, l1, rel(p1, p0), max(abs(t0[k] - t1[k]) / max(1.0, abs(t0[k])) for k in t0)))
    assert abs(l0 - l1) <= 2e-5 * abs(l0)
    assert set(t0) == set(t1)
    for k in t0:
        assert abs(t0[k] - t1[k]) <= 2e-5 * max(1.0, abs(t0[k])), k
    assert rel(p1, p0) < 1e-6
