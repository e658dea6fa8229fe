"""GPU: the focal label loss inside the fused set-criterion node (gwd_set_losses_focal_forward / _backward, csrc/setloss.hip).

1. the node (forward_packed, FUSED_SETLOSS on) against the reference's own criterion in fp64 (tests/golden/focal_labels.npz),
2. the two kernels on shapes where they can go wrong (fewer queries than threads, a ragged stride loop with a full target table and
   empty images, no target at all) against an fp64 evaluation of the formulas on the CPU, per element,
3. g_ce = NULL, 4. a bf16 train step eager and as a replayed HIP graph, 5. the cross-entropy pair before and after a focal call.
Tolerance: tests/focal_cases.py (the bar of the cross-entropy node's own test), always against fp64 values."""
import pytest
import torch

from gw_depth_amd import hip
from gw_depth_amd.criteria import HungarianMatcherLine, SetCriterion, pack_targets
from tests import focal_cases as fc

pytestmark = pytest.mark.gpu

# L, B, Q, targets per image
SHAPES = {"fewer_queries_than_threads": (2, 1, 7, [3]),           # B*Q = 7 < 256: idle threads must contribute zero
          "ragged_stride_full_table": (2, 3, 100, [64, 0, 0]),    # B*Q = 300: stride loop with a ragged tail; capacity 64 exactly full
          "no_target_at_all": (1, 2, 130, [0, 0])}                # every query is "no object", dlines stays exactly zero


@pytest.fixture(autouse=True)
def real_library():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    hip.set_library(None)
    assert not getattr(hip.library(), "is_fake", False)
    yield


def layer_weights(L_, offset):
    return torch.tensor([1.0 + 0.1 * (2 * l + offset) for l in range(L_)], dtype=torch.float32, device="cuda")


class Problem:
    """One packed set-criterion problem on the device with its assignment (gwd_match_cost + gwd_lsap), and the two set-loss launches
    on ONE set of output buffers - the call sequence of criteria._SetLossFn, entry point by entry point."""

    def __init__(self, L_, B, Q, sizes, seed=7):
        g = torch.Generator().manual_seed(seed)
        logits = torch.randn(L_, B, Q, 2, generator=g) * 2.0
        logits[:, :, 0] = torch.tensor([30.0, -30.0])
        logits[:, :, Q - 1] = torch.tensor([-60.0, 60.0])
        self.logits, self.lines = logits.cuda(), torch.rand(L_, B, Q, 6, generator=g).cuda()
        targets = [{"labels": torch.zeros(n, dtype=torch.int64, device="cuda"), "lines": torch.rand(n, 6, generator=g).cuda()} for n in sizes]
        self.packed = p = pack_targets(targets, "cuda")
        cap = p["lines"].shape[0]
        meta = p["meta"]
        self.col_off, self.bidx, self.valid = meta[:B + 1].contiguous(), meta[B + 1:B + 1 + cap].contiguous(), meta[B + 1 + cap:].contiguous()
        self.cw = torch.tensor([1.0, 0.1], device="cuda")
        self.lib = lib = hip.library()
        cost = torch.empty((L_, B, Q, cap), dtype=torch.float32, device="cuda")
        lib.match_cost(self.logits, self.lines, p["lines"], p["labels"], cost, 5.0, 1.0)
        self.qot = torch.empty((L_, cap), dtype=torch.int32, device="cuda")
        lib.lsap(cost, self.col_off, self.qot, min(hip.LSAP_MAX_TARGETS, Q))
        self.tc = torch.empty((L_, B, Q), dtype=torch.int32, device="cuda")
        self.out = torch.empty((3, L_), dtype=torch.float32, device="cuda")
        self.dlogits, self.dlines = torch.empty_like(self.logits), torch.empty_like(self.lines)
        self.g_ce, self.g_l1 = layer_weights(L_, 0), layer_weights(L_, 1)

    def run(self, gamma, with_g_ce=True):
        """-> (ce, l1, wsum, target classes, dlogits, dlines), copies; gamma None: the cross-entropy pair."""
        p, out = self.packed, self.out
        self.lib.set_losses_forward(self.logits, self.lines, p["lines"], p["labels"], self.bidx, self.valid, self.qot, self.cw, p["num_items"], 1.0,
                                    self.tc, out[0], out[1], out[2], gamma=gamma)
        self.dlogits.fill_(float("nan"))                     # the kernel writes every element
        self.dlines.zero_()                                  # ... and ADDS to these
        self.lib.set_losses_backward(self.logits, self.lines, p["lines"], self.bidx, self.valid, self.qot, self.cw, p["num_items"], 1.0, self.tc,
                                     out[2], self.g_ce if with_g_ce else None, self.g_l1, self.dlogits, self.dlines, gamma=gamma)
        torch.cuda.synchronize()
        return tuple(t.clone() for t in (out[0], out[1], out[2], self.tc, self.dlogits, self.dlines))

    def reference(self, gamma, with_g_ce=True):
        p = self.packed
        return fc.criterion_fp64(self.logits, self.lines, p["lines"], p["labels"], self.bidx, self.valid, self.qot, self.cw, float(p["num_items"]),
                                 gamma, self.g_ce if with_g_ce else None, self.g_l1)


def check_layers(got, want, name):
    for l, (a, b) in enumerate(zip(got.double().cpu().tolist(), want.tolist())):
        print("%s[%d] %.9f  fp64 %.9f  |diff| %.2e" % (name, l, a, b, abs(a - b)))
        assert abs(a - b) <= fc.TOL * max(1.0, abs(b)), (name, l, a, b)


@pytest.mark.parametrize("gamma", fc.GAMMAS)
def test_fused_node_reproduces_the_reference(gamma, monkeypatch):
    g = fc.fixture()
    tag = "g%s_fp64_" % gamma
    monkeypatch.setattr("gw_depth_amd.criteria.FUSED_SETLOSS", True)
    crit = SetCriterion(1, fc.weight_dict(6, float(g["line_coef"])), float(g["eos_coef"]), ["lines_labels", "lines"],
                        HungarianMatcherLine(float(g["cost_class"]), float(g["cost_line"])), label_loss_func="focal_loss",
                        label_loss_params={"gamma": gamma}).cuda()
    logits, lines, targets = fc.fixture_problem("cuda")
    lg, ln = logits.requires_grad_(True), lines.requires_grad_(True)
    losses = crit.forward_packed(fc.as_outputs(lg, ln), pack_targets(targets, "cuda"))
    assert crit.last_stacks is not None                      # the fused node ran, not the torch formulation
    fc.ranked_total(losses, crit.weight_dict).backward()
    torch.cuda.synchronize()
    total = int(g["in_sizes"].sum())
    qot = crit.last_query_of_target.cpu()
    assert (qot[:, :total].numpy() == g[tag + "qot"]).all() and bool((qot[:, total:] == 100).all())
    fc.check_terms({k: v.detach() for k, v in losses.items()}, g["keys"], g[tag + "terms"])
    fc.check_grads(lg.grad, ln.grad, g[tag + "dlogits"], g[tag + "dlines"])
    assert torch.isfinite(lg.grad[:, :, list(fc.SATURATED_QUERIES)]).all()


@pytest.mark.parametrize("shape", list(SHAPES))
def test_kernels_on_edge_shapes_against_fp64(shape):
    L_, B, Q, sizes = SHAPES[shape]
    prob = Problem(L_, B, Q, sizes)
    n_matched = int((prob.qot < Q).sum())
    assert n_matched == L_ * sum(sizes)
    for gamma in fc.GAMMAS:
        ce, l1, _, tc, dlg, dln = prob.run(gamma)
        want_ce, want_l1, want_dlg, want_dln = prob.reference(gamma)
        assert int((tc == 0).sum()) == n_matched and int((tc == 1).sum()) == L_ * B * Q - n_matched
        check_layers(ce, want_ce, "ce gamma %s" % gamma)
        check_layers(l1, want_l1, "l1 gamma %s" % gamma)
        fc.check_grads(dlg, dln, want_dlg, want_dln, per_element=True)
        if sum(sizes) == 0:
            assert not bool(dln.any())


def test_without_label_gradient_dlogits_is_zero():
    L_, B, Q, sizes = SHAPES["ragged_stride_full_table"]
    prob = Problem(L_, B, Q, sizes)
    _, _, _, _, dlg, dln = prob.run(2.0, with_g_ce=False)
    _, _, want_dlg, want_dln = prob.reference(2.0, with_g_ce=False)
    assert not bool(dlg.any()) and not bool(want_dlg.any())
    fc.check_grads(dlg, dln, want_dlg, want_dln, per_element=True)
    assert bool(dln.any())


@pytest.mark.parametrize("shape", list(SHAPES))
def test_cross_entropy_pair_is_untouched_by_a_focal_call(shape):
    """The cross-entropy entry points on the same buffers before and after a focal call: identical bits (no shared state), and the
    values of the weighted mean, not of the focal mean."""
    L_, B, Q, sizes = SHAPES[shape]
    prob = Problem(L_, B, Q, sizes)
    before = prob.run(None)
    focal = prob.run(2.0)
    after = prob.run(None)
    assert all(torch.equal(a, b) for a, b in zip(before, after))
    assert not torch.equal(before[0], focal[0]) and torch.equal(before[1], focal[1]) and torch.equal(before[3], focal[3])
    tc = before[3].long()
    nll = torch.nn.functional.cross_entropy(prob.logits.double().flatten(0, 2), tc.flatten(), reduction="none").reshape(L_, -1)
    w = prob.cw.double()[tc].reshape(L_, -1)
    check_layers(before[0], ((nll * w).sum(1) / w.sum(1)).cpu(), "weighted cross entropy")


def focal_train_step(graph):
    from gw_depth_amd import Config, build_model
    from gw_depth_amd.engine import TrainStep
    from gw_depth_amd.synth import det_fill_, synth_batch
    from tests.golden_check import to_device
    from tests.helpers import reference_state_shapes
    cfg = Config(device="cuda", dropout=0.0, log_depth_error=True, label_loss_func="focal_loss", label_loss_params='{"gamma": 2.0}')
    model, crits, _ = build_model(cfg)
    model.load_state_dict(det_fill_(reference_state_shapes(), seed=0), strict=True)
    model.cuda()
    crits[0].cuda()
    assert crits[0].focal_gamma == 2.0
    n_lines = [4, 6]
    b = to_device(synth_batch(2, 96, 128, seed=41, n_lines=n_lines), "cuda")
    step = TrainStep(model, crits, cfg, compute_dtype=torch.bfloat16, graph=graph)
    out, total, terms = step(b)
    torch.cuda.synchronize()
    if graph:
        assert step._graphs and all(e["graph"] is not None for e in step._graphs.values()), "capture was refused"
    assert len(terms) == 17 and crits[0].last_stacks is not None
    # the six label terms again, in fp64 on the CPU, from the step's own logits and assignment
    logits = torch.stack([o["pred_logits"] for o in [out] + out["aux_outputs"]]).detach().double().cpu()
    qot = crits[0].last_query_of_target.cpu()
    L_, B, Q, K = logits.shape
    tc = torch.full((L_, B, Q), K - 1, dtype=torch.int64)
    col = 0
    for bi, n in enumerate(n_lines):
        for _ in range(n):
            tc[torch.arange(L_), bi, qot[:, col]] = 0
            col += 1
    assert bool((qot[:, col:] == Q).all()) and int((tc == 0).sum()) == L_ * sum(n_lines)
    recomputed = fc.focal_ce_fp64(logits, tc, crits[0].empty_weight.cpu(), 2.0)
    res = float(total), {k: float(v) for k, v in terms.items()}, recomputed.tolist()
    del step, out, total, terms                     # no autograd graph of this step outlives it (the next one captures)
    return res


def test_bf16_train_step_eager_and_replayed_graph():
    (l0, t0, r0), (l1, t1, r1) = focal_train_step(False), focal_train_step(True)
    names = ["loss_ce"] + ["loss_ce_%d" % i for i in range(5)]
    for t, r in ((t0, r0), (t1, r1)):
        for k, want in zip(names, r):
            print("%-10s %.9f  fp64 %.9f" % (k, t[k], want))
            assert abs(t[k] - want) <= fc.TOL * max(1.0, abs(want)), (k, t[k], want)
    # the bar of tests/test_bf16_pinning.py::test_bf16_graph_replay_equals_the_eager_bf16_step for the first step of this very batch
    assert set(t0) == set(t1) and abs(l0 - l1) <= 2e-3 * abs(l0), (l0, l1)
    for k in t0:
        print("%-16s eager %.9f  graph %.9f" % (k, t0[k], t1[k]))
        assert abs(t0[k] - t1[k]) <= 2e-3 * max(1.0, abs(t0[k])), (k, t0[k], t1[k])
