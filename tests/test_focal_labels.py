"""CPU: --label_loss_func focal_loss through Config, build_model and SetCriterion against the reference's own criterion
(fixture tests/golden/focal_labels.npz from tools/make_golden_focal.py: L = 6, B = 3, Q = 100, targets [1, 12, 0], saturated
logit rows, gamma 0 / 1 / 2 / 2.5; always the reference's fp64 run).  The two torch formulations run here - forward() with the
host matcher and forward_packed with FUSED_SETLOSS off (device LSAP replaced by tests/fake_device.py); the fused node needs the
kernels and is checked by tests/test_focal_labels_gpu.py.  Tolerance: tests/focal_cases.py."""
import argparse

import pytest
import torch

from gw_depth_amd import build_model, hip
from gw_depth_amd.criteria import HungarianMatcherLine, SetCriterion, pack_targets
from tests import focal_cases as fc
from tests.fake_device import FakeDevice

LOSSES = ["lines_labels", "lines"]


@pytest.fixture()
def fake():
    hip.set_library(FakeDevice())
    yield
    hip.set_library(None)


def criterion(**kw):
    g = fc.fixture()
    return SetCriterion(1, fc.weight_dict(6, float(g["line_coef"])), float(g["eos_coef"]), LOSSES,
                        HungarianMatcherLine(float(g["cost_class"]), float(g["cost_line"])), **kw)


def run(crit, path, monkeypatch, fused=False):
    """-> (losses, dlogits, dlines, query of every target column per layer) of the fixture problem through one formulation."""
    g = fc.fixture()
    logits, lines, targets = fc.fixture_problem()
    lg, ln = logits.requires_grad_(True), lines.requires_grad_(True)
    if path == "forward":
        losses = crit(fc.as_outputs(lg, ln), targets)
        qot = fc.qot_of_indices(crit.last_indices, g["in_sizes"])
    else:
        monkeypatch.setattr("gw_depth_amd.criteria.FUSED_SETLOSS", fused)
        losses = crit.forward_packed(fc.as_outputs(lg, ln), pack_targets(targets, "cpu"))
        total = int(g["in_sizes"].sum())
        assert bool((crit.last_query_of_target[:, total:] == 100).all())           # padding columns sit on the dummy query
        qot = crit.last_query_of_target[:, :total].numpy()
    fc.ranked_total(losses, crit.weight_dict).backward()
    return {k: v.detach() for k, v in losses.items()}, lg.grad, ln.grad, qot


@pytest.mark.parametrize("path", ["forward", "packed"])
@pytest.mark.parametrize("gamma", fc.GAMMAS)
def test_focal_criterion_reproduces_the_reference(fake, monkeypatch, gamma, path):
    g = fc.fixture()
    tag = "g%s_fp64_" % gamma
    losses, dlg, dln, qot = run(criterion(label_loss_func="focal_loss", label_loss_params={"gamma": gamma}), path, monkeypatch)
    assert (qot == g[tag + "qot"]).all()
    fc.check_terms(losses, g["keys"], g[tag + "terms"])
    fc.check_grads(dlg, dln, g[tag + "dlogits"], g[tag + "dlines"])
    assert torch.isfinite(dlg[:, :, list(fc.SATURATED_QUERIES)]).all()


@pytest.mark.parametrize("params", ['{"gamma":2.0}', {"gamma": 2.0}], ids=["string", "dict"])
def test_build_model_honours_the_focal_namespace(params):
    g = fc.fixture()
    args = argparse.Namespace(device="cpu", label_loss_func="focal_loss", label_loss_params=params)
    crit = build_model(args)[1][0]
    assert (crit.eos_coef, crit.matcher.cost_class, crit.matcher.cost_line) == (float(g["eos_coef"]), float(g["cost_class"]), float(g["cost_line"]))
    logits, lines, targets = fc.fixture_problem()
    with torch.no_grad():
        got = crit(fc.as_outputs(logits, lines), targets)
        plain = criterion()(fc.as_outputs(logits, lines), targets)
    fc.check_terms(got, g["keys"], g["g2.0_fp64_terms"])
    want = float(g["g2.0_fp64_terms"][list(g["keys"]).index("loss_ce")])
    assert abs(float(plain["loss_ce"]) - want) > 1e-2 and abs(float(got["loss_ce"]) - float(plain["loss_ce"])) > 1e-2    # not the cross entropy


def test_gamma_defaults_to_two_as_in_the_reference():
    for params in (None, "{}", {}):
        assert criterion(label_loss_func="focal_loss", label_loss_params=params).focal_gamma == 2.0


def test_refusals():
    with pytest.raises(ValueError):
        criterion(label_loss_func="dice")
    with pytest.raises(ValueError):
        criterion(label_loss_func="focal_loss", label_loss_params={"gamma": -0.5})
    with pytest.raises(ValueError):
        criterion(label_loss_func="focal_loss", label_loss_params='{"gamma": -1}')
    with pytest.raises(TypeError):
        criterion(label_loss_func="focal_loss", label_loss_params={"gamma": 2.0, "alpha": 0.25})
    with pytest.raises(TypeError):
        criterion(label_loss_func="focal_loss", label_loss_params='{"alpha": 0.25}')
    with pytest.raises(ValueError):                                # literal_eval, not eval: an expression is not evaluated
        criterion(label_loss_func="focal_loss", label_loss_params='dict(gamma=__import__("os").getpid())')
    with pytest.raises(ValueError):
        build_model(argparse.Namespace(device="cpu", label_loss_func="dice"))


@pytest.mark.parametrize("args", [argparse.Namespace(device="cpu"),
                                  argparse.Namespace(device="cpu", label_loss_func="cross_entropy", label_loss_params="{}")],
                         ids=["no_flags", "reference_defaults"])
def test_default_namespace_builds_todays_criterion(fake, monkeypatch, args):
    built = build_model(args)[1][0]
    g = fc.fixture()
    today = SetCriterion(1, built.weight_dict, float(g["eos_coef"]), LOSSES, HungarianMatcherLine(float(g["cost_class"]), float(g["cost_line"])))
    assert built.focal_gamma is None and today.focal_gamma is None
    for path, fused in (("forward", False), ("packed", False), ("packed", True)):
        a, b = run(built, path, monkeypatch, fused), run(today, path, monkeypatch, fused)
        assert set(a[0]) == set(b[0]) and len(a[0]) == 12
        assert all(torch.equal(a[0][k], b[0][k]) for k in a[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and (a[3] == b[3]).all()


def test_entry_point_table_lists_the_focal_pair():
    assert "gwd_set_losses_focal_forward" in hip.ENTRY_POINTS and "gwd_set_losses_focal_backward" in hip.ENTRY_POINTS


def test_focal_entry_points_refuse_bad_arguments_before_any_launch():
    """Status returns of the cross-entropy pair: -1 for a missing operand or a negative gamma, -4 for K or D out of range."""
    import ctypes
    lib = hip.HipLibrary().lib
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def fwd(gamma, K, D, first=p):
        return lib.gwd_set_losses_focal_forward(first, *[p] * 8, 1.0, gamma, *[p] * 4, 1, 1, 1, 1, K, D, None)

    def bwd(gamma, K, D, first=p):
        return lib.gwd_set_losses_focal_backward(first, *[p] * 7, 1.0, gamma, *[p] * 6, 1, 1, 1, 1, K, D, None)

    for call in (fwd, bwd):
        assert call(2.0, 2, 6, first=None) == -1 and call(-1.0, 2, 6) == -1 and call(float("nan"), 2, 6) == -1
        assert call(2.0, 9, 6) == -4 and call(2.0, 0, 6) == -4 and call(2.0, 2, 9) == -4
