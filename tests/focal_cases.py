"""Shared by tests/test_focal_labels.py (CPU) and tests/test_focal_labels_gpu.py: the fixture of the reference's focal label loss
(tests/golden/focal_labels.npz, written by tools/make_golden_focal.py from the reference's own SetCriterion), the tolerance, and an
fp64 evaluation of the criterion's formulas for shapes the fixture does not have.

Tolerance (the bar tests/test_hip_kernels.py sets for the same quantities of the cross-entropy node), always against fp64 values:
  loss terms  |a - b| <= 1e-5 * max(1, |b|)
  gradients   max|a - b| / max|b| < 1e-5, per decoder layer for the logit gradients (one large layer cannot hide another)."""
import functools
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "focal_labels.npz")
GAMMAS = (0.0, 1.0, 2.0, 2.5)
TOL = 1e-5
SATURATED_QUERIES = (0, 1, 2, 3)


@functools.lru_cache(maxsize=None)
def fixture():
    g = {k: v for k, v in np.load(GOLDEN).items()}
    assert tuple(g["gammas"]) == GAMMAS
    return g


def fixture_problem(device="cpu"):
    """(logits (L,B,Q,2), lines (L,B,Q,6), targets) of the fixture as fresh tensors on `device`."""
    g = fixture()
    lines = torch.from_numpy(g["in_tgt_lines"]).split([int(n) for n in g["in_sizes"]])
    targets = [{"labels": torch.zeros(len(t), dtype=torch.int64, device=device), "lines": t.clone().to(device)} for t in lines]
    return torch.from_numpy(g["in_logits"]).clone().to(device), torch.from_numpy(g["in_lines"]).clone().to(device), targets


def weight_dict(layers, line_coef=5.0):
    wd = {"loss_ce": 1.0, "loss_line": line_coef}
    for i in range(layers - 1):
        wd.update({"loss_ce_%d" % i: 1.0, "loss_line_%d" % i: line_coef})
    return wd


def as_outputs(lg, ln):
    return {"pred_logits": lg[0], "pred_lines": ln[0], "aux_outputs": [{"pred_logits": lg[i], "pred_lines": ln[i]} for i in range(1, lg.shape[0])]}


def ranked_total(losses, wd):
    """sum_k wd[k] * (1 + 0.1 * rank(k)) * loss_k, keys ranked in sorted order: every term gets its own upstream gradient."""
    return sum(wd[k] * (1.0 + 0.1 * i) * losses[k] for i, k in enumerate(sorted(losses)))


def qot_of_indices(last_indices, sizes):
    """Per-layer [(query ids, target ids) per image] -> the query of every target column of the concatenated targets."""
    qot = np.zeros((len(last_indices), int(sum(sizes))), dtype=np.int64)
    for l, idx in enumerate(last_indices):
        off = 0
        for b, (i, j) in enumerate(idx):
            qot[l, off + j.numpy()] = i.numpy()
            off += int(sizes[b])
    return qot


def check_terms(got, want_keys, want_terms):
    assert sorted(got) == list(want_keys)
    for k, b in zip(want_keys, want_terms):
        a = float(got[k])
        print("%-12s %.9f  fp64 %.9f  |diff| %.2e" % (k, a, b, abs(a - b)))
        assert abs(a - b) <= TOL * max(1.0, abs(b)), (k, a, b)


def check_grads(dlogits, dlines, want_dlogits, want_dlines, per_element=False):
    a, b = dlogits.detach().double().cpu(), torch.as_tensor(want_dlogits).double()
    assert a.shape == b.shape and torch.isfinite(a).all()
    for l in range(b.shape[0]):
        scale = float(b[l].abs().max())
        err = float((a[l] - b[l]).abs().max())
        print("dlogits layer %d: max|diff| %.2e, max|ref| %.2e" % (l, err, scale))
        # a layer whose reference gradient is all zero has no scale: it must be zero exactly
        assert err < TOL * scale or (scale == 0.0 and err == 0.0), (l, err, scale)
        if per_element:
            assert bool(((a[l] - b[l]).abs() <= TOL * scale).all()), l
    a, b = dlines.detach().double().cpu(), torch.as_tensor(want_dlines).double()
    assert a.shape == b.shape and torch.isfinite(a).all()
    scale, err = float(b.abs().max()), float((a - b).abs().max())
    print("dlines: max|diff| %.2e, max|ref| %.2e" % (err, scale))
    assert err < TOL * scale or (scale == 0.0 and err == 0.0), (err, scale)


def focal_ce_fp64(logits, target_class, class_weight, gamma):
    """Per layer, in fp64: mean over the B*Q queries of w * nll * u^gamma with u the sum of the OTHER classes' probabilities.
    logits (L,B,Q,K), target_class (L,B,Q) int64 -> (L,)."""
    lg = logits.double()
    logp = torch.log_softmax(lg, -1)
    nll = -logp.gather(-1, target_class[..., None])[..., 0]
    hit = torch.nn.functional.one_hot(target_class, lg.shape[-1]).bool()
    u = logp.exp().masked_fill(hit, 0.0).sum(-1)
    return (class_weight.double()[target_class] * nll * u ** gamma).flatten(1).mean(1)


def criterion_fp64(logits, lines, tgt_lines, tgt_labels, bidx, valid, qot, class_weight, num_items, gamma, g_ce, g_l1):
    """The set criterion of one packed problem in fp64 on the CPU, for a GIVEN assignment qot (L,cap; padding columns carry Q):
    (ce (L,), l1 (L,), dlogits, dlines) with the gradients of sum(g_ce * ce) + sum(g_l1 * l1) (g_ce None: no label gradient)."""
    L_, B, Q, K = logits.shape
    lg, ln = logits.double().cpu().clone().requires_grad_(True), lines.double().cpu().clone().requires_grad_(True)
    qot, bidx, valid = qot.long().cpu(), bidx.long().cpu(), valid.double().cpu()
    li, bi = torch.arange(L_)[:, None], bidx[None].expand(L_, -1)
    tc = torch.full((L_, B, Q + 1), K - 1, dtype=torch.int64)
    tc[li, bi, qot] = tgt_labels.cpu()[None].expand(L_, -1)
    tc = tc[:, :, :Q]
    ce = focal_ce_fp64(lg, tc, class_weight.cpu(), gamma)
    n = max(float(num_items), 1.0)
    l1 = ((ln[li, bi, qot.clamp(max=Q - 1)] - tgt_lines.double().cpu()[None]).abs().sum(-1) * valid[None]).sum(1) / n
    total = (l1 * g_l1.double().cpu()).sum()
    if g_ce is not None:
        total = total + (ce * g_ce.double().cpu()).sum()
    total.backward()
    dlg = lg.grad if lg.grad is not None else torch.zeros_like(lg)
    dln = ln.grad if ln.grad is not None else torch.zeros_like(ln)
    return ce.detach(), l1.detach(), dlg, dln
