"""Generate tests/golden/focal_labels.npz with the REAL reference's SetCriterion under --label_loss_func focal_loss, on the CPU.

TEST INFRASTRUCTURE ONLY.  Usage: python tools/make_golden_focal.py   (needs the reference tree; see oracle/ref_stubs.py).

What runs is the reference's own SetCriterion and HungarianMatcher_Line (src/models/glassrgbd.py:133-358, src/models/matcher.py),
imported unmodified under oracle.ref_stubs.install(); this file only draws inputs and stores arrays:
  * L = 6 decoder layers, B = 3 images, Q = 100 queries, K = 2 classes, 6-wide lines, targets [1, 12, 0] (one image without any),
  * logits randn * 2; in every layer and image the queries 0..3 carry the saturated pairs (30,-30), (-30,30), (60,-60), (-60,60), and in
    the 12-target image their lines sit on targets 0..3, so the matcher hands them a target: saturated rows occur both as matched
    (class 0) and as "no object" (class 1) queries, confidently right and confidently wrong,
  * for every gamma in GAMMAS the criterion runs on the fp32 inputs and on fp64 copies of them; stored per run: the twelve loss terms
    (sorted key order), the gradients w.r.t. logits and lines of sum_k weight_dict[k] * (1 + 0.1 * rank(k)) * loss_k (rank in sorted key
    order) and the matcher's assignment as the query of every target column, per layer.
The reference's own fp32 run must stay within the test tolerance (tests/test_focal_labels.py) of its fp64 run, or this script fails.
"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")

GAMMAS = (0.0, 1.0, 2.0, 2.5)
L_, B, Q, K, D = 6, 3, 100, 2, 6
SIZES = (1, 12, 0)
SATURATED = ((30.0, -30.0), (-30.0, 30.0), (60.0, -60.0), (-60.0, 60.0))
EOS_COEF, COST_CLASS, COST_LINE, LINE_COEF = 0.1, 1.0, 5.0, 5.0
TOL = 1e-5


def inputs():
    g = torch.Generator().manual_seed(2025)
    logits = torch.randn(L_, B, Q, K, generator=g) * 2.0
    lines = torch.rand(L_, B, Q, D, generator=g)
    tgt = [torch.rand(n, D, generator=g) for n in SIZES]
    for q, pair in enumerate(SATURATED):
        logits[:, :, q] = torch.tensor(pair)
        lines[:, 1, q] = tgt[1][q] + 0.001 * (q + 1)
    return logits, lines, tgt


def weight_dict():
    wd = {"loss_ce": 1.0, "loss_line": LINE_COEF}
    for i in range(L_ - 1):
        wd.update({"loss_ce_%d" % i: 1.0, "loss_line_%d" % i: LINE_COEF})
    return wd


def run(SetCriterion, Matcher, logits, lines, tgt, gamma, dtype):
    args = types.SimpleNamespace(label_loss_func="focal_loss", label_loss_params='{"gamma": %r}' % gamma, with_line_depth=False)
    crit = SetCriterion(1, weight_dict(), EOS_COEF, ["lines_labels", "lines"], args, matcher=Matcher(COST_CLASS, COST_LINE)).to(dtype)
    assert crit.args.label_loss_params == {"gamma": gamma}
    lg, ln = logits.detach().clone().to(dtype).requires_grad_(True), lines.detach().clone().to(dtype).requires_grad_(True)
    targets = [{"labels": torch.zeros(len(t), dtype=torch.int64), "lines": t.to(dtype)} for t in tgt]
    outs = {"pred_logits": lg[0], "pred_lines": ln[0], "aux_outputs": [{"pred_logits": lg[i], "pred_lines": ln[i]} for i in range(1, L_)]}
    losses = crit(outs, targets)
    keys = sorted(losses)
    assert keys == sorted(weight_dict()) and all(v.dtype == dtype for v in losses.values())
    sum(crit.weight_dict[k] * (1.0 + 0.1 * i) * losses[k] for i, k in enumerate(keys)).backward()
    # the assignment per layer (final layer first, then aux 0..4), as the query of every target column of the concatenated targets
    qot = np.zeros((L_, sum(SIZES)), dtype=np.int64)
    with torch.no_grad():
        for l in range(L_):
            off = 0
            for b, (i, j) in enumerate(crit.matcher({"pred_logits": lg[l], "pred_lines": ln[l]}, targets)):
                qot[l, off + j.numpy()] = i.numpy()
                off += SIZES[b]
    return keys, np.array([float(losses[k].detach()) for k in keys], dtype=np.float64), lg.grad.numpy(), ln.grad.numpy(), qot


def main():
    from oracle import ref_stubs
    ref_stubs.install()
    from models.glassrgbd import SetCriterion                # the reference's classes
    from models.matcher import HungarianMatcher_Line
    logits, lines, tgt = inputs()
    out = {"in_logits": logits.numpy(), "in_lines": lines.numpy(), "in_tgt_lines": torch.cat(tgt).numpy(),
           "in_sizes": np.array(SIZES, dtype=np.int64), "gammas": np.array(GAMMAS), "eos_coef": np.array(EOS_COEF),
           "cost_class": np.array(COST_CLASS), "cost_line": np.array(COST_LINE), "line_coef": np.array(LINE_COEF)}
    for gamma in GAMMAS:
        res = {}
        for name, dtype in (("fp32", torch.float32), ("fp64", torch.float64)):
            keys, terms, dlg, dln, qot = res[name] = run(SetCriterion, HungarianMatcher_Line, logits, lines, tgt, gamma, dtype)
            tag = "g%s_%s_" % (gamma, name)
            out.update({tag + "terms": terms, tag + "dlogits": dlg, tag + "dlines": dln, tag + "qot": qot})
        out["keys"] = np.array(res["fp64"][0])
        a, b = res["fp32"], res["fp64"]
        assert np.array_equal(a[4], b[4]), "fp32 and fp64 assignments differ"
        assert all(np.isfinite(x).all() for r in (a, b) for x in r[1:4])
        e_terms = float(np.max(np.abs(a[1] - b[1]) / np.maximum(1.0, np.abs(b[1]))))
        e_dlg = max(float(np.abs(a[2][l] - b[2][l]).max() / np.abs(b[2][l]).max()) for l in range(L_))
        e_dln = float(np.abs(a[3] - b[3]).max() / np.abs(b[3]).max())
        print("gamma %.1f: loss_ce %.6f; reference fp32 vs fp64: terms %.1e, dlogits (worst layer) %.1e, dlines %.1e"
              % (gamma, b[1][list(b[0]).index("loss_ce")], e_terms, e_dlg, e_dln))
        assert e_terms <= TOL and e_dlg < TOL and e_dln < TOL, (gamma, e_terms, e_dlg, e_dln)
    path = os.path.join(GOLDEN_DIR, "focal_labels.npz")
    np.savez_compressed(path, **out)
    print(path, "%.1f KB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
