"""Generate tests/golden/postprocess_line.npz with the REAL reference's PostProcess_Line on the CPU.

TEST INFRASTRUCTURE ONLY.  Usage: python tools/make_golden_postprocess.py   (needs the reference tree; see oracle/ref_stubs.py).

What runs is the reference's own class (src/models/glassrgbd.py:452-506), imported unmodified under oracle.ref_stubs.install();
this file only draws inputs and stores arrays:
  * 'prediction' and 'prediction_POST' on B = 3 images of different target_sizes, Q = 100, 4-wide pred_lines and a DIFFERENT
    POST_pred_lines (the reference raises on 6-wide lines: its scale is 4-wide),
  * 'ground_truth' on B = 1 (the reference broadcasts (n,4) * (B,4): nothing else works).
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")


def inputs():
    g = torch.Generator().manual_seed(2024)
    B, Q = 3, 100
    return {"pred_logits": torch.randn(B, Q, 2, generator=g) * 2.0,
            "pred_lines": torch.rand(B, Q, 4, generator=g),
            "POST_pred_lines": torch.rand(B, Q, 4, generator=g),
            "target_sizes": torch.tensor([[480.0, 640.0], [960.0, 1280.0], [427.0, 569.0]]),
            "gt_lines": torch.rand(7, 4, generator=g),
            "gt_labels": torch.zeros(7, dtype=torch.int64),
            "gt_image_id": torch.tensor([31]),
            "gt_target_sizes": torch.tensor([[375.0, 1242.0]])}


def main():
    from oracle import ref_stubs
    ref_stubs.install()
    from models.glassrgbd import PostProcess_Line            # the reference's class
    post = PostProcess_Line()
    x = inputs()
    out = {"in_" + k: v.numpy() for k, v in x.items()}
    outputs = {k: x[k] for k in ("pred_logits", "pred_lines", "POST_pred_lines")}
    for kind in ("prediction", "prediction_POST"):
        res = post(outputs, x["target_sizes"], kind)
        assert len(res) == 3 and sorted(res[0]) == ["labels", "lines", "scores"]
        for k in ("scores", "labels", "lines"):
            out["%s_%s" % (kind, k)] = torch.stack([r[k] for r in res]).numpy()
    res = post([{"lines": x["gt_lines"], "labels": x["gt_labels"], "image_id": x["gt_image_id"]}], x["gt_target_sizes"], "ground_truth")
    assert len(res) == 1 and sorted(res[0]) == ["image_id", "labels", "lines"]
    for k in ("labels", "lines", "image_id"):
        out["ground_truth_" + k] = res[0][k].numpy()
    path = os.path.join(GOLDEN_DIR, "postprocess_line.npz")
    np.savez_compressed(path, **out)
    print(path, "%.1f KB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
