"""CPU: criteria.PostProcessLine against the reference's own PostProcess_Line (src/models/glassrgbd.py:452-506), all three
branches.  Fixture: tests/golden/postprocess_line.npz, written by tools/make_golden_postprocess.py from the reference's class
(B = 3 images of different target_sizes, Q = 100, 4-wide pred_lines and a different POST_pred_lines; 'ground_truth' with B = 1).
Labels and image_id must be equal; floats within 1e-6 relative (the same torch ops, possibly on another host's vector units)."""
import os

import numpy as np
import pytest
import torch

from gw_depth_amd.criteria import PostProcessLine

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "postprocess_line.npz")
RTOL = 1e-6


@pytest.fixture(scope="module")
def g():
    return {k: torch.from_numpy(v) for k, v in np.load(GOLDEN).items()}


def close(a, b):
    a, b = a.double(), b.double()
    return bool(((a - b).abs() <= RTOL * b.abs()).all())


def outputs_of(g):
    return {k: g["in_" + k] for k in ("pred_logits", "pred_lines", "POST_pred_lines")}


@pytest.mark.parametrize("kind", ["prediction", "prediction_POST"])
def test_prediction_branches_reproduce_the_reference(g, kind):
    assert not torch.equal(g["in_pred_lines"], g["in_POST_pred_lines"])
    assert not torch.equal(g["prediction_lines"], g["prediction_POST_lines"])
    res = PostProcessLine()(outputs_of(g), g["in_target_sizes"], kind)
    assert len(res) == 3
    for i, r in enumerate(res):
        assert sorted(r) == ["labels", "lines", "scores"]
        assert torch.equal(r["labels"], g[kind + "_labels"][i])
        assert r["scores"].shape == (100,) and close(r["scores"], g[kind + "_scores"][i])
        assert r["lines"].shape == (100, 4) and close(r["lines"], g[kind + "_lines"][i])


def test_prediction_is_the_default_branch(g):
    a = PostProcessLine()(outputs_of(g), g["in_target_sizes"])
    b = PostProcessLine()(outputs_of(g), g["in_target_sizes"], "prediction")
    for x, y in zip(a, b):
        assert all(torch.equal(x[k], y[k]) for k in x)


def test_ground_truth_branch_reproduces_the_reference(g):
    tgt = [{"lines": g["in_gt_lines"], "labels": g["in_gt_labels"], "image_id": g["in_gt_image_id"]}]
    res = PostProcessLine()(tgt, g["in_gt_target_sizes"], "ground_truth")
    assert len(res) == 1 and sorted(res[0]) == ["image_id", "labels", "lines"]
    assert torch.equal(res[0]["labels"], g["ground_truth_labels"])
    assert torch.equal(res[0]["image_id"], g["ground_truth_image_id"])
    assert res[0]["lines"].shape == g["ground_truth_lines"].shape and close(res[0]["lines"], g["ground_truth_lines"])


@pytest.mark.parametrize("kind", ["prediction", "prediction_POST"])
def test_six_wide_lines_give_the_first_four_coordinates(g, kind):
    out = outputs_of(g)
    gen = torch.Generator().manual_seed(3)
    wide = {k: (torch.cat([v, torch.rand(3, 100, 2, generator=gen)], -1) if k.endswith("lines") else v) for k, v in out.items()}
    a = PostProcessLine()(out, g["in_target_sizes"], kind)
    b = PostProcessLine()(wide, g["in_target_sizes"], kind)
    for x, y in zip(a, b):
        assert y["lines"].shape == (100, 4) and torch.equal(x["lines"], y["lines"]) and torch.equal(x["scores"], y["scores"])
    tgt = [{"lines": torch.rand(5, 6, generator=gen), "labels": torch.zeros(5, dtype=torch.int64), "image_id": torch.tensor([4])}]
    sz = torch.tensor([[480.0, 640.0]])
    r = PostProcessLine()(tgt, sz, "ground_truth")[0]
    assert torch.equal(r["lines"], tgt[0]["lines"][:, :4] * torch.tensor([640.0, 480.0, 640.0, 480.0]))


def test_ground_truth_of_two_images_equals_two_single_calls():
    gen = torch.Generator().manual_seed(11)
    tgt = [{"lines": torch.rand(n, 4, generator=gen), "labels": torch.zeros(n, dtype=torch.int64), "image_id": torch.tensor([i])}
           for i, n in enumerate((6, 9))]
    sizes = torch.tensor([[480.0, 640.0], [375.0, 1242.0]])
    both = PostProcessLine()(tgt, sizes, "ground_truth")
    assert len(both) == 2
    for i in range(2):
        one = PostProcessLine()(tgt[i:i + 1], sizes[i:i + 1], "ground_truth")[0]
        assert sorted(both[i]) == ["image_id", "labels", "lines"]
        assert all(torch.equal(both[i][k], one[k]) for k in one)
    assert not torch.equal(both[1]["lines"], tgt[1]["lines"] * torch.tensor([640.0, 480.0, 640.0, 480.0]))


def test_unknown_output_type_raises(g):
    with pytest.raises(AssertionError):
        PostProcessLine()(outputs_of(g), g["in_target_sizes"], "prediction_post")
