"""GPU: gwd_line_score (csrc/linescore.hip) and evaluate.LineMetrics against tests/golden/line_score.npz - what the reference's own
line NMS and msTPFP returned on float64 arrays - and, at the sizes the fixture does not hold, against tests/line_score_ref.py.

Bars (fixed before any run): kept ids and every flag identical; clipped lines within 1e-9 px (f64, about 20 operations on coordinates
below 1e3: an error near 1e-13, the bar is 1e4 times that); scores bit-equal to torch.softmax on the same device; AP / F within 1e-12
of the fixture; bytes beside the written slots untouched.  Every measured figure is printed before it is asserted."""
import numpy as np
import pytest
import torch

from gw_depth_amd import hip
from gw_depth_amd.evaluate import LineMetrics, evaluate
from tests import line_score_ref as R
from tests.test_line_score import GOLDEN, LINE_TOL, check_stats

pytestmark = pytest.mark.gpu
GUARD, FILL = 256, 0xA5


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLDEN))


@pytest.fixture()
def dev():
    hip.set_library(None)
    return torch.device("cuda")


def guarded(shape, dtype, device):
    n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    raw = torch.full((GUARD + n + GUARD,), FILL, dtype=torch.uint8, device=device)
    return raw, raw[GUARD:GUARD + n].view(dtype).view(shape)


def run_kernel(dev, logits, lines, sizes, gt, counts, nms=R.NMS_THRESHOLDS, sap=R.SAP_THRESHOLDS, cap=None, slot=0):
    """One gwd_line_score call into guarded buffers of `cap` image slots.  Returns numpy outputs and the raw guarded buffers."""
    B, Q = logits.shape[:2]
    cap = B if cap is None else cap
    T, S = len(nms), len(sap)
    bufs = {"flag": guarded((T, S, cap, Q), torch.uint8, dev), "kept": guarded((T, cap, Q, 4), torch.float64, dev),
            "score": guarded((cap, Q), torch.float32, dev), "seen": guarded((cap,), torch.int32, dev)}
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).to(dev)
    gt = np.zeros((B, 1, 4), np.float32) if gt.shape[1] == 0 else gt
    hip.library().line_score(t(logits, torch.float32), t(lines, torch.float32), t(sizes, torch.int32), t(gt, torch.float32),
                             t(counts, torch.int32), [float(v) for v in nms], [float(v) for v in sap], bufs["flag"][1], bufs["kept"][1],
                             bufs["score"][1], bufs["seen"][1], slot)
    torch.cuda.synchronize()
    for k, (raw, _) in bufs.items():
        assert bool((raw[:GUARD] == FILL).all()) and bool((raw[-GUARD:] == FILL).all()), "bytes beside %s were written" % k
    return {k: v[1].cpu().numpy() for k, v in bufs.items()}, bufs


def check_against(out, b_slot, kept, kept_lines, flag, size, what):
    """One image slot of the kernel's outputs against (T,Q) kept, (T,Q,4) lines, (T,S,Q) flags."""
    got_flag, got_lines = out["flag"][:, :, b_slot], out["kept"][:, b_slot]
    got_kept = (got_flag != 2).any(1) | (got_lines != 0).any(-1)                    # kept by the NMS (scored, or behind the second trim)
    assert (got_kept == kept).all(), what
    assert (got_flag == flag).all(), what
    scale = np.array([size[0], size[1], size[0], size[1]]) / 128.0
    err = float(np.abs((got_lines - kept_lines) * scale).max())
    print("%s: clipped lines off by %.3g px" % (what, err))
    assert err <= LINE_TOL, what


def test_kernel_equals_the_reference_fixture(dev, gold):
    B = len(gold["sizes"])
    out, _ = run_kernel(dev, gold["pred_logits"], gold["pred_lines"], gold["sizes"], gold["gt_lines"], gold["gt_counts"],
                        gold["nms_thresholds"], gold["sap_thresholds"])
    for b in range(B):
        check_against(out, b, gold["kept"][:, b], gold["kept_lines"][:, b], gold["flag"][:, :, b], gold["sizes"][b], "image %d" % b)
    want = torch.softmax(torch.from_numpy(gold["pred_logits"]).to(dev), -1)[..., 0].cpu().numpy()
    diff = int((out["score"].view(np.int32) != want.view(np.int32)).sum())
    print("scores that differ from torch.softmax on the device in any bit: %d of %d" % (diff, want.size))
    assert diff == 0
    assert (out["seen"] == gold["gt_counts"]).all()


def test_kernel_writes_its_slots_only(dev, gold):
    B, cap, slot = len(gold["sizes"]), len(gold["sizes"]) + 5, 3
    out, bufs = run_kernel(dev, gold["pred_logits"], gold["pred_lines"], gold["sizes"], gold["gt_lines"], gold["gt_counts"],
                           gold["nms_thresholds"], gold["sap_thresholds"], cap=cap, slot=slot)
    for b in range(B):
        check_against(out, slot + b, gold["kept"][:, b], gold["kept_lines"][:, b], gold["flag"][:, :, b], gold["sizes"][b], "slot %d" % (slot + b))
    outside = [i for i in range(cap) if not slot <= i < slot + B]
    assert bool((bufs["flag"][1][:, :, outside] == FILL).all())
    assert bool((bufs["kept"][1][:, outside].contiguous().view(torch.uint8) == FILL).all())
    assert bool((bufs["score"][1][outside].contiguous().view(torch.uint8) == FILL).all())
    assert bool((bufs["seen"][1][outside].contiguous().view(torch.uint8) == FILL).all())


@pytest.mark.parametrize("B,Q,G,ld", [(2, 1, 3, 6), (1, 1024, 40, 6), (3, 100, 0, 4), (32, 100, 16, 6), (2, 257, 1024, 4)])
def test_kernel_equals_the_restatement_at_other_sizes(dev, B, Q, G, ld):
    logits, lines, sizes, gts, counts = R.random_case(B, Q, G, seed=B * 1000 + Q + G)
    if B > 2:
        sizes[2] = (427, 569)
    lines = np.ascontiguousarray(lines[:, :, :ld])
    out, _ = run_kernel(dev, logits, lines, sizes, gts, counts)
    for b in range(B):
        kept, kept_lines, flag = R.image_chain(lines[b], sizes[b], gts[b, :counts[b]])
        check_against(out, b, kept, kept_lines, flag, sizes[b], "B %d Q %d G %d image %d" % (B, Q, G, b))
        if Q >= 100:
            assert kept.any() and not kept[:, :Q].all(), "the case exercises nothing"
    assert (out["seen"] == counts).all()


def test_four_thresholds_of_either_kind_at_the_largest_size(dev):
    """T = S = 4 at Q = 1024: the largest LDS footprint the entry point accepts (80 KB of dynamic LDS)."""
    nms, sap = (0.005, 0.010, 0.015, 0.020), (2, 5, 10, 15)
    logits, lines, sizes, gts, counts = R.random_case(1, 1024, 40, seed=4444, size=(427, 569))
    out, _ = run_kernel(dev, logits, lines, sizes, gts, counts, nms, sap)
    kept, kept_lines, flag = R.image_chain(lines[0], sizes[0], gts[0], nms, sap)
    check_against(out, 0, kept, kept_lines, flag, sizes[0], "T 4 S 4 Q 1024")
    assert all((flag == v).any() for v in (0, 1, 2))


def test_kernel_refuses_what_it_cannot_hold(dev):
    logits, lines, sizes, gts, counts = R.random_case(1, 1025, 2, seed=5)
    with pytest.raises(RuntimeError, match="-2"):
        run_kernel(dev, logits, lines, sizes, gts, counts)
    logits, lines, sizes, gts, counts = R.random_case(1, 8, 1025, seed=6)
    with pytest.raises(RuntimeError, match="-2"):
        run_kernel(dev, logits, lines, sizes, gts, counts)
    logits, lines, sizes, gts, counts = R.random_case(2, 8, 2, seed=7)
    with pytest.raises(ValueError):
        run_kernel(dev, logits, lines, sizes, gts, counts, cap=3, slot=2)              # the second image has no slot


def sync_debug_mode_works():
    torch.cuda.set_sync_debug_mode("error")
    try:
        torch.ones(2, device="cuda").sum().item()
        return False
    except RuntimeError:
        return True
    finally:
        torch.cuda.set_sync_debug_mode("default")


def feed(lm, gold, dev, splits):
    t = lambda k, dt: torch.from_numpy(gold[k]).to(dev).to(dt)
    ops = (t("pred_logits", torch.float32), t("pred_lines", torch.float32), t("sizes", torch.int32), t("gt_lines", torch.float32),
           t("gt_counts", torch.int32))
    torch.cuda.synchronize()
    strict = sync_debug_mode_works()
    lo = 0
    for n in splits:
        batch = [o[lo:lo + n].contiguous() for o in ops]
        if strict:
            torch.cuda.set_sync_debug_mode("error")
        try:
            lm.update(*batch)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        lo += n
    assert lo == len(gold["sizes"]) and lm.images_seen == lo
    return strict


@pytest.mark.parametrize("splits,capacity", [((6,), 256), ((1, 3, 2), 256), ((1, 3, 2), 1)])
def test_line_metrics_batches_give_the_fixture_values(dev, gold, splits, capacity):
    lm = LineMetrics(dev, gold["nms_thresholds"], gold["sap_thresholds"], capacity_images=capacity)
    strict = feed(lm, gold, dev, splits)
    print("update() ran under set_sync_debug_mode('error'): %s" % strict)
    stats = lm.compute()
    check_stats(stats, gold)
    assert stats["n_gt"] == int(gold["gt_counts"].sum())
    err = float(np.abs(lm.kept_lines().cpu().numpy() - gold["kept_lines"]).max())
    assert err <= LINE_TOL * 128 / 640
    lm.reset()
    feed(lm, gold, dev, (6,))
    check_stats(lm.compute(), gold)


def test_evaluate_line_ap_module_and_session(dev):
    """evaluate(..., line_ap) through the module and through an InferenceSession over it: the same line stats, fp32."""
    from gw_depth_amd.infer import InferenceSession
    from gw_depth_amd.model import NestedTensor
    from gw_depth_amd.synth import synth_batch
    from tests.golden_check import build
    cfg, model, crits = build(device="cuda")
    loader = []
    for seed, sizes in ((211, [(96, 128), (80, 104)]), (212, None)):
        b = synth_batch(2, 96, 128, seed=seed, n_lines=[3, 4], sizes=sizes)
        loader.append((NestedTensor(b["images"], b["pad_mask"]), NestedTensor(b["depth"], b["pad_mask"]),
                       NestedTensor(b["seg"], b["pad_mask"]), b["targets"], ["synthetic\n"]))
    flags = {"with_line": True, "with_dense": True, "min_depth_eval": 1e-3, "max_depth_eval": 10.0}
    model.compute_dtype = torch.float32
    before = evaluate(model, crits, None, loader, None, "cuda", None, type("A", (), dict(flags))())
    args = type("A", (), dict(flags, line_ap=True))()
    want = evaluate(model, crits, None, loader, None, "cuda", None, args)
    sess = InferenceSession(model, compute_dtype=torch.float32, graph=True)
    got = evaluate(sess, crits, None, loader, None, "cuda", None, args)
    line_keys = sorted(set(want) - set(before))
    print("line keys:", {k: want[k] for k in line_keys})
    assert line_keys == sorted(["n_gt"] + [R.key(k, s, t) for k in ("sAP", "sF") for s in (5, 10, 15) for t in (0.010, 0.015)])
    assert want["n_gt"] == 14 and sorted(got) == sorted(want)
    for k in before:
        assert abs(want[k] - before[k]) <= 2e-5 * max(1.0, abs(before[k])), k        # the flag changes nothing else (fp32 rerun bar)
    for k in line_keys:
        print("%-16s module %.12g session %.12g" % (k, want[k], got[k]))
        assert got[k] == want[k], k
