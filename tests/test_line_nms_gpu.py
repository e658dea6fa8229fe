"""GPU: gwd_line_nms (csrc/linenms.hip), ops.line_nms and InferenceSession(line_nms=...) against tests/golden/line_nms.npz - what the
reference's own postprocess returned on float64 arrays - and, at the shapes the fixture does not hold, against tests/line_nms_ref.py.

Bars (fixed before any run): nms_ids and nms_count identical; lines within 1e-9 px (f64, about 20 operations on coordinates below 2e3:
an error near 1e-13, the bar is 1e4 times that); nms_scores bit-equal to gwd_line_postprocess's scores of the same queries; rows from
nms_count on 0 / 0 / -1; 64 sentinel bytes either side of every output untouched.  The restatement is handed the scores the device
computed, so the order and the floor are decided on the same bits.  Every measured figure is printed before it is asserted."""
import numpy as np
import pytest
import torch

from gw_depth_amd import hip, ops
from gw_depth_amd.infer import NMS_KEYS, RESULT_KEYS, InferenceSession
from gw_depth_amd.model import NestedTensor
from tests import line_nms_ref as N
from tests.test_line_nms import GOLDEN, LINE_TOL, case_of

pytestmark = pytest.mark.gpu
GUARD, FILL = 64, 0xA5


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


def run_kernel(dev, logits, lines, sizes, t, by_score=False, min_score=None, twin=0):
    """One gwd_line_nms call into guarded buffers.  Returns the four outputs as NumPy arrays, and gwd_line_postprocess's scores and
    order of all B + twin images (the order is what the call was given when by_score)."""
    tt = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).to(dev)
    logits, lines, sizes = tt(logits, torch.float32), tt(lines, torch.float32), tt(sizes, torch.int32)
    Bs, Q, _ = lines.shape
    B, C = Bs - twin, Q * (2 if twin else 1)
    scores, _, order, _ = ops.line_postprocess(logits, lines, torch.cat([sizes, sizes[:twin]]), 0.6)
    bufs = {"nms_lines": guarded((B, C, 4), torch.float64, dev), "nms_scores": guarded((B, C), torch.float32, dev),
            "nms_ids": guarded((B, C), torch.int32, dev), "nms_count": guarded((B,), torch.int32, dev)}
    hip.library().line_nms(logits, lines, sizes, order if by_score else None, t, min_score, *(bufs[k][1] for k in NMS_KEYS), twin)
    torch.cuda.synchronize()
    for k, (raw, _) in bufs.items():
        assert bool((raw[:GUARD] == FILL).all()) and bool((raw[-GUARD:] == FILL).all()), "bytes beside %s were written" % k
    return [bufs[k][1].cpu().numpy() for k in NMS_KEYS], scores.cpu().numpy(), order.cpu().numpy()


def check(got, want, dev_scores, twin, what):
    """got / want: (lines, scores, ids, count).  The scores are compared with gwd_line_postprocess's, bit for bit."""
    lines, scores, ids, count = got
    w_lines, _, w_ids, w_count = want
    print("%s: kept %s of %d rows" % (what, count.tolist(), ids.shape[1]))
    assert (count == w_count).all(), what
    assert (ids == w_ids).all(), what
    err = float(np.abs(lines - w_lines).max())
    print("%s: clipped lines off by %.3g px" % (what, err))
    assert err <= LINE_TOL, what
    Q = dev_scores.shape[1]
    for b in range(len(count)):
        k = int(count[b])
        assert (lines[b, k:] == 0).all() and (scores[b, k:].view(np.int32) == 0).all() and (ids[b, k:] == -1).all(), what
        src = dev_scores[np.where(ids[b, :k] >= Q, b + twin, b), ids[b, :k] % Q]
        assert (scores[b, :k].view(np.int32) == src.view(np.int32)).all(), what


def against_restatement(dev, logits, lines, sizes, t, by_score, min_score, twin, what):
    got, dev_scores, order = run_kernel(dev, logits, lines, sizes, t, by_score, min_score, twin)
    want = N.line_nms(dev_scores, lines, sizes, t, order if by_score else None, min_score, twin)
    check(got, want, dev_scores, twin, what)
    return got


def test_kernel_equals_the_reference_fixture(dev, gold):
    for name in gold["cases"]:
        c = case_of(gold, name)
        got, dev_scores, order = run_kernel(dev, c["logits"], c["lines"], c["sizes"], c["t"], c["by_score"], c["min_score"], c["twin"])
        if c["by_score"]:                                  # the fixture's order is the host softmax's: the device ranks the same way
            assert (order == np.stack([N.score_order(s) for s in c["scores"]])).all(), name
        if c["min_score"] is not None:
            assert ((dev_scores > c["min_score"]) == (c["scores"] > c["min_score"])).all(), name
        check(got, (c["nms_lines"], None, c["ids"], c["count"]), dev_scores, c["twin"], name)


@pytest.mark.parametrize("B,Q,ld,by_score", [(1, 1, 6, False), (1, 2, 4, True), (3, 63, 6, True), (1, 64, 6, False), (3, 65, 4, False),
                                             (32, 100, 6, True), (3, 129, 6, True), (1, 1024, 6, False), (1, 1024, 4, True)])
def test_kernel_equals_the_restatement_at_other_sizes(dev, B, Q, ld, by_score):
    logits, lines, sizes = N.random_case(B, Q, seed=7000 + 10 * Q + B, ld=ld)
    if B > 2:
        sizes[2] = (427, 569)
    t = 0.015 if Q % 2 else 0.010
    got = against_restatement(dev, logits, lines, sizes, t, by_score, None, 0, "B %d Q %d ld %d by_score %s" % (B, Q, ld, by_score))
    if Q >= 63:
        assert (got[3] < Q).all() and (got[3] > 1).all(), "the case exercises nothing"


@pytest.mark.parametrize("by_score", [False, True], ids=["query", "score"])
def test_twin_at_the_largest_size(dev, by_score):
    """Q = 512 with a twin: 1024 candidates, every LDS table full."""
    logits, lines, sizes = N.random_case(2, 512, seed=5120, ld=6, twin=True)
    sizes[1] = (427, 569)
    got = against_restatement(dev, logits, lines, sizes, 0.010, by_score, 0.2 if by_score else None, 2, "twin Q 512 by_score %s" % by_score)
    assert (got[2] >= 512).any() and (got[3] > 1).all()


def horizontal(rows):
    """(x1, y, x2, y) per row, 6 wide."""
    a = np.array([[x1, y, x2, y, (x1 + x2) / 2, y] for x1, x2, y in rows], np.float32)
    return a[None]


def test_edge_inputs(dev):
    sizes = np.array([[480, 640]], np.int32)
    r = np.random.RandomState(3)
    logit = lambda q: r.normal(0, 2, (1, q, 2)).astype(np.float32)
    # all candidates suppressed but the first: sub-segments of line 0 (never equal to it, so the trim leaves them in; none of
    # zero length, which the reference keeps)
    inside = horizontal([(0.1, 0.9, 0.5)] + [(0.2 + 0.005 * k, 0.8 - 0.005 * k, 0.5) for k in range(69) if k != 60])
    got = against_restatement(dev, logit(69), inside, sizes, 0.010, False, None, 0, "all but the first suppressed")
    assert got[3].tolist() == [1] and got[2][0, 0] == 0
    # none suppressed: parallel lines 24 px apart (the threshold is 8 px)
    apart = horizontal([(0.1, 0.9, 0.05 + 0.05 * k) for k in range(18)])
    for by_score in (False, True):
        got = against_restatement(dev, logit(18), apart, sizes, 0.010, by_score, None, 0, "none suppressed")
        assert got[3].tolist() == [18]
    # a floor above every score
    got = against_restatement(dev, logit(18), apart, sizes, 0.010, True, 1.5, 0, "floor above every score")
    assert got[3].tolist() == [0] and (got[2] == -1).all() and (got[0] == 0).all()
    # NaN logits: such a query has a NaN score; without a floor it is a candidate (first in score order), with one it never is
    lg = logit(18)
    lg[0, 3, 0] = lg[0, 11, 1] = np.nan
    for by_score in (False, True):
        got = against_restatement(dev, lg, apart, sizes, 0.010, by_score, None, 0, "NaN logits, no floor")
        assert got[3].tolist() == [18] and np.isnan(got[1][0]).sum() == 2
        if by_score:
            assert sorted(got[2][0, :2].tolist()) == [3, 11]
    got = against_restatement(dev, lg, apart, sizes, 0.010, True, -1.0, 0, "NaN logits, floor -1")
    assert got[3].tolist() == [16] and not np.isnan(got[1]).any()
    # a repeat of line 0 at i = 1: one candidate
    rep = apart.copy()
    rep[0, 1] = rep[0, 0]
    for by_score in (False, True):
        got = against_restatement(dev, logit(18), rep, sizes, 0.010, by_score, None, 0, "repeat of line 0 at 1")
        assert got[3].tolist() == [1] and got[2][0, 0] == 0


def test_refusals(dev):
    on = lambda *arrays: [torch.from_numpy(a).to(dev) for a in arrays]
    with pytest.raises(RuntimeError, match="-2"):
        ops.line_nms(*on(*N.random_case(1, 1025, seed=5)), 0.01)
    with pytest.raises(RuntimeError, match="-2"):
        ops.line_nms(*on(*N.random_case(1, 513, seed=6, twin=True)), 0.01, twin=1)


# ---------------------------------------------------------------------------------------------------------------------- the session
def sync_debug_mode_works():
    torch.cuda.set_sync_debug_mode("error")
    try:
        torch.ones(2, device="cuda").sum().item()
        return False
    except RuntimeError:
        return True
    finally:
        torch.cuda.set_sync_debug_mode("default")


def want_from_raw(raw, sizes, t, twin=0):
    """The restatement on a forward's raw outputs, in score order, on the device's own scores and ranking."""
    logits, lines = raw["pred_logits"].float(), raw["pred_lines"].float()
    sz = torch.as_tensor(sizes, dtype=torch.int32, device=logits.device)
    scores, _, order, _ = ops.line_postprocess(logits, lines, torch.cat([sz, sz[:twin]]), 0.6)
    return N.line_nms(scores.cpu().numpy(), lines.cpu().numpy(), np.asarray(sizes), t, order.cpu().numpy(), None, twin), scores.cpu().numpy()


def check_result(res, raw, sizes, t, twin, what):
    want, dev_scores = want_from_raw(raw, sizes, t, twin)
    torch.cuda.synchronize()
    check([res[k].cpu().numpy() for k in NMS_KEYS], want, dev_scores, twin, what)


@pytest.fixture(scope="module")
def model():
    from tests.golden_check import build
    hip.set_library(None)
    return build(device="cuda")[1]


def test_session_eager_capture_and_replays(model):
    from gw_depth_amd.synth import synth_batch
    b = synth_batch(2, 96, 128, seed=31)
    nt = NestedTensor(b["images"].cuda(), b["pad_mask"].cuda())
    sizes, t = [(96, 128), (96, 128)], 0.010
    eager = InferenceSession(model, compute_dtype=torch.float32, graph=False, line_nms=t)
    raw, post = eager._run(nt, None, True)
    check_result(post, raw, sizes, t, 0, "eager")
    assert tuple(post) == RESULT_KEYS + NMS_KEYS
    sess = InferenceSession(model, compute_dtype=torch.float32, graph=True, line_nms=t)
    first = sess.predict(nt, copy=True)                    # warms up, captures, replays
    assert sess.graphs[(2, 96, 128)]["captured"], sess.graphs
    check_result(first, sess._graphs[(2, 96, 128)]["result"][0], sizes, t, 0, "capturing call")
    second = sess.predict(nt, copy=True)
    torch.cuda.synchronize()
    strict = sync_debug_mode_works()
    assert strict, "set_sync_debug_mode('error') does not catch a sync here: the no-host-sync check of the replay cannot be made"
    torch.cuda.set_sync_debug_mode("error")
    try:
        third = sess.predict(nt, copy=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    check_result(third, sess._graphs[(2, 96, 128)]["result"][0], sizes, t, 0, "second replay")
    for k in RESULT_KEYS + NMS_KEYS:
        for name, other in (("eager", post), ("replay 1", second), ("replay 2", third)):
            assert torch.equal(first[k].view(torch.uint8), other[k].view(torch.uint8)), (k, name)
    # a session without line_nms equals a plain session on every existing key, bit for bit
    plain = InferenceSession(model, compute_dtype=torch.float32, graph=True).predict(nt, copy=True)
    none = InferenceSession(model, compute_dtype=torch.float32, graph=True, line_nms=None, line_nms_order="query").predict(nt, copy=True)
    torch.cuda.synchronize()
    assert tuple(plain) == tuple(none) == RESULT_KEYS
    for k in RESULT_KEYS:
        assert torch.equal(plain[k].view(torch.uint8), none[k].view(torch.uint8)), k
        assert torch.equal(plain[k].view(torch.uint8), first[k].view(torch.uint8)), k


def test_predict_frames_ensemble_with_line_nms(model):
    g = torch.Generator().manual_seed(11)
    frames = [torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, generator=g) for h, w in ((72, 110), (100, 60))]
    fs, t = [(72, 110), (100, 60)], 0.015
    sess = InferenceSession(model, compute_dtype=torch.bfloat16, graph=True, line_nms=t)
    for ensemble in (True, False):
        res = sess.predict_frames(frames, size=96, max_size=128, ensemble=ensemble, copy=True)
        torch.cuda.synchronize()
        key = (4, 128, 128, "twin") if ensemble else (2, 128, 128)
        assert sess.graphs[key]["captured"], sess.graphs
        Q = res["scores"].shape[1]
        assert res["nms_ids"].shape == (2, 2 * Q if ensemble else Q)
        check_result(res, sess._graphs[key]["result"][0], fs, t, 2 if ensemble else 0, "predict_frames ensemble %s" % ensemble)
        assert sorted(res) == sorted(RESULT_KEYS + NMS_KEYS + ("net_sizes",))
