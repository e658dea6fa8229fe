"""CPU: line NMS on the device (gwd_line_nms, ops.line_nms, InferenceSession(line_nms=...)) - everything that needs no GPU.

  * the NumPy restatement tests/line_nms_ref.py against tests/golden/line_nms.npz, which holds what the reference's OWN postprocess
    returned (tools/make_golden_linenms.py): ids and counts identical, lines within 1e-9 px (f64, about 20 operations on coordinates
    below 2e3: an error near 1e-13; the bar is 1e4 times that, as for the line scorer);
  * header, binding and library agree on the entry point; it refuses bad arguments before any launch (there is no GPU here);
  * the session's plumbing on a CPU stand-in of the device library: the default session is today's, line_nms adds four keys.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

from gw_depth_amd import hip, infer, ops
from gw_depth_amd.infer import RESULT_KEYS, InferenceSession
from tests import line_nms_ref as N

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "line_nms.npz")
LINE_TOL = 1e-9
NMS_KEYS = ("nms_lines", "nms_scores", "nms_ids", "nms_count")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLDEN))


def case_of(gold, name):
    c = {k[len(name) + 1:]: v for k, v in gold.items() if k.startswith(name + "/")}
    c["min_score"] = None if np.isnan(c["min_score"]) else float(c["min_score"])
    c["t"], c["twin"], c["by_score"] = float(c["t"]), int(c["twin"]), bool(c["by_score"])
    return c


def order_of(scores):
    return np.stack([N.score_order(s) for s in scores])


def check_rows(got, want_lines, want_ids, want_count, what):
    lines, _, ids, count = got
    assert (count == want_count).all(), what
    assert (ids == want_ids).all(), what
    err = float(np.abs(lines - want_lines).max())
    print("%s: kept %s, clipped lines off by %.3g px" % (what, count.tolist(), err))
    assert err <= LINE_TOL, what


def test_fixture_covers_the_cases(gold):
    names = list(gold["cases"])
    assert len(names) == 11 and os.path.getsize(GOLDEN) < 256 * 1024
    cases = {n: case_of(gold, n) for n in names}
    assert {c["t"] for c in cases.values()} == {0.010, 0.015}
    assert any(c["by_score"] for c in cases.values()) and any(not c["by_score"] for c in cases.values())
    sizes = {tuple(s) for c in cases.values() for s in c["sizes"].tolist()}
    assert {(480, 640), (427, 569), (720, 1280), (128, 128)} <= sizes
    assert cases["floor_0010"]["min_score"] == 0.5 and cases["twin_score_0015"]["twin"] == 2
    assert cases["twin_query_0010"]["lines"].shape == (4, 100, 4) and (cases["twin_query_0010"]["ids"] >= 100).any()
    assert N.first_repeat(cases["repeat_0015"]["lines"][0]) == 70 and N.first_repeat(cases["exact_query_0010"]["lines"][0]) == 15
    for n, c in cases.items():
        C = c["ids"].shape[1]
        assert (c["count"] > 0).all() and (c["count"] < C).all(), n                  # something is suppressed or left out everywhere
        whole = N.pixels(c["lines"][0], c["sizes"][0])[:, :, ::-1].reshape(-1, 4).astype(np.float64)
        own = c["ids"][0][:c["count"][0]]
        own_rows = np.nonzero(own < 100)[0]
        if n.startswith(("query", "score", "twin", "exact")):
            assert (np.abs(c["nms_lines"][0][own_rows] - whole[own[own_rows]]).max(-1) > 1e-3).any(), n      # a clipped line
    s = cases["score_0010"]["scores"]
    assert any(len(np.unique(row)) < len(row) for row in s)                          # equal scores: the order's tie rule is used


def test_restatement_equals_the_reference(gold):
    for name in gold["cases"]:
        c = case_of(gold, name)
        order = order_of(c["scores"]) if c["by_score"] else None
        got = N.line_nms(c["scores"], c["lines"], c["sizes"], c["t"], order, c["min_score"], c["twin"])
        check_rows(got, c["nms_lines"], c["ids"], c["count"], name)
        k = c["count"]
        for b in range(len(k)):
            assert (got[0][b, k[b]:] == 0).all() and (got[1][b, k[b]:] == 0).all() and (got[2][b, k[b]:] == -1).all()
            src = c["scores"].reshape(-1, 100)
            ids = c["ids"][b, :k[b]]
            assert (got[1][b, :k[b]] == src[np.where(ids >= 100, b + c["twin"], b), ids % 100]).all()


def test_header_binding_and_library_agree():
    from tests.test_abi_surface import declared_entry_points
    assert "gwd_line_nms" in hip.ENTRY_POINTS and "gwd_line_nms" in declared_entry_points()
    text = open(os.path.join(ROOT, "include", "gwdepth.h")).read()
    assert "#define GWD_VERSION 10" in text
    lib = hip.HipLibrary()
    assert lib.version() == 10
    assert len(lib.lib.gwd_line_nms.argtypes) == 15 and lib.lib.gwd_line_nms.argtypes[4] is ctypes.c_double


def test_entry_point_refuses_before_any_launch():
    """Every call below must return before the launch: this host has no device to launch on."""
    lib = hip.HipLibrary().lib
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    nan = float("nan")

    def call(logits=p, lines=p, sizes=p, order=None, t=0.01, floor=nan, o1=p, o2=p, o3=p, o4=p, B=1, Q=4, ld=4, twin=0):
        return lib.gwd_line_nms(logits, lines, sizes, order, t, floor, o1, o2, o3, o4, B, Q, ld, twin, None)

    for k in ("logits", "lines", "sizes", "o1", "o2", "o3", "o4"):
        assert call(**{k: None}) == -1, k
    assert call(ld=5) == -1 and call(ld=3) == -1
    assert call(B=0) == -1 and call(Q=0) == -1
    assert call(B=2, twin=1) == -1 and call(B=2, twin=3) == -1 and call(twin=-1) == -1
    assert call(t=-0.01) == -1 and call(t=nan) == -1
    assert call(Q=1025) == -2 and call(Q=513, twin=1) == -2 and call(Q=2 ** 30, twin=1) == -2


def test_wrapper_checks_shapes_and_needs_the_device():
    hip.set_library(None)
    z = torch.zeros
    with pytest.raises(hip.HipUnavailable):
        ops.line_nms(z(1, 4, 2), z(1, 4, 6), z(1, 2, dtype=torch.int32), 0.01)
    with pytest.raises(ValueError):
        ops.line_nms(z(3, 4, 2), z(3, 4, 6), z(1, 2, dtype=torch.int32), 0.01, twin=2)
    lib = hip.library()
    out = (z(1, 4, 4, dtype=torch.float64), z(1, 4), z(1, 4, dtype=torch.int32), z(1, dtype=torch.int32))
    with pytest.raises(ValueError):
        lib.line_nms(z(1, 4, 2), z(1, 4, 6), z(2, 2, dtype=torch.int32), None, 0.01, None, *out, 0)
    with pytest.raises(TypeError):
        lib.line_nms(z(1, 4, 2), z(1, 4, 6), z(1, 2, dtype=torch.int64), None, 0.01, None, *out, 0)


@pytest.fixture
def fake():
    from tests.line_nms_fake import LineNmsFakeDevice
    lib = LineNmsFakeDevice()
    hip.set_library(lib)
    yield lib
    hip.set_library(None)


def images(B=2, H=24, W=32, seed=0):
    return torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(seed))


def test_default_session_is_todays(fake):
    from tests.test_frames_post import FramesFakeDevice, TinyModel
    x = images()
    plain = InferenceSession(TinyModel(), compute_dtype=torch.float32, graph=False).predict(x)
    assert fake.nms_calls == [] and tuple(plain) == RESULT_KEYS and infer.RESULT_KEYS == (
        "depth", "depth_mm", "labels", "scores", "lines", "order", "count", "sizes")
    hip.set_library(FramesFakeDevice())                                              # the stand-in without the new call: not needed
    old = InferenceSession(TinyModel(), compute_dtype=torch.float32, graph=False, line_nms=None).predict(x)
    hip.set_library(fake)
    with_nms = InferenceSession(TinyModel(), compute_dtype=torch.float32, graph=False, line_nms=0.01).predict(x)
    for k in RESULT_KEYS:
        assert torch.equal(plain[k], old[k]) and torch.equal(plain[k], with_nms[k]), k


def test_line_nms_adds_four_keys(fake):
    from tests.test_frames_post import TinyModel
    x = images()
    Q = TinyModel.Q
    sess = InferenceSession(TinyModel(), compute_dtype=torch.float32, graph=False, line_nms=0.01)
    res = sess.predict(x, target_sizes=[(48, 64), (30, 40)])
    assert tuple(res) == RESULT_KEYS + NMS_KEYS == RESULT_KEYS + infer.NMS_KEYS
    assert fake.nms_calls == [{"threshold": 0.01, "by_order": True, "min_score": None, "twin": 0, "sizes": [[48, 64], [30, 40]]}]
    assert res["nms_lines"].shape == (2, Q, 4) and res["nms_lines"].dtype == torch.float64
    assert res["nms_scores"].shape == (2, Q) and res["nms_ids"].dtype == torch.int32 and res["nms_count"].shape == (2,)
    raw = sess(x)
    scores = torch.softmax(raw["pred_logits"], -1)[..., 0].numpy()
    want = N.line_nms(scores, raw["pred_lines"].numpy(), [(48, 64), (30, 40)], 0.01, res["order"].numpy())
    for k, w in zip(NMS_KEYS, want):
        assert np.array_equal(res[k].numpy(), w), k
    assert int(res["nms_count"].min()) >= 1
    # the options reach the call
    sess = InferenceSession(TinyModel(), compute_dtype=torch.float32, graph=False, line_nms=0.015, line_nms_order="query",
                            line_nms_min_score=0.45)
    res = sess.predict(x)
    assert fake.nms_calls[-1] == {"threshold": 0.015, "by_order": False, "min_score": 0.45, "twin": 0, "sizes": [[24, 32], [24, 32]]}
    k = int(res["nms_count"][0])
    assert bool((res["nms_scores"][0, :k] > 0.45).all()) and bool((res["nms_ids"][0, :k].diff() > 0).all())
    for bad in ({"line_nms_order": "best"}, {"line_nms": -0.1}, {"line_nms": float("nan")}):
        with pytest.raises(ValueError):
            InferenceSession(TinyModel(), compute_dtype=torch.float32, graph=False, **bad)


def test_copy_clones_the_nms_results(fake, monkeypatch):
    from tests.test_frames_post import TinyModel
    sess = InferenceSession(TinyModel(), compute_dtype=torch.float32, graph=False, line_nms=0.01)
    held = {}
    post = sess._post

    def keeping(*a, **k):
        held.update(post(*a, **k))
        return held

    monkeypatch.setattr(sess, "_post", keeping)
    x = images()
    same = sess.predict(x)
    fresh = sess.predict(x, copy=True)
    for k in NMS_KEYS + ("lines",):
        assert same[k].data_ptr() == held[k].data_ptr(), k
        assert fresh[k].data_ptr() != held[k].data_ptr() and torch.equal(fresh[k], held[k]), k


@pytest.mark.parametrize("ensemble", [False, True], ids=["plain", "ensemble"])
def test_predict_frames_passes_the_twin_and_the_frame_sizes(fake, ensemble):
    from tests.test_frames_post import TinyModel, frames_of
    frames, Q = frames_of(3), TinyModel.Q
    fs = [list(f.shape[:2]) for f in frames]
    sess = InferenceSession(TinyModel(), compute_dtype=torch.float32, graph=False, line_nms=0.01)
    for copy in (False, True):
        res = sess.predict_frames(frames, size=48, max_size=64, ensemble=ensemble, copy=copy)
        assert sorted(res) == sorted(RESULT_KEYS + NMS_KEYS + ("net_sizes",))
        assert fake.nms_calls[-1]["twin"] == (3 if ensemble else 0) and fake.nms_calls[-1]["sizes"] == fs
        C = 2 * Q if ensemble else Q
        assert res["nms_lines"].shape == (3, C, 4) and res["nms_ids"].shape == (3, C) and res["nms_count"].shape == (3,)
        assert res["scores"].shape == (3, Q)
    # without line_nms the twin's lines stay unused, and no NMS runs
    n = len(fake.nms_calls)
    res = InferenceSession(TinyModel(), compute_dtype=torch.float32, graph=False).predict_frames(frames, size=48, max_size=64, ensemble=ensemble)
    assert sorted(res) == sorted(RESULT_KEYS + ("net_sizes",)) and len(fake.nms_calls) == n
