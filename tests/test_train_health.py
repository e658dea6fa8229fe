"""CPU: the host side of the guarded optimizer step (gw_depth_amd/health.py, engine.TrainStep(guard=..., stats_every=...),
checkpoint.FlatAdamW) over tests/health_fake.py, and the fp64 restatement of the kernels (tests/health_ref.py) on hand cases."""
import math
import os
import re

import numpy as np
import pytest
import torch

from gw_depth_amd import health as H
from gw_depth_amd import hip
from gw_depth_amd.checkpoint import FlatAdamW
from gw_depth_amd.engine import ALIGN, TrainStep
from tests import health_ref as R
from tests.golden_check import build
from tests.health_fake import HealthFakeDevice

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CH = hip.HEALTH_CHUNK
NEW_CALLS = {"segment_stats", "health_decide", "adamw_step_guarded"}


@pytest.fixture()
def fake():
    dev = HealthFakeDevice()
    hip.set_library(dev)
    yield dev
    hip.set_library(None)


def _fake_grads(step, seed):
    g = torch.Generator().manual_seed(seed)
    r = torch.randn(step.flat_g.shape, generator=g) * 1e-3
    step.flat_g.zero_()
    for n, p in step.params.items():
        o = step.offsets[n]
        step.flat_g[o:o + p.numel()].copy_(r[o:o + p.numel()])


def _state(step):
    return [t.clone() for t in (step.flat_p, step.flat_m, step.flat_v)] + ([] if step.flat_p16 is None else [step.flat_p16.clone()])


def _same(step, saved):
    now = [step.flat_p, step.flat_m, step.flat_v] + ([] if step.flat_p16 is None else [step.flat_p16])
    return all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(now, saved))


def _check_cover(begin, end, chunks, chunk):
    """Every segment covered exactly once, no piece straddles a segment or touches padding, every piece at most `chunk` long."""
    covered = {s: [] for s in range(len(begin))}
    for c in chunks:
        s, b, n = int(c["segment"]), int(c["begin"]), int(c["len"])
        assert 1 <= n <= chunk and begin[s] <= b and b + n <= end[s], (s, b, n)
        assert b % 8 == 0
        covered[s].append((b, b + n))
    assert [int(c["segment"]) for c in chunks] == sorted(int(c["segment"]) for c in chunks)       # segment order
    for s, spans in covered.items():
        pos = begin[s]
        for lo, hi in spans:                                     # ascending, gap-free, no overlap
            assert lo == pos
            pos = hi
        assert pos == end[s], (s, pos, end[s])


def ragged_table(lengths):
    begin, off = [], 0
    for n in lengths:
        begin.append(off)
        off += (n + ALIGN - 1) // ALIGN * ALIGN + ALIGN * (len(begin) % 3)       # padding of 0, 8 or 16 elements and more
    return begin, [b + n for b, n in zip(begin, lengths)], off


@pytest.mark.parametrize("chunk", [8, 16, CH])
def test_chunk_table_covers_a_ragged_table(chunk):
    lengths = [0, 1, 3, 4, 5, 8, chunk - 1, chunk, chunk + 1, 2 * chunk + 5, 0]
    begin, end, total = ragged_table(lengths)
    chunks = H.chunk_table(begin, end, chunk)
    _check_cover(begin, end, chunks, chunk)
    assert len(chunks) == sum((n + chunk - 1) // chunk for n in lengths)
    H.check_tables(begin, end, chunks, total, chunk)
    broken = chunks.copy()
    broken["len"][-1] += 1                                       # into the padding
    with pytest.raises(ValueError):
        H.check_tables(begin, end, broken, total, chunk)
    with pytest.raises(ValueError):
        H.check_tables(begin, end, chunks[:-1], total, chunk)    # a piece missing


def test_chunk_table_of_the_model_layout(fake):
    cfg, model, crits = build()
    step = TrainStep(model, crits, cfg, guard="skip")
    numels = {n: p.numel() for n, p in step.params.items()}
    begin, end = H.segment_table(step.names, step.offsets, numels)
    assert len(begin) == len(step.names) == 738 and begin[0] == 0 and end[-1] <= step.total
    assert all(e - b == numels[n] for b, e, n in zip(begin, end, step.names))
    chunks = H.chunk_table(begin, end)
    _check_cover(begin, end, chunks, CH)
    hs = step._health
    assert hs.chunks.shape == (len(chunks), 2) and hs.seg_begin.tolist() == begin and hs.seg_end.tolist() == end
    assert hs.partial.numel() == len(chunks) * 16


def test_reference_stats_on_hand_cases():
    nan, inf = float("nan"), float("inf")
    x = torch.tensor([3.0, -4.0, nan, 9.0, 9.0, 9.0, 9.0, 9.0,      # segment 0: [0, 3); the 9s are padding
                      inf, -inf, -0.5, 2.0, 9.0, 9.0, 9.0, 9.0,     # segment 1: [8, 12)
                      1e30, -2e30])                                 # segment 2: [16, 18): squares beyond fp32, finite in fp64
    got = R.segment_stats(x, [0, 8, 16, 24], [3, 12, 18, 24])
    assert got[0] == (25.0, 4.0, 1)
    assert got[1] == (4.25, 2.0, 2)
    assert got[2][0] == float(np.float64(np.float32(1e30)) ** 2 + np.float64(np.float32(2e30)) ** 2) and math.isfinite(got[2][0])
    assert got[2][1:] == (float(np.float32(2e30)), 0)
    assert got[3] == (0.0, 0.0, 0)                                  # an empty segment


def test_reference_decide_on_hand_cases():
    c = R.new_ctl()
    c, rec, bad = R.decide([(9.0, 3.0, 0), (16.0, 4.0, 0)], c, 1.5, 0.9, 0.999, 0.1, 1.0)
    assert (c["sq"], c["apply"], c["applied"], c["skipped"], c["streak"]) == (25.0, 1, 1, 0, 0)
    assert c["bc1"] == float(np.float32(1 - 0.9)) and c["bc2"] == float(np.float32(1 - 0.999))
    assert c["clip_coef"] == float(np.float32(0.1) / (np.float32(5.0) + np.float32(1e-6))) and bad is None
    assert rec == {"step": 1, "apply": True, "grad_norm": 5.0, "clip_coef": c["clip_coef"], "loss": 1.5, "nonfinite_total": 0}
    before = (c["bc1"], c["bc2"])
    c, rec, bad = R.decide([(9.0, 3.0, 2), (16.0, 4.0, 0)], c, float("inf"), 0.9, 0.999, 0.0, 0.5, bad)
    assert (c["apply"], c["applied"], c["skipped"], c["streak"], c["nonfinite_total"]) == (0, 1, 1, 1, 2)
    assert (c["bc1"], c["bc2"]) == before and c["clip_coef"] == 1.0 and c["loss_finite"] == 0 and bad == [2, 0]
    assert rec["step"] == 2 and rec["grad_norm"] == 2.5 and not rec["apply"]
    c, rec, bad = R.decide([(1.0, 1.0, 0), (0.0, 0.0, 0)], c, None, 0.9, 0.999, 0.1, 1.0, bad)
    assert (c["applied"], c["skipped"], c["streak"]) == (2, 1, 0) and bad == [2, 0]             # the culprits of the last skipped step stay
    assert c["bc1"] == float(np.float32(1 - 0.9 ** 2)) and c["clip_coef"] == float(np.float32(0.1) / (np.float32(1.0) + np.float32(1e-6)))


def test_default_step_issues_todays_calls(fake):
    cfg, model, crits = build()
    step = TrainStep(model, crits, cfg)
    assert step._health is None
    _fake_grads(step, 1)
    step.optimizer_step()
    assert fake.calls == ["sqnorm", "adamw_step", "adamw_step"] and not NEW_CALLS & set(fake.calls)
    assert fake.bias_corrections[0] == (1 - 0.9 ** 1, 1 - 0.999 ** 1)
    with pytest.raises(RuntimeError):
        step.health()
    with pytest.raises(ValueError):
        TrainStep(model, crits, cfg, guard="maybe")


def test_stats_every_without_the_guard_adds_passes_every_kth_step(fake):
    cfg, model, crits = build()
    step = TrainStep(model, crits, cfg, stats_every=2)
    _fake_grads(step, 1)
    step.optimizer_step()
    assert fake.calls == ["sqnorm", "adamw_step", "adamw_step"]
    del fake.calls[:]
    step.optimizer_step()
    assert fake.calls == ["sqnorm", "adamw_step", "adamw_step", "segment_stats", "segment_stats"]
    stats = step.tensor_stats()
    n = step.names[3]
    o, k = step.offsets[n], step.params[n].numel()
    gn, gmax, gbad, pn = stats[n]
    assert gn == pytest.approx(float(step.flat_g[o:o + k].double().norm()), rel=1e-12) and gbad == 0
    assert gmax == float(step.flat_g[o:o + k].abs().max()) and pn == pytest.approx(float(step.flat_p[o:o + k].double().norm()), rel=1e-12)


def test_guard_skips_a_poisoned_step_and_keeps_adams_step(fake):
    cfg, model, crits = build()
    step = TrainStep(model, crits, cfg, compute_dtype=torch.bfloat16, guard="skip")
    _fake_grads(step, 1)
    step.optimizer_step()
    assert fake.calls == ["segment_stats", "health_decide", "adamw_step_guarded", "adamw_step_guarded"]
    h = step.health()
    assert (h["applied"], h["skipped"], h["streak"]) == (1, 0, 0) and h["last"]["apply"]
    assert step.grad_norm() == pytest.approx(float(step.flat_g.double().norm()), rel=1e-12)

    saved = _state(step)
    _fake_grads(step, 2)
    victim = step.names[5]
    step.flat_g[step.offsets[victim] + step.params[victim].numel() - 1] = float("inf")
    step.optimizer_step(torch.tensor(2.5))
    assert _same(step, saved)                                    # parameters, both moments and the bf16 shadow
    h = step.health()
    assert (h["applied"], h["skipped"], h["streak"], step.step_count) == (1, 1, 1, 2)
    assert not h["last"]["apply"] and h["last"]["nonfinite_total"] == 1 and h["last"]["loss"] == 2.5 and h["last"]["step"] == 2
    assert step.first_nonfinite() == [victim] and step.tensor_stats()[victim][2] == 1

    _fake_grads(step, 3)
    step.optimizer_step()
    assert not _same(step, saved)
    h = step.health()
    assert (h["applied"], h["skipped"], h["streak"], step.step_count) == (2, 1, 0, 3)
    assert fake.bias_corrections == [R.bias_corrections(0.9, 0.999, 1)] * 2 + [R.bias_corrections(0.9, 0.999, 2)] * 2   # applied + 1, not attempt 3
    assert step.first_nonfinite() == [victim]                    # of the last SKIPPED step
    hist = step.history()
    assert [r["step"] for r in hist] == [1, 2, 3] and [r["apply"] for r in hist] == [True, False, True]
    step.flush()                                                 # a streak of 1 is below the limit: nothing raised


def test_history_ring_wraps_in_step_order(fake):
    cfg, model, crits = build()
    step = TrainStep(model, crits, cfg, guard="skip", ring=4)
    _fake_grads(step, 1)
    for _ in range(6):
        step.optimizer_step()
    assert [r["step"] for r in step.history()] == [3, 4, 5, 6]


def test_a_streak_beyond_the_limit_raises_and_names_the_tensor(fake):
    cfg, model, crits = build()
    step = TrainStep(model, crits, cfg, guard="skip", max_consecutive_skips=2)
    _fake_grads(step, 1)
    victim = step.names[-1]
    step.flat_g[step.offsets[victim]] = float("nan")
    saved = _state(step)
    step.optimizer_step()
    step.optimizer_step()
    step.flush()                                                 # a streak of 2 is allowed
    step.optimizer_step()
    with pytest.raises(FloatingPointError, match=re.escape(victim)):
        step.flush()
    assert _same(step, saved) and step.health()["streak"] == 3


def test_checkpoint_round_trip_carries_the_applied_steps(fake):
    cfg, model, crits = build()
    step = TrainStep(model, crits, cfg, guard="skip")
    opt = FlatAdamW(step)
    for seed, poison in ((1, False), (2, True), (3, False)):
        _fake_grads(step, seed)
        if poison:
            step.flat_g[0] = float("nan")
        opt.step()
    assert step.step_count == 3
    sd = opt.state_dict()
    assert {float(st["step"]) for st in sd["state"].values()} == {2.0}          # applied, not attempted

    cfg2, model2, crits2 = build()
    step2 = TrainStep(model2, crits2, cfg2, guard="skip")
    opt2 = FlatAdamW(step2)
    opt2.load_state_dict(sd)
    h = step2.health()
    assert (h["applied"], h["skipped"], h["streak"]) == (2, 0, 0)
    step2.flat_p.copy_(step.flat_p)
    for s in (step, step2):
        _fake_grads(s, 4)
    opt.step()
    opt2.step()
    assert fake.bias_corrections[-1] == R.bias_corrections(0.9, 0.999, 3)
    assert torch.equal(step2.flat_p, step.flat_p) and torch.equal(step2.flat_m, step.flat_m) and torch.equal(step2.flat_v, step.flat_v)
    assert {float(st["step"]) for st in opt2.state_dict()["state"].values()} == {3.0}


def test_header_and_binding_declare_the_three_symbols():
    text = open(os.path.join(ROOT, "include", "gwdepth.h")).read()
    assert re.search(r"#define\s+GWD_VERSION\s+10\b", text)
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("gwd_segment_stats", "gwd_health_decide", "gwd_adamw_step_guarded"):
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert name in hip.ENTRY_POINTS
    assert re.search(r"#define\s+GWD_HEALTH_CHUNK\s+%d\b" % hip.HEALTH_CHUNK, text)
    assert re.search(r"GWD_WS_HEALTH\s*=\s*%d\b" % hip.WS_HEALTH, code)
