"""GPU: gwd_adamw_step_ema and gwd_ema_swap (csrc/ema.hip) through the hip.py wrappers, and TrainStep(ema_decay=...) in eager and graph
mode.

p, m, v and the bf16 shadow of the new entry point are compared BIT FOR BIT with gwd_adamw_step / gwd_adamw_step_guarded on copies of
the same inputs (tests/loss_ref.py's generators): the three kernels share one element function.  The average is checked element by
element against tests/ema_ref.py under its derived bound, charged against the p' the kernel returned.  PASS = hip.EMA_PASS is the
element count of one grid-stride pass: the sizes sit on either side of one pass and in the third, ragged one; the element offsets
0..3 from a 16-byte boundary exercise the scalar head and tail around the float4 body.

The end-to-end cases hold the whole flat buffer (66 M elements) against the same reference evaluated on the device in fp64; model
outputs are compared within the run-to-run spread of the bf16 forward (tests/test_infer_session.py's instrument), never across
separately run train steps."""
import numpy as np
import pytest
import torch

from gw_depth_amd import health as H
from gw_depth_amd import hip
from tests import ema_ref as E
from tests import loss_ref as R

pytestmark = pytest.mark.gpu
PASS = hip.EMA_PASS
GUARD = 64
SENTINEL = -777.25                                               # exact in fp32 and in bf16
SMALL = [1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 255, 256, 257, 1023, 1025]
LARGE = [PASS - 1, PASS, PASS + 1, 2 * PASS + 259]
SIZES = [(n, off) for n in SMALL for off in (0, 1, 2, 3)] + [(n, off) for n in LARGE for off in (0, 3)]
SIZE_IDS = ["n%d-off%d" % s for s in SIZES]
INF = float("inf")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    hip.set_library(None)
    torch.set_num_threads(16)
    yield hip.library()
    _INPUTS.clear()


# ------------------------------------------------------------------------------------------------------------- helpers
_INPUTS = {}


def case_inputs(n, clip):
    """loss_ref's adamw operands for (n, clip), made once and shared by the offsets and modes (read only)."""
    key = (n, clip)
    if key not in _INPUTS:
        c = R._case("adamw", "f32", n=n, off=0, ps="visible", clip=clip, var="", chained=0)
        inp = R.inputs(c)
        inp["ema"] = E.ema_values(n, n % 1000 + (7 if clip == "on" else 11))
        inp["sq"] = float((inp["g"].double() ** 2).sum())
        _INPUTS[key] = (c, inp)
    return _INPUTS[key]


def guarded(values, off, dtype=torch.float32):
    """-> (buffer, view): the values `off` elements past a 16-byte boundary (8-byte for bf16), GUARD sentinels on either side."""
    n = values.numel()
    buf = torch.full((GUARD + off + n + GUARD,), SENTINEL, dtype=dtype, device="cuda")
    view = buf[GUARD + off:GUARD + off + n]
    view.copy_(values.to(dtype))
    assert view.data_ptr() % (16 if dtype == torch.float32 else 8) == off * view.element_size()
    return buf, view


def sentinels_intact(buf, off, n, what):
    lo, hi = buf[:GUARD + off], buf[GUARD + off + n:]
    assert bool((lo == SENTINEL).all()) and bool((hi == SENTINEL).all()) and hi.numel() == GUARD, "%s: written outside [0, n)" % what


def bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def control_block(sq, bc1, bc2, applied, apply=1):
    c = np.zeros(1, dtype=H.CTL_DTYPE)
    c["sq"], c["bc1"], c["bc2"], c["applied"], c["apply"], c["clip_coef"] = sq, bc1, bc2, applied, apply, 1.0
    return torch.from_numpy(c.view(np.uint8).copy()).cuda()


def device_buffers(inp, off, with_p16, names=("p", "g", "m", "v", "ema")):
    bufs = {k: guarded(inp[k], off) for k in names}
    if with_p16:
        bufs["p16"] = guarded(torch.full((inp["p"].numel(),), 3.0), off, torch.bfloat16)      # stale values: every one is rewritten
    return bufs


HYPER = dict(decay_on=(0.9998, True, 5), decay_off=(0.9998, False, 3))       # clip on: the ramp's 6/15; clip off: omd = 2e-4


def run_pair(dev, n, off, clip, with_p16, mode):
    """The old entry point and gwd_adamw_step_ema on copies of one input -> (old outputs, new outputs, inputs, omd), on the host."""
    c, inp = case_inputs(n, clip)
    prm = R.adamw_params(c)
    decay, warmup, t = HYPER["decay_" + clip]
    old = device_buffers(inp, off, with_p16, ("p", "g", "m", "v"))
    new = device_buffers(inp, off, with_p16)
    v = lambda b, k: b[k][1] if k in b else None
    tail = (prm["max_norm"], prm["gs"])
    if mode == "guarded":
        ema_t = 40
        ctl = control_block(inp["sq"], np.float32(prm["bc1"]), np.float32(prm["bc2"]), ema_t + t)
        dev.adamw_step_guarded(v(old, "p"), v(old, "g"), v(old, "m"), v(old, "v"), v(old, "p16"), ctl, n, prm["lr"], prm["b1"], prm["b2"],
                               prm["eps"], prm["wd"], *tail)
        dev.adamw_step_ema(v(new, "p"), v(new, "g"), v(new, "m"), v(new, "v"), v(new, "p16"), v(new, "ema"), None, ctl, n, prm["lr"],
                           prm["b1"], prm["b2"], prm["eps"], prm["wd"], 0.5, 0.5, *tail, decay, warmup, ema_t)      # bc1, bc2: ignored
    else:
        sq = torch.tensor([inp["sq"]], dtype=torch.float64, device="cuda")
        dev.adamw_step(v(old, "p"), v(old, "g"), v(old, "m"), v(old, "v"), v(old, "p16"), sq, n, prm["lr"], prm["b1"], prm["b2"],
                       prm["eps"], prm["wd"], prm["bc1"], prm["bc2"], *tail)
        dev.adamw_step_ema(v(new, "p"), v(new, "g"), v(new, "m"), v(new, "v"), v(new, "p16"), v(new, "ema"), sq, None, n, prm["lr"],
                           prm["b1"], prm["b2"], prm["eps"], prm["wd"], prm["bc1"], prm["bc2"], *tail, decay, warmup, t)
    torch.cuda.synchronize()
    what = "n=%d off=%d clip=%s p16=%d %s" % (n, off, clip, with_p16, mode)
    for b in (old, new):
        for k, (buf, view) in b.items():
            sentinels_intact(buf, off, n, what + " " + k)
        assert torch.equal(bits(b["g"][1]).cpu(), bits(inp["g"])), what + ": g was written"
    return {k: x[1].cpu() for k, x in old.items()}, {k: x[1].cpu() for k, x in new.items()}, inp, E.omd_at(t, decay, warmup), what


# ------------------------------------------------------------------- 1 + 2: bit-identity with today's kernels, and the average
@pytest.mark.parametrize("mode", ["plain", "guarded"])
@pytest.mark.parametrize("n,off", SIZES, ids=SIZE_IDS)
def test_new_entry_point_equals_the_old_bit_for_bit_and_averages_within_the_bound(dev, n, off, mode):
    for clip in ("on", "off"):
        for with_p16 in (True, False):
            old, new, inp, omd, what = run_pair(dev, n, off, clip, with_p16, mode)
            for k in ("p", "m", "v") + (("p16",) if with_p16 else ()):
                same = bits(old[k]) == bits(new[k])
                assert bool(same.all()), "%s: %s differs from the old entry point in %d of %d elements, first at %d" % (
                    what, k, int((~same).sum()), n, int((~same).nonzero()[0]))
            assert not torch.equal(new["p"], inp["p"]) and not torch.equal(new["ema"], inp["ema"]), what + ": nothing was stored"
            if with_p16:
                assert torch.equal(bits(new["p16"]), bits(new["p"].to(torch.bfloat16))), what + ": p16 is not bf16(p')"
            worst = E.check(new["ema"], inp["ema"], new["p"], omd, what + " ema")
            print("%s: ema worst ratio %.3f of the bound, omd %.9g" % (what, worst, omd))


# ------------------------------------------------------------------------------------------- 3: the decay the device forms
T_VALUES = list(range(1, 65)) + [1000, 10 ** 6]


@pytest.mark.parametrize("mode", ["plain", "guarded"])
@pytest.mark.parametrize("warmup", [True, False], ids=["warmup", "flat"])
@pytest.mark.parametrize("decay", [0.5, 0.999, 0.9998])
def test_the_decay_the_device_forms(dev, decay, warmup, mode):
    """g = m = v = 0, weight_decay = 0, p = 1, ema = 0: p' = 1 and ema' = omd exactly."""
    n, k = 8, len(T_VALUES)
    p, ema = torch.ones(k, n, device="cuda"), torch.zeros(k, n, device="cuda")
    g, m, v = (torch.zeros(k, n, device="cuda") for _ in range(3))
    ema_t = 123
    for i, t in enumerate(T_VALUES):
        if mode == "guarded":
            ctl = control_block(0.0, 0.1, 0.001, ema_t + t)
            dev.adamw_step_ema(p[i], g[i], m[i], v[i], None, ema[i], None, ctl, n, 1e-4, 0.9, 0.999, 1e-8, 0.0, 1.0, 1.0, 0.1, 1.0, decay, warmup, ema_t)
        else:
            dev.adamw_step_ema(p[i], g[i], m[i], v[i], None, ema[i], None, None, n, 1e-4, 0.9, 0.999, 1e-8, 0.0, 0.1, 0.001, 0.1, 1.0, decay, warmup, t)
    torch.cuda.synchronize()
    assert bool((p == 1.0).all()) and bool((m == 0).all()) and bool((v == 0).all())
    got = ema.cpu().double()
    for i, t in enumerate(T_VALUES):
        want = E.omd_at(t, decay, warmup)
        assert got[i].tolist() == [want] * n, (t, decay, warmup, mode, got[i].tolist(), want)


# --------------------------------------------------------------------------------- 4: a still parameter keeps its average
@pytest.mark.parametrize("mode", ["plain", "guarded"])
def test_a_still_parameter_keeps_its_average(dev, mode):
    n, off = 1025, 1
    vals = E.ema_values(n, 21)
    z = torch.zeros(n)
    (pb, p), (eb, ema), (_, g), (_, m), (_, v) = (guarded(x, off) for x in (vals, vals, z, z, z))
    ctl = control_block(0.0, 0.1, 0.001, 9) if mode == "guarded" else None
    dev.adamw_step_ema(p, g, m, v, None, ema, None, ctl, n, 1e-4, 0.9, 0.999, 1e-8, 0.0, 0.1, 0.001, 0.1, 1.0, 0.9998, True, 4)
    torch.cuda.synchronize()
    assert torch.equal(bits(p).cpu(), bits(vals)) and torch.equal(bits(ema).cpu(), bits(vals))
    sentinels_intact(pb, off, n, "p")
    sentinels_intact(eb, off, n, "ema")


# ---------------------------------------------------------------------------------------- 5: the skip path stores nothing
@pytest.mark.parametrize("n", [257, 2 * PASS + 259])
def test_the_skip_path_stores_nothing(dev, n):
    c, inp = case_inputs(n, "on")
    prm = R.adamw_params(c)
    g = inp["g"].clone()
    g[n // 2] = INF
    bufs = device_buffers(dict(inp, g=g), 3, True)
    bufs["p16"][1].copy_(inp["p"])
    before = {k: b[0].clone() for k, b in bufs.items()}
    ctl = control_block(inp["sq"], np.float32(prm["bc1"]), np.float32(prm["bc2"]), 2, apply=0)
    x = lambda k: bufs[k][1]
    dev.adamw_step_ema(x("p"), x("g"), x("m"), x("v"), x("p16"), x("ema"), None, ctl, n, prm["lr"], prm["b1"], prm["b2"], prm["eps"], prm["wd"],
                       0.5, 0.5, prm["max_norm"], prm["gs"], 0.5, False, 0)
    torch.cuda.synchronize()
    for k in ("p", "g", "m", "v", "ema", "p16"):
        assert torch.equal(bits(bufs[k][0]), bits(before[k])), k


# ------------------------------------------------------------------------------------------------------- 6: gwd_ema_swap
@pytest.mark.parametrize("n,off", SIZES, ids=SIZE_IDS)
def test_swap_exchanges_and_a_second_call_restores(dev, n, off):
    g = torch.Generator().manual_seed(n + off)
    p0, e0 = torch.randn(n, generator=g), E.ema_values(n, n + 5)
    for with_p16 in (True, False):
        (pb, p), (eb, ema) = guarded(p0, off), guarded(e0, off)
        sb, p16 = guarded(p0, off, torch.bfloat16) if with_p16 else (None, None)
        dev.ema_swap(p, ema, p16, n)
        torch.cuda.synchronize()
        assert torch.equal(bits(p).cpu(), bits(e0)) and torch.equal(bits(ema).cpu(), bits(p0))
        if with_p16:
            assert torch.equal(bits(p16).cpu(), bits(e0.to(torch.bfloat16)))
        dev.ema_swap(p, ema, p16, n)
        torch.cuda.synchronize()
        assert torch.equal(bits(p).cpu(), bits(p0)) and torch.equal(bits(ema).cpu(), bits(e0))
        sentinels_intact(pb, off, n, "p")
        sentinels_intact(eb, off, n, "ema")
        if with_p16:
            assert torch.equal(bits(p16).cpu(), bits(p0.to(torch.bfloat16)))
            sentinels_intact(sb, off, n, "p16")


def test_misaligned_ranges_are_refused_through_the_binding(dev):
    x = [torch.zeros(64, device="cuda") for _ in range(5)]
    with pytest.raises(RuntimeError, match="-3"):
        dev.adamw_step_ema(x[0][1:9], x[1][:8], x[2][1:9], x[3][1:9], None, x[4][1:9], None, None, 8, 1e-4, 0.9, 0.999, 1e-8, 0.0, 0.1, 0.001,
                           0.1, 1.0, 0.5, True, 1)
    with pytest.raises(RuntimeError, match="-3"):
        dev.ema_swap(x[0][:8], x[1][2:10], None, 8)
    torch.cuda.synchronize()
    assert all(bool((t == 0).all()) for t in x)


# --------------------------------------------------------------------------------------------------- 7: TrainStep, end to end
def _batch():
    from gw_depth_amd.synth import synth_batch
    from tests.golden_check import to_device
    return to_device(synth_batch(2, 96, 128, seed=45, n_lines=[3, 4]), "cuda")


def _step(graph, **kw):
    from gw_depth_amd.engine import TrainStep
    from tests.golden_check import build
    cfg, model, crits = build(device="cuda")
    return model, TrainStep(model, crits, cfg, compute_dtype=torch.bfloat16, graph=graph, ema_decay=0.5, ema_warmup=False, **kw)


def _eval_depth(model, b):
    from gw_depth_amd.model import NestedTensor
    model.compute_dtype = torch.bfloat16
    model.eval()
    with torch.no_grad():
        out = model(NestedTensor(b["images"], b["pad_mask"]))["pred_depth"][-1].float().clone()
    torch.cuda.synchronize()
    return out


def _rel(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-12))


def _check_flat(step, before, t, what):
    """flat_e against the recurrence from `before` and the flat_p read back after the step: the reference of ema_ref.py, on the device."""
    worst = E.check(step.flat_e, before, step.flat_p, E.omd_at(t, 0.5, False), what)
    print("%s: flat_e worst ratio %.3f of the bound over %d elements" % (what, worst, step.total))


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_train_step_averages_and_use_ema_serves_the_average(dev, graph):
    from gw_depth_amd.engine import TrainStep
    from gw_depth_amd.infer import InferenceSession
    from gw_depth_amd.model import NestedTensor
    from tests.golden_check import build
    b = _batch()
    model, step = _step(graph)
    assert step.flat_p16 is not None and torch.equal(step.flat_e, step.flat_p)
    for t in (1, 2, 3):
        before = step.flat_e.clone()
        step(b)
        step.flush()
        torch.cuda.synchronize()
        _check_flat(step, before, t, "%s step %d" % ("graph" if graph else "eager", t))
    assert step.ema_updates() == 3 and not torch.equal(step.flat_e, step.flat_p)
    if graph:
        assert step.graph_stats()["replays"] >= 1, step.graph_stats()

    outside = _eval_depth(model, b)
    spread = _rel(_eval_depth(model, b), outside)
    bar = max(4 * spread, 2e-5)                                  # the run-to-run spread of the bf16 forward decides what "equal" means
    p_bits, s_bits, e_bits = bits(step.flat_p).clone(), bits(step.flat_p16).clone(), bits(step.flat_e).clone()
    nt = NestedTensor(b["images"], b["pad_mask"])
    with step.use_ema():
        assert torch.equal(bits(step.flat_p), e_bits) and torch.equal(bits(step.flat_p16), bits(step.flat_p.to(torch.bfloat16)))
        inside = _eval_depth(model, b)
        sess = InferenceSession(model, compute_dtype=torch.bfloat16, graph=graph)
        sess_inside = sess(nt)["pred_depth"][-1].float().clone()
        with pytest.raises(RuntimeError, match="use_ema"):
            step(b)
    torch.cuda.synchronize()
    assert torch.equal(bits(step.flat_p), p_bits) and torch.equal(bits(step.flat_p16), s_bits) and torch.equal(bits(step.flat_e), e_bits)
    moved = _rel(inside, outside)
    print("eval forward inside use_ema() against outside: %.3e (run-to-run spread %.3e, bar %.3e)" % (moved, spread, bar))
    assert moved > bar, "the averaged weights gave the outside result"
    assert _rel(sess_inside, inside) <= bar

    sess_after = sess(nt)["pred_depth"][-1].float().clone()      # the block has ended: the session still serves the average
    torch.cuda.synchronize()
    d_after = _rel(sess_after, sess_inside)
    print("session built inside the block, called after it: %.3e from its inside result" % d_after)
    assert d_after <= bar and _rel(sess_after, outside) > bar
    assert _rel(_eval_depth(model, b), outside) <= bar           # and the model itself is back on its weights

    sd = step.ema_state_dict()
    cfg2, model2, crits2 = build(device="cuda")
    step2 = TrainStep(model2, crits2, cfg2, compute_dtype=torch.bfloat16, graph=graph)      # the same mode: flat buffers and a bf16 shadow
    model2.load_state_dict(sd)
    step2.flat_p16.copy_(step2.flat_p)
    assert torch.equal(bits(step2.flat_p), e_bits)               # the state dict carries the average bit for bit, layouts included
    second = _eval_depth(model2, b)
    d_second = _rel(second, inside)
    print("a second model that loaded ema_state_dict(): %.3e from the inside result" % d_second)
    assert d_second <= bar


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_guarded_train_step_keeps_the_average_across_a_skipped_step(dev, graph):
    b = _batch()
    model, step = _step(graph, guard="skip")
    before = step.flat_e.clone()
    step(b)
    step.flush()
    torch.cuda.synchronize()
    _check_flat(step, before, 1, "guarded step 1")
    assert step.ema_updates() == 1

    saved = [bits(t).clone() for t in (step.flat_p, step.flat_e, step.flat_m, step.flat_v, step.flat_p16)]
    if graph:
        step._on_graph_stream(b, None)                   # the eager forward/backward of a graph-mode step
    else:
        step.forward_backward(b)
    victim = step.names[len(step.names) // 2]
    step.flat_g[step.offsets[victim] + step.params[victim].numel() - 1] = INF
    step.optimizer_step()
    torch.cuda.synchronize()
    now = [bits(t) for t in (step.flat_p, step.flat_e, step.flat_m, step.flat_v, step.flat_p16)]
    assert all(torch.equal(a, s) for a, s in zip(now, saved))    # the average too, bit for bit
    h = step.health()
    assert (h["applied"], h["skipped"]) == (1, 1) and step.ema_updates() == 1

    before = step.flat_e.clone()
    step(b)
    step.flush()
    torch.cuda.synchronize()
    _check_flat(step, before, 2, "guarded step 3 (update 2)")
    assert step.ema_updates() == 2 and step.step_count == 3 and bool(torch.isfinite(step.flat_e).all())
