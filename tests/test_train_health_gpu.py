"""GPU: the three entry points of csrc/health.hip through the hip.py wrappers against tests/health_ref.py and tests/loss_ref.py, and
TrainStep(guard="skip") in eager and graph mode.  Non-finite values enter only through flat_g after backward.

Bounds.  nonfinite and absmax are exact.  sumsq: the squares are exact in fp64, so a sum of the n_s terms of a segment is within
n_s 2^-53 sumsq of the exact sum (math.fsum), whatever the order.  The fold of gwd_health_decide is compared with the same
sequential fp64 sum of the same records: equal.  bc1 / bc2: 1 fp32 ulp of float32(1 - beta**t) (the device's pow).  clip_coef: four
fp32 roundings (the conversion of sqrt(sq), the product, the sum, the division): 4 * 2^-24 relative.  The guarded AdamW is checked
by tests/loss_ref.py's adamw reference and constants, fed the bc1, bc2 and sq of the control block."""
import math

import numpy as np
import pytest
import torch

from gw_depth_amd import health as H
from gw_depth_amd import hip
from tests import health_ref as HR
from tests import loss_ref as R

pytestmark = pytest.mark.gpu
CH = hip.HEALTH_CHUNK
ALIGN = 8
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    hip.set_library(None)
    torch.set_num_threads(16)
    return hip.library()


# ------------------------------------------------------------------------------------------------------------- helpers
def layout(lengths):
    """Ragged table: segment s starts on a multiple of 8, with 0, 8 or 16 elements of padding and the alignment slack behind it."""
    begin, off = [], 0
    for n in lengths:
        begin.append(off)
        off += (n + ALIGN - 1) // ALIGN * ALIGN + ALIGN * (len(begin) % 3)
    return begin, [b + n for b, n in zip(begin, lengths)], off + ALIGN


def tables(begin, end, total):
    chunks = H.chunk_table(begin, end)
    H.check_tables(begin, end, chunks, total)
    return (torch.tensor(begin, dtype=torch.int64, device="cuda"), torch.tensor(end, dtype=torch.int64, device="cuda"),
            torch.from_numpy(chunks.view("<i8").reshape(-1, 2).copy()).cuda(), len(chunks))


def run_stats(dev, x, begin, end):
    """-> STAT_DTYPE records of one gwd_segment_stats; partial and out start as 0xFF bytes (NaN / -1: nothing may survive)."""
    sb, se, ch, n_chunks = tables(begin, end, x.numel())
    nbytes = dev.workspace_bytes(hip.WS_HEALTH, n_chunks)
    assert nbytes == max(n_chunks, 1) * 16
    partial = torch.full((nbytes,), 255, dtype=torch.uint8, device="cuda")
    out = torch.full((len(begin) * 16,), 255, dtype=torch.uint8, device="cuda")
    dev.segment_stats(x, sb, se, ch, partial, out)
    torch.cuda.synchronize()
    return H.decode(out.cpu(), H.STAT_DTYPE), out


def fill(lengths, seed, poison=()):
    """Values with a wide dynamic range in the segments, NaN in EVERY padding element; poison: (segment, index, value)."""
    begin, end, total = layout(lengths)
    g = torch.Generator().manual_seed(seed)
    x = torch.full((total,), NAN)
    for b, e in zip(begin, end):
        v = torch.randn(e - b, generator=g) * torch.exp(3.0 * torch.randn(e - b, generator=g))
        x[b:e] = v
    for s, i, val in poison:
        x[begin[s] + (i if i >= 0 else lengths[s] + i)] = val
    return x, begin, end


def check_stats(rec, x, begin, end):
    ref = HR.segment_stats(x, begin, end)
    for s, (sumsq, absmax, nonfinite) in enumerate(ref):
        n = end[s] - begin[s]
        got = rec[s]
        err, bound = abs(float(got["sumsq"]) - sumsq), HR.sumsq_bound(n, sumsq)
        print("segment %d n=%d: sumsq %.17g ref %.17g err %.3g bound %.3g absmax %r nonfinite %d" %
              (s, n, float(got["sumsq"]), sumsq, err, bound, float(got["absmax"]), int(got["nonfinite"])))
        assert int(got["nonfinite"]) == nonfinite, (s, int(got["nonfinite"]), nonfinite)
        assert float(got["absmax"]) == absmax, (s, float(got["absmax"]), absmax)
        assert math.isfinite(float(got["sumsq"])) and err <= bound, (s, float(got["sumsq"]), sumsq, err, bound)


LENGTHS = [0, 1, 3, 4, 5, 8, CH - 1, CH, CH + 1, 2 * CH + 5]
# first and last element of a segment; either side of both chunk boundaries of the 2 CH + 5 segment; the ragged tail; a short segment
POISON = [(9, 0, NAN), (9, -1, INF), (9, CH - 1, -INF), (9, CH, NAN), (9, 2 * CH - 1, INF), (9, 2 * CH, -INF), (9, 2 * CH + 3, NAN),
          (8, 0, INF), (8, -1, NAN), (7, CH - 1, NAN), (6, 0, -INF), (6, -1, INF), (4, 0, NAN), (4, 4, INF), (2, 1, NAN), (1, 0, INF)]


# ----------------------------------------------------------------------------------------------------- gwd_segment_stats
@pytest.mark.parametrize("poisoned", [0, 1], ids=["finite", "poisoned"])
def test_segment_stats_against_the_fp64_reference(dev, poisoned):
    x, begin, end = fill(LENGTHS, 11 + poisoned, POISON if poisoned else ())
    xd = x.cuda()
    rec, out1 = run_stats(dev, xd, begin, end)
    check_stats(rec, x, begin, end)
    assert (rec["nonfinite"].sum() == len(POISON)) if poisoned else (rec["nonfinite"].sum() == 0)     # no record saw the NaN padding
    _, out2 = run_stats(dev, xd, begin, end)
    assert torch.equal(out1, out2)                               # bit-equal from run to run
    assert torch.equal(xd.cpu().view(torch.int32), x.view(torch.int32))                                # x is read only


@pytest.mark.parametrize("n", [1, CH + 3])
def test_segment_stats_of_a_single_segment(dev, n):
    x, begin, end = fill([n], 5)
    rec, _ = run_stats(dev, x.cuda(), begin, end)
    check_stats(rec, x, begin, end)


def test_segment_stats_squares_in_fp64(dev):
    """1e30^2 overflows fp32: a finite gradient never gives an infinite norm."""
    x = torch.tensor([1e30, -2e30, 3e-30, 0.0, 0.0, 0.0, 0.0, 0.0])
    rec, _ = run_stats(dev, x.cuda(), [0], [3])
    check_stats(rec, x, [0], [3])
    assert float(rec[0]["sumsq"]) > 1e60


def test_segment_stats_return_codes(dev):
    x = torch.ones(64, device="cuda")
    sb, se, ch, n_chunks = tables([0], [40], 64)
    partial = torch.zeros(16, dtype=torch.uint8, device="cuda")
    out = torch.full((16,), 255, dtype=torch.uint8, device="cuda")
    p, stream = hip._ptr, dev._stream(x)
    assert dev.lib.gwd_segment_stats(p(x[1:]), p(sb), p(se), 1, p(ch), n_chunks, p(partial), p(out), stream) == -3
    assert dev.lib.gwd_segment_stats(None, p(sb), p(se), 1, p(ch), n_chunks, p(partial), p(out), stream) == -1
    assert dev.lib.gwd_segment_stats(p(x), p(sb), p(se), 0, p(ch), n_chunks, p(partial), p(out), stream) == -1
    torch.cuda.synchronize()
    assert bool((out == 255).all())
    assert dev.workspace_bytes(hip.WS_HEALTH, 0) == 16 and dev.workspace_bytes(hip.WS_HEALTH, 5000) == 80000


# ----------------------------------------------------------------------------------------------------- gwd_health_decide
class Decider:
    """A control block, ring and bad table on the device, with the reference's state next to them."""

    def __init__(self, dev, S, ring_len, applied=0):
        self.dev, self.S, self.ring_len = dev, S, ring_len
        c = np.zeros(1, dtype=H.CTL_DTYPE)
        c["applied"] = applied
        self.ctl = torch.from_numpy(c.view(np.uint8).copy()).cuda()
        self.ring = torch.zeros(ring_len * 32, dtype=torch.uint8, device="cuda")
        self.bad = torch.full((S,), -7, dtype=torch.int32, device="cuda")
        self.ref = HR.new_ctl()
        self.ref["applied"] = applied
        self.ref_bad = None

    def step(self, stats, loss, max_norm, gs, beta1=0.9, beta2=0.999):
        rec = np.array(stats, dtype=H.STAT_DTYPE)
        sd = torch.from_numpy(rec.view(np.uint8).copy()).cuda()
        ld = None if loss is None else torch.tensor([loss], dtype=torch.float32, device="cuda")
        self.dev.health_decide(sd, self.S, ld, self.ctl, self.ring, self.ring_len, self.bad, beta1, beta2, max_norm, gs)
        torch.cuda.synchronize()
        self.ref, ref_rec, self.ref_bad = HR.decide(stats, self.ref, loss, beta1, beta2, max_norm, gs, self.ref_bad)
        return H.decode(self.ctl.cpu(), H.CTL_DTYPE)[0], ref_rec


def _same_float(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


def _ulp32(x):
    return float(np.spacing(np.float32(x)))


def test_health_decide_over_apply_skip_skip_apply(dev):
    S, ring_len = 70, 3                                  # more than one round of 64 records; the ring wraps at the fourth step
    g = torch.Generator().manual_seed(3)

    def stats(bad):
        sumsq = (torch.rand(S, generator=g, dtype=torch.float64) * torch.exp(4 * torch.randn(S, generator=g, dtype=torch.float64))).tolist()
        return [(sumsq[s], 1.0 + s, bad.get(s, 0)) for s in range(S)]

    d = Decider(dev, S, ring_len)
    plan = [({}, 1.25, 0.1, 1.0), ({0: 2, 69: 1}, INF, 0.1, 0.5), ({33: 4}, NAN, 0.0, 0.5), ({}, None, 0.1, 0.125)]
    for k, (bad, loss, max_norm, gs) in enumerate(plan):
        got, ref_rec = d.step(stats(bad), loss, max_norm, gs)
        ref = d.ref
        print("step %d: ctl %r" % (k + 1, got))
        for key in ("applied", "skipped", "streak", "nonfinite_total", "apply", "loss_finite"):
            assert int(got[key]) == ref[key], (k, key, int(got[key]), ref[key])
        assert float(got["sq"]) == ref["sq"], (k, float(got["sq"]), ref["sq"])           # the same sequential fp64 sum: equal
        assert _same_float(float(got["loss"]), ref["loss"])
        for key in ("bc1", "bc2"):
            assert abs(float(got[key]) - ref[key]) <= _ulp32(ref[key]), (k, key, float(got[key]), ref[key])
        assert abs(float(got["clip_coef"]) - ref["clip_coef"]) <= 4 * 2.0 ** -24 * ref["clip_coef"], (k, float(got["clip_coef"]), ref["clip_coef"])
        ring = H.decode(d.ring.cpu(), H.RING_DTYPE)
        slot = ring[k % ring_len]
        assert int(slot["step"]) == ref_rec["step"] == k + 1 and bool(slot["apply"]) == ref_rec["apply"]
        assert int(slot["nonfinite_total"]) == ref_rec["nonfinite_total"] and _same_float(float(slot["loss"]), ref_rec["loss"])
        assert float(slot["clip_coef"]) == float(got["clip_coef"])
        assert abs(float(slot["grad_norm"]) - ref_rec["grad_norm"]) <= 2.0 ** -51 * ref_rec["grad_norm"]
        want_bad = [-7] * S if d.ref_bad is None else d.ref_bad
        assert d.bad.cpu().tolist() == want_bad, k
    assert (d.ref["applied"], d.ref["skipped"], d.ref["streak"]) == (2, 2, 0)
    assert d.ref_bad[33] == 4 and sum(d.ref_bad) == 4                                   # the culprits of the LAST skipped step
    ring = H.decode(d.ring.cpu(), H.RING_DTYPE)
    assert sorted(int(r["step"]) for r in ring) == [2, 3, 4]


@pytest.mark.parametrize("beta1,beta2", [(0.9, 0.999)])
def test_bias_corrections_of_the_device(dev, beta1, beta2):
    worst = 0.0
    for t in list(range(1, 65)) + [1000]:
        d = Decider(dev, 1, 1, applied=t - 1)
        got, _ = d.step([(1.0, 1.0, 0)], None, 0.1, 1.0, beta1, beta2)
        assert int(got["applied"]) == t
        for key, want in zip(("bc1", "bc2"), HR.bias_corrections(beta1, beta2, t)):
            err = abs(float(got[key]) - want) / _ulp32(want)
            worst = max(worst, err)
            assert err <= 1.0, (t, key, float(got[key]), want)
    print("bias corrections: worst error %.1f ulp" % worst)


# ------------------------------------------------------------------------------------------------ gwd_adamw_step_guarded
def _adamw_case(n, var, ps="visible", clip="on"):
    return R._case("adamw", "f32", n=n, off=0, ps=ps, clip=clip, var=var, chained=0)


def _control_block(dev, g, prm, t):
    """segment_stats + health_decide over g as ONE segment, with applied = t - 1 before -> (ctl device tensor, its record)."""
    n = g.numel()
    sb, se, ch, n_chunks = tables([0], [n], n)
    partial = torch.empty(dev.workspace_bytes(hip.WS_HEALTH, n_chunks), dtype=torch.uint8, device="cuda")
    stats = torch.empty(16, dtype=torch.uint8, device="cuda")
    dev.segment_stats(g, sb, se, ch, partial, stats)
    d = Decider(dev, 1, 2, applied=t - 1)
    dev.health_decide(stats, 1, None, d.ctl, d.ring, 2, d.bad, R.BETA1, R.BETA2, prm["max_norm"], prm["gs"])
    torch.cuda.synchronize()
    return d.ctl, H.decode(d.ctl.cpu(), H.CTL_DTYPE)[0]


def _run_guarded(dev, c, inp, ctl, prm):
    bufs = {k: inp[k].clone().cuda() for k in ("p", "g", "m", "v")}
    p16 = None if c.var == "nop16" else torch.full((c.n,), NAN, dtype=torch.bfloat16, device="cuda")
    dev.adamw_step_guarded(bufs["p"], bufs["g"], bufs["m"], bufs["v"], p16, ctl, c.n, prm["lr"], prm["b1"], prm["b2"], prm["eps"], prm["wd"],
                           prm["max_norm"], prm["gs"])
    torch.cuda.synchronize()
    assert torch.equal(bufs["g"].cpu(), inp["g"]), "g was written"
    out = {k: bufs[k].cpu() for k in ("p", "m", "v")}
    if p16 is not None:
        out["p16"] = p16.cpu()
    return out


ADAMW_CASES = [(n, var, "visible", "on") for n in (1, 255, 257, 2 * R.ADAMW_PASS + 259) for var in ("nop16", "")] + \
              [(257, "", "ship_c", "off"), (257, "", "ship_b", "on")]


@pytest.mark.parametrize("n,var,ps,clip", ADAMW_CASES, ids=["n%d-%s-%s-clip_%s" % (n, var or "p16", ps, clip) for n, var, ps, clip in ADAMW_CASES])
def test_guarded_adamw_apply_path(dev, monkeypatch, n, var, ps, clip):
    c = _adamw_case(n, var, ps, clip)
    inp = R.inputs(c)
    prm = R.adamw_params(c)
    t = R.PSETS[ps][3]
    ctl, rec = _control_block(dev, inp["g"].cuda(), prm, t)
    assert int(rec["apply"]) == 1 and int(rec["applied"]) == t
    exact = math.fsum((inp["g"].double() ** 2).tolist())
    assert abs(float(rec["sq"]) - exact) <= HR.sumsq_bound(n, exact)
    for key in ("bc1", "bc2"):
        assert abs(float(rec[key]) - float(np.float32(prm[key]))) <= _ulp32(prm[key]), (key, float(rec[key]), prm[key])
    got = _run_guarded(dev, c, inp, ctl, prm)
    # float operands are operands: the reference is fed the bias corrections and the sq the kernel read
    fed = dict(prm, bc1=float(rec["bc1"]), bc2=float(rec["bc2"]))
    coef = R._adamw_coef
    monkeypatch.setattr(R, "adamw_params", lambda case: dict(fed))
    monkeypatch.setattr(R, "_adamw_coef", lambda case, p, sq: coef(case, p, None if sq is None else float(rec["sq"])))
    for name, worst in R.check(c, got, inp).items():
        print("%s %s: worst ratio %.3f of C = %.1f" % (c.text, name, worst, R.C[R.key_of(c, name)]))


@pytest.mark.parametrize("n", [257, 2 * R.ADAMW_PASS + 259])
def test_guarded_adamw_skip_path_stores_nothing(dev, n):
    c = _adamw_case(n, "")
    inp = R.inputs(c)
    prm = R.adamw_params(c)
    g = inp["g"].clone()
    g[n // 2] = INF
    ctl, rec = _control_block(dev, g.cuda(), prm, 3)
    assert int(rec["apply"]) == 0 and int(rec["applied"]) == 2 and int(rec["skipped"]) == 1
    bufs = {k: inp[k].clone().cuda() for k in ("p", "m", "v")}
    p16 = inp["p"].to(torch.bfloat16).cuda()
    before = {k: v.clone() for k, v in bufs.items()}
    before16 = p16.clone()
    dev.adamw_step_guarded(bufs["p"], g.cuda(), bufs["m"], bufs["v"], p16, ctl, n, prm["lr"], prm["b1"], prm["b2"], prm["eps"], prm["wd"],
                           prm["max_norm"], prm["gs"])
    torch.cuda.synchronize()
    for k in bufs:
        assert torch.equal(bufs[k].view(torch.int32), before[k].view(torch.int32)), k
    assert torch.equal(p16.view(torch.int16), before16.view(torch.int16))


# ------------------------------------------------------------------------------------------------------------- TrainStep
def _bits(step):
    return [t.clone() for t in (step.flat_p, step.flat_m, step.flat_v)] + ([] if step.flat_p16 is None else [step.flat_p16.clone()])


def _unchanged(step, saved):
    now = [step.flat_p, step.flat_m, step.flat_v] + ([] if step.flat_p16 is None else [step.flat_p16])
    return all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(now, saved))


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_train_step_skips_a_poisoned_gradient(dev, graph):
    """Fails without the guard: the poisoned step turns every parameter into NaN."""
    from gw_depth_amd.engine import TrainStep
    from gw_depth_amd.synth import synth_batch
    from tests.golden_check import build, to_device
    b = to_device(synth_batch(2, 96, 128, seed=45, n_lines=[3, 4]), "cuda")
    cfg, model, crits = build(device="cuda")
    step = TrainStep(model, crits, cfg, compute_dtype=torch.bfloat16, graph=graph, guard="skip")
    assert step.flat_p16 is not None
    step(b)
    step(b)
    step.flush()
    h = step.health()
    assert (h["applied"], h["skipped"], h["streak"]) == (2, 0, 0) and h["last"]["apply"] and h["loss_finite"]
    assert step.health(wait=False)["applied"] == 2

    saved = _bits(step)
    if graph:
        step._on_graph_stream(b, None)                   # the eager forward/backward of a graph-mode step
    else:
        step.forward_backward(b)
    victim = step.names[len(step.names) // 2]
    step.flat_g[step.offsets[victim] + step.params[victim].numel() - 1] = INF
    step.optimizer_step()
    torch.cuda.synchronize()
    assert _unchanged(step, saved)                       # parameters, both moments and the bf16 shadow, bit for bit
    h = step.health()
    assert (h["applied"], h["skipped"], h["streak"]) == (2, 1, 1) and not h["last"]["apply"] and h["last"]["nonfinite_total"] == 1
    assert step.first_nonfinite() == [victim]
    step.flush()                                         # one skipped step is no reason to stop

    step(b)
    step.flush()
    torch.cuda.synchronize()
    h = step.health()
    assert (h["applied"], h["skipped"], h["streak"]) == (3, 1, 0) and step.step_count == 4
    assert not _unchanged(step, saved) and bool(torch.isfinite(step.flat_p).all())
    assert [r["apply"] for r in step.history()] == [True, True, False, True]

    # per-tensor statistics of the last step's gradient against fp64 sums of the same buffer
    stats = step.tensor_stats()
    grec, _ = step._health.read_stats()
    flat = step.flat_g.cpu()
    for i, n in enumerate(step.names):
        o, k = step.offsets[n], step.params[n].numel()
        v = flat[o:o + k].double()
        ref = math.fsum((v * v).tolist()) if k <= 4096 else float((v * v).sum())
        assert abs(float(grec[i]["sumsq"]) - ref) <= HR.sumsq_bound(k, ref), (n, float(grec[i]["sumsq"]), ref)
        assert stats[n][0] == math.sqrt(float(grec[i]["sumsq"])) and stats[n][1] == float(v.abs().max()) and stats[n][2] == 0
        assert abs(stats[n][0] - float(v.norm())) <= (k * 2.0 ** -54 + 2.0 ** -51) * float(v.norm()), n
    total = float(flat.double().norm())                  # the padding of flat_g is zero; the bound above over all elements
    assert abs(step.grad_norm() - total) <= (step.total * 2.0 ** -54 + 2.0 ** -51) * total
