"""GPU: gwd_set_losses_forward / _backward and the _focal_ pair, gwd_lsap and gwd_pos_sine, run through hip.library() at every case of
tests/setloss_ref.py, tests/lsap_ref.py and tests/posenc_ref.py.  The losses, their gradients and the embedding are compared ELEMENT
by element, every element of every output, with the fp64 references there: bound C u (|ref| + cond) with C from the CPU rounding
models (never from a kernel's output); target classes, weight sums, level masks, counts and the LSAP's assignment - ties included -
for equality.  Every output is prefilled (floats with NaN, integers and bytes with a value no result can equal, dlines with its
entry value), every operand and output has guard elements on both sides, every operand is bit-identical after the call, and every
call is made twice from fresh buffers and must return identical bits: all three families have a fixed summation order (the atomics
of dlines hit distinct addresses).

tests/test_criterion_witnesses.py proves on the CPU that the cases reach the launch edges they claim.  Run the file with -x: a fault
is a finding."""
import collections

import numpy as np
import pytest
import torch

from gw_depth_amd import hip
from tests import lsap_ref as LR
from tests import posenc_ref as PR
from tests import setloss_ref as SR

pytestmark = pytest.mark.gpu
WORST = collections.defaultdict(float)            # (operation, output, type) -> worst ratio over the file
GUARD = 8                                         # elements on either side
GUARD_INT = {torch.int16: -31073, torch.int32: -31073, torch.int64: -31073, torch.uint8: 0xA5}
LOSS, LSAP, POS = SR.cases(), LR.cases(), PR.cases()


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    hip.set_library(None)
    torch.set_num_threads(16)
    return hip.library()


def _guard_value(dtype):
    return float("nan") if dtype.is_floating_point else GUARD_INT[dtype]


def _guarded(shape, dtype=torch.float32, values=None, fill=None):
    """-> (buffer, view): a tensor of `shape` with GUARD guard elements in front of it and behind it; `values` or `fill` inside
    (neither: the guard value - NaN for floats)."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), _guard_value(dtype), dtype=dtype, device="cuda")
    view = buf[GUARD:GUARD + n].view(tuple(shape))
    if values is not None:
        view.copy_(torch.as_tensor(values).reshape(tuple(shape)))
    elif fill is not None:
        view.fill_(fill)
    return buf, view


def _guards_intact(buf, what):
    g = torch.cat([buf[:GUARD], buf[-GUARD:]])
    ok = torch.isnan(g) if buf.dtype.is_floating_point else g == GUARD_INT[buf.dtype]
    assert bool(ok.all()), "%s: written outside its range" % what


def _bits(t):
    return t.contiguous().view({torch.float32: torch.int32, torch.float64: torch.int64}.get(t.dtype, t.dtype))


def _operands_intact(ops, inp, what):
    for k, (buf, view) in ops.items():
        _guards_intact(buf, "%s %s" % (what, k))
        assert torch.equal(_bits(view.cpu()), _bits(inp[k].to(view.dtype))), "%s: %s was written" % (what, k)


def _twice(what, call):
    """call() -> {name: CPU tensor}; made twice from fresh buffers: the same bits."""
    first, second = call(), call()
    for name in first:
        assert torch.equal(_bits(first[name]), _bits(second[name])), "%s %s: two calls, different bits" % (what, name)
    return first


def _note(key, worst, what):
    WORST[key] = max(WORST[key], worst)
    print("%s: worst ratio %.3f" % (what, worst))


# ============================================================================================================ set losses
def run_losses(dev, c, inp):
    names = ["logits", "lines", "tgt", "labels", "bidx", "valid", "qot", "cls_w", "num_items"] + [g for g in ("g_ce", "g_l1") if inp[g] is not None]
    ops = {k: _guarded(inp[k].shape, inp[k].dtype, values=inp[k]) for k in names}
    o = {k: v[1] for k, v in ops.items()}
    outs = {"target_class": _guarded((c.L, c.B, c.Q), torch.int32, fill=SR.TC_SENTINEL), "ce": _guarded((c.L,)), "l1": _guarded((c.L,)),
            "wsum": _guarded((c.L,)), "dlogits": _guarded((c.L, c.B, c.Q, c.K)), "dlines": _guarded((c.L, c.B, c.Q, c.D), values=inp["c0"])}
    r = {k: v[1] for k, v in outs.items()}
    dev.set_losses_forward(o["logits"], o["lines"], o["tgt"], o["labels"], o["bidx"], o["valid"], o["qot"], o["cls_w"], o["num_items"], c.world,
                           r["target_class"], r["ce"], r["l1"], r["wsum"], gamma=c.gamma)
    dev.set_losses_backward(o["logits"], o["lines"], o["tgt"], o["bidx"], o["valid"], o["qot"], o["cls_w"], o["num_items"], c.world,
                            r["target_class"], r["wsum"], o.get("g_ce"), o.get("g_l1"), r["dlogits"], r["dlines"], gamma=c.gamma)
    torch.cuda.synchronize()
    for k, (buf, view) in outs.items():
        _guards_intact(buf, "%s %s" % (c.text, k))
    _operands_intact(ops, inp, c.text)
    return {k: v.cpu() for k, v in r.items()}


@pytest.mark.parametrize("c", LOSS, ids=[c.id for c in LOSS])
def test_set_losses(dev, c):
    inp = SR.inputs(c)
    got = _twice(c.text, lambda: run_losses(dev, c, inp))
    assert SR.TC_SENTINEL not in got["target_class"], c.text + ": a target class was not written"
    for name in ("ce", "l1", "wsum", "dlogits", "dlines"):
        bad = int(torch.isnan(got[name]).sum())
        assert bad == 0, "%s: %d elements of %s are NaN (not written, or inf * 0)" % (c.text, bad, name)
    for name, worst in SR.check(c, got, inp).items():
        _note(SR.key_of(c, name), worst, "%s %s" % (c.text, name))


@pytest.mark.parametrize("args", SR.rejected(), ids=[r[0] for r in SR.rejected()])
def test_set_losses_return_codes(dev, args):
    """Returned before anything is launched: every output keeps its bytes."""
    name, (L, B, Q, cap, K, D), gamma, rc = args
    n = max(cap, 1)
    z = lambda *shape, dtype=torch.float32: torch.zeros(*shape, dtype=dtype, device="cuda")          # noqa: E731
    logits, lines, tgt, labels = z(L, B, Q, K), z(L, B, Q, D), z(n, D), z(n, dtype=torch.int64)
    bidx, valid, qot = z(n, dtype=torch.int32), torch.ones(n, dtype=torch.int32, device="cuda"), z(L, n, dtype=torch.int32)
    cls_w, num_items, g = torch.ones(K, device="cuda"), torch.ones(1, device="cuda"), torch.ones(L, device="cuda")
    outs = [_guarded((L, B, Q), torch.int32), _guarded((L,)), _guarded((L,)), _guarded((L,)), _guarded((L, B, Q, K)), _guarded((L, B, Q, D))]
    (tc, ce, l1, wsum, dlogits, dlines), p, s = [v[1] for v in outs], hip._ptr, dev._stream(logits)
    wsum_in, tc_in = torch.ones(L, device="cuda"), z(L, B, Q, dtype=torch.int32)
    head = (p(logits), p(lines), p(tgt), p(labels), p(bidx), p(valid), p(qot), p(cls_w), p(num_items), 1.0)
    bhead = (p(logits), p(lines), p(tgt), p(bidx), p(valid), p(qot), p(cls_w), p(num_items), 1.0)
    ftail = (p(tc), p(ce), p(l1), p(wsum), L, B, Q, cap, K, D, s)
    btail = (p(tc_in), p(wsum_in), p(g), p(g), p(dlogits), p(dlines), L, B, Q, cap, K, D, s)
    if gamma is None:
        assert dev.lib.gwd_set_losses_forward(*head, *ftail) == rc and dev.lib.gwd_set_losses_backward(*bhead, *btail) == rc
    else:
        assert dev.lib.gwd_set_losses_focal_forward(*head, gamma, *ftail) == rc
        assert dev.lib.gwd_set_losses_focal_backward(*bhead, gamma, *btail) == rc
    torch.cuda.synchronize()
    for buf, _ in outs:
        ok = torch.isnan(buf) if buf.dtype.is_floating_point else buf == GUARD_INT[buf.dtype]
        assert bool(ok.all()), name + ": an output was written"


# ================================================================================================================== LSAP
def run_lsap(dev, c, inp):
    cost, off = torch.from_numpy(inp["cost"]), torch.from_numpy(inp["off"])
    ops = {"cost": _guarded(cost.shape, values=cost), "off": _guarded(off.shape, torch.int32, values=off)}
    obuf, out = _guarded((LR.LAYERS, cost.shape[-1]), torch.int32, fill=LR.SENTINEL)
    dev.lsap(ops["cost"][1], ops["off"][1], out, max(c.sizes))
    torch.cuda.synchronize()
    _guards_intact(obuf, c.text + " query_of_target")
    _operands_intact(ops, {"cost": cost, "off": off}, c.text)
    return {"query_of_target": out.cpu()}


@pytest.mark.parametrize("c", LSAP, ids=[c.id for c in LSAP])
def test_lsap(dev, c):
    """The assignment equals the sequential reference's exactly (the tie rule makes the argmin independent of the reduction order);
    and, without the reference: a valid matching, surplus and padding on Q, scipy's cost."""
    inp = LR.inputs(c)
    got = _twice(c.text, lambda: run_lsap(dev, c, inp))["query_of_target"].numpy()
    assert LR.SENTINEL not in got, "%s: %d columns were not written" % (c.text, int((got == LR.SENTINEL).sum()))
    ref = LR.reference(c, inp)
    bad = np.argwhere(got != ref)
    assert len(bad) == 0, "%s: %d columns differ from the sequential search, first (layer, column) %s: got %d, reference %d" % (
        c.text, len(bad), bad[0].tolist(), got[tuple(bad[0])], ref[tuple(bad[0])])
    LR.check_matching(c, inp, got)


@pytest.mark.parametrize("args", LR.rejected(), ids=[r[0] for r in LR.rejected()])
def test_lsap_return_codes(dev, args):
    """Returned before anything is launched (Q = 1025 is an argument only, no cost block of that size)."""
    name, (layers, B, Q, sum_targets, max_targets), rc = args
    cost, off = torch.zeros(64, device="cuda"), torch.zeros(B + 1, dtype=torch.int32, device="cuda")
    obuf, out = _guarded((64,), torch.int32)
    p = hip._ptr
    assert dev.lib.gwd_lsap(p(cost), p(off), p(out), layers, B, Q, sum_targets, max_targets, dev._stream(cost)) == rc
    torch.cuda.synchronize()
    assert bool((obuf == GUARD_INT[torch.int32]).all()), name + ": the assignment was written"


# ============================================================================================================= sine positions
def run_pos(dev, c, inp):
    """A level with an embedding goes through the raw entry point in ONE call (mask, counts and embedding); a level without one
    through pos_counts; an emit-only call through pos_emit."""
    ops, outs, what = {}, {}, c.text
    if c.F:
        ops["dim_t"] = _guarded((c.F,), values=inp["dim_t"])
        outs["out"] = _guarded((c.B, c.h, c.w, 2 * c.F))
    if c.mask is not None:
        ops["mask"] = _guarded((c.B, c.H, c.W), torch.uint8, values=inp["mask"].to(torch.uint8))
        outs["mask"] = _guarded((c.B, c.h, c.w), torch.uint8, fill=PR.MASK_SENTINEL)
        outs["counts"] = _guarded((c.B, c.h, c.w, 2), torch.int16, fill=PR.COUNT_SENTINEL)
        if c.F:
            p = hip._ptr
            rc = dev.lib.gwd_pos_sine(p(ops["mask"][1]), p(outs["mask"][1]), p(outs["counts"][1]), p(ops["dim_t"][1]), p(outs["out"][1]),
                                      c.B, c.H, c.W, c.h, c.w, c.F, c.normalize, dev._stream(ops["mask"][1]))
            assert rc == 0, (what, rc)
        else:
            dev.pos_counts(ops["mask"][1], outs["mask"][1], outs["counts"][1])
    else:
        ops["counts"] = _guarded((c.B, c.h, c.w, 2), torch.int16, values=inp["counts"])
        dev.pos_emit(ops["counts"][1], ops["dim_t"][1], outs["out"][1], c.normalize)
    torch.cuda.synchronize()
    for k, (buf, view) in outs.items():
        _guards_intact(buf, "%s %s" % (what, k))
    _operands_intact(ops, {"mask": inp["mask"].to(torch.uint8) if c.mask is not None else None, "dim_t": inp["dim_t"], "counts": inp.get("counts")}, what)
    return {k: v[1].cpu() for k, v in outs.items()}


@pytest.mark.parametrize("c", POS, ids=[c.id for c in POS])
def test_pos_sine(dev, c):
    inp = PR.inputs(c)
    got = _twice(c.text, lambda: run_pos(dev, c, inp))
    if c.mask is not None:
        assert not bool((got["mask"] == PR.MASK_SENTINEL).any()) and not bool((got["counts"] == PR.COUNT_SENTINEL).any()), c.text + ": not written"
    if c.F:
        bad = int(torch.isnan(got["out"]).sum())
        assert bad == 0, "%s: %d elements of the embedding were not written" % (c.text, bad)
    worst = PR.check(c, got, inp)
    if c.F:
        _note(PR.KEY, worst, c.text)


@pytest.mark.parametrize("args", PR.rejected(), ids=[r[0] for r in PR.rejected()])
def test_pos_sine_return_codes(dev, args):
    """Returned before a launch (the sizes are arguments only: no buffer of that size): every output keeps its bytes."""
    name, (B, h, w, F, with_mask), rc = args
    mask, dim_t = torch.zeros(64, dtype=torch.uint8, device="cuda"), torch.ones(8, device="cuda")
    outs = [_guarded((64,), torch.uint8), _guarded((64,), torch.int16), _guarded((64,))]
    lvl, counts, out = [v[1] for v in outs]
    p = hip._ptr
    got = dev.lib.gwd_pos_sine(p(mask) if with_mask else None, p(lvl) if with_mask else None, p(counts), p(dim_t), p(out), B, 8 if with_mask else 0,
                               8 if with_mask else 0, h, w, F, 1, dev._stream(mask))
    assert got == rc
    torch.cuda.synchronize()
    for buf, _ in outs:
        ok = torch.isnan(buf) if buf.dtype.is_floating_point else buf == GUARD_INT[buf.dtype]
        assert bool(ok.all()), name + ": an output was written"


# ============================================================================================================== report
def test_worst_ratios_are_reported(dev):
    """Prints the worst ratio per (operation, output, type) of the cases above."""
    consts = dict(SR.C)
    consts.update(PR.C)
    assert len(WORST) == len(consts) or len(WORST) == 0       # (0: this test was selected on its own)
    for key, w in sorted(WORST.items()):
        print("criterion witnesses: %-10s %-7s %-4s worst ratio %.3f of C = %.1f" % (key + (w, consts[key])))
        assert w <= consts[key]
