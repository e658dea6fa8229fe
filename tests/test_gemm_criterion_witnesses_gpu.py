"""GPU: gwd_bmm, gwd_match_cost and gwd_plane_loss_forward / _backward, run through hip.library() at every case of tests/bmm_ref.py,
tests/matchcost_ref.py and tests/plane_loss_ref.py and compared ELEMENT by element, every element of every output, with the fp64
references there: bound C u (|ref| + cond) with C from the CPU rounding models (never from a kernel's output), equality for the
counts.  Every output is NaN before the call (an added-to GEMM result holds its c0), every operand and output has NaN guard elements
on both sides, a GEMM operand is a view of a NaN-filled buffer laid out as on the CPU, and every call whose summation order is fixed
is made twice and must return identical bits (a split-K GEMM adds its slices with atomics in any order: no bit equality there).

tests/test_gemm_criterion_witnesses.py proves on the CPU that the cases reach the launch edges they claim.  Run the file with -x: a
fault is a finding."""
import collections
import ctypes

import numpy as np
import pytest
import torch

from gw_depth_amd import hip
from tests import bmm_ref as BR
from tests import matchcost_ref as MR
from tests import plane_loss_ref as PR

pytestmark = pytest.mark.gpu
WORST = collections.defaultdict(float)            # (operation, output, type) -> worst ratio over the file
GUARD = 8                                         # elements: 16 bytes of bf16, 32 of fp32 - the views stay 16-byte aligned
BMM, COST, PLANE = BR.cases(), MR.cases(), PR.cases()


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    hip.set_library(None)
    torch.set_num_threads(16)
    return hip.library()


def _guarded(shape, dtype=torch.float32, values=None, fill=float("nan")):
    """-> (buffer, view): a tensor of `shape` inside a NaN-filled allocation, GUARD NaNs in front of it and behind it."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=dtype, device="cuda")
    view = buf[GUARD:GUARD + n].view(shape)
    if values is not None:
        view.copy_(torch.as_tensor(values).reshape(shape))
    elif fill == fill:
        view.fill_(fill)
    return buf, view


def _guards_intact(buf, what):
    assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all()), "%s: written outside its range" % what


def _bits(t):
    return t.contiguous().view({torch.bfloat16: torch.int16, torch.float32: torch.int32, torch.float64: torch.int64}[t.dtype])


def _twice(what, call, same_bits=True):
    """call() -> {name: CPU tensor}; made twice from fresh buffers: the same bits."""
    first, second = call(), call()
    for name in first:
        assert not same_bits or torch.equal(_bits(first[name]), _bits(second[name])), "%s %s: two calls, different bits" % (what, name)
    return first


def _note(key, worst, what):
    WORST[key] = max(WORST[key], worst)
    print("%s: worst ratio %.3f" % (what, worst))


# ========================================================================================================== batched GEMM
def _device_view(op):
    """The operand's buffer on the device, NaN guards around it, and the same view of it."""
    buf, flat = _guarded(op.base.shape, op.base.dtype, values=op.base)
    return buf, torch.as_strided(buf, op.size, op.stride, GUARD + op.offset)


def run_bmm(dev, c, inp):
    a, b = _device_view(inp["a"]), _device_view(inp["b"])
    assert a[1].data_ptr() % 16 == (inp["a"].offset * a[1].element_size()) % 16            # laid out as the CPU model assumes
    cbuf, out = _guarded((c.nb0, c.nb1, c.M, c.N), torch.float32 if c.accumulate else BR.torch_dtype(c), values=inp["c0"])
    dev.bmm(a[1], b[1], out, c.M, c.N, c.K, a_kmajor=c.akm, b_kmajor=c.bkm, alpha=c.alpha, accumulate=c.accumulate, splits=c.splits)
    torch.cuda.synchronize()
    _guards_intact(cbuf, c.text + " c")
    for (buf, view), op, name in ((a, inp["a"], "a"), (b, inp["b"], "b")):
        _guards_intact(buf, "%s %s" % (c.text, name))
        assert torch.equal(_bits(view.cpu()), _bits(op.view)), name + " was written"
    return {"c": out.cpu()}


@pytest.mark.parametrize("c", BMM, ids=[c.id for c in BMM])
def test_bmm(dev, c):
    inp = BR.inputs(c)
    got = _twice(c.text, lambda: run_bmm(dev, c, inp), same_bits=BR.launch(c).grid_z == 1)["c"]
    assert not bool(torch.isnan(got.float()).any()), "%s: %d elements are NaN (not written, or read outside an operand)" % (
        c.text, int(torch.isnan(got.float()).sum()))
    _note(BR.key_of(c), BR.check(c, got, inp), c.text)


@pytest.mark.parametrize("args", BR.rejected(), ids=[r[0] for r in BR.rejected()])
def test_bmm_return_codes(dev, args):
    """Returned before anything is launched: the result keeps its bytes (batch=65536 is a descriptor only, no buffer of that size)."""
    name, over, rc = args
    a, b = torch.ones(1, 1, 8, 8, device="cuda"), torch.ones(1, 1, 8, 8, device="cuda")
    cbuf, out = _guarded((1, 1, 8, 8))
    d = hip.BmmDesc()
    d.a, d.b, d.c = a.data_ptr(), b.data_ptr(), out.data_ptr()
    d.a_sb0 = d.a_sb1 = d.b_sb0 = d.b_sb1 = d.c_sb0 = d.c_sb1 = 0 if name.startswith("batch") else 64
    d.a_ld = d.b_ld = d.c_ld = 8
    d.M = d.N = d.K = 8
    d.nb0 = d.nb1 = d.splits = 1
    d.alpha, d.dtype = 1.0, hip.F32
    for k, v in over.items():
        setattr(d, k, v)
    assert dev.lib.gwd_bmm(ctypes.byref(d), dev._stream(a)) == rc
    torch.cuda.synchronize()
    assert bool(torch.isnan(cbuf).all()), name + ": the result was written"


# ============================================================================================================ match cost
def run_cost(dev, c, inp):
    ops = {k: _guarded(inp[k].shape, inp[k].dtype, values=inp[k]) for k in ("logits", "lines", "tgt")}
    labels = inp["labels"].cuda()
    cbuf, cost = _guarded((c.L, c.B, c.Q, c.cap))
    dev.match_cost(ops["logits"][1], ops["lines"][1], ops["tgt"][1], labels, cost, c.w_line, c.w_class)
    torch.cuda.synchronize()
    _guards_intact(cbuf, c.text + " cost")
    for k, (buf, view) in ops.items():
        _guards_intact(buf, "%s %s" % (c.text, k))
        assert torch.equal(view.cpu(), inp[k]), k + " was written"
    assert torch.equal(labels.cpu(), inp["labels"])
    return {"cost": cost.cpu()}


@pytest.mark.parametrize("c", COST, ids=[c.id for c in COST])
def test_match_cost(dev, c):
    inp = MR.inputs(c)
    got = _twice(c.text, lambda: run_cost(dev, c, inp))["cost"]
    assert not bool(torch.isnan(got).any()), "%s: %d costs were not written" % (c.text, int(torch.isnan(got).sum()))
    _note(MR.KEY, MR.check(c, got, inp), c.text)


@pytest.mark.parametrize("args", MR.rejected(), ids=[r[0] for r in MR.rejected()])
def test_match_cost_return_codes(dev, args):
    name, (L, B, Q, cap, K, D), rc = args
    logits, lines = torch.zeros(L, B, Q, K, device="cuda"), torch.zeros(L, B, Q, D, device="cuda")
    tgt, labels = torch.zeros(max(cap, 1), D, device="cuda"), torch.zeros(max(cap, 1), dtype=torch.int64, device="cuda")
    cbuf, cost = _guarded((L, B, Q, max(cap, 1)))
    p = hip._ptr
    assert dev.lib.gwd_match_cost(p(logits), p(lines), p(tgt), p(labels), p(cost), L, B, Q, cap, K, D, 5.0, 2.0, dev._stream(logits)) == rc
    torch.cuda.synchronize()
    assert bool(torch.isnan(cbuf).all()), name + ": the cost block was written"


# ============================================================================================================ plane loss
def run_plane(dev, c, inp):
    dt = PR.torch_dtype(c)
    depth = _guarded((c.H, c.W), dt, values=inp["depth"])
    valid, tri, n_planes, gloss = inp["valid"].cuda(), inp["tri"].cuda(), inp["n_planes"].cuda(), inp["gloss"].cuda()
    sbuf, stats = _guarded((4 * c.P + 1,), torch.float64)
    lbuf, loss = _guarded((1,))
    gbuf, gdepth = _guarded((c.H, c.W), dt)
    ws = torch.full((dev.workspace_bytes(hip.WS_PLANE, c.P, c.H * c.W) // 8,), float("nan"), dtype=torch.float64, device="cuda")
    dev.plane_loss_forward(depth[1], valid, tri, n_planes, c.P, c.H, c.W, c.min_area, ws, stats, loss)
    dev.plane_loss_backward(depth[1], valid, tri, n_planes, c.P, c.H, c.W, stats, gloss, gdepth)
    torch.cuda.synchronize()
    for buf, name in ((sbuf, "stats"), (lbuf, "loss"), (gbuf, "gdepth"), (depth[0], "depth")):
        _guards_intact(buf, "%s %s" % (c.text, name))
    assert torch.equal(_bits(depth[1].cpu()), _bits(inp["depth"])) and torch.equal(valid.cpu(), inp["valid"]) and torch.equal(tri.cpu(), inp["tri"])
    return {"stats": stats.cpu(), "loss": loss.cpu(), "gdepth": gdepth.cpu()}


@pytest.mark.parametrize("c", PLANE, ids=[c.id for c in PLANE])
def test_plane_loss(dev, c):
    inp = PR.inputs(c)
    out = _twice(c.text, lambda: run_plane(dev, c, inp))
    for name in ("stats", "loss", "gdepth"):
        bad = int(torch.isnan(out[name].double()).sum())
        assert bad == 0, "%s: %d elements of %s are NaN (not written)" % (c.text, bad, name)
    got = dict(PR.split_stats(out["stats"], c.P), loss=out["loss"], gdepth=out["gdepth"])
    for name, worst in PR.check(c, got, inp).items():
        _note(PR.key_of(c, name), worst, "%s %s" % (c.text, name))


@pytest.mark.parametrize("args", PR.rejected(), ids=[r[0] for r in PR.rejected()])
def test_plane_loss_return_codes(dev, args):
    """Returned before anything is launched (H = 32769 takes no map of that size): every output keeps its NaNs."""
    name, P, H, W, code, rc = args
    depth, valid = torch.ones(8, 8, device="cuda"), torch.ones(8, 8, dtype=torch.uint8, device="cuda")
    tri, n_planes = torch.zeros(P, 6, dtype=torch.int64, device="cuda"), torch.ones(1, dtype=torch.int32, device="cuda")
    gloss = torch.ones(1, device="cuda")
    sbuf, stats = _guarded((4 * P + 1,), torch.float64)
    lbuf, loss = _guarded((1,))
    gbuf, gdepth = _guarded((8, 8))
    ws = torch.full((PR.PMAX * PR.FWD_MAX_BLOCKS * 5,), float("nan"), dtype=torch.float64, device="cuda")
    p = hip._ptr
    s = dev._stream(depth)
    assert dev.lib.gwd_plane_loss_forward(p(depth), p(valid), p(tri), p(n_planes), P, H, W, 1, p(ws), p(stats), p(loss), code, s) == rc
    assert dev.lib.gwd_plane_loss_backward(p(depth), p(valid), p(tri), p(n_planes), P, H, W, p(stats), p(gloss), p(gdepth), code, s) == rc
    torch.cuda.synchronize()
    for buf in (sbuf, lbuf, gbuf, ws):
        assert bool(torch.isnan(buf).all()), name + ": an output was written"


# ============================================================================================================== report
def test_worst_ratios_are_reported(dev):
    """Prints the worst ratio per (operation, output, type) of the cases above."""
    consts = dict(BR.C)
    consts.update(MR.C)
    consts.update(PR.C)
    assert len(WORST) == len(consts) or len(WORST) == 0       # (0: this test was selected on its own)
    for key, w in sorted(WORST.items()):
        print("gemm and criterion witnesses: %-10s %-6s %-4s worst ratio %.3f of C = %.1f" % (key + (w, consts[key])))
        assert w <= consts[key]
