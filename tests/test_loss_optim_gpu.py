"""GPU: the nine entry points of csrc/losses.hip and csrc/optim.hip, run through the hip.py wrappers at every case of tests/loss_ref.py
and compared ELEMENT by element, every element of every output, with the fp64 reference there: bound c u (|ref| + cond), c from the
CPU rounding model (never from a kernel's output), exact values where the bound is zero.  Every output is NaN before the call, the
ACCUMULATED ones (sq, the CE sum, danchor) hold a non-zero prefill that the reference adds, every buffer has NaN guard elements around
the range the call may touch, and the kernels that take sums are fed the reference's fp64 sums (the chained cases: the device's own).

tests/test_loss_optim.py proves on the CPU that the cases reach the launch edges they claim.  Run the file with -x: a fault is a finding."""
import collections

import pytest
import torch

from gw_depth_amd import hip, ops
from tests import loss_ref as R

pytestmark = pytest.mark.gpu
TABLE = R.cases()
WORST = collections.defaultdict(float)            # (operation, output, type) -> worst ratio over the file
GUARD = 8


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    hip.set_library(None)
    torch.set_num_threads(16)
    return hip.library()


def _guarded(n, dtype=torch.float32, off=0, values=None):
    """-> (buffer, view): `n` elements that start `off` elements into a NaN-filled allocation with GUARD more NaNs behind them."""
    buf = torch.full((off + n + GUARD,), float("nan"), dtype=dtype, device="cuda")
    view = buf[off:off + n]
    if values is not None:
        view.copy_(values.reshape(-1))
    return buf, view


def _guards_intact(buf, off, n, what):
    assert bool(torch.isnan(buf[:off]).all()) and bool(torch.isnan(buf[off + n:]).all()), "%s: written outside [0, n)" % what


def run_adamw(dev, c, inp, wd=None):
    prm = R.adamw_params(c)
    n, off = c.n, c.off
    bufs = {k: _guarded(n, off=off, values=inp[k]) for k in ("p", "g", "m", "v")}
    p16 = None if c.var == "nop16" else _guarded(n, torch.bfloat16, off)
    fed = R.feeds(c, inp)
    if c.chained:
        sq = torch.zeros(1, dtype=torch.float64, device="cuda")
        dev.sqnorm(bufs["g"][1], sq, n)
    else:
        sq = None if fed is None else fed["sq"].cuda()
    dev.adamw_step(bufs["p"][1], bufs["g"][1], bufs["m"][1], bufs["v"][1], None if p16 is None else p16[1], sq, n, prm["lr"], prm["b1"], prm["b2"],
                   prm["eps"], prm["wd"] if wd is None else wd, prm["bc1"], prm["bc2"], prm["max_norm"], prm["gs"])
    torch.cuda.synchronize()
    for k, (buf, _) in bufs.items():
        _guards_intact(buf, off, n, c.text + " " + k)
    assert torch.equal(bufs["g"][1].cpu(), inp["g"]), "g was written"
    out = {k: bufs[k][1].cpu() for k in ("p", "m", "v")}
    if p16 is not None:
        _guards_intact(p16[0], off, n, c.text + " p16")
        out["p16"] = p16[1].cpu()
    return out


def run(dev, c, inp):
    """The case on the device -> its outputs (CPU tensors)."""
    out = {}
    if c.family == "sqnorm":
        buf, _ = _guarded(c.n, values=inp["g"])                  # the allocation, not the view: an empty view's address is NULL
        sq = torch.full((1,), R.SQ_PREFILL, dtype=torch.float64, device="cuda")
        dev.sqnorm(buf, sq, c.n)                                 # (the NaN guards behind n would poison the sum if they were read)
        out["sq"] = sq.cpu()
    elif c.family == "adamw":
        out = run_adamw(dev, c, inp)
        if c.ps.startswith("ship"):                              # 1.0f - lr wd == 1.0f: the shipped decay is the identity, bit for bit
            assert torch.equal(run_adamw(dev, c, inp, wd=0.0)["p"], out["p"])
    elif c.family == "silog":
        B, h, w, H, W = c.B, c.h, c.w, c.H, c.W
        pred, gt = inp["pred"].cuda(), inp["gt"].cuda()
        sums = torch.zeros(3, dtype=torch.float64, device="cuda")
        dev.silog_sums(pred, gt, sums, B, h, w, H, W, c.log_err)
        fed = R.feeds(c, inp)
        sums_in = sums if fed is None else fed["sums"].cuda()
        lbuf, loss = _guarded(1)
        dev.silog_finalize(sums_in, R.LAMBDA, 10.0 * R.LOSS_WEIGHT, loss)
        gbuf, gpred = _guarded(B * h * w, R.torch_dtype(c))
        gloss = torch.tensor([R.GLOSS], device="cuda")
        dev.silog_backward(pred, gt, sums_in, gloss, R.LOSS_WEIGHT, R.LAMBDA, gpred, B, h, w, H, W, c.log_err)
        torch.cuda.synchronize()
        _guards_intact(lbuf, 0, 1, c.text + " loss")
        _guards_intact(gbuf, 0, B * h * w, c.text + " gpred")
        s = sums.cpu()
        out.update(s0=s[0:1], s1=s[1:2], count=s[2:3], loss=loss.cpu(), gpred=gpred.cpu().view(B, h, w))
    elif c.family == "seg_ce":
        logits, target = inp["logits"].cuda(), inp["target"].cuda()
        total = torch.full((1,), R.CE_PREFILL, dtype=torch.float64, device="cuda")
        dev.seg_ce_sum(logits, target, total, c.P)
        gbuf, gl = _guarded(2 * c.P, R.torch_dtype(c))
        dev.seg_ce_backward(logits, target, torch.tensor([R.GLOSS], device="cuda"), R.CE_SCALE, gl, c.P)
        torch.cuda.synchronize()
        _guards_intact(gbuf, 0, 2 * c.P, c.text + " gl")
        out.update(sum=total.cpu(), gl=gl.cpu().view(c.P, 2))
    else:
        B, P, Rr = c.B, c.P, c.R
        att, anchor, gp = inp["att"].cuda(), inp["anchor"].cuda(), inp["gpred"].cuda()
        pbuf, pred = _guarded(B * P)
        dev.anchor_depth_forward(att, anchor, pred, B, P, Rr)
        dbuf, datt = _guarded(B * P * Rr, R.torch_dtype(c))
        danchor = R.pattern(Rr)[None].expand(B, Rr).contiguous().cuda()
        alone = danchor.clone()
        dev.anchor_depth_backward(att, anchor, gp, datt, danchor, B, P, Rr)
        dev.anchor_depth_backward(att, anchor, gp, None, alone, B, P, Rr)
        torch.cuda.synchronize()
        _guards_intact(pbuf, 0, B * P, c.text + " pred")
        _guards_intact(dbuf, 0, B * P * Rr, c.text + " datt")
        out.update(pred=pred.cpu().view(B, P), datt=datt.cpu().view(B, P, Rr), danchor=danchor.cpu(), danchor_nodatt=alone.cpu())
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("c", TABLE, ids=[c.id for c in TABLE])
def test_case(dev, c):
    inp = R.inputs(c)
    got = run(dev, c, inp)
    for name, worst in R.check(c, got, inp).items():
        WORST[R.key_of(c, name)] = max(WORST[R.key_of(c, name)], worst)
        print("%s %s: worst ratio %.3f" % (c.text, name, worst))


def test_worst_ratios_are_reported(dev):
    """Prints the worst ratio per (operation, output, type) of the cases above (DESIGN.md section 16 holds a copy)."""
    assert len(WORST) == len(R.C) or len(WORST) == 0          # (0: this test was selected on its own)
    for key, w in sorted(WORST.items()):
        print("loss / optimizer kernels: %-15s %-7s %-4s worst ratio %.3f of C = %.1f" % (key + (w, R.C[key])))


# ---------------------------------------------------------------------------------------- the return codes of include/gwdepth.h
def test_sqnorm_return_codes_leave_sq_untouched(dev):
    buf = torch.ones(64, device="cuda")
    sq = torch.full((1,), R.SQ_PREFILL, dtype=torch.float64, device="cuda")
    stream = dev._stream(buf, sq)
    assert buf.data_ptr() % 16 == 0
    assert dev.lib.gwd_sqnorm(hip._ptr(buf[1:]), hip._ptr(sq), 40, stream) == -3          # g 4 bytes past a 16-byte boundary
    assert dev.lib.gwd_sqnorm(None, hip._ptr(sq), 40, stream) == -1
    assert dev.lib.gwd_sqnorm(hip._ptr(buf), None, 40, stream) == -1
    torch.cuda.synchronize()
    assert float(sq.cpu()) == R.SQ_PREFILL


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_anchor_depth_with_257_channels_returns_minus_1(dev, dtype):
    B, P, Rr = 2, 5, 257
    dt = torch.bfloat16 if dtype == "bf16" else torch.float32
    att = torch.ones(B, P, Rr, dtype=dt, device="cuda")
    anchor, gp = torch.ones(B, Rr, device="cuda"), torch.ones(B, P, device="cuda")
    pred = torch.full((B, P), float("nan"), device="cuda")
    datt = torch.full((B, P, Rr), float("nan"), dtype=dt, device="cuda")
    danchor = R.pattern(Rr)[None].expand(B, Rr).contiguous().cuda()
    p, stream = hip._ptr, dev._stream(att)
    assert dev.lib.gwd_anchor_depth_forward(p(att), p(anchor), p(pred), B, P, Rr, hip.dtype_code(att), stream) == -1
    assert dev.lib.gwd_anchor_depth_backward(p(att), p(anchor), p(gp), p(datt), p(danchor), B, P, Rr, hip.dtype_code(att), stream) == -1
    torch.cuda.synchronize()
    assert bool(torch.isnan(pred).all()) and bool(torch.isnan(datt).all()) and torch.equal(danchor.cpu(), R.pattern(Rr)[None].expand(B, Rr))


# ------------------------------------------------------------------------- the autograd nodes of ops.py against the same reference
def _pick(family, dtype, **kw):
    return next(c for c in TABLE if c.family == family and c.dtype == dtype and all(getattr(c, k) == v for k, v in kw.items()))


@pytest.mark.parametrize("layout", ["B,h,w,1", "B,1,h,w"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_silog_loss_autograd(dev, dtype, layout):
    """ops.silog_loss: both accepted layouts, 10 weight as the finalize scale, weight and the incoming gradient in the backward; the node
    feeds the device's own sums, so the case is the chained one."""
    c = _pick("silog", dtype, chained=1)
    inp = R.inputs(c)
    shape = (c.B, c.h, c.w, 1) if layout == "B,h,w,1" else (c.B, 1, c.h, c.w)
    pred = inp["pred"].cuda().view(shape).requires_grad_()
    loss = ops.silog_loss(pred, inp["gt"].cuda().view(c.B, 1, c.H, c.W), weight=R.LOSS_WEIGHT, variance_focus=R.LAMBDA, log_depth_error=bool(c.log_err))
    loss.backward(torch.tensor(R.GLOSS, device="cuda"))
    torch.cuda.synchronize()
    assert loss.shape == () and pred.grad.shape == shape and pred.grad.dtype == pred.dtype
    ref, cond = R.reference(c, inp)
    for name, got in (("loss", loss.detach().cpu().reshape(1)), ("gpred", pred.grad.cpu().view(c.B, c.h, c.w))):
        R.assert_elementwise(got, ref[name], cond[name], R.C[R.key_of(c, name)], ("image", "row", "column")[:got.dim()], u=R.out_unit(c, name), what="ops.silog_loss " + name)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_seg_cross_entropy_autograd(dev, dtype):
    """ops.seg_cross_entropy: (B,H,W,2) logits, the sum from zero times scale / P in fp64 and rounded ONCE to fp32 (one more unit of c),
    scale / P and the incoming gradient in the backward."""
    c = _pick("seg_ce", dtype, P=256, kind="spread", target="mixed")
    inp = R.inputs(c)
    logits = inp["logits"].cuda().view(2, 8, 16, 2).requires_grad_()
    loss = ops.seg_cross_entropy(logits, inp["target"].cuda().view(2, 8, 16), scale=R.CE_SCALE)
    loss.backward(torch.tensor(R.GLOSS, device="cuda"))
    torch.cuda.synchronize()
    ref, cond = R.reference(c, inp)
    k = R.CE_SCALE / c.P
    R.assert_elementwise(loss.detach().cpu().reshape(1), (ref["sum"] - R.CE_PREFILL) * k, (cond["sum"][0] * k, None), R.C[R.key_of(c, "sum")] + 1.0, ("element",),
                         u=R.U_F32, what="ops.seg_cross_entropy loss")
    assert logits.grad.shape == logits.shape and logits.grad.dtype == logits.dtype
    R.assert_elementwise(logits.grad.cpu().view(c.P, 2), ref["gl"], cond["gl"], R.C[R.key_of(c, "gl")], ("pixel", "class"), u=R.out_unit(c, "gl"),
                         what="ops.seg_cross_entropy gradient")


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_anchor_depth_autograd(dev, dtype):
    """ops.anchor_depth: danchor accumulated from the zeros the node allocates, datt in the storage type."""
    c = _pick("anchor", dtype, P=37, R=100)
    inp = R.inputs(c)
    att, anchor = inp["att"].cuda().requires_grad_(), inp["anchor"].cuda().requires_grad_()
    pred = ops.anchor_depth(att, anchor)
    pred.backward(inp["gpred"].cuda())
    torch.cuda.synchronize()
    ref, cond = R.reference(c, inp)
    pre = R.pattern(c.R).double()[None]
    ref["danchor"], cond["danchor"] = ref["danchor"] - pre, (cond["danchor"][0] - pre, None)
    for name, got in (("pred", pred.detach()), ("datt", att.grad), ("danchor", anchor.grad)):
        assert got.dtype == (att.dtype if name == "datt" else torch.float32)
        R.assert_elementwise(got.cpu(), ref[name], cond[name], R.C[R.key_of(c, name)], ("image", "pixel", "channel")[:got.dim()], u=R.out_unit(c, name),
                             what="ops.anchor_depth " + name)
