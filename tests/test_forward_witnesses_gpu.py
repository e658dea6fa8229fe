"""GPU: gwd_certain_sample, gwd_stem_pack / gwd_stem_forward and gwd_inorm_gelu_forward / _backward, run through the hip.py wrappers at
every case of tests/sample_ref.py, tests/stem_ref.py and tests/inorm_ref.py and compared ELEMENT by element, every element of every
output, with the fp64 references there: bound C u (|ref| + cond) with C from the CPU rounding models (never from a kernel's output),
equality where the bound is zero (the coordinates, the packed weights, the channels shifted by -1000).  Every output is NaN before
the call (the stem's y: -1, a NaN would hide in a maximum), every operand and output has NaN guard elements on both sides, inorm's
workspace is NaN before each of its two calls, and every call is made twice and must return identical bits.

tests/test_forward_witnesses.py proves on the CPU that the cases reach the launch edges they claim.  Run the file with -x: a fault is
a finding."""
import collections

import numpy as np
import pytest
import torch

from gw_depth_amd import hip
from tests import inorm_ref as IR
from tests import sample_ref as SR
from tests import stem_ref as TR

pytestmark = pytest.mark.gpu
WORST = collections.defaultdict(float)            # (operation, output, type) -> worst ratio over the file
GUARD = 8                                         # elements: 16 bytes of bf16, 32 of fp32 - the views stay 16-byte aligned
SAMPLE, STEM, INORM = SR.cases(), TR.cases(), IR.cases()


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
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _twice(what, call):
    """call() -> {name: CPU tensor}; made twice from fresh buffers: the same bits."""
    first, second = call(), call()
    for name in first:
        assert torch.equal(_bits(first[name]), _bits(second[name])), "%s %s: two calls, different bits" % (what, name)
    return first


# ======================================================================================================== CertainSample
def run_sample(dev, c, inp):
    small = _guarded(inp["small"].shape, values=inp["small"])
    large = _guarded(inp["large"].shape, values=inp["large"])
    edges = _guarded(inp["edges"].shape, values=inp["edges"])
    cbuf, coords = _guarded((c.B, c.S, 1, 2))
    dev.certain_sample(small[1], large[1], coords, edges[1], c.S)
    torch.cuda.synchronize()
    _guards_intact(cbuf, c.text + " coords")
    for name, (buf, view) in (("small", small), ("large", large), ("edges", edges)):
        _guards_intact(buf, c.text + " " + name)
        assert torch.equal(view.cpu(), torch.as_tensor(inp[name])), name + " was written"
    return {"coords": coords.cpu()}


@pytest.mark.parametrize("c", SAMPLE, ids=[c.id for c in SAMPLE])
def test_certain_sample(dev, c):
    inp = SR.inputs(c)
    ref, cond = SR.reference(c, inp)
    got = _twice(c.text, lambda: run_sample(dev, c, inp))["coords"].numpy()
    assert got.shape == ref.shape and not np.isnan(got).any(), "%s: %d coordinates were not written" % (c.text, int(np.isnan(got).sum()))
    bad = np.nonzero((got != ref).any(axis=(2, 3)))
    if len(bad[0]):
        b, s = int(bad[0][0]), int(bad[1][0])
        raise AssertionError("%s: %d of %d points differ; first at image %d, point %d: got %r, reference %r (branch %s, k %r)"
                             % (c.text, len(bad[0]), c.B * c.S, b, s, got[b, s, 0].tolist(), ref[b, s, 0].tolist(), cond["branch"][b], cond["ks"][b]))
    WORST[("certain_sample", "coords", "f32")] = max(WORST[("certain_sample", "coords", "f32")], 0.0)


@pytest.mark.parametrize("args", SR.rejected(), ids=["HW>36864", "S>256", "S>HW", "n_int>8"])
def test_certain_sample_rejects_with_minus_4(dev, args):
    B, hs, ws, H, W, S, n_int = args
    small, large = torch.rand(B, 1, hs, ws, device="cuda"), torch.rand(B, 1, H, W, device="cuda")
    edges = torch.linspace(0, 1, n_int + 1, device="cuda")
    cbuf, coords = _guarded((B, S, 1, 2))
    p = hip._ptr
    assert dev.lib.gwd_certain_sample(p(small), p(large), p(coords), B, hs, ws, H, W, p(edges), n_int, S, dev._stream(small)) == -4
    torch.cuda.synchronize()
    assert bool(torch.isnan(cbuf).all())
    with pytest.raises(RuntimeError):
        dev.certain_sample(small, large, coords, edges, S)


# ================================================================================================================= stem
def run_stem_pack(dev, c, inp):
    w = _guarded(inp["w"].shape, values=inp["w"])
    scale = None if inp["scale"] is None else _guarded((64,), values=inp["scale"])
    pbuf, packed = _guarded((TR.PACKED,), torch.bfloat16)
    dev.stem_pack(w[1], None if scale is None else scale[1], packed)
    torch.cuda.synchronize()
    _guards_intact(pbuf, c.text + " packed")
    return {"packed": packed.cpu()}


def run_stem(dev, c, inp, packed):
    L = TR.launch(c)
    x = _guarded(inp["x"].shape, torch.bfloat16, values=inp["x"])
    pk = _guarded((TR.PACKED,), torch.bfloat16, values=packed)
    shift = None if inp["shift"] is None else _guarded((64,), values=inp["shift"])
    ybuf, y = _guarded((c.B, L.Hp, L.Wp, 64), torch.bfloat16, fill=-1.0)
    dev.stem_forward(x[1], pk[1], None if shift is None else shift[1], y)
    torch.cuda.synchronize()
    _guards_intact(ybuf, c.text + " y")
    assert torch.equal(x[1].cpu(), inp["x"]), "x was written"
    return {"y": y.cpu()}


@pytest.mark.parametrize("c", STEM, ids=[c.id for c in STEM])
def test_stem(dev, c):
    inp = TR.inputs(c)
    packed = _twice(c.text, lambda: run_stem_pack(dev, c, inp))["packed"]
    want = TR.pack_reference(inp["w"], inp["scale"])
    diff = _bits(packed) != _bits(want)                        # the bound is zero; -0 against +0 counts
    assert not bool(diff.any()), "%s: %d packed values differ, first at index %d" % (c.text, int(diff.sum()), int(torch.nonzero(diff)[0]))
    got = _twice(c.text, lambda: run_stem(dev, c, inp, packed))["y"]
    assert bool((got >= 0).all()), "%s: %d outputs were not written" % (c.text, int((got < 0).sum()))
    worst = TR.check(c, got, inp, packed)
    WORST[TR.KEY] = max(WORST[TR.KEY], worst)
    print("%s y: worst ratio %.3f" % (c.text, worst))


def test_stem_return_codes(dev):
    x32 = torch.zeros(1, 8, 8, 3, device="cuda")
    pk = torch.zeros(TR.PACKED, dtype=torch.bfloat16, device="cuda")
    ybuf, y = _guarded((1, 2, 2, 64), torch.bfloat16, fill=-1.0)
    p = hip._ptr
    assert dev.lib.gwd_stem_forward(p(x32), p(pk), None, p(y), 1, 8, 8, hip.F32, dev._stream(x32)) == -2
    with pytest.raises(ValueError):
        dev.stem_forward(torch.zeros(1, 8, 8, 4, dtype=torch.bfloat16, device="cuda"), pk, None, y)
    torch.cuda.synchronize()
    assert bool((y == -1).all())
    _guards_intact(ybuf, "y")


# ================================================================================================== instance-norm GELU
def run_inorm_forward(dev, c, inp):
    dt = IR.torch_dtype(c)
    B, L, C, S = c.B, c.L, c.C, c.S
    a, u = _guarded((B, L, C), dt, values=inp["a"]), _guarded((B, L, C), dt, values=inp["u"])
    ybuf, y = _guarded((B, L, C), dt)
    pbuf, part = _guarded((B, S, C, 2))
    sbuf, stat = _guarded((B, C, 2))
    dev.inorm_gelu_forward(a[1], u[1], y, part, stat, B, L, C, S, IR.EPS)
    torch.cuda.synchronize()
    for buf, name in ((ybuf, "y"), (pbuf, "part"), (sbuf, "stat"), (a[0], "a"), (u[0], "u")):
        _guards_intact(buf, "%s %s" % (c.text, name))
    assert torch.equal(u[1].cpu(), inp["u"]) and torch.equal(a[1].cpu(), inp["a"])
    st = stat.cpu()
    return {"y": y.cpu(), "mean": st[..., 0].contiguous(), "rstd": st[..., 1].contiguous()}


def run_inorm_backward(dev, c, inp, stat_in):
    dt = IR.torch_dtype(c)
    B, L, C, S = c.B, c.L, c.C, c.S
    gy, u = _guarded((B, L, C), dt, values=inp["gy"]), _guarded((B, L, C), dt, values=inp["u"])
    stat = _guarded((B, C, 2), values=stat_in)
    pbuf, part = _guarded((B, S, C, 2))
    dbuf, du = _guarded((B, L, C), dt)
    dev.inorm_gelu_backward(gy[1], u[1], stat[1], part, du, B, L, C, S)
    torch.cuda.synchronize()
    for buf, name in ((dbuf, "du"), (pbuf, "part"), (stat[0], "stat"), (gy[0], "gy"), (u[0], "u")):
        _guards_intact(buf, "%s %s" % (c.text, name))
    assert torch.equal(stat[1].cpu(), stat_in), "stat was written"
    return {"du": du.cpu()}


@pytest.mark.parametrize("c", INORM, ids=[c.id for c in INORM])
def test_inorm_gelu(dev, c):
    inp = IR.inputs(c)
    got = _twice(c.text, lambda: run_inorm_forward(dev, c, inp))
    fed = torch.stack([got["mean"], got["rstd"]], dim=-1) if c.chained else IR.stat_fed(c, inp)
    got.update(_twice(c.text, lambda: run_inorm_backward(dev, c, inp, fed)))
    for name, worst in IR.check(c, got, inp).items():
        WORST[IR.key_of(c, name)] = max(WORST[IR.key_of(c, name)], worst)
        print("%s %s: worst ratio %.3f" % (c.text, name, worst))


@pytest.mark.parametrize("args", IR.rejected(), ids=["f32-C=6", "f32-C=12", "S=4097", "bf16-C=12", "dtype"])
def test_inorm_gelu_return_codes(dev, args):
    dt, C, S, rc = args
    B, L = 2, 10
    tdt = torch.bfloat16 if dt == "bf16" else torch.float32
    code = {"f32": hip.F32, "bf16": hip.BF16}.get(dt, 7)
    t = torch.ones(B, L, C, dtype=tdt, device="cuda")
    ybuf, y = _guarded((B, L, C), tdt)
    part = torch.full((B, S, C, 2), float("nan"), device="cuda")
    stat = torch.full((B, C, 2), float("nan"), device="cuda")
    p = hip._ptr
    assert dev.lib.gwd_inorm_gelu_forward(p(t), p(t), p(y), p(part), p(stat), B, L, C, S, IR.EPS, code, dev._stream(t)) == rc
    assert dev.lib.gwd_inorm_gelu_backward(p(t), p(t), p(stat), p(part), p(y), B, L, C, S, code, dev._stream(t)) == rc
    torch.cuda.synchronize()
    assert bool(torch.isnan(ybuf).all()) and bool(torch.isnan(part).all()) and bool(torch.isnan(stat).all())


# ============================================================================================================== report
def test_worst_ratios_are_reported(dev):
    """Prints the worst ratio per (operation, output, type) of the cases above."""
    consts = dict(IR.C)
    consts.update(TR.C)
    consts[("certain_sample", "coords", "f32")] = SR.C
    assert len(WORST) == len(consts) or len(WORST) == 0       # (0: this test was selected on its own)
    for key, w in sorted(WORST.items()):
        print("forward witnesses: %-14s %-6s %-4s worst ratio %.3f of C = %.1f" % (key + (w, consts[key])))
        assert w <= consts[key]
