"""GPU: every kernel the twelve row entry points of csrc/rowops.hip and csrc/inorm.hip can launch, run once through the hip.py wrappers
at its witness call (tests/golden/row_witnesses.txt) and compared ELEMENT by element, every element of every output, with the fp64
reference of tests/row_ref.py: bound c u (|ref| + cond), c from the CPU rounding model (never from a kernel's output), exact zeros
where the bound is zero.  Every output is NaN before the call (statistics, scratch and padding columns included), the ACCUMULATED ones
(colsum's out, dbias) hold row_ref.pattern, dgamma / dbeta are zeroed as ops.py zeroes them.

tests/test_row_witnesses.py proves on the CPU that each call reaches the kernel its line names.  Run the file with -x: a fault is a finding."""
import collections

import pytest
import torch

from gw_depth_amd import hip
from tests import row_ref as R
from tests import row_witness as W

pytestmark = pytest.mark.gpu
TABLE = W.load()
IDS = [W.short_name(k) for k, _ in TABLE]
assert len(set(IDS)) == len(IDS)
WORST = collections.defaultdict(float)            # (family, operation, output, type) -> worst ratio over the file


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    hip.set_library(None)
    torch.set_num_threads(16)
    return hip.library()


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda")


def run(dev, c, inp):
    """The call on the device -> its outputs (device tensors)."""
    d = {k: v.cuda() for k, v in inp.items()}
    dt = R.torch_dtype(c)
    out = {}
    if c.call == "LF":
        out.update(y=_nan(c.rows, c.pitch, dtype=dt), mean=_nan(c.rows), rstd=_nan(c.rows))
        dev.layernorm_forward(d["x"], d.get("gamma"), d.get("beta"), out["y"], out["mean"], out["rstd"], c.rows, c.C, c.gelu, residual=d.get("residual"), ld=c.ld)
    elif c.call == "LB":
        out["gx"] = _nan(c.rows, c.pitch, dtype=dt)
        if c.dgamma:
            out.update(dgamma=torch.zeros(c.C, device="cuda"), dbeta=torch.zeros(c.C, device="cuda"))
        done = dev.layernorm_backward(d["gy"], d["x"], d.get("gamma"), d.get("beta"), d["mean"], d["rstd"], out["gx"], out.get("dgamma"), out.get("dbeta"),
                                      c.rows, c.C, c.gelu, ld=c.ld, gskip=d.get("gskip"), elu_input=bool(c.elu))
        assert done is True, "the library declined gskip / the ELU input"
    elif c.call in ("SF", "SM"):
        out["y"] = _nan(c.rows, c.L, dtype=dt)
        if c.call == "SF":
            dev.softmax_forward(d["x"], out["y"], c.rows, c.L)
        else:
            dev.softmax_masked_forward(d["x"], d.get("mask"), out["y"], c.rows, c.L, c.rpm if c.mask else 1, c.scale)
    elif c.call in ("SB", "SS"):
        out["gx"] = _nan(c.rows, c.L, dtype=dt)
        if c.call == "SB":
            dev.softmax_backward(d["gy"], d["y"], out["gx"], c.rows, c.L)
        else:
            dev.softmax_scaled_backward(d["gy"], d["y"], out["gx"], c.rows, c.L, c.scale)
    elif c.call == "AB":
        out["gx"] = _nan(c.rows, c.C, dtype=dt)
        dev.act_backward(d["gy"], d.get("ref"), out["gx"], d.get("scale"), c.rows, c.C, c.act, c.act_scale)
    elif c.call == "AC":
        out.update(gx=_nan(c.rows, c.C, dtype=dt), dbias=R.pattern(c.C).cuda())
        assert dev.act_backward_colsum(d["gy"], d.get("ref"), out["gx"], out["dbias"], c.rows, c.C, c.act, c.act_scale, mult=d.get("mult")) is True
    elif c.call == "CS":
        out["out"] = R.pattern(c.C).cuda()
        dev.colsum(d["g"], out["out"], c.rows, c.C)
    elif c.call == "CB":
        for i, (rows, C) in enumerate(c.jobs):
            out["out%d" % i] = R.pattern(C).cuda()
        dev.colsum_batch([(d["g%d" % i], out["out%d" % i], rows, C) for i, (rows, C) in enumerate(c.jobs)])
    elif c.call == "IF":
        out.update(y=_nan(c.B, c.L, c.C, dtype=dt), stat=_nan(c.B, c.C, 2), part=_nan(c.B, c.S, c.C, 2))
        dev.inorm_gelu_forward(d["a"], d["u"], out["y"], out["part"], out["stat"], c.B, c.L, c.C, c.S, R.LN_EPS)
    else:
        out.update(du=_nan(c.B, c.L, c.C, dtype=dt), part=_nan(c.B, c.S, c.C, 2))
        dev.inorm_gelu_backward(d["gy"], d["u"], d["stat"], out["part"], out["du"], c.B, c.L, c.C, c.S)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("kernel,c", TABLE, ids=IDS)
def test_witness(dev, kernel, c):
    for f in R.forms(c):
        inp = R.inputs(f)
        got = {k: v.cpu() for k, v in run(dev, f, inp).items()}
        for name, v in got.items():
            assert bool(torch.isfinite(v).all()), "%s %s: not finite (an element was never written?)" % (f.text, name)
        for name, worst in R.check(f, got, inp).items():
            key = (f.family, R.OPERATION[f.call], name.rstrip("0123456789"), R.dtype_name(f))
            WORST[key] = max(WORST[key], worst)
            print("%s %s: worst ratio %.3f" % (f.text, name, worst))


def test_worst_ratios_are_reported(dev):
    """Prints the worst ratio per family and per (operation, output, type) of the cases above (DESIGN.md section 11 holds a copy)."""
    assert len(WORST) == len(R.C) or len(WORST) == 0          # (0: this test was selected on its own)
    fam = collections.defaultdict(float)
    for (family, op, name, dt), w in sorted(WORST.items()):
        fam[family] = max(fam[family], w / R.C[(op, name, dt)])
        print("row witnesses: %-14s %-6s %-4s worst ratio %.3f of C = %.1f" % (op, name, dt, w, R.C[(op, name, dt)]))
    for family, share in sorted(fam.items()):
        print("row witnesses: family %-10s worst ratio / C = %.2f" % (family, share))


# ------------------------------------------------------------------------------------ the -4 returns of include/gwdepth.h
def _ln_backward_raw(dev, c, inp, out, flags, gskip):
    p = hip._ptr
    d = {k: v.cuda() for k, v in inp.items()}
    rc = dev.lib.gwd_layernorm_backward(p(d["gy"]), p(d["x"]), p(d.get("gamma")), p(d.get("beta")), p(d["mean"]), p(d["rstd"]), p(out["gx"]), p(out["dgamma"]),
                                        p(out["dbeta"]), c.rows, c.C, c.ld, flags, p(gskip), hip.dtype_code(d["x"]), dev._stream(d["gy"], d["x"], out["gx"]))
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("call", ["LB 1 37 30 0 1 0 1 0 1", "LB 0 37 258 0 1 0 0 1 1", "LB 1 37 161 0 0 1 1 1 1"])
def test_gskip_and_elu_input_without_a_vector_kernel_return_minus_4(dev, call):
    c = W.parse_call(call)
    inp = R.inputs(c)
    out = dict(gx=_nan(c.rows, c.pitch, dtype=R.torch_dtype(c)), dgamma=torch.zeros(c.C, device="cuda"), dbeta=torch.zeros(c.C, device="cuda"))
    gskip = inp["gskip"].cuda() if c.gskip else None
    assert _ln_backward_raw(dev, c, inp, out, c.gelu | (2 if c.elu else 0), gskip) == -4
    assert bool(torch.isnan(out["gx"]).all()) and not out["dgamma"].any() and not out["dbeta"].any()      # nothing was written


@pytest.mark.parametrize("dtype,C,ld", [(W.BF16, 30, 36), (W.F32, 30, 34), (W.BF16, 60, 68)])
def test_a_pitch_that_is_no_multiple_of_16_bytes_returns_minus_4(dev, dtype, C, ld):
    c = W.parse_call("LF %d 37 %d %d 1 0 0" % (dtype, C, ld))
    inp = R.inputs(c)
    dt = R.torch_dtype(c)
    y, mean, rstd = _nan(c.rows, ld, dtype=dt), _nan(c.rows), _nan(c.rows)
    with pytest.raises(RuntimeError, match="status -4"):
        dev.layernorm_forward(inp["x"].cuda(), inp["gamma"].cuda(), inp["beta"].cuda(), y, mean, rstd, c.rows, C, 0, ld=ld)
    torch.cuda.synchronize()
    assert bool(torch.isnan(y).all()) and bool(torch.isnan(mean).all()) and bool(torch.isnan(rstd).all())
    b = W.parse_call("LB %d 37 %d %d 1 0 0 0 1" % (dtype, C, ld))
    binp = R.inputs(b)
    out = dict(gx=_nan(b.rows, ld, dtype=dt), dgamma=torch.zeros(C, device="cuda"), dbeta=torch.zeros(C, device="cuda"))
    assert _ln_backward_raw(dev, b, binp, out, 0, None) == -4
    assert bool(torch.isnan(out["gx"]).all()) and not out["dgamma"].any() and not out["dbeta"].any()


@pytest.mark.parametrize("dtype", [W.BF16, W.F32])
def test_colsum_batch_with_a_non_vector_job_returns_minus_4(dev, dtype):
    dt = torch.bfloat16 if dtype == W.BF16 else torch.float32
    jobs = [(torch.ones(37, C, dtype=dt, device="cuda"), R.pattern(C).cuda(), 37, C) for C in (64, 7, 96)]
    with pytest.raises(RuntimeError, match="status -4"):
        dev.colsum_batch(jobs)
    torch.cuda.synchronize()
    for _, out, _, C in jobs:
        assert torch.equal(out.cpu(), R.pattern(C))
