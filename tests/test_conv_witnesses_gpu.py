"""GPU: every kernel the convolution dispatcher can launch, run once through the C ABI at its witness call
(tests/golden/conv_witnesses.txt) and compared ELEMENT by element with the fp64 reference of tests/conv_ref.py: bound
c u (|ref| + cond), c from the CPU rounding model (never from a kernel's output), exact zeros where the bound is zero.

tests/test_conv_witnesses.py proves on the CPU that each call reaches the kernel its line names - for a device with the 256 compute
units the recorder stubs.  On another CU count a few weight-gradient calls may split differently or take a neighbouring kernel; every
case is a valid numeric check all the same, so the count is printed and nothing is skipped.  Run the file with -x: a fault is a finding."""
import pytest
import torch

from gw_depth_amd import hip
from tests import conv_ref as R
from tests import conv_witness as W

pytestmark = pytest.mark.gpu
TABLE = W.load()
IDS = [W.short_name(k) for k, _ in TABLE]
assert len(set(IDS)) == len(IDS)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    hip.set_library(None)
    torch.set_num_threads(16)
    print("compute units: %d (the witness table is generated for 256)" % torch.cuda.get_device_properties(0).multi_processor_count)
    return hip.library()


def _common_kw(c, inp):
    kw = dict(stride=c.stride, pad=c.pad, gather=c.gather, virt=(c.Hv, c.Wv), zero_page=bool(c.zero_page))
    if inp.scale is not None:
        kw["scale"] = inp.scale.cuda()
    return kw


def _dims(c):
    return (c.B, c.Hi, c.Wi, c.Cin, c.Ho, c.Wo, c.Cout, c.k, c.k)


def _nan(*shape, dtype):
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda")


def _forward(dev, c):
    inp, e, M = R.Inputs(c), R.epilogue(c), R.rows_of(c)
    dt = inp.dtype
    x, w = inp.full("x", c.B * c.Hi * c.Wi, "cuda"), inp.w.cuda()
    out = dict(y=_nan(M, c.Cout, dtype=dt))
    kw = _common_kw(c, inp)
    kw["act"], kw["act_scale"] = e.act, e.act_scale
    if e.shift:
        kw["shift"] = inp.shift.cuda()
    for name in ("residual", "mult"):
        if getattr(inp, name) is not None:
            kw[name] = inp.full(name, M, "cuda")
    if e.gate is not None:
        kw["gate"], kw["gate_act"] = inp.full("gate", M, "cuda"), e.gate
    if e.z:
        kw["z"] = out["z"] = _nan(M, c.Cout, dtype=dt)
    if e.ln:
        out["ln_mean"], out["ln_rstd"] = _nan(M, dtype=torch.float32), _nan(M, dtype=torch.float32)
        kw["ln"] = (out["ln_mean"], out["ln_rstd"], c.ln_C)
    assert dev.conv_forward(x, w, out["y"], _dims(c), **kw) is not False, "the library declined the call"
    torch.cuda.synchronize()
    rows, skipped = R.compare_rows(c)
    assert skipped == 0
    ref, cond = R.conv_ref_cond(c, inp, rows)
    assert set(ref) == set(out)
    for name in sorted(out):
        assert bool(torch.isfinite(out[name]).all()), "%s: not finite (an element was never written?)" % name
        worst = R.assert_elementwise(out[name][rows.cuda()].cpu(), ref[name], cond[name], R.C[(R.operation(c), name, R.dtype_name(c))],
                                     ("row", "channel")[:ref[name].dim()], u=R.out_unit(c, name), what="%s %s" % (c.text, name))
        print("%s %s: %d of %d rows, worst ratio %.3f" % (c.text, name, len(rows), M, worst))


def _wgrad(dev, c):
    jobs, keep = [], []
    for i in range(c.n):
        j = W.with_batch(c, i)
        inp = R.Inputs(j, seed=i)
        x, gy = inp.full("x", j.B * j.Hi * j.Wi, "cuda"), inp.full("gy", R.rows_of(j), "cuda")
        dw = torch.zeros(c.Cout, c.k * c.k, c.Cin, device="cuda")
        jobs.append((x, gy, dw, _dims(j), _common_kw(j, inp)))
        keep.append((j, inp, dw))
    if c.call == "W":
        x, gy, dw, dims, kw = jobs[0]
        dev.conv_wgrad(x, gy, dw, dims, **kw)
    else:
        dev.conv_wgrad_batch(jobs)
    torch.cuda.synchronize()
    for j, inp, dw in keep:
        assert bool(torch.isfinite(dw).all())
        blocks = R.wgrad_blocks(j)
        ref, cond = R.wgrad_ref_cond(j, inp, blocks)
        dw = dw.cpu()
        for (n0, n1, c0, c1), r, cd in zip(blocks, ref, cond):
            worst = R.assert_elementwise(dw[n0:n1, :, c0:c1], r, cd, R.C[("wgrad", "dw", R.dtype_name(c))], ("n", "tap", "c"), u=R.U_F32,
                                         what="%s B=%d block n %d c %d" % (c.text, j.B, n0, c0))
            print("%s B=%d dw[%d:%d, :, %d:%d]: worst ratio %.3f" % (c.text, j.B, n0, n1, c0, c1, worst))


@pytest.mark.parametrize("kernel,c", TABLE, ids=IDS)
def test_witness(dev, kernel, c):
    (_forward if c.call == "F" else _wgrad)(dev, c)
