"""GPU: the fifteen entry points of csrc/resample.hip and csrc/pointsample.hip, run through the hip.py wrappers over the case table of
tests/spatial_ref.py and compared ELEMENT by element, every element of every output, with its fp64 reference: bound C u (|ref| + cond), C from
the CPU rounding model (never from a kernel's output), exact zeros where the bound is zero, bit-exact copies where the operation is one.
Every output is NaN before the call (the fp32 scratch of the separable backward included); the ACCUMULATED ones (dw of the fold, gmap of
the scatter backward in its second sub-case) hold spatial_ref.pattern.  A pitched output lives in a wider map whose other columns must come
back bit-identical; a pitched input has NaN neighbours.  One test per (entry point, dtype) loops over that entry point's cases.

tests/test_spatial_ref.py proves on the CPU that the table covers the dispatch.  Run the file with -x: a fault is a finding."""
import collections

import pytest
import torch

from gw_depth_amd import hip
from tests import spatial_ref as R

pytestmark = pytest.mark.gpu
GROUPS = sorted({(c.op, c.dtype) for c in R.cases()})
WORST = collections.defaultdict(float)            # (operation, output, type) -> worst ratio over the file


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    hip.set_library(None)
    torch.set_num_threads(16)
    return hip.library()


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda")


def _in_wide(t, ld, off):
    """t (B,H,W,C) on the device as the channel slice [off, off + C) of a (B,H,W,ld) map whose other columns hold NaN."""
    wide = _nan(*t.shape[:3], ld, dtype=t.dtype)
    wide[..., off:off + t.shape[3]] = t
    return wide[..., off:off + t.shape[3]]


def run(dev, c, inp):
    """The case on the device -> its outputs (device tensors)."""
    d = {k: v.cuda() for k, v in inp.items()}
    dt = R.torch_dtype(c)
    op = c.op
    if op == "resample_fwd":
        if c.ld:
            wide = R.pattern(c.B, c.Ho, c.Wo, c.ld).to(dt).cuda()
            before = wide.clone()
            wide[..., c.off:c.off + c.C] = float("nan")
            y = wide[..., c.off:c.off + c.C]
        else:
            y = _nan(c.B, c.Ho, c.Wo, c.C, dtype=dt)
        dev.resample_forward(d["x"], y, c.B, c.Hs, c.Ws, c.Ho, c.Wo, c.C, c.mode)
        if c.ld:
            torch.cuda.synchronize()
            keep = torch.ones(c.ld, dtype=torch.bool, device="cuda")
            keep[c.off:c.off + c.C] = False
            assert torch.equal(wide[..., keep].view(torch.int16 if dt == torch.bfloat16 else torch.int32),
                               before[..., keep].view(torch.int16 if dt == torch.bfloat16 else torch.int32)), "%s: a neighbouring slice was written" % c.text
        out = {"y": y}
    elif op == "resample_bwd":
        out = {"gx": _nan(c.B, c.Hs, c.Ws, c.C, dtype=dt)}
        assert dev.resample_backward(d["gy"], out["gx"], c.B, c.Hs, c.Ws, c.Ho, c.Wo, c.C, c.mode, gate=d.get("gate"), gate_act=c.gate) is True
    elif op == "resample_bwd_sep":
        out = {"gx": _nan(c.B, c.Hs, c.Ws, c.C, dtype=dt)}
        tmp = _nan(c.B * c.Ho * c.Ws * c.C)
        gy = _in_wide(d["gy"], c.ld, c.off) if c.ld else d["gy"]
        assert dev.resample_backward_sep(gy, tmp, out["gx"], c.B, c.Hs, c.Ws, c.Ho, c.Wo, c.C, c.mode) is True
    elif op == "avgpool_fwd":
        out = {"y": _nan(c.B, c.H // c.k, c.W // c.k, c.C, dtype=dt)}
        dev.avgpool_forward(d["x"], out["y"], c.B, c.H, c.W, c.C, c.k)
    elif op == "avgpool_bwd":
        out = {"gx": _nan(c.B, c.H, c.W, c.C, dtype=dt)}
        dev.avgpool_backward(d["gy"], out["gx"], c.B, c.H, c.W, c.C, c.k)
    elif op == "psp_fwd":
        out = {"p%d" % k: _nan(c.B, c.H // k, c.W // k, c.C, dtype=dt) for k in (16, 8, 4, 2)}
        assert dev.psp_pool_forward(d["x"], out["p16"], out["p8"], out["p4"], out["p2"]) is True
    elif op == "psp_bwd":
        out = {"gx": _nan(c.B, c.H, c.W, c.C, dtype=dt)}
        gpass = _in_wide(d["gpass"], 3 * c.C, c.C) if c.gpass == 2 else d.get("gpass")
        dev.psp_pool_backward(gpass, d.get("g16"), d.get("g8"), d.get("g4"), d.get("g2"), out["gx"])
    elif op == "stride_place":
        out = {"dst": _nan(c.B, c.H, c.W, c.C, dtype=dt)}
        assert dev.stride_place(d["src"], d.get("residual"), out["dst"], c.s) is True
    elif op == "taps_collapse":
        out = {"wk": _nan(c.Cin, 4, 4, c.Cout, dtype=dt)}
        dev.upsample_taps_collapse(d["w"], out["wk"])
    elif op == "taps_fold":
        out = {"dw": R.pattern(c.Cout, 3, 3, c.Cin).cuda()}
        dev.upsample_taps_fold(d["D"], out["dw"])
    elif op == "point_fwd":
        out = {"out": _nan(c.B, c.S, c.C)}
        dev.point_sample_forward(d["map"], d["coords"], out["out"], c.B, c.H, c.W, c.C, c.S, c.mode)
    elif op == "point_framed_fwd":
        out = {"out": _nan(c.B, c.S, c.C)}
        dev.point_sample_framed_forward(d["map"], d["coords"], out["out"], c.B, c.H, c.W, c.C, c.S, (c.Hf, c.Wf, c.shift))
    elif op == "point_framed_bwd":
        out = {"gmap": _nan(c.B, c.H, c.W, c.C, dtype=dt)}
        dev.point_sample_framed_backward(d["gout"], d["coords"], out["gmap"], c.B, c.H, c.W, c.C, c.S, (c.Hf, c.Wf, c.shift))
    elif op == "point_bwd_gather":
        n = c.B * c.H * c.W * c.C
        if c.view:                                               # one element into a larger buffer: not 16-byte aligned, the scalar kernel
            buf = R.pattern(n + 16).to(dt).cuda()
            buf[1:1 + n] = float("nan")
            gmap = buf[1:1 + n].view(c.B, c.H, c.W, c.C)
            assert gmap.data_ptr() % 16 != 0
        else:
            gmap = _nan(c.B, c.H, c.W, c.C, dtype=dt)
        assert dev.point_sample_backward_gather(d["gout"], d["coords"], gmap, c.B, c.H, c.W, c.C, c.S, c.mode) is True
        if c.view:
            torch.cuda.synchronize()
            want = R.pattern(n + 16).to(dt).cuda()
            assert torch.equal(buf[:1], want[:1]) and torch.equal(buf[1 + n:], want[1 + n:]), "%s: written outside gmap" % c.text
        out = {"gmap": gmap}
    else:
        out = {"gmap": (R.pattern(c.B, c.H, c.W, c.C) if c.pat else torch.zeros(c.B, c.H, c.W, c.C)).to(dt).cuda()}
        dev.point_sample_backward(d["gout"], d["coords"], out["gmap"], c.B, c.H, c.W, c.C, c.S, c.mode)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("op,dtype", GROUPS, ids=["%s-%s" % g for g in GROUPS])
def test_entry_point(dev, op, dtype):
    for c in [c for c in R.cases() if (c.op, c.dtype) == (op, dtype)]:
        inp = R.inputs(c)
        got = {k: v.cpu() for k, v in run(dev, c, inp).items()}
        for name, v in got.items():
            if not bool(torch.isfinite(v).all()):
                first = int(torch.nonzero(~torch.isfinite(v).reshape(-1))[0])
                raise AssertionError("%s %s: not finite from flat index %d of %d on (an element was never written?)" % (c.text, name, first, v.numel()))
        for name, worst in R.check(c, got, inp).items():
            WORST[R.key_of(c, name)] = max(WORST[R.key_of(c, name)], worst)
            print("%s %s: worst ratio %.3f" % (c.text, name, worst))


def test_worst_ratios_are_reported(dev):
    """Prints the worst ratio per (operation, output, type) of the cases above (DESIGN.md section 24 holds a copy)."""
    assert len(WORST) == len(R.C) or len(WORST) == 0          # (0: this test was selected on its own)
    for (op, name, dt), w in sorted(WORST.items()):
        print("spatial edges: %-25s %-6s %-4s worst ratio %.3f of C = %.1f" % (op, name, dt, w, R.C[(op, name, dt)]))


# ------------------------------------------------------------------------ return codes: every one of these paths returns before a launch
P = hip._ptr
PP = hip._ptr_pitched
BF, F32 = torch.bfloat16, torch.float32


def _code(t):
    return hip.dtype_code(t)


def _untouched(*ts):
    torch.cuda.synchronize()
    return all(bool(torch.isnan(t).all()) for t in ts)


def _resample_forward_raw(dev, x, y, B, Hs, Ws, Ho, Wo, C, mode, ldy):
    return dev.lib.gwd_resample_forward(P(x), PP(y), B, Hs, Ws, Ho, Wo, C, mode, ldy, _code(x), dev._stream(x, y))


@pytest.mark.parametrize("dtype,C,ld,off,mode,code", [
    (BF, 8, 4, 0, 0, -1), (F32, 4, 3, 0, 0, -1),          # 0 < ldy < C
    (BF, 3, 6, 0, 0, -4), (F32, 6, 8, 0, 1, -4),          # a pitch without a vector kernel
    (BF, 8, 12, 0, 0, -4),                                # 16-byte vectors at an 8-byte pitch
    (BF, 8, 0, 0, 2, -1), (F32, 3, 0, 0, 2, -1),          # no such mode
    (BF, 8, 24, 4, 0, -4), (BF, 4, 12, 2, 1, -4), (F32, 4, 8, 2, 0, -4),      # a slice that starts inside a vector
])
def test_resample_forward_return_codes(dev, dtype, C, ld, off, mode, code):
    x = torch.randn(2, 3, 5, C, device="cuda").to(dtype)
    wide = _nan(2, 7, 9, max(ld, C + off), dtype=dtype)
    assert _resample_forward_raw(dev, x, wide[..., off:off + C], 2, 3, 5, 7, 9, C, mode, ld) == code
    assert _untouched(wide)


@pytest.mark.parametrize("dtype", [BF, F32])
def test_resample_backward_gate_return_codes(dev, dtype):
    c = next(c for c in R.cases() if c.op == "resample_bwd" and R.torch_dtype(c) == dtype and c.C == 8 and c.mode == R.BILINEAR and (c.Hs, c.Ho) == (3, 7))
    inp = R.inputs(c)
    gy = inp["gy"].cuda()
    gate = R._gate_values(torch.Generator().manual_seed(1), (c.B, c.Hs, c.Ws, c.C), dtype).cuda()
    gx = _nan(c.B, c.Hs, c.Ws, c.C, dtype=dtype)
    raw = lambda mode, act: dev.lib.gwd_resample_backward(P(gy), P(gx), c.B, c.Hs, c.Ws, c.Ho, c.Wo, c.C, mode, P(gate), act, _code(gy), dev._stream(gy, gx))
    assert raw(R.BILINEAR, hip.ACT_RELU) == -4 and _untouched(gx)           # the gate needs the vector kernels of the nearest mode
    assert raw(R.NEAREST, hip.ACT_GELU) == -1 and _untouched(gx)
    assert raw(R.NEAREST, hip.ACT_SIGMOID) == -1 and _untouched(gx)
    gy3, gate3, gx3 = gy[..., :3].contiguous(), gate[..., :3].contiguous(), _nan(c.B, c.Hs, c.Ws, 3, dtype=dtype)
    assert dev.lib.gwd_resample_backward(P(gy3), P(gx3), c.B, c.Hs, c.Ws, c.Ho, c.Wo, 3, R.NEAREST, P(gate3), hip.ACT_RELU, _code(gy), dev._stream(gy3, gx3)) == -4
    assert _untouched(gx3)
    # the wrapper then runs WITHOUT the gate and says so: the un-gated result must pass the un-gated bound
    assert dev.resample_backward(gy, gx, c.B, c.Hs, c.Ws, c.Ho, c.Wo, c.C, R.BILINEAR, gate=gate, gate_act=hip.ACT_RELU) is False
    torch.cuda.synchronize()
    R.check(c, {"gx": gx.cpu()}, inp)


@pytest.mark.parametrize("dtype,C,ld,off", [(BF, 3, 0, 0), (F32, 6, 0, 0), (BF, 8, 12, 0), (BF, 8, 24, 4), (BF, 4, 12, 2), (F32, 4, 8, 2)])
def test_resample_backward_sep_return_codes(dev, dtype, C, ld, off):
    """-4: no vector kernel for C, a pitch that breaks the vectors, a slice that starts inside one."""
    wide = torch.randn(2, 7, 9, max(ld, C + off), device="cuda").to(dtype)
    gy = wide[..., off:off + C]
    tmp, gx = _nan(2 * 7 * 5 * C), _nan(2, 3, 5, C, dtype=dtype)
    assert dev.lib.gwd_resample_backward_sep(PP(gy), P(tmp), P(gx), 2, 3, 5, 7, 9, C, 0, ld, _code(gx), dev._stream(gy, gx)) == -4
    assert _untouched(tmp, gx)
    if ld == 0:
        assert dev.resample_backward_sep(gy.contiguous(), tmp, gx, 2, 3, 5, 7, 9, C, 0) is False and _untouched(tmp, gx)


@pytest.mark.parametrize("dtype", [BF, F32])
def test_psp_pool_return_codes(dev, dtype):
    vec = 8 if dtype == BF else 4
    for (H, W, C, code) in ((15, 16, vec, -1), (16, 15, vec, -1), (16, 16, vec + 4 if dtype == BF else 6, -4), (17, 31, 3, -4)):
        x = torch.randn(1, H, W, C, device="cuda").to(dtype)
        p = [_nan(1, max(H // k, 1), max(W // k, 1), C, dtype=dtype) for k in (16, 8, 4, 2)]
        assert dev.lib.gwd_psp_pool_forward(P(x), *[P(t) for t in p], 1, H, W, C, _code(x), dev._stream(x)) == code
        gx = _nan(1, H, W, C, dtype=dtype)
        g = [torch.randn_like(t) for t in p]
        assert dev.lib.gwd_psp_pool_backward(None, *[P(t) for t in g], P(gx), 1, H, W, C, 0, _code(gx), dev._stream(gx)) == code
        assert _untouched(gx, *p)
    # a pitch that is no multiple of the vector, a pitch below C, a g_pass that starts inside a vector
    C = 2 * vec
    g = [torch.randn(1, 16 // k, 16 // k, C, device="cuda").to(dtype) for k in (16, 8, 4, 2)]
    gx = _nan(1, 16, 16, C, dtype=dtype)
    wide = torch.randn(1, 16, 16, 3 * C + vec // 2, device="cuda").to(dtype)
    for (off, ld) in ((0, C + vec // 2), (0, vec), (vec // 2, 3 * C)):
        gp = wide[..., off:off + C]
        assert dev.lib.gwd_psp_pool_backward(PP(gp), *[P(t) for t in g], P(gx), 1, 16, 16, C, ld, _code(gx), dev._stream(gx)) == -4
        assert _untouched(gx)


@pytest.mark.parametrize("dtype,C", [(BF, 4), (BF, 12), (F32, 6), (F32, 1)])
def test_stride_place_without_a_vector_kernel_returns_minus_4(dev, dtype, C):
    src, res, dst = torch.randn(1, 4, 4, C, device="cuda").to(dtype), torch.randn(1, 8, 8, C, device="cuda").to(dtype), _nan(1, 8, 8, C, dtype=dtype)
    assert dev.stride_place(src, res, dst, 2) is False and _untouched(dst)
    assert dev.stride_place(src, None, dst, 2) is False and _untouched(dst)


@pytest.mark.parametrize("dtype", [BF, F32])
def test_gather_backward_declines_what_its_grid_cannot_hold(dev, dtype):
    C = 8 if dtype == BF else 4
    for (B, H, W, C_, S) in ((1, 5, 7, C, 257), (65536, 1, 1, 1, 1)):
        gout, coords = torch.randn(B, S, C_, device="cuda"), torch.zeros(B, S, 2, device="cuda")
        gmap = _nan(B, H, W, C_, dtype=dtype)
        assert dev.point_sample_backward_gather(gout, coords, gmap, B, H, W, C_, S, 0) is False and _untouched(gmap)
        assert dev.lib.gwd_point_sample_backward_gather(P(gout), P(coords), P(gmap), B, H, W, C_, S, 1, _code(gmap), dev._stream(gout, gmap)) == -4
        assert _untouched(gmap)


@pytest.mark.parametrize("dtype", [BF, F32])
@pytest.mark.parametrize("Hf,Wf,shift", [(14, 21, 3), (21, 19, 3), (21, 21, 21), (21, 22, 21), (21, 21, -1)])
def test_framed_entry_points_reject_a_bad_frame(dev, dtype, Hf, Wf, shift):
    B, H, W, C, S = 1, 15, 20, 8, 5
    fmap, coords, gout = torch.randn(B, H, W, C, device="cuda").to(dtype), torch.zeros(B, S, 2, device="cuda"), torch.randn(B, S, C, device="cuda")
    out, gmap = _nan(B, S, C), _nan(B, H, W, C, dtype=dtype)
    st = dev._stream(fmap, out)
    assert dev.lib.gwd_point_sample_framed_forward(P(fmap), P(coords), P(out), B, H, W, C, S, Hf, Wf, shift, _code(fmap), st) == -1
    assert dev.lib.gwd_point_sample_framed_backward(P(gout), P(coords), P(gmap), B, H, W, C, S, Hf, Wf, shift, _code(gmap), st) == -1
    assert _untouched(out, gmap)
