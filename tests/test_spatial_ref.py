"""CPU: tests/spatial_ref.py against itself and against torch.  The references equal float64 torch (F.interpolate, F.avg_pool2d,
F.grid_sample and their autograd; the legacy-nearest index rule against fp32 torch, where the values are copies), an honest fp32
implementation (tests/fake_device.py) fits the bound, every injected defect of the model is caught on a named case, the table covers
every combination the dispatch of csrc/resample.hip and csrc/pointsample.hip distinguishes, and MEASURED is fresh."""
import itertools
import re

import pytest
import torch
import torch.nn.functional as F

from tests import spatial_ref as R
from tests.fake_device import FakeDevice

NCHW = lambda t: t.permute(0, 3, 1, 2)
NHWC = lambda t: t.permute(0, 2, 3, 1)


def pick(op, dtype, **attrs):
    return next(c for c in R.cases() if c.op == op and c.dtype == dtype and all(getattr(c, k, None) == v for k, v in attrs.items()))


def _close(a, b, what, tol=1e-12):
    scale = max(1.0, float(b.abs().max())) if b.numel() else 1.0
    assert tuple(a.shape) == tuple(b.shape), what
    assert float((a - b).abs().max()) <= tol * scale if b.numel() else True, (what, float((a - b).abs().max()))


def _interp(x, c):
    if c.mode == R.NEAREST:
        return F.interpolate(x, size=(c.Ho, c.Wo), mode="nearest")
    return F.interpolate(x, size=(c.Ho, c.Wo), mode="bilinear", align_corners=True)


def _grad(fn, x0, g):
    x0 = x0.clone().requires_grad_(True)
    with torch.enable_grad():
        (gx,) = torch.autograd.grad(fn(x0), x0, g)
    return gx


def _torch64(c, inp):
    """The outputs of the case from torch's own operators in float64 (float32 for the legacy-nearest index rule)."""
    d = {k: v.double() for k, v in inp.items()}
    op = c.op
    if op == "resample_fwd":
        if c.mode == R.NEAREST:
            return {"y": NHWC(_interp(NCHW(inp["x"].float()), c)).double()}
        return {"y": NHWC(_interp(NCHW(d["x"]), c))}
    if op in ("resample_bwd", "resample_bwd_sep"):
        wd = torch.float32 if c.mode == R.NEAREST else torch.float64
        gx = NHWC(_grad(lambda x: _interp(x, c), torch.zeros(c.B, c.C, c.Hs, c.Ws, dtype=wd), NCHW(inp["gy"].to(wd)))).double()
        if getattr(c, "gate", 0):
            gx = gx * R._gate_grad(d["gate"], c.gate)
        return {"gx": gx}
    if op == "avgpool_fwd":
        return {"y": NHWC(F.avg_pool2d(NCHW(d["x"]), c.k, c.k))}
    if op == "avgpool_bwd":
        return {"gx": NHWC(_grad(lambda x: F.avg_pool2d(x, c.k, c.k), torch.zeros(c.B, c.C, c.H, c.W, dtype=torch.float64), NCHW(d["gy"])))}
    if op == "psp_fwd":
        return {"p%d" % k: NHWC(F.avg_pool2d(NCHW(d["x"]), k, k)) for k in (16, 8, 4, 2)}
    if op == "psp_bwd":
        gx = d["gpass"].clone() if "gpass" in d else torch.zeros(c.B, c.H, c.W, c.C, dtype=torch.float64)
        for k in (16, 8, 4, 2):
            if "g%d" % k in d:
                gx += NHWC(_grad(lambda x: F.avg_pool2d(x, k, k), torch.zeros(c.B, c.C, c.H, c.W, dtype=torch.float64), NCHW(d["g%d" % k])))
        return {"gx": gx}
    if op == "stride_place":                                     # the data gradient of a 1x1 / stride s convolution with a unit weight
        x0 = torch.zeros(c.B, c.C, c.H, c.W, dtype=torch.float64)
        gx = NHWC(_grad(lambda x: x[:, :, ::c.s, ::c.s][:, :, :c.Ho, :c.Wo], x0, NCHW(d["src"])))
        return {"dst": gx + d["residual"] if "residual" in d else gx}
    H, W = (c.Hf, c.Wf) if "framed" in op else (c.H, c.W)
    mode = "nearest" if c.mode == R.NEAREST else "bilinear"
    grid = d["coords"].reshape(c.B, c.S, 1, 2)
    sample = lambda m: F.grid_sample(m, grid, mode=mode, align_corners=False, padding_mode="zeros")
    if op in ("point_fwd", "point_framed_fwd"):
        fmap = FakeDevice._framed(d["map"], (c.Hf, c.Wf, c.shift)) if "framed" in op else d["map"]
        return {"out": sample(NCHW(fmap)).reshape(c.B, c.C, c.S).permute(0, 2, 1)}
    g = NHWC(_grad(sample, torch.zeros(c.B, c.C, H, W, dtype=torch.float64), d["gout"].permute(0, 2, 1).reshape(c.B, c.C, c.S, 1)))
    if "framed" in op:
        g = R._frame_roll_back(g, c)
    if op == "point_bwd" and c.pat:
        g = g + R.pattern(c.B, c.H, c.W, c.C).double()
    return {"gmap": g}


@pytest.mark.parametrize("op", sorted({c.op for c in R.cases()} - {"taps_collapse", "taps_fold"}))
def test_reference_equals_torch_in_float64(op):
    for c in [c for c in R.cases() if c.op == op]:
        inp = R.inputs(c)
        ref, _ = R.reference(c, inp)
        want = _torch64(c, inp)
        assert set(ref) == set(want)
        for name in ref:
            if op == "resample_fwd" and c.mode == R.NEAREST:
                assert torch.equal(ref[name], want[name]), c.text            # copies: the index rule itself
            elif op.startswith("resample") and c.mode == R.NEAREST:
                _close(ref[name], want[name], c.text, tol=1e-5 * max(1, c.Ho // c.Hs + 1) * max(1, c.Wo // c.Ws + 1))      # torch summed in fp32
            else:
                _close(ref[name], want[name], "%s %s" % (c.text, name))


def test_tap_collapse_and_fold_equal_the_stand_in_on_integers():
    """Integer-valued weights are exact in fp32: the fp64 formulas of include/gwdepth.h must equal the stand-in's slices bit for bit."""
    g = torch.Generator().manual_seed(5)
    fake = FakeDevice()
    for (Cout, Cin) in ((1, 1), (3, 5), (64, 64)):
        w = torch.randint(-9, 10, (Cout, 3, 3, Cin), generator=g).float()
        wk = torch.empty(Cin, 4, 4, Cout)
        fake.upsample_taps_collapse(w, wk)
        assert torch.equal(R._collapse(w.double()), wk.double())
        D = torch.randint(-9, 10, (Cin, 4, 4, Cout), generator=g).float()
        dw = torch.zeros(Cout, 3, 3, Cin)
        fake.upsample_taps_fold(D, dw)
        assert torch.equal(R._fold(D.double()), dw.double())


def test_the_two_rounding_witnesses_of_legacy_nearest():
    assert int(R.nearest_index(14, 46)[23]) == 6 and 23 * 14 // 46 == 7
    assert int(R.nearest_index(26, 22)[11]) == 12 and 11 * 26 // 22 == 13
    for n_in, n_out, o in ((14, 46, 23), (26, 22, 11)):
        x = torch.arange(n_in, dtype=torch.float32).reshape(1, 1, n_in, 1)
        assert int(F.interpolate(x, size=(n_out, 1), mode="nearest")[0, 0, o, 0]) == int(R.nearest_index(n_in, n_out)[o])
        assert int(R.axis32(n_in, n_out, R.NEAREST).idx[o, 0]) == int(R.nearest_index(n_in, n_out)[o])
        assert int(R.axis32(n_in, n_out, R.NEAREST, "nearest_rational").idx[o, 0]) == o * n_in // n_out


# ------------------------------------------------------------------------------------------------- an honest fp32 implementation
def run_fake(c, inp):
    dev, dt = FakeDevice(), R.torch_dtype(c)
    nan = lambda *s, dtype=dt: torch.full(s, float("nan"), dtype=dtype)
    op = c.op
    if op == "resample_fwd":
        wide = nan(c.B, c.Ho, c.Wo, c.ld or c.C)
        y = wide[..., c.off:c.off + c.C]
        dev.resample_forward(inp["x"], y, c.B, c.Hs, c.Ws, c.Ho, c.Wo, c.C, c.mode)
        return {"y": y}
    if op == "resample_bwd":
        gx = nan(c.B, c.Hs, c.Ws, c.C)
        dev.resample_backward(inp["gy"], gx, c.B, c.Hs, c.Ws, c.Ho, c.Wo, c.C, c.mode, gate=inp.get("gate"), gate_act=c.gate)
        return {"gx": gx}
    if op == "resample_bwd_sep":
        gx = nan(c.B, c.Hs, c.Ws, c.C)
        dev.resample_backward_sep(inp["gy"], None, gx, c.B, c.Hs, c.Ws, c.Ho, c.Wo, c.C, c.mode)
        return {"gx": gx}
    if op == "avgpool_fwd":
        y = nan(c.B, c.H // c.k, c.W // c.k, c.C)
        dev.avgpool_forward(inp["x"], y, c.B, c.H, c.W, c.C, c.k)
        return {"y": y}
    if op == "avgpool_bwd":
        gx = nan(c.B, c.H, c.W, c.C)
        dev.avgpool_backward(inp["gy"], gx, c.B, c.H, c.W, c.C, c.k)
        return {"gx": gx}
    if op == "psp_fwd":
        out = {"p%d" % k: nan(c.B, c.H // k, c.W // k, c.C) for k in (16, 8, 4, 2)}
        dev.psp_pool_forward(inp["x"], out["p16"], out["p8"], out["p4"], out["p2"])
        return out
    if op == "psp_bwd":
        gx = nan(c.B, c.H, c.W, c.C)
        dev.psp_pool_backward(inp.get("gpass"), inp.get("g16"), inp.get("g8"), inp.get("g4"), inp.get("g2"), gx)
        return {"gx": gx}
    if op == "stride_place":
        dst = nan(c.B, c.H, c.W, c.C)
        dev.stride_place(inp["src"], inp.get("residual"), dst, c.s)
        return {"dst": dst}
    if op == "taps_collapse":
        wk = nan(c.Cin, 4, 4, c.Cout)
        dev.upsample_taps_collapse(inp["w"], wk)
        return {"wk": wk}
    if op == "taps_fold":
        dw = R.pattern(c.Cout, 3, 3, c.Cin)
        dev.upsample_taps_fold(inp["D"], dw)
        return {"dw": dw}
    args = (c.B, c.H, c.W, c.C, c.S)
    if op == "point_fwd":
        out = nan(c.B, c.S, c.C, dtype=torch.float32)
        dev.point_sample_forward(inp["map"], inp["coords"], out, *args, c.mode)
        return {"out": out}
    if op == "point_framed_fwd":
        out = nan(c.B, c.S, c.C, dtype=torch.float32)
        dev.point_sample_framed_forward(inp["map"], inp["coords"], out, *args, (c.Hf, c.Wf, c.shift))
        return {"out": out}
    gmap = nan(c.B, c.H, c.W, c.C)
    if op == "point_framed_bwd":
        dev.point_sample_framed_backward(inp["gout"], inp["coords"], gmap, *args, (c.Hf, c.Wf, c.shift))
    elif op == "point_bwd_gather":
        dev.point_sample_backward_gather(inp["gout"], inp["coords"], gmap, *args, c.mode)
    else:
        gmap = (R.pattern(c.B, c.H, c.W, c.C) if c.pat else torch.zeros(c.B, c.H, c.W, c.C)).to(R.torch_dtype(c))
        dev.point_sample_backward(inp["gout"], inp["coords"], gmap, *args, c.mode)
    return {"gmap": gmap}


@pytest.mark.parametrize("op", sorted({c.op for c in R.cases()}))
def test_the_stand_in_device_fits_the_bound(op):
    for c in [c for c in R.cases() if c.op == op]:
        inp = R.inputs(c)
        got = run_fake(c, inp)
        for v in got.values():
            assert bool(torch.isfinite(v).all()), c.text
        R.check(c, got, inp)


# --------------------------------------------------------------------------------------------------------- injected defects
G = dict(B=2, Hs=3, Ws=5, Ho=7, Wo=9)
DEFECT_CASES = {
    "last_row_clamp": (lambda: pick("resample_fwd", "bf16", C=8, mode=R.BILINEAR, ld=0, **G), r"row [45]\b|column 7\b"),
    "footprint_short": (lambda: pick("resample_bwd", "f32", C=4, mode=R.BILINEAR, gate=0, B=1, Hs=6, Ws=8, Ho=12, Wo=16), r"worst ratio"),
    "nearest_rational": (lambda: pick("resample_fwd", "bf16", C=8, mode=R.NEAREST, Hs=14, Ho=46), r"first at flat index %d\b" % (23 * 5 * 8)),
    "stride_tail": (lambda: pick("resample_fwd", "bf16", C=3, grid=1), r"first wrong flat index %d of" % R.FLAT_CAP),
    "pitch_as_c": (lambda: pick("resample_fwd", "bf16", C=8, ld=24, mode=R.BILINEAR, **G), r"first wrong flat index \d+"),
    "pool_remainder": (lambda: pick("avgpool_bwd", "bf16", C=8, H=17, W=19, k=8), r"reference 0\b"),
    "psp_partial_block": (lambda: pick("psp_fwd", "bf16", H=17, W=31), r"p16: .*image 1, row 0, column 0"),
    "stride_live_guard": (lambda: pick("stride_place", "bf16", C=8, H=9, s=3, res=0), r"first at flat index %d\b" % (6 * 8)),
    "tie_away": (lambda: pick("point_fwd", "bf16", C=8, H=16, S=37, mode=R.NEAREST), r"point \d+"),
    "border_weight": (lambda: pick("point_fwd", "f32", C=4, H=16, S=37, mode=R.BILINEAR), r"point \d+"),
    "collision_lost": (lambda: pick("point_bwd_gather", "f32", C=4, H=16, S=37, mode=R.BILINEAR, view=0), r"row \d+, column \d+"),
    "frame_no_wrap": (lambda: pick("point_framed_fwd", "bf16", C=8, Hf=21, shift=3), r"point \d+"),
    "gate_dropped": (lambda: pick("resample_bwd", "bf16", C=8, mode=R.NEAREST, gate=R.ACT_RELU, **G), r"reference 0\b"),
}


def test_every_listed_defect_has_a_case():
    assert set(DEFECT_CASES) == set(R.DEFECTS)


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_injected_defect_is_caught(defect):
    c = DEFECT_CASES[defect][0]()
    inp = R.inputs(c)
    R.check(c, R.model(c, inp), inp)                              # the honest model passes ...
    with pytest.raises(AssertionError) as e:                      # ... the defective one fails, on an element the message names
        R.check(c, R.model(c, inp, defect), inp)
    assert c.text in str(e.value) and re.search(DEFECT_CASES[defect][1], str(e.value)), str(e.value)
    also = [pick("point_bwd", "bf16", C=8, H=16, S=37, mode=R.BILINEAR, pat=0)] if defect == "collision_lost" else \
        [pick("point_bwd", "bf16", C=7945, grid=1), pick("point_fwd", "bf16", C=2056, grid=1)] if defect == "stride_tail" else \
        [pick("point_framed_bwd", "f32", C=4, Hf=21, shift=3)] if defect == "frame_no_wrap" else []
    for c in also:
        inp = R.inputs(c)
        with pytest.raises(AssertionError):
            R.check(c, R.model(c, inp, defect), inp)


# ----------------------------------------------------------------------------------------------------------------- coverage
def _classes(dt):
    return ("v8", "v4", "s") if dt == "bf16" else ("v4", "s")


def test_the_table_covers_the_dispatch_product():
    """Per entry point every combination its dispatch distinguishes: dtype x channel class x mode x pitch x gate x frame."""
    have = lambda op, dt, cls, **a: any(c.op == op and c.dtype == dt and R.channel_class(c) == cls and all(getattr(c, k) == v for k, v in a.items()) for c in R.cases())
    missing = []
    need = lambda *a, **k: None if have(*a, **k) else missing.append((a, k))
    for dt in ("bf16", "f32"):
        for cls, mode in itertools.product(_classes(dt), (R.BILINEAR, R.NEAREST)):
            need("resample_fwd", dt, cls, mode=mode, ld=0)
            need("resample_bwd", dt, cls, mode=mode, gate=0)
            if cls != "s":                                       # a pitch, the separable form and the gate need a vector kernel (-4 else)
                assert any(c.op == "resample_fwd" and c.dtype == dt and R.channel_class(c) == cls and c.mode == mode and c.ld > c.C for c in R.cases()), (dt, cls, mode)
                for pitched in (False, True):
                    assert any(c.op == "resample_bwd_sep" and c.dtype == dt and R.channel_class(c) == cls and c.mode == mode and bool(c.ld) == pitched for c in R.cases()), (dt, cls, mode, pitched)
                if mode == R.NEAREST:
                    for gate in (R.ACT_RELU, R.ACT_ELU):
                        need("resample_bwd", dt, cls, mode=mode, gate=gate)
        for cls in _classes(dt):
            need("avgpool_fwd", dt, cls)
            need("avgpool_bwd", dt, cls)
            for mode in (R.BILINEAR, R.NEAREST):
                need("point_fwd", dt, cls, mode=mode)
                need("point_bwd", dt, cls, mode=mode, pat=0)
                need("point_bwd", dt, cls, mode=mode, pat=1)
                need("point_bwd_gather", dt, cls, mode=mode, view=0)
            need("point_framed_fwd", dt, cls)
            need("point_framed_bwd", dt, cls)
        vec = "v8" if dt == "bf16" else "v4"
        for mode in (R.BILINEAR, R.NEAREST):
            need("point_bwd_gather", dt, vec, mode=mode, view=1)     # only the alignment decides
        need("psp_fwd", dt, vec)
        for gpass in (0, 1, 2):
            need("psp_bwd", dt, vec, gpass=gpass)
        need("psp_bwd", dt, vec, absent=16)
        for res in (0, 1):
            need("stride_place", dt, vec, res=res)
        assert any(c.op == "taps_collapse" and c.dtype == dt for c in R.cases())
    assert any(c.op == "taps_fold" for c in R.cases())
    assert not missing, missing
    # the pitched cases of the issue, where the f32 pitch is 2 C
    for dt, C, ld, off in R.PITCHED:
        assert any(c.op == "resample_fwd" and c.dtype == dt and c.C == C and c.ld == ld and c.off == off for c in R.cases())
    # one grid-stride case per launcher, each just above its cap
    for c in [c for c in R.cases() if R.is_grid(c)]:
        cap, per = R.work_items(c)
        items = {"resample_fwd": lambda: c.B * c.Ho * c.Wo * c.C // per, "resample_bwd": lambda: c.B * c.Hs * c.Ws * c.C // per,
                 "resample_bwd_sep": lambda: min(c.B * c.Hs * c.Ws * c.C // 4, c.B * c.Ho * c.Ws * c.C // 4),
                 "avgpool_fwd": lambda: c.B * (c.H // c.k) * (c.W // c.k) * c.C // per, "avgpool_bwd": lambda: c.B * c.H * c.W * c.C // per,
                 "psp_bwd": lambda: c.B * c.H * c.W * c.C // per, "stride_place": lambda: c.B * c.H * c.W * c.C // per,
                 "point_fwd": lambda: c.B * c.S * c.C, "point_bwd": lambda: c.B * c.C}[c.op]()
        cap = R.POINT_BWD_CAP if c.op == "point_bwd" else cap
        assert cap < items < 1.01 * cap + 4096, (c.text, items, cap)
    assert {c.op for c in R.cases() if R.is_grid(c)} == {"resample_fwd", "resample_bwd", "resample_bwd_sep", "avgpool_fwd", "avgpool_bwd", "psp_bwd", "stride_place", "point_fwd", "point_bwd"}
    for c in R.cases():                                          # all operands of a case together stay under 64 MB
        assert sum(v.numel() * v.element_size() for v in R.inputs(c).values()) < 64 << 20, c.text


def test_point_lists_hold_the_edges():
    c = pick("point_fwd", "bf16", C=8, H=16, S=37, mode=R.NEAREST)
    pts = R.inputs(c)["coords"]
    ix = R.unnormalize64(pts[0, :, 0], 16)
    assert {-0.5, 0.5, 1.5, 15.5} <= set(ix.tolist()) and bool((pts[0, 0] == pts[0, 1]).all())
    assert bool((pts.abs() == 3).any()) and bool((pts.abs() == 1e6).any())
    for c in R.cases():                                          # ties and pixel centres only where the coordinate arithmetic is exact
        if c.op.startswith("point") and c.pts == "mix":
            Hs, Ws = (c.Hf, c.Wf) if hasattr(c, "Hf") else (c.H, c.W)
            if not (R._pow2(Hs) and R._pow2(Ws)):
                p = R.inputs(c)["coords"]
                rand = p[:, 6:] if c.S > 6 else p[:, :0]
                assert not bool(R._near_boundary(c, rand, Hs, Ws).any()), c.text
    f = pick("point_framed_fwd", "bf16", Hf=21, shift=3)
    taps, _, _ = R._point_taps(R.inputs(f)["coords"].double(), f.Hf, f.Wf, R.NEAREST, torch.float64)
    y, x, _, ok = taps[0]
    ym, xm = (y + f.shift) % f.Hf, (x + f.shift) % f.Wf
    assert bool((~ok).any()) and bool((ok & ((ym >= f.H) | (xm >= f.W))).any()) and bool((ok & (y + f.shift >= f.Hf)).any())     # outside, padding, wrapped


def test_redrawn_points_are_rare():
    total = drawn = 0
    for c in R.cases():
        if c.op.startswith("point"):
            R.inputs(c)
            a, n = R.REDRAWN[c.text]
            assert a <= 0.01 * n, (c.text, a, n)
            total, drawn = total + a, drawn + n
    print("re-drawn points: %d of %d (%.4f %%)" % (total, drawn, 100.0 * total / drawn))
    assert total <= 0.01 * drawn


def test_measured_is_fresh():
    fresh = R.measure_c()
    assert set(fresh) == set(R.MEASURED)
    for k, v in fresh.items():
        assert "%.3f" % v == "%.3f" % R.MEASURED[k], (k, v, R.MEASURED[k])
    assert R.format_table(R.MEASURED) in R.__doc__
    assert all(R.C[k] == R.c_of(v) for k, v in R.MEASURED.items())
