"""fp64 references, error bounds and rounding models of the gather / scatter kernels of csrc/resample.hip and csrc/pointsample.hip (CPU only,
plain module; the instrument is the one of tests/attn_ref.py: assert_elementwise, ratio, FLOOR and the unit round-offs come from there).

``cases()`` is the table: one small namespace per call, its one-line text the test id and the seed of its operands.  ``inputs(c)`` draws the
operands in the storage type; every reference works on those rounded operands, so the only error left between a kernel and its reference is
the kernel's own arithmetic.  The table is written against the predicates of the dispatch (dtype, C % 8, C % 4, mode, pitch, gate, frame);
tests/test_spatial_ref.py proves that it covers their product.

* ``reference(c, inp)`` -> (ref, cond): per output the fp64 result and the pair (A, B) of the bound
      |got - ref| <= C u (|ref| + A + (2^-24 / u) B),      u = 2^-9 for a bf16 output, 2^-24 for an fp32 one.
  A is in units of the output's own rounding, B in units of fp32's.  Every kernel but the scatter backward computes in fp32 and rounds once, at
  the store (A = 0).  A zero bound demands an exact zero: remainder rows of avgpool_backward, dead pixels of stride_place without a residual,
  pixels no point touches in the gather backward, out-of-image points in the forward, a closed ReLU gate.  u32 = 2^-24 below.
      resample, bilinear   y = A_y x A_x^T, gx = A_y^T gy A_x with the per-axis operators A (Ho x Hs), weights from the exact ratio (Hs-1)/(Ho-1)
                           (0 when Ho == 1).  The kernel's coordinate f = fl(fl(scale) o) carries |df| <= 2 u32 f, so each of its two weights is off
                           by 2 u32 f + u32 ABSOLUTELY, and at an integer coordinate it may take the pixel pair (s-1, s) with weights (~0, ~1) where
                           the reference takes (s, s+1): the result is continuous there, but its error scales with |x| of a pixel the reference
                           never reads.  Hence W = S_y |x| S_x^T over the support WIDENED by one pixel each side per axis (S: ones on s0-1 .. s0+2), and
                               forward   B = 4 (|A_y| |x| |A_x|^T) + (2 f_y + 2 f_x + 4) W                       (4: two products, two sums per tap pair)
                               backward  B = (sqrt(n) + 4) (|A_y|^T |gy| |A_x|) + (2 (s_y + 2) + 2 (s_x + 2) + 4) (S_y^T |gy| S_x),
                           n = taps of the source pixel's footprint (an fp32 sum of n terms, sqrt as for the column sums of tests/row_ref.py); the
                           outputs that reach source s have a coordinate below s + 2.  The separable form sums the same terms in two passes.
      resample, nearest    index floorf(o * ((float)Hs / (float)Ho)) evaluated in numpy float32: that rule IS the specification (it is torch's;
                           14 -> 46 sends row 23 to 6, 26 -> 22 row 11 to 12, the rational floor(o Hs / Ho) gives 7 and 13).  Forward: a copy, bound
                           zero beyond the store (asserted bit-exact as well).  Backward: B = (sqrt(n) + 1) sum |gy| over the footprint, no
                           coordinate term (the weights are exactly 0 / 1).  Gate: gx *= act'(gate); B = act' B (+ 2 |gx| for the ELU's r + 1);
                           a closed gate and a source no output reads are exact zeros.
      average pool         forward B = (k + 2) mean |x| (an fp32 sum of k^2 terms, then 1 / k^2 rounded); backward gx = gy / k^2: B = 2 |gx|, remainder
                           rows and columns zero.  PSP forward: the same per level k = 16, 8, 4, 2 (the coarser levels are sums of the finer fp32
                           sums); PSP backward gx = g_pass + sum_k g_k / k^2: B = 5 (|g_pass| + sum_k |g_k| / k^2).
      stride_place         without a residual a copy and exact zeros (bit-exact); with one, a single rounded sum of two storage values: bound u |ref|.
      tap collapse, fold   sums of at most four fp32 values: B = 2 sum |w|;  fold: dw = pattern + sum D, B = 3 (|pattern| + sum |D|).
      point sample         grid_sample(align_corners=False, padding_mode='zeros'), i = ((c + 1) size - 1) / 2.  In fp32 (fused or not)
                           |di| <= 3 u32 (|i| + size); with W the sum of |map| over the in-image pixels of x0-1 .. x0+2, y0-1 .. y0+2:
                               forward (fp32 out)   B = 4 sum |w x| + (3 (|ix| + |iy| + W + H) + 4) Wide;    far outside the image Wide = 0: exact zero
                               gather backward      B = (sqrt(n) + 4) sum |w g| + (6 (W + H) + 4) sum_{points within the widened support} |g|
                               scatter backward     the same B, and A = n (|pattern| + sum |w g|): the kernel rounds gmap to STORAGE after every one
                                                    of the n tap hits of a pixel (n = S when all points sit on one pixel)
                           nearest: copies (forward) and plain sums of g (backward: B = (sqrt(n) + 1) sum |g|; scatter A as above), the pixel being
                           nearbyint (half to even) of i.  Discontinuous decisions are used only where they are exact: ties and pixel centres
                           appear only where H, W are powers of two ((c + 1) W - 1 is then exact in fp32, fused or not); elsewhere a point
                           within 1e-4 of a rounding boundary (half-integer for nearest, integer for the bilinear floor) is re-drawn
                           (REDRAWN counts them; tests/test_spatial_ref.py caps the share at 1 %).
                           framed: the same on torch.roll(F.pad(map, to (Hf, Wf)), (-shift, -shift)), nearest only.
* ``model(c, inp, defect=None)`` - the kernels' arithmetic in fp32 on the CPU with the ONE rounding at the store (the scatter backward rounds after
  every hit, as the kernel does), the taps summed in the opposite order.  It sizes C without a kernel's output and carries the injected
  DEFECTS of tests/test_spatial_ref.py.

The constants.  ``measure_c()`` evaluates the model over cases() and takes the largest |model - ref| / bound per operation, output and type; C is
twice that, rounded up to one decimal (the factor 2 covers the device's summation order and its fused multiply-adds).  Measured on the CPU, 2026-10:

@TABLE@

A kernel that needs more than its C has a defect or the bound lacks a term: neither is repaired by raising C.
"""
import types
import zlib

import numpy as np
import torch
import torch.nn.functional as F

from tests.attn_ref import FLOOR, U_BF16, U_F32, assert_elementwise, ratio        # noqa: F401  (the instrument)
from tests.conv_ref import c_of

BILINEAR, NEAREST = 0, 1
ACT_NONE, ACT_RELU, ACT_ELU = 0, 1, 3
FLAT_CAP, POINT_FWD_CAP, POINT_BWD_CAP = 8192 * 256, 4096 * 256, 4096 * 64       # work items of one grid-stride trip
DEFECTS = ("last_row_clamp", "footprint_short", "nearest_rational", "stride_tail", "pitch_as_c", "pool_remainder", "psp_partial_block",
           "stride_live_guard", "tie_away", "border_weight", "collision_lost", "frame_no_wrap", "gate_dropped")
F32_OUT = ("point_fwd", "point_framed_fwd", "taps_fold")                          # fp32 outputs whatever the map's type
REDRAWN = {}                                                                     # case text -> (re-drawn, random points drawn)


def torch_dtype(c):
    return torch.bfloat16 if c.dtype == "bf16" else torch.float32


def out_unit(c):
    return U_F32 if c.op in F32_OUT or c.dtype == "f32" else U_BF16


def channel_class(c):
    if c.C % 8 == 0 and c.dtype == "bf16":
        return "v8"
    return "v4" if c.C % 4 == 0 else "s"


def pattern(*shape):
    """What the ACCUMULATED outputs (dw of the fold, gmap of the scatter backward) hold before the call: non-zero, exact in bf16."""
    n = int(np.prod(shape))
    return (0.5 + 0.25 * (torch.arange(n) % 7).float()).reshape(shape)


# ---------------------------------------------------------------------------------------------------------------- cases
def _case(op, dtype, **kw):
    c = types.SimpleNamespace(op=op, dtype=dtype, **kw)
    c.text = "%s %s %s" % (op, dtype, " ".join("%s=%s" % (k, v) for k, v in kw.items()))
    return c


RESAMPLE_GEOMETRIES = [(2, 3, 5, 7, 9), (1, 1, 1, 4, 3), (1, 4, 3, 1, 1), (1, 5, 4, 5, 4), (1, 14, 3, 46, 5), (1, 26, 7, 22, 3), (2, 2, 2, 33, 31), (1, 6, 8, 12, 16)]
CHANNELS = {"bf16": (8, 16, 4, 12, 3, 1), "f32": (4, 8, 3, 1)}
PITCHED = [("bf16", 8, 24, 8), ("bf16", 4, 12, 4), ("f32", 4, 8, 4)]                # dtype, C, pitch, offset
POOL_GEOMETRIES = [(1, 4, 6, 2), (2, 17, 19, 8), (1, 5, 5, 5), (1, 3, 3, 1), (1, 7, 10, 3)]
PSP_GEOMETRIES = [("bf16", 1, 16, 16, 8), ("bf16", 2, 17, 31, 40), ("bf16", 1, 33, 47, 24), ("f32", 1, 16, 16, 4), ("f32", 2, 17, 31, 20), ("f32", 1, 33, 47, 4)]
STRIDE_GEOMETRIES = [(1, 8, 8, 4, 4, 2), (2, 7, 9, 4, 5, 2), (1, 9, 9, 2, 2, 3)]
POINT_MAPS = [(16, 16), (5, 7), (1, 1), (21, 21)]
POINT_CHANNELS = {"bf16": (8, 16, 4, 1), "f32": (4, 3, 1)}
FRAMES = [(15, 20, 21, 21, 3), (16, 16, 16, 16, 0), (5, 7, 8, 8, 7), (1, 1, 4, 4, 2)]


def _build_cases():
    out = []
    add = lambda *a, **k: out.append(_case(*a, **k))
    for dt in ("bf16", "f32"):
        for (B, Hs, Ws, Ho, Wo) in RESAMPLE_GEOMETRIES:
            for C in CHANNELS[dt]:
                for mode in (BILINEAR, NEAREST):
                    g = dict(B=B, Hs=Hs, Ws=Ws, Ho=Ho, Wo=Wo, C=C, mode=mode)
                    add("resample_fwd", dt, ld=0, off=0, **g)
                    add("resample_bwd", dt, gate=ACT_NONE, **g)
                    if C % 4 == 0:
                        add("resample_bwd_sep", dt, ld=0, off=0, **g)
                        if mode == NEAREST:
                            add("resample_bwd", dt, gate=ACT_RELU, **g)
                            add("resample_bwd", dt, gate=ACT_ELU, **g)
    for dt, C, ld, off in PITCHED:
        for (B, Hs, Ws, Ho, Wo) in ((2, 3, 5, 7, 9), (2, 2, 2, 33, 31)):
            for mode in (BILINEAR, NEAREST):
                g = dict(B=B, Hs=Hs, Ws=Ws, Ho=Ho, Wo=Wo, C=C, mode=mode)
                add("resample_fwd", dt, ld=ld, off=off, **g)
                add("resample_bwd_sep", dt, ld=ld, off=off, **g)
    for dt in ("bf16", "f32"):
        for (B, H, W, k) in POOL_GEOMETRIES:
            for C in CHANNELS[dt]:
                add("avgpool_fwd", dt, B=B, H=H, W=W, C=C, k=k)
                add("avgpool_bwd", dt, B=B, H=H, W=W, C=C, k=k)
    for dt, B, H, W, C in PSP_GEOMETRIES:
        add("psp_fwd", dt, B=B, H=H, W=W, C=C)
        for gpass in (0, 1, 2):                                                  # absent, contiguous, a slice at C of a 3 C wide map
            add("psp_bwd", dt, B=B, H=H, W=W, C=C, gpass=gpass, absent=0)
        add("psp_bwd", dt, B=B, H=H, W=W, C=C, gpass=1, absent=16)               # a pool the loss never read: its gradient is None
        add("psp_bwd", dt, B=B, H=H, W=W, C=C, gpass=0, absent=2)
    for dt, C in (("bf16", 8), ("bf16", 24), ("f32", 4), ("f32", 12)):
        for (B, H, W, Ho, Wo, s) in STRIDE_GEOMETRIES:
            for res in (0, 1):
                add("stride_place", dt, B=B, H=H, W=W, Ho=Ho, Wo=Wo, s=s, C=C, res=res)
    for (Cout, Cin) in ((1, 1), (3, 5), (64, 64)):
        add("taps_collapse", "bf16", Cout=Cout, Cin=Cin)
        add("taps_collapse", "f32", Cout=Cout, Cin=Cin)
        add("taps_fold", "f32", Cout=Cout, Cin=Cin)
    n = 0
    for (H, W) in POINT_MAPS:
        for S in (1, 2, 37, 256):
            for dt in ("bf16", "f32"):
                for C in POINT_CHANNELS[dt]:
                    for mode in (BILINEAR, NEAREST):
                        n += 1
                        g = dict(B=1 + n % 2, H=H, W=W, C=C, S=S, mode=mode, pts="mix")
                        add("point_fwd", dt, **g)
                        add("point_bwd_gather", dt, view=0, **g)
                        add("point_bwd", dt, pat=n // 2 % 2, **g)
    for dt, C in (("bf16", 8), ("f32", 4)):
        for mode in (BILINEAR, NEAREST):
            add("point_bwd", dt, pat=0, B=1, H=5, W=7, C=C, S=257, mode=mode, pts="mix")
            add("point_bwd", dt, pat=1, B=2, H=16, W=16, C=C, S=257, mode=mode, pts="mix")
            add("point_bwd_gather", dt, view=1, B=2, H=16, W=16, C=C, S=37, mode=mode, pts="mix")      # gmap one element into a larger buffer
            for op, extra in (("point_fwd", {}), ("point_bwd_gather", {"view": 0}), ("point_bwd", {"pat": 0}), ("point_bwd", {"pat": 1})):
                add(op, dt, B=1, H=16, W=16, C=C, S=256, mode=mode, pts="onepixel", **extra)
    for (H, W, Hf, Wf, shift) in FRAMES:
        for dt in ("bf16", "f32"):
            for i, C in enumerate(POINT_CHANNELS[dt]):
                g = dict(B=1 + i % 2, H=H, W=W, C=C, S=(37, 256, 2, 1)[i], Hf=Hf, Wf=Wf, shift=shift, mode=NEAREST, pts="mix")
                add("point_framed_fwd", dt, **g)
                add("point_framed_bwd", dt, **g)
    # one grid-stride case per kernel template, the work-item count just above the launcher's cap
    add("resample_fwd", "bf16", B=1, Hs=5, Ws=7, Ho=701, Wo=1000, C=3, mode=BILINEAR, ld=0, off=0, grid=1)
    add("resample_fwd", "bf16", B=1, Hs=3, Ws=3, Ho=1449, Wo=1449, C=8, mode=BILINEAR, ld=0, off=0, grid=1)
    add("resample_bwd", "bf16", B=1, Hs=1450, Ws=1450, Ho=1451, Wo=1452, C=1, mode=BILINEAR, gate=ACT_NONE, grid=1)
    add("resample_bwd", "bf16", B=1, Hs=1450, Ws=1450, Ho=1451, Wo=1452, C=4, mode=NEAREST, gate=ACT_NONE, grid=1)
    add("resample_bwd_sep", "bf16", B=1, Hs=1450, Ws=1450, Ho=1451, Wo=1452, C=4, mode=BILINEAR, ld=0, off=0, grid=1)
    add("avgpool_fwd", "bf16", B=1, H=2898, W=2899, C=1, k=2, grid=1)
    add("avgpool_fwd", "bf16", B=1, H=1449, W=1450, C=4, k=1, grid=1)
    add("avgpool_bwd", "bf16", B=1, H=1449, W=1450, C=1, k=2, grid=1)
    add("avgpool_bwd", "bf16", B=1, H=1449, W=1450, C=4, k=2, grid=1)
    add("psp_bwd", "bf16", B=1, H=1449, W=1449, C=8, gpass=0, absent=0, grid=1)
    add("stride_place", "bf16", B=1, H=1449, W=1449, Ho=725, Wo=725, s=2, C=8, res=0, grid=1)
    add("point_fwd", "bf16", B=2, H=3, W=3, C=2056, S=256, mode=BILINEAR, pts="mix", grid=1)
    add("point_bwd", "bf16", pat=0, B=33, H=1, W=2, C=7945, S=2, mode=BILINEAR, pts="mix", grid=1)
    assert len({c.text for c in out}) == len(out)
    return out


_CASES = []


def cases():
    if not _CASES:
        _CASES.extend(_build_cases())
    return _CASES


def is_grid(c):
    return bool(getattr(c, "grid", 0))


def exact_kind(c):
    if c.op == "resample_fwd" and c.mode == NEAREST:
        return "nearest_fwd"
    if c.op == "stride_place" and not c.res:
        return "stride_place_plain"
    return None


def operation(c):
    if c.op.startswith("resample"):
        return c.op + ("_nearest" if c.mode == NEAREST else "_bilinear")
    if c.op.startswith("point") and "framed" not in c.op:
        return c.op + ("_nearest" if c.mode == NEAREST else "_bilinear")
    return c.op


# --------------------------------------------------------------------------------------------------------------- inputs
def _gen(c):
    return torch.Generator().manual_seed(zlib.crc32(c.text.encode()))


def _pow2(n):
    return n & (n - 1) == 0


def unnormalize64(coord, size):
    return ((coord.double() + 1.0) * size - 1.0) / 2.0


def _near_boundary(c, pts, Hs, Ws):
    half = 0.5 if c.mode == NEAREST else 0.0
    near = torch.zeros(pts.shape[:-1], dtype=torch.bool)
    for k, size in ((0, Ws), (1, Hs)):
        i = unnormalize64(pts[..., k], size) - half
        near |= (i - i.round()).abs() < 1e-4
    return near


def _points(c, g):
    """(B, S, 2) normalised (x, y) in fp32: see the module docstring and the issue's list."""
    B, S = c.B, c.S
    Hs, Ws = (c.Hf, c.Wf) if hasattr(c, "Hf") else (c.H, c.W)
    if c.pts == "onepixel":                                      # every point inside pixel (6, 5): one bilinear cell, one nearest pixel
        jit = torch.rand(B, S, 2, generator=g) * 0.4 + 0.05
        pix = torch.tensor([5.0, 6.0]) + jit
        pts = (2 * pix + 1) / torch.tensor([float(Ws), float(Hs)]) - 1
        REDRAWN[c.text] = (0, B * S)
        return pts.float()
    pts = (torch.rand(B, S, 2, generator=g) * 2.4 - 1.2).float()
    redrawn = 0
    if not (_pow2(Hs) and _pow2(Ws)):
        for _ in range(8):
            near = _near_boundary(c, pts, Hs, Ws)
            if not bool(near.any()):
                break
            redrawn += int(near.sum())
            pts[near] = (torch.rand(int(near.sum()), 2, generator=g) * 2.4 - 1.2).float()
        assert not bool(_near_boundary(c, pts, Hs, Ws).any())
    REDRAWN[c.text] = (redrawn, B * S)
    special = [None, "dup", (3.0, 0.1), (-0.2, -3.0), (1e6, 0.0), (0.3, -1e6)]
    if (Hs, Ws) == (16, 16):
        special += [(-1.0, -1.0), (1.0, -1.0), (-1.0, 1.0), (1.0, 1.0)]                                  # corners: i = -0.5 and 15.5
        special += [((2 * x + 1) / 16.0 - 1, (2 * y + 1) / 16.0 - 1) for x, y in ((0, 0), (15, 15), (3, 9), (15, 0))]     # pixel centres
        tie = [(2 * i + 1) / 16.0 - 1 for i in (-0.5, 0.5, 1.5, 15.5)]
        special += [(tie[0], tie[1]), (tie[2], tie[3]), (tie[1], 0.3), (0.1, tie[2]), (tie[3], tie[0])]
    for s, p in enumerate(special[:S]):
        if p == "dup":
            pts[:, 1] = pts[:, 0]
        elif p is not None:
            pts[:, s] = torch.tensor(p)
    return pts


def _gate_values(g, shape, dt):
    """An activation OUTPUT: positive, negative above -1 (an ELU's range) and exact zeros."""
    r = torch.randn(shape, generator=g)
    r = torch.where(r > 0, r, torch.expm1(r).clamp_min(-0.98))
    r[torch.rand(shape, generator=g) < 0.15] = 0.0
    return r.to(dt)


def inputs(c):
    """The operands of a case: a dict of CPU tensors in the storage type (fp32 for coordinates, point gradients and tap weights)."""
    g, dt = _gen(c), torch_dtype(c)
    rnd = lambda *shape: torch.randn(*shape, generator=g)
    op = c.op
    if op == "resample_fwd":
        return {"x": rnd(c.B, c.Hs, c.Ws, c.C).to(dt)}
    if op in ("resample_bwd", "resample_bwd_sep"):
        inp = {"gy": rnd(c.B, c.Ho, c.Wo, c.C).to(dt)}
        if getattr(c, "gate", 0):
            inp["gate"] = _gate_values(g, (c.B, c.Hs, c.Ws, c.C), dt)
        return inp
    if op == "avgpool_fwd":
        return {"x": (rnd(c.B, c.H, c.W, c.C) + 0.5).to(dt)}
    if op == "avgpool_bwd":
        return {"gy": rnd(c.B, c.H // c.k, c.W // c.k, c.C).to(dt)}
    if op == "psp_fwd":
        return {"x": (rnd(c.B, c.H, c.W, c.C) + 0.5).to(dt)}
    if op == "psp_bwd":
        inp = {}
        if c.gpass:
            inp["gpass"] = rnd(c.B, c.H, c.W, c.C).to(dt)
        for k in (16, 8, 4, 2):
            if k != c.absent:
                inp["g%d" % k] = rnd(c.B, c.H // k, c.W // k, c.C).to(dt)
        return inp
    if op == "stride_place":
        inp = {"src": rnd(c.B, c.Ho, c.Wo, c.C).to(dt)}
        if c.res:
            inp["residual"] = rnd(c.B, c.H, c.W, c.C).to(dt)
        return inp
    if op == "taps_collapse":
        return {"w": rnd(c.Cout, 3, 3, c.Cin)}
    if op == "taps_fold":
        return {"D": rnd(c.Cin, 4, 4, c.Cout)}
    inp = {"coords": _points(c, g)}
    if op in ("point_fwd", "point_framed_fwd"):
        inp["map"] = rnd(c.B, c.H, c.W, c.C).to(dt)
    else:
        inp["gout"] = rnd(c.B, c.S, c.C)
    return inp


# ------------------------------------------------------------------------------------------------------ axis operators
class Axis:
    """A sparse per-axis operator (n_out x n_in): row o reads the columns idx[o, :] with the weights w[o, :]."""

    def __init__(self, n_in, idx, w, coord=None):
        self.n_in, self.idx, self.w, self.coord = n_in, idx, w, coord

    @staticmethod
    def _shape(t, dim):
        s = [1] * t.dim()
        s[dim] = -1
        return s

    def fwd(self, t, dim, w=None):
        w = self.w if w is None else w
        out = None
        for k in reversed(range(self.idx.shape[1])):
            term = t.index_select(dim, self.idx[:, k]) * w[:, k].to(t.dtype).reshape(self._shape(t, dim))
            out = term if out is None else out + term
        return out

    def bwd(self, t, dim, w=None):
        w = self.w if w is None else w
        shape = list(t.shape)
        shape[dim] = self.n_in
        out = torch.zeros(shape, dtype=t.dtype)
        for k in reversed(range(self.idx.shape[1])):
            out.index_add_(dim, self.idx[:, k], t * w[:, k].to(t.dtype).reshape(self._shape(t, dim)))
        return out

    def taps(self):
        """Per source column the number of non-zero taps."""
        return self.bwd(torch.ones(self.idx.shape[0], dtype=torch.float64), 0, (self.w != 0).double())

    def widened(self):
        """S: ones on the columns i0-1 .. i0+2 (inside the axis) of each row."""
        i0 = self.idx[:, :1]
        idx = i0 + torch.arange(-1, 3)[None, :]
        ok = (idx >= 0) & (idx < self.n_in)
        return Axis(self.n_in, idx.clamp(0, self.n_in - 1), ok.double())

    def drop_last_output(self):
        """The footprint of every source column one output short at its upper end (defect footprint_short)."""
        o = torch.arange(self.idx.shape[0])[:, None].expand_as(self.idx)
        live = self.w != 0
        top = torch.full((self.n_in,), -1, dtype=torch.long)
        top.scatter_reduce_(0, self.idx[live], o[live], "amax")
        w = self.w.clone()
        w[live & (o == top[self.idx])] = 0
        return Axis(self.n_in, self.idx, w, self.coord)


def nearest_index(n_in, n_out):
    """torch's (and the kernel's) legacy-nearest source index: floorf(o * ((float)n_in / (float)n_out)) in fp32, clamped."""
    scale = np.float32(n_in) / np.float32(n_out)
    f = np.arange(n_out, dtype=np.float32) * scale
    assert f.dtype == np.float32
    return torch.from_numpy(np.minimum(np.floor(f).astype(np.int64), n_in - 1))


def axis64(n_in, n_out, mode):
    if mode == NEAREST:
        idx = nearest_index(n_in, n_out)
        return Axis(n_in, idx[:, None], torch.ones(n_out, 1, dtype=torch.float64), idx.double())
    o = torch.arange(n_out, dtype=torch.float64)
    f = o * (n_in - 1) / (n_out - 1) if n_out > 1 else torch.zeros(1, dtype=torch.float64)
    i0 = f.floor().long().clamp_max(n_in - 1)
    i1 = (i0 + 1).clamp_max(n_in - 1)
    l = f - i0
    return Axis(n_in, torch.stack([i0, i1], 1), torch.stack([1 - l, l], 1), f)


def axis32(n_in, n_out, mode, defect=None):
    """The operator as the kernels compute it in fp32 (ac_scale, tap_weight of csrc/resample.hip)."""
    o = torch.arange(n_out, dtype=torch.float32)
    if mode == NEAREST:
        if defect == "nearest_rational":
            idx = (torch.arange(n_out) * n_in) // n_out
        else:
            idx = torch.floor(o * (torch.tensor(float(n_in)) / torch.tensor(float(n_out)))).long().clamp_max(n_in - 1)
        return Axis(n_in, idx[:, None], torch.ones(n_out, 1))
    scale = torch.tensor(float(n_in - 1)) / torch.tensor(float(n_out - 1)) if n_out > 1 else torch.tensor(0.0)
    f = scale * o
    i0 = f.long()
    i1 = i0 + (i0 < n_in - (2 if defect == "last_row_clamp" else 1)).long()
    l = f - i0.float()
    return Axis(n_in, torch.stack([i0, i1], 1), torch.stack([1.0 - l, l], 1))


# ------------------------------------------------------------------------------------------------------------ reference
def _bcast(v_y, v_x):
    return (v_y[:, None] + v_x[None, :])[None, :, :, None]


def _gate_grad(r, act):
    return (r > 0).to(r.dtype) if act == ACT_RELU else torch.where(r > 0, torch.ones_like(r), r + 1.0)


def _pool(x, k):
    B, H, W, C = x.shape
    Ho, Wo = H // k, W // k
    return x[:, :Ho * k, :Wo * k].reshape(B, Ho, k, Wo, k, C).mean((2, 4))


def _unpool(g, k, H, W):
    """g (B, H/k, W/k, C) / k^2 spread over its windows; remainder rows and columns zero."""
    B, Ho, Wo, C = g.shape
    out = torch.zeros(B, H, W, C, dtype=g.dtype)
    out[:, :Ho * k, :Wo * k] = (g / (k * k))[:, :, None, :, None, :].expand(B, Ho, k, Wo, k, C).reshape(B, Ho * k, Wo * k, C)
    return out


def _collapse(w):
    """w (Cout,3,3,Cin) -> (Cin,4,4,Cout): wk[ci][t][s][co] = sum over kh in [max(0,2-t), min(2,3-t)], kw likewise."""
    Cout, _, _, Cin = w.shape
    out = torch.zeros(Cin, 4, 4, Cout, dtype=w.dtype)
    for t in range(4):
        for s in range(4):
            for kh in range(max(0, 2 - t), min(2, 3 - t) + 1):
                for kw in range(max(0, 2 - s), min(2, 3 - s) + 1):
                    out[:, t, s, :] += w[:, kh, kw, :].t()
    return out


def _fold(D):
    """D (Cin,4,4,Cout) -> (Cout,3,3,Cin): sum over t in [2-kh, 3-kh], s in [2-kw, 3-kw]."""
    Cin, _, _, Cout = D.shape
    out = torch.zeros(Cout, 3, 3, Cin, dtype=D.dtype)
    for kh in range(3):
        for kw in range(3):
            for t in range(2 - kh, 4 - kh):
                for s in range(2 - kw, 4 - kw):
                    out[:, kh, kw, :] += D[:, t, s, :].t()
    return out


def framed(fmap, Hf, Wf, shift):
    t = F.pad(fmap, (0, 0, 0, Wf - fmap.shape[2], 0, Hf - fmap.shape[1]))
    return torch.roll(t, shifts=(-shift, -shift), dims=(1, 2)) if shift else t


def _point_taps(coords, H, W, mode, dtype, defect=None):
    """-> list of (y, x, weight, inside) per tap, each (B, S), and the un-normalised (ix, iy)."""
    if dtype == torch.float64:
        ix, iy = unnormalize64(coords[..., 0], W), unnormalize64(coords[..., 1], H)
    else:
        one, two = torch.tensor(1.0), torch.tensor(2.0)
        ix, iy = ((coords[..., 0] + one) * float(W) - one) / two, ((coords[..., 1] + one) * float(H) - one) / two
    inside = lambda y, x: (y >= 0) & (y < H) & (x >= 0) & (x < W)
    if mode == NEAREST:
        rnd = (lambda v: torch.sign(v) * torch.floor(v.abs() + 0.5)) if defect == "tie_away" else torch.round
        x, y = rnd(ix).long(), rnd(iy).long()
        return [(y, x, torch.ones_like(ix), inside(y, x))], ix, iy
    x0, y0 = torch.floor(ix), torch.floor(iy)
    wx1, wy1 = ix - x0, iy - y0
    wx0, wy0 = (x0 + 1) - ix, (y0 + 1) - iy
    x0, y0 = x0.long(), y0.long()
    taps = []
    for (dy, wy) in ((0, wy0), (1, wy1)):
        for (dx, wx) in ((0, wx0), (1, wx1)):
            y, x = y0 + dy, x0 + dx
            ok = inside(y, x)
            if defect == "border_weight":                        # clamped to the border instead of dropped
                ok = torch.ones_like(ok) & (y > -3) & (y < H + 2) & (x > -3) & (x < W + 2)
            taps.append((y, x, wx * wy, ok))
    return taps, ix, iy


def _sample(fmap, taps):
    """sum over the taps of map[b, y, x, :] * w  ->  (B, S, C), in the map's dtype."""
    B, H, W, C = fmap.shape
    b = torch.arange(B)[:, None]
    out = None
    for (y, x, w, ok) in reversed(taps):
        term = fmap[b, y.clamp(0, H - 1), x.clamp(0, W - 1)] * (w * ok).to(fmap.dtype)[..., None]
        out = term if out is None else out + term
    return out


def _spread(g, taps, H, W, accumulate=True):
    """The transpose: (B, H, W, C) += g (B, S, C) * w at the taps."""
    B, S, C = g.shape
    out = torch.zeros(B, H, W, C, dtype=g.dtype)
    b = torch.arange(B)[:, None].expand(B, S)
    for (y, x, w, ok) in reversed(taps):
        out.index_put_((b[ok], y.clamp(0, H - 1)[ok], x.clamp(0, W - 1)[ok]), (g * w.to(g.dtype)[..., None])[ok], accumulate=accumulate)
    return out


def _wide_taps(taps, H, W):
    y0, x0 = taps[0][0], taps[0][1]
    out = []
    for dy in range(-1, 3):
        for dx in range(-1, 3):
            y, x = y0 + dy, x0 + dx
            out.append((y, x, torch.ones(y.shape, dtype=torch.float64), (y >= 0) & (y < H) & (x >= 0) & (x < W)))
    return out


def _frame_roll_back(gf, c):
    if c.shift:
        gf = torch.roll(gf, shifts=(c.shift, c.shift), dims=(1, 2))
    return gf[:, :c.H, :c.W]


def reference(c, inp):
    """-> (ref, cond) over the outputs of the case."""
    d = {k: v.double() for k, v in inp.items()}
    op = c.op
    z = lambda t: torch.zeros_like(t)
    if op.startswith("resample"):
        ay, ax = axis64(c.Hs, c.Ho, c.mode), axis64(c.Ws, c.Wo, c.mode)
        if op == "resample_fwd":
            x = d["x"]
            ref = ax.fwd(ay.fwd(x, 1), 2)
            if c.mode == NEAREST:
                return {"y": ref}, {"y": (z(ref), None)}
            absr = ax.fwd(ay.fwd(x.abs(), 1), 2)
            wide = ax.widened().fwd(ay.widened().fwd(x.abs(), 1), 2)
            return {"y": ref}, {"y": (z(ref), 4 * absr + (_bcast(2 * ay.coord, 2 * ax.coord) + 4) * wide)}
        gy = d["gy"]
        ref = ay.bwd(ax.bwd(gy, 2), 1)
        absr = ay.bwd(ax.bwd(gy.abs(), 2), 1)
        n = (ay.taps()[:, None] * ax.taps()[None, :])[None, :, :, None]
        if c.mode == NEAREST:
            b = (n.sqrt() + 1) * absr
        else:
            wide = ay.widened().bwd(ax.widened().bwd(gy.abs(), 2), 1)
            sy, sx = torch.arange(c.Hs, dtype=torch.float64), torch.arange(c.Ws, dtype=torch.float64)
            b = (n.sqrt() + 4) * absr + (_bcast(2 * (sy + 2), 2 * (sx + 2)) + 4) * wide
        if getattr(c, "gate", 0):
            a = _gate_grad(d["gate"], c.gate)
            ref = ref * a
            b = a * b + (2 * ref.abs() if c.gate == ACT_ELU else 0)
        return {"gx": ref}, {"gx": (z(ref), b)}
    if op == "avgpool_fwd":
        ref = _pool(d["x"], c.k)
        return {"y": ref}, {"y": (z(ref), (c.k + 2) * _pool(d["x"].abs(), c.k))}
    if op == "avgpool_bwd":
        ref = _unpool(d["gy"], c.k, c.H, c.W)
        return {"gx": ref}, {"gx": (z(ref), 2 * ref.abs())}
    if op == "psp_fwd":
        ref = {"p%d" % k: _pool(d["x"], k) for k in (16, 8, 4, 2)}
        return ref, {"p%d" % k: (z(ref["p%d" % k]), (k + 2) * _pool(d["x"].abs(), k)) for k in (16, 8, 4, 2)}
    if op == "psp_bwd":
        ref = d["gpass"].clone() if "gpass" in d else torch.zeros(c.B, c.H, c.W, c.C, dtype=torch.float64)
        absr = ref.abs()
        for k in (16, 8, 4, 2):
            if "g%d" % k in d:
                ref = ref + _unpool(d["g%d" % k], k, c.H, c.W)
                absr = absr + _unpool(d["g%d" % k].abs(), k, c.H, c.W)
        return {"gx": ref}, {"gx": (z(ref), 5 * absr)}
    if op == "stride_place":
        ref = d["residual"].clone() if "residual" in d else torch.zeros(c.B, c.H, c.W, c.C, dtype=torch.float64)
        ref[:, 0:c.Ho * c.s:c.s, 0:c.Wo * c.s:c.s] += d["src"]
        return {"dst": ref}, {"dst": (z(ref), None)}
    if op == "taps_collapse":
        ref = _collapse(d["w"])
        return {"wk": ref}, {"wk": (z(ref), 2 * _collapse(d["w"].abs()))}
    if op == "taps_fold":
        p = pattern(c.Cout, 3, 3, c.Cin).double()
        return {"dw": p + _fold(d["D"])}, {"dw": (z(p), 3 * (p + _fold(d["D"].abs())))}
    # ---- point sample
    H, W = (c.Hf, c.Wf) if "framed" in op else (c.H, c.W)
    taps, ix, iy = _point_taps(d["coords"], H, W, c.mode, torch.float64)
    if op in ("point_fwd", "point_framed_fwd"):
        fmap = framed(d["map"], c.Hf, c.Wf, c.shift) if "framed" in op else d["map"]
        ref = _sample(fmap, taps)
        if c.mode == NEAREST:
            return {"out": ref}, {"out": (z(ref), None)}
        wide = _sample(fmap.abs(), _wide_taps(taps, H, W))
        coef = (3 * (ix.abs() + iy.abs() + W + H) + 4)[..., None]
        return {"out": ref}, {"out": (z(ref), 4 * _sample(fmap.abs(), taps) + coef * wide)}
    g = d["gout"]
    ref, absg = _spread(g, taps, H, W), _spread(g.abs(), taps, H, W)
    n = _spread(torch.ones_like(g), [(y, x, (w != 0).double(), ok) for (y, x, w, ok) in taps], H, W)
    if c.mode == NEAREST:
        b = (n.sqrt() + 1) * absg
    else:
        b = (n.sqrt() + 4) * absg + (6 * (W + H) + 4) * _spread(g.abs(), _wide_taps(taps, H, W), H, W)
    if "framed" in op:
        ref, b = _frame_roll_back(ref, c), _frame_roll_back(b, c)
        return {"gmap": ref}, {"gmap": (z(ref), b)}
    if op == "point_bwd":
        p = pattern(c.B, c.H, c.W, c.C).double() if c.pat else z(ref)
        return {"gmap": p + ref}, {"gmap": (n * (p + absg), b)}
    return {"gmap": ref}, {"gmap": (z(ref), b)}


# ---------------------------------------------------------------------------------------------------------------- model
def work_items(c):
    """(cap, elements per work item) of the launcher of the case's (last) kernel: output element e belongs to item e // per."""
    v = {"v8": 8, "v4": 4, "s": 1}[channel_class(c)] if hasattr(c, "C") else 1
    if c.op == "point_fwd":
        return POINT_FWD_CAP, 1
    if c.op == "resample_bwd" and c.mode == BILINEAR:
        return FLAT_CAP, 1
    if c.op == "resample_bwd_sep":
        return FLAT_CAP, 4
    if c.op in ("psp_bwd", "stride_place"):
        return FLAT_CAP, 8 if c.dtype == "bf16" else 4
    if c.dtype == "f32" and c.op in ("avgpool_fwd", "avgpool_bwd"):
        return FLAT_CAP, 1
    return FLAT_CAP, v


def _skip_tail(c, out, fill=float("nan")):
    cap, per = work_items(c)
    flat = out.reshape(-1)
    flat[cap * per:] = fill
    return out


def _pool32(x, k):
    B, H, W, C = x.shape
    Ho, Wo = H // k, W // k
    w = x[:, :Ho * k, :Wo * k].reshape(B, Ho, k, Wo, k, C)
    return torch.flip(w, (2, 4)).sum((2, 4)) * (torch.tensor(1.0) / float(k * k))


def _unpool32(g, k, H, W):
    B, Ho, Wo, C = g.shape
    out = torch.zeros(B, H, W, C)
    out[:, :Ho * k, :Wo * k] = (g * (torch.tensor(1.0) / float(k * k)))[:, :, None, :, None, :].expand(B, Ho, k, Wo, k, C).reshape(B, Ho * k, Wo * k, C)
    return out


def _scatter_model(c, inp, taps, defect):
    """point_sample_bwd_kernel: one thread per (image, channel) walks the points in order, a read-modify-write in STORAGE per tap."""
    dt = torch_dtype(c)
    gmap = (pattern(c.B, c.H, c.W, c.C) if c.pat else torch.zeros(c.B, c.H, c.W, c.C)).to(dt)
    g = inp["gout"]
    live = torch.ones(c.B, c.C, dtype=torch.bool)
    if defect == "stride_tail":
        live = (torch.arange(c.B * c.C) < POINT_BWD_CAP).reshape(c.B, c.C)
    for s in range(c.S):
        for (y, x, w, ok) in taps:
            for b in range(c.B):
                if bool(ok[b, s]):
                    cur = gmap[b, y[b, s], x[b, s]].float()
                    new = (g[b, s] * w[b, s]) if defect == "collision_lost" else cur + g[b, s] * w[b, s]
                    gmap[b, y[b, s], x[b, s]] = torch.where(live[b], new, cur).to(dt)
    return gmap


def model(c, inp, defect=None):
    """The outputs of the case as the kernels compute them (see the module docstring); defect: one of DEFECTS, or None."""
    dt = torch_dtype(c)
    f = {k: v.float() for k, v in inp.items()}
    op = c.op
    tail = defect == "stride_tail"
    if op.startswith("resample"):
        ay, ax = axis32(c.Hs, c.Ho, c.mode, defect), axis32(c.Ws, c.Wo, c.mode, defect)
        if op == "resample_fwd":
            y = ay.fwd(ax.fwd(f["x"], 2), 1).to(dt)
            if defect == "pitch_as_c" and c.ld:                  # the pixel pitch taken as C: pixel p lands at p * C of the wide map
                wide = torch.full((c.B * c.Ho * c.Wo * c.ld,), float("nan")).to(dt)
                flat = y.reshape(-1, c.C)
                pos = (torch.arange(flat.shape[0]) * c.C + c.off)[:, None] + torch.arange(c.C)[None, :]
                wide[pos.reshape(-1)] = flat.reshape(-1)
                y = wide.reshape(c.B, c.Ho, c.Wo, c.ld)[..., c.off:c.off + c.C].clone()
            return {"y": _skip_tail(c, y) if tail else y}
        if defect == "footprint_short":
            ay, ax = ay.drop_last_output(), ax.drop_last_output()
        gx = ay.bwd(ax.bwd(f["gy"], 2), 1)
        if getattr(c, "gate", 0) and defect != "gate_dropped":
            r = f["gate"]
            gx = torch.where(r > 0, gx, torch.zeros_like(gx)) if c.gate == ACT_RELU else gx * torch.where(r > 0, torch.ones_like(r), r + 1.0)
        gx = gx.to(dt)
        return {"gx": _skip_tail(c, gx) if tail else gx}
    if op == "avgpool_fwd":
        y = _pool32(f["x"], c.k).to(dt)
        return {"y": _skip_tail(c, y) if tail else y}
    if op == "avgpool_bwd":
        inv = torch.tensor(1.0) / float(c.k * c.k)
        oy, ox = torch.arange(c.H) // c.k, torch.arange(c.W) // c.k
        Ho, Wo = c.H // c.k, c.W // c.k
        gx = f["gy"][:, oy.clamp_max(Ho - 1)][:, :, ox.clamp_max(Wo - 1)] * inv
        if defect != "pool_remainder":
            gx = gx * ((oy < Ho)[:, None] & (ox < Wo)[None, :])[None, :, :, None]
        gx = gx.to(dt)
        return {"gx": _skip_tail(c, gx) if tail else gx}
    if op == "psp_fwd":
        out = {"p%d" % k: _pool32(f["x"], k).to(dt) for k in (16, 8, 4, 2)}
        if defect == "psp_partial_block":                        # a block that overhangs the map also writes its (partial) 16-pool
            H16, W16 = c.H // 16, c.W // 16
            xp = F.pad(f["x"], (0, 0, 0, -c.W % 16, 0, -c.H % 16))
            full = _pool32(xp, 16)
            flat = out["p16"].reshape(-1, c.C)
            for b in range(c.B):
                for by in range(full.shape[1]):
                    for bx in range(full.shape[2]):
                        pix = (b * H16 + by) * W16 + bx
                        if (by >= H16 or bx >= W16) and pix < flat.shape[0]:
                            flat[pix] = full[b, by, bx].to(dt)
        return out
    if op == "psp_bwd":
        acc = f["gpass"].clone() if "gpass" in f else torch.zeros(c.B, c.H, c.W, c.C)
        for k in (2, 4, 8, 16):
            if "g%d" % k in f:
                acc = acc + _unpool32(f["g%d" % k], k, c.H, c.W)
        gx = acc.to(dt)
        return {"gx": _skip_tail(c, gx) if tail else gx}
    if op == "stride_place":
        out = f["residual"].clone() if "residual" in f else torch.zeros(c.B, c.H, c.W, c.C)
        if defect == "stride_live_guard":                        # every pixel of the stride grid reads src, past its last row / column too
            ys, xs = torch.arange(0, c.H, c.s), torch.arange(0, c.W, c.s)
            out[:, ys[:, None], xs[None, :]] += f["src"][:, (ys // c.s).clamp_max(c.Ho - 1)][:, :, (xs // c.s).clamp_max(c.Wo - 1)]
        else:
            out[:, 0:c.Ho * c.s:c.s, 0:c.Wo * c.s:c.s] += f["src"]
        out = out.to(dt)
        return {"dst": _skip_tail(c, out) if tail else out}
    if op == "taps_collapse":
        return {"wk": _collapse(f["w"]).to(dt)}
    if op == "taps_fold":
        return {"dw": pattern(c.Cout, 3, 3, c.Cin) + _fold(f["D"])}
    # ---- point sample
    H, W = (c.Hf, c.Wf) if "framed" in op else (c.H, c.W)
    taps, _, _ = _point_taps(f["coords"], H, W, c.mode, torch.float32, defect)
    if "framed" in op:                                           # frame pixel -> map pixel, as frame_pixel of csrc/pointsample.hip
        (y, x, w, ok) = taps[0]
        ym, xm = y + c.shift, x + c.shift
        if defect != "frame_no_wrap":
            ym, xm = torch.where(ym >= c.Hf, ym - c.Hf, ym), torch.where(xm >= c.Wf, xm - c.Wf, xm)
        taps = [(ym, xm, w, ok & (ym >= 0) & (ym < c.H) & (xm >= 0) & (xm < c.W))]
    if op in ("point_fwd", "point_framed_fwd"):
        out = _sample(f["map"], taps)
        return {"out": _skip_tail(c, out) if tail else out}
    if op == "point_bwd":
        return {"gmap": _scatter_model(c, inp, taps, defect)}
    return {"gmap": _spread(f["gout"], taps, c.H, c.W, accumulate=defect != "collision_lost").to(dt)}


# ------------------------------------------------------------------------------------------------------------ constants
AXES = {"y": ("image", "row", "column", "channel"), "gx": ("image", "row", "column", "channel"), "dst": ("image", "row", "column", "channel"),
        "gmap": ("image", "row", "column", "channel"), "p": ("image", "row", "column", "channel"), "out": ("image", "point", "channel"),
        "wk": ("cin", "t", "s", "cout"), "dw": ("cout", "kh", "kw", "cin")}


def key_of(c, name):
    return (operation(c), name.rstrip("0123456789"), c.dtype)


def check(c, got, inp, what=None, constants=None):
    """Every element of every output of the case against its bound; -> {output: worst ratio}.  The message names the first wrong flat index."""
    ref, cond = reference(c, inp)
    assert set(got) == set(ref), (sorted(got), sorted(ref))
    constants = C if constants is None else constants
    worst = {}
    for name in sorted(ref):
        label = "%s %s" % (what or c.text, name)
        g = got[name].detach().cpu()
        assert tuple(g.shape) == tuple(ref[name].shape), (label, tuple(g.shape), tuple(ref[name].shape))
        if exact_kind(c):
            same = g == ref[name].to(g.dtype)
            if not bool(same.all()):
                first = int(torch.nonzero(~same.reshape(-1))[0])
                raise AssertionError("%s: not a bit-exact copy: %d of %d elements differ, the first at flat index %d" % (label, int((~same).sum()), same.numel(), first))
        r = ratio(g, ref[name], cond[name], out_unit(c))
        bad = r > constants[key_of(c, name)]
        if bool(bad.any()):
            first = int(torch.nonzero(bad.reshape(-1))[0])
            try:
                assert_elementwise(g, ref[name], cond[name], constants[key_of(c, name)], AXES[name.rstrip("0123456789")], u=out_unit(c), what=label)
            except AssertionError as e:
                raise AssertionError("%s; first wrong flat index %d of %d" % (e, first, r.numel())) from None
        worst[name] = float(r.max()) if r.numel() else 0.0
    return worst


def measure_c(table=None):
    """{(operation, output, type): largest model ratio} over cases()."""
    worst = {}
    for c in (cases() if table is None else table):
        inp = inputs(c)
        got = model(c, inp)
        ref, cond = reference(c, inp)
        for name in ref:
            k = key_of(c, name)
            worst[k] = max(worst.get(k, 0.0), float(ratio(got[name], ref[name], cond[name], out_unit(c)).max()))
    return worst


def format_table(worst):
    lines = ["    operation                   output   type   model max   C", "    -------------------------   ------   ----   ---------   ----"]
    for (op, out, dt), v in sorted(worst.items()):
        lines.append("    %-25s   %-6s   %-4s   %9.3f   %4.1f" % (op, out, dt, v, c_of(v)))
    return "\n".join(lines)


# C[(operation, output, type)]: twice the largest model ratio over cases(), one decimal up; the module docstring shows
# format_table(MEASURED) (tests/test_spatial_ref.py checks both)
MEASURED = {
    ("avgpool_bwd", "gx", "bf16"): 1.761,
    ("avgpool_bwd", "gx", "f32"): 0.402,
    ("avgpool_fwd", "y", "bf16"): 1.992,
    ("avgpool_fwd", "y", "f32"): 0.293,
    ("point_bwd_bilinear", "gmap", "bf16"): 1.241,
    ("point_bwd_bilinear", "gmap", "f32"): 0.157,
    ("point_bwd_gather_bilinear", "gmap", "bf16"): 1.942,
    ("point_bwd_gather_bilinear", "gmap", "f32"): 0.058,
    ("point_bwd_gather_nearest", "gmap", "bf16"): 1.981,
    ("point_bwd_gather_nearest", "gmap", "f32"): 0.376,
    ("point_bwd_nearest", "gmap", "bf16"): 1.061,
    ("point_bwd_nearest", "gmap", "f32"): 0.462,
    ("point_framed_bwd", "gmap", "bf16"): 1.986,
    ("point_framed_bwd", "gmap", "f32"): 0.417,
    ("point_framed_fwd", "out", "bf16"): 0.000,
    ("point_framed_fwd", "out", "f32"): 0.000,
    ("point_fwd_bilinear", "out", "bf16"): 0.131,
    ("point_fwd_bilinear", "out", "f32"): 0.109,
    ("point_fwd_nearest", "out", "bf16"): 0.000,
    ("point_fwd_nearest", "out", "f32"): 0.000,
    ("psp_bwd", "gx", "bf16"): 1.992,
    ("psp_bwd", "gx", "f32"): 0.511,
    ("psp_fwd", "p", "bf16"): 1.992,
    ("psp_fwd", "p", "f32"): 0.370,
    ("resample_bwd_bilinear", "gx", "bf16"): 1.937,
    ("resample_bwd_bilinear", "gx", "f32"): 0.206,
    ("resample_bwd_nearest", "gx", "bf16"): 1.992,
    ("resample_bwd_nearest", "gx", "f32"): 0.426,
    ("resample_bwd_sep_bilinear", "gx", "bf16"): 1.967,
    ("resample_bwd_sep_bilinear", "gx", "f32"): 0.235,
    ("resample_bwd_sep_nearest", "gx", "bf16"): 1.992,
    ("resample_bwd_sep_nearest", "gx", "f32"): 0.409,
    ("resample_fwd_bilinear", "y", "bf16"): 1.991,
    ("resample_fwd_bilinear", "y", "f32"): 0.229,
    ("resample_fwd_nearest", "y", "bf16"): 0.000,
    ("resample_fwd_nearest", "y", "f32"): 0.000,
    ("stride_place", "dst", "bf16"): 1.992,
    ("stride_place", "dst", "f32"): 0.996,
    ("taps_collapse", "wk", "bf16"): 1.989,
    ("taps_collapse", "wk", "f32"): 0.691,
    ("taps_fold", "dw", "f32"): 0.511,
}
C = {k: c_of(v) for k, v in MEASURED.items()}
__doc__ = __doc__.replace("@TABLE@", format_table(MEASURED))
