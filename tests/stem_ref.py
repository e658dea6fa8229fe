"""fp64 reference, error bound and fp32 model of the fused stem (csrc/stem.hip, gwd_stem_pack / gwd_stem_forward: conv 7x7 / 2 / 3
(3 -> 64) + shift + ReLU + max-pool 3x3 / 2 / 1 in one kernel, bf16; CPU only, plain module; the instrument is tests/attn_ref.py's).

A case is (B, H, W, shift kind, scale kind).  ``inputs(c)`` draws x (B, H, W, 3) in bf16 - a smooth function of (b, y, x, c) plus
noise, so that a tap shifted by one pixel moves a value by far more than the bound -, w fp32 (64, 7, 7, 3), scale fp32 (64) or None,
shift fp32 (64), None, or with -1000 on the channels NEG (those outputs are exactly 0 everywhere).

* ``pack_reference(w, scale)``: the 14 * 2 * 64 * 8 packed values.  Index i = ((s * 2 + mt) * 64 + lane) * 8 + j holds channel
  co = 32 mt + lane % 32, kh = s >> 1, kw = 4 (s & 1) + 2 (lane >> 5) + (j >> 2), c = j & 3: the bf16 rounding of the single fp32 product
  w scale (of w without a scale), and exactly 0 at kw = 7 or c = 3.  The bound is zero: every value is compared for equality.
  ``unpack(packed)`` is the inverse -> (64, 7, 8, 4) fp64.
* ``reference(c, inp, packed)`` -> (y, cond), fp64: the convolution over the bf16 x and the unpacked weights THE KERNEL RECEIVED, as
  49 shifted products summed in fp64 (no F.conv2d), plus the fp32 shift, ReLU, the 3x3 / 2 / 1 maximum with -inf padding.
      |got - y| <= C u_bf16 (|y| + (2^-24 / u_bf16) A),   A = max over the window's in-range conv positions of sum |w x| + |shift|
  (the products of two bf16 are exact in fp32, the accumulation and the shift are fp32; the error of a maximum is at most the
  largest error of its arguments; one rounding to bf16 at the store).
* ``model(c, inp, defect=None)`` -> (packed, y): the pack as above and the kernel's arithmetic in fp32 with the taps summed last to
  first, workgroup tiles of 8 x 15 pooled pixels.  Defects: ``pad_neighbour`` (the pool's padding column / row takes the conv value
  computed beyond the map's edge - what a neighbouring tile's column would be - instead of nothing), ``seam_drop`` (the first
  pooled column of every tile but the first loses its left conv column), ``kw7`` (the packed kw = 7 slot repeats kw = 6),
  ``shift_after`` (the shift added after the pool's ReLU).

The constants.  ``measure_c()``: largest |model - ref| / bound over the case list; C twice that, one decimal up.  CPU, 2026-10:

@TABLE@

A kernel that needs more than its C has a defect or the bound lacks a term: neither is repaired by raising C.
"""
import types
import zlib

import torch

from tests.attn_ref import FLOOR, U_BF16, U_F32, assert_elementwise, ratio        # noqa: F401  (the instrument)
from tests.conv_ref import c_of

DEFECTS = ("pad_neighbour", "seam_drop", "kw7", "shift_after")
PXS, PYS, MAX_GRID, PACKED = 15, 8, 512, 14 * 2 * 64 * 8         # csrc/stem.hip
NEG = (3, 40, 63)                                               # channels whose shift is -1000 in the "neg" cases
AXES = ("image", "row", "column", "channel")


def launch(c):
    """The launch arithmetic of gwd_stem_forward."""
    Hc, Wc = (c.H - 1) // 2 + 1, (c.W - 1) // 2 + 1
    Hp, Wp = (Hc - 1) // 2 + 1, (Wc - 1) // 2 + 1
    ty, tx = (Hp + PYS - 1) // PYS, (Wp + PXS - 1) // PXS
    ntiles = c.B * ty * tx
    rounds = (ntiles + MAX_GRID - 1) // MAX_GRID
    return types.SimpleNamespace(Hc=Hc, Wc=Wc, Hp=Hp, Wp=Wp, tiles_y=ty, tiles_x=tx, ntiles=ntiles, rounds=rounds,
                                 grid=(ntiles + rounds - 1) // rounds)


def _case(B, H, W, shift="rand", scale="rand"):
    c = types.SimpleNamespace(B=B, H=H, W=W, shift=shift, scale=scale)
    c.text = "stem B=%d H=%d W=%d shift=%s scale=%s" % (B, H, W, shift, scale)
    c.id = c.text.replace(" ", "-")
    return c


def cases():
    out = [_case(2, h, w) for h in (1, 2, 3, 4) for w in (1, 2, 3, 4)]
    # Wp = 15 | 16 | 30 | 31 (W = 57..60 | 61 | 117..120 | 121..124), Hp = 8 | 9 | 16 | 17 (H = 29..32 | 33 | 61..64 | 65..68); odd and even Hc, Wc
    out += [_case(1, 31, 59), _case(1, 30, 58), _case(2, 33, 61), _case(1, 36, 64), _case(1, 63, 119), _case(1, 62, 118),
            _case(1, 65, 121), _case(2, 68, 124), _case(1, 29, 124), _case(1, 67, 57)]
    out += [_case(3, 97, 131), _case(513, 5, 7)]
    out += [_case(2, 33, 61, "none"), _case(2, 33, 61, "neg"), _case(2, 33, 61, "rand", "none"), _case(1, 4, 3, "none", "none")]
    return out


# ---------------------------------------------------------------------------------------------------------------- inputs
def _gen(c):
    g = torch.Generator()
    g.manual_seed(zlib.crc32(c.text.encode()))
    return g


def inputs(c):
    g = _gen(c)
    b = torch.arange(c.B, dtype=torch.float64)[:, None, None, None]
    y = torch.arange(c.H, dtype=torch.float64)[None, :, None, None]
    x = torch.arange(c.W, dtype=torch.float64)[None, None, :, None]
    ch = torch.arange(3, dtype=torch.float64)[None, None, None, :]
    smooth = torch.sin(0.9 * y + 0.37 * b + 1.3 * ch) * torch.cos(0.7 * x - 0.21 * b + 0.5 * ch) + 0.3 * torch.sin(2.1 * x + 1.7 * y)
    xs = (smooth + 0.1 * torch.randn((c.B, c.H, c.W, 3), generator=g, dtype=torch.float64)).to(torch.bfloat16)
    w = (torch.randn((64, 7, 7, 3), generator=g, dtype=torch.float64) * 0.15).float()
    scale = None if c.scale == "none" else (0.5 + torch.rand(64, generator=g, dtype=torch.float64)).float()
    shift = None if c.shift == "none" else (0.5 * torch.randn(64, generator=g, dtype=torch.float64)).float()
    if c.shift == "neg":
        shift[list(NEG)] = -1000.0
    return {"x": xs, "w": w, "scale": scale, "shift": shift}


# ------------------------------------------------------------------------------------------------------------------ pack
def _pack_index():
    i = torch.arange(PACKED)
    j, lane, mt, s = i & 7, (i >> 3) & 63, (i >> 9) & 1, i >> 10
    return 32 * mt + (lane & 31), s >> 1, 4 * (s & 1) + 2 * (lane >> 5) + (j >> 2), j & 3


def pack_reference(w, scale, defect=None):
    """-> bf16 (PACKED,)."""
    co, kh, kw, ch = _pack_index()
    v = w if scale is None else w * scale[:, None, None, None]          # ONE fp32 product
    if defect == "kw7":
        kw = kw.clamp_max(6)
    ok = (kw < 7) & (ch < 3)
    out = torch.zeros(PACKED, dtype=torch.float32)
    out[ok] = v[co[ok], kh[ok], kw[ok], ch[ok]]
    return out.to(torch.bfloat16)


def unpack(packed):
    """bf16 (PACKED,) -> fp64 (64, 7, 8, 4)."""
    co, kh, kw, ch = _pack_index()
    out = torch.zeros(64, 7, 8, 4, dtype=torch.float64)
    out[co, kh, kw, ch] = packed.double().cpu()
    return out


# ------------------------------------------------------------------------------------------------------------- reference
def _conv_ext(x, wt, L, dtype, absolute=False, kws=7, chs=3):
    """Conv values at positions -1 .. Hc, -1 .. Wc -> (B, Hc + 2, Wc + 2, 64); x zero-padded, the taps summed last to first."""
    B, H, W, _ = x.shape
    xp = torch.zeros(B, H + 16, W + 16, 4, dtype=dtype)
    xp[:, 8:8 + H, 8:8 + W, :3] = x.to(dtype)
    acc = torch.zeros(B, L.Hc + 2, L.Wc + 2, 64, dtype=dtype)
    for kh in range(6, -1, -1):
        for kw in range(kws - 1, -1, -1):
            tap = xp[:, 3 + kh:3 + kh + 2 * (L.Hc + 2):2, 3 + kw:3 + kw + 2 * (L.Wc + 2):2, :chs]
            wk = wt[:, kh, kw, :chs].to(dtype)
            if absolute:
                tap, wk = tap.abs(), wk.abs()
            acc = acc + tap @ wk.t()
    return acc


def _inside(L):
    """(Hc + 2, Wc + 2) mask of the in-range conv positions of the extended map."""
    m = torch.zeros(L.Hc + 2, L.Wc + 2, dtype=torch.bool)
    m[1:-1, 1:-1] = True
    return m


def _pool(v, L):
    """3x3 / 2 / 1 maximum over the extended map: pooled (py, px) covers extended rows 2 py .. 2 py + 2."""
    out = None
    for dy in range(3):
        for dx in range(3):
            t = v[:, dy:dy + 2 * L.Hp:2, dx:dx + 2 * L.Wp:2]
            out = t if out is None else torch.maximum(out, t)
    return out


def reference(c, inp, packed):
    L = launch(c)
    wt = unpack(packed)
    x = inp["x"].double()
    shift = torch.zeros(64, dtype=torch.float64) if inp["shift"] is None else inp["shift"].double()
    inside = _inside(L)[None, :, :, None]
    conv = _conv_ext(x, wt, L, torch.float64)
    mag = _conv_ext(x, wt, L, torch.float64, absolute=True) + shift.abs()
    ninf = torch.full_like(conv, float("-inf"))
    y = _pool(torch.where(inside, (conv + shift).clamp_min(0.0), ninf), L)
    A = _pool(torch.where(inside, mag, torch.zeros_like(mag)), L)
    assert tuple(y.shape) == (c.B, L.Hp, L.Wp, 64) and bool(torch.isfinite(y).all())
    return y, (torch.zeros_like(y), A)


# ----------------------------------------------------------------------------------------------------------------- model
def model(c, inp, defect=None):
    assert defect is None or defect in DEFECTS
    L = launch(c)
    packed = pack_reference(inp["w"], inp["scale"], defect)
    wt = unpack(packed).float()
    shift = torch.zeros(64) if inp["shift"] is None else inp["shift"]
    conv = _conv_ext(inp["x"].float(), wt, L, torch.float32, kws=8 if defect == "kw7" else 7, chs=4)
    v = conv if defect == "shift_after" else conv + shift
    if defect != "pad_neighbour":
        v = torch.where(_inside(L)[None, :, :, None], v, torch.zeros_like(v))
    else:                                                    # the corners and what lies left of / above the map stay padding
        m = _inside(L)
        m[1:-1, -1] = True
        m[-1, 1:-1] = True
        v = torch.where(m[None, :, :, None], v, torch.zeros_like(v))
    v = v.clamp_min(0.0)
    if defect == "seam_drop":
        for px in range(PXS, L.Wp, PXS):
            v[:, :, 2 * px] = 0.0                            # extended column 2 px = conv column 2 px - 1
    y = _pool(v, L)
    if defect == "shift_after":
        y = y + shift
    return packed, y.to(torch.bfloat16)


# ------------------------------------------------------------------------------------------------------------ constants
KEY = ("stem_forward", "y", "bf16")


def check(c, got, inp, packed, what=None):
    ref, cond = reference(c, inp, packed)
    worst = assert_elementwise(got, ref, cond, C[KEY], AXES, u=U_BF16, what="%s y" % (what or c.text))
    if c.shift == "neg":
        assert bool((got[..., list(NEG)] == 0).all()), "%s: a channel shifted by -1000 is not exactly 0" % c.text
    return worst


def measure_c(case_list=None):
    worst = 0.0
    for c in (cases() if case_list is None else case_list):
        inp = inputs(c)
        packed, got = model(c, inp)
        ref, cond = reference(c, inp, packed)
        worst = max(worst, float(ratio(got, ref, cond, U_BF16).max()))
    return {KEY: worst}


def format_table(worst):
    lines = ["    operation      output   type   model max   C", "    ------------   ------   ----   ---------   ----"]
    for (op, out, dt), v in sorted(worst.items()):
        lines.append("    %-12s   %-6s   %-4s   %9.3f   %4.1f" % (op, out, dt, v, c_of(v)))
    return "\n".join(lines)


MEASURED = {
    ("stem_forward", "y", "bf16"): 1.992,
}
C = {k: c_of(v) for k, v in MEASURED.items()}
__doc__ = __doc__.replace("@TABLE@", format_table(MEASURED))
