"""Exact reference of the level masks and counts, fp64 reference, error bound and fp32 model of the sine position embedding
(csrc/posenc.hip, gwd_pos_sine; CPU only, plain module; the instrument is tests/attn_ref.py's).

A case is (B, H, W, h, w, mask kind, F, normalize, counts kind).  With a mask kind the call is the first stage (mask_full -> level
mask + counts) followed, when F > 0, by the second (counts -> embedding); with a counts kind it is an emit-only call (mask_full =
NULL) on counts the test wrote.  Mask kinds (True = padded): ``none``; ``ragged`` (right / bottom padding); ``batch3`` (an unpadded
image, a ragged one, a fully padded one); ``holes`` (30 % random padding plus one source row and one source column, both read by the
level, padded throughout).  Counts kinds: ``scan`` (counts of a random 5 x 7 mask) and ``max`` (32767 in a 1 x 1 level).

* ``launch(c)``: the launch arithmetic restated: the trips of the scan loop ceil((w + h) / 1024), the LDS branch h w <= 32768, the
  emit grid min(4096, ceil(total / 256)) and its trips, and whether floorf(i * (float)H / h) differs from i * H // h anywhere.
* ``reference(c, inp)`` -> {"mask", "counts", "out", "arg"}: the level mask is F.interpolate(mask[None].float(), size=(h, w)).to(bool)
  on the CPU (ATen's nearest: min(floorf(i * (float)H / h), H - 1)), the counts a numpy cumulative sum of the un-masked pixels - both
  compared for EQUALITY.  The embedding is fp64 from the stored int16 counts and the stored fp32 dim_t:
      v = count,  normalize: v = count / (last + 1e-6) * 2 pi,   arg = v / dim_t[k],   out = sin(arg) (k even) or cos(arg) (k odd)
      |got - ref| <= C u_f32 (|ref| + |arg|)
  |arg| is the condition of the sine: an argument error of a few u |arg| moves it by as much.  The kernel's argument carries the
  roundings of last + 1e-6f (for last >= 32 the sum returns last: the 1e-6 is absorbed, a relative 1e-6 / last <= 0.53 u), of the
  quotient, of the product with fp32's 2 pi (which is 0.47 u from 2 pi) and of the division by dim_t - all terms of the form
  u |arg|.  A last count of 0 makes the count 0 as well: sin 0 = 0 and cos 0 = 1 exactly: ``check`` demands equality wherever the
  argument is 0 (the bound alone would leave C u around the 1).
* ``model(c, inp, defect=None)``: the kernel's rounding sequence in fp32 - v / (last + 1e-6f) * 2pi_f32 / dim_t - followed by an fp64
  sine or cosine rounded to fp32.  Defects: ``integer_nearest`` (i * H // h), ``masked_counted`` (padded pixels counted),
  ``scan_tail_skipped`` (the scans of threads 1024 on are not run: their counts keep the sentinel), ``emit_tail_skipped`` (the
  elements beyond the first grid-stride trip are not written), ``parity_from_c`` (sin / cos chosen by the channel c instead of
  k = c - F: the x half flips when F is odd), ``x_by_column_last`` (the x count normalised by the last y count of its column),
  ``two_pi_before_division`` (the factor 2 pi applied in front of the division's branch: an unnormalised level is scaled too).

The constant.  ``measure_c()``: largest |model - ref| / bound over the case list; C twice that, one decimal up (the factor 2 covers
the device's sinf / cosf).  CPU, 2026-10:

@TABLE@

A kernel that needs more than its C has a defect or the bound lacks a term: neither is repaired by raising C.
"""
import math
import types
import zlib

import numpy as np
import torch

from tests.attn_ref import FLOOR, U_F32, assert_elementwise, ratio        # noqa: F401  (the instrument)
from tests.conv_ref import c_of

DEFECTS = ("integer_nearest", "masked_counted", "scan_tail_skipped", "emit_tail_skipped", "parity_from_c", "x_by_column_last",
           "two_pi_before_division")
SCAN_THREADS, LDS_PIXELS, EMIT_THREADS, EMIT_MAX_BLOCKS, MAX_SIDE = 1024, 32768, 256, 4096, 32767        # csrc/posenc.hip
TEMPERATURE = 10000.0
COUNT_SENTINEL, MASK_SENTINEL = -12345, 0x5A
AXES = ("image", "row", "column", "channel")
KEY = ("pos_sine", "out", "f32")


def nearest_index(n_out, n_in, integer=False):
    """The source index of every level index: ATen's nearest (fp32 scale, fp32 product, floor, clamp), or the integer formula."""
    i = np.arange(n_out)
    if integer:
        return np.minimum(i * n_in // n_out, n_in - 1)
    scale = np.float32(n_in) / np.float32(n_out)
    return np.minimum(np.floor(i.astype(np.float32) * scale).astype(np.int64), n_in - 1)


def launch(c):
    total = c.B * c.h * c.w * 2 * c.F
    blocks = min(EMIT_MAX_BLOCKS, (total + EMIT_THREADS - 1) // EMIT_THREADS)
    differs = c.mask is not None and (bool((nearest_index(c.h, c.H) != nearest_index(c.h, c.H, True)).any()) or
                                      bool((nearest_index(c.w, c.W) != nearest_index(c.w, c.W, True)).any()))
    return types.SimpleNamespace(scan_trips=(c.w + c.h + SCAN_THREADS - 1) // SCAN_THREADS, in_lds=c.h * c.w <= LDS_PIXELS,
                                 pixel_trips=(c.h * c.w + SCAN_THREADS - 1) // SCAN_THREADS, total=total, blocks=blocks,
                                 emit_trips=(total + blocks * EMIT_THREADS - 1) // (blocks * EMIT_THREADS) if total else 0,
                                 tail=total > EMIT_MAX_BLOCKS * EMIT_THREADS, index_differs=differs)


def _case(B, H, W, h, w, mask, F=0, normalize=1, counts=None):
    c = types.SimpleNamespace(B=B, H=H, W=W, h=h, w=w, mask=mask, F=F, normalize=normalize, counts=counts)
    c.text = "pos_sine B=%d %dx%d->%dx%d mask=%s counts=%s F=%d normalize=%d" % (B, H, W, h, w, mask, counts, F, normalize)
    c.id = c.text.replace(" ", "-").replace(">", "")
    return c


def cases():
    out = [_case(1, 9, 13, 9, 13, "ragged"), _case(1, 26, 39, 22, 33, "holes"), _case(1, 62, 26, 14, 22, "holes"), _case(1, 3, 5, 7, 9, "ragged"),
           _case(1, 3, 4, 1, 1, "none"), _case(1, 1, 1, 1, 1, "none", F=1), _case(1, 130, 300, 128, 256, "ragged"), _case(1, 150, 260, 129, 255, "ragged"),
           _case(1, 5, 1200, 3, 1100, "holes"), _case(1, 1200, 5, 1100, 3, "holes"), _case(3, 20, 30, 10, 15, "batch3"), _case(3, 26, 39, 22, 33, "batch3")]
    out += [_case(3, 20, 30, 10, 15, "batch3", F=F, normalize=n) for F in (1, 3, 16, 64) for n in (0, 1)]
    out += [_case(1, 26, 39, 22, 33, "holes", F=F, normalize=n) for F in (3, 16) for n in (0, 1)]
    out += [_case(1, 5, 1200, 3, 1100, "none", F=3, normalize=0), _case(1, 1200, 5, 1100, 3, "none", F=3, normalize=0),
            _case(1, 5, 1200, 3, 1100, "ragged", F=1, normalize=1)]
    out += [_case(2, 0, 0, 5, 7, None, F=3, normalize=n, counts="scan") for n in (0, 1)]
    out += [_case(1, 0, 0, 1, 1, None, F=1, normalize=n, counts="max") for n in (0, 1)]
    out += [_case(1, 65, 127, 65, 127, "ragged", F=64, normalize=1)]
    return out


def rejected():
    """(name, (B, h, w, F, with_mask), return code): all returned before a launch."""
    return [("h=32768", (1, 32768, 1, 1, True), -7), ("w=32768_emit_only", (1, 1, 32768, 1, False), -7),
            ("total=2^31", (1, 32767, 32767, 2, False), -7), ("total=2^31_B", (2, 16384, 16384, 2, False), -7), ("F=0", (1, 4, 4, 0, False), -1)]


def dim_t_of(F):
    """gw_depth_amd/ops.py: temperature ** (2 (k // 2) / F) in fp32."""
    t = torch.arange(F, dtype=torch.float32)
    return TEMPERATURE ** (2 * torch.div(t, 2, rounding_mode="floor") / F)


# ---------------------------------------------------------------------------------------------------------------- inputs
def _counts_of(level_mask, counted=False):
    free = np.ones_like(level_mask, np.int64) if counted else (~level_mask).astype(np.int64)
    return np.stack([np.cumsum(free, 1), np.cumsum(free, 2)], -1).astype(np.int16)               # (B, h, w, 2): y, x


def inputs(c):
    rng = np.random.default_rng(zlib.crc32(c.text.encode()))
    inp = {"dim_t": dim_t_of(c.F) if c.F else None}
    if c.mask is None:
        if c.counts == "max":
            cnt = np.full((c.B, c.h, c.w, 2), 32767, np.int16)
        else:
            cnt = _counts_of(rng.random((c.B, c.h, c.w)) < 0.3)
        inp["counts"] = torch.from_numpy(cnt)
        return inp
    m = np.zeros((c.B, c.H, c.W), bool)
    for b in range(c.B):
        kind = c.mask if c.mask != "batch3" else ("none", "ragged", "all")[b % 3]
        if kind == "ragged":
            m[b, c.H - c.H // 4:, :] = True
            m[b, :, c.W - c.W // 3:] = True
        elif kind == "all":
            m[b] = True
        elif kind == "holes":
            m[b] = rng.random((c.H, c.W)) < 0.3
            m[b, nearest_index(c.h, c.H)[c.h // 2], :] = True
            m[b, :, nearest_index(c.w, c.W)[c.w // 3]] = True
    inp["mask"] = torch.from_numpy(m)
    return inp


# ------------------------------------------------------------------------------------------------------------- reference
def _embed64(c, counts, dim_t):
    """counts (B, h, w, 2) int16 -> (out, |arg|) fp64, (B, h, w, 2F)."""
    cnt = counts.double()
    y, x = cnt[..., 0], cnt[..., 1]
    if c.normalize:
        y = y / (y[:, -1:, :] + 1e-6) * (2 * math.pi)
        x = x / (x[:, :, -1:] + 1e-6) * (2 * math.pi)
    d = dim_t.double()
    arg = torch.cat([y[..., None] / d, x[..., None] / d], -1)
    odd = (torch.arange(c.F) % 2 == 1).repeat(2)
    return torch.where(odd, torch.cos(arg), torch.sin(arg)), arg.abs()


def reference(c, inp):
    ref = {}
    if c.mask is not None:
        lvl = torch.nn.functional.interpolate(inp["mask"][None].float(), size=(c.h, c.w)).to(torch.bool)[0]
        ref["mask"] = lvl.to(torch.uint8)
        ref["counts"] = torch.from_numpy(_counts_of(lvl.numpy()))
    counts = ref["counts"] if c.mask is not None else inp["counts"]
    if c.F:
        ref["out"], ref["arg"] = _embed64(c, counts, inp["dim_t"])
        assert tuple(ref["out"].shape) == (c.B, c.h, c.w, 2 * c.F) and bool(torch.isfinite(ref["out"]).all())
    return ref


# ----------------------------------------------------------------------------------------------------------------- model
def model(c, inp, defect=None):
    assert defect is None or defect in DEFECTS
    got = {}
    if c.mask is not None:
        yi, xj = nearest_index(c.h, c.H, defect == "integer_nearest"), nearest_index(c.w, c.W, defect == "integer_nearest")
        lvl = inp["mask"].numpy()[:, yi][:, :, xj]
        cnt = _counts_of(lvl, counted=defect == "masked_counted")
        if defect == "scan_tail_skipped":                                   # thread t < w scans column t, thread w + i row i
            cnt[:, :, SCAN_THREADS:, 0] = COUNT_SENTINEL
            cnt[:, max(SCAN_THREADS - c.w, 0):, :, 1] = COUNT_SENTINEL
        got["mask"], got["counts"] = torch.from_numpy(lvl.astype(np.uint8)), torch.from_numpy(cnt)
    counts = got["counts"] if c.mask is not None else inp["counts"]
    if c.F:
        f = counts.float()
        y, x = f[..., 0], f[..., 1]
        eps, two_pi = torch.tensor(1e-6, dtype=torch.float32), torch.tensor(6.283185307179586, dtype=torch.float32)
        if c.normalize:
            last_x = f[:, -1:, :, 0] if defect == "x_by_column_last" else x[:, :, -1:]
            y = y / (y[:, -1:, :] + eps) * two_pi
            x = x / (last_x + eps) * two_pi
        elif defect == "two_pi_before_division":
            y, x = y * two_pi, x * two_pi
        arg = torch.cat([y[..., None] / inp["dim_t"], x[..., None] / inp["dim_t"]], -1)
        assert arg.dtype == torch.float32
        k = torch.arange(2 * c.F) if defect == "parity_from_c" else torch.arange(c.F).repeat(2)
        out = torch.where(k % 2 == 1, torch.cos(arg.double()), torch.sin(arg.double())).float()
        if defect == "emit_tail_skipped":
            out.view(-1)[EMIT_MAX_BLOCKS * EMIT_THREADS:] = float("nan")
        got["out"] = out
    return got


# ------------------------------------------------------------------------------------------------------------ constants
def check(c, got, inp, ref=None, what=None):
    """Equality of the mask and the counts, exact 0 / 1 at a zero argument, the bound for the rest of the embedding -> worst ratio (0
    without an embedding)."""
    ref = reference(c, inp) if ref is None else ref
    what = what or c.text
    if c.mask is not None:
        bad = int((got["mask"] != ref["mask"]).sum())
        assert bad == 0, "%s: %d level mask bytes differ" % (what, bad)
        bad = int((got["counts"] != ref["counts"]).sum())
        assert bad == 0, "%s: %d counts differ" % (what, bad)
    if not c.F:
        return 0.0
    zero = ref["arg"] == 0                                                  # a count of 0 (every count whose last count is 0): sin 0, cos 0
    bad = int((got["out"].double()[zero] != ref["out"][zero]).sum())
    assert bad == 0, "%s: %d elements with a zero argument are not exactly 0 (sin) / 1 (cos)" % (what, bad)
    return assert_elementwise(got["out"], ref["out"], (ref["arg"], None), C[KEY], AXES, u=U_F32, what=what)


def measure_c(case_list=None):
    worst = 0.0
    for c in (cases() if case_list is None else case_list):
        if c.F:
            inp = inputs(c)
            ref = reference(c, inp)
            worst = max(worst, float(ratio(model(c, inp)["out"], ref["out"], (ref["arg"], None), U_F32).max()))
    return {KEY: worst}


def format_table(worst):
    lines = ["    operation   output   type   model max   C", "    ---------   ------   ----   ---------   ----"]
    for (op, out, dt), v in sorted(worst.items()):
        lines.append("    %-9s   %-6s   %-4s   %9.3f   %4.1f" % (op, out, dt, v, c_of(v)))
    return "\n".join(lines)


MEASURED = {
    ("pos_sine", "out", "f32"): 2.247,
}
C = {k: c_of(v) for k, v in MEASURED.items()}
__doc__ = __doc__.replace("@TABLE@", format_table(MEASURED))
