"""fp64 reference, error bound and rounding model of the convolution kernels (CPU only, plain module; the instrument is the one of
tests/attn_ref.py: assert_elementwise, ratio, FLOOR and the unit round-offs come from there).

The calls are the lines of tests/golden/conv_witnesses.txt (tests/conv_witness.py parses them).  Every reference works on operands
that are ALREADY rounded to the storage type; the only error left between a kernel and its reference is the kernel's arithmetic.

* ``conv_ref64`` / ``wgrad_ref64`` - include/gwdepth.h's formulas in fp64 for chosen output rows (all Cout of each) / chosen
  (n, c) blocks of dw (all taps).  Gather (output pixel (oh, ow), tap (kh, kw) -> input pixel):
      CONV        ih = oh stride - pad + kh
      TRANSPOSED  ih = (oh + pad - kh) / stride where divisible and >= 0
      UPSAMPLED   vh = oh - pad + kh inside (Hv, Wv), ih = floor(vh Hi / Hv)
  a tap outside the image contributes nothing.  Epilogue, in this order:
      v = scale conv + shift (+ residual, unless there is a multiplier);   z = v;   a = act_scale act(v);
      with a multiplier  a = a mult + residual;   with a gate  a = a act'(.) of the gate (ReLU / ELU from the OUTPUT `gate`, GELU from
      the PRE-activation `gate`), last.
  ConvLn:  mu, var over the first ln_C channels of conv (biased, eps 1e-5), t = (conv - mu) rstd gamma + beta, y = act(t) + residual,
      columns >= ln_C exact zeros, z = conv, ln_mean = mu, ln_rstd = rstd.
  dw[n][tap][c] = scale[n] sum_m gy[m][n] x[gather(m, tap)][c].
* ``conv_cond`` - per output element a pair (A, B) for the bound  c u (|ref| + A + (2^-24 / u) B).  No forward kernel rounds
  anything to the storage type before the final store (accumulators, LayerNorm statistics and the whole epilogue are fp32), so A = 0
  there; B collects, in units of 2^-24, the fp32 errors (S = sum_k |x_k| |w_k|, K_len = KH KW Cin, L = max |act'| = 1, GELU 1.13):
      Bv = sqrt(K_len) |scale| S + |scale conv| + |shift| + |residual|                      (z: B = Bv)
      Ba = act_scale (L Bv + E) (+ |a| when act_scale is not 1: one more product),   E = 2 |act(v)| for ELU / GELU (expm1 / erf),
            + 2 |v| for GELU (the bf16 kernels' erf: 1.5e-7);  SIGMOID: L = 1/4, E = |act(v)| (3 + |v|) (expf of -v, the reciprocal)
      with a multiplier   By = |mult| Ba + |a mult| + |residual|,   else By = Ba
      with a gate factor f (a the value in front of it)   By = |f| By + e_f,  e_f = 0 (ReLU: f is 0 or 1), |a f| (ELU: gate + 1 rounds once),
            4 |a| (GELU: the fast erf's error in gelu' is ABSOLUTE, 1.5e-7 in erf = 1.3 x 2^-24 in the cdf, and stays when f crosses zero at -0.75)
  A closed ReLU gate has f = 0: the bound is zero and demands an exact zero.  ConvLn, e_c = Bc_c + mean_c' Bc_c' with
  Bc = sqrt(K_len) S + |conv| (the element's error and the mean's), d = conv - mu, q = rstd^2 mean_c |d_c| e_c (relative error of rstd):
      ln_mean: A = mean_c Bc_c   ln_rstd: A = rstd (q + 2)      (fp32 outputs, u = 2^-24)
      Bt = rstd |gamma| e_c + |d rstd gamma| (q + 4) + |beta|;   By = L Bt + E + |residual|;   zero (exact) in the padding columns
  Weight gradient (fp32 output, fp32 atomics; the sum runs over the M output pixels):  A = |scale| sqrt(M) sum_m |gy| |x|.
* ``conv_model`` / ``wgrad_model`` - the kernels' arithmetic in fp32 on the CPU with ONE rounding to the storage type, at the store
  (csrc/igemm.hip's epilogues keep everything else in fp32); the K reduction runs over 64- or 32-channel blocks in REVERSED order
  (the weight gradient: over 8 splits of M, reversed); inside a block the fp32 kernels' MFMA is a chain of fp32 fmas, one link per
  product, a bf16 MFMA adds its 16 exact products at once: the accumulators are modelled as those chains, not as a BLAS sum (whose
  vector-wide partial sums round far less often).  The bf16 GELU is common.h's gelu_fast.  It sizes C without a kernel's output
  and carries the injected defects of tests/test_conv_witnesses.py.

The constants.  ``measure_c()`` evaluates the model over the witness table (rows subsampled where a witness is big) and takes the
largest |model - ref64| / bound per operation, output and type; C is twice that, rounded up to one decimal - the factor 2 covers the
device's summation order and its exp / erf, as in attn_ref.py.  Measured on the CPU, 2026-10:

    operation   output    type   model max   C
    ---------   -------   ----   ---------   ----
    conv        y         bf16       1.989    4.0
    conv        y         f32        0.197    0.4
    conv        z         bf16       1.985    4.0
    convln      ln_mean   bf16       0.010    0.1
    convln      ln_rstd   bf16       0.012    0.1
    convln      y         bf16       1.991    4.0
    convln      z         bf16       1.984    4.0
    wgrad       dw        bf16       0.012    0.1
    wgrad       dw        f32        0.022    0.1

A kernel that needs more than its C has a defect or the cond lacks a term: neither is repaired by raising C.

On the fp32 weight gradient's constant.  The first form of wgrad_model summed with a BLAS einsum and measured 0.46 (C 1.0); the
device then needed 1.18 on the 12-row fp32 witness.  That was no reason to raise C, and C was not raised to fit: the cause was looked
for, and an fp32 fma chain over the rows IN KERNEL ORDER, evaluated on the CPU, gave the device's dw to the last bit (1.180) - the
kernel is right, and the model was not "the kernels' arithmetic": a BLAS dot product keeps vector-wide partial sums and rounds a
fraction as often as v_mfma_f32_32x32x2_f32, which is one fma per product.  The model now is that chain (exact products, one
rounding per link; reversed order, as the issue asks of a model), and C follows from it by the same rule as every other constant.
"""
import math
import types
import zlib

import torch

from tests.attn_ref import FLOOR, U_BF16, U_F32, assert_elementwise, ratio, unit_roundoff        # noqa: F401  (the instrument)
from tests import conv_witness as W

ACT_NONE, ACT_RELU, ACT_GELU, ACT_ELU, ACT_SIGMOID = 0, 1, 2, 3, 4
ACT_LIP = {ACT_NONE: 1.0, ACT_RELU: 1.0, ACT_GELU: 1.13, ACT_ELU: 1.0, ACT_SIGMOID: 0.25}      # max |act'|; GELU' peaks at 1.1290 (v = sqrt 2)
# Per-pixel operands repeat with these (prime) periods, so that the CPU side of a big witness (model, reference rows) never builds
# the whole tensors.  The limit of it: a defect that displaces data by a multiple of a period, all channels alike, is not seen - no
# tile, patch or ring of the kernels has a prime size, and the weights do not repeat.
PERIOD_X, PERIOD_ROW = 4099, 1021
LN_EPS = 1e-5

# what each epilogue kind of tests/dispatch_recorder.cpp sets (ConvLn gets z and a residual on top: run-time pointers of the same kernel)
EPILOGUES = {
    0: dict(), 1: dict(scale=1, shift=1, act=ACT_RELU), 2: dict(shift=1, act=ACT_GELU, z=1), 3: dict(shift=1, act=ACT_ELU),
    4: dict(mult=1, residual=1), 5: dict(mult=1, act=ACT_RELU), 6: dict(mult=1, act=ACT_RELU, z=1), 7: dict(gate=ACT_RELU), 8: dict(gate=ACT_GELU),
    9: dict(scale=1, shift=1, ln=1, z=1, residual=1), 10: dict(scale=1, shift=1, ln=1, act=ACT_GELU, z=1, residual=1), 11: dict(shift=1, residual=1, act=ACT_RELU)}


def variant(c):
    """0 | 1, fixed per call: which of two RUN-TIME forms of an epilogue a witness takes where the dispatcher cannot tell them apart."""
    return zlib.crc32(c.text.encode()) & 1


def epilogue(c):
    """Kind 3 runs as ELU or SIGMOID and the kind-7 gate as ReLU or ELU, by variant(c): the selection treats each pair alike (both
    activations are 'decided at run time', both gates are GATE = 1), so no shape moves; act_scale comes from the call."""
    e = dict(scale=0, shift=0, act=ACT_NONE, z=0, mult=0, residual=0, gate=None, ln=0, act_scale=c.act_scale)
    e.update(EPILOGUES[c.kind] if c.call == "F" else dict(scale=c.scaled))
    if c.call == "F" and variant(c):
        if c.kind == 3 and c.k != 3:                            # (tileconv.hip's 3x3 kernels have ELU as a compile-time variant of its own)
            e["act"] = ACT_SIGMOID
        if c.kind == 7:
            e["gate"] = ACT_ELU
    return types.SimpleNamespace(**e)


def torch_dtype(c):
    return torch.bfloat16 if c.dtype == W.BF16 else torch.float32


def rows_of(c):
    return c.B * c.Ho * c.Wo


# --------------------------------------------------------------------------------------------------------------- inputs
class Inputs:
    """Operands of one call in the storage type.  Per-pixel operands are a random block repeated with a prime period."""

    def __init__(self, c, seed=0):
        g = torch.Generator().manual_seed(1000003 * seed + 7919 * c.Cin + 31 * c.Cout + c.kind + 13 * c.B)
        dt, e, M = torch_dtype(c), epilogue(c), rows_of(c)
        rnd = lambda *s: torch.randn(*s, generator=g)
        self.c, self.e, self.dtype = c, e, dt
        self.x = rnd(min(c.B * c.Hi * c.Wi, PERIOD_X), c.Cin).to(dt)
        nrow = min(M, PERIOD_ROW)
        if c.call == "F":
            w = rnd(c.Cout, c.k * c.k, c.Cin) * c.K ** -0.5
            if e.ln:
                w[c.ln_C:] = 0                                   # the padding channels of a ConvLn layer are zero rows of its weight
            self.w = w.to(dt)
            nsc = c.ln_C if e.ln else c.Cout
            self.scale = rnd(nsc) if e.scale else None
            self.shift = rnd(nsc) if e.shift else None
            self.residual = rnd(nrow, c.Cout).to(dt) if e.residual else None
            if e.ln and self.residual is not None:
                self.residual[:, c.ln_C:] = 0
            self.mult = ((torch.rand(nrow, c.Cout, generator=g) > 0.2).float() / 0.8).to(dt) if e.mult else None      # dropout keep-mask / (1 - p)
            # the gate as the producer leaves it: the OUTPUT of a ReLU, or the PRE-activation of a GELU
            # (ReLU / ELU: a real output of that activation)
            gt = None if e.gate is None else rnd(nrow, c.Cout)
            if e.gate == ACT_RELU:
                gt = gt.clamp_min(0)
            elif e.gate == ACT_ELU:
                gt = torch.where(gt > 0, gt, torch.expm1(gt))
            self.gate = None if gt is None else gt.to(dt)
        else:
            self.gy = rnd(nrow, c.Cout).to(dt)
            self.scale = rnd(c.Cout) if e.scale else None

    def at(self, name, rows):
        t = getattr(self, name)
        return None if t is None else t[rows % t.shape[0]]

    def full(self, name, n, device="cpu"):
        """The whole per-pixel operand (n pixels / rows) on `device`."""
        t = getattr(self, name)
        if t is None:
            return None
        t = t.to(device)
        return t if t.shape[0] == n else t[torch.arange(n, device=device) % t.shape[0]].contiguous()


def tap_pixels(c, rows):
    """rows (R,) -> (R, taps) index of the input pixel in [0, B Hi Wi), -1 where the tap reads nothing."""
    rows = rows.long()
    ow, oh, b = rows % c.Wo, (rows // c.Wo) % c.Ho, rows // (c.Wo * c.Ho)
    kh, kw = torch.arange(c.k).repeat_interleave(c.k), torch.arange(c.k).repeat(c.k)
    oh, ow = oh[:, None], ow[:, None]
    if c.gather == W.GATHER_CONV:
        ih, iw = oh * c.stride - c.pad + kh, ow * c.stride - c.pad + kw
        ok = (ih >= 0) & (ih < c.Hi) & (iw >= 0) & (iw < c.Wi)
    elif c.gather == W.GATHER_TRANSPOSED:
        th, tw = oh + c.pad - kh, ow + c.pad - kw
        ok = (th >= 0) & (tw >= 0) & (th % c.stride == 0) & (tw % c.stride == 0)
        ih, iw = th.clamp_min(0) // c.stride, tw.clamp_min(0) // c.stride
        ok &= (ih < c.Hi) & (iw < c.Wi)
    else:
        vh, vw = oh - c.pad + kh, ow - c.pad + kw
        ok = (vh >= 0) & (vh < c.Hv) & (vw >= 0) & (vw < c.Wv)
        ih, iw = (vh.clamp_min(0) * c.Hi // c.Hv).clamp_max(c.Hi - 1), (vw.clamp_min(0) * c.Wi // c.Wv).clamp_max(c.Wi - 1)
    pix = (b[:, None] * c.Hi + ih) * c.Wi + iw
    return torch.where(ok, pix, torch.full_like(pix, -1))


def gathered(c, inp, rows, dtype, pix=None):
    """(R, taps, Cin): the im2col rows, zeros where a tap reads nothing."""
    pix = tap_pixels(c, rows) if pix is None else pix
    xg = inp.x[pix.clamp_min(0) % inp.x.shape[0]].to(dtype)
    return xg * (pix >= 0).to(dtype)[..., None]


# ------------------------------------------------------------------------------------------------------------ reference
def _act64(v, act):
    if act == ACT_RELU:
        return v.clamp_min(0)
    if act == ACT_GELU:
        return 0.5 * v * (1.0 + torch.erf(v * 0.7071067811865476))
    if act == ACT_ELU:
        return torch.where(v > 0, v, torch.expm1(v))
    if act == ACT_SIGMOID:
        return 1.0 / (1.0 + torch.exp(-v))
    return v


def _gelu_grad64(v):
    return 0.5 * (1.0 + torch.erf(v * 0.7071067811865476)) + v * 0.3989422804014327 * torch.exp(-0.5 * v * v)


def _act_error(v, a, act):
    if act == ACT_GELU:
        return 2 * a.abs() + 2 * v.abs()
    if act == ACT_SIGMOID:                                      # expf of -v: relative error (1 + |v|), seen through a (1 - a) <= a; the reciprocal
        return a.abs() * (3 + v.abs())
    return 2 * a.abs() if act == ACT_ELU else torch.zeros_like(v)


def conv_ref_cond(c, inp, rows, chunk=1024):
    """-> (ref, cond): dicts over the outputs (y, z, ln_mean, ln_rstd as present), fp64, for the output rows `rows`."""
    e = inp.e
    w = inp.w.double().reshape(c.Cout, c.K)
    acc, sab = [], []
    for r0 in range(0, len(rows), chunk):
        xg = gathered(c, inp, rows[r0:r0 + chunk], torch.float64).reshape(-1, c.K)
        acc.append(xg @ w.t())
        sab.append(xg.abs() @ w.abs().t())
    acc, sab = torch.cat(acc), torch.cat(sab)
    rk = math.sqrt(c.K)
    res = inp.at("residual", rows)
    res = None if res is None else res.double()
    zero = torch.zeros_like(acc)
    ref, cond = {}, {}
    if e.ln:
        C = c.ln_C
        gamma, beta = inp.scale.double(), inp.shift.double()
        a, bc = acc[:, :C], rk * sab[:, :C] + acc[:, :C].abs()
        mu = a.mean(1, keepdim=True)
        d = a - mu
        rstd = 1.0 / torch.sqrt((d * d).mean(1, keepdim=True) + LN_EPS)
        ec = bc + bc.mean(1, keepdim=True)
        q = rstd * rstd * (d.abs() * ec).mean(1, keepdim=True)
        t = d * rstd * gamma + beta
        bt = rstd * gamma.abs() * ec + (d * rstd * gamma).abs() * (q + 4) + beta.abs()
        y = _act64(t, e.act)
        by = ACT_LIP[e.act] * bt + _act_error(t, y, e.act)
        y, by = torch.cat([y, zero[:, C:]], 1), torch.cat([by, zero[:, C:]], 1)
        if res is not None:
            y, by = y + res, by + res.abs()
        ref.update(y=y, ln_mean=mu[:, 0], ln_rstd=rstd[:, 0])
        cond.update(y=(zero, by), ln_mean=(bc.mean(1), None), ln_rstd=((rstd * (q + 2))[:, 0], None))
        if e.z:
            ref["z"], cond["z"] = acc, (zero, rk * sab + acc.abs())
        return ref, cond
    sc = inp.scale.double() if e.scale else torch.ones(c.Cout, dtype=torch.float64)
    sh = inp.shift.double() if e.shift else torch.zeros(c.Cout, dtype=torch.float64)
    pre = res if (res is not None and not e.mult) else zero
    v = acc * sc + sh + pre
    bv = rk * sc.abs() * sab + (acc * sc).abs() + sh.abs() + pre.abs()
    a = _act64(v, e.act) * e.act_scale
    y, by = a, e.act_scale * (ACT_LIP[e.act] * bv + _act_error(v, a / e.act_scale, e.act)) + (a.abs() if e.act_scale != 1.0 else 0)
    if e.mult:
        m = inp.at("mult", rows).double()
        post = res if res is not None else zero
        y, by = a * m + post, m.abs() * by + (a * m).abs() + post.abs()
    if e.gate is not None:
        g = inp.at("gate", rows).double()
        f = (g > 0).double() if e.gate == ACT_RELU else (_gelu_grad64(g) if e.gate == ACT_GELU else torch.where(g > 0, torch.ones_like(g), g + 1))
        # the factor's own error: ReLU 0 | 1 exact; ELU one rounding of gate + 1 (relative); GELU gelu' from the fast erf: ABSOLUTE, 4 x 2^-24
        by = f.abs() * by + (4 * y.abs() if e.gate == ACT_GELU else (y * f).abs() if e.gate == ACT_ELU else 0)
        y = y * f
    ref["y"], cond["y"] = y, (zero, by)
    if e.z:
        ref["z"], cond["z"] = v, (zero, bv)
    return ref, cond


def conv_ref64(c, inp, rows):
    return conv_ref_cond(c, inp, rows)[0]


def conv_cond(c, inp, rows):
    return conv_ref_cond(c, inp, rows)[1]


def wgrad_ref_cond(c, inp, blocks, chunk=8192):
    """blocks: [(n0, n1, c0, c1)] -> ([dw block (n1 - n0, taps, c1 - c0) fp64], [cond (A, None)]), summed over all M rows."""
    M = rows_of(c)
    ref = [torch.zeros(n1 - n0, c.k * c.k, c1 - c0, dtype=torch.float64) for n0, n1, c0, c1 in blocks]
    sab = [torch.zeros_like(r) for r in ref]
    for r0 in range(0, M, chunk):
        rows = torch.arange(r0, min(M, r0 + chunk))
        xg, gy = gathered(c, inp, rows, torch.float64), inp.at("gy", rows).double()
        for i, (n0, n1, c0, c1) in enumerate(blocks):
            ref[i] += torch.einsum("mn,mtc->ntc", gy[:, n0:n1], xg[:, :, c0:c1])
            sab[i] += torch.einsum("mn,mtc->ntc", gy[:, n0:n1].abs(), xg[:, :, c0:c1].abs())
    cond = []
    for i, (n0, n1, c0, c1) in enumerate(blocks):
        sc = inp.scale[n0:n1].double()[:, None, None] if inp.scale is not None else 1.0
        ref[i] = ref[i] * sc
        cond.append((math.sqrt(M) * sab[i] * (sc.abs() if inp.scale is not None else 1.0), None))
    return ref, cond


def wgrad_ref64(c, inp, blocks):
    return wgrad_ref_cond(c, inp, blocks)[0]


# ---------------------------------------------------------------------------------------------------------------- model
def _gelu_fast(v):
    """common.h gelu_fast: erf by Abramowitz & Stegun 7.1.26, fp32."""
    x = v.abs() * 0.70710678118654752440
    t = 1.0 / (1.0 + 0.3275911 * x)
    e = torch.exp(-0.5 * v * v)
    poly = t * (0.254829592 + t * (-0.284496736 + t * (1.421413741 + t * (-1.453152027 + t * 1.061405429))))
    return v * (0.5 + torch.where(v < 0, -0.5, 0.5) * (1.0 - poly * e))


def _gelu_grad_fast(v):
    x = v.abs() * 0.70710678118654752440
    t = 1.0 / (1.0 + 0.3275911 * x)
    e = torch.exp(-0.5 * v * v)
    poly = t * (0.254829592 + t * (-0.284496736 + t * (1.421413741 + t * (-1.453152027 + t * 1.061405429))))
    return 0.5 + torch.where(v < 0, -0.5, 0.5) * (1.0 - poly * e) + v * 0.39894228040143267794 * e


def _act32(v, act, bf16):
    if act == ACT_GELU:
        return _gelu_fast(v) if bf16 else 0.5 * v * (1.0 + torch.erf(v * 0.70710678118654752440))
    return _act64(v, act)


DEFECTS = ("k_tile", "tap_shift", "row_unwritten", "block_swap", "residual_side", "tail_nonzero", "split_dropped", "act_scale", "wgrad_scale")


def conv_model(c, inp, rows, defect=None):
    """The forward kernels' arithmetic in fp32, outputs in the storage type.  defect: one of DEFECTS (tests that the instrument bites)."""
    e, dt, bf16 = inp.e, inp.dtype, c.dtype == W.BF16
    rows = rows.long()
    M = rows_of(c)
    if defect == "block_swap":                                 # the first 64-row block and its neighbour trade places
        rows = torch.where(rows < 64, rows + 64, torch.where(rows < 128, rows - 64, rows)).clamp_max(M - 1)
    pix = tap_pixels(c, rows)
    if defect == "tap_shift":                                  # tap (0, 0) reads one pixel to the right where the output sits on the left border
        left = (rows % c.Wo == 0) & (pix[:, 0] < 0) & (pix[:, 1] >= 0)
        pix[:, 0] = torch.where(left, pix[:, 1], pix[:, 0])
    xg = gathered(c, inp, rows, torch.float32, pix)
    w = inp.w.float()
    blk = 64 if c.Cin % 64 == 0 else 32
    acc = torch.zeros(len(rows), c.Cout)
    steps = [(t, c0) for t in range(c.k * c.k) for c0 in range(0, c.Cin, blk)]
    # every MFMA adds into the SAME fp32 accumulator: one chain over all of K, a link per instruction - 16 exact bf16 products at once,
    # or one fma (v_mfma_f32_32x32x2_f32 is a k-ordered chain of fp32 fmas, one rounding per product); fp64 holds the products exactly
    link = 16 if bf16 else 1
    for i, (t, c0) in enumerate(reversed(steps)):
        for k0 in reversed(range(c0, min(c.Cin, c0 + blk), link)):
            if bf16:                                           # (the 16 products are exact in fp32 as well; their sum is taken as good as exact)
                prod = xg[:, t, k0:k0 + link] @ w[:, t, k0:k0 + link].t()
            else:
                prod = xg[:, t, k0:k0 + link].double() @ w[:, t, k0:k0 + link].double().t()
            if defect == "k_tile" and i == 0:                  # the last K tile never reaches the first 32 columns
                prod[:, :32] = 0
            acc = acc + prod if bf16 else (acc.double() + prod).float()
    if defect == "tail_nonzero":                               # the channel past the tail of every tap reads the next tap's first value
        for t in range(c.k * c.k):
            acc += xg[:, t, :1] @ w[:, (t + 1) % (c.k * c.k), :1].t()
    res = inp.at("residual", rows)
    res = None if res is None else res.float()
    out = {}
    if e.ln:
        C = c.ln_C
        a = acc[:, :C]
        mu = torch.flip(a, (1,)).sum(1, keepdim=True) * (1.0 / C)
        d = a - mu
        rstd = torch.rsqrt(torch.flip(d * d, (1,)).sum(1, keepdim=True) * (1.0 / C) + LN_EPS)
        t = d * rstd * inp.scale + inp.shift
        y = torch.cat([_gelu_fast(t) if e.act == ACT_GELU else t, torch.zeros(len(rows), c.Cout - C)], 1)
        if res is not None:
            y = y + res
        out.update(y=y.to(dt), ln_mean=mu[:, 0], ln_rstd=rstd[:, 0])
        if e.z:
            out["z"] = acc.to(dt)
    else:
        sc = inp.scale if e.scale else torch.ones(c.Cout)
        sh = inp.shift if e.shift else torch.zeros(c.Cout)
        pre_side = (res is not None and not e.mult) != (defect == "residual_side" and res is not None)
        v = acc * sc + sh
        if pre_side:
            v = v + res
        y = _act32(v, e.act, bf16)
        if defect != "act_scale":
            y = y * torch.tensor(e.act_scale, dtype=torch.float32)
        if e.mult:
            y = y * inp.at("mult", rows).float()
        if res is not None and not pre_side:
            y = y + res
        if defect == "act_scale" and (e.mult or e.gate is not None):      # the factor behind the multiplier and the residual instead of in front
            y = y * torch.tensor(e.act_scale, dtype=torch.float32)       # (without either: dropped)
        if e.gate is not None:
            g = inp.at("gate", rows).float()
            y = y * ((g > 0).float() if e.gate == ACT_RELU else (_gelu_grad_fast(g) if e.gate == ACT_GELU else torch.where(g > 0, torch.ones_like(g), g + 1)))
        out["y"] = y.to(dt)
        if e.z:
            out["z"] = v.to(dt)
    if defect == "row_unwritten":                              # the last row of M keeps what the buffer held (zeros here)
        for t in out.values():
            t[rows == M - 1] = 0
    return out


def wgrad_model(c, inp, blocks, defect=None, splits=8):
    M = rows_of(c)
    per = (M + splits - 1) // splits
    splits = (M + per - 1) // per                              # no empty split
    # rows per link of the chain: a bf16 MFMA adds 16 exact products at once, the fp32 MFMA is one fma per row (cdna: k-ordered fmaf
    # chain, one rounding per product); a long fp32 sum is modelled in 16-row links as well (time)
    step = 1 if (c.dtype == W.F32 and M <= 16384) else 16
    out = [torch.zeros(n1 - n0, c.k * c.k, c1 - c0) for n0, n1, c0, c1 in blocks]
    for s in reversed(range(splits)):
        if defect == "split_dropped" and s == splits - 1:
            continue
        part = [torch.zeros_like(o) for o in out]
        end = min(M, (s + 1) * per)
        for r0 in reversed(range(s * per, end, 4096)):
            rows = torch.arange(r0, min(end, r0 + 4096))
            xg, gy = gathered(c, inp, rows, torch.float32), inp.at("gy", rows).float()
            for i, (n0, n1, c0, c1) in enumerate(blocks):
                for m0 in reversed(range(0, len(rows), step)):                 # the accumulator is a CHAIN over the reduction steps
                    # one link: the exact products (fp64 holds them) added to the fp32 accumulator with one rounding - an fma
                    part[i] = (part[i].double() + torch.einsum("mn,mtc->ntc", gy[m0:m0 + step, n0:n1].double(), xg[m0:m0 + step, :, c0:c1].double())).float()
        for i, (n0, n1, c0, c1) in enumerate(blocks):
            if inp.scale is not None and not (defect == "wgrad_scale" and s == 0):      # the scale rides on every flush (defect: one flush without)
                part[i] = part[i] * inp.scale[n0:n1, None, None]
            out[i] += part[i]
    return out


# ------------------------------------------------------------------------------------------------- what a test compares
WHOLE_LIMIT = 2e9                              # multiply-accumulates of the fp64 reference up to which the whole output is compared


def _hash(i, salt=0):
    return ((i + salt) * 2654435761 >> 7) & 0x7FFFFFFF


def border_rows(c, count=256):
    """count output pixels on the border of their image (pseudo-random, all four sides, all images in turn)."""
    out = []
    for i in range(count):
        b, side, h = i % c.B, (i // c.B) % 4, _hash(i, 17)
        oh, ow = ((0, h % c.Wo), (c.Ho - 1, h % c.Wo), (h % c.Ho, 0), (h % c.Ho, c.Wo - 1))[side]
        out.append((b * c.Ho + oh) * c.Wo + ow)
    return out


def parity_rows(c, per=2, chunk=256):
    """Stride-2 transposed gather: `per` pseudo-random pixels of each (oy % 2, ox % 2) class out of every `chunk` consecutive pixels
    (all of a class that has fewer there)."""
    m = torch.arange(rows_of(c))
    cls = ((m // c.Wo) % c.Ho % 2) * 2 + (m % c.Wo) % 2
    key = (m // chunk) * 4 + cls
    h = (m * 2654435761 >> 7) & 0xFFFF
    order = torch.argsort(key * 65536 + h)
    ks = key[order]
    start = torch.ones_like(ks, dtype=torch.bool)
    start[1:] = ks[1:] != ks[:-1]
    first = torch.cummax(torch.where(start, torch.arange(len(ks)), torch.zeros_like(ks)), 0).values
    return order[torch.arange(len(ks)) - first < per]


def compare_rows(c, limit=WHOLE_LIMIT):
    """Output rows a test compares: all of them while the reference costs <= limit, else every row of the first and last two 64-row
    blocks, the last row, the first and one pseudo-random row of every 64-row block, 256 border pixels and, for the stride-2 transposed
    gather, parity_rows(): two pixels of each (oy % 2, ox % 2) class per 256 pixels.
    -> (rows, number of 64-row blocks without a row)."""
    M = rows_of(c)
    if M * c.Cout * c.K <= limit:
        return torch.arange(M), 0
    nb = (M + 63) // 64
    rows = set(range(min(128, M))) | set(range(max(0, (nb - 2) * 64), M)) | {M - 1} | set(border_rows(c))
    for b in range(nb):
        rows.update((b * 64, min(b * 64 + _hash(b) % 64, M - 1)))
    if c.gather == W.GATHER_TRANSPOSED and c.stride == 2:
        rows.update(parity_rows(c).tolist())
    rows = torch.tensor(sorted(rows))
    return rows, nb - int(torch.unique(rows // 64).numel())


def model_rows(c, budget=5e6):
    """The subsample measure_c() uses: all rows of a small witness, else first / last / border / pseudo-random rows within budget."""
    M = rows_of(c)
    if M * c.Cout * c.K <= budget:
        return torch.arange(M)
    n = max(8, int(budget // (c.Cout * c.K)))
    if c.call == "F" and c.kind in (9, 10):
        n = max(n, 8192)                                       # ln_mean / ln_rstd are ONE value per row: their maximum needs rows, not elements
    rows = {0, 1, M - 2, M - 1} | set(border_rows(c, n // 4)) | {_hash(i, 5) % M for i in range(n // 2)}
    return torch.tensor(sorted(r for r in rows if 0 <= r < M))


def wgrad_blocks(c, limit=WHOLE_LIMIT):
    """(n0, n1, c0, c1) blocks of dw a test compares: the whole gradient while cheap, else 32-wide blocks such that every n-block and
    every c-block index is hit."""
    M = rows_of(c)
    if M * c.Cout * c.K <= limit:
        return [(0, c.Cout, 0, c.Cin)]
    nb, cb = (c.Cout + 31) // 32, (c.Cin + 31) // 32
    return [(32 * (i % nb), min(c.Cout, 32 * (i % nb) + 32), 32 * ((i + 1) % cb), min(c.Cin, 32 * ((i + 1) % cb) + 32)) for i in range(max(nb, cb))]


def operation(c):
    return "wgrad" if c.call != "F" else ("convln" if c.kind in (9, 10) else "conv")


def dtype_name(c):
    return "bf16" if c.dtype == W.BF16 else "f32"


def out_unit(c, name):
    return U_F32 if name in ("ln_mean", "ln_rstd", "dw") else (U_BF16 if c.dtype == W.BF16 else U_F32)


# ------------------------------------------------------------------------------------------------------------ constants
def measure_c(table=None):
    """{(operation, output, type): largest model ratio} over the witness table."""
    worst = {}
    for _, c in (W.load() if table is None else table):
        if c.call == "F":
            inp, rows = Inputs(c), model_rows(c)
            ref, cond = conv_ref_cond(c, inp, rows)
            got = conv_model(c, inp, rows)
            rs = {k: float(ratio(got[k], ref[k], cond[k], out_unit(c, k)).max()) for k in ref}
        else:
            rs = {"dw": 0.0}
            for i in range(c.n):
                j = W.with_batch(c, i)
                if rows_of(j) * c.Cout * c.K > 2e7:             # a big weight gradient: one 32 x 32 block (the sum still runs over all M)
                    blocks = wgrad_blocks(j, 0)[:1]
                else:
                    blocks = wgrad_blocks(j)
                inp = Inputs(j, seed=i)
                ref, cond = wgrad_ref_cond(j, inp, blocks)
                got = wgrad_model(j, inp, blocks)
                rs["dw"] = max([rs["dw"]] + [float(ratio(g, r, cd, U_F32).max()) for g, r, cd in zip(got, ref, cond)])
        for k, v in rs.items():
            key = (operation(c), k, dtype_name(c))
            worst[key] = max(worst.get(key, 0.0), v)
    return worst


def c_of(measured):
    return math.ceil(2 * measured * 10 - 1e-9) / 10


def format_table(worst):
    lines = ["    operation   output    type   model max   C", "    ---------   -------   ----   ---------   ----"]
    for (op, out, dt), v in sorted(worst.items()):
        lines.append("    %-9s   %-7s   %-4s   %9.3f   %4.1f" % (op, out, dt, v, c_of(v)))
    return "\n".join(lines)


# C[(operation, output, type)]: twice the largest model ratio over the witness table, one decimal up; the module docstring shows
# format_table(MEASURED) (tests/test_conv_witnesses.py checks both)
MEASURED = {
    ("conv", "y", "bf16"): 1.989,
    ("conv", "y", "f32"): 0.197,
    ("conv", "z", "bf16"): 1.985,
    ("convln", "ln_mean", "bf16"): 0.010,
    ("convln", "ln_rstd", "bf16"): 0.012,
    ("convln", "y", "bf16"): 1.991,
    ("convln", "z", "bf16"): 1.984,
    ("wgrad", "dw", "bf16"): 0.012,
    ("wgrad", "dw", "f32"): 0.022,
}
C = {k: c_of(v) for k, v in MEASURED.items()}
