"""fp64 references, error bounds and rounding models of the row kernels of csrc/rowops.hip and csrc/inorm.hip (CPU only, plain
module; the instrument is the one of tests/attn_ref.py: assert_elementwise, ratio, FLOOR and the unit round-offs come from there).

The calls are the lines of tests/golden/row_witnesses.txt (tests/row_witness.py parses them).  ``inputs(c)`` draws the operands of a
call with a generator seeded by the line, in the storage type; every reference works on those rounded operands, so the only error
left between a kernel and its reference is the kernel's own arithmetic.

* ``reference(c, inp)`` -> (ref, cond): per output the fp64 result of include/gwdepth.h's formula and the pair (A, B) of the bound
      |got - ref| <= c u (|ref| + A + (2^-24 / u) B),      u = 2^-9 for a bf16 output, 2^-24 for an fp32 one.
  A is in units of the output's own rounding, B in units of fp32's (every kernel here computes in fp32 and rounds once, at the store,
  so the forward and element-wise outputs have A = 0).  A zero bound demands an exact zero: padding columns, a closed ReLU, masked keys.
  With e = mean_c |x_c| (the fp32 error of the mean; x itself is exact in storage, so the element's own error of the ConvLn bound of
  tests/conv_ref.py is zero), d = x - mu, q = rstd^2 mean_c |d_c| e (the relative error of rstd), t = d rstd gamma + beta:
      LayerNorm forward     mean: A = e          rstd: A = rstd (q + 2)          (fp32 outputs)
                            Bt = rstd |gamma| e + |d rstd gamma| (q + 4) + |beta|;   y: B = L Bt + E + |residual|,  L = max |act'| (1, GELU 1.13),
                            E = 2 |gelu(t)| (erf) + 2 |t| (bf16: the ABSOLUTE 1.5e-7 of common.h's gelu_parts_fast; a relative bound
                            fails in the far negative tail, which is no kernel defect);  columns C..ld-1: zero
      LayerNorm backward    (mean, rstd are operands)  xh = d rstd, g = gy gelu'(t), gw = g gamma;
                            Eg = |gamma| (|gy| (4 + 0.8 (3 |xh gamma| + |beta|)) + 2 |g|) with the GELU (4 |gy|: the fast erf's absolute
                            error in gelu', which stays where gelu' crosses zero at -0.75; in fp32 2 |gy|: gelu' = cdf + v pdf is a sum of
                            two terms of opposite sign there, each rounded on its own, |cdf| + |v pdf| <= 1.2, and the model showed a
                            relative bound to fail by 1.5e5 at the crossing; 0.8 = max |gelu''| times the error of t), + |gw|
                            gx: B = rstd (Eg + mean Eg + |xh| mean (Eg |xh| + 2 |gw xh|) + 2 |xh mean(gw xh)|) + |gx| + |gskip|, and with
                            the ELU input  B = elu'(x) B + 2 |gx + gskip| (|x| + |mu|) where x <= 0 (x is rebuilt as xh / rstd + mu) + |out|
                            dgamma, dbeta: fp32 atomic sums over rows,  A = sqrt(rows) sum_r |term_r| + sum_r (the term's own error)
      softmax               attn_ref.softmax_cond:  y: B = y (2 max |scale x| + 1);  gx (from the STORED y): A = B = |scale| y (sum y |gy| + |gy - <y, gy>|)
      activation backward   a' = act'(.), f = act_scale * per-channel scale:  gx: B = 4 |gx| + |gy f| E,  E = 2 |ref / act_scale| (ELU, ref <= 0: the
                            division), 3 sg (SIGMOID), 4 + 2 |a'| (GELU; 2 + 2 |a'| in fp32, see above);  with mult, gy mult is rounded to storage
                            first in the reference as in the kernel (the product of two storage values, rounded once, is exact arithmetic)
      colsum, colsum_batch  out = pattern + sum_r g:  A = sqrt(rows) sum_r |g| + |pattern|       (fp32 atomics; the caller's prefill is kept)
      dbias                 of gwd_act_backward_colsum: against the fp64 column sum of the gx THE KERNEL RETURNED, A as colsum (tighter
                            than a bound that carries `rows` storage roundings); gx is checked on its own
      inorm forward         per slice s of n_s positions: part mean_s: A = mean_s |u|;  M2_s: A = sum_s (2 |d_s| e_s + 3 d_s^2);  empty slice: zeros
                            stat mean: A = e;  rstd: A = rstd (q + 2);   n = (u - mean) rstd:  y: B = 1.13 (rstd e + |n| (q + 4)) + E(n) + |a|
      inorm backward        gn = gy gelu'(n), Eg = |gy| (4 + 2.4 |n|) + 2 |gn| (fp32: 2 + 2.4 |n|);  part: A = sqrt(n_s) sum_s |term| + sum_s (Eg, Eg |n| + 2 |gn n|)
                            du: B = rstd (Eg + mean Eg + |n| mean (Eg |n| + 2 |gn n|) + 2 |n mean(gn n)| + |gn| + |mean gn|) + |du|
* ``model(c, inp, defect=None)`` - the kernels' arithmetic in fp32 on the CPU with the ONE rounding at the store (act_bwd_colsum rounds
  gy mult once more, as the kernel documents), the bf16 GELU as common.h's gelu_fast, every reduction over the flipped axis (another
  order than the device's).  It sizes C without a kernel's output and carries the injected defects of tests/test_row_witnesses.py.

The constants.  ``measure_c()`` evaluates the model over the witness table and takes the largest |model - ref| / bound per operation,
output and type; C is twice that, rounded up to one decimal (the factor 2 covers the device's summation order and its exp / erf / rsqrt),
as in attn_ref.py and conv_ref.py.  Measured on the CPU, 2026-10:

@TABLE@

A kernel that needs more than its C has a defect or the bound lacks a term: neither is repaired by raising C.
"""
import math
import zlib

import torch

from tests.attn_ref import FLOOR, U_BF16, U_F32, assert_elementwise, ratio, softmax_backward_ref64, softmax_cond        # noqa: F401  (the instrument)
from tests.conv_ref import _act64, _gelu_fast, _gelu_grad64, _gelu_grad_fast, c_of
from tests import row_witness as W

LN_EPS = 1e-5
DEFECTS = ("ragged_unwritten", "onepass_var", "pad_nonzero", "lanes_beyond_c", "dgamma_wave", "softmax_tail", "mask_mod", "scale_dropped", "elu_no_div",
           "merge_no_between", "last_slice_short", "block0_off_by_one")
OPERATION = {"LF": "ln_fwd", "LB": "ln_bwd", "SF": "softmax_fwd", "SM": "softmax_fwd", "SB": "softmax_bwd", "SS": "softmax_bwd", "AB": "act_bwd",
             "AC": "act_bwd_colsum", "CS": "colsum", "CB": "colsum", "IF": "inorm_fwd", "IB": "inorm_bwd"}
F32_OUTPUTS = ("mean", "rstd", "dgamma", "dbeta", "out", "dbias", "stat", "part")


def torch_dtype(c):
    return torch.bfloat16 if c.dtype == W.BF16 else torch.float32


def dtype_name(c):
    return "bf16" if c.dtype == W.BF16 else "f32"


def out_unit(c, name):
    return U_F32 if name.rstrip("0123456789") in F32_OUTPUTS else (U_BF16 if c.dtype == W.BF16 else U_F32)


def pattern(C):
    """What the ACCUMULATED outputs (colsum's out, dbias) hold before the call: fixed, non-zero, exact in fp32."""
    return 0.5 + 0.25 * (torch.arange(C) % 7).float()


def forms(c):
    """The call and its run-time siblings that launch the same kernel at the same shape and that one witness per kernel cannot spread
    over a family: the five activations of the kernels that switch on `act` at run time, mult on and off for the single
    fp32 act_bwd_colsum kernel, a colsum_batch call of one job."""
    if c.call == "AB" or (c.call == "AC" and c.dtype == W.F32):
        acts = range(5)
    elif c.call == "AC" and c.act in (W.ACT_ELU, W.ACT_SIGMOID):
        acts = (W.ACT_ELU, W.ACT_SIGMOID)
    elif c.call == "CB":
        return [c, W.parse_call("CB %d 1 %d %d" % (c.dtype, c.jobs[-1][0], c.jobs[-1][1]))]
    else:
        return [c]
    f = c.text.split()
    out = [c] + [W.parse_call(" ".join(f[:4] + [str(a)] + f[5:])) for a in acts if a != c.act]
    if c.call == "AC" and c.dtype == W.F32:                      # the one fp32 kernel: with and without the multiplier
        out.append(W.parse_call(" ".join(f[:6] + [str(1 - c.mult)])))
    return out


# --------------------------------------------------------------------------------------------------------------- inputs
def _gen(c):
    return torch.Generator().manual_seed(zlib.crc32(c.text.encode()))


def _rows_with_offsets(g, rows, n, dt, positive=False):
    """(rows, n) values: row r % 4 == 0, 2 zero mean (std 1 and 3); r % 4 == 1, 3 offset rows, mean = +-k std with k = 12 in bf16 (after
    the rounding |mean| >= 10 std and std >= 8 ulp: an ulp of bf16 at m is m / 128 at most, std = m / 12 = 10.7 ulp) and 1000 in
    fp32; one constant row in the middle."""
    x = torch.randn(rows, n, generator=g)
    r = torch.arange(rows)
    k = 12.0 if dt == torch.bfloat16 else 1000.0
    std = torch.where(r % 4 == 2, 3.0, 1.0) * torch.where(r % 4 == 3, 0.25, 1.0)
    mean = torch.where(r % 4 == 1, k, 0.0) * std + torch.where(r % 4 == 3, k if positive else -k, 0.0) * std
    x = x * std[:, None] + mean[:, None]
    x[rows // 2] = 3.0
    return x


def _elu(z):
    return torch.where(z > 0, z, torch.expm1(z))


def inputs(c):
    """The operands of a call: a dict of CPU tensors in the storage type (fp32 for parameters and statistics)."""
    g, dt = _gen(c), torch_dtype(c)
    rnd = lambda *shape: torch.randn(*shape, generator=g)
    inp = {}
    if c.call in ("LF", "LB"):
        rows, C, ld = c.rows, c.C, c.pitch
        elu = c.call == "LB" and c.elu
        x = _rows_with_offsets(g, rows, C, dt, positive=elu)
        if elu:                                                  # a true ELU output: above -1, both sides of 0, some exactly 0
            x = _elu(x).clamp_min(-0.99)                         # (stays above -1 after the rounding to bf16)
            x[torch.rand(rows, C, generator=g) < 0.05] = 0.0
            x[rows // 2] = 3.0

        def pitched(t):                                          # the padding columns of an input hold NaN: never read
            full = torch.full((rows, ld), float("nan"))
            full[:, :C] = t
            return full.to(dt)
        inp["x"] = pitched(x)
        if c.affine:
            inp["gamma"], inp["beta"] = 1.0 + 0.5 * rnd(C), 0.5 * rnd(C)
        if c.call == "LF":
            if c.residual:
                inp["residual"] = pitched(rnd(rows, C))
        else:
            inp["gy"] = pitched(rnd(rows, C))
            if c.gskip:
                inp["gskip"] = pitched(rnd(rows, C))
            xd = inp["x"][:, :C].double()
            mu = xd.mean(1)
            inp["mean"] = mu.float()
            inp["rstd"] = (1.0 / torch.sqrt(((xd - mu[:, None]) ** 2).mean(1) + LN_EPS)).float()
    elif c.family == "softmax":
        rows, L = c.rows, c.L
        spread = 40.0 / (c.scale if c.call == "SM" else 1.0)
        x = rnd(rows, L) * spread                                # hard logits: most terms underflow
        x[torch.rand(rows, L, generator=g) < 0.02] = float("-inf")
        nm = (rows + c.rpm - 1) // c.rpm if c.call == "SM" and c.mask else 0
        keep = 1 + (7 * torch.arange(max(nm, rows))) % max(L - 2, 1) if L >= 3 else torch.zeros(max(nm, rows), dtype=torch.long)
        if nm:
            m = torch.arange(nm)
            mask = torch.rand(nm, L, generator=g) < 0.3
            if L >= 3:
                mask[m % 5 == 0, 0] = True                       # the first key, the last key, a whole 64-key stripe, all keys but one
                mask[m % 5 == 1, L - 1] = True
                mask[m % 5 == 2, 64 * ((L - 1) // 64 // 2):64 * ((L - 1) // 64 // 2) + 64] = True
                mask[m % 5 == 3] = True
                mask[m, keep[:nm]] = False
            else:
                mask[:] = False
            assert not mask.all(-1).any()                        # no fully masked row: it is NaN by definition and has no reference
            inp["mask"] = mask.to(torch.uint8)
            kr = keep[:nm].repeat_interleave(c.rpm)[:rows]
        else:
            kr = keep[:rows]
        x[torch.arange(rows), kr] = rnd(rows) * spread           # the key that stays is finite
        if c.call in ("SF", "SM"):
            inp["x"] = x.to(dt)
        else:
            s = x.double() * 0.25
            e = torch.exp(s - s.max(-1, keepdim=True).values)
            inp["y"] = (e / e.sum(-1, keepdim=True)).to(dt)
            inp["gy"] = rnd(rows, L).to(dt)
    elif c.call in ("AB", "AC"):
        rows, C = c.rows, c.C
        inp["gy"] = rnd(rows, C).to(dt)
        pre = 1.5 * rnd(rows, C)
        edge = torch.rand(rows, C, generator=g)
        special = torch.tensor([0.0, 1e-3, -1e-3, 2.0 ** -20, -2.0 ** -20])[torch.randint(0, 5, (rows, C), generator=g)]
        if c.act == W.ACT_GELU:                                  # the pre-activation, a tenth of it around -0.7518 where gelu' crosses zero
            pre = torch.where(edge < 0.1, -0.7518 + special * 8, pre)
            inp["ref"] = pre.to(dt)
        elif c.act != W.ACT_NONE:                                # the stored OUTPUT act_scale act(v), a tenth of it at and around 0
            pre = torch.where(edge < 0.1, special, pre)
            inp["ref"] = (c.act_scale * _act64(pre.double(), c.act)).to(dt)
            if c.act == W.ACT_ELU:
                inp["ref"] = torch.maximum(inp["ref"], torch.tensor(-c.act_scale * 0.996).to(dt))      # stays above -act_scale after rounding
        if c.call == "AB" and c.chscale:
            inp["scale"] = 1.0 + 0.5 * rnd(C)
        if c.call == "AC" and c.mult:
            inp["mult"] = ((torch.rand(rows, C, generator=g) < 0.9).float() / 0.9).to(dt)             # a dropout multiplier, 1 / 0.9 rounded
    elif c.call == "CS":
        inp["g"] = _rows_with_offsets(g, c.rows, c.C, dt).to(dt)
    elif c.call == "CB":
        for i, (rows, C) in enumerate(c.jobs):
            inp["g%d" % i] = (rnd(rows, C) + 0.1 * i).to(dt)
    else:
        B, L, C = c.B, c.L, c.C
        u = rnd(B, L, C)
        ch = torch.arange(B * C).reshape(B, 1, C)
        k = 12.0 if dt == torch.bfloat16 else 1000.0
        u = u * torch.where(ch % 3 == 2, 3.0, 1.0) + torch.where(ch % 3 == 1, k, 0.0)
        inp["u"] = u.to(dt)
        if c.call == "IF":
            inp["a"] = rnd(B, L, C).to(dt)
        else:
            inp["gy"] = rnd(B, L, C).to(dt)
            ud = inp["u"].double()
            mu = ud.mean(1)
            rs = 1.0 / torch.sqrt(((ud - mu[:, None]) ** 2).mean(1) + LN_EPS)
            inp["stat"] = torch.stack([mu, rs], -1).float()
    return inp


# ------------------------------------------------------------------------------------------------------------ reference
def _gelu_error(c, t, a):
    return 2 * a.abs() + (2 * t.abs() if c.dtype == W.BF16 else 0)


def _gelu_grad_error(c, gy, t_err, g):
    """Eg without gamma: |gy| (absolute error of gelu' + max |gelu''| times the error of its argument) + 2 |g|."""
    return gy.abs() * ((4 if c.dtype == W.BF16 else 2) + 0.8 * t_err) + 2 * g.abs()


def slice_bounds(L, S):
    per = (L + S - 1) // S
    return [(min(s * per, L), min(s * per + per, L)) for s in range(S)]


def _pad(t, ld):
    out = torch.zeros(t.shape[0], ld, dtype=t.dtype)
    out[:, :t.shape[1]] = t
    return out


def _colsum_ref(gd, rows):
    C = gd.shape[1]
    p = pattern(C).double()
    return p + gd.sum(0), (math.sqrt(rows) * gd.abs().sum(0) + p, None)


def reference(c, inp, got=None):
    """-> (ref, cond) over the outputs of the call.  got: the outputs under test (dbias is checked against the column sum of got's gx)."""
    d64 = {k: v.double() for k, v in inp.items()}
    ref, cond = {}, {}
    if c.call in ("LF", "LB"):
        C, ld = c.C, c.pitch
        x = d64["x"][:, :C]
        gamma, beta = d64.get("gamma", torch.ones(C, dtype=torch.float64)), d64.get("beta", torch.zeros(C, dtype=torch.float64))
        gelu = bool(c.gelu)
        if c.call == "LF":
            mu = x.mean(1, keepdim=True)
            d = x - mu
            rstd = 1.0 / torch.sqrt((d * d).mean(1, keepdim=True) + LN_EPS)
            e = x.abs().mean(1, keepdim=True)
            q = rstd * rstd * (d.abs() * e).mean(1, keepdim=True)
            t = d * rstd * gamma + beta
            bt = rstd * gamma.abs() * e + (d * rstd * gamma).abs() * (q + 4) + beta.abs()
            a = _act64(t, W.ACT_GELU) if gelu else t
            by = (1.13 * bt + _gelu_error(c, t, a)) if gelu else bt
            if "residual" in d64:
                a = a + d64["residual"][:, :C]
                by = by + d64["residual"][:, :C].abs()
            ref.update(y=_pad(a, ld), mean=mu[:, 0], rstd=rstd[:, 0])
            cond.update(y=(torch.zeros(c.rows, ld, dtype=torch.float64), _pad(by, ld)), mean=(e[:, 0], None), rstd=((rstd * (q + 2))[:, 0], None))
        else:
            mu, rstd = d64["mean"][:, None], d64["rstd"][:, None]
            gy = d64["gy"][:, :C]
            xh = (x - mu) * rstd
            t = xh * gamma + beta
            g = gy * _gelu_grad64(t) if gelu else gy
            gw = g * gamma
            eg = gamma.abs() * _gelu_grad_error(c, gy, 3 * (xh * gamma).abs() + beta.abs(), g) if gelu else torch.zeros_like(g)
            eg = eg + gw.abs()
            m = lambda v: v.mean(1, keepdim=True)
            s2 = m(gw * xh)
            gx = rstd * (gw - m(gw) - xh * s2)
            b = rstd * (eg + m(eg) + xh.abs() * m(eg * xh.abs() + 2 * (gw * xh).abs()) + 2 * (xh * s2).abs()) + gx.abs()
            if "gskip" in d64:
                gx = gx + d64["gskip"][:, :C]
                b = b + d64["gskip"][:, :C].abs()
            if c.elu:
                f = torch.where(x > 0, 1.0, x + 1.0)
                b = f * b + torch.where(x > 0, 0.0, 2 * gx.abs() * (x.abs() + mu.abs()))
                gx = gx * f
                b = b + gx.abs()
            ref["gx"] = _pad(gx, ld)
            cond["gx"] = (torch.zeros(c.rows, ld, dtype=torch.float64), _pad(b, ld))
            if c.dgamma:
                eg0 = _gelu_grad_error(c, gy, 3 * (xh * gamma).abs() + beta.abs(), g) if gelu else torch.zeros_like(g)
                sq = math.sqrt(c.rows)
                ref.update(dgamma=(g * xh).sum(0), dbeta=g.sum(0))
                cond.update(dgamma=(sq * (g * xh).abs().sum(0) + (eg0 * xh.abs() + 2 * (g * xh).abs()).sum(0), None), dbeta=(sq * g.abs().sum(0) + eg0.sum(0), None))
    elif c.call in ("SF", "SM"):
        scale = c.scale if c.call == "SM" else 1.0
        s = d64["x"] * scale
        mask = inp.get("mask")
        if mask is not None:
            s = s.masked_fill(mask.bool().repeat_interleave(c.rpm, 0)[:c.rows], float("-inf"))
        e = torch.exp(s - s.max(-1, keepdim=True).values)
        y = e / e.sum(-1, keepdim=True)
        big = torch.where(torch.isfinite(s), s.abs(), torch.zeros_like(s)).max(-1, keepdim=True).values
        ref["y"], cond["y"] = y, (torch.zeros_like(y), y * (2 * big + 1))
    elif c.call in ("SB", "SS"):
        scale = c.scale if c.call == "SS" else 1.0
        ref["gx"] = softmax_backward_ref64(d64["y"], d64["gy"], scale)
        cond["gx"] = softmax_cond(d64["y"], d64["gy"], scale, y_stored=d64["y"])["gx"]
    elif c.call in ("AB", "AC"):
        gy = d64["gy"]
        if "mult" in inp:
            gy = (gy * d64["mult"]).to(torch_dtype(c)).double()     # rounded as the separate multiply it replaces
        f = torch.full((c.C,), c.act_scale, dtype=torch.float64) * d64.get("scale", 1.0)
        rv = d64["ref"] / c.act_scale if c.act not in (W.ACT_NONE, W.ACT_GELU) else d64.get("ref")
        err = torch.zeros_like(gy)
        if c.act == W.ACT_RELU:
            a = (rv > 0).double()
        elif c.act == W.ACT_GELU:
            a = _gelu_grad64(rv)
            err = (4 if c.dtype == W.BF16 else 2) + 2 * a.abs()
        elif c.act == W.ACT_ELU:
            a = torch.where(rv > 0, 1.0, rv + 1.0)
            err = torch.where(rv > 0, 0.0, 2 * rv.abs())
        elif c.act == W.ACT_SIGMOID:
            a = rv * (1.0 - rv)
            err = 3 * rv.abs()
        else:
            a = torch.ones_like(gy)
        gx = gy * a * f
        ref["gx"], cond["gx"] = gx, (torch.zeros_like(gx), 4 * gx.abs() + (gy * f).abs() * err)
        if c.call == "AC":
            stored = gx.to(torch_dtype(c)).double() if got is None else got["gx"].detach().double().cpu()
            ref["dbias"], cond["dbias"] = _colsum_ref(stored, c.rows)
    elif c.call == "CS":
        ref["out"], cond["out"] = _colsum_ref(d64["g"], c.rows)
    elif c.call == "CB":
        for i, (rows, C) in enumerate(c.jobs):
            ref["out%d" % i], cond["out%d" % i] = _colsum_ref(d64["g%d" % i], rows)
    else:
        B, L, C, S = c.B, c.L, c.C, c.S
        u = d64["u"]
        part = torch.zeros(B, S, C, 2, dtype=torch.float64)
        pa = torch.zeros_like(part)
        if c.call == "IF":
            for s, (lo, hi) in enumerate(slice_bounds(L, S)):
                if hi > lo:
                    us = u[:, lo:hi]
                    ms = us.mean(1, keepdim=True)
                    ds = us - ms
                    es = us.abs().mean(1, keepdim=True)
                    part[:, s, :, 0], part[:, s, :, 1] = ms[:, 0], (ds * ds).sum(1)
                    pa[:, s, :, 0], pa[:, s, :, 1] = es[:, 0], (2 * ds.abs() * es + 3 * ds * ds).sum(1)
            mu = u.mean(1, keepdim=True)
            d = u - mu
            rstd = 1.0 / torch.sqrt((d * d).mean(1, keepdim=True) + LN_EPS)
            e = u.abs().mean(1, keepdim=True)
            q = rstd * rstd * (d.abs() * e).mean(1, keepdim=True)
            n = d * rstd
            ge = _act64(n, W.ACT_GELU)
            y = d64["a"] + ge
            ref.update(y=y, stat=torch.stack([mu[:, 0], rstd[:, 0]], -1), part=part)
            cond.update(y=(torch.zeros_like(y), 1.13 * (rstd * e + n.abs() * (q + 4)) + _gelu_error(c, n, ge) + d64["a"].abs()),
                        stat=(torch.stack([e[:, 0], (rstd * (q + 2))[:, 0]], -1), None), part=(pa, None))
        else:
            mu, rstd = d64["stat"][:, None, :, 0], d64["stat"][:, None, :, 1]
            gy = d64["gy"]
            n = (u - mu) * rstd
            gn = gy * _gelu_grad64(n)
            eg = _gelu_grad_error(c, gy, 3 * n.abs(), gn)
            for s, (lo, hi) in enumerate(slice_bounds(L, S)):
                if hi > lo:
                    sl, sq = slice(lo, hi), math.sqrt(hi - lo)
                    part[:, s, :, 0], part[:, s, :, 1] = gn[:, sl].sum(1), (gn[:, sl] * n[:, sl]).sum(1)
                    pa[:, s, :, 0] = sq * gn[:, sl].abs().sum(1) + eg[:, sl].sum(1)
                    pa[:, s, :, 1] = sq * (gn[:, sl] * n[:, sl]).abs().sum(1) + (eg[:, sl] * n[:, sl].abs() + 2 * (gn[:, sl] * n[:, sl]).abs()).sum(1)
            m = lambda v: v.mean(1, keepdim=True)
            m1, m2 = m(gn), m(gn * n)
            du = rstd * (gn - m1 - n * m2)
            b = rstd * (eg + m(eg) + n.abs() * m(eg * n.abs() + 2 * (gn * n).abs()) + 2 * (n * m2).abs() + gn.abs() + m1.abs()) + du.abs()
            ref.update(du=du, part=part)
            cond.update(du=(torch.zeros_like(du), b), part=(pa, None))
    return ref, cond


# ---------------------------------------------------------------------------------------------------------------- model
def _fsum(t, dim):
    """An fp32 sum in another order than the device's: over the flipped axis."""
    return torch.flip(t, (dim,)).sum(dim, keepdim=True)


def _gelu32(c, v):
    return _gelu_fast(v) if c.dtype == W.BF16 else 0.5 * v * (1.0 + torch.erf(v * 0.70710678118654752440))


def _gelu_grad32(c, v):
    if c.dtype == W.BF16:
        return _gelu_grad_fast(v)
    return 0.5 * (1.0 + torch.erf(v * 0.70710678118654752440)) + v * 0.39894228040143267794 * torch.exp(-0.5 * v * v)


def _ln_group(c):
    """Rows one wave of the vector kernels normalises at once (64 / LPR) - 1 for the generic kernels."""
    vb = 16 if (c.ld or c.C % (16 // W.esize(c)) == 0) else 8
    need = c.pitch * W.esize(c) // vb
    if (c.pitch * W.esize(c)) % vb or need > 128:
        return 1
    return 64 // next(l for l in (8, 16, 32, 64) if need <= l or l == 64)


def _act_model(c, inp, defect):
    dt = torch_dtype(c)
    gy = inp["gy"].float()
    if "mult" in inp:
        gy = (gy * inp["mult"].float()).to(dt).float()
    rv = inp["ref"].float() if "ref" in inp else None
    if c.act == W.ACT_RELU:
        g = torch.where(rv > 0, gy, torch.zeros_like(gy))
    elif c.act == W.ACT_GELU:
        g = gy * _gelu_grad32(c, rv)
    elif c.act == W.ACT_ELU:
        g = gy * torch.where(rv > 0, torch.ones_like(rv), (rv if defect == "elu_no_div" else rv / c.act_scale) + 1.0)
    elif c.act == W.ACT_SIGMOID:
        sg = rv / c.act_scale
        g = gy * (sg * (1.0 - sg))
    else:
        g = gy
    g = g * torch.tensor(c.act_scale, dtype=torch.float32)
    if "scale" in inp:
        g = g * inp["scale"]
    return g.to(dt)


def _colsum_model(g):
    return pattern(g.shape[1]) + _fsum(g.float(), 0)[0]


def model(c, inp, defect=None):
    """The outputs of the call as the kernels compute them (see the module docstring); defect: one of DEFECTS, or None."""
    dt = torch_dtype(c)
    out = {}
    if c.call in ("LF", "LB"):
        C, ld, rows = c.C, c.pitch, c.rows
        x = inp["x"][:, :C].float()
        gamma, beta = inp.get("gamma", torch.ones(C)), inp.get("beta", torch.zeros(C))
        ragged = rows - (rows % _ln_group(c) or _ln_group(c))             # first row of the last (partial) row group
        if c.call == "LF":
            if defect == "lanes_beyond_c":                               # the padding lanes counted into the mean
                mu = _fsum(torch.nan_to_num(inp["x"].float(), nan=1.0), 1) / C
            else:
                mu = _fsum(x, 1) / C
            d = x - mu
            var = (_fsum(x * x, 1) / C - mu * mu) if defect == "onepass_var" else _fsum(d * d, 1) / C
            rs = torch.rsqrt(var + LN_EPS)
            o = d * rs * gamma + beta
            if c.gelu:
                o = _gelu32(c, o)
            if "residual" in inp:
                o = o + inp["residual"][:, :C].float()
            y = _pad(o, ld).to(dt)
            mean, rstd = mu[:, 0].clone(), rs[:, 0].clone()
            if defect == "pad_nonzero" and ld > C:
                y[:, C] = 1e-30
            if defect == "ragged_unwritten":
                y[ragged:], mean[ragged:], rstd[ragged:] = float("nan"), float("nan"), float("nan")
            out.update(y=y, mean=mean, rstd=rstd)
        else:
            mu, rs = inp["mean"][:, None], inp["rstd"][:, None]
            xh = (x - mu) * rs
            g = inp["gy"][:, :C].float()
            if c.gelu:
                g = g * _gelu_grad32(c, xh * gamma + beta)
            gw = g * gamma
            s1, s2 = _fsum(gw, 1) / C, _fsum(gw * xh, 1) / C
            o = rs * (gw - s1 - xh * s2)
            if "gskip" in inp:
                o = o + inp["gskip"][:, :C].float()
            if c.elu:
                xo = xh / rs + mu
                o = o * torch.where(xo > 0, torch.ones_like(xo), xo + 1.0)
            gx = _pad(o, ld).to(dt)
            if defect == "pad_nonzero" and ld > C:
                gx[:, C] = 1e-30
            if defect == "ragged_unwritten":
                gx[ragged:] = float("nan")
            out["gx"] = gx
            if c.dgamma:
                keep = torch.ones(rows, 1)
                if defect == "dgamma_wave":                              # one of 16 waves' partial sums is lost
                    keep[(torch.arange(rows) // _ln_group(c)) % 16 == 0] = 0.0
                out.update(dgamma=_fsum(g * xh * keep, 0)[0], dbeta=_fsum(g * keep, 0)[0])
    elif c.call in ("SF", "SM"):
        s = inp["x"].float() * torch.tensor(c.scale if c.call == "SM" else 1.0, dtype=torch.float32)
        if "mask" in inp:
            m = inp["mask"].bool()
            idx = torch.arange(c.rows) % c.rpm if defect == "mask_mod" else torch.arange(c.rows) // c.rpm
            s = s.masked_fill(m[idx.clamp_max(m.shape[0] - 1)], float("-inf"))
        live = c.L if defect != "softmax_tail" else 64 * ((c.L - 1) // 64)     # the last 64-element chunk is never loaded
        sl = s[:, :live]
        e = torch.exp(sl - sl.max(-1, keepdim=True).values)
        y = torch.full((c.rows, c.L), float("nan"))
        y[:, :live] = e * (1.0 / _fsum(e, 1))
        out["y"] = y.to(dt)
    elif c.call in ("SB", "SS"):
        scale = torch.tensor(c.scale if c.call == "SS" and defect != "scale_dropped" else 1.0, dtype=torch.float32)
        y, g = inp["y"].float(), inp["gy"].float()
        out["gx"] = (scale * y * (g - _fsum(y * g, 1))).to(dt)
    elif c.call in ("AB", "AC"):
        out["gx"] = _act_model(c, inp, defect)
        if c.call == "AC":
            out["dbias"] = _colsum_model(out["gx"])
    elif c.call == "CS":
        out["out"] = _colsum_model(inp["g"])
    elif c.call == "CB":
        vec = 16 // W.esize(c)
        for i, (rows, C) in enumerate(c.jobs):
            g = inp["g%d" % i].float()
            w = torch.ones(rows, 1)
            if defect == "block0_off_by_one":                            # `blockIdx > block0`: a job's first block runs as its predecessor's
                rpb = 256 // (C // vec)
                nblk = min(512, max(1, -(-rows // (rpb * 16))))
                first = (torch.arange(rows) // rpb) % nblk == 0
                if i > 0:
                    w[first] -= 1.0                                      # block 0 of this job never runs ...
                if i + 1 < len(c.jobs):
                    w[first & (torch.arange(rows) >= nblk * rpb)] += 1.0   # ... and the next job's runs here as block `nblk`
            out["out%d" % i] = pattern(C) + _fsum(g * w, 0)[0]
    else:
        B, L, C, S = c.B, c.L, c.C, c.S
        u = inp["u"].float()
        bounds = slice_bounds(L, S)
        if defect == "last_slice_short":
            last = max(s for s, (lo, hi) in enumerate(bounds) if hi > lo)
            bounds[last] = (bounds[last][0], bounds[last][1] - 1)
        part = torch.zeros(B, S, C, 2)
        if c.call == "IF":
            for s, (lo, hi) in enumerate(bounds):
                if hi > lo:
                    ms = _fsum(u[:, lo:hi], 1) / float(hi - lo)
                    part[:, s, :, 0], part[:, s, :, 1] = ms[:, 0], _fsum((u[:, lo:hi] - ms) ** 2, 1)[:, 0]
            nb = torch.tensor([float(max(hi - lo, 0)) for lo, hi in bounds])[None, :, None]
            mean = _fsum(nb * part[..., 0], 1) / float(L)
            between = 0.0 if defect == "merge_no_between" else nb * (part[..., 0] - mean) ** 2
            rstd = torch.rsqrt(_fsum(part[..., 1] + between, 1) / float(L) + LN_EPS)
            y = inp["a"].float() + _gelu32(c, (u - mean) * rstd)
            out.update(y=y.to(dt), stat=torch.stack([mean[:, 0], rstd[:, 0]], -1), part=part)
        else:
            mean, rstd = inp["stat"][:, None, :, 0], inp["stat"][:, None, :, 1]
            gy = inp["gy"].float()
            n = (u - mean) * rstd
            gn = gy * _gelu_grad32(c, n)
            for s, (lo, hi) in enumerate(bounds):
                if hi > lo:
                    part[:, s, :, 0], part[:, s, :, 1] = _fsum(gn[:, lo:hi], 1)[:, 0], _fsum(gn[:, lo:hi] * n[:, lo:hi], 1)[:, 0]
            m1, m2 = _fsum(part[..., 0], 1) * (1.0 / L), _fsum(part[..., 1], 1) * (1.0 / L)
            out.update(du=(rstd * (gn - m1 - n * m2)).to(dt), part=part)
    return out


# ------------------------------------------------------------------------------------------------------------ constants
def check(c, got, inp, what=None):
    """Every element of every output of the call against its bound; -> {output: worst ratio}."""
    ref, cond = reference(c, inp, got)
    assert set(got) == set(ref), (sorted(got), sorted(ref))
    worst = {}
    for name in sorted(ref):
        key = (OPERATION[c.call], name.rstrip("0123456789"), dtype_name(c))
        names = ("row", "column", "channel", "value")[:ref[name].dim()] if ref[name].dim() > 1 else ("channel",)
        worst[name] = assert_elementwise(got[name], ref[name], cond[name], C[key], names, u=out_unit(c, name), what="%s %s" % (what or c.text, name))
    return worst


def measure_c(table=None):
    """{(operation, output, type): largest model ratio} over the witness table, the run-time siblings of forms() included."""
    worst = {}
    for _, line in (W.load() if table is None else table):
        for c in forms(line):
            inp = inputs(c)
            got = model(c, inp)
            ref, cond = reference(c, inp, got)
            for name in ref:
                key = (OPERATION[c.call], name.rstrip("0123456789"), dtype_name(c))
                worst[key] = max(worst.get(key, 0.0), float(ratio(got[name], ref[name], cond[name], out_unit(c, name)).max()))
    return worst


def format_table(worst):
    lines = ["    operation        output   type   model max   C", "    --------------   ------   ----   ---------   ----"]
    for (op, out, dt), v in sorted(worst.items()):
        lines.append("    %-14s   %-6s   %-4s   %9.3f   %4.1f" % (op, out, dt, v, c_of(v)))
    return "\n".join(lines)


# C[(operation, output, type)]: twice the largest model ratio over the witness table, one decimal up; the module docstring shows
# format_table(MEASURED) (tests/test_row_witnesses.py checks both)
MEASURED = {
    ("act_bwd", "gx", "bf16"): 1.992,
    ("act_bwd", "gx", "f32"): 0.514,
    ("act_bwd_colsum", "dbias", "bf16"): 0.022,
    ("act_bwd_colsum", "dbias", "f32"): 0.033,
    ("act_bwd_colsum", "gx", "bf16"): 1.977,
    ("act_bwd_colsum", "gx", "f32"): 0.350,
    ("colsum", "out", "bf16"): 0.225,
    ("colsum", "out", "f32"): 0.472,
    ("inorm_bwd", "du", "bf16"): 1.989,
    ("inorm_bwd", "du", "f32"): 0.273,
    ("inorm_bwd", "part", "bf16"): 0.062,
    ("inorm_bwd", "part", "f32"): 0.296,
    ("inorm_fwd", "part", "bf16"): 0.601,
    ("inorm_fwd", "part", "f32"): 1.160,
    ("inorm_fwd", "stat", "bf16"): 0.667,
    ("inorm_fwd", "stat", "f32"): 0.421,
    ("inorm_fwd", "y", "bf16"): 1.991,
    ("inorm_fwd", "y", "f32"): 0.533,
    ("ln_bwd", "dbeta", "bf16"): 0.012,
    ("ln_bwd", "dbeta", "f32"): 0.003,
    ("ln_bwd", "dgamma", "bf16"): 0.005,
    ("ln_bwd", "dgamma", "f32"): 0.005,
    ("ln_bwd", "gx", "bf16"): 1.992,
    ("ln_bwd", "gx", "f32"): 1.428,
    ("ln_fwd", "mean", "bf16"): 0.486,
    ("ln_fwd", "mean", "f32"): 1.755,
    ("ln_fwd", "rstd", "bf16"): 0.858,
    ("ln_fwd", "rstd", "f32"): 0.829,
    ("ln_fwd", "y", "bf16"): 1.992,
    ("ln_fwd", "y", "f32"): 3.206,
    ("softmax_bwd", "gx", "bf16"): 0.989,
    ("softmax_bwd", "gx", "f32"): 2.936,
    ("softmax_fwd", "y", "bf16"): 1.980,
    ("softmax_fwd", "y", "f32"): 0.930,
}
C = {k: c_of(v) for k, v in MEASURED.items()}
__doc__ = __doc__.replace("@TABLE@", format_table(MEASURED))
