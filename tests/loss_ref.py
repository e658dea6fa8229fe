"""fp64 references, error bounds and rounding models of the loss and optimizer kernels of csrc/losses.hip and csrc/optim.hip (CPU only,
plain module; the instrument is the one of tests/attn_ref.py: assert_elementwise, ratio, FLOOR and the unit round-offs come from there).

These kernels have one launch stub per type, so there is no recorder and no witness table: ``cases()`` is a plain list.  A case is one
call sequence of a family - ``sqnorm``; ``adamw``; ``silog`` (sums, finalize, backward); ``seg_ce`` (sum, backward); ``anchor``
(forward, backward with and without datt) - at one shape, type and input regime; ``inputs(c)`` draws its operands with a generator
seeded by the case's text, in the storage type; every reference works on those rounded operands (the float hyper-parameters are
operands too: the reference widens the fp32 value the kernel receives), so the only error left between a kernel and its reference is
the kernel's own arithmetic.

* ``reference(c, inp, got=None)`` -> (ref, cond): per output the fp64 result of include/gwdepth.h's formula and the pair (A, B) of
      |got - ref| <= c u (|ref| + A + (2^-24 / u) B),      u = 2^-9 for a bf16 output, 2^-24 for an fp32 AND for an fp64 one
  (the fp64 outputs are sums of fp32 terms: their error is counted in fp32 units).  A zero bound demands an exact value.  Nothing
  goes through FakeDevice, F.cross_entropy, torch.optim or an fp32 intermediate.  The nearest source index is what CPU
  F.interpolate(index_map, mode="nearest") returns (``nearest_index``): the oracle of "as ATen".
      sqnorm    sq = prefill + sum g^2:  A = sum g^2   (each pair g0^2 + g1^2 is squared and added in fp32 before it becomes a double)
      adamw     KC = roundings on the way to gi = g coef: 1 without the clip branch (coef = grad_scale), 6 with it (the fp32 image
                of sqrt(sq), * grad_scale, + 1e-6, the division, * grad_scale, * g), + C[sqnorm] in the chained case (d coef / coef
                = d sq / 2 sq and A = sq);  with m' = m + (gi - m)(1 - b1), v' = v b2 + gi^2 (1 - b2), den = sqrt(v') / sqrt(bc2) + eps,
                update = (lr / bc1) m' / den:
                m: B = |m| + 2 |(gi - m)(1 - b1)| + (1 - b1) KC |gi|             (its two products)
                v: B = v b2 + (2 KC + 2) gi^2 (1 - b2)
                p: B = 2 |p| + (lr / bc1) (|m'| + B_m) / den + |update| (v' + B_v) / (2 v') (sqrt(v') / sqrt(bc2) / den) + k |update|,
                   k = 8: lr / bc1, rsqrtf, sqrtf, their product, + eps, the division, * step, the subtraction
                p16: the p THE KERNEL RETURNED rounded once to bf16: zero bound, bit-exact (like dbias against the returned gx in row_ref)
      silog     valid: float32(0.2) <= g < 10 (NaN, inf, 0, negatives are invalid);  d = log p - log g, or (p + log p) - (g + log g);
                e = 2 (|log p| + |log g|) + |d|   (the absolute fp32 error of the two logs and of the difference; the non-log form:
                3 (|log p| + |log g|) + |p| + |g| + |d|)
                sums[0]: A = sum e;   sums[1]: A = sum 2 |d| e;   sums[2] (the count): zero bound, exact
                finalize  loss = scale sqrt(s1 / n - lambda (s0 / n)^2) from the FED fp64 sums: one rounding, A = 0; all pixels invalid: NaN
                backward  c = 10 / sqrt(var) / n * loss_weight * gloss, f = 1 / p (log) or 1 + 1 / p:  gpred = c (d - lambda mean) f:
                          B = |c f| (e + |lambda mean|) + 5 |gpred|;   invalid pixels: zero bound, an exact 0
                chained   (the device's own sums): dvar = (C1 (|s1| + A1) + 2 lambda |mean| C0 (|s0| + A0)) / n, dmean = C0 (|s0| + A0) / n;
                          loss: A += scale dvar / (2 sqrt(var));   gpred: B += |gpred| dvar / (2 var) + |c f| lambda dmean
      seg_ce    term = mx + log(exp(a - mx) + exp(b - mx)) - chosen:  e = 2 (|a| + |b|) + 4  ((mx + log(..)) - chosen cancels when the
                chosen logit is the maximum; 4: exp, exp, the sum, log on [1, 2]);   sum = prefill + sum term:  A = sum e
                backward  c = gloss scale / P, pa, pb the two probabilities:  gl_x = c (p_x - [target = x]):
                          B = |c| (pa pb (4 + 2 |a - b|) + 2 p_x) + 3 |gl_x|
      anchor    pred = sum_r att an:  A = (1 + sqrt(R)) sum_r |att an|;   datt = gpred an:  B = |datt|;
                danchor = prefill + sum_p att gpred:  A = sqrt(P) sum_p |att gpred| + |prefill|   (fp32 atomics, as colsum in row_ref)
  The kernels that take sums as an operand (silog finalize / backward, adamw with sq) are fed the reference's fp64 sums (``feeds``),
  so each kernel is charged for its own arithmetic only; one chained case per family (silog, adamw) feeds the device's own sums.
* ``model(c, inp, defect=None)`` - the kernels' arithmetic in fp32 on the CPU with the ONE rounding at the store, every sum over the
  flipped order (another order than the device's).  It sizes C without a kernel's output and carries the injected defects of
  tests/test_loss_optim.py.

The constants.  ``measure_c()`` evaluates the model over the case list and takes the largest |model - ref| / bound per operation,
output and type; C is twice that, rounded up to one decimal (the factor 2 covers the device's summation order and its log / exp /
sqrt), as in row_ref.py, attn_ref.py and conv_ref.py.  Measured on the CPU, 2026-10:

@TABLE@

A kernel that needs more than its C has a defect or the bound lacks a term: neither is repaired by raising C.
"""
import math
import types
import zlib

import torch
import torch.nn.functional as F

from tests.attn_ref import FLOOR, U_BF16, U_F32, assert_elementwise, ratio        # noqa: F401  (the instrument)
from tests.conv_ref import c_of

DEFECTS = ("sqnorm_tail", "last_pass_sqnorm", "last_pass_adamw", "last_pass_seg_ce", "last_pass_silog_rows", "silog_col_loop", "exact_index",
           "gt_le_10", "lambda_missing", "nonlog_one_missing", "ce_no_div_p", "wd_dropped", "eps_inside_bc", "clip_always", "grad_scale_twice",
           "p16_stale", "danchor_overwrite", "anchor_16_lanes")
OPERATION = {"sq": "sqnorm", "p": "adamw", "m": "adamw", "v": "adamw", "p16": "adamw", "s0": "silog_sums", "s1": "silog_sums", "count": "silog_sums",
             "loss": "silog_finalize", "gpred": "silog_backward", "sum": "seg_ce_sum", "gl": "seg_ce_backward", "pred": "anchor_fwd",
             "datt": "anchor_bwd", "danchor": "anchor_bwd", "danchor_nodatt": "anchor_bwd"}
STORAGE_OUTPUTS = ("gpred", "gl", "datt")                   # outputs in the case's storage type; all others are fp32 or fp64

# launch constants of the .hip files (tests/test_loss_optim.py re-derives the passes from them)
SQNORM_PASS = 2048 * 256                                    # float4 vectors per pass of sqnorm_kernel
ADAMW_PASS = 4096 * 256
CE_PASS = 2048 * 256
SILOG_SUMS_ROWS, SILOG_BWD_ROWS = 512, 2048
BIG_SQNORM = 2 * 2097152 + 1200 + 3
BIG_ADAMW = 2 * 1048576 + 259
BIG_CE = 2 * 524288 + 300

SQ_PREFILL, CE_PREFILL = 3.25, 2.5
GLOSS, LOSS_WEIGHT, LAMBDA, CE_SCALE = 0.75, 1.5, 0.85, 0.4
BETA1, BETA2, EPS, MAX_NORM = 0.9, 0.999, 1e-8, 0.1
# name -> (lr, weight decay, grad_scale, step): the shipped hyper-parameters, and a set at which every term is visible above U_F32 |p|
PSETS = {"ship_a": (1e-4, 1e-4, 1.0, 1), "ship_b": (1e-5, 1e-4, 0.125, 3), "ship_c": (1e-4, 1e-4, 0.125, 1000), "ship_d": (1e-5, 1e-4, 1.0, 1000),
         "visible": (1e-2, 0.5, 1.0, 3), "visible_gs": (1e-2, 0.5, 0.125, 3)}


def f32(x):
    """The fp32 image of a Python number, as the double the kernel's float argument widens to."""
    return float(torch.tensor(x, dtype=torch.float32))


def torch_dtype(c):
    return torch.bfloat16 if c.dtype == "bf16" else torch.float32


def out_unit(c, name):
    return U_BF16 if (name in STORAGE_OUTPUTS and c.dtype == "bf16") else U_F32


def pattern(n):
    """What danchor holds before the call: fixed, non-zero, exact in fp32."""
    return 0.5 + 0.25 * (torch.arange(n) % 7).float()


# ---------------------------------------------------------------------------------------------------------------- cases
def _case(family, dtype, **kw):
    c = types.SimpleNamespace(family=family, dtype=dtype, **kw)
    c.text = "%s %s %s" % (family, dtype, " ".join("%s=%s" % (k, kw[k]) for k in sorted(kw)))
    c.id = c.text.replace(" ", "-")
    return c


def cases():
    """The case list (DESIGN.md section 16 gives the reason of every entry)."""
    out = []
    for n in (0, 1, 2, 3, 4, 5, 7, 1023, 1024, 1025, 1027, BIG_SQNORM):
        out.append(_case("sqnorm", "f32", n=n, outlier=0))
    out.append(_case("sqnorm", "f32", n=1027, outlier=1))
    sets = [(ps, clip, "") for ps in PSETS for clip in ("on", "off")]
    sets += [(ps, "on", var) for ps in ("ship_a", "visible") for var in ("nosq", "mn0", "nop16")]
    for n in (1, 255, 256, 257):
        for off in (0, 1, 3):
            for ps, clip, var in sets:
                out.append(_case("adamw", "f32", n=n, off=off, ps=ps, clip=clip, var=var, chained=0))
    for off, ps, clip, var in ((0, "visible", "off", ""), (1, "visible", "on", ""), (3, "ship_c", "off", ""), (3, "ship_a", "on", "nop16")):
        out.append(_case("adamw", "f32", n=BIG_ADAMW, off=off, ps=ps, clip=clip, var=var, chained=0))
    out.append(_case("adamw", "f32", n=257, off=0, ps="visible", clip="on", var="", chained=1))
    out.append(_case("adamw", "f32", n=BIG_ADAMW, off=0, ps="ship_a", clip="on", var="", chained=1))
    shapes = [(2, 5, w, 11, 2 * w + 1) for w in (1, 63, 64, 65, 128, 129, 256, 257, 300)]
    shapes += [(2, 14, 20, 62, 84), (2, 21, 21, 93, 93), (2, 6, 70, 6, 70), (3, 700, 20, 1400, 84)]
    for dt in ("f32", "bf16"):
        for B, h, w, H, W in shapes:
            for log_err in (1, 0):
                for regime in ("early", "converged"):
                    out.append(_case("silog", dt, B=B, h=h, w=w, H=H, W=W, log_err=log_err, regime=regime, chained=0))
        out.append(_case("silog", dt, B=2, h=5, w=65, H=11, W=131, log_err=1, regime="invalid", chained=0))
        out.append(_case("silog", dt, B=2, h=14, w=20, H=62, W=84, log_err=1, regime="converged", chained=1))
        for P in (1, 255, 256, 257):
            for kind in ("spread", "gap", "equal"):
                for target in ("zeros", "ones", "mixed"):
                    out.append(_case("seg_ce", dt, P=P, kind=kind, target=target))
        for kind in ("spread", "gap", "equal"):
            out.append(_case("seg_ce", dt, P=BIG_CE, kind=kind, target="mixed"))
        for R in (1, 7, 15, 16, 17, 80, 100, 128, 129, 255, 256):
            for P in (1, 15, 16, 17, 37, 1000):
                out.append(_case("anchor", dt, B=3, P=P, R=R))
        out.append(_case("anchor", dt, B=1, P=262437, R=7))
        out.append(_case("anchor", dt, B=1, P=8229, R=256))
    return out


def nbytes(c):
    """Bytes of all operands and outputs of the case."""
    e = 2 if c.dtype == "bf16" else 4
    if c.family == "sqnorm":
        return 4 * c.n + 8
    if c.family == "adamw":
        return c.n * (16 + (0 if c.var == "nop16" else 2)) + 8
    if c.family == "silog":
        return 2 * e * c.B * c.h * c.w + 4 * c.B * c.H * c.W + 32
    if c.family == "seg_ce":
        return c.P * (4 * e + 8) + 8
    return c.B * (2 * e * c.P * c.R + 8 * c.P + 8 * c.R)


# --------------------------------------------------------------------------------------------------------------- inputs
def _gen(c):
    return torch.Generator().manual_seed(zlib.crc32(c.text.encode()))


def nearest_index(h, w, H, W):
    """(h, w) flat source index of the nearest resize (H, W) -> (h, w), as ATen computes it: CPU F.interpolate of an index map."""
    assert H * W < 2 ** 24
    idx = torch.arange(H * W, dtype=torch.float32).view(1, 1, H, W)
    return F.interpolate(idx, size=(h, w), mode="nearest").view(h, w).long()


def exact_index(h, w, H, W):
    """The same map with the exact integer dst * in // out (the injected defect; differs for some size pairs)."""
    return (torch.arange(h) * H // h)[:, None] * W + (torch.arange(w) * W // w)[None, :]


def gt_specials():
    """The GT edge values: float32(0.2) (valid) and its predecessor, 10.0 (invalid) and its predecessor (valid), 0, a negative, +inf, NaN."""
    lo, hi = torch.tensor(0.2, dtype=torch.float32), torch.tensor(10.0, dtype=torch.float32)
    return torch.stack([lo, torch.nextafter(lo, torch.tensor(0.0)), hi, torch.nextafter(hi, torch.tensor(0.0)), torch.tensor(0.0),
                        torch.tensor(-1.5), torch.tensor(float("inf")), torch.tensor(float("nan"))])


def gt_valid(g):
    return (g >= torch.tensor(0.2, dtype=torch.float32)) & (g < 10.0)


def adamw_params(c):
    """The float arguments of the call, as Python floats (ctypes rounds them to fp32; the reference widens that fp32 value)."""
    lr, wd, gs, t = PSETS[c.ps]
    return dict(lr=lr, b1=BETA1, b2=BETA2, eps=EPS, wd=wd, bc1=1 - BETA1 ** t, bc2=1 - BETA2 ** t, max_norm=0.0 if c.var == "mn0" else MAX_NORM, gs=gs)


def inputs(c):
    """The operands of a case: a dict of CPU tensors in the storage type."""
    g, dt = _gen(c), torch_dtype(c)
    rnd = lambda *shape: torch.randn(*shape, generator=g)
    uni = lambda *shape: torch.rand(*shape, generator=g)
    if c.family == "sqnorm":
        x = rnd(c.n)
        if c.outlier:
            x[::251] *= 1e4
        if c.n == BIG_SQNORM:                                    # the three tail elements stay visible above the bound of a sum of 4 M squares
            x[-3:] = torch.tensor([1.5, -1.5, 1.5])
        return {"g": x}
    if c.family == "adamw":
        n, prm = c.n, adamw_params(c)
        i = torch.arange(n)
        g0 = rnd(n)
        g0[i % 7 == 3] = 0.0
        norm = float(g0.double().norm()) * prm["gs"]
        target = MAX_NORM * (10.0 if c.clip == "on" else 0.1)    # ||g|| grad_scale: ten times max_norm, or a tenth of it
        gr = (g0.double() * (target / norm)).float()
        sg = target / prm["gs"] / math.sqrt(n)                   # the size of one gradient element
        v = (rnd(n) * sg) ** 2
        m = rnd(n) * sg * 0.5
        v[i % 7 == 3] = 0.0                                      # with g = 0: the denominator is eps alone
        m[i % 7 == 3] = 1e-9 * (1.0 + (i[i % 7 == 3] % 5).float())
        return {"p": rnd(n), "g": gr, "m": m, "v": v}
    if c.family == "silog":
        B, h, w, H, W = c.B, c.h, c.w, c.H, c.W
        src = nearest_index(h, w, H, W).flatten()
        lo = 0.3 + 9.0 * uni(B, h * w)
        pos = torch.arange(B * h * w).view(B, h * w)
        sp = gt_specials()
        if c.regime == "invalid":
            lo = sp[torch.tensor([1, 2, 4, 5, 6, 7])][pos % 6]
        else:
            k = pos % 5 == 2
            lo[k] = sp[(pos // 5) % 8][k]
        full = 0.3 + 9.0 * uni(B, H * W)                         # the pixels the resize does not pick: other depths, a tenth NaN
        full[uni(B, H * W) < 0.1] = float("nan")
        full[:, src] = lo
        lo = full[:, src]
        valid = gt_valid(lo)
        assert bool(valid.any()) == (c.regime != "invalid"), c.text             # the valid share stays > 0 (all invalid: the one such case)
        if c.regime == "early":
            pred = 0.05 + 0.9 * uni(B, h * w)
        else:
            pred = torch.where(valid, lo * (1.0 + 1e-3 * (rnd(B, h * w) + 0.5)), 1.0 + uni(B, h * w))
        return {"pred": pred.view(B, h, w).to(dt), "gt": full.view(B, H, W)}
    if c.family == "seg_ce":
        P = c.P
        i = torch.arange(P)
        t = {"zeros": torch.zeros(P, dtype=torch.int64), "ones": torch.ones(P, dtype=torch.int64), "mixed": (uni(P) < 0.5).long()}[c.target]
        if c.kind == "spread":
            x = rnd(P, 2) * 2.0
        elif c.kind == "equal":
            x = (rnd(P, 1) * 3.0).expand(P, 2).clone()
        else:
            a = rnd(P) * 2.0
            x = torch.stack([a, a + torch.where(uni(P) < 0.5, 80.0, -80.0)], -1)
            if c.dtype == "bf16":                                # the bf16 range: +-1.5e38, the chosen logit the larger one (the term is 0,
                k = i % 17 == 5                                  # so that these pixels do not drown the sum's bound)
                big = torch.where(t == 0, 1.5e38, -1.5e38)
                x[k] = torch.stack([big, -big], -1)[k]
        return {"logits": x.to(dt), "target": t}
    B, P, R = c.B, c.P, c.R
    return {"att": torch.softmax(rnd(B, P, R) * 2.0, -1).to(dt), "anchor": 0.2 + 9.8 * uni(B, R), "gpred": rnd(B, P)}


# ------------------------------------------------------------------------------------------------------------ reference
def _one(x):
    return torch.as_tensor(x, dtype=torch.float64).reshape(1)


def _zero_like(t):
    return torch.zeros_like(t, dtype=torch.float64)


def _silog_terms(c, inp, src=None):
    """fp64 d, e (0 where invalid), valid, p of the (B, h w) prediction pixels."""
    B = c.B
    src = nearest_index(c.h, c.w, c.H, c.W).flatten() if src is None else src
    g32 = inp["gt"].view(B, -1)[:, src]
    valid = gt_valid(g32)
    p = inp["pred"].double().view(B, -1)
    ps, gs = torch.where(valid, p, torch.ones_like(p)), torch.where(valid, g32.double(), torch.ones_like(p))
    lp, lg = torch.log(ps), torch.log(gs)
    if c.log_err:
        d = lp - lg
        e = 2 * (lp.abs() + lg.abs()) + d.abs()
    else:
        d = (ps + lp) - (gs + lg)
        e = 3 * (lp.abs() + lg.abs()) + ps.abs() + gs.abs() + d.abs()
    z = torch.zeros_like(d)
    return torch.where(valid, d, z), torch.where(valid, e, z), valid, ps


def _adamw_coef(c, prm, sq):
    """fp64 coef, and whether the clip branch is taken."""
    gs, mn = f32(prm["gs"]), f32(prm["max_norm"])
    if sq is None or not mn > 0:
        return gs, False
    total = math.sqrt(float(sq)) * gs
    return gs * min(mn / (total + f32(1e-6)), 1.0), True


def feeds(c, inp):
    """The fp64 sums a case's later kernels are fed (None: they take the device's own - the chained cases - or none at all)."""
    if c.family == "adamw" and c.var != "nosq" and not c.chained:
        return {"sq": _one((inp["g"].double() ** 2).sum())}
    if c.family == "silog" and not c.chained:
        d, _, valid, _ = _silog_terms(c, inp)
        return {"sums": torch.stack([d.sum(), (d * d).sum(), valid.sum().double()])}
    return None


def reference(c, inp, got=None):
    """-> (ref, cond) over the outputs of the case.  got: the outputs under test (p16 is checked against got's p)."""
    ref, cond = {}, {}
    if c.family == "sqnorm":
        s = (inp["g"].double() ** 2).sum()
        ref["sq"], cond["sq"] = _one(SQ_PREFILL + s), (_one(s), None)
    elif c.family == "adamw":
        prm = adamw_params(c)
        lr, b1, b2, eps, wd, bc1, bc2 = (f32(prm[k]) for k in ("lr", "b1", "b2", "eps", "wd", "bc1", "bc2"))
        p, g, m, v = (inp[k].double() for k in ("p", "g", "m", "v"))
        sq = None if c.var == "nosq" else (g ** 2).sum()
        coef, clip = _adamw_coef(c, prm, sq)
        kc = (6.0 if clip else 1.0) + (C[("sqnorm", "sq", "f32")] if c.chained else 0.0)
        gi = g * coef
        m2 = m + (gi - m) * (1 - b1)
        v2 = v * b2 + gi * gi * (1 - b2)
        bm = m.abs() + 2 * ((gi - m) * (1 - b1)).abs() + (1 - b1) * kc * gi.abs()
        bv = v * b2 + (2 * kc + 2) * gi * gi * (1 - b2)
        step, root = lr / bc1, torch.sqrt(v2) / math.sqrt(bc2)
        den = root + eps
        upd = step * m2 / den
        p2 = p * (1 - lr * wd) - upd
        rel_v = torch.where(v2 > 0, (v2 + bv) / (2 * v2.clamp_min(1e-300)), torch.zeros_like(v2))
        bp = 2 * p.abs() + step * (m2.abs() + bm) / den + upd.abs() * rel_v * (root / den) + 8 * upd.abs()
        ref.update(p=p2, m=m2, v=v2)
        cond.update(p=(_zero_like(p), bp), m=(_zero_like(p), bm), v=(_zero_like(p), bv))
        if c.var != "nop16":
            ret = p2.float() if got is None else got["p"].detach().cpu()
            ref["p16"], cond["p16"] = ret.to(torch.bfloat16).double(), (_zero_like(p), None)
    elif c.family == "silog":
        d, e, valid, ps = _silog_terms(c, inp)
        s0, s1, n = d.sum(), (d * d).sum(), valid.sum().double()
        a0, a1 = e.sum(), (2 * d.abs() * e).sum()
        ref.update(s0=_one(s0), s1=_one(s1), count=_one(n))
        cond.update(s0=(_one(a0), None), s1=(_one(a1), None), count=(_one(0.0), None))
        shape = (c.B, c.h, c.w)
        if float(n) == 0:
            ref.update(loss=_one(float("nan")), gpred=torch.zeros(shape, dtype=torch.float64))
            cond.update(loss=(_one(0.0), None), gpred=(torch.zeros(shape, dtype=torch.float64), None))
            return ref, cond
        lam, scale = f32(LAMBDA), f32(10.0 * LOSS_WEIGHT)
        mean = s0 / n
        var = s1 / n - lam * mean * mean
        dvar = dmean = 0.0
        if c.chained:
            dt = c.dtype
            c0, c1 = C[("silog_sums", "s0", dt)], C[("silog_sums", "s1", dt)]
            dmean = c0 * (s0.abs() + a0) / n
            dvar = (c1 * (s1.abs() + a1) + 2 * lam * mean.abs() * c0 * (s0.abs() + a0)) / n
        ref["loss"], cond["loss"] = _one(torch.sqrt(var) * scale), (_one(scale * dvar / (2 * torch.sqrt(var))), None)
        cc = 10.0 / torch.sqrt(var) / n * f32(LOSS_WEIGHT) * f32(GLOSS)
        f = 1.0 / ps if c.log_err else 1.0 + 1.0 / ps
        gp = torch.where(valid, cc * (d - lam * mean) * f, torch.zeros_like(d))
        b = (cc * f).abs() * (e + (lam * mean).abs()) + 5 * gp.abs() + gp.abs() * dvar / (2 * var) + (cc * f).abs() * lam * dmean
        ref["gpred"], cond["gpred"] = gp.view(shape), (torch.zeros(shape, dtype=torch.float64), torch.where(valid, b, torch.zeros_like(b)).view(shape))
    elif c.family == "seg_ce":
        x, t = inp["logits"].double(), inp["target"]
        a, b = x[:, 0], x[:, 1]
        mx = torch.maximum(a, b)
        ea, eb = torch.exp(a - mx), torch.exp(b - mx)
        term = torch.log(ea + eb) + (mx - torch.where(t != 0, b, a))
        e = 2 * (a.abs() + b.abs()) + 4
        ref["sum"], cond["sum"] = _one(CE_PREFILL + term.sum()), (_one(e.sum()), None)
        cc = f32(GLOSS) * f32(CE_SCALE) / c.P
        pa, pb = ea / (ea + eb), eb / (ea + eb)
        gl = cc * torch.stack([torch.where(t == 0, -pb, pa), torch.where(t != 0, -pa, pb)], -1)
        pp = (pa * pb * (4 + 2 * (a - b).abs()))[:, None] + 2 * torch.stack([pa, pb], -1)
        ref["gl"], cond["gl"] = gl, (_zero_like(gl), abs(cc) * pp + 3 * gl.abs())
    else:
        att, an, gp = inp["att"].double(), inp["anchor"].double(), inp["gpred"].double()
        t = att * an[:, None, :]
        ref["pred"], cond["pred"] = t.sum(-1), ((1 + math.sqrt(c.R)) * t.abs().sum(-1), None)
        datt = gp[:, :, None] * an[:, None, :]
        ref["datt"], cond["datt"] = datt, (_zero_like(datt), datt.abs())
        u = att * gp[:, :, None]
        pre = pattern(c.R).double()[None].expand(c.B, c.R)
        ref["danchor"], cond["danchor"] = pre + u.sum(1), (math.sqrt(c.P) * u.abs().sum(1) + pre, None)
        ref["danchor_nodatt"], cond["danchor_nodatt"] = ref["danchor"], cond["danchor"]
    return ref, cond


# ---------------------------------------------------------------------------------------------------------------- model
def _fsum(t, dim=0):
    """A sum in another order than the device's: over the flipped axis."""
    return torch.flip(t, (dim,)).sum(dim)


def _partial_pass_start(n, per_pass):
    """First index of the last, partial grid-stride pass over n items (n: no such pass)."""
    return (n // per_pass) * per_pass if n > per_pass and n % per_pass else n


def _t32(x):
    return torch.tensor(x, dtype=torch.float32)


def model_sqnorm(g, defect=None):
    n = g.numel()
    n4 = n // 4
    v = g[:4 * n4].view(n4, 4)
    if defect == "last_pass_sqnorm":
        v = v[:_partial_pass_start(n4, SQNORM_PASS)]
    s = _fsum((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]).double() + (v[:, 2] * v[:, 2] + v[:, 3] * v[:, 3]).double())
    if defect != "sqnorm_tail":
        s = s + _fsum(g[4 * n4:].double() ** 2)
    return s


def model(c, inp, defect=None):
    """The outputs of the case as the kernels compute them (see the module docstring); defect: one of DEFECTS, or None."""
    dt = torch_dtype(c)
    fed = feeds(c, inp)
    out = {}
    if c.family == "sqnorm":
        out["sq"] = _one(SQ_PREFILL + model_sqnorm(inp["g"], defect))
    elif c.family == "adamw":
        prm = adamw_params(c)
        lr, b1, b2, eps, wd, bc1, bc2, mn, gs = (_t32(prm[k]) for k in ("lr", "b1", "b2", "eps", "wd", "bc1", "bc2", "max_norm", "gs"))
        p, g, m, v = inp["p"], inp["g"], inp["m"], inp["v"]
        sq = model_sqnorm(g) if c.chained else (None if fed is None else fed["sq"][0])
        coef = gs.clone()
        if sq is not None and float(mn) > 0:
            total = torch.sqrt(sq).float() * gs
            ratio_ = mn / (total + _t32(1e-6))
            coef = coef * (ratio_ if defect == "clip_always" else torch.minimum(ratio_, _t32(1.0)))
        if defect == "grad_scale_twice":
            coef = coef * gs
        step, rs2 = lr / bc1, torch.rsqrt(bc2)
        gi = g * coef
        pi = p if defect == "wd_dropped" else p * (_t32(1.0) - lr * wd)
        mi = m + (gi - m) * (_t32(1.0) - b1)
        vi = v * b2 + gi * gi * (_t32(1.0) - b2)
        den = (torch.sqrt(vi) + eps) * rs2 if defect == "eps_inside_bc" else torch.sqrt(vi) * rs2 + eps
        pi = pi - step * mi / den
        p16 = (p if defect == "p16_stale" else pi).to(torch.bfloat16)
        if defect == "last_pass_adamw":
            k = _partial_pass_start(c.n, ADAMW_PASS)
            pi, mi, vi, p16 = (torch.cat([new[:k], old[k:]]) for new, old in ((pi, p), (mi, m), (vi, v), (p16, torch.full_like(p16, float("nan")))))
        out.update(p=pi, m=mi, v=vi)
        if c.var != "nop16":
            out["p16"] = p16
    elif c.family == "silog":
        B, h, w = c.B, c.h, c.w
        src = (exact_index if defect == "exact_index" else nearest_index)(h, w, c.H, c.W).flatten()
        g32 = inp["gt"].view(B, -1)[:, src]
        valid = ((g32 >= _t32(0.2)) & (g32 <= 10.0)) if defect == "gt_le_10" else gt_valid(g32)
        p = inp["pred"].float().view(B, -1)
        ps, gs_ = torch.where(valid, p, torch.ones_like(p)), torch.where(valid, g32, torch.ones_like(p))
        d = (torch.log(ps) - torch.log(gs_)) if c.log_err else ((ps + torch.log(ps)) - (gs_ + torch.log(gs_)))
        block = 256 if w > 128 else (128 if w > 64 else 64)
        ran_s = torch.ones(B * h, w, dtype=torch.bool)               # (row, column) pairs the sums / the backward kernel visit
        ran_b = ran_s.clone()
        if defect == "silog_col_loop":
            ran_s[:, block:], ran_b[:, block:] = False, False
        if defect == "last_pass_silog_rows":
            ran_s[_partial_pass_start(B * h, SILOG_SUMS_ROWS):] = False
            ran_b[_partial_pass_start(B * h, SILOG_BWD_ROWS):] = False
        vs = (valid & ran_s.view(B, -1)).flatten()
        dd = d.flatten()[vs].double()
        mine = torch.stack([_fsum(dd), _fsum(dd * dd), vs.sum().double()])
        out.update(s0=mine[0:1], s1=mine[1:2], count=mine[2:3])
        sums = mine if fed is None else fed["sums"]
        lam = _t32(LAMBDA).double()
        n = sums[2]
        mean = sums[0] / n
        var = sums[1] / n - lam * mean * mean
        out["loss"] = (torch.sqrt(var) * _t32(10.0 * LOSS_WEIGHT).double()).float().reshape(1)
        cc = (10.0 / torch.sqrt(var) / n).float() * _t32(LOSS_WEIGHT) * _t32(GLOSS)
        lm = (mean if defect == "lambda_missing" else lam * mean).float()
        f = 1.0 / ps if (c.log_err or defect == "nonlog_one_missing") else 1.0 + 1.0 / ps
        gp = torch.where(valid, cc * (d - lm) * f, torch.zeros_like(d)).to(dt)
        gp = torch.where(ran_b.view(B, -1), gp, torch.full_like(gp, float("nan")))
        out["gpred"] = gp.view(B, h, w)
    elif c.family == "seg_ce":
        x, t = inp["logits"].float(), inp["target"]
        a, b = x[:, 0], x[:, 1]
        mx = torch.maximum(a, b)
        ea, eb = torch.exp(a - mx), torch.exp(b - mx)
        term = ((mx + torch.log(ea + eb)) - torch.where(t != 0, b, a)).double()
        k = _partial_pass_start(c.P, CE_PASS) if defect == "last_pass_seg_ce" else c.P
        out["sum"] = _one(CE_PREFILL + _fsum(term[:k]))
        cc = _t32(GLOSS) * _t32(CE_SCALE)
        if defect != "ce_no_div_p":
            cc = cc / _t32(float(c.P))
        inv = 1.0 / (ea + eb)
        one, zero = torch.ones_like(a), torch.zeros_like(a)
        gl = torch.stack([cc * (ea * inv - torch.where(t != 0, zero, one)), cc * (eb * inv - torch.where(t != 0, one, zero))], -1).to(dt)
        gl[k:] = float("nan")
        out["gl"] = gl
    else:
        att, an, gp = inp["att"].float(), inp["anchor"], inp["gpred"]
        t = att * an[:, None, :]
        out["pred"] = _fsum(t[..., :16] if defect == "anchor_16_lanes" else t, 2)
        out["datt"] = (gp[:, :, None] * an[:, None, :]).to(dt)
        pre = torch.zeros(c.B, c.R) if defect == "danchor_overwrite" else pattern(c.R)[None].expand(c.B, c.R)
        out["danchor"] = pre + _fsum(att * gp[:, :, None], 1)
        out["danchor_nodatt"] = out["danchor"].clone()
    return out


# ------------------------------------------------------------------------------------------------------------ constants
def key_of(c, name):
    return (OPERATION[name], "danchor" if name == "danchor_nodatt" else name, c.dtype)


def check(c, got, inp, what=None):
    """Every element of every output of the case against its bound; -> {output: worst ratio}."""
    ref, cond = reference(c, inp, got)
    assert set(got) == set(ref), (sorted(got), sorted(ref))
    worst = {}
    for name in sorted(ref):
        label = "%s %s" % (what or c.text, name)
        if bool(torch.isnan(ref[name]).all()):                   # the all-invalid SiLog: NaN by definition
            assert bool(torch.isnan(got[name]).all()), "%s: %d elements outside: NaN expected, got %r" % (label, got[name].numel(), got[name])
            worst[name] = 0.0
            continue
        names = ("image", "row", "column")[:ref[name].dim()] if ref[name].dim() > 1 else ("element",)
        worst[name] = assert_elementwise(got[name], ref[name], cond[name], C[key_of(c, name)], names, u=out_unit(c, name), what=label)
    return worst


def measure_c(case_list=None):
    """{(operation, output, type): largest model ratio} over the case list."""
    worst = {}
    for c in (cases() if case_list is None else case_list):
        inp = inputs(c)
        got = model(c, inp)
        ref, cond = reference(c, inp, got)
        for name in ref:
            if bool(torch.isnan(ref[name]).all()):
                continue
            r = ratio(got[name], ref[name], cond[name], out_unit(c, name))
            worst[key_of(c, name)] = max(worst.get(key_of(c, name), 0.0), float(r.max()) if r.numel() else 0.0)
    return worst


def format_table(worst):
    lines = ["    operation         output    type   model max   C", "    ---------------   -------   ----   ---------   ----"]
    for (op, out, dt), v in sorted(worst.items()):
        lines.append("    %-15s   %-7s   %-4s   %9.3f   %4.1f" % (op, out, dt, v, c_of(v)))
    return "\n".join(lines)


# C[(operation, output, type)]: twice the largest model ratio over the case list, one decimal up; the module docstring shows
# format_table(MEASURED) (tests/test_loss_optim.py checks both)
MEASURED = {
    ("adamw", "m", "f32"): 0.506,
    ("adamw", "p", "f32"): 0.684,
    ("adamw", "p16", "f32"): 0.000,
    ("adamw", "v", "f32"): 0.993,
    ("anchor_bwd", "danchor", "bf16"): 0.663,
    ("anchor_bwd", "danchor", "f32"): 0.774,
    ("anchor_bwd", "datt", "bf16"): 1.992,
    ("anchor_bwd", "datt", "f32"): 0.500,
    ("anchor_fwd", "pred", "bf16"): 1.093,
    ("anchor_fwd", "pred", "f32"): 0.918,
    ("seg_ce_backward", "gl", "bf16"): 1.989,
    ("seg_ce_backward", "gl", "f32"): 0.744,
    ("seg_ce_sum", "sum", "bf16"): 0.052,
    ("seg_ce_sum", "sum", "f32"): 0.191,
    ("silog_backward", "gpred", "bf16"): 1.988,
    ("silog_backward", "gpred", "f32"): 0.897,
    ("silog_finalize", "loss", "bf16"): 0.942,
    ("silog_finalize", "loss", "f32"): 0.898,
    ("silog_sums", "count", "bf16"): 0.000,
    ("silog_sums", "count", "f32"): 0.000,
    ("silog_sums", "s0", "bf16"): 0.051,
    ("silog_sums", "s0", "f32"): 0.087,
    ("silog_sums", "s1", "bf16"): 0.136,
    ("silog_sums", "s1", "f32"): 0.151,
    ("sqnorm", "sq", "f32"): 0.151,
}
C = {k: c_of(v) for k, v in MEASURED.items()}
__doc__ = __doc__.replace("@TABLE@", format_table(MEASURED))
