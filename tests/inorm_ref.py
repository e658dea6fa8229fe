"""fp64 reference, error bounds and fp32 model of the instance-norm GELU kernels (csrc/inorm.hip, gwd_inorm_gelu_forward / _backward;
CPU only, plain module; the instrument is the one of tests/attn_ref.py).

A case is (type, B, L, C, S, regime, chained); tensors are (B, L, C), statistics run over the L positions of an image per channel.
``inputs(c)`` draws a, u, gy in the storage type with a generator seeded by the case's text; every reference works on those rounded
operands.  Regimes: ``plain`` (u = 1.5 + 0.7 z), ``offset`` (f32: u = 100 + 0.05 z; bf16: the representable 96 + k / 2, k in -3..3: a
mean far above the spread), ``const`` (channel 1 of every image is the constant 0.75 next to live channels: var = 0, rstd =
1 / sqrt(eps)), ``spike`` (plain u, gy with one element of 1000 per image).

* ``reference(c, inp, got=None)`` -> (ref, cond), all fp64; per output the pair (A, B) of
      |got - ref| <= c u (|ref| + A + (2^-24 / u) B),   u = 2^-9 for a bf16 output, 2^-24 for an fp32 one (stat is fp32 in both types)
  With mu = sum u / L, var = sum (u - mu)^2 / L, rstd = 1 / sqrt(var + eps), n = (u - mu) rstd, Phi / phi the normal distribution and
  density (exact erf):
      dmu   = sum |u| / L                                      (a sum of L fp32 terms, then the weighted merge of the slice means)
      dvar  = 3 var + 2 sqrt(var_b) dmu                        (var_b = sum_s n_s (mean_s - mu)^2 / L <= var: the merge squares the
                                                                difference of two means that each carry dmu; the slice M2 are two-pass)
      stat  mean: B = dmu;     rstd: B = rstd dvar / (2 (var + eps)) + 2 rstd     (rsqrtf and the division)
      dn    = rstd (|u| + dmu) + |n| dvar / (2 (var + eps)) + |n|
      y     = a + n Phi(n):    B = |a| + |n Phi(n)| + |Phi(n) + n phi(n)| dn + (1 + FAST) |n|
  (1: Phi = 0.5 (1 + erf) carries an ABSOLUTE error of a unit - the sum cancels for n << 0 - which n multiplies.)
  FAST prices the bf16 kernels' erf (Abramowitz & Stegun 7.1.26, |error| <= 1.5e-7 = 2.6 x 2^-24, halved in Phi, plus the hardware
  reciprocal and exponential at about one unit each): FAST = 4 for bf16, 0 for f32.  The model's ``exact_erf`` variant - erf where
  the bf16 kernel uses its fast form - stays inside the same bound, which shows that the bound prices the fast form.
  The backward is fed ``stat_fed``: the reference's stat rounded to fp32 (the chained cases: the stat the device returned, which the
  forward check has bounded), and the reference evaluates the header's formula on exactly that operand, so the kernel is charged
  for its own arithmetic only:  n = (u - mean) rstd, gn = gy (Phi(n) + n phi(n)), m1 = sum gn / L, m2 = sum gn n / L,
      du    = rstd (gn - m1 - n m2)
      dnb   = 2 |n|;   dgn = |gy| (|phi(n) (2 - n^2)| dnb + 4 |Phi + n phi| + 1 + FAST (1 + |n|))
      dm1   = sum (dgn + |gn|) / L;   dm2 = sum (dgn |n| + |gn| dnb + |gn n|) / L
      B     = rstd (dgn + dm1 + |n| dm2 + |m2| dnb + 2 |gn| + 2 |m1| + 3 |n m2|)
* ``model(c, inp, defect=None)``: the kernels' arithmetic in fp32 on the CPU - slice bounds, two-pass slice statistics, the weighted
  merge, the apply - with the device's depth of summation in another order (a thread's rows last to first, the partial sums in
  a tree of adjacent pairs where the device pairs t with t + stride, the slices last to first), one rounding at the store.  Defects: ``one_pass`` (M2_s = sum u^2 - n mean_s^2), ``merge_unweighted``
  (the slice sizes ignored), ``empty_as_per`` (an empty or clamped slice counted as ceil(L / S) rows), ``m2_no_div`` (the backward's
  m2 not divided by L); ``exact_erf`` is the variant above and must pass.

The constants.  ``measure_c()`` takes the largest |model - ref| / bound per (operation, output, type) over the case list; C is twice
that, rounded up to one decimal.  Measured on the CPU, 2026-10:

@TABLE@

A kernel that needs more than its C has a defect or the bound lacks a term: neither is repaired by raising C.
"""
import math
import types
import zlib

import torch

from tests.attn_ref import FLOOR, U_BF16, U_F32, assert_elementwise, ratio        # noqa: F401  (the instrument)
from tests.conv_ref import c_of

DEFECTS = ("one_pass", "merge_unweighted", "empty_as_per", "m2_no_div")
VARIANTS = ("exact_erf",)
NT, GRID_CAP, MAX_S, EPS = 256, 256, 4096, 1e-5                 # csrc/inorm.hip
OPERATION = {"y": "inorm_fwd", "mean": "inorm_fwd", "rstd": "inorm_fwd", "du": "inorm_bwd"}


def torch_dtype(c):
    return torch.bfloat16 if c.dtype == "bf16" else torch.float32


def vn_of(c):
    return 8 if c.dtype == "bf16" else 4


def out_unit(c, name):
    return U_BF16 if (name in ("y", "du") and c.dtype == "bf16") else U_F32


def slice_bounds(L, S, s):
    per = (L + S - 1) // S
    lo = s * per
    hi = min(lo + per, L)
    return min(lo, L), hi


def launch(c):
    """The launch arithmetic of gwd_inorm_gelu_forward / _backward: CG, rows per block pass, the apply grid and whether it was capped,
    the slice sizes."""
    cg = c.C // vn_of(c)
    rows = NT // cg
    nb = (c.L + rows - 1) // rows
    sizes = [max(0, slice_bounds(c.L, c.S, s)[1] - slice_bounds(c.L, c.S, s)[0]) for s in range(c.S)]
    return types.SimpleNamespace(CG=cg, rows=rows, blocks=nb, grid=min(nb, GRID_CAP), capped=nb > GRID_CAP, sizes=sizes)


def _case(dtype, B, L, C, S, regime="plain", chained=0):
    c = types.SimpleNamespace(dtype=dtype, B=B, L=L, C=C, S=S, regime=regime, chained=chained)
    c.text = "inorm %s B=%d L=%d C=%d S=%d %s chained=%d" % (dtype, B, L, C, S, regime, chained)
    c.id = c.text.replace(" ", "-")
    return c


def cases():
    out = []
    for dt, c1, c256, cw in (("f32", 4, 1024, 16), ("bf16", 8, 2048, 32)):
        out += [_case(dt, 2, 300, c1, 3),                      # CG = 1: 256 rows per pass, L > NT / CG
                _case(dt, 1, 3, c256, 2),                      # CG = 256: no tree step, a slot is one row; L < rows of slice 0 + 1
                _case(dt, 2, 300, c256, 3),                    # CG = 256 and more than 256 blocks of one row: the grid cap
                _case(dt, 2, 441, cw, 32),                     # the workload's shape
                _case(dt, 2, 441, cw, 32, "offset"),
                _case(dt, 2, 441, cw, 32, "const"),
                _case(dt, 2, 441, cw, 32, "spike"),
                _case(dt, 2, 441, cw, 32, "plain", 1),         # chained: the backward takes the device's own stat
                _case(dt, 2, 7, cw, 2),                        # L < NT / CG
                _case(dt, 3, 100, cw, 1),                      # S = 1, B = 3
                _case(dt, 2, 5, 16, 32),                       # S > L: 27 empty slices
                _case(dt, 2, 9, cw, 4),                        # 3 3 3 0
                _case(dt, 2, 5, cw, 4),                        # 2 2 1 0
                _case(dt, 2, 10, cw, 4),                       # 3 3 3 1
                _case(dt, 2, 10, cw, 4, "offset"),
                _case(dt, 3, 37, cw, 7, "const")]
    return out


def rejected():
    """(entry point arguments dtype, C, S) -> return code, at B = 2, L = 10."""
    return [("f32", 6, 2, -4), ("f32", 12, 2, -4), ("f32", 16, 4097, -4), ("bf16", 12, 2, -4), ("bad", 16, 2, -2)]


# ---------------------------------------------------------------------------------------------------------------- inputs
def _gen(c):
    g = torch.Generator()
    g.manual_seed(zlib.crc32(c.text.encode()))
    return g


def inputs(c):
    g, dt = _gen(c), torch_dtype(c)
    shape = (c.B, c.L, c.C)
    z = torch.randn(shape, generator=g, dtype=torch.float64)
    if c.regime == "offset":
        u = (100.0 + 0.05 * z) if c.dtype == "f32" else 96.0 + 0.5 * torch.randint(-3, 4, shape, generator=g).double()
    else:
        u = 1.5 + 0.7 * z
    if c.regime == "const":
        u[:, :, 1] = 0.75
    a = torch.randn(shape, generator=g, dtype=torch.float64)
    gy = torch.randn(shape, generator=g, dtype=torch.float64)
    if c.regime == "spike":
        for b in range(c.B):
            gy[b, (3 * b + 1) % c.L, (5 * b + 2) % c.C] = 1000.0
    return {"a": a.to(dt), "u": u.to(dt), "gy": gy.to(dt)}


# ------------------------------------------------------------------------------------------------------------- reference
def _phi(n):
    return torch.exp(-0.5 * n * n) / math.sqrt(2 * math.pi)


def _Phi(n):
    return 0.5 * (1 + torch.erf(n / math.sqrt(2)))


def stat_fed(c, inp):
    """What the un-chained backward receives: the reference's stat rounded to fp32, (B, C, 2)."""
    ref = reference_forward(c, inp)[0]
    return torch.stack([ref["mean"], ref["rstd"]], dim=-1).float()


def reference_forward(c, inp):
    a, u = inp["a"].double(), inp["u"].double()
    L = c.L
    fast = 4.0 if c.dtype == "bf16" else 0.0
    mu = u.mean(dim=1)
    var = ((u - mu[:, None]) ** 2).mean(dim=1)
    rstd = 1.0 / torch.sqrt(var + EPS)
    n = (u - mu[:, None]) * rstd[:, None]
    ge = n * _Phi(n)
    var_b = torch.zeros_like(var)
    for s in range(c.S):
        lo, hi = slice_bounds(L, c.S, s)
        if hi > lo:
            var_b += (hi - lo) * (u[:, lo:hi].mean(dim=1) - mu) ** 2 / L
    dmu = u.abs().mean(dim=1)
    dvar = 3 * var + 2 * torch.sqrt(var_b) * dmu
    rel = dvar / (2 * (var + EPS))
    dn = rstd[:, None] * (u.abs() + dmu[:, None]) + n.abs() * rel[:, None] + n.abs()
    zero = torch.zeros_like
    ref = {"y": a + ge, "mean": mu, "rstd": rstd}
    cond = {"y": (zero(a), a.abs() + ge.abs() + (_Phi(n) + n * _phi(n)).abs() * dn + (1 + fast) * n.abs()),
            "mean": (zero(mu), dmu), "rstd": (zero(mu), rstd * rel + 2 * rstd)}
    return ref, cond


def reference_backward(c, inp, stat):
    gy, u = inp["gy"].double(), inp["u"].double()
    fast = 4.0 if c.dtype == "bf16" else 0.0
    mean, rstd = stat[..., 0].double()[:, None], stat[..., 1].double()[:, None]
    n = (u - mean) * rstd
    gp = _Phi(n) + n * _phi(n)
    gn = gy * gp
    m1, m2 = gn.mean(dim=1, keepdim=True), (gn * n).mean(dim=1, keepdim=True)
    du = rstd * (gn - m1 - n * m2)
    dnb = 2 * n.abs()
    dgn = gy.abs() * ((_phi(n) * (2 - n * n)).abs() * dnb + 4 * gp.abs() + 1 + fast * (1 + n.abs()))
    dm1 = (dgn + gn.abs()).mean(dim=1, keepdim=True)
    dm2 = (dgn * n.abs() + gn.abs() * dnb + (gn * n).abs()).mean(dim=1, keepdim=True)
    bnd = rstd * (dgn + dm1 + n.abs() * dm2 + m2.abs() * dnb + 2 * gn.abs() + 2 * m1.abs() + 3 * (n * m2).abs())
    return du, (torch.zeros_like(du), bnd)


def reference(c, inp, got=None):
    """got: the outputs under test; a chained case takes its backward operand (mean, rstd) from there."""
    ref, cond = reference_forward(c, inp)
    if c.chained:
        assert got is not None
        stat = torch.stack([got["mean"], got["rstd"]], dim=-1).float()
    else:
        stat = stat_fed(c, inp)
    ref["du"], cond["du"] = reference_backward(c, inp, stat)
    return ref, cond


# ----------------------------------------------------------------------------------------------------------------- model
def _seq_sum(rows, nthr):
    """fp32 sum over dim 1 of (B, n, C) with the device's DEPTH in another order: thread t of nthr adds its rows t, t + nthr, .. last
    to first, then the partial sums meet in a tree of ADJACENT pairs (the device pairs t with t + stride)."""
    B, n, C = rows.shape
    steps = -(-n // nthr) if n else 0
    pad = torch.zeros(B, steps * nthr - n, C, dtype=torch.float32)
    grid = torch.cat([rows, pad], dim=1).view(B, steps, nthr, C) if steps else torch.zeros(B, 0, nthr, C)
    acc = torch.zeros(B, nthr, C, dtype=torch.float32)
    for i in range(steps - 1, -1, -1):
        acc = acc + grid[:, i]
    while acc.shape[1] > 1:
        acc = acc[:, 0::2] + acc[:, 1::2]
    return acc[:, 0]


def _erf_fast(v):
    x = v.abs() * 0.70710678118654752440
    t = 1.0 / (1.0 + 0.3275911 * x)
    e = torch.exp(-0.5 * v * v)
    poly = t * (0.254829592 + t * (-0.284496736 + t * (1.421413741 + t * (-1.453152027 + t * 1.061405429))))
    cdf = 0.5 + torch.where(v < 0, -0.5, 0.5) * (1.0 - poly * e)
    return cdf, e


def _gelu_parts(c, v, variant):
    """fp32 (Phi, exp(-v^2 / 2)) as gelu_t / gelu_grad_t evaluate them."""
    if c.dtype == "bf16" and variant != "exact_erf":
        return _erf_fast(v)
    return 0.5 * (1.0 + torch.erf(v * 0.70710678118654752440)), torch.exp(-0.5 * v * v)


def model(c, inp, defect=None, stat=None):
    assert defect is None or defect in DEFECTS + VARIANTS
    dt = torch_dtype(c)
    a, u, gy = inp["a"].float(), inp["u"].float(), inp["gy"].float()
    B, L, C, S = c.B, c.L, c.C, c.S
    per = (L + S - 1) // S
    nthr = launch(c).rows
    means, m2s, nbs = [], [], []
    for s in range(S):
        lo, hi = slice_bounds(L, S, s)
        rows = u[:, lo:hi]
        cnt = max(hi - lo, 0)
        if cnt > 0:
            mean = _seq_sum(rows, nthr) / float(cnt)
            if defect == "one_pass":
                m2 = _seq_sum(rows * rows, nthr) - float(cnt) * mean * mean
            else:
                d = rows - mean[:, None]
                m2 = _seq_sum(d * d, nthr)
        else:
            mean, m2 = torch.zeros(B, C), torch.zeros(B, C)
        means.append(mean)
        m2s.append(m2)
        nbs.append(float(per if defect == "empty_as_per" else cnt))
    if defect == "merge_unweighted":
        nbs = [float(L) / S] * S
    acc = torch.zeros(B, C)
    for s in range(S - 1, -1, -1):
        acc = acc + nbs[s] * means[s]
    mean = acc / float(L)
    acc = torch.zeros(B, C)
    for s in range(S - 1, -1, -1):
        d = means[s] - mean
        acc = acc + (m2s[s] + nbs[s] * d * d)
    rstd = torch.rsqrt(acc / float(L) + torch.tensor(EPS, dtype=torch.float32))
    n = (u - mean[:, None]) * rstd[:, None]
    cdf, _ = _gelu_parts(c, n, defect)
    y = (a + n * cdf).to(dt)
    out = {"y": y, "mean": mean, "rstd": rstd}
    # backward on the fed stat
    st = stat if stat is not None else (torch.stack([mean, rstd], dim=-1) if c.chained else stat_fed(c, inp))
    bm, br = st[..., 0][:, None], st[..., 1][:, None]
    n = (u - bm) * br
    cdf, e = _gelu_parts(c, n, defect)
    gn = gy * (cdf + n * 0.39894228040143267794 * e)
    s1, s2 = torch.zeros(B, C), torch.zeros(B, C)
    for s in range(S - 1, -1, -1):
        lo, hi = slice_bounds(L, S, s)
        if hi > lo:
            s1 = s1 + _seq_sum(gn[:, lo:hi], nthr)
            s2 = s2 + _seq_sum((gn * n)[:, lo:hi], nthr)
    inv = torch.tensor(1.0, dtype=torch.float32) / float(L)
    m1, m2 = s1 * inv, (s2 if defect == "m2_no_div" else s2 * inv)
    out["du"] = (br * (gn - m1[:, None] - n * m2[:, None])).to(dt)
    return out


# ------------------------------------------------------------------------------------------------------------ constants
def key_of(c, name):
    return (OPERATION[name], name, c.dtype)


AXES = {"y": ("image", "position", "channel"), "du": ("image", "position", "channel"), "mean": ("image", "channel"), "rstd": ("image", "channel")}


def check(c, got, inp, what=None):
    """Every element of every output of the case against its bound; -> {output: worst ratio}."""
    ref, cond = reference(c, inp, got)
    assert set(got) == set(ref), (sorted(got), sorted(ref))
    return {name: assert_elementwise(got[name], ref[name], cond[name], C[key_of(c, name)], AXES[name], u=out_unit(c, name),
                                     what="%s %s" % (what or c.text, name)) for name in sorted(ref)}


def measure_c(case_list=None):
    worst = {}
    for c in (cases() if case_list is None else case_list):
        inp = inputs(c)
        got = model(c, inp)
        ref, cond = reference(c, inp, got)
        for name in ref:
            r = ratio(got[name], ref[name], cond[name], out_unit(c, name))
            worst[key_of(c, name)] = max(worst.get(key_of(c, name), 0.0), float(r.max()))
    return worst


def format_table(worst):
    lines = ["    operation   output   type   model max   C", "    ---------   ------   ----   ---------   ----"]
    for (op, out, dt), v in sorted(worst.items()):
        lines.append("    %-9s   %-6s   %-4s   %9.3f   %4.1f" % (op, out, dt, v, c_of(v)))
    return "\n".join(lines)


MEASURED = {
    ("inorm_bwd", "du", "bf16"): 1.989,
    ("inorm_bwd", "du", "f32"): 0.385,
    ("inorm_fwd", "mean", "bf16"): 0.740,
    ("inorm_fwd", "mean", "f32"): 2.744,
    ("inorm_fwd", "rstd", "bf16"): 1.126,
    ("inorm_fwd", "rstd", "f32"): 0.813,
    ("inorm_fwd", "y", "bf16"): 1.991,
    ("inorm_fwd", "y", "f32"): 2.541,
}
C = {k: c_of(v) for k, v in MEASURED.items()}
__doc__ = __doc__.replace("@TABLE@", format_table(MEASURED))
