"""fp64 reference, error bounds and fp32 model of the set criterion's four entry points (csrc/setloss.hip: gwd_set_losses_forward /
_backward and the _focal_ pair; CPU only, plain module; the instrument is tests/attn_ref.py's).

The assignment ``qot`` is GIVEN: the test constructs it, it does not come from the LSAP, so surplus, negative and padded columns stand
where the case wants them.  A case is (L = 2, B, Q, cap, K, D, gamma - None is the cross entropy -, logit kind, table kind, num_items,
world, with g_ce, with g_l1, a nonzero dlines on entry, a zero class weight, an equal coordinate).  ``inputs(c)`` draws, seeded from
the case text, logits (L, B, Q, K), lines (L, B, Q, D), targets (cap, D), int64 labels, bidx, valid, qot (L, cap), positive class
weights, the per-layer upstream gradients (all distinct) and the entry value c0 of dlines.

Table kinds.  ``full``: every column valid and matched (needs cap <= B Q).  ``kinds``: the columns of every image cycle through a
matched column (four in seven), ``valid = 1, qot = Q`` (a surplus target), ``valid = 0, qot = Q`` (padding), ``valid = 0, qot < Q``
(a free query: neither guard of the kernel's ``if`` may let it through alone) and ``valid = 1, qot = -1``; matched columns beyond an
image's Q queries become surplus ones.  ``ordered``: as ``kinds``, but the matched columns of an image take its queries 0, 1, 2 ...
in turn, so that with the hard logits below the target class of a known row is known.  Labels of matched columns run through
0 .. K - 1 (other valid columns carry t mod K); out-of-range labels (-1, K, -5, K + 7) stand ONLY in columns with ``valid = 0`` and must not reach target_class.
Logit kinds: ``rand`` (2 randn); ``hard2`` (K = 2: the rows cycle through matchcost_ref.HARD_ROWS - [30, -30], [-60, 60],
[100, -100], [1.5, 1.5] - and a random one); ``hard8`` (K = 8: every other row has one class at +50 and the rest at -50).

``reference(c, inp)`` -> (ref, cond): the formulas of the kernel file's header in fp64 from the operands as stored, n =
max(num_items / world, 1), p = softmax, c = target_class, nll = -log p_c, u = sum_{k != c} p_k, w = class_weight[c]:

  target_class  K - 1, or the label of the valid column matched to the query        equality
  wsum[l]       sum_i w_i, the fp64 sum rounded to fp32                              equality
  ce[l]         cross entropy: sum_i w nll / sum_i w;  focal: sum_i w nll u^gamma / (B Q)
                cond = the same sum (every term is positive)
  l1[l]         sum over matched columns of sum_d |line - tgt| / n,  cond = the same sum
  dlogits       f (p_k - [k = c]),  cross entropy: f = g_ce w / wsum;  focal: f = g_ce w / (B Q) m,
                m = u^gamma + gamma u^(gamma - 1) p_c nll  (the second summand absent for gamma = 0 and, as its limit, 0 at u = 0)
                cond = |f| (p_k + [k = c]), both summands of m counted in |f| (they are positive: |f| is f's magnitude)
  dlines        c0 + g_l1 sign(line - tgt) / n on matched rows, c0 elsewhere;  cond = |g_l1 sign / n| + |c0|
      |got - ref| <= C u_f32 (|ref| + cond)

An unmatched row of dlines has cond = 0 and ref = c0: it must be bit-identical to c0 (exactly 0 in production), and so must every row when g_l1 is
absent: ``check`` compares the bits, because around a nonzero c0 the bound would leave C u |c0|.  At K = 1 every term of
ce and dlogits is exactly 0, and so must the results be.  tests/attn_ref.FLOOR applies where the reference is below fp32's
subnormals: at gamma = 0.5 the row [100, -100] with target class 0 has u = e^-200 in fp64 (m about 1e-43) and u = 0, m = 0 in fp32.

The negative log likelihood.  Up to this work the focal kernels formed nll = -((lg_c - mx) - log s), s = sum_k exp(lg_k - mx).  With
c the largest class that is log(1 + so), and the rounding of s = 1 + so is an ABSOLUTE error u_f32 of nll: at u = 1e-3 a relative error
6e-5 of nll, carried into the second summand of m and so into every element of the row's gradient (the defect ``nll_from_lse`` below
keeps that formulation: its ratios are in the hundreds).  The kernels now use nll = -log1p(-u) where u < 1/2 - u is a sum of positive
terms, accurate to a few ulp - and the old expression elsewhere, where its two terms mx - lg_c and log s are both positive.  The cross
entropy pair keeps the old expression: there nll only enters sums in which its absolute error does not show.

``model(c, inp, defect=None)``: the kernels' arithmetic in fp32 (the maximum, exp(lg - mx) and their sum in ascending k, u = so / s,
focal_pow's special cases gamma = 0 and 2, (nll w) u^gamma, ((gamma u^(gamma-1)) p_c) nll, ((g_ce w) / BQ) m), the per-query products
and the per-column L1 sums added in fp64 as on the device.  ``model`` also returns how many rows took either side of the backward
kernel's guard ``gamma != 0 && (u > 0 || gamma >= 1)``.  Defects: ``cap_tail_skipped`` / ``bq_tail_skipped`` (the second trip of the
256-thread loop over the columns / the queries not made), ``valid_ignored``, ``surplus_labelled`` (qot = Q not excluded: the label
lands on the next image's first query), ``clamp_dropped`` (n = num_items / world), ``one_minus_pt`` (u = 1 - p_c), ``guard_removed``
(inf * 0 = NaN at u = 0), ``focal_over_wsum`` (the focal ce divided by wsum), ``weight_last_class`` (matched queries weighted as "no
object"), ``sign0_is_1`` (an equal coordinate gets +1), ``nll_from_lse`` (above).

The constants.  ``measure_c()``: largest |model - ref| / bound over the case list per (operation, output); C twice that, one decimal
up (the factor 2 covers the device's exp / log / pow and a contracted multiply-add).  CPU, 2026-10:

@TABLE@

A kernel that needs more than its C has a defect or the bound lacks a term: neither is repaired by raising C.
"""
import types
import zlib

import numpy as np
import torch

from tests.attn_ref import FLOOR, U_F32, assert_elementwise, ratio        # noqa: F401  (the instrument)
from tests.conv_ref import c_of
from tests.matchcost_ref import HARD_ROWS

DEFECTS = ("cap_tail_skipped", "bq_tail_skipped", "valid_ignored", "surplus_labelled", "clamp_dropped", "one_minus_pt", "guard_removed",
           "focal_over_wsum", "weight_last_class", "sign0_is_1", "nll_from_lse")
KMAX, DMAX, THREADS, LAYERS = 8, 8, 256, 2                      # csrc/setloss.hip
GAMMAS = (None, 0.0, 0.5, 1.0, 2.0, 2.5)
TC_SENTINEL = -77
OOB = lambda K: [-1, K, -5, K + 7]                              # noqa: E731
OUTPUTS = ("ce", "l1", "dlogits", "dlines")
AXES = {"ce": ("layer",), "l1": ("layer",), "dlogits": ("layer", "image", "query", "class"), "dlines": ("layer", "image", "query", "coordinate")}


def launch(c):
    bq = c.B * c.Q
    return types.SimpleNamespace(BQ=bq, bq_trips=(bq + THREADS - 1) // THREADS, cap_trips=(c.cap + THREADS - 1) // THREADS,
                                 idle=THREADS - min(bq, THREADS), blocks=LAYERS, focal=c.gamma is not None)


def _case(B, Q, cap, K=2, D=6, gamma=None, logits="rand", table="kinds", ni=(37, 1), gce=True, gl1=True, c0=False, zero_w=False, eq=False):
    c = types.SimpleNamespace(L=LAYERS, B=B, Q=Q, cap=cap, K=K, D=D, gamma=gamma, logits=logits, table=table, num_items=float(ni[0]),
                              world=float(ni[1]), gce=gce, gl1=gl1, c0=c0, zero_w=zero_w, eq=eq)
    c.text = "set_losses B=%d Q=%d cap=%d K=%d D=%d gamma=%s logits=%s table=%s n=%g:%g gce=%d gl1=%d c0=%d zero_w=%d eq=%d" % (
        B, Q, cap, K, D, "ce" if gamma is None else "%g" % gamma, logits, table, ni[0], ni[1], gce, gl1, c0, zero_w, eq)
    c.id = c.text.replace(" ", "-")
    return c


def cases():
    out = [_case(1, 1, 1, gamma=g, table="full") for g in (None, 2.0)]
    out += [_case(B, Q, 21, gamma=g) for B, Q in ((1, 7), (3, 85), (2, 128), (1, 257), (3, 171)) for g in (None, 2.0)]     # B Q = 7 ... 513
    out += [_case(3, 110, cap, gamma=g, table=t) for cap, t in ((64, "kinds"), (256, "full"), (256, "kinds"), (257, "full"), (257, "kinds"),
                                                               (300, "full"), (300, "kinds")) for g in (None, 2.5)]
    out += [_case(2, 9, 28, K=K, D=D, gamma=g) for K in (1, 2, 3, 8) for D in (1, 6, 8) for g in (None, 1.0)]
    out += [_case(2, 9, 14, ni=ni, gamma=g) for ni in ((0, 1), (3, 2), (4, 8), (37, 1)) for g in (None, 0.5)]
    out += [_case(2, 10, 12, gamma=g, logits="hard2", table="ordered") for g in GAMMAS]
    out += [_case(2, 9, 28, K=8, gamma=g, logits="hard8") for g in (None, 0.5, 2.5)]
    out += [_case(2, 9, 14, K=3, gamma=g) for g in GAMMAS[1:]]
    out += [_case(2, 9, 14, gamma=g, gce=False) for g in (None, 0.5)] + [_case(2, 9, 14, gl1=False), _case(2, 9, 14, gamma=2.0, gl1=False, c0=True)]
    out += [_case(2, 9, 14, c0=True, eq=True), _case(2, 9, 14, gamma=0.5, c0=True), _case(2, 9, 14, eq=True), _case(3, 110, 300, gamma=1.0, eq=True)]
    out += [_case(2, 9, 14, K=3, gamma=g, zero_w=True) for g in (None, 2.0)]
    seen = set()
    return [c for c in out if not (c.text in seen or seen.add(c.text))]              # (two of the sweeps meet in one case)


def rejected():
    """(name, (L, B, Q, cap, K, D), gamma, return code)."""
    return [("K=9", (1, 2, 3, 4, 9, 6), None, -4), ("D=9", (1, 2, 3, 4, 2, 9), None, -4), ("cap=0", (1, 2, 3, 0, 2, 6), None, -1),
            ("K=9_focal", (1, 2, 3, 4, 9, 6), 2.0, -4), ("gamma=-1", (1, 2, 3, 4, 2, 6), -1.0, -1), ("gamma=nan", (1, 2, 3, 4, 2, 6), float("nan"), -1)]


# ---------------------------------------------------------------------------------------------------------------- inputs
CYCLE = ("m", "m", "surplus", "m", "pad", "free", "m", "neg")            # the column kinds of a ``kinds`` table, in turn


def inputs(c):
    g = torch.Generator()
    g.manual_seed(zlib.crc32(c.text.encode()))
    rng = np.random.default_rng(zlib.crc32(c.text.encode()))
    L, B, Q, K, D, cap = c.L, c.B, c.Q, c.K, c.D, c.cap
    logits = (2.0 * torch.randn((L, B, Q, K), generator=g, dtype=torch.float64)).float()
    flat = logits.view(-1, K)
    if c.logits == "hard2":
        assert K == 2 and Q % 5 == 0
        for r in range(flat.shape[0]):
            if r % 5 < 4:
                flat[r] = torch.tensor(HARD_ROWS[r % 5])
    if c.logits == "hard8":
        assert K == 8
        for r in range(0, flat.shape[0], 2):
            flat[r] = -50.0
            flat[r, (r // 2) % K] = 50.0
    lines = torch.rand((L, B, Q, D), generator=g, dtype=torch.float64).float()
    tgt = torch.rand((cap, D), generator=g, dtype=torch.float64).float()
    bidx = (np.arange(cap) * B // cap).astype(np.int32)                                   # sorted by image, even shares
    kind = ["m"] * cap if c.table == "full" else [CYCLE[t % len(CYCLE)] for t in range(cap)]
    valid = np.ones(cap, np.int32)
    qot = np.full((L, cap), Q, np.int32)
    for l in range(L):
        for b in range(B):
            cols = np.nonzero(bidx == b)[0]
            order = np.arange(Q) if c.table == "ordered" else rng.permutation(Q)
            used = 0
            for t in cols:
                if kind[t] in ("m", "free") and used < Q:
                    qot[l, t] = order[used]
                    used += 1
                elif kind[t] == "m":
                    assert c.table != "full"
                    if l == L - 1:
                        kind[t] = "surplus"
                elif kind[t] == "neg":
                    qot[l, t] = -1
    for t in range(cap):
        if kind[t] in ("pad", "free"):
            valid[t] = 0
    labels = np.zeros(cap, np.int64)
    nm = 0
    for t in range(cap):
        if kind[t] == "m":                                                              # the matched columns run through every class
            labels[t] = nm % K
            nm += 1
        else:
            labels[t] = t % K if valid[t] else OOB(K)[t % 4]
    cls_w = (0.1 + torch.rand(K, generator=g, dtype=torch.float64)).float()
    if c.zero_w:
        assert K >= 2
        cls_w[0] = 0.0
    if c.eq:                                                                            # one coordinate of a matched pair bit-equal
        l, t = 0, next(t for t in range(cap) if valid[t] and 0 <= qot[0, t] < Q)
        tgt[t, D - 1] = lines[l, int(bidx[t]), int(qot[l, t]), D - 1]
    return {"logits": logits, "lines": lines, "tgt": tgt, "labels": torch.from_numpy(labels), "bidx": torch.from_numpy(bidx),
            "valid": torch.from_numpy(valid), "qot": torch.from_numpy(qot), "cls_w": cls_w,
            "num_items": torch.tensor([c.num_items], dtype=torch.float32),
            "g_ce": torch.tensor([0.7 + 0.45 * l for l in range(L)], dtype=torch.float32) if c.gce else None,
            "g_l1": torch.tensor([-1.3 + 2.9 * l for l in range(L)], dtype=torch.float32) if c.gl1 else None,
            "c0": (torch.randn((L, B, Q, D), generator=g, dtype=torch.float64).float() if c.c0 else torch.zeros(L, B, Q, D)),
            "kinds": kind}


def matched(c, inp, defect=None):
    """[(layer, column, flat query row)] of the columns that carry a label and an L1 term."""
    out = []
    for l in range(c.L):
        for t in range(c.cap):
            if defect == "cap_tail_skipped" and t >= THREADS:
                continue
            q, b = int(inp["qot"][l, t]), int(inp["bidx"][t])
            ok_q = 0 <= q < c.Q or (defect == "surplus_labelled" and q == c.Q and b * c.Q + q < c.B * c.Q)
            if ok_q and (int(inp["valid"][t]) or defect == "valid_ignored"):
                out.append((l, t, b * c.Q + q))
    return out


def _target_class(c, inp, pairs):
    tc = torch.full((c.L, c.B * c.Q), c.K - 1, dtype=torch.int32)
    for l, t, row in pairs:
        tc[l, row] = int(inp["labels"][t])
    return tc.view(c.L, c.B, c.Q)


def _n64(c):
    return max(c.num_items / c.world, 1.0)


# ------------------------------------------------------------------------------------------------------------- reference
def reference(c, inp):
    L, B, Q, K, D = c.L, c.B, c.Q, c.K, c.D
    BQ = B * Q
    pairs = matched(c, inp)
    tc = _target_class(c, inp, pairs)
    assert int(tc.min()) >= 0 and int(tc.max()) <= K - 1                                 # no out-of-range label is live
    lg = inp["logits"].double().view(L, BQ, K)
    logp = torch.log_softmax(lg, -1)
    p = logp.exp()
    cidx = tc.view(L, BQ, 1).long()
    hit = torch.zeros(L, BQ, K, dtype=torch.bool).scatter_(-1, cidx, True)
    u = p.masked_fill(hit, 0.0).sum(-1)
    nll = -logp.gather(-1, cidx)[..., 0]
    nll = torch.where(u < 0.5, -torch.log1p(-u), nll)                                    # (fp64's log-sum-exp loses a u below 1e-16, too)
    pc = p.gather(-1, cidx)[..., 0]
    w = inp["cls_w"].double()[cidx[..., 0]]
    ref, cond = {"target_class": tc}, {}
    wsum = w.sum(1)
    ref["wsum"] = wsum.float()
    if c.gamma is None:
        ce = (w * nll).sum(1) / wsum
        m = torch.ones_like(u)
        denom = wsum[:, None]
    else:
        ce = (w * nll * u ** c.gamma).sum(1) / BQ
        m = u ** c.gamma
        if c.gamma != 0.0:
            m = m + torch.where(u > 0, c.gamma * u.clamp_min(1e-300) ** (c.gamma - 1.0) * pc * nll, torch.zeros_like(u))
        denom = torch.full((L, 1), float(BQ), dtype=torch.float64)
    ref["ce"], cond["ce"] = ce, ce.abs()
    n = _n64(c)
    l1 = torch.zeros(L, dtype=torch.float64)
    dlines = inp["c0"].double().clone().view(L, BQ, D)
    cl = inp["c0"].double().abs().clone().view(L, BQ, D)
    ln, tg = inp["lines"].double().view(L, BQ, D), inp["tgt"].double()
    gl1 = inp["g_l1"].double() if inp["g_l1"] is not None else torch.zeros(L, dtype=torch.float64)
    for l, t, row in pairs:
        df = ln[l, row] - tg[t]
        l1[l] += df.abs().sum() / n
        step = gl1[l] * torch.sign(df) / n
        dlines[l, row] += step
        cl[l, row] += step.abs()
    touched = torch.zeros(L, BQ, dtype=torch.bool)
    for l, t, row in pairs:
        touched[l, row] = True
    cl = torch.where(touched[..., None], cl, torch.zeros_like(cl))                        # an unmatched row: bit-identical to c0
    ref["l1"], cond["l1"] = l1, l1.abs()
    ref["dlines"], cond["dlines"] = dlines.view(L, B, Q, D), cl.view(L, B, Q, D)
    gce = inp["g_ce"].double() if inp["g_ce"] is not None else torch.zeros(L, dtype=torch.float64)
    f = gce[:, None] * w / denom * m                                                      # (L, BQ)
    ref["dlogits"] = (f[..., None] * (p - hit.double())).view(L, B, Q, K)
    cond["dlogits"] = (f.abs()[..., None] * (p + hit.double())).view(L, B, Q, K)
    if K == 1:
        assert not bool(ref["ce"].any()) and not bool(ref["dlogits"].any())                # every term is exactly 0
    return ref, cond


# ----------------------------------------------------------------------------------------------------------------- model
def _pow(u, g):
    """focal_pow: u^0 = 1 also at u = 0, u^2 = u u, powf otherwise."""
    if g == 0.0:
        return torch.ones_like(u)
    if g == 2.0:
        return u * u
    return torch.pow(u, torch.tensor(g, dtype=torch.float32))


def model(c, inp, defect=None):
    """-> {target_class, ce, l1, wsum, dlogits, dlines, guard: (rows that took the second summand, rows the guard kept from it)}."""
    assert defect is None or defect in DEFECTS
    L, B, Q, K, D = c.L, c.B, c.Q, c.K, c.D
    BQ = B * Q
    f32 = lambda x: torch.tensor(x, dtype=torch.float32)                                 # noqa: E731
    pairs = matched(c, inp, defect)
    tc_raw = _target_class(c, inp, pairs)
    tc = tc_raw.clamp(0, K - 1).view(L, BQ, 1).long()                                    # (a defect's out-of-range label: kept readable)
    lg = inp["logits"].view(L, BQ, K)
    mx = lg[..., 0]
    for k in range(1, K):
        mx = torch.maximum(mx, lg[..., k])
    e = torch.exp(lg - mx[..., None])
    s = torch.zeros_like(mx)
    for k in range(K):
        s = s + e[..., k]
    p = e / s[..., None]
    hit = torch.zeros(L, BQ, K, dtype=torch.bool).scatter_(-1, tc, True)
    lgc, pc = lg.gather(-1, tc)[..., 0], p.gather(-1, tc)[..., 0]
    w = inp["cls_w"][(torch.full_like(tc, K - 1) if defect == "weight_last_class" else tc)[..., 0]]
    nll = -((lgc - mx) - torch.log(s))
    live = torch.ones(L, BQ, dtype=torch.bool)
    if defect == "bq_tail_skipped":
        live[:, THREADS:] = False
    taken = kept = 0
    if c.gamma is None:
        term, m = nll * w, None
    else:
        so = torch.zeros_like(mx)
        for k in range(K):
            so = so + torch.where(hit[..., k], torch.zeros_like(mx), e[..., k])
        u = (1.0 - pc) if defect == "one_minus_pt" else so / s
        if defect != "nll_from_lse":
            nll = torch.where(u < 0.5, -torch.log1p(-u), nll)
        gm = f32(c.gamma)
        term = nll * w * _pow(u, c.gamma)
        m = _pow(u, c.gamma)
        if c.gamma != 0.0:
            guard = (u > 0) | torch.tensor(c.gamma >= 1.0)
            if defect == "guard_removed":
                guard = torch.ones_like(guard)
            second = gm * _pow(u, c.gamma - 1.0) * pc * nll
            m = torch.where(guard, m + second, m)
            taken, kept = int(guard.sum()), int((~guard).sum())
    s_n = torch.where(live, term, torch.zeros_like(term)).double().sum(1)
    s_w = torch.where(live, w, torch.zeros_like(w)).double().sum(1)
    got = {"target_class": tc_raw, "wsum": s_w.float(), "guard": (taken, kept)}
    if defect == "bq_tail_skipped" and BQ > THREADS:
        got["target_class"] = tc_raw.clone()
        got["target_class"].view(L, BQ)[:, THREADS:] = TC_SENTINEL
    focal_denom = s_w if defect == "focal_over_wsum" else torch.full((L,), float(BQ), dtype=torch.float64)
    got["ce"] = (s_n / (s_w if c.gamma is None else focal_denom)).float()
    # ---- the L1 term and its gradient
    n = inp["num_items"][0] / f32(c.world)
    if defect != "clamp_dropped":
        n = torch.maximum(n, f32(1.0))
    ln, tg = inp["lines"].view(L, BQ, D), inp["tgt"]
    s_l1 = torch.zeros(L, dtype=torch.float64)
    dlines = inp["c0"].clone().view(L, BQ, D)
    for l, t, row in pairs:
        a = f32(0.0)
        for d in range(D):
            a = a + (ln[l, row, d] - tg[t, d]).abs()
        s_l1[l] += a.double()
        if inp["g_l1"] is not None:
            df = ln[l, row] - tg[t]
            sg = torch.where(df >= 0, 1.0, -1.0) if defect == "sign0_is_1" else torch.sign(df)
            dlines[l, row] = dlines[l, row] + inp["g_l1"][l] * sg / n
        else:
            dlines[l, row] = dlines[l, row] + f32(0.0) * torch.sign(ln[l, row] - tg[t]) / n
    got["l1"] = (s_l1 / n.double()).float()
    got["dlines"] = dlines.view(L, B, Q, D)
    # ---- the label gradient
    gce = inp["g_ce"] if inp["g_ce"] is not None else torch.zeros(L)
    if c.gamma is None:
        f = gce[:, None] * w / got["wsum"][:, None]
    else:
        f = gce[:, None] * w / f32(float(BQ)) * m
    dlogits = f[..., None] * (p - hit.float())
    if defect == "bq_tail_skipped":
        dlogits[:, THREADS:] = float("nan")
    got["dlogits"] = dlogits.view(L, B, Q, K)
    return got


# ------------------------------------------------------------------------------------------------------------ constants
def key_of(c, name):
    return ("set_losses" if c.gamma is None else "set_focal", name, "f32")


def check(c, got, inp, ref=None, cond=None, what=None):
    """Equality of target_class and wsum, bit equality of the untouched rows of dlines, the bounds for the rest -> {output: worst ratio}."""
    if ref is None:
        ref, cond = reference(c, inp)
    what = what or c.text
    bad = int((got["target_class"] != ref["target_class"]).sum())
    assert bad == 0, "%s: %d target classes differ" % (what, bad)
    assert torch.equal(got["wsum"], ref["wsum"]), "%s: wsum %r, fp64 sum %r" % (what, got["wsum"].tolist(), ref["wsum"].tolist())
    # rows of dlines that no matched column touches - all rows without g_l1 - keep the BITS of their entry value (the bound below would
    # allow C u |c0| around a nonzero c0)
    keep = torch.ones(c.L, c.B * c.Q, dtype=torch.bool)
    if inp["g_l1"] is not None:
        for l, t, row in matched(c, inp):
            keep[l, row] = False
    same = got["dlines"].contiguous().view(torch.int32) == inp["c0"].contiguous().view(torch.int32)
    bad = int((~same.view(c.L, c.B * c.Q, c.D) & keep[..., None]).sum())
    assert bad == 0, "%s: %d elements of dlines outside the matched rows differ from their entry value" % (what, bad)
    return {name: assert_elementwise(got[name], ref[name], (cond[name], None), C[key_of(c, name)], AXES[name], u=U_F32,
                                     what="%s %s" % (what, name)) for name in OUTPUTS}


def measure_c(case_list=None):
    worst = {}
    for c in (cases() if case_list is None else case_list):
        inp = inputs(c)
        ref, cond = reference(c, inp)
        got = model(c, inp)
        for name in OUTPUTS:
            k = key_of(c, name)
            worst[k] = max(worst.get(k, 0.0), float(ratio(got[name], ref[name], (cond[name], None), U_F32).max()))
    return worst


def format_table(worst):
    lines = ["    operation    output    type   model max   C", "    ----------   -------   ----   ---------   ----"]
    for (op, out, dt), v in sorted(worst.items()):
        lines.append("    %-10s   %-7s   %-4s   %9.3f   %4.1f" % (op, out, dt, v, c_of(v)))
    return "\n".join(lines)


MEASURED = {
    ("set_losses", "ce", "f32"): 1.126,
    ("set_losses", "l1", "f32"): 0.572,
    ("set_losses", "dlogits", "f32"): 4.736,
    ("set_losses", "dlines", "f32"): 0.554,
    ("set_focal", "ce", "f32"): 6.517,
    ("set_focal", "l1", "f32"): 0.608,
    ("set_focal", "dlogits", "f32"): 14.508,
    ("set_focal", "dlines", "f32"): 0.398,
}
C = {k: c_of(v) for k, v in MEASURED.items()}
__doc__ = __doc__.replace("@TABLE@", format_table(MEASURED))
