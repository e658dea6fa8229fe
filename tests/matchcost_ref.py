"""fp64 reference, error bound and fp32 model of the matcher's cost block (csrc/setloss.hip, gwd_match_cost:
cost[l][b][q][t] = w_line sum_d |lines[l][b][q][d] - tgt[t][d]| - w_class softmax(logits[l][b][q])[clamp(label[t], 0, K - 1)], fp32;
CPU only, plain module; the instrument is tests/attn_ref.py's).

A case is (L, B, Q, cap, K, D, w_line, w_class, logit kind, label kind).  ``inputs(c)`` draws, seeded from the case text, logits
(L, B, Q, K), lines (L, B, Q, D), targets (cap, D) and int64 labels (cap,).  Logit kinds: ``rand``; ``hard``: the rows cycle through
[30, -30], [-60, 60], [100, -100] (the probability of the smaller class underflows fp32), an equal row and a random one (K = 2).  Label
kinds: ``range`` (t mod K: every class, K - 1 included), ``oob`` (the last columns - padding - carry -1, K, -5 and K + 7: the clamp
keeps the read inside p[0 .. K - 1]).

* ``launch(c)``: total = L B Q cap, blocks = min(2048, ceil(total / 256)), trips of the grid-stride loop.
* ``reference(c, inp)`` -> (ref, cond), fp64 from the stored fp32 operands:
      |got - ref| <= C u_f32 (|ref| + cond),   cond = |w_line| sum_d |line - tgt| + |w_class| p
* ``model(c, inp, defect=None)``: the kernel's arithmetic in fp32: the maximum, exp(lg - mx), their sum and the quotient, the L1 sum
  in ascending d, the two products and their sum.  Defects: ``label_unclamped_wraps`` (an out-of-range label is taken modulo K),
  ``stride_tail_skipped`` (the elements beyond the first grid-stride trip are not written), ``softmax_no_max`` (exp of the raw
  logits: overflow on the saturated rows), ``d_last_dropped`` (the L1 sum stops one coordinate early).

The constant.  ``measure_c()``: largest |model - ref| / bound over the case list; C twice that, one decimal up (the factor 2 covers the
device's exp and a contracted multiply-add).  CPU, 2026-10:

@TABLE@

A kernel that needs more than its C has a defect or the bound lacks a term: neither is repaired by raising C.
"""
import types
import zlib

import torch

from tests.attn_ref import FLOOR, U_F32, assert_elementwise, ratio        # noqa: F401  (the instrument)
from tests.conv_ref import c_of

DEFECTS = ("label_unclamped_wraps", "stride_tail_skipped", "softmax_no_max", "d_last_dropped")
KMAX, DMAX, THREADS, MAX_BLOCKS = 8, 8, 256, 2048               # csrc/setloss.hip
AXES = ("layer", "image", "query", "target")
HARD_ROWS = ((30.0, -30.0), (-60.0, 60.0), (100.0, -100.0), (1.5, 1.5))


def oob_labels(K):
    """The labels of the last four (padding) columns of an ``oob`` case."""
    return [-1, K, -5, K + 7]


def launch(c):
    total = c.L * c.B * c.Q * c.cap
    blocks = min(MAX_BLOCKS, (total + THREADS - 1) // THREADS)
    return types.SimpleNamespace(total=total, blocks=blocks, trips=(total + blocks * THREADS - 1) // (blocks * THREADS),
                                 tail=total > MAX_BLOCKS * THREADS)


def _case(L, B, Q, cap, K, D, w_line=5.0, w_class=2.0, logits="rand", labels="range"):
    c = types.SimpleNamespace(L=L, B=B, Q=Q, cap=cap, K=K, D=D, w_line=w_line, w_class=w_class, logits=logits, labels=labels)
    c.text = "match_cost L=%d B=%d Q=%d cap=%d K=%d D=%d w_line=%g w_class=%g logits=%s labels=%s" % (L, B, Q, cap, K, D, w_line, w_class, logits, labels)
    c.id = c.text.replace(" ", "-")
    return c


def cases():
    out = [_case(2, 2, 5, 19, K, D) for K in (1, 2, 8) for D in (1, 6, 8)]
    out += [_case(2, 2, 5, 9, 2, 6, labels="oob"), _case(1, 2, 3, 13, 8, 6, labels="oob")]
    out += [_case(2, 2, 5, 7, 2, 6, logits="hard"), _case(2, 1, 5, 7, 2, 6, w_line=0.0, logits="hard")]
    out += [_case(2, 2, 5, 7, 2, 6, w_class=0.0), _case(2, 2, 5, 7, 2, 6, w_line=0.0)]
    out += [_case(1, 1, 1, 1, 2, 6), _case(1, 1, 5, 51, 2, 6), _case(1, 1, 1, 257, 2, 6)]
    out += [_case(1, 1, 3, 174763, 2, 6)]
    return out


def rejected():
    """(name, (L, B, Q, cap, K, D), return code)."""
    return [("K=9", (1, 2, 3, 4, 9, 6), -4), ("D=9", (1, 2, 3, 4, 2, 9), -4), ("cap=0", (1, 2, 3, 0, 2, 6), -1)]


# ---------------------------------------------------------------------------------------------------------------- inputs
def inputs(c):
    g = torch.Generator()
    g.manual_seed(zlib.crc32(c.text.encode()))
    logits = (2.0 * torch.randn((c.L, c.B, c.Q, c.K), generator=g, dtype=torch.float64)).float()
    if c.logits == "hard":
        assert c.K == 2
        flat = logits.view(-1, 2)
        for r in range(flat.shape[0]):
            if r % 5 < 4:
                flat[r] = torch.tensor(HARD_ROWS[r % 5])
    lines = torch.rand((c.L, c.B, c.Q, c.D), generator=g, dtype=torch.float64).float()
    tgt = torch.rand((c.cap, c.D), generator=g, dtype=torch.float64).float()
    labels = torch.arange(c.cap, dtype=torch.int64) % c.K
    if c.labels == "oob":
        labels[-4:] = torch.tensor(oob_labels(c.K))
    return {"logits": logits, "lines": lines, "tgt": tgt, "labels": labels}


# ------------------------------------------------------------------------------------------------------------- reference
def reference(c, inp):
    p = torch.softmax(inp["logits"].double(), dim=-1)                                        # (L, B, Q, K)
    lab = inp["labels"].clamp(0, c.K - 1)
    pt = p[..., lab]                                                                         # (L, B, Q, cap)
    l1 = (inp["lines"].double()[..., None, :] - inp["tgt"].double()).abs().sum(-1)           # (L, B, Q, cap)
    ref = c.w_line * l1 - c.w_class * pt
    cond = abs(c.w_line) * l1 + abs(c.w_class) * pt
    assert tuple(ref.shape) == (c.L, c.B, c.Q, c.cap) and bool(torch.isfinite(ref).all())
    return ref, (cond, None)


# ----------------------------------------------------------------------------------------------------------------- model
def model(c, inp, defect=None):
    assert defect is None or defect in DEFECTS
    lg = inp["logits"]
    mx = lg[..., 0]
    for k in range(1, c.K):
        mx = torch.maximum(mx, lg[..., k])
    if defect == "softmax_no_max":
        mx = torch.zeros_like(mx)
    e = torch.exp(lg - mx[..., None])
    s = torch.zeros_like(mx)
    for k in range(c.K):
        s = s + e[..., k]
    p = e / s[..., None]
    lab = inp["labels"] % c.K if defect == "label_unclamped_wraps" else inp["labels"].clamp(0, c.K - 1)
    l1 = torch.zeros(c.L, c.B, c.Q, c.cap)
    for d in range(c.D - (1 if defect == "d_last_dropped" else 0)):
        l1 = l1 + (inp["lines"][..., None, d] - inp["tgt"][:, d]).abs()
    w_line, w_class = torch.tensor(c.w_line, dtype=torch.float32), torch.tensor(c.w_class, dtype=torch.float32)
    cost = w_line * l1 + w_class * (-p[..., lab])
    if defect == "stride_tail_skipped":
        cost.view(-1)[MAX_BLOCKS * THREADS:] = float("nan")
    return cost


# ------------------------------------------------------------------------------------------------------------ constants
KEY = ("match_cost", "cost", "f32")


def check(c, got, inp, ref=None, cond=None, what=None):
    if ref is None:
        ref, cond = reference(c, inp)
    return assert_elementwise(got, ref, cond, C[KEY], AXES, u=U_F32, what=what or c.text)


def measure_c(case_list=None):
    worst = 0.0
    for c in (cases() if case_list is None else case_list):
        inp = inputs(c)
        ref, cond = reference(c, inp)
        worst = max(worst, float(ratio(model(c, inp), ref, cond, U_F32).max()))
    return {KEY: worst}


def format_table(worst):
    lines = ["    operation    output   type   model max   C", "    ----------   ------   ----   ---------   ----"]
    for (op, out, dt), v in sorted(worst.items()):
        lines.append("    %-10s   %-6s   %-4s   %9.3f   %4.1f" % (op, out, dt, v, c_of(v)))
    return "\n".join(lines)


MEASURED = {
    ("match_cost", "cost", "f32"): 2.121,
}
C = {k: c_of(v) for k, v in MEASURED.items()}
__doc__ = __doc__.replace("@TABLE@", format_table(MEASURED))
