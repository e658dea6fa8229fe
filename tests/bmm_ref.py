"""fp64 reference, error bound and fp32 model of the library's own batched GEMM (csrc/bmm.hip, gwd_bmm: c[b0][b1] (M x N) =
alpha a (M x K) b (N x K)^T, each operand row-major in k or k-major, bf16 or fp32, optionally added into an fp32 result and split over
k; CPU only, plain module; the instrument is tests/attn_ref.py's).

A case is (dtype, a_kmajor, b_kmajor, M, N, K, nb0, nb1, alpha, splits, accumulate, kind).  ``inputs(c)`` draws, seeded from the case's
seed text, each operand as a VIEW (size, strides, offset) of a NaN-filled 1-D buffer: whatever the kernel reads outside the operand
is a NaN in the result.  Element 0 of a buffer is taken to be 16-byte aligned, so the view's offset and strides decide which branch of
load_vec a vector takes.  The kinds: ``plain`` (dense operands), ``unaligned`` (ld = 27 bf16 / 30 fp32, base moved by one element:
t[..., 1:] of a wider buffer), ``aligned`` (its twin: the same values, the same seed text, ld = 32 and no offset), ``heads_qk`` /
``heads_pv`` (the (B, L, 2E) -> (B, H, L, hd) head views of the fp32 attention path, nb0 = 3, nb1 = 5), ``a_bcast0`` (a has one b0),
``b_bcast`` (b has one matrix for the whole batch), ``acc`` (c holds nonzero values and is added to).

* ``launch(c)``: the launch arithmetic of gwd_bmm: kps (k per split, a multiple of BK), grid.x / y / z, the length of the last slice.
* ``reference(c, inp)`` -> (ref, cond), fp64, from the operands as stored:  ref = c0 + alpha a b^T,  cond = (0, |c0| + |alpha| sum_k |a||b|):
      |got - ref| <= C u (|ref| + (2^-24 / u) cond),   u that of the type stored in c (fp32 for an accumulated result)
  (products of the stored values accumulate in fp32 whatever the operand type; one rounding at the store).
* ``model(c, inp, defect=None)``: the kernel's arithmetic in fp32: per grid.z slice an fma chain over k in ascending order (each step
  the exact product added to the fp32 accumulator and rounded once), times alpha in fp32, then rounded to the storage type or added
  into c slice after slice.  Defects: ``k_tail_dropped`` (the last partial BK slab of a slice is ignored), ``edge_row`` (row M - 1 of
  a ragged tile is read from row M - 2), ``kmajor_swapped`` (a k-major operand is read as row-major where rows <= K keeps that inside
  the matrix), ``split_lost`` (the last grid.z slice is not added), ``unaligned_zero`` (the element-wise branch of load_vec - taken
  by a vector that is short or not 16-byte aligned - zero-fills one element too many).

The constants.  ``measure_c()``: largest |model - ref| / bound over the case list per (output, operand type); C twice that, one
decimal up.  CPU, 2026-10:

@TABLE@

(``c``: the result in the operands' type; ``acc``: the fp32 result that is added to.  A single rounding to bf16 gives up to 2.0 in
this measure.)  The atomics of a split reduction leave the order of the slices free; the bound covers any order, so no bit equality
is asked of those cases.  A kernel that needs more than its C has a defect or the bound lacks a term: neither is repaired by raising C.
"""
import types
import zlib

import torch

from tests.attn_ref import FLOOR, U_BF16, U_F32, assert_elementwise, ratio        # noqa: F401  (the instrument)
from tests.conv_ref import c_of

DEFECTS = ("k_tail_dropped", "edge_row", "kmajor_swapped", "split_lost", "unaligned_zero")
VEC = {"f32": 4, "bf16": 8}                                     # BCfg of csrc/bmm.hip
BK = {"f32": 16, "bf16": 32}
TILE = 64
MAX_BATCH, MAX_SPLITS = 65535, 65535
AXES = ("b0", "b1", "row", "column")
ALPHA = 0.37
ODD_LD = {"f32": 30, "bf16": 27}


def torch_dtype(c):
    return torch.bfloat16 if c.dtype == "bf16" else torch.float32


def launch(c):
    """The launch arithmetic of gwd_bmm."""
    bk = BK[c.dtype]
    kps = (c.K + c.splits - 1) // c.splits
    kps = (kps + bk - 1) // bk * bk
    gz = (c.K + kps - 1) // kps
    return types.SimpleNamespace(bk=bk, vec=VEC[c.dtype], kps=kps, grid_x=((c.M + 63) // 64) * ((c.N + 63) // 64), grid_y=c.nb0 * c.nb1,
                                 grid_z=gz, last=c.K - (gz - 1) * kps)


def _case(dtype, akm, bkm, M, N, K, kind="plain", nb0=1, nb1=1, alpha=ALPHA, splits=1, accumulate=False, seed=None):
    c = types.SimpleNamespace(dtype=dtype, akm=akm, bkm=bkm, M=M, N=N, K=K, kind=kind, nb0=nb0, nb1=nb1, alpha=alpha, splits=splits,
                              accumulate=accumulate)
    c.text = "bmm %s %s a=%s b=%s M=%d N=%d K=%d batch=%dx%d alpha=%g splits=%d acc=%d" % (
        dtype, kind, "km" if akm else "rm", "km" if bkm else "rm", M, N, K, nb0, nb1, alpha, splits, int(accumulate))
    c.seed_text = seed or c.text                                # twins share their values
    c.id = c.text.replace(" ", "-")
    return c


def k_tails(dt):
    v, bk = VEC[dt], BK[dt]
    return sorted({1, 3, v - 1, v, bk - 1, bk, 2 * bk + 1})


def cases():
    out = []
    for dt in ("f32", "bf16"):
        v, bk = VEC[dt], BK[dt]
        # every layout: a second tile row of one row, a second wave column of one column, one k past BK
        out += [_case(dt, akm, bkm, 65, 33, bk + 1) for akm in (False, True) for bkm in (False, True)]
        out += [_case(dt, km, km, 33, 17, K, alpha=-1.25) for km in (False, True) for K in k_tails(dt)]
        ld = ODD_LD[dt]
        for kind in ("unaligned", "aligned"):
            seed = "bmm %s vector loads" % dt
            out.append(_case(dt, False, False, 37, 21, ld - 1, kind, seed=seed + " rm"))
            out.append(_case(dt, True, True, ld - 1, ld - 1, 19, kind, seed=seed + " km"))
        out.append(_case(dt, False, False, 9, 9, 6, "heads_qk", 3, 5, alpha=6 ** -0.5))
        out.append(_case(dt, False, True, 9, 6, 9, "heads_pv", 3, 5, alpha=1.0))
        out.append(_case(dt, False, False, 20, 10, 12, "a_bcast0", 3, 5))
        out.append(_case(dt, False, True, 20, 10, 12, "b_bcast", 3, 5))
        out.append(_case(dt, True, True, 80, 64, 2 * bk + 5, "plain", splits=3, accumulate=True))
        out.append(_case(dt, True, False, 20, 12, bk + 3, "a_bcast0", 2, 2, splits=2, accumulate=True))
        out.append(_case(dt, False, True, 65, 33, bk + 1, "acc", splits=1, accumulate=True))
    return out


def rejected():
    """(name, descriptor fields that differ from a valid 8 x 8 x 8 product, return code): gwd_bmm returns before it launches."""
    return [("dtype", {"dtype": 7}, -2), ("K=0", {"K": 0}, -3), ("splits=0", {"splits": 0}, -3),
            ("splits-without-accumulate", {"splits": 2}, -4), ("batch=65536", {"nb0": 256, "nb1": 256}, -7)]


# ---------------------------------------------------------------------------------------------------------------- inputs
def _gen(c):
    g = torch.Generator()
    g.manual_seed(zlib.crc32(c.seed_text.encode()))
    return g


def _view(base, size, stride, offset):
    return types.SimpleNamespace(base=base, size=tuple(size), stride=tuple(stride), offset=offset,
                                 view=torch.as_strided(base, size, stride, offset))


def _operand(values, km, ld=None, offset=0):
    """values (n0, n1, rows, K) -> the operand as stored: (n0, n1, rows, K), or (n0, n1, K, rows) when k-major, row pitch ld."""
    st = values.transpose(-1, -2) if km else values
    n0, n1, outer, inner = st.shape
    ld = inner if ld is None else ld
    assert ld >= inner
    base = torch.full((offset + n0 * n1 * outer * ld,), float("nan"), dtype=values.dtype)
    op = _view(base, st.shape, (n1 * outer * ld, outer * ld, ld, 1), offset)
    op.view.copy_(st)
    return op


def _heads(values, E, second):
    """values (B, H, L, hd) -> the head view of channels [second E, second E + E) of a (B, L, 2E) buffer."""
    B, H, L, hd = values.shape
    assert H * hd == E
    base = torch.full((B * L * 2 * E,), float("nan"), dtype=values.dtype)
    op = _view(base, (B, H, L, hd), (L * 2 * E, hd, 2 * E, 1), E if second else 0)
    op.view.copy_(values)
    return op


def inputs(c):
    g, dt = _gen(c), torch_dtype(c)
    na = (1, c.nb1) if c.kind == "a_bcast0" else (c.nb0, c.nb1)
    nb = (1, 1) if c.kind == "b_bcast" else (c.nb0, c.nb1)
    a = torch.randn(na + (c.M, c.K), generator=g, dtype=torch.float64).to(dt)
    b = torch.randn(nb + (c.N, c.K), generator=g, dtype=torch.float64).to(dt)
    if c.kind in ("unaligned", "aligned"):
        ld, off = (ODD_LD[c.dtype], 1) if c.kind == "unaligned" else (32, 0)
        A, B = _operand(a, c.akm, ld, off), _operand(b, c.bkm, ld, off)
    elif c.kind == "heads_qk":                                  # q, k: (B, H, L, hd) row-major in k = hd
        A, B = _heads(a, c.nb1 * c.K, False), _heads(b, c.nb1 * c.K, True)
    elif c.kind == "heads_pv":                                  # p dense (B, H, L, L); v (B, H, L, hd) is b^T: k-major, rows = hd
        A, B = _operand(a, False), _heads(b.transpose(-1, -2).contiguous(), c.nb1 * c.N, True)
    else:
        A, B = _operand(a, c.akm), _operand(b, c.bkm)
    c0 = None
    if c.accumulate:
        c0 = torch.zeros(c.nb0, c.nb1, c.M, c.N)
        if c.kind == "acc":
            c0 = (3.0 * torch.randn(c0.shape, generator=g, dtype=torch.float64)).float()
    return {"a": A, "b": B, "c0": c0}


def _logical(op, km):
    return op.view.transpose(-1, -2) if km else op.view


def _alpha(c):
    return torch.tensor(c.alpha, dtype=torch.float32)


# ------------------------------------------------------------------------------------------------------------- reference
def reference(c, inp):
    a = _logical(inp["a"], c.akm).double().expand(c.nb0, c.nb1, c.M, c.K)
    b = _logical(inp["b"], c.bkm).double().expand(c.nb0, c.nb1, c.N, c.K)
    al = float(_alpha(c))
    ref = al * (a @ b.transpose(-1, -2))
    cond = abs(al) * (a.abs() @ b.abs().transpose(-1, -2))
    if c.accumulate:
        ref, cond = ref + inp["c0"].double(), cond + inp["c0"].double().abs()
    assert bool(torch.isfinite(ref).all())
    return ref, (torch.zeros_like(ref), cond)


# ----------------------------------------------------------------------------------------------------------------- model
def _batch_stride(op):
    return [0 if n == 1 else s for n, s in zip(op.size[:2], op.stride[:2])]


def _swapped(op, K):
    """The k-major operand (stored (K, rows)) read as (rows, K) with the same pitch -> logical (.., rows, K)."""
    rows = op.size[3]
    if rows > K:                                                # the read would leave the matrix: the shapes do not allow it
        return op.view.transpose(-1, -2)
    return torch.as_strided(op.base, op.size[:2] + (rows, K), op.stride, op.offset)


def _vectors(op, vec):
    """Per stored element: (its vector takes load_vec's element-wise branch, it is the last existing element of its vector).  A vector
    starts at every multiple of VEC along the inner dim (tiles start at multiples of 64 and BK); it is loaded whole when all VEC
    elements exist and its address - element 0 of the buffer being 16-byte aligned - is a multiple of 16 bytes = VEC elements."""
    n0, n1, outer, inner = op.size
    s0, s1 = _batch_stride(op)
    ar = lambda n, d: torch.arange(n).view([-1 if i == d else 1 for i in range(4)])
    i = ar(inner, 3)
    i0 = i // vec * vec
    n = (inner - i0).clamp_max(vec)
    addr0 = op.offset + ar(n0, 0) * s0 + ar(n1, 1) * s1 + ar(outer, 2) * op.stride[2] + i0
    slow = (n < vec) | (addr0 % vec != 0)
    return slow, (i == i0 + n - 1).expand_as(slow)


def load_branches(c, inp):
    """-> (vectors loaded whole, vectors loaded element by element) over both operands."""
    fast = slow = 0
    for op in (inp["a"], inp["b"]):
        s, last = _vectors(op, VEC[c.dtype])
        slow += int((s & last).sum())
        fast += int((~s & last).sum())
    return fast, slow


def _zero_tail(op, vec):
    """unaligned_zero: the stored view with the last element of every element-wise loaded vector zeroed."""
    slow, last = _vectors(op, vec)
    return torch.where(slow & last, torch.zeros((), dtype=op.view.dtype), op.view)


def model(c, inp, defect=None):
    assert defect is None or defect in DEFECTS
    L = launch(c)
    mats = []
    for op, km, rows in ((inp["a"], c.akm, c.M), (inp["b"], c.bkm, c.N)):
        if defect == "kmajor_swapped" and km:
            m = _swapped(op, c.K)
        elif defect == "unaligned_zero":
            st = _zero_tail(op, L.vec)
            m = st.transpose(-1, -2) if km else st
        else:
            m = _logical(op, km)
        mats.append(m.double().expand(c.nb0, c.nb1, rows, c.K))
    a, b = mats
    if defect == "edge_row" and c.M % TILE and c.M >= 2:
        a = a.clone()
        a[..., c.M - 1, :] = a[..., c.M - 2, :]
    alpha = _alpha(c)
    out = inp["c0"].clone() if c.accumulate else None
    slices = L.grid_z - (1 if defect == "split_lost" and L.grid_z > 1 else 0)
    for z in range(slices):
        k0, k1 = z * L.kps, min(c.K, (z + 1) * L.kps)
        if defect == "k_tail_dropped":
            k1 = k0 + (k1 - k0) // L.bk * L.bk
        acc = torch.zeros(c.nb0, c.nb1, c.M, c.N)
        for k in range(k0, k1):
            acc = (acc.double() + a[..., :, k, None] * b[..., None, :, k]).float()       # fma: one rounding
        v = acc * alpha
        out = out + v if c.accumulate else v.to(torch_dtype(c))
    return out


# ------------------------------------------------------------------------------------------------------------ constants
def key_of(c):
    return ("bmm", "acc" if c.accumulate else "c", c.dtype)


def unit_of(c):
    return U_F32 if c.accumulate or c.dtype == "f32" else U_BF16


def check(c, got, inp, ref=None, cond=None, what=None):
    if ref is None:
        ref, cond = reference(c, inp)
    return assert_elementwise(got, ref, cond, C[key_of(c)], AXES, u=unit_of(c), what=what or c.text)


def measure_c(case_list=None):
    worst = {}
    for c in (cases() if case_list is None else case_list):
        inp = inputs(c)
        ref, cond = reference(c, inp)
        r = float(ratio(model(c, inp), ref, cond, unit_of(c)).max())
        worst[key_of(c)] = max(worst.get(key_of(c), 0.0), r)
    return worst


def format_table(worst):
    lines = ["    operation   output   type   model max   C", "    ---------   ------   ----   ---------   ----"]
    for (op, out, dt), v in sorted(worst.items()):
        lines.append("    %-9s   %-6s   %-4s   %9.3f   %4.1f" % (op, out, dt, v, c_of(v)))
    return "\n".join(lines)


MEASURED = {
    ("bmm", "acc", "bf16"): 0.959,
    ("bmm", "acc", "f32"): 1.862,
    ("bmm", "c", "bf16"): 1.991,
    ("bmm", "c", "f32"): 1.935,
}
C = {k: c_of(v) for k, v in MEASURED.items()}
__doc__ = __doc__.replace("@TABLE@", format_table(MEASURED))
