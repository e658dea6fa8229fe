#!/usr/bin/env python
"""Writes tests/golden/row_witnesses.txt: for every kernel the twelve row entry points of csrc/rowops.hip and csrc/inorm.hip can
launch, the most demanding call that reaches it (format: tests/row_witness.py).  CPU only: the calls go through
tests/row_recorder.cpp, which links the two objects of gw_depth_amd/csrc against stubs of the HIP runtime.

    python tools/make_row_witnesses.py            # rewrites the fixture (after a change that is MEANT to move a shape)

The grid: ragged row counts from 1 to 300 007; for LayerNorm every channel count just above a (LPR, NCH) bucket's lower limit and at
its own limit, for the 16-byte and the 8-byte forms of both types, C = 160, padded rows whose last vector is part real and part
padding (30 in 32, 60 in 64, 300 in 304 and one per bucket), odd C and the fp32 C = 2 mod 4 above 256 of the generic kernels; softmax
rows on both sides of every NPL switch and of the long kernel; column sums with C = 96 (12 vectors per row: a threadblock tail);
the inorm shapes with empty slices, L = 1, one and 256 channel groups and a grid above the 256-block cap; every flag both ways.

Choice per kernel, among the calls that launch it (and nothing else; the inorm calls launch two) under row_witness.MAX_BYTES:
  0. the width (C and ld, or L): the kernels that the same widths of the grid reach take turns over them, in the order of their
     names, so that every width of a bucket occurs (PINNED fixes a width where the issue of this table names one);
  1. ragged rows: one point when rows is no multiple of the rows a wave handles at once, one when it is no multiple of a workgroup's,
     one when threads of the block stay without a row slot (256 % vectors per row);
  2. one point when the grid-stride loop runs at least twice and its last pass is partial, then one for more than one workgroup;
  3. the fewest bytes (optional operands not counted);
  4. the flags the selection does not look at (gamma / beta, residual, gskip, the ELU input, the activation, act_scale, mult, the
     per-channel scale, the mask and the scale; SF or SM, SB or SS): the kernels of one entry point and type take turns over the
     sorted lines, from both ends (turn k takes line k (n - 1) mod n), so that every flag occurs both ways.
tests/test_row_witnesses.py asserts that every form and every width named in the grid above occurs."""
import collections
import os
import re
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import row_witness as W        # noqa: E402

ROWS = [1, 3, 7, 13, 37, 101, 259, 1031, 2053, 4099, 8209, 12301, 16411, 24593, 33013, 49157, 150001, 300007]
LN_C = {   # (dtype, form) -> channel counts: per bucket of ld / VEC (8, 16, 32, 64, 128 slots) just above the previous limit and at its own
    (W.BF16, 16): [8, 64, 72, 128, 136, 160, 256, 264, 512],
    (W.BF16, 8): [4, 28, 36, 60, 68, 120, 124, 132, 252, 260, 300, 508],
    (W.F32, 16): [4, 32, 36, 64, 68, 128, 132, 160, 256, 260, 512],
    (W.F32, 8): [2, 14, 18, 30, 34, 62, 66, 126, 130, 254],
}
LN_PAD = {  # dtype -> (C, ld): the last vector part real and part padding
    W.BF16: [(5, 8), (30, 32), (60, 64), (67, 72), (121, 128), (130, 136), (250, 256), (257, 264), (300, 304), (509, 512)],
    W.F32: [(3, 4), (30, 32), (33, 36), (60, 64), (65, 68), (125, 128), (129, 132), (251, 256), (257, 260), (300, 304), (509, 512)],
}
LN_GENERIC = {W.BF16: [1, 7, 30, 161, 258, 511], W.F32: [1, 7, 33, 161, 258, 510, 511]}
SOFTMAX_L = [1, 63, 64, 65, 128, 129, 192, 193, 320, 321, 512, 513, 1024, 1025, 1200]
VEC_C = {W.BF16: [8, 64, 96, 160, 2048], W.F32: [4, 32, 48, 160, 1024]}          # 96 bf16 / 48 fp32: 12 vectors per row, 256 % 12 = 4 idle threads
GENERIC_C = [1, 7, 33, 161]
# B L cg S (cg = C / vector): empty slices (L < S) with one channel group; L = 1 (zero variance) with 256 groups; grids above the
# 256-block cap of the apply kernels (C = 16 bf16: 128 positions per block); L no multiple of S
INORM = ["%d %d %d %d" % s for s in [(3, 37, 1, 64), (2, 1, 256, 4), (2, 33013, 2, 32), (2, 66571, 1, 32), (3, 1001, 4, 6), (1, 5000, 16, 32)]]
# 16 jobs in one call: widths from one vector to 256, rows so that jobs 2, 3, 4, 9 and 15 own exactly one block (block0 moves by one)
COLSUM_JOBS = [(4099, 8), (37, 96), (16, 2048), (336, 96), (1, 8), (1031, 160), (2053, 64), (259, 2048), (101, 96), (512, 64), (8209, 96), (13, 160), (777, 8), (3, 64),
               (1000, 2048), (7, 96)]
PINNED = {"colsum_vec_kernelIDF16b": "96", "colsum_vec_kernelIf": "48",
          "layernorm_fwd_kernelIDF16b": "161/0", "layernorm_bwd_kernelIDF16b": "7/0", "layernorm_fwd_kernelIf": "511/0", "layernorm_bwd_kernelIf": "258/0",
          "inorm_stats_kernelIDF16b": "3 37 8 64", "inorm_gelu_fwd_kernelIDF16b": "2 33013 16 32", "inorm_gelu_bwd_sums_kernelIDF16b": "2 1 2048 4",
          "inorm_gelu_bwd_kernelIDF16b": "1 5000 128 32", "inorm_stats_kernelIf": "2 1 1024 4", "inorm_gelu_fwd_kernelIf": "2 66571 4 32",
          "inorm_gelu_bwd_sums_kernelIf": "3 1001 16 6", "inorm_gelu_bwd_kernelIf": "3 37 4 64"}


def flags(n):
    return [" ".join(str((i >> b) & 1) for b in range(n)) for i in range(1 << n)]


def grid():
    for dt in (W.BF16, W.F32):
        vec = 8 if dt == W.BF16 else 4
        widths = [(C, 0) for form in (16, 8) for C in LN_C[(dt, form)]] + LN_PAD[dt] + [(C, 0) for C in LN_GENERIC[dt]]
        for C, ld in widths:
            for rows in ROWS:
                for f in flags(3):
                    yield "LF %d %d %d %d %s" % (dt, rows, C, ld, f)
                for f in flags(5):
                    yield "LB %d %d %d %d %s" % (dt, rows, C, ld, f)
        for L in SOFTMAX_L:
            for rows in ROWS:
                yield "SF %d %d %d" % (dt, rows, L)
                yield "SB %d %d %d" % (dt, rows, L)
                for rpm in (1, 3, 7):
                    for sc in (0, 1):
                        yield "SM %d %d %d 1 %d %d" % (dt, rows, L, rpm, sc)
                yield "SM %d %d %d 0 0 1" % (dt, rows, L)
                yield "SS %d %d %d 1" % (dt, rows, L)
                yield "SS %d %d %d 0" % (dt, rows, L)
        for C in VEC_C[dt] + GENERIC_C:
            for rows in ROWS:
                yield "CS %d %d %d" % (dt, rows, C)
                for act in range(5):
                    for a in (0, 1):
                        for b in (0, 1):
                            yield "AB %d %d %d %d %d %d" % (dt, rows, C, act, a, b)
                            yield "AC %d %d %d %d %d %d" % (dt, rows, C, act, a, b)
        yield "CB %d %d %s" % (dt, len(COLSUM_JOBS), " ".join("%d %d" % (r, C * vec // 8) for r, C in COLSUM_JOBS))
        for s in INORM:
            B, L, cg, S = s.split()
            for op in ("IF", "IB"):
                yield "%s %d %s %s %d %s" % (op, dt, B, L, int(cg) * vec, S)


def width(c):
    if c.call in ("LF", "LB"):
        return "%d/%d" % (c.C, c.ld)
    if c.family == "softmax":
        return str(c.L)
    if c.call == "CB":
        return "batch"
    if c.family == "inorm":
        return "%d %d %d %d" % (c.B, c.L, c.C, c.S)
    return str(c.C)


def rows_per_block(c, kernel, block):
    """(rows a wave or row slot group handles at once, rows one workgroup handles per pass of its loop, idle threads)."""
    vec = 16 // W.esize(c)
    m = re.search(r"layernorm_(?:fwd|bwd)_vec_kernelI(?:DF16b|f)Li(\d+)E", kernel)
    if m:
        rpw = 64 // int(m.group(1))
        return rpw, rpw * block // 64, 0
    if "layernorm" in kernel or "softmax" in kernel:
        return 1, 4, 0
    if "act_bwd_vec" in kernel or "act_bwd_kernel" in kernel:
        return 1, 256, 0                                   # counted in vectors / elements, see units()
    if "colsum_kernel" in kernel:
        cw = 32 if c.C <= 32 else 64 if c.C <= 64 else 128 if c.C <= 128 else 256
        return 1, 256 // cw, c.C % cw
    vpr = c.C // vec
    return 1, 256 // vpr, 256 % vpr


def units(c, kernel):
    """What the kernel's grid-stride loop counts."""
    if "act_bwd_vec" in kernel:
        return c.rows * c.C // (16 // W.esize(c))
    if "act_bwd_kernel" in kernel:
        return c.rows * c.C
    return c.rows


def score(c, kernel, grid_x, block):
    if c.family == "inorm" or c.call == "CB":
        return (0, 0, 0)
    rpw, rpb, idle = rows_per_block(c, kernel, block)
    n = units(c, kernel)
    ragged = (rpw > 1 and n % rpw != 0) + (n % rpb != 0) + (idle != 0)
    one_pass = grid_x * rpb
    return (ragged, int(n > one_pass and n % one_pass != 0), int(grid_x > 1))


def base_bytes(c):
    d = dict(vars(c))
    for k in ("residual", "gskip", "mult", "mask"):
        if k in d:
            d[k] = 0
    return W.nbytes(type(c)(**d))


def build_table():
    """The text of the fixture and the chosen call per kernel."""
    cands = collections.defaultdict(list)          # kernel -> [(width, score, bytes, call)]
    with tempfile.TemporaryDirectory() as t:
        exe = W.build_recorder(t)
        calls = list(grid())
        for call, rec in zip(calls, W.replay(exe, calls)):
            rc, ls = W.launches(rec)
            c = W.parse_call(call)
            if rc != 0 or len(ls) != (2 if c.family == "inorm" else 1) or W.nbytes(c) > W.MAX_BYTES:
                continue
            for kernel, gx, block in ls:
                cands[kernel].append((width(c), score(c, kernel, gx, block), base_bytes(c), call))
    best = {}
    turn = collections.Counter()
    for kernel in sorted(cands):
        cs = cands[kernel]
        widths = sorted({w for w, _, _, _ in cs})
        pin = [v for k, v in PINNED.items() if k in kernel]
        w = pin[0] if pin else widths[turn[tuple(widths)] % len(widths)]
        turn[tuple(widths)] += 1
        cs = [x for x in cs if x[0] == w]
        top = max(x[1] for x in cs)
        cs = [x for x in cs if x[1] == top]
        low = min(x[2] for x in cs)
        forms = sorted(x[3] for x in cs if x[2] == low)
        key = (tuple(sorted({f.split()[0] for f in forms})), W.parse_call(forms[0]).dtype)
        best[kernel] = forms[turn[key] * (len(forms) - 1) % len(forms)]
        turn[key] += 1
    text = "# one call per kernel of the row entry points; written by tools/make_row_witnesses.py, format in tests/row_witness.py\n"
    text += "".join("%s %s\n" % (kernel, best[kernel]) for kernel in sorted(best))
    return text, best


def main():
    text, best = build_table()
    with open(W.FIXTURE, "w") as f:
        f.write(text)
    sizes = sorted(W.nbytes(W.parse_call(c)) for c in best.values())
    print("wrote %s: %d kernels, bytes median %.3g, max %.3g, sum %.3g" % (W.FIXTURE, len(best), sizes[len(sizes) // 2], sizes[-1], sum(sizes)))
    for fam, n in sorted(collections.Counter(W.parse_call(c).family for c in best.values()).items()):
        print("  %-10s %d" % (fam, n))


if __name__ == "__main__":
    main()
