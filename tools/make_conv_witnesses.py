#!/usr/bin/env python
"""Writes tests/golden/conv_witnesses.txt: for every kernel the convolution dispatcher can launch, the cheapest ragged call that
reaches it (format: tests/conv_witness.py).  CPU only: the calls go through the `--stdin` mode of tests/dispatch_recorder.cpp,
which links the objects of gw_depth_amd/csrc against stubs of the HIP runtime.

    python tools/make_conv_witnesses.py            # rewrites the fixture (after a change that is MEANT to move a shape)

The grid is the recorder's own grid plus small and ragged maps (odd H / W, M no multiple of 64 / 128 / 256, maps just above the
131 072 rows from which the 256-row tiles run), channel counts that are no multiple of a tile width and the 8-mod-32 channel tails;
all twelve epilogue kinds, both types, with and without zero page, single and batched weight gradients.

Choice per kernel, among the calls that launch it (and nothing else) below tests/conv_witness.py's MAX_MACS:
  1. the most ragged: one point each for a partial last 64-row tile, a Cout that is no multiple of 32, a Cin that is no multiple
     of 32, a workgroup count that is no multiple of the 256 CUs (a short last round - all that is left to the halo and
     parity variants, whose maps are whole patches), more than eight workgroups that are no multiple of eight (several
     tiles, and the remainder branch of the XCD band remap), and, for a filter wider than 1 x 1, a map wider than the filter (taps
     inside and outside the image), a reduction longer than twice the deepest ring (forward: K_len > 384 = 12 tiles of 32 channels;
     weight gradient: at least 1 024 rows), an act_scale that is no power of two, and a scaled weight gradient;
  2. among those, the fewest multiply-accumulates.
A kernel that only calls above MAX_MACS reach is an error."""
import collections
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import conv_witness as W        # noqa: E402

MAPS = [(8, 240, 320), (8, 120, 160), (8, 60, 80), (8, 30, 40), (8, 15, 20), (2, 96, 128), (2, 24, 32), (800, 1, 1), (2400, 1, 1),     # the recorder's
        (1, 7, 9), (2, 13, 17), (3, 19, 23), (1, 33, 47), (2, 61, 83), (77, 1, 1), (531, 1, 1),                                      # small, odd
        (1, 363, 363), (2, 257, 259), (3, 211, 209),                     # just above 131 072 rows, M no multiple of 64
        (33, 64, 64), (9, 128, 128), (17, 96, 96), (5, 168, 160)]        # whole 8 x 32 patches, a short last round of 256-row tiles
CHANNELS = [1, 2, 3, 8, 16, 24, 30, 32, 40, 48, 60, 64, 72, 80, 96, 104, 128, 136, 160, 200, 256, 320, 1024, 2048]
BATCH = 3


def grid():
    for dtype in (W.BF16, W.F32):
        for zp in ((1, 0) if dtype == W.BF16 else (1,)):      # the fp32 selection never looks at the zero page
            for m in MAPS:
                for cin in CHANNELS:
                    for cout in CHANNELS:
                        for k in (1, 2, 3):
                            for s in (1, 2):
                                for g in (0, 1, 2):
                                    if g == 2 and s == 2:
                                        continue              # refused by the library
                                    d = "%d %d %d %d %d %d %d %d %d %d" % (m[0], m[1], m[2], cin, cout, k, s, g, dtype, zp)
                                    for kind in range(len(W.KINDS)):
                                        if kind in (9, 10):               # ConvLn takes act_scale 1 only
                                            yield "F %s %d %d 0" % (d, kind, cout - 2 if cout % 8 == 0 and cout > 8 else 0)
                                            yield "F %s %d 0 0" % (d, kind)
                                            continue
                                        yield "F %s %d 0 1" % (d, kind)
                                        if kind == 0:                     # thin_dgrad_kernel takes the bare convolution only
                                            yield "F %s 0 0 0" % d
                                    yield "W %s 1" % d
                                    yield "W %s 0" % d                    # thin_wgrad_kernel takes no scale
                                    if dtype == W.BF16 and zp:
                                        yield "B %d %s 1" % (BATCH, d)


def score(call, groups):
    c = W.parse_call(call)
    m = c.B * c.Ho * c.Wo
    ragged = (m % 64 != 0) + (c.Cout % 32 != 0) + (c.Cin % 32 != 0) + (groups % 256 != 0) + (groups > 8 and groups % 8 != 0) + (c.k > 1 and min(c.Hi, c.Wi) > c.k)
    ragged += (c.K > 384) if c.call == "F" else (m >= 1024)
    ragged += (c.act_scale != 1.0) + (c.scaled != 0)
    return (-ragged, W.macs(c))


def main():
    best = {}
    reached = collections.Counter()
    with tempfile.TemporaryDirectory() as t:
        exe = W.build_recorder(t)
        chunk = []

        def flush():
            for call, rec in zip(chunk, W.replay(exe, chunk)):
                rc, ls = W.launches(rec)
                if rc != 0 or len(ls) != 1:
                    continue
                kernel, groups = ls[0]
                reached[kernel] += 1
                sc = score(call, groups)
                if sc[1] <= W.MAX_MACS and (kernel not in best or sc < best[kernel][0]):
                    best[kernel] = (sc, call)
            del chunk[:]
        for call in grid():
            chunk.append(call)
            if len(chunk) >= 200000:
                flush()
        flush()
    too_big = sorted(k for k in reached if k not in best)
    if too_big:
        sys.exit("only calls above %.0e multiply-accumulates reach:\n%s" % (W.MAX_MACS, "\n".join(too_big)))
    with open(W.FIXTURE, "w") as f:
        f.write("# one call per kernel of the convolution dispatch; written by tools/make_conv_witnesses.py, format in tests/conv_witness.py\n")
        for kernel in sorted(best):
            f.write("%s %s\n" % (kernel, best[kernel][1]))
    sizes = sorted(sc[1] for sc, _ in best.values())
    print("wrote %s: %d kernels, MACs median %.2g, max %.2g, sum %.2g" % (W.FIXTURE, len(best), sizes[len(sizes) // 2], sizes[-1], sum(sizes)))
    by_family = collections.Counter(W.family(k) for k in best)
    for fam, n in sorted(by_family.items()):
        print("  %-28s %d" % (fam, n))


if __name__ == "__main__":
    main()
