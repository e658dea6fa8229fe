"""CPU: rendering of predict_frames' results (gwd_render_frames, ops.render_frames, InferenceSession(render=...), render.save_panels)
- everything that needs no GPU.

  * gw_depth_amd/csrc/rendergeom.h - the scalar geometry the device kernel calls - compiled for the host with g++ -ffp-contract=off
    (tests/rendergeom_host.cpp) against the numpy statement tests/render_ref.py: quantisation, per-pixel coverage, score index, bit
    for bit over the golden cases; the tile test never rejects a tile that holds a covered pixel;
  * known answers from the statement alone;
  * the colour tables against matplotlib (where it imports) and against tests/golden/render_lut.npy;
  * tests/golden/render.npz is what the statement gives and covers the cases;
  * header, binding and Makefile agree; the entry point refuses bad arguments before any launch (there is no GPU here);
  * ops.render_frames and the session's plumbing over a stand-in library (tests/render_fake.py);
  * save_panels round-trips through Pillow byte for byte."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from gw_depth_amd import data, hip, infer, ops
from gw_depth_amd import render as R
from gw_depth_amd.infer import FUSION_KEYS, NMS_KEYS, PROFILE_KEYS, REGION_KEYS, RENDER_KEYS, RESULT_KEYS, InferenceSession
from tests import render_cases as K
from tests import render_ref as P
from tests.render_fake import RenderFakeDevice
from tests.test_frames_post import BUDGET, FramesFakeDevice, TinyModel, frames_of

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = P.load_golden()
CASES = {name: make() for name, make in K.CASES.items()}                               # built once, never written to
OPTS = dict(width8=16, end_radius=2, min_score=float("-inf"), score_lo=0.92, score_k=256.0 / (1.02 - 0.92))


def drawn_rows(case):
    """Per frame: (fh, fw), the drawn rows, the options."""
    shape, _, _, _, _, _, _, opts = K.operands(case)
    out = []
    for b in range(shape[0]):
        fh, fw = P.frame_size(b, case["sizes"], shape[2], shape[3], [])
        out.append(((fh, fw), P.rows_of(b, case["lines"].shape[1], case["lines"], case["count"], case["order"], case["scores"], case["kinds"], opts), opts))
    return out


# ------------------------------------------------------------------------------------------------------------------ host geometry
@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("rendergeom") / "librendergeom_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-I",
                           os.path.join(ROOT, "gw_depth_amd", "csrc"), os.path.join(HERE, "rendergeom_host.cpp"), "-o", out])
    lib = ctypes.CDLL(out)
    i32p = ctypes.POINTER(ctypes.c_int32)
    lib.rg_host_quantise.argtypes = [ctypes.POINTER(ctypes.c_double), i32p]
    lib.rg_host_cover.argtypes = [i32p] + [ctypes.c_int32] * 4 + [ctypes.POINTER(ctypes.c_uint8)]
    lib.rg_host_tile.argtypes = [i32p] + [ctypes.c_int32] * 5
    lib.rg_host_score_index.argtypes = [ctypes.c_double] * 3
    return lib


def host_cover(lib, row, h, radius, fh, fw):
    buf = (ctypes.c_uint8 * (fh * fw))()
    lib.rg_host_cover((ctypes.c_int32 * 4)(*row), h, radius, fh, fw, buf)
    return np.frombuffer(buf, dtype=np.uint8).reshape(fh, fw)


def test_host_build_quantises_as_the_statement(host_lib):
    q = (ctypes.c_int32 * 4)()
    seen = 0
    rows = [r for case in CASES.values() for r in case["lines"].reshape(-1, 4)]
    rows += [(0.03124, 0.03125, -0.03125, -0.03126), (32767.0, -32767.0, 0.5, -0.5), (32767.01, 0, 0, 0), (0, 0, 0, -32768.0),
             (math.nan, 0, 0, 0), (0, math.inf, 0, 0), (0, 0, -math.inf, 0), (1e300, 0, 0, 0), (5e-324, -5e-324, 0.96875, 0.968749999)]
    for v in rows:
        v = np.asarray(v, np.float64)
        ok = bool(np.isfinite(v).all() and (np.abs(v) <= P.MAX_COORD).all())
        assert host_lib.rg_host_quantise((ctypes.c_double * 4)(*v), q) == int(ok), v
        if ok:
            assert list(q) == [P.quantise(c) for c in v], v
            seen += 1
    assert seen > 2500
    assert P.quantise(0.03124) == 0 and P.quantise(0.03125) == 1 and P.quantise(-0.03125) == 0 and P.quantise(-0.03126) == -1      # half up


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_build_covers_the_statements_pixels_and_never_rejects_their_tile(host_lib, name):
    """Per drawn row of the golden cases (a seeded subset of the two long lists): coverage and end discs of every pixel of the frame
    equal the statement's; every tile of the kernel's grid that holds such a pixel passes the tile test, at the row's own reach and
    for tiles of other sizes too."""
    rng = np.random.default_rng(5)
    pixels = tiles = 0
    for (fh, fw), rows, opts in drawn_rows(CASES[name]):
        if not fh:
            continue
        if len(rows) > 80:
            rows = [rows[k] for k in sorted(rng.choice(len(rows), 80, replace=False))]
        h, radius = opts["width8"], 16 * opts["end_radius"]
        py, px = np.meshgrid(16 * np.arange(fh, dtype=np.int64) + 8, 16 * np.arange(fw, dtype=np.int64) + 8, indexing="ij")
        for _, row, _, _ in rows:
            want = P.covered(px, py, row, h).astype(np.uint8) | (2 * (P.disc(px, py, row[0], row[1], radius) | P.disc(px, py, row[2], row[3], radius))).astype(np.uint8)
            got = host_cover(host_lib, row, h, radius, fh, fw)
            assert np.array_equal(got, want), (name, row)
            pixels += int((want != 0).sum())
            q = (ctypes.c_int32 * 4)(*row)
            for tw, th in ((P.TILE_W, P.TILE_H), (16, 16), (7, 3)):
                for y0 in range(0, fh, th):
                    for x0 in range(0, fw, tw):
                        y1, x1 = min(y0 + th, fh) - 1, min(x0 + tw, fw) - 1
                        if want[y0:y1 + 1, x0:x1 + 1].any():
                            tiles += 1
                            assert host_lib.rg_host_tile(q, x0, y0, x1, y1, max(h, radius)) == 1, (name, row, x0, y0)
    assert pixels > 300 and tiles > 30


def test_tile_test_rejects_what_is_far(host_lib):
    """Not required for correctness, but what binning is for: a tile away from the row's bounding box, and one inside the box of a
    long diagonal but far from the line, are rejected."""
    row = (ctypes.c_int32 * 4)(0, 0, 16 * 1000, 16 * 1000)
    assert host_lib.rg_host_tile(row, 0, 0, 63, 15, 16) == 1 and host_lib.rg_host_tile(row, 500, 484, 563, 499, 16) == 1
    assert host_lib.rg_host_tile(row, 1100, 0, 1163, 15, 16) == 0                      # outside the box
    assert host_lib.rg_host_tile(row, 64, 900, 127, 915, 16) == 0                      # inside the box, far from the line
    assert host_lib.rg_host_tile(row, 64, 900, 127, 915, 1024) == 0 and host_lib.rg_host_tile(row, 440, 500, 503, 515, 1024) == 1
    far = (ctypes.c_int32 * 4)(-16 * 30000, 0, 16 * 30000, 16 * 30000)               # |cross product| beyond 2^31 at the corners
    assert host_lib.rg_host_tile(far, 0, 12000, 63, 12015, 128) == 0 and host_lib.rg_host_tile(far, 0, 15000, 63, 15015, 128) == 1


def test_host_build_gives_the_statements_score_index(host_lib):
    lo, k = OPTS["score_lo"], OPTS["score_k"]
    cases = [0.92, 1.02, 0.0, -1.0, 2.0, 1e300, -1e300, math.inf, -math.inf, math.nextafter(0.92, 0.0), math.nextafter(0.92, 1.0), math.nextafter(1.02, 0.0)]
    cases += [0.92 + 0.1 * j / 256.0 for j in range(257)] + [math.nextafter(0.92 + 0.1 * j / 256.0, 0.0) for j in range(257)]
    cases += [float(np.float32(v)) for v in np.random.default_rng(3).uniform(0.9, 1.04, 500)]
    for s in cases:
        assert host_lib.rg_host_score_index(s, lo, k) == P.score_index(s, lo, k), s
    assert P.score_index(0.92, lo, k) == 0 and P.score_index(1.02, lo, k) == 255 and P.score_index(0.97, lo, k) in (127, 128)
    assert {P.score_index(s, lo, k) for s in cases} == set(range(256))


# ------------------------------------------------------------------------------------------------------------------ known answers
def grid(fh, fw):
    return np.meshgrid(16 * np.arange(fh, dtype=np.int64) + 8, 16 * np.arange(fw, dtype=np.int64) + 8, indexing="ij")


def test_horizontal_width_two_line_covers_three_rows_ties_inside():
    py, px = grid(20, 30)
    row = tuple(P.quantise(v) for v in (5.0, 10.5, 20.0, 10.5))
    got = P.covered(px, py, row, 16)                                                    # width 2: h = 16 sixteenths
    assert got[9:12, 5:20].all() and not got[8].any() and not got[12].any()            # centres 9.5, 10.5, 11.5: |dy| = 1, 0, 1 <= 1
    assert got[10, 4] and not got[10, 3] and got[10, 20] and not got[10, 21]           # the round caps reach one centre further along
    assert not got[9, 4] and not got[11, 20]                                           # ... and fall short of the diagonal ones
    assert int(got.sum()) == 3 * 15 + 2
    assert not P.covered(px, py, row, 15)[9].any()                                      # one sixteenth narrower: the tie rows go


def test_zero_length_row_is_a_disc_and_the_tie_at_exactly_h():
    py, px = grid(24, 24)
    row = tuple(P.quantise(v) for v in (10.5, 10.5, 10.5, 10.5))
    got = P.covered(px, py, row, 5 * 16)
    want = (px - 168) ** 2 + (py - 168) ** 2 <= 80 * 80
    assert np.array_equal(got, want) and got[10, 15] and got[10, 5] and got[13, 14] and not got[14, 14]      # (3, 4, 5): the tie is inside
    assert np.array_equal(P.disc(px, py, 168, 168, 80), want)
    long_row = (8, 8, 16 * 23 + 8, 8)                                                   # pixel centres along y = 0.5
    assert P.covered(px, py, long_row, 48)[3, 5] and not P.covered(px, py, long_row, 47)[3, 5]      # distance exactly 3 pixels


def one_frame(fh, fw, panels, lines=None, scores=None, kinds=None, order=None, label=None, mm=None, rmap=None, frame=None, **options):
    n = 0 if lines is None else len(lines)
    case = dict(sizes=np.asarray([(fh, fw)], np.int32), panels=panels, frames=None if frame is None else [frame],
                planes=[] if mm is None else [mm[None]], label_planes=[] if label is None else [label[None]],
                region_map=None if rmap is None else rmap[None], lines=None if lines is None else np.asarray([lines], np.float64),
                count=None if lines is None else np.asarray([n], np.int32), order=order, scores=None if scores is None else np.asarray([scores], np.float64),
                kinds=None if kinds is None else np.asarray([kinds], np.int32), options=dict({"canvas_size": (fh, fw)}, **options))
    return K.statement(case)[0]


def test_the_lowest_row_wins_whatever_the_order_of_the_list():
    lines = [(2.0, 8.5, 28.0, 8.5), (15.5, 1.0, 15.5, 15.0)]
    a = one_frame(16, 32, [{"base": "black", "lines": "kind", "ends": False}], lines, kinds=[1, 2])
    kc = np.asarray(R.KIND_COLORS, np.uint8)
    assert (a[0, 8, 15] == kc[1]).all() and (a[0, 3, 15] == kc[2]).all() and (a[0, 8, 3] == kc[1]).all() and not a[0, 0, 0].any()
    b = one_frame(16, 32, [{"base": "black", "lines": "kind", "ends": False}], lines[::-1], kinds=[2, 1])
    assert (b[0, 8, 15] == kc[2]).all()                                                 # the same lines, the other one first
    c = one_frame(16, 32, [{"base": "black", "lines": "kind", "ends": False}], lines[::-1], kinds=[1, 2], order=np.asarray([[1, 0]], np.int32))
    assert np.array_equal(c, a)                                                         # row 0 reads source 1: row order decides, kinds go by row
    ends = one_frame(16, 32, [{"base": "black", "lines": "kind"}], lines, kinds=[1, 2], end_radius=1)
    assert (ends[0, 8, 2] == R.END_COLOR).all() and (ends[0, 1, 15] == R.END_COLOR).all() and (ends[0, 8, 15] == kc[1]).all()      # above all lines


def test_one_pixel_region_is_its_own_outline_and_a_block_keeps_its_inside():
    rmap = np.zeros((12, 12), np.uint8)
    rmap[5, 5] = 2
    rmap[7:12, 0:4] = 1                                                                 # touches the frame's left and bottom border
    out = one_frame(12, 12, [{"base": "black", "outlines": True}], rmap=rmap)[0]
    colors = R.region_colors()
    assert (out[5, 5] == colors[1]).all() and (colors[1] == R.jet_table()[8 * 16 + 4]).all()      # rank 2 -> index 1 -> bitrev5(1) = 16
    block = np.zeros((12, 12), bool)
    block[7:12, 0:4] = True
    block[8:11, 1:3] = False                                                            # 4-neighbours all rank 1 and inside the frame
    assert ((out == colors[0]).all(-1) == block).all() and (colors[0] == R.jet_table()[4]).all()


def test_tint_with_alpha_0_is_the_identity_and_256_a_replacement():
    frame = np.random.default_rng(1).integers(0, 256, (6, 7, 3)).astype(np.uint8)
    label = np.zeros((6, 7), np.uint8)
    label[2:4] = 1
    label[5] = 2
    for alpha, want in ((0, frame), (256, np.where((label == 1)[..., None], np.asarray((9, 200, 255), np.uint8), frame))):
        out = one_frame(6, 7, [{"base": "frame", "tint": 0, "tint_alpha": alpha, "tint_color": (9, 200, 255)}], label=label, frame=frame)[0]
        assert np.array_equal(out, want), alpha
    half = one_frame(6, 7, [{"base": "frame", "tint": 0, "tint_alpha": 128, "tint_color": (255, 0, 1)}], label=label, frame=frame)[0]
    assert np.array_equal(half[2], (frame[2].astype(int) * 128 + np.asarray((255, 0, 1)) * 128 + 128) >> 8) and np.array_equal(half[0], frame[0])
    assert (P.tint(255, 255, 77) == 255) and (P.tint(0, 0, 77) == 0)                  # no channel leaves 0 .. 255


def test_depth_indices_at_the_ends_of_the_range():
    assert P.depth_index([0, 1, 16, 17, 50, 150, 8483, 8484, 8500, 65535], 0, 8500).tolist() == [0, 0, 0, 1, 2, 5, 254, 255, 255, 255]
    assert [int(P.depth_index(m, 0, 8500)) for m in (50, 150, 250)] == [2, 5, 8]        # x.5 goes up, where OpenCV's cvRound goes to even
    assert P.depth_index([0, 999, 1000, 1001, 1002, 2000], 1000, 2000).tolist() == [0, 0, 0, 0, 1, 255]
    mm = np.asarray([[0, 1, 8500, 65535]], np.uint16)
    out = one_frame(1, 4, [{"base": ("depth", 0), "void": (7, 8, 9)}], mm=mm)[0, 0]
    jet = R.jet_table()
    assert out.tolist() == [[7, 8, 9], jet[0].tolist(), jet[255].tolist(), jet[255].tolist()]      # 0 mm is void, not the table's first entry


# ------------------------------------------------------------------------------------------------------------------ the tables
def test_default_table_is_matplotlibs_jet():
    cm = pytest.importorskip("matplotlib").colormaps["jet"]
    assert np.array_equal(cm(np.arange(256), bytes=True)[:, :3], R.jet_table())


def test_tables_are_pinned_and_written_twice():
    lut = np.load(P.GOLDEN_LUT)
    assert lut.dtype == np.uint8 and lut.shape == (256, 3)
    assert np.array_equal(R.jet_table(), lut) and np.array_equal(P.jet_table(), lut)
    assert lut[0].tolist() == [0, 0, 127] and lut[255].tolist() == [127, 0, 0] and lut[128].tolist()[1] == 255
    pal = R.voc_palette()
    assert np.array_equal(pal, P.voc_palette()) and pal[255].tolist() == [0, 0, 0]
    first = [(0, 0, 0), (128, 0, 0), (0, 128, 0), (128, 128, 0), (0, 0, 128), (128, 0, 128), (0, 128, 128), (128, 128, 128), (64, 0, 0), (192, 0, 0),
             (64, 128, 0), (192, 128, 0), (64, 0, 128), (192, 0, 128), (64, 128, 128), (192, 128, 128), (0, 64, 0), (128, 64, 0), (0, 192, 0),
             (128, 192, 0), (0, 64, 128)]                                               # the 21 PASCAL-VOC classes
    assert [tuple(c) for c in pal[:21].tolist()] == first and len({tuple(c) for c in pal[:255].tolist()}) == 255
    assert len({tuple(c) for c in R.region_colors()[:32].tolist()}) == 32


# ------------------------------------------------------------------------------------------------------------------ the fixture
def test_fixture_is_what_the_statement_gives_and_covers_the_cases():
    assert os.path.getsize(P.GOLDEN) < 256 * 1024
    painted = {"tint": 0, "outline": 0, "lines": 0, "ends": 0, "void": 0, "outside": 0}
    bases, modes, most = set(), set(), 0
    for name, case in CASES.items():
        for key in ("sizes", "lines", "count", "order", "scores", "kinds", "region_map"):
            assert (case[key] is None) == ("%s.%s" % (name, key) not in GOLD), (name, key)
            if case[key] is not None:
                assert np.array_equal(GOLD["%s.%s" % (name, key)], case[key], equal_nan=True), (name, key)
        for key in ("planes", "label_planes"):
            for i, v in enumerate(case[key]):
                assert np.array_equal(GOLD["%s.%s%d" % (name, key, i)], v)
        for b, f in enumerate(case["frames"] or []):
            assert np.array_equal(GOLD["%s.frame%d" % (name, b)], f)
        canvas = K.statement(case)
        assert np.array_equal(GOLD["%s.canvas" % name], canvas), name
        # what each layer painted: the same case with the layer taken out differs somewhere
        shape, tables, recs, frames, planes, labels, rmap, opts = K.operands(case)
        for r in recs:
            bases.add(r["base"])
            modes.add(r["lines"])
        args = (shape, case["sizes"], tables)
        rest = (frames, planes, labels, rmap, case["lines"], case["count"], case["order"], case["scores"], case["kinds"], opts)
        for layer, off in (("tint", dict(tint=-1)), ("outline", dict(outlines=0)), ("lines", dict(lines=P.LINES_NONE)), ("ends", dict(ends=0))):
            painted[layer] += int((P.render(*args, [dict(r, **off) for r in recs], *rest) != canvas).any(-1).sum())
        for k, r in enumerate(recs):
            if r["base"] == P.DEPTH:
                painted["void"] += int(sum((planes[r["plane"]][b][:s[0], :s[1]] == 0).sum() for b, s in enumerate(case["sizes"])))
        for b, (fh, fw) in enumerate(case["sizes"]):
            outside = np.ones(shape[2:], bool)
            outside[:fh, :fw] = False
            painted["outside"] += int(outside.sum())
            assert not canvas[b][:, outside].any()
        for (fh, fw), rows, opts in drawn_rows(case):
            if fh and name in ("overflow", "ragged"):
                most = max(most, int(P.rows_through_tiles(fh, fw, rows, opts).max()))
    assert all(v > 0 for v in painted.values()), painted
    assert bases == {P.BLACK, P.FRAME, P.DEPTH, P.LABELS} and modes == {P.LINES_NONE, P.LINES_SCORE, P.LINES_KIND, P.LINES_FIXED}
    assert most > P.LIST                                                                # a tile with more rows than the kernel's list holds
    rows = drawn_rows(CASES["ragged"])
    assert [len(r[1]) for r in rows] == [33, 31, 0]                                     # min_score, NaN, bad sources and coordinates took theirs
    assert CASES["many"]["lines"].shape[1] == hip.PROFILE_MAX_LINES


# ------------------------------------------------------------------------------------------------------------------ the ABI
def test_header_binding_and_makefile_agree(tmp_path):
    header = open(os.path.join(ROOT, "include", "gwdepth.h")).read()
    for name, value in (("GWD_RENDER_MAX_PANELS", hip.RENDER_MAX_PANELS), ("GWD_RENDER_MAX_PLANES", hip.RENDER_MAX_PLANES),
                        ("GWD_RENDER_MAX_TABLES", hip.RENDER_MAX_TABLES), ("GWD_RENDER_MAX_WIDTH8", hip.RENDER_MAX_WIDTH8),
                        ("GWD_RENDER_MAX_END_RADIUS", hip.RENDER_MAX_END_RADIUS), ("GWD_RENDER_BLACK", R.BLACK), ("GWD_RENDER_FRAME", R.FRAME),
                        ("GWD_RENDER_DEPTH", R.DEPTH), ("GWD_RENDER_LABELS", R.LABELS), ("GWD_RENDER_LINES_NONE", R.LINES_NONE),
                        ("GWD_RENDER_LINES_SCORE", R.LINES_SCORE), ("GWD_RENDER_LINES_KIND", R.LINES_KIND), ("GWD_RENDER_LINES_FIXED", R.LINES_FIXED)):
        assert "#define %s %d" % (name, value) in header, name
    assert (R.MAX_PANELS, R.MAX_PLANES, R.MAX_TABLES, R.MAX_WIDTH8, R.MAX_END_RADIUS) == \
        (hip.RENDER_MAX_PANELS, hip.RENDER_MAX_PLANES, hip.RENDER_MAX_TABLES, hip.RENDER_MAX_WIDTH8, hip.RENDER_MAX_END_RADIUS)
    assert (P.BLACK, P.FRAME, P.DEPTH, P.LABELS, P.LINES_NONE, P.LINES_SCORE, P.LINES_KIND, P.LINES_FIXED) == \
        (R.BLACK, R.FRAME, R.DEPTH, R.LABELS, R.LINES_NONE, R.LINES_SCORE, R.LINES_KIND, R.LINES_FIXED)
    assert "#define GWD_VERSION 10" in header and "gwd_render_frames" in hip.ENTRY_POINTS
    make = open(os.path.join(ROOT, "gw_depth_amd", "csrc", "Makefile")).read()
    # render.o follows rendergeom.h through the dependencies the compiler writes: the flags ask for them and the Makefile reads them
    assert "render.hip" in make and re.search(r"^CXXFLAGS\b.*-MMD", make, re.M) and re.search(r"^-include \$\(OBJS:\.o=\.d\)", make, re.M)
    kernel = open(os.path.join(ROOT, "gw_depth_amd", "csrc", "render.hip")).read()
    assert '#include "rendergeom.h"' in kernel and "kList = %d" % P.LIST in kernel and "kTileW = %d, kTileH = %d" % (P.TILE_W, P.TILE_H) in kernel
    assert infer.RENDER_KEYS == ops.RENDER_KEYS == ("canvas",)
    # the descriptor's layout, as a C compiler lays the header out
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include "gwdepth.h"\n'
                   'long layout(int k) { switch (k) { case 0: return sizeof(gwd_render_desc); case 1: return offsetof(gwd_render_desc, min_score);\n'
                   'case 2: return offsetof(gwd_render_desc, B); case 3: return offsetof(gwd_render_desc, ext_h); case 4: return offsetof(gwd_render_desc, frames);\n'
                   'case 5: return offsetof(gwd_render_desc, planes); case 6: return offsetof(gwd_render_desc, panels); case 7: return sizeof(gwd_render_panel);\n'
                   'case 8: return offsetof(gwd_render_panel, void_rgb); case 9: return sizeof(gwd_render_slot); default: return -1; } }\n')
    out = str(tmp_path / "liblayout.so")
    subprocess.check_call(["gcc", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"), str(src), "-o", out])
    layout = ctypes.CDLL(out).layout
    layout.restype = ctypes.c_long
    D, Pn = hip.RenderDesc, hip.RenderPanel
    want = [ctypes.sizeof(D), D.min_score.offset, D.B.offset, D.ext_h.offset, D.frames.offset, D.planes.offset, D.panels.offset, ctypes.sizeof(Pn),
            Pn.void_rgb.offset, ctypes.sizeof(hip.RenderSlot)]
    assert [layout(k) for k in range(10)] == want and ctypes.sizeof(D) < 4096       # it travels by value as a kernel argument


def test_entry_point_refuses_before_any_launch():
    """Every call below must return before the launch: this host has no device to launch on."""
    lib = hip.HipLibrary()
    assert lib.version() == 10
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(buf, ctypes.c_void_p).value
    p += (-p) % 16

    def call(edit=None, panel=None, **kw):
        d = hip.RenderDesc()
        d.canvas, d.sizes, d.tables, d.lines, d.count, d.scores, d.kinds = p, p, p, p, p, p, p
        d.B, d.P, d.Fh, d.Fw, d.C, d.n_planes, d.n_label_planes, d.n_tables = 2, 1, 8, 8, 4, 1, 1, 2
        d.lines_dtype, d.scores_dtype, d.width8, d.end_radius, d.has_frames, d.has_region_map = 1, 0, 16, 2, 1, 1
        d.min_score, d.score_lo, d.score_k = -math.inf, 0.92, 2560.0
        for slot in (d.frames, d.region_map, d.planes[0], d.label_planes[0]):
            for b in range(2):
                slot.ptr[b], slot.pitch[b] = p, 8
        for b in range(2):
            d.ext_h[b] = d.ext_w[b] = 8
        pn = d.panels[0]
        pn.base, pn.plane, pn.table, pn.lo_mm, pn.hi_mm, pn.tint, pn.tint_alpha, pn.outlines, pn.lines, pn.ends = R.DEPTH, 0, 0, 0, 8500, 0, 100, 1, R.LINES_SCORE, 1
        for k, v in kw.items():
            setattr(d, k, v)
        for k, v in (panel or {}).items():
            setattr(pn, k, v)
        if edit:
            edit(d)
        return lib.lib.gwd_render_frames(ctypes.byref(d), None)

    def slot_ptr(name, value, index=None):
        def edit(d):
            s = getattr(d, name) if index is None else getattr(d, name)[index]
            s.ptr[1] = value
        return edit

    assert lib.lib.gwd_render_frames(None, None) == -1
    for k in ("canvas", "sizes", "tables", "count"):
        assert call(**{k: None}) == -1, k
    assert call(B=0) == -1 and call(B=17) == -1 and call(P=0) == -1 and call(P=9) == -1 and call(Fh=0) == -1 and call(Fw=16385) == -1
    assert call(n_planes=5) == -1 and call(n_label_planes=-1) == -1 and call(n_tables=0) == -1 and call(n_tables=17) == -1
    assert call(C=0) == -1 and call(C=2049) == -1 and call(width8=0) == -1 and call(width8=129) == -1 and call(end_radius=-1) == -1 and call(end_radius=65) == -1
    assert call(min_score=math.nan) == -1 and call(score_k=0.0) == -1 and call(score_k=math.inf) == -1 and call(score_lo=math.nan) == -1
    assert call(lines=None) == -1                                                       # count, scores, kinds without lines
    assert call(edit=slot_ptr("frames", None)) == -1 and call(edit=slot_ptr("planes", None, 0)) == -1 and call(edit=slot_ptr("region_map", None)) == -1
    assert call(edit=lambda d: d.ext_h.__setitem__(1, -1)) == -1
    assert call(lines_dtype=2) == -2 and call(scores_dtype=-1) == -2
    assert call(panel=dict(base=4)) == -2 and call(panel=dict(base=-1)) == -2 and call(panel=dict(plane=1)) == -2 and call(panel=dict(table=2)) == -2
    assert call(panel=dict(lo_mm=8500)) == -2 and call(panel=dict(hi_mm=65536)) == -2 and call(panel=dict(lo_mm=-1)) == -2
    assert call(panel=dict(tint=1)) == -2 and call(panel=dict(tint_alpha=257)) == -2 and call(panel=dict(region_table=2)) == -2
    assert call(panel=dict(lines=4)) == -2 and call(panel=dict(line_table=2)) == -2 and call(panel=dict(lines=R.LINES_KIND), kinds=None) == -2
    assert call(scores=None) == -2 and call(panel=dict(base=R.FRAME), has_frames=0) == -2 and call(has_region_map=0) == -2
    assert call(lines=None, count=None, scores=None, kinds=None) == -2                  # a panel with lines, a call without
    assert call(canvas=p + 8) == -3 and call(sizes=p + 2) == -3 and call(lines=p + 4) == -3 and call(scores=p + 2) == -3 and call(kinds=p + 1) == -3
    assert call(edit=slot_ptr("planes", p + 1, 0)) == -3 and call(order=p + 2) == -3
    assert call(canvas=p + 8, B=0) == -1


# ------------------------------------------------------------------------------------------------------------------ host logic
@pytest.fixture
def fake(monkeypatch):
    lib = RenderFakeDevice()
    upload = data.upload_tables

    def counted(host, device):
        lib.calls["upload_tables"] += 1
        return upload(host, device)

    monkeypatch.setattr(data, "upload_tables", counted)
    hip.set_library(lib)
    yield lib
    hip.set_library(None)


@pytest.mark.parametrize("views", [False, True], ids=["tensors", "views"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_render_frames_gives_the_fixture(fake, name, views):
    canvas = K.call(CASES[name], views=views)
    want = GOLD["%s.canvas" % name]
    assert canvas.dtype == torch.uint8 and tuple(canvas.shape) == want.shape and np.array_equal(canvas.numpy(), want)
    rec = fake.render_calls[-1]
    assert rec["shape"] == want.shape and rec["rows"] == tuple(CASES[name]["lines"].shape[:2]) and rec["after"] == (0, 0, 0)


def test_render_frames_validates_before_any_launch(fake):
    case = CASES["ragged"]
    T = lambda v: torch.from_numpy(np.ascontiguousarray(v))
    sizes, mm, labels, lines, count = T(case["sizes"]), T(case["planes"][0]), T(case["label_planes"][0]), T(case["lines"]), T(case["count"])
    for kw in ({"width": 0.0}, {"width": 16.5}, {"width": 0.01}, {"end_radius": -1}, {"end_radius": 65}, {"end_radius": 1.5}, {"score_range": (1.0, 1.0)},
               {"score_range": (0.0, math.inf)}, {"min_score": math.nan}, {"canvas_size": (0, 5)}, {"canvas_size": (16385, 5)}):
        with pytest.raises(ValueError):
            ops.render_frames(sizes, ["black"], **kw)
    with pytest.raises(TypeError, match="unknown option"):
        ops.render_frames(sizes, ["black"], thickness=2)
    with pytest.raises(TypeError, match="unknown key"):
        ops.render_frames(sizes, [{"base": "black", "colour": 1}])
    with pytest.raises(TypeError):
        ops.render_frames(sizes.long(), ["black"])
    for panels in ([], ["black"] * 9, {"base": "black"}, ["sky"], [("depth", 4)], [{"base": "black", "range": (5, 5)}], [{"base": "black", "tint_alpha": 300}],
                   [{"base": "black", "lines": "colour"}], [{"base": "black", "lines": (1, 2, 256)}], [{"base": "black", "void": (1, 2)}],
                   [{"base": "black", "table": np.zeros((255, 3), np.uint8)}], [{"base": "black", "table": np.zeros((256, 3), np.int32)}]):
        with pytest.raises(ValueError):
            ops.render_frames(sizes, panels)
    for panels, kw in (([("depth", 1)], dict(planes=[mm])), (["frame"], {}), ([("labels", 0)], {}), ([{"base": "black", "tint": 0}], {}),
                       ([{"base": "black", "outlines": True}], {}), ([{"base": "black", "lines": "score"}], {}),
                       ([{"base": "black", "lines": "score"}], dict(lines=lines, count=count)), ([{"base": "black", "lines": "kind"}], dict(lines=lines, count=count)),
                       ([{"base": "black", "ends": True}], {})):
        with pytest.raises(ValueError):
            ops.render_frames(sizes, panels, **kw)
    with pytest.raises(TypeError):                                                      # a float plane is no millimetre plane
        ops.render_frames(sizes, [("depth", 0)], planes=[mm.float()])
    with pytest.raises(ValueError):
        ops.render_frames(sizes, [("depth", 0)], planes=[mm[:2]])
    with pytest.raises(ValueError):                                                     # a column stride
        ops.render_frames(sizes, [("labels", 0)], label_planes=[labels[:, :, ::2]])
    with pytest.raises(ValueError):
        ops.render_frames(sizes, [{"base": "black", "lines": (1, 2, 3)}], lines=lines, count=count[:2])
    with pytest.raises(ValueError):
        ops.render_frames(sizes, [{"base": "black", "lines": (1, 2, 3)}], lines=lines[..., :3], count=count)
    with pytest.raises(TypeError):
        ops.render_frames(sizes, [{"base": "black", "lines": (1, 2, 3)}], lines=lines.half(), count=count)
    with pytest.raises(ValueError):
        ops.render_frames(sizes, ["black"], canvas_size=(4, 4), count=count)
    assert fake.render_calls == []
    # what is allowed: a canvas of one's own size, equal tables stored once, a frame clipped to what its operands cover
    out = ops.render_frames(sizes, [("depth", 0), {"base": ("labels", 0), "table": R.jet_table()}, "black"], planes=mm, label_planes=labels, canvas_size=(70, 90))
    assert tuple(out.shape) == (3, 3, 70, 90, 3) and fake.render_calls[-1]["tables"] == 1 and not out[:, :, 64:].any() and not out[:, :, :, 80:].any()
    with pytest.raises(ValueError, match="out must be"):
        ops.render_frames(sizes, ["black"], canvas_size=(4, 4), out=torch.zeros(3, 1, 4, 5, 3, dtype=torch.uint8))
    mine = torch.full((3, 1, 4, 4, 3), 7, dtype=torch.uint8)
    assert ops.render_frames(sizes, ["black"], canvas_size=(4, 4), out=mine) is mine and not mine.any()
    small = ops.render_frames(sizes, [("labels", 0)], label_planes=[labels[:, :20, :30]])
    assert tuple(small.shape) == (3, 1, 20, 30, 3) and np.array_equal(small[1, 0].numpy(), R.voc_palette()[case["label_planes"][0][1, :20, :30]])


def test_default_session_issues_todays_launches_and_keys(fake):
    sess = InferenceSession(TinyModel(), compute_dtype=torch.float32, graph=False)
    assert sess.render is None
    res = sess.predict_frames(frames_of(3), size=48, max_size=64)
    assert fake.calls == dict(BUDGET, gather2d_batch=0) and fake.render_calls == [] and fake.region_calls == [] and fake.profile_calls == []
    assert sorted(res) == sorted(RESULT_KEYS + ("net_sizes",))
    hip.set_library(FramesFakeDevice())                                                 # the stand-in without the new call: not needed
    old = InferenceSession(TinyModel(), compute_dtype=torch.float32, graph=False, render=None).predict_frames(frames_of(3), size=48, max_size=64)
    for k in res:
        assert torch.equal(res[k], old[k]), k


def session_canvas(res, frames, panels, nms, fused=False, **options):
    """ops.render_frames' statement on the session's own outputs."""
    B = len(frames)
    case = dict(sizes=res["sizes"].numpy(), panels=panels, frames=[f.numpy() for f in frames],
                planes=[res["depth_fused_mm" if fused else "depth_mm"].numpy()], label_planes=[res["labels"].numpy()],
                region_map=res["region_map"].numpy() if "region_map" in res else None,
                lines=res["nms_lines" if nms else "lines"].numpy(), count=res["nms_count" if nms else "count"].numpy(),
                order=None if nms else res["order"].numpy(), scores=res["nms_scores" if nms else "scores"].numpy(),
                kinds=res["profile_kind"].numpy() if "profile_kind" in res else None,
                options=dict({"canvas_size": tuple(res["labels"].shape[1:])}, **options))
    return K.statement(case)


@pytest.mark.parametrize("ensemble", [False, True], ids=["plain", "ensemble"])
def test_session_renders_its_own_results_behind_everything_else(fake, ensemble):
    sess = InferenceSession(TinyModel(), compute_dtype=torch.float32, graph=False, render=True, score_thresh=0.45)
    frames = frames_of(3)
    res = sess.predict_frames(frames, size=48, max_size=64, ensemble=ensemble)
    assert fake.calls == dict(BUDGET, gather2d_batch=0)                                 # the launches before it are the same
    assert sorted(res) == sorted(RESULT_KEYS + ("net_sizes",) + RENDER_KEYS)
    Fh, Fw = res["labels"].shape[1:]
    assert len(fake.render_calls) == 1
    rec = fake.render_calls[0]
    assert rec["shape"] == (3, 3, Fh, Fw, 3) and rec["frames"] and rec["planes"] == 1 and rec["label_planes"] == 1 and not rec["region_map"]
    assert rec["rows"] == (3, TinyModel.Q) and rec["dtype"] == torch.float32 and rec["order"] and rec["scores"] and not rec["kinds"]
    assert [p["base"] for p in rec["panels"]] == [R.FRAME, R.DEPTH, R.LABELS] and [p["lines"] for p in rec["panels"]] == [R.LINES_SCORE, 0, 0]
    assert rec["panels"][0]["tint"] == 0 and rec["panels"][0]["outlines"] == 0 and rec["opts"]["width8"] == 16
    panels = [{"base": "frame", "tint": 0, "lines": "score"}, ("depth", 0), ("labels", 0)]
    want = session_canvas(res, frames, panels, nms=False)
    assert np.array_equal(res["canvas"].numpy(), want)
    assert 0 < int(res["count"].min()) and (want[:, 0] != want[:, 0, :1, :1]).any()
    plain = InferenceSession(TinyModel(), compute_dtype=torch.float32, graph=False, score_thresh=0.45).predict_frames(frames, size=48, max_size=64, ensemble=ensemble)
    assert sorted(plain) == sorted(set(res) - set(RENDER_KEYS))
    for k in plain:
        assert torch.equal(plain[k], res[k]), k


def test_session_with_nms_regions_profiles_and_fusion_draws_them(fake):
    sess = InferenceSession(TinyModel(), compute_dtype=torch.float32, graph=False, line_nms=0.01, regions={"min_area": 4, "max_regions": 8},
                            line_profiles=True, fusion=True, render={"width": 1.0, "end_radius": 0, "score_range": (0.0, 1.0)})
    frames = frames_of(3)
    sensor = [torch.full(tuple(f.shape[:2]), 1500, dtype=torch.uint16) for f in frames]
    res = sess.predict_frames(frames, size=48, max_size=64, sensor_depth=sensor)
    assert sorted(res) == sorted(RESULT_KEYS + ("net_sizes",) + NMS_KEYS + REGION_KEYS + PROFILE_KEYS[:3] + FUSION_KEYS + RENDER_KEYS)
    rec = fake.render_calls[-1]
    assert rec["after"] == (len(fake.region_calls), len(fake.profile_calls), len(fake.fusion_calls)) and rec["after"][2] == 3      # behind all of them
    assert rec["region_map"] and rec["kinds"] and not rec["order"] and rec["dtype"] == torch.float64 and rec["rows"] == (3, TinyModel.Q)
    assert rec["panels"][0]["lines"] == R.LINES_KIND and rec["panels"][0]["outlines"] == 1 and rec["opts"]["width8"] == 8 and rec["opts"]["end_radius"] == 0
    panels = [{"base": "frame", "tint": 0, "outlines": True, "lines": "kind"}, ("depth", 0), ("labels", 0)]
    want = session_canvas(res, frames, panels, nms=True, fused=True, width=1.0, end_radius=0, score_range=(0.0, 1.0))
    assert np.array_equal(res["canvas"].numpy(), want)
    no_sensor = sess.predict_frames(frames, size=48, max_size=64)                       # the call did not fuse: the depth panel shows depth_mm
    assert np.array_equal(no_sensor["canvas"].numpy(), session_canvas(no_sensor, frames, panels, nms=True, width=1.0, end_radius=0, score_range=(0.0, 1.0)))
    # panels of one's own, planes by name
    own = InferenceSession(TinyModel(), compute_dtype=torch.float32, graph=False, regions={"min_area": 4, "max_regions": 8},
                           render={"panels": [("labels", "region_map"), {"base": ("depth", "depth_planar_mm"), "tint": "labels"}, "black"]})
    out = own.predict_frames(frames, size=48, max_size=64)
    rec = fake.render_calls[-1]
    assert rec["planes"] == 1 and rec["label_planes"] == 2 and [p["base"] for p in rec["panels"]] == [R.LABELS, R.DEPTH, R.BLACK]
    assert np.array_equal(out["canvas"][:, 0].numpy(), R.voc_palette()[out["region_map"].numpy()] * (out["labels"].numpy() != 255)[..., None])
    assert not out["canvas"][:, 2].any()


def test_session_options_are_validated():
    mk = lambda **kw: InferenceSession(TinyModel(), compute_dtype=torch.float32, graph=False, **kw)
    for bad, exc in ((False, TypeError), (3, TypeError), ({"colour": 3}, TypeError), ({"width": 0}, ValueError), ({"end_radius": 100}, ValueError),
                     ({"panels": []}, ValueError), ({"panels": [{"base": "frame", "shade": 1}]}, TypeError), ({"panels": [("depth", "depth_fused_mm")]}, ValueError),
                     ({"panels": [("depth", "depth_planar_mm")]}, ValueError), ({"panels": [("labels", "region_map")]}, ValueError),
                     ({"panels": [{"base": "frame", "tint": "fused_source"}]}, ValueError), ({"panels": [{"base": "frame", "outlines": True}]}, ValueError),
                     ({"panels": [{"base": "frame", "lines": "kind"}]}, ValueError), ({"panels": [("depth", 0)]}, ValueError),
                     ({"canvas_size": (4, 4)}, TypeError)):
        with pytest.raises(exc):
            mk(render=bad)
    with pytest.raises(ValueError):
        mk(regions={"planar": False, "planes": False}, render={"panels": [("depth", "depth_planar_mm")]})
    assert mk(regions=True, render={"panels": [("depth", "depth_planar_mm"), ("labels", "region_map")]}).render["options"] == {}


# ------------------------------------------------------------------------------------------------------------------ saving
@pytest.mark.parametrize("layout", ["row", "files"])
def test_save_panels_round_trips_through_pillow(tmp_path, layout):
    Image = pytest.importorskip("PIL.Image")
    canvas = torch.from_numpy(GOLD["ragged.canvas"])
    sizes = torch.from_numpy(CASES["ragged"]["sizes"][:2])
    paths = [str(tmp_path / ("frame%d.png" % b)) for b in range(2)]
    written = R.save_panels(canvas[:2], sizes, paths, layout=layout, suffixes=["", "_depth", "_seg"])
    if layout == "row":
        assert written == paths
        for b, (fh, fw) in enumerate(sizes.tolist()):
            got = np.asarray(Image.open(paths[b]).convert("RGB"))
            assert got.shape == (fh, 3 * fw, 3) and np.array_equal(got, np.concatenate(list(canvas[b, :, :fh, :fw].numpy()), axis=1))
    else:
        assert written == [str(tmp_path / ("frame%d%s.png" % (b, s))) for b in range(2) for s in ("", "_depth", "_seg")]
        for k, path in enumerate(written):
            fh, fw = sizes[k // 3].tolist()
            assert np.array_equal(np.asarray(Image.open(path).convert("RGB")), canvas[k // 3, k % 3, :fh, :fw].numpy())
    with pytest.raises(ValueError):
        R.save_panels(canvas[:2], sizes, paths[:1])
    with pytest.raises(ValueError):
        R.save_panels(canvas[:2], sizes, paths, layout="grid")
    with pytest.raises(ValueError):
        R.save_panels(canvas[:2], sizes, paths, layout="files", suffixes=["a"])


class StubSession:
    """What evaluate_frames(save_dir=) needs of a session, with canned results."""
    min_depth, max_depth, line_nms = 1e-3, 10.0, None

    def __init__(self, case):
        self.case, self.calls = case, 0

    def _device(self):
        return torch.device("cpu")

    @staticmethod
    def _upload_frame(frame, device):
        return frame

    def predict_frames(self, rgb, **kw):
        self.calls += 1
        c = self.case
        T = lambda v: torch.from_numpy(np.ascontiguousarray(v))
        return dict(sizes=T(c["sizes"][:2]), labels=T(c["label_planes"][0][:2]), depth_mm=T(c["planes"][0][:2]), lines=T(c["lines"][:2]),
                    count=T(c["count"][:2]), order=T(c["order"][:2]), scores=T(c["scores"][:2]))


class StubMetrics:
    def __init__(self):
        self.seen = []

    def update(self, res, gt, ids=None):
        self.seen.append((sorted(res), ids))

    def compute(self):
        return {"n": len(self.seen)}


class StubSource:
    def __init__(self, case):
        self.case = case

    def __len__(self):
        return 2

    def frames(self, idx):
        c = self.case
        return [(torch.from_numpy(c["frames"][i]), torch.from_numpy(c["planes"][0][i, :c["sizes"][i][0], :c["sizes"][i][1]].astype(np.int32)) + 100,
                 torch.from_numpy(np.ascontiguousarray(c["region_map"][i, :c["sizes"][i][0], :c["sizes"][i][1]]))) for i in idx]

    def name(self, i):
        return "scene/img%d" % i


def test_evaluate_frames_saves_six_panels_per_sample_and_scores_the_same(fake, tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from gw_depth_amd.evaluate import SAVE_SUFFIXES, evaluate_frames
    case = CASES["ragged"]
    plain, saved = StubMetrics(), StubMetrics()
    a = evaluate_frames(StubSession(case), StubSource(case), batch=2, metrics=plain)
    assert fake.render_calls == []
    b = evaluate_frames(StubSession(case), StubSource(case), batch=2, metrics=saved, save_dir=str(tmp_path / "vis"))
    assert a == b and plain.seen == saved.seen and len(fake.render_calls) == 1 and fake.render_calls[0]["shape"] == (2, 6, 64, 80, 3)
    assert sorted(os.listdir(tmp_path / "vis")) == sorted("scene_img%d%s.png" % (i, s) for i in range(2) for s in SAVE_SUFFIXES)
    assert SAVE_SUFFIXES == ("", "_depth", "_seg", "_gt-depth", "_gt-seg", "_lines")
    jet, pal = R.jet_table(), R.voc_palette()
    for i, (fh, fw) in enumerate(case["sizes"][:2].tolist()):
        read = lambda s: np.asarray(Image.open(tmp_path / "vis" / ("scene_img%d%s.png" % (i, s))).convert("RGB"))
        mm = case["planes"][0][i, :fh, :fw].astype(np.int64)
        assert np.array_equal(read(""), case["frames"][i])
        assert np.array_equal(read("_depth"), np.where((mm == 0)[..., None], 0, jet[P.depth_index(mm, 0, 8500)]))
        assert np.array_equal(read("_seg"), pal[case["label_planes"][0][i, :fh, :fw]])
        assert np.array_equal(read("_gt-depth"), jet[P.depth_index(mm + 100, 0, 8500)])
        assert np.array_equal(read("_gt-seg"), pal[case["region_map"][i, :fh, :fw]])
        lines = read("_lines")
        assert lines.shape == (fh, fw, 3) and (lines != case["frames"][i]).any()
