"""CPU: the case lists of the batched GEMM (tests/bmm_ref.py), the matcher's cost block (tests/matchcost_ref.py) and the plane loss
(tests/plane_loss_ref.py) reach the launch edges they name - shown from the launch arithmetic of csrc/bmm.hip, csrc/setloss.hip and
csrc/planeloss.hip, restated there -, the clean fp32 models pass every case within C, the constants are the measured ones, every
injected defect is caught on at least one case, and the min_area cases have the areas they claim.
tests/test_gemm_criterion_witnesses_gpu.py applies the same instrument to the kernels."""
import pytest
import torch

from tests import bmm_ref as BR
from tests import matchcost_ref as MR
from tests import plane_loss_ref as PR


def _constants_hold(R, got):
    assert set(got) == set(R.C) == set(R.MEASURED)
    for key, worst in sorted(got.items()):
        print("%s %s %s: model maximum %.3f, table %.3f, C %.1f" % (key + (worst, R.MEASURED[key], R.C[key])))
        assert worst <= R.C[key] <= 2 * worst + 0.1 + 1e-9, (key, worst)
        assert abs(worst - R.MEASURED[key]) <= 0.02, "%s's table is out of date: %s measured %.3f" % (R.__name__, key, worst)
    assert R.format_table(R.MEASURED) in R.__doc__


# ========================================================================================================== batched GEMM
@pytest.fixture(scope="module")
def bmm_table():
    out = []
    for c in BR.cases():
        inp = BR.inputs(c)
        out.append((c, inp) + BR.reference(c, inp))
    return out


def test_bmm_cases_reach_every_layout_tail_and_split(bmm_table):
    cs = [t[0] for t in bmm_table]
    assert len({c.text for c in cs}) == len(cs)
    for dt in ("f32", "bf16"):
        mine = [c for c in cs if c.dtype == dt]
        v, bk = BR.VEC[dt], BR.BK[dt]
        assert (v, bk) == {"f32": (4, 16), "bf16": (8, 32)}[dt] and v * {"f32": 4, "bf16": 2}[dt] == 16
        every = [c for c in mine if (c.M, c.N, c.K, c.kind, c.accumulate) == (65, 33, bk + 1, "plain", False)]
        assert {(c.akm, c.bkm) for c in every} == {(False, False), (False, True), (True, False), (True, True)}
        for c in every:                                         # 2 x 1 tiles; the second tile row and the second wave column hold one line each
            assert BR.launch(c).grid_x == 2 and c.M - BR.TILE == 1 and c.N - 32 == 1 and c.alpha == 0.37
            assert (c.K + bk - 1) // bk == 2 and c.K % bk == 1
        for km in (False, True):
            tails = sorted(c.K for c in mine if (c.M, c.N, c.akm, c.bkm, c.kind) == (33, 17, km, km, "plain"))
            assert tails == sorted({1, 3, v - 1, v, bk - 1, bk, 2 * bk + 1})
        assert any(c.K < v for c in mine) and any(c.K % bk for c in mine)
        # split-K: grid.z >= 3 with a ragged last slice; splits > 1 on a broadcast operand; an added-to result with splits = 1
        split = next(c for c in mine if c.splits == 3)
        L = BR.launch(split)
        assert (split.M, split.N, split.akm, split.bkm, split.accumulate) == (80, 64, True, True, True)
        assert L.kps == bk and split.K == 2 * L.kps + 5 and L.grid_z == 3 and L.last == 5 and L.grid_x == 2
        bc = next(c for c in mine if c.splits == 2)
        assert bc.kind == "a_bcast0" and BR.launch(bc).grid_z == 2 and 0 < BR.launch(bc).last < bk and BR.launch(bc).grid_y == 4
        acc = next(c for c in mine if c.kind == "acc")
        assert acc.splits == 1 and acc.accumulate and BR.launch(acc).grid_z == 1
        assert all(BR.launch(c).grid_z == 1 for c in mine if not c.accumulate)
        assert {c.kind for c in mine} == {"plain", "unaligned", "aligned", "heads_qk", "heads_pv", "a_bcast0", "b_bcast", "acc"}
    assert max(t[2].numel() for t in bmm_table) <= 80 * 64 * 4


def test_bmm_operand_views_are_what_the_cases_claim(bmm_table):
    by = {c.text: (c, inp, ref, cond) for c, inp, ref, cond in bmm_table}
    for c, inp, ref, cond in bmm_table:
        fast, slow = BR.load_branches(c, inp)
        v = BR.VEC[c.dtype]
        for op in (inp["a"], inp["b"]):
            assert op.stride[3] == 1 and not bool(torch.isnan(op.view.float()).any())
        if c.kind == "unaligned":
            ld = {"f32": 30, "bf16": 27}[c.dtype]
            # fp32: 1 + 30 r + 4 j is odd, no vector is 16-byte aligned; bf16: 1 + 27 r + 8 j is a multiple of 8 in one row of eight ...
            assert slow > 4 * fast and (fast == 0 or c.dtype == "bf16")
            for op, km in ((inp["a"], c.akm), (inp["b"], c.bkm)):
                assert op.offset == 1 and op.stride[2] == ld and op.size[3] == ld - 1 and (ld * (4 if c.dtype == "f32" else 2)) % 16
                if km:
                    assert op.size[3] % v != 0                   # R % VEC != 0
        if c.kind == "aligned":
            assert fast > 0 and slow > 0                        # ... the twin takes both branches of load_vec
            twin = by[c.text.replace(" aligned ", " unaligned ")]
            assert torch.equal(twin[2], ref) and torch.equal(twin[3][1], cond[1])          # one reference for both branches
        if c.kind.startswith("heads"):
            assert (c.nb0, c.nb1) == (3, 5)
            for op in (inp["a"], inp["b"]):
                if op.size[1] == 5 and op.base.numel() > op.view.numel():
                    assert not op.view.is_contiguous() and op.stride[1] == op.size[3] and op.stride[2] == 2 * 5 * op.size[3]
        if c.kind == "a_bcast0":
            assert inp["a"].size[0] == 1 and inp["b"].size[0] == c.nb0 > 1
        if c.kind == "b_bcast":
            assert inp["b"].size[:2] == (1, 1) and c.nb0 * c.nb1 == 15
        if c.kind == "acc":
            assert float(inp["c0"].abs().min()) > 0 and bool((cond[1] >= inp["c0"].double().abs()).all())
    assert any(c.kind == "heads_qk" and c.K < BR.VEC[c.dtype] for c, _, _, _ in bmm_table)


def test_bmm_rejected_descriptors_stop_at_the_guards():
    """The guard order of gwd_bmm: dtype, sizes, batch / splits limits, splits without accumulate - all before the launch."""
    base = dict(M=8, N=8, K=8, nb0=1, nb1=1, splits=1, dtype=0, accumulate=0)
    for name, over, rc in BR.rejected():
        d = dict(base, **over)
        if d["dtype"] not in (0, 1):
            want = -2
        elif min(d["M"], d["N"], d["K"], d["nb0"], d["nb1"], d["splits"]) <= 0:
            want = -3
        elif d["nb0"] * d["nb1"] > BR.MAX_BATCH or d["splits"] > BR.MAX_SPLITS:
            want = -7
        elif d["splits"] > 1 and not d["accumulate"]:
            want = -4
        else:
            want = 0
        assert want == rc, name
    assert sorted(rc for _, _, rc in BR.rejected()) == [-7, -4, -3, -3, -2]


def test_bmm_clean_model_passes_and_constants_are_the_measured_ones(bmm_table):
    _constants_hold(BR, BR.measure_c([t[0] for t in bmm_table]))
    for c, inp, ref, cond in bmm_table:
        BR.check(c, BR.model(c, inp), inp, ref, cond)


@pytest.mark.parametrize("defect", BR.DEFECTS)
def test_bmm_defect_is_caught(bmm_table, defect):
    caught = []
    for c, inp, ref, cond in bmm_table:
        try:
            BR.check(c, BR.model(c, inp, defect), inp, ref, cond)
        except AssertionError:
            caught.append(c)
    print("%s: caught on %d cases" % (defect, len(caught)))
    assert caught and {c.dtype for c in caught} == {"f32", "bf16"}
    if defect == "k_tail_dropped":
        assert all(c.K % BR.BK[c.dtype] for c in caught)
    if defect == "edge_row":
        assert all(c.M % BR.TILE for c in caught)
    if defect == "kmajor_swapped":
        assert all(c.akm or c.bkm for c in caught) and any(c.K == 2 * BR.BK[c.dtype] + 1 for c in caught)
    if defect == "split_lost":
        assert {c.splits for c in caught} == {2, 3}
    if defect == "unaligned_zero":
        assert {"unaligned", "aligned"} <= {c.kind for c in caught}


# ============================================================================================================ match cost
@pytest.fixture(scope="module")
def cost_table():
    out = []
    for c in MR.cases():
        inp = MR.inputs(c)
        out.append((c, inp) + MR.reference(c, inp))
    return out


def test_match_cost_cases_reach_the_limits_and_the_stride_tail(cost_table):
    cs = [t[0] for t in cost_table]
    assert len({c.text for c in cs}) == len(cs)
    assert {(c.K, c.D) for c in cs} >= {(K, D) for K in (1, 2, 8) for D in (1, 6, 8)} and (MR.KMAX, MR.DMAX) == (8, 8)
    L = {c.text: MR.launch(c) for c in cs}
    assert {1, 255, 257} <= {l.total for l in L.values()}
    assert {l.blocks for l in L.values() if l.total in (1, 255, 257)} == {1, 2}
    big = [c for c in cs if L[c.text].tail]
    assert len(big) == 1 and eval("total > 2048 * 256", {"total": L[big[0].text].total})
    l = L[big[0].text]
    assert (l.total, l.blocks, l.trips) == (MR.MAX_BLOCKS * MR.THREADS + 1, MR.MAX_BLOCKS, 2) and (big[0].Q, big[0].cap) == (3, 174763)
    assert all(l.trips == 1 for t, l in L.items() if t != big[0].text)
    for c, inp, ref, cond in cost_table:
        lab = inp["labels"]
        if c.labels == "range":
            assert int(lab.min()) == 0 and int(lab.max()) == min(c.K, c.cap) - 1         # every class, K - 1 included
        else:
            assert lab[-4:].tolist() == [-1, c.K, -5, c.K + 7] and 0 <= int(lab[:-4].min()) and int(lab[:-4].max()) == c.K - 1
    assert {c.K for c in cs if c.labels == "oob"} == {2, 8}
    assert any(c.w_class == 0 and c.w_line != 0 for c in cs) and any(c.w_line == 0 and c.w_class != 0 and c.logits == "rand" for c in cs)


def test_match_cost_hard_rows_are_what_they_claim(cost_table):
    for c, inp, ref, cond in cost_table:
        if c.logits != "hard":
            continue
        rows = inp["logits"].view(-1, 2)
        assert rows.shape[0] >= 10
        assert [tuple(r) for r in rows[:4].tolist()] == [(30.0, -30.0), (-60.0, 60.0), (100.0, -100.0), (1.5, 1.5)]
        p = torch.softmax(rows.double(), dim=-1)
        assert 0 < float(p[0, 1]) < 1e-25 and float(p[0, 0]) == 1.0                       # saturated
        assert 0 < float(p[2, 1]) < 2.0 ** -149                                           # below fp32's smallest subnormal
        assert float(p[3, 0]) == 0.5
        assert {0, 1} <= set(inp["labels"].tolist())                                      # both columns of every row are targets
        assert not bool(torch.isfinite(torch.exp(rows[2])).all())                          # exp of the raw logit overflows


def test_match_cost_clean_model_passes_and_constants_are_the_measured_ones(cost_table):
    _constants_hold(MR, MR.measure_c([t[0] for t in cost_table]))
    for c, inp, ref, cond in cost_table:
        MR.check(c, MR.model(c, inp), inp, ref, cond)


@pytest.mark.parametrize("defect", MR.DEFECTS)
def test_match_cost_defect_is_caught(cost_table, defect):
    caught = []
    for c, inp, ref, cond in cost_table:
        try:
            MR.check(c, MR.model(c, inp, defect), inp, ref, cond)
        except AssertionError:
            caught.append(c)
    print("%s: caught on %d cases" % (defect, len(caught)))
    assert caught
    if defect == "label_unclamped_wraps":
        assert {c.labels for c in caught} == {"oob"} and len(caught) == 2
    if defect == "stride_tail_skipped":
        assert [MR.launch(c).tail for c in caught] == [True]
    if defect == "softmax_no_max":
        assert {c.logits for c in caught} == {"hard"}
    if defect == "d_last_dropped":
        assert {c.D for c in caught} == {1, 6, 8}


def test_match_cost_rejected_shapes_are_the_documented_ones():
    for name, (L, B, Q, cap, K, D), rc in MR.rejected():
        want = -1 if min(L, B, Q, cap) <= 0 else (-4 if not (0 < K <= MR.KMAX and 0 < D <= MR.DMAX) else 0)
        assert want == rc, name
    assert [rc for _, _, rc in MR.rejected()] == [-4, -4, -1]


# ============================================================================================================ plane loss
@pytest.fixture(scope="module")
def plane_table():
    out = []
    for c in PR.cases():
        inp = PR.inputs(c)
        masks = PR.masks_of(c, inp)
        out.append((c, inp, masks) + PR.reference(c, inp, masks))
    return out


def _kind(plane_table, kind, dtype="f32", valid=None):
    return next(t for t in plane_table if t[0].kind == kind and t[0].dtype == dtype and (valid is None or t[0].valid == valid))


def test_plane_cases_reach_both_grid_stride_loops_and_the_caps(plane_table):
    cs = [t[0] for t in plane_table]
    assert len({c.text for c in cs}) == len(cs)
    L = {c.text: PR.launch(c) for c in cs}
    large = [c for c in cs if L[c.text].tail]
    assert len(large) == 1 and eval("H * W > 2048 * 256", {"H": large[0].H, "W": large[0].W})
    c = large[0]
    l = L[c.text]
    assert (c.H, c.W, c.P, c.dtype) == (513, 1023, 3, "f32")
    assert (l.fwd_blocks, l.bwd_blocks) == (PR.FWD_MAX_BLOCKS, PR.BWD_MAX_BLOCKS) == (128, 2048)       # both caps
    assert l.fwd_trips == 17 and l.bwd_trips == 2 and l.HW - PR.BWD_MAX_BLOCKS * PR.THREADS == 511
    assert all(L[t.text].bwd_trips == 1 for t in cs if t is not c)
    assert {L[t.text].fwd_blocks for t in cs} >= {1, 3, 128} and PR.launch(_kind(plane_table, "random")[0]).fwd_trips == 3
    for dt in ("f32", "bf16"):
        mine = [t for t in cs if t.dtype == dt]
        assert {(t.H, t.W) for t in mine if t.kind == "tiny"} == {(1, 1), (1, 9), (9, 1), (3, 3)}
        assert {t.kind for t in mine} >= {"tiny", "corners", "degenerate", "overlap", "none_counted", "beyond", "random", "invalid"}
        assert any(t.P == PR.PMAX == 64 for t in mine) and any(t.gloss == 3.0 for t in mine)
        assert {t.valid for t in mine} == {"all", "holes", "none"}
    # the gradient of the large map's second trip is not trivially zero
    c, inp, masks, ref, conds = _kind(plane_table, "large")
    tail = ref["gdepth"].view(-1)[PR.BWD_MAX_BLOCKS * PR.THREADS:]
    assert tail.numel() == 511 and int((tail != 0).sum()) > 100


def test_plane_cases_are_what_they_claim(plane_table):
    for dt in ("f32", "bf16"):
        c, inp, masks, ref, conds = _kind(plane_table, "corners", dt, "all")
        corners = {(0, 0), (c.W - 1, 0), (0, c.H - 1)}
        assert {tuple(v) for v in inp["tri"][0].view(3, 2).tolist()} == corners
        border = torch.ones(c.H, c.W, dtype=torch.bool)
        border[1:-1, 1:-1] = False
        print("%s: %d border pixels inside the corner triangle" % (c.text, int((masks[0] & border).sum())))
        assert int((masks[0] & border).sum()) > 5 and bool(masks[2].all()) and ref["active"].tolist() == [1.0, 1.0, 1.0]
        c, inp, masks, ref, conds = _kind(plane_table, "corners", dt, "holes")
        assert 0 < int(inp["valid"].sum()) < c.H * c.W and int((masks[0] & ~inp["valid"].bool()).sum()) == 0
        assert int(masks[1][-1].sum()) > 5 and int(masks[1][:, -1].sum()) > 5                                # the other two borders
        c, inp, masks, ref, conds = _kind(plane_table, "overlap", dt)
        assert int((masks[0] & masks[1] & masks[2]).sum()) >= 6                                            # a block inside all three
        assert ref["active"].tolist() == [1.0, 1.0, 1.0, 0.0] and int((masks[3] & masks[0]).sum()) == int(masks[3].sum()) > 0
        assert c.gloss == 3.0
        c, inp, masks, ref, conds = _kind(plane_table, "none_counted", dt)
        assert c.n_planes == 0 and float(ref["loss"]) == 0.0 and not bool(ref["gdepth"].any()) and int(masks.sum()) > 300
        c, inp, masks, ref, conds = _kind(plane_table, "beyond", dt)
        assert (c.n_planes, c.P) == (2, 5) and all(int(masks[j].sum()) > 150 for j in (2, 3, 4)) and ref["n"][2:].tolist() == [0.0] * 3
        assert float(ref["count"]) == 2.0
        c, inp, masks, ref, conds = _kind(plane_table, "invalid", dt)
        assert int(inp["valid"].sum()) == 0 and float(ref["count"]) == 0.0 and not bool(ref["gdepth"].any())
        c, inp, masks, ref, conds = _kind(plane_table, "random", dt)
        assert 0 < float(ref["count"]) < 64 and int((masks.sum(0) >= 3).sum()) > 0
        for c, inp, masks, ref, conds in (t for t in plane_table if t[0].kind == "tiny" and t[0].dtype == dt):
            assert int(masks[0].sum()) == c.H * c.W and ref["active"][0] == 1.0


def test_plane_min_area_cases_have_the_areas_they_claim(plane_table):
    for dt in ("f32", "bf16"):
        c, inp, masks, ref, conds = _kind(plane_table, "degenerate", dt)
        tri = inp["tri"].view(5, 3, 2)
        assert len({tuple(v) for v in tri[0].tolist()}) == 1                                               # three equal vertices
        (x0, y0), (x1, y1), (x2, y2) = tri[1].tolist()
        assert (x1 - x0) * (y2 - y0) == (x2 - x0) * (y1 - y0) and len({(x0, y0), (x1, y1), (x2, y2)}) == 3  # collinear
        counts = [PR.count_inside(tri[j].tolist(), c.H, c.W) for j in range(5)]
        assert counts == [int(masks[j].sum()) for j in range(5)] == [int(v) for v in ref["n"].tolist()]
        assert counts[0] == 0 and counts[1] < c.min_area and counts[2] == c.min_area and counts[3] == c.min_area - 1
        assert counts[4] > c.min_area >= 12 and int((masks[2] & masks[3]).sum()) == 0
        assert ref["active"].tolist() == [0.0, 0.0, 1.0, 0.0, 1.0] and float(ref["count"]) == 2.0


def test_plane_clean_model_passes_and_constants_are_the_measured_ones(plane_table):
    _constants_hold(PR, PR.measure_c([t[0] for t in plane_table]))
    for c, inp, masks, ref, conds in plane_table:
        PR.check(c, PR.model(c, inp, masks=masks), inp, ref, conds)


def test_plane_inputs_make_a_wrong_pixel_visible(plane_table):
    """The normal of the neighbouring pixel changes the means by far more than the bound."""
    c, inp, masks, ref, conds = _kind(plane_table, "overlap")
    moved = dict(inp, depth=torch.roll(inp["depth"], 1, dims=1))
    other, _ = PR.reference(c, moved, masks)
    r = PR.ratio(other["mean_x"], ref["mean_x"], conds["mean_x"], PR.U_F32)
    assert float(r[:3].min()) > 100 * PR.C[PR.key_of(c, "mean_x")]


@pytest.mark.parametrize("defect", PR.DEFECTS)
def test_plane_defect_is_caught(plane_table, defect):
    caught = []
    for c, inp, masks, ref, conds in plane_table:
        try:
            PR.check(c, PR.model(c, inp, defect, masks=masks), inp, ref, conds)
        except AssertionError:
            caught.append(c)
    print("%s: caught on %d cases" % (defect, len(caught)))
    assert caught
    kinds = {c.kind for c in caught}
    if defect == "border_clamped":
        assert "corners" in kinds and {c.dtype for c in caught} == {"f32", "bf16"}
    if defect == "bwd_untransposed":
        assert {c.dtype for c in caught} == {"f32", "bf16"}
    if defect == "inactive_counts":
        assert "overlap" in kinds
    if defect == "beyond_count":
        assert kinds == {"beyond", "none_counted"}
    if defect == "area_off_by_one":
        assert "degenerate" in kinds
    if defect == "stride_once":
        assert kinds == {"large"}


def test_plane_rejected_arguments_are_the_documented_ones():
    for name, P, H, W, code, rc in PR.rejected():
        if P <= 0 or P > PR.PMAX or H <= 0 or W <= 0:
            want = -1
        elif H * W >= 2 ** 31 or H > 32768 or W > 32768:
            want = -7
        elif code not in (0, 1):
            want = -2
        else:
            want = 0
        assert want == rc, name
