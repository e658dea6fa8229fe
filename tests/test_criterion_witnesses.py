"""CPU: the case lists of the set losses (tests/setloss_ref.py), the device LSAP (tests/lsap_ref.py) and the sine position embedding
(tests/posenc_ref.py) reach the edges they name - shown from the launch arithmetic of csrc/setloss.hip, csrc/lsap.hip and
csrc/posenc.hip, restated there -, the clean fp32 models pass every case within C, the constants are the measured ones, every injected
defect is caught on at least one case, and the sequential LSAP reference equals the kernel's own source compiled for the CPU
(tests/lsap_host.cpp) and scipy.  tests/test_criterion_witnesses_gpu.py applies the same instruments to the kernels."""
import math

import numpy as np
import pytest
import torch

from tests import lsap_build
from tests import lsap_ref as LR
from tests import posenc_ref as PR
from tests import setloss_ref as SR


def _constants_hold(R, got):
    assert set(got) == set(R.C) == set(R.MEASURED)
    for key, worst in sorted(got.items()):
        print("%s %s %s: model maximum %.3f, table %.3f, C %.1f" % (key + (worst, R.MEASURED[key], R.C[key])))
        assert worst <= R.C[key] <= 2 * worst + 0.1 + 1e-9, (key, worst)
        assert abs(worst - R.MEASURED[key]) <= 0.02, "%s's table is out of date: %s measured %.3f" % (R.__name__, key, worst)
    assert R.format_table(R.MEASURED) in R.__doc__


def _caught(R, table, defect):
    out = []
    for row in table:
        c, inp = row[0], row[1]
        try:
            R.check(c, R.model(c, inp, defect), inp, *row[2:])
        except AssertionError:
            out.append(c)
    print("%s: caught on %d cases" % (defect, len(out)))
    return out


# ============================================================================================================ set losses
@pytest.fixture(scope="module")
def loss_table():
    out = []
    for c in SR.cases():
        inp = SR.inputs(c)
        out.append((c, inp) + SR.reference(c, inp))
    return out


def _column_kinds(c, inp):
    """The kinds of the columns as the kernel's two guards see them, per layer."""
    v, q = inp["valid"].bool()[None], inp["qot"]
    inq = (q >= 0) & (q < c.Q)
    return {"matched": int((v & inq).sum()), "surplus": int((v & (q == c.Q)).sum()), "padding": int((~v & (q == c.Q)).sum()),
            "free": int((~v & inq).sum()), "negative": int((v & (q == -1)).sum())}


def test_set_loss_cases_reach_both_stride_loops_and_every_limit(loss_table):
    cs = [t[0] for t in loss_table]
    assert len({c.text for c in cs}) == len(cs) and all(c.L == 2 for c in cs)
    L = {c.text: SR.launch(c) for c in cs}
    for focal in (False, True):
        mine = [c for c in cs if L[c.text].focal == focal]
        assert {1, 7, 255, 256, 257, 513} <= {L[c.text].BQ for c in mine}
        assert {L[c.text].bq_trips for c in mine if L[c.text].BQ in (255, 256)} == {1}
        assert {L[c.text].bq_trips for c in mine if L[c.text].BQ == 257} == {2} and {L[c.text].bq_trips for c in mine if L[c.text].BQ == 513} == {3}
        assert 513 % SR.THREADS == 1 and {L[c.text].idle for c in mine} >= {255, 249, 1, 0}         # idle threads of the tree reduction add zero
        assert {1, 64, 256, 257, 300} <= {c.cap for c in mine}
        assert {L[c.text].cap_trips for c in mine if c.cap == 256} == {1} and {L[c.text].cap_trips for c in mine if c.cap in (257, 300)} == {2}
        assert {c.table for c in mine if c.cap >= 256} == {"full", "kinds"}
        assert {(c.K, c.D) for c in mine} >= {(K, D) for K in (1, 2, 3, 8) for D in (1, 6, 8)} and (SR.KMAX, SR.DMAX) == (8, 8)
        assert {(c.num_items, c.world) for c in mine} >= {(0.0, 1.0), (3.0, 2.0), (4.0, 8.0), (37.0, 1.0)}
    assert [max(n / w, 1.0) for n, w in ((0, 1), (3, 2), (4, 8), (37, 1))] == [1.0, 1.5, 1.0, 37.0]
    assert {c.gamma for c in cs} == set(SR.GAMMAS) and {c.gamma for c in cs if c.logits == "hard2"} == set(SR.GAMMAS)
    assert any(c.gamma is None and not c.gce for c in cs) and any(c.gamma is not None and not c.gce for c in cs)
    assert any(not c.gl1 and not c.c0 for c in cs) and any(not c.gl1 and c.c0 for c in cs) and any(c.c0 and c.gl1 for c in cs)
    assert max(t[2]["dlogits"].numel() + t[2]["dlines"].numel() for t in loss_table) * 4 < 4 << 20


def test_set_loss_tables_hold_the_columns_they_claim(loss_table):
    for c, inp, ref, cond in loss_table:
        kinds = _column_kinds(c, inp)
        valid, labels, qot = inp["valid"].bool(), inp["labels"], inp["qot"]
        assert int(inp["bidx"].min()) >= 0 and int(inp["bidx"].max()) < c.B
        if c.table == "full":
            assert kinds == {"matched": c.L * c.cap, "surplus": 0, "padding": 0, "free": 0, "negative": 0} and c.cap <= c.B * c.Q
        elif c.cap >= 8:
            assert all(v >= c.L for v in kinds.values()), (c.text, kinds)               # every kind in every layer of one case
        # matched and free columns of one image never share a query: the labels and the atomics of dlines hit distinct addresses
        for l in range(c.L):
            inq = (qot[l] >= 0) & (qot[l] < c.Q)
            rows = (inp["bidx"].long() * c.Q + qot[l].long())[inq]
            assert len(set(rows.tolist())) == int(inq.sum())
        lab_valid = labels[valid]
        assert int(lab_valid.min()) == 0 and int(lab_valid.max()) == min(c.K, int(valid.sum())) - 1
        per_layer = _column_kinds(c, inp)["matched"] // c.L
        assert all(int(x) in SR.OOB(c.K) for x in labels[~valid])                        # out of range ONLY where valid = 0
        assert int(ref["target_class"].min()) >= 0 and int(ref["target_class"].max()) <= c.K - 1
        if per_layer >= c.K > 1:
            assert set(ref["target_class"].flatten().tolist()) == set(range(c.K)), c.text
        assert bool((inp["cls_w"][1:] > 0).all()) and len(set(inp["cls_w"].tolist())) == c.K
        for g in ("g_ce", "g_l1"):
            assert inp[g] is None or len(set(inp[g].tolist())) == c.L
        if c.zero_w:
            assert float(inp["cls_w"][0]) == 0.0 and int((ref["target_class"] == 0).sum()) > 0 and float(ref["wsum"].min()) > 0


def test_set_loss_hard_rows_and_the_gamma_guard(loss_table):
    sides = {}
    for c, inp, ref, cond in loss_table:
        got = SR.model(c, inp)
        sides[c.text] = got["guard"]
        if c.logits == "hard2":
            rows, tc = inp["logits"].view(-1, 2), ref["target_class"].flatten()
            assert [tuple(r) for r in rows[:4].tolist()] == [tuple(r) for r in SR.HARD_ROWS]
            p = torch.softmax(rows.double(), -1)
            u = 1.0 - p.gather(-1, tc.long()[:, None])[:, 0]
            nll = torch.where(u < 0.5, -torch.log1p(-p.flip(-1).gather(-1, tc.long()[:, None])[:, 0]),
                              -torch.log_softmax(rows.double(), -1).gather(-1, tc.long()[:, None])[:, 0])
            sat0 = [i for i in range(len(tc)) if tuple(rows[i].tolist()) == (100.0, -100.0) and tc[i] == 0]
            tiny = [i for i in range(len(tc)) if tuple(rows[i].tolist()) == (30.0, -30.0) and tc[i] == 0]
            other = [i for i in range(len(tc)) if tuple(rows[i].tolist()) == (100.0, -100.0) and tc[i] == 1]
            assert sat0 and tiny and other
            assert math.exp(-200.0) < 2.0 ** -149 and math.exp(-60.0) > 2.0 ** -126        # u = 0 in fp32 / a normal fp32 number
            assert abs(float(nll[other[0]]) - 200.0) < 1e-9 and abs(float(nll[tiny[0]]) / math.exp(-60.0) - 1) < 1e-12
            if c.gamma == 0.5:
                assert got["guard"][0] > 0 and got["guard"][1] >= len(sat0)               # both sides of the guard are taken
                m64 = math.exp(-200.0) ** 0.5 * 1.5
                assert 0 < m64 < 2.0 ** -140                                              # the reference's factor: below fp32's subnormals
                assert not bool(got["dlogits"].view(-1, 2)[sat0].any())                    # the model's (and the kernel's): 0
        if c.logits == "hard8":
            rows = inp["logits"].view(-1, 8)
            assert rows[0].tolist().count(50.0) == 1 and rows[0].tolist().count(-50.0) == 7 and float(rows[1].abs().max()) < 20
    for c, inp, ref, cond in loss_table:
        if c.gamma is None or c.gamma == 0.0:
            assert sides[c.text] == (0, 0)
        elif c.gamma >= 1.0:
            assert sides[c.text] == (c.L * c.B * c.Q, 0)
    assert sum(1 for c, _, _, _ in loss_table if c.gamma == 0.5 and sides[c.text][1] > 0) == 1


def test_set_loss_special_gradients_are_what_they_claim(loss_table):
    for c, inp, ref, cond in loss_table:
        touched = cond["dlines"].sum(-1) > 0 if c.gl1 else None
        if not c.gce:
            assert not bool(ref["dlogits"].any()) and not bool(cond["dlogits"].any())       # exact zeros are demanded
        if c.K == 1:
            assert not bool(ref["dlogits"].any()) and not bool(ref["ce"].any()) and not bool(cond["ce"].any())
        if not c.c0:
            assert not bool(inp["c0"].any())
            if c.gl1:
                assert not bool(ref["dlines"][~touched].any()) and int(touched.sum()) == len(SR.matched(c, inp))
        else:
            assert float(inp["c0"].abs().min()) > 0
            if c.gl1:
                assert torch.equal(ref["dlines"][~touched], inp["c0"].double()[~touched]) and bool((cond["dlines"][touched] >= inp["c0"].double().abs()[touched]).all())
        if not c.gl1:
            assert torch.equal(ref["dlines"], inp["c0"].double())                           # matched rows stay at their entry value
        if c.eq:
            l, t, row = SR.matched(c, inp)[0]
            b, q = row // c.Q, row % c.Q
            assert l == 0 and float(inp["lines"][l, b, q, c.D - 1]) == float(inp["tgt"][t, c.D - 1])
            assert float(ref["dlines"][l, b, q, c.D - 1]) == float(inp["c0"][l, b, q, c.D - 1]) and float(ref["dlines"][l, b, q, 0]) != float(inp["c0"][l, b, q, 0])


def test_set_loss_check_compares_the_bits_of_untouched_rows(loss_table):
    """One ulp on an unmatched row of a nonzero c0, on a matched row without g_l1, and a -0 for a 0: all refused."""
    def ulp_up(t, idx):
        t = t.clone()
        t.view(-1).view(torch.int32)[idx] += 1
        return t
    for c, inp, ref, cond in loss_table:
        got = SR.model(c, inp)
        rows = {row for l, t, row in SR.matched(c, inp) if l == 0}
        free = next(r for r in range(c.B * c.Q + 1) if r not in rows)
        if c.c0 and free < c.B * c.Q:
            with pytest.raises(AssertionError, match="entry value"):
                SR.check(c, dict(got, dlines=ulp_up(got["dlines"], free * c.D)), inp, ref, cond)
        if not c.gl1 and rows:
            with pytest.raises(AssertionError, match="entry value"):
                SR.check(c, dict(got, dlines=ulp_up(got["dlines"], min(rows) * c.D)), inp, ref, cond)
        if not c.c0 and free < c.B * c.Q:
            neg = got["dlines"].clone()
            neg.view(-1)[free * c.D] = -0.0
            with pytest.raises(AssertionError, match="entry value"):
                SR.check(c, dict(got, dlines=neg), inp, ref, cond)
    assert sum(1 for c, _, _, _ in loss_table if c.c0 and c.gl1) >= 2 and any(c.c0 and not c.gl1 for c, _, _, _ in loss_table)


def test_set_loss_clean_model_passes_and_constants_are_the_measured_ones(loss_table):
    _constants_hold(SR, SR.measure_c([t[0] for t in loss_table]))
    for c, inp, ref, cond in loss_table:
        SR.check(c, SR.model(c, inp), inp, ref, cond)


@pytest.mark.parametrize("defect", SR.DEFECTS)
def test_set_loss_defect_is_caught(loss_table, defect):
    caught = _caught(SR, loss_table, defect)
    assert caught
    L = [SR.launch(c) for c in caught]
    if defect == "cap_tail_skipped":
        assert {c.cap for c in caught} == {257, 300} and {c.table for c in caught} == {"full", "kinds"}
    if defect == "bq_tail_skipped":
        assert all(l.bq_trips > 1 for l in L) and {l.BQ for l in L} >= {257, 513}
    if defect in ("valid_ignored", "surplus_labelled"):
        assert all(c.table != "full" for c in caught)
    if defect == "clamp_dropped":
        assert {(c.num_items, c.world) for c in caught} == {(0.0, 1.0), (4.0, 8.0)}
    if defect in ("one_minus_pt", "guard_removed", "focal_over_wsum", "nll_from_lse"):
        assert all(c.gamma is not None for c in caught)
    if defect == "guard_removed":
        assert [(c.gamma, c.logits) for c in caught] == [(0.5, "hard2")]
    if defect == "weight_last_class":
        assert {c.gamma is None for c in caught} == {True, False}
    if defect == "sign0_is_1":
        assert all(c.eq for c in caught) and len(caught) == sum(1 for t in loss_table if t[0].eq)


def test_set_loss_rejected_shapes_are_the_documented_ones():
    for name, (L, B, Q, cap, K, D), gamma, rc in SR.rejected():
        if min(L, B, Q, cap) <= 0 or (gamma is not None and not gamma >= 0.0):
            want = -1
        else:
            want = -4 if not (0 < K <= SR.KMAX and 0 < D <= SR.DMAX) else 0
        assert want == rc, name
    assert sorted(rc for _, _, _, rc in SR.rejected()) == [-4, -4, -4, -1, -1, -1]


# ================================================================================================================== LSAP
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return lsap_build.build(tmp_path_factory.mktemp("lsap"))


@pytest.fixture(scope="module")
def lsap_table():
    out = []
    for c in LR.cases():
        inp = LR.inputs(c)
        out.append((c, inp, LR.reference(c, inp)))
    return out


def test_lsap_cases_reach_the_dispatch_boundary_and_the_columns_per_lane(lsap_table):
    cs = [t[0] for t in lsap_table]
    assert len({c.text for c in cs}) == len(cs) and (LR.LAYERS, LR.PAD) == (2, 5)
    for kind in LR.KINDS:
        mine = [c for c in cs if c.kind == kind]
        assert {c.Q for c in mine} == {1, 2, 20, 63, 64, 65, 255, 256, 257}
        assert {LR.launch(c).NW for c in mine if c.Q <= 256} == {1} and {LR.launch(c).NW for c in mine if c.Q == 257} == {4}
        for Q in LR.QS:
            c = next(c for c in mine if c.Q == Q and c.sizes == LR.sizes_of(Q))
            assert set(c.sizes) == {t for t in (0, 1, Q - 1, Q, Q + 1) if 0 <= t <= 260} and 0 in c.sizes[1:-1]    # an empty image inside
        per_lane = {(c.Q, im.T): (im.per_lane, im.by_query, LR.launch(c).NT) for c in mine for im in LR.launch(c).images}
        assert per_lane[(64, 64)] == (1, False, 64) and per_lane[(65, 65)] == (2, False, 64) and per_lane[(64, 65)] == (2, True, 64)
        assert per_lane[(256, 256)] == (4, False, 64) and per_lane[(257, 257)] == (2, False, 256) and per_lane[(256, 257)] == (5, True, 64)
        assert per_lane[(257, 256)] == (2, False, 256) and per_lane[(257, 258)] == (2, True, 256) and per_lane[(1, 2)] == (1, True, 64)
        for Q in (2, 20):
            assert [per_lane[(Q, T)] for T in (64, 65, 130)] == [(1, True, 64), (2, True, 64), (3, True, 64)]
    for c, inp, ref in lsap_table:
        cost = inp["cost"]
        assert cost.shape == (2, c.B, c.Q, sum(c.sizes) + 5) and int(inp["off"][-1]) == sum(c.sizes) > 0
        blocks = [cost[l, b, :, inp["off"][b]:inp["off"][b + 1]].tobytes() for l in range(2) for b, T in enumerate(c.sizes) if T]
        assert c.kind not in ("uniform", "const") or len(set(blocks)) == len(blocks)      # distinct per (layer, image)
        if c.kind == "const":
            assert all(len(np.unique(cost[l, b])) == 1 for l in range(2) for b in range(c.B))
        if c.kind == "int012":
            assert set(np.unique(cost).tolist()) <= {0.0, 1.0, 2.0}
        if c.kind == "nan_some":
            assert 0.3 < float(np.isnan(cost).mean()) < 0.5 or cost.size < 100
        if c.kind == "inf_row":
            assert bool(np.isinf(cost[:, :, 0]).all()) and (c.Q == 1 or bool(np.isfinite(cost[:, :, 1:]).all()))


@pytest.mark.parametrize("row", range(len(LR.cases())), ids=[c.id for c in LR.cases()])
def test_lsap_reference_equals_the_kernels_source_on_the_cpu(host, lsap_table, row):
    """Every case, both layers, in both wave configurations: the one gwd_lsap dispatches for its Q and the other one (four waves and
    their cross-wave reduce at small Q and on ties, one wave at up to five columns per lane)."""
    c, inp, ref = lsap_table[row]
    for waves in (1, 4):
        got, barriers = lsap_build.launch(host, inp["cost"], inp["off"], waves, sentinel=LR.SENTINEL)
        assert (got == ref).all(), (c.text, waves, np.argwhere(got != ref)[:5].tolist())


def test_lsap_reference_is_a_valid_matching_with_scipys_cost(lsap_table):
    for c, inp, ref in lsap_table:
        LR.check_matching(c, inp, ref)
        assert SR.TC_SENTINEL not in ref and LR.SENTINEL not in ref


@pytest.mark.parametrize("defect", LR.DEFECTS)
def test_lsap_defect_is_caught(lsap_table, defect):
    caught = [c for c, inp, ref in lsap_table if c.Q <= 65 and not (LR.model(c, inp, defect) == ref).all()]
    print("%s: caught on %d of the cases up to Q = 65" % (defect, len(caught)))
    assert caught
    if defect in ("tie_highest_index", "no_sink_preference"):
        assert "uniform" not in {c.kind for c in caught} and {"const", "int012"} & {c.kind for c in caught}
    if defect == "strides_swapped":
        assert all(any(T > c.Q for T in c.sizes) for c in caught)
    if defect in ("padding_unwritten", "offset_ignored", "surplus_minus_one"):
        assert {c.kind for c in caught} == set(LR.KINDS)


def test_lsap_rejected_arguments_are_the_documented_ones():
    for name, (layers, B, Q, sum_targets, max_targets), rc in LR.rejected():
        want = -1 if min(layers, B, Q, sum_targets) <= 0 else (-4 if Q > LR.MAXN or max_targets > LR.MAXN else 0)
        assert want == rc, name
    assert [rc for _, _, rc in LR.rejected()] == [-4, -4, -1]


# ============================================================================================================= sine positions
@pytest.fixture(scope="module")
def pos_table():
    out = []
    for c in PR.cases():
        inp = PR.inputs(c)
        out.append((c, inp, PR.reference(c, inp)))
    return out


def test_pos_cases_reach_both_lds_branches_the_scan_tail_and_the_emit_tail(pos_table):
    cs = [t[0] for t in pos_table]
    assert len({c.text for c in cs}) == len(cs)
    L = {c.text: PR.launch(c) for c in cs}
    hw = {(c.h, c.w): L[c.text] for c in cs}
    assert 128 * 256 == PR.LDS_PIXELS and hw[(128, 256)].in_lds and not hw[(129, 255)].in_lds and 129 * 255 == 32895
    assert sorted(hw_ for hw_, l in hw.items() if not l.in_lds) == [(129, 255)]
    assert hw[(3, 1100)].scan_trips == 2 and hw[(1100, 3)].scan_trips == 2 and 3 + 1100 > PR.SCAN_THREADS
    assert all(l.scan_trips == 1 for k, l in hw.items() if k not in ((3, 1100), (1100, 3)))
    assert {(c.H, c.W, c.h, c.w) for c in cs} >= {(9, 13, 9, 13), (26, 39, 22, 33), (62, 26, 14, 22), (3, 5, 7, 9), (3, 4, 1, 1)}
    assert all(c.mask is None or (c.H <= 2 * c.h and c.W <= 2 * c.w) or (c.H, c.h) == (62, 14) or (c.h, c.w) == (1, 1) for c in cs)
    tails = [c for c in cs if L[c.text].tail]
    assert len(tails) == 1 and (tails[0].B, tails[0].h, tails[0].w, tails[0].F) == (1, 65, 127, 64)
    l = L[tails[0].text]
    assert l.total == 1056640 > PR.EMIT_MAX_BLOCKS * PR.EMIT_THREADS == 1048576 and l.blocks == 4096 and l.emit_trips == 2
    assert min(L[c.text].total for c in cs if c.F) == 2
    emb = [c for c in cs if c.F and c.mask == "batch3"]
    assert {(c.F, c.normalize) for c in emb} == {(F, n) for F in (1, 3, 16, 64) for n in (0, 1)}
    assert any(c.mask is None and c.counts == "max" and (c.h, c.w, c.F) == (1, 1, 1) for c in cs)
    assert any(c.F and not c.normalize and c.w == 1100 for c in cs) and any(c.F and not c.normalize and c.h == 1100 for c in cs)
    assert {c.mask for c in cs} == {"none", "ragged", "batch3", "holes", None}


def test_pos_float_and_integer_nearest_indices_differ_where_claimed(pos_table):
    for n_in, n_out, first in ((26, 22, 11), (39, 33, None), (62, 14, None)):
        f, i = PR.nearest_index(n_out, n_in), PR.nearest_index(n_out, n_in, True)
        assert bool((f != i).any()) and (first is None or int(np.nonzero(f != i)[0][0]) == first)
    # 11 * 26 / 22 is 13; fp32's 26 / 22 is below 13 / 11 and the fp32 product stays below 13
    assert int(PR.nearest_index(22, 26)[11]) == 12 and 11 * 26 // 22 == 13 and float(np.float32(11) * (np.float32(26) / np.float32(22))) < 13.0
    for c, inp, ref in pos_table:
        if c.mask is None:
            continue
        assert PR.launch(c).index_differs == ((c.H, c.h) in ((26, 22), (62, 14)) or (c.W, c.w) in ((26, 22), (39, 33)))
        got = PR.model(c, inp)
        assert torch.equal(got["mask"], ref["mask"]) and torch.equal(got["counts"], ref["counts"])     # the restated index IS ATen's
        if PR.launch(c).index_differs and c.mask == "holes":
            assert not torch.equal(PR.model(c, inp, "integer_nearest")["mask"], ref["mask"])
        assert int(ref["counts"].max()) <= max(c.h, c.w) and int(ref["counts"].min()) >= 0


def test_pos_masks_and_counts_are_what_they_claim(pos_table):
    for c, inp, ref in pos_table:
        if c.mask is None:
            assert inp["counts"].dtype == torch.int16 and (c.counts != "max" or inp["counts"].flatten().tolist() == [32767, 32767])
            continue
        lvl, cnt = ref["mask"].bool(), ref["counts"]
        if c.mask == "batch3":
            assert not bool(lvl[0].any()) and bool(lvl[2].all()) and 0 < int(lvl[1].sum()) < c.h * c.w
            assert not bool(cnt[2].any()) and int(cnt[0, -1, -1, 0]) == c.h and int(cnt[0, -1, -1, 1]) == c.w
            assert bool(lvl[1, -1].all()) and bool(lvl[1, :, -1].all()) and not bool(lvl[1, 0, 0])          # ragged right / bottom
        if c.mask == "holes":
            rows, cols = lvl[0].all(1), lvl[0].all(0)
            assert int(rows.sum()) >= 1 and int(cols.sum()) >= 1 and 0.2 < float(lvl[0].float().mean()) < 0.6
            assert int(cnt[0, rows.nonzero()[0, 0], -1, 1]) == 0 and int(cnt[0, -1, cols.nonzero()[0, 0], 0]) == 0       # last = 0
            # not affine in the index: some count repeats inside a row
            assert bool((cnt[0, :, 1:, 1] == cnt[0, :, :-1, 1]).any())
        if c.F and c.normalize and c.mask in ("batch3", "holes"):
            last0 = (cnt[..., -1:, 1] == 0).expand(cnt.shape[:-1])                                          # rows whose x count ends at 0
            assert bool(last0.any())
            x = ref["out"][..., c.F:]
            k = torch.arange(c.F)
            assert bool((x[last0][:, k % 2 == 0] == 0).all()) and bool((x[last0][:, k % 2 == 1] == 1).all())     # sin 0, cos 0: exact
            got = PR.model(c, inp)["out"][..., c.F:]
            assert torch.equal(got[last0].double(), x[last0])
    big = next(t for t in pos_table if t[0].F and not t[0].normalize and t[0].w == 1100)
    assert float(big[2]["arg"].max()) == 1100.0                                          # unnormalised arguments up to 1100


def test_pos_check_demands_exact_zeros_and_ones_at_a_zero_argument(pos_table):
    hit = 0
    for c, inp, ref in pos_table:
        if not c.F or not bool((ref["arg"] == 0).any()):
            continue
        got = PR.model(c, inp)
        for want in (0.0, 1.0):                                                          # a sine / a cosine of 0, one ulp off
            at = ((ref["arg"] == 0) & (ref["out"] == want)).view(-1).nonzero()
            if len(at):
                out = got["out"].clone()
                out.view(-1)[int(at[0])] = float(np.nextafter(np.float32(want), np.float32(-1.0 if want else 1.0)))
                with pytest.raises(AssertionError, match="zero argument"):
                    PR.check(c, dict(got, out=out), inp, ref)
                hit += 1
    assert hit >= 10


def test_pos_clean_model_passes_and_the_constant_is_the_measured_one(pos_table):
    _constants_hold(PR, PR.measure_c([t[0] for t in pos_table]))
    for c, inp, ref in pos_table:
        PR.check(c, PR.model(c, inp), inp, ref)


@pytest.mark.parametrize("defect", PR.DEFECTS)
def test_pos_defect_is_caught(pos_table, defect):
    caught = _caught(PR, pos_table, defect)
    assert caught
    if defect == "integer_nearest":
        assert all(PR.launch(c).index_differs for c in caught) and {(c.H, c.h) for c in caught} >= {(26, 22), (62, 14)}
    if defect == "scan_tail_skipped":
        assert {(c.h, c.w) for c in caught} == {(3, 1100), (1100, 3)}
    if defect == "emit_tail_skipped":
        assert [PR.launch(c).tail for c in caught] == [True]
    if defect == "parity_from_c":
        assert {c.F % 2 for c in caught} == {1}                                        # only an odd F
    if defect == "x_by_column_last":
        assert all(c.normalize for c in caught)
    if defect == "two_pi_before_division":
        assert all(not c.normalize for c in caught)


def test_pos_rejected_arguments_are_the_documented_ones():
    for name, (B, h, w, F, with_mask), rc in PR.rejected():
        if B <= 0 or h <= 0 or w <= 0:
            want = -1
        elif h > PR.MAX_SIDE or w > PR.MAX_SIDE:
            want = -7
        elif F <= 0:
            want = -1
        else:
            want = -7 if B * h * w * 2 * F >= 2 ** 31 else 0
        assert want == rc, name
    assert any(B * h * w * 2 * F == 2 ** 31 for _, (B, h, w, F, _), _ in PR.rejected())
