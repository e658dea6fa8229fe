"""CPU: the case lists of CertainSample (tests/sample_ref.py), the fused stem (tests/stem_ref.py) and the instance-norm GELU
(tests/inorm_ref.py) reach the launch edges they name - shown from the launch arithmetic of the .hip files, restated here -, the
sampling conditions hold for the reference alone, the clean fp32 models pass every case, the constants are the measured ones, and
every injected defect is caught on at least one case.  tests/test_forward_witnesses_gpu.py applies the same instrument to the kernels."""
import numpy as np
import pytest
import torch

from tests import inorm_ref as IR
from tests import sample_ref as SR
from tests import stem_ref as TR


# ======================================================================================================== CertainSample
@pytest.fixture(scope="module")
def sample_table():
    out = []
    for c in SR.cases():
        inp = SR.inputs(c)
        ref, cond = SR.reference(c, inp)
        out.append((c, inp, ref, cond))
    return out


def _sample(sample_table, kind):
    return next(t for t in sample_table if t[0].kind == kind)


def test_sample_clean_model_selects_what_the_reference_selects(sample_table):
    assert len({t[0].text for t in sample_table}) == len(sample_table)
    for c, inp, ref, cond in sample_table:
        assert c.B >= 2 and ref.shape == (c.B, c.S, 1, 2) and ref.dtype == np.float32
        assert np.array_equal(SR.model(c, inp), ref), c.text
        assert float(ref.min()) >= -1.0 and float(ref.max()) < 1.0


def test_sample_exact_regime_variance_is_bit_exact(sample_table):
    """Regime 1: the fp32 variance map of the model equals the fp64 one bit for bit, so ties are real ties on the device too."""
    n = 0
    for c, inp, ref, cond in sample_table:
        if c.regime != "exact":
            continue
        n += 1
        if c.kind not in ("allequal", "thr33000"):              # the half-integer geometry with operands in multiples of 1/64
            assert (c.H == 1 or c.hs == 1 or c.H - 1 == 2 * (c.hs - 1)) and (c.W == 1 or c.ws == 1 or c.W - 1 == 2 * (c.ws - 1)), c.text
        else:
            assert bool((inp["small"] == 0.5).all())
        for k in ("small", "large"):
            assert bool((inp[k] * 64 == np.round(inp[k] * 64)).all()) and float(inp[k].min()) >= 0
        var32 = SR.model_var(c, inp)
        for b in range(c.B):
            assert np.array_equal(var32[b].astype(np.float64), cond["var"][b]), c.text
    assert n >= 10
    ties = [c.kind for c, inp, ref, cond in sample_table if c.regime == "exact" and min(cond["gap"]) == 0.0]
    assert len(ties) >= 6                                      # ties inside the selected range, not merely somewhere


def test_sample_margin_regime_selection_survives_the_fp32_error(sample_table):
    """Regime 2: consecutive variances among the kmax + 1 largest differ by more than twice err, err itself twice the model's largest
    variance error - moving every variance by +- err leaves the reference's selection unchanged."""
    margin = [t for t in sample_table if t[0].regime == "margin"]
    assert {(c.hs, c.ws, c.H, c.W) for c, _, _, _ in margin} == {(15, 20, 30, 40), (50, 70, 192, 192)}
    for c, inp, ref, cond in margin:
        for b in range(c.B):
            print("%s image %d: gap %.3e, err %.3e" % (c.text, b, cond["gap"][b], cond["err"][b]))
            assert cond["err"][b] > 0 and cond["gap"][b] > 2 * cond["err"][b]
            var, kmax = cond["var"][b], cond["kmax"][b]
            for sign in (+1.0, -1.0):                            # the adversarial move: alternate pixels up and down
                moved = var + sign * cond["err"][b] * np.where(np.arange(var.size) % 2 == 0, 1.0, -1.0)
                assert np.array_equal(np.argsort(-moved, kind="stable")[:kmax], np.argsort(-var, kind="stable")[:kmax])
    err, gap = SR.measure_c()
    assert err <= 2 * SR.MEASURED["err"] and gap >= 0.5 * SR.MEASURED["gap"] and SR.C == 0.0


def test_sample_cases_reach_the_limits_and_every_branch(sample_table):
    c, inp, ref, cond = _sample(sample_table, "limits")
    assert (c.H * c.W, c.S, c.n_int) == (SR.MAX_PIX, SR.MAX_S, SR.MAX_INT) == (192 * 192, 256, 8)
    table_bytes = (6 * SR.MAX_S + 2 * SR.MAX_INT + 2 * (SR.THREADS // 64) + 4) * 4
    assert table_bytes + 4 * c.H * c.W > 150000                # dynamic LDS beyond 64 KiB: the attribute path
    assert sum(k > 0 for k in cond["ks"][0]) >= 5
    kinds = {t[0].kind: t for t in sample_table}
    assert (kinds["h1"][0].H, kinds["w1"][0].W) == (1, 1) and (kinds["hsws1"][0].hs, kinds["hsws1"][0].ws) == (1, 1)
    assert any(c.H * c.W < SR.THREADS for c, _, _, _ in sample_table)
    assert kinds["s_eq_hw"][0].S == kinds["s_eq_hw"][0].H * kinds["s_eq_hw"][0].W and kinds["s1"][0].S == 1
    assert kinds["oneint"][0].n_int == 1
    branches = {b for _, _, _, cond in sample_table for b in cond["branch"]}
    assert {"global", "repeat", "complement", "exact"} <= branches           # exact: remain = 0
    c, inp, ref, cond = kinds["repeat"]
    assert cond["branch"][:2] == ["repeat", "complement"] and len(set(cond["branch"])) >= 2
    for b in range(c.B):                                                       # the branch conditions, from the counts
        already, remain = sum(cond["ks"][b]), c.S - sum(cond["ks"][b])
        assert {"repeat": remain >= already > 0, "complement": 0 < remain < already, "global": already == 0}[cond["branch"][b]]
    assert kinds["oneint"][3]["branch"][0] == "exact" and sum(kinds["oneint"][3]["ks"][0]) == kinds["oneint"][0].S
    c, inp, ref, cond = kinds["global"]
    assert cond["branch"] == ["global", "global"] and all(sum(n) == 0 for n in cond["n"])
    assert float(inp["large"][0].max()) < float(inp["edges"][0]) and float(inp["large"][1].min()) >= float(inp["edges"][-1])
    c, inp, ref, cond = kinds["allequal"]
    assert all(len(np.unique(v)) == 1 for v in cond["var"]) and cond["branch"] == ["exact", "complement"]


def test_sample_depths_on_interval_edges(sample_table):
    c, inp, ref, cond = _sample(sample_table, "onedges")
    e = inp["edges"]
    for b in range(c.B):
        l = inp["large"][b].reshape(-1)
        assert bool(np.isin(l, e).all()) and all(int((l == v).sum()) > 0 for v in e)
        assert cond["n"][b] == [int((l == e[i]).sum()) for i in range(c.n_int)]       # an edge belongs to the interval it opens
        assert sum(cond["n"][b]) == l.size - int((l == e[-1]).sum())


def test_sample_threshold_index_search_reaches_bit_15(sample_table):
    c, inp, ref, cond = _sample(sample_table, "thr33000")
    var32 = SR.model_var(c, inp)
    for b in range(c.B):
        T, n_gt, need, I = SR.threshold_search(var32[b], cond["kmax"][b])
        tied = np.nonzero(var32[b].view(np.uint32) == T)[0]
        print("%s image %d: n_gt %d need_eq %d I %d" % (c.text, b, n_gt, need, I))
        assert tied.min() >= 33000 and I >= 32768 and 0 < n_gt < cond["kmax"][b] and need >= 1 and len(tied) > need
        assert I == tied[need - 1]
    assert len(set(int(SR.threshold_search(var32[b], cond["kmax"][b])[3]) for b in range(c.B))) == c.B


def test_sample_k_is_the_fp32_evaluation(sample_table):
    c, inp, ref, cond = _sample(sample_table, "ksplit")
    HW = c.H * c.W
    assert cond["n"][0][0] == SR.KSPLIT_N and c.S == SR.KSPLIT_S
    assert SR.k_of(SR.KSPLIT_N, HW, c.S) != SR.k_of_fp64(SR.KSPLIT_N, HW, c.S) and cond["ks"][0][0] == SR.k_of(SR.KSPLIT_N, HW, c.S)
    n, S = np.float32(SR.KSPLIT_N), np.float32(c.S)
    assert SR.k_of(SR.KSPLIT_N, HW, c.S) == int(min(np.floor((n / np.float32(HW)) * S), n))


def test_sample_rejected_shapes_are_the_documented_ones():
    for B, hs, ws, H, W, S, n_int in SR.rejected():
        assert H * W > SR.MAX_PIX or S > SR.MAX_S or S > H * W or n_int > SR.MAX_INT
    assert len(SR.rejected()) == 4


@pytest.mark.parametrize("defect", SR.DEFECTS)
def test_sample_defect_is_caught(sample_table, defect):
    caught = [c.kind for c, inp, ref, cond in sample_table if not np.array_equal(SR.model(c, inp, defect), ref)]
    print("%s: caught on %s" % (defect, caught))
    assert caught
    want = {"k_fp64": "ksplit", "repeat_off": "repeat", "edge_inclusive": "onedges", "tie_high": "allequal", "x1_noclamp": "hsws1"}[defect]
    assert want in caught


# ================================================================================================================= stem
@pytest.fixture(scope="module")
def stem_table():
    return TR.cases()


def test_stem_cases_reach_seams_padding_and_the_persistent_loop(stem_table):
    assert len({c.text for c in stem_table}) == len(stem_table)
    L = {c.text: TR.launch(c) for c in stem_table}
    tiny = [c for c in stem_table if c.H <= 4 and c.W <= 4 and c.shift == "rand"]
    assert {(c.H, c.W) for c in tiny} == {(h, w) for h in (1, 2, 3, 4) for w in (1, 2, 3, 4)}
    assert {(L[c.text].Hp, L[c.text].Wp) for c in tiny} == {(1, 1)} and {L[c.text].Hc for c in tiny} == {1, 2}
    assert {15, 16, 30, 31} <= {l.Wp for l in L.values()} and {8, 9, 16, 17} <= {l.Hp for l in L.values()}
    assert {l.Wp % TR.PXS for l in L.values()} >= {0, 1} and {l.Hp % TR.PYS for l in L.values()} >= {0, 1}
    assert {(l.Hc % 2, l.Wc % 2) for l in L.values()} == {(0, 0), (0, 1), (1, 0), (1, 1)}      # the last window has / lacks its padding
    big = next(c for c in stem_table if c.B == 513)
    l = L[big.text]
    assert (l.tiles_y, l.tiles_x, l.ntiles, l.rounds, l.grid) == (1, 1, 513, 2, 257)             # tile 256 + blockIdx: a second LDS refill
    assert all(L[c.text].rounds == 1 for c in stem_table if c.B != 513)
    ragged = next(c for c in stem_table if c.B == 3)
    assert (ragged.H, ragged.W) == (97, 131) and L[ragged.text].tiles_y * L[ragged.text].tiles_x > 4
    assert {c.shift for c in stem_table} == {"rand", "none", "neg"} and {c.scale for c in stem_table} == {"rand", "none"}
    assert max(c.B * c.H * c.W * 3 * 2 for c in stem_table) <= 3 * 1000 * 1000


def test_stem_launch_arithmetic_matches_the_wrapper(stem_table):
    from gw_depth_amd import hip
    for c in stem_table:
        assert (TR.launch(c).Hp, TR.launch(c).Wp) == (hip.stem_out(c.H), hip.stem_out(c.W))
    assert TR.PACKED == hip.STEM_PACKED_ELEMS


def test_stem_pack_layout_and_padding(stem_table):
    c = stem_table[0]
    inp = TR.inputs(c)
    packed = TR.pack_reference(inp["w"], inp["scale"])
    wt = TR.unpack(packed)
    assert bool((wt[:, :, 7, :] == 0).all()) and bool((wt[:, :, :, 3] == 0).all())
    want = (inp["w"] * inp["scale"][:, None, None, None]).to(torch.bfloat16).double()
    assert torch.equal(wt[:, :, :7, :3], want) and int((packed != 0).sum()) == 64 * 7 * 7 * 3
    assert not torch.equal(TR.pack_reference(inp["w"], inp["scale"], "kw7"), packed)


def test_stem_clean_model_passes_and_constants_are_the_measured_ones(stem_table):
    worst = 0.0
    for c in stem_table:
        inp = TR.inputs(c)
        packed, got = TR.model(c, inp)
        worst = max(worst, TR.check(c, got, inp, packed))
        if c.shift == "neg":
            assert bool((got[..., [0, 1]] != 0).any())
    print("stem model maximum %.3f, table %.3f, C %.1f" % (worst, TR.MEASURED[TR.KEY], TR.C[TR.KEY]))
    assert worst <= TR.C[TR.KEY] <= 2 * worst + 0.1 + 1e-9 and abs(worst - TR.MEASURED[TR.KEY]) <= 0.02
    assert TR.format_table(TR.MEASURED) in TR.__doc__


def test_stem_inputs_make_a_shifted_tap_visible(stem_table):
    """A tap moved by one pixel changes the outputs by far more than the bound."""
    c = next(c for c in stem_table if (c.B, c.H, c.W, c.shift, c.scale) == (2, 33, 61, "rand", "rand"))
    inp = TR.inputs(c)
    packed, _ = TR.model(c, inp)
    ref, cond = TR.reference(c, inp, packed)
    moved = dict(inp, x=torch.roll(inp["x"], 1, dims=2))
    r = TR.ratio(TR.reference(c, moved, packed)[0], ref, cond, TR.U_BF16)
    assert float(r.median()) > 10 * TR.C[TR.KEY]


@pytest.mark.parametrize("defect", TR.DEFECTS)
def test_stem_defect_is_caught(stem_table, defect):
    caught = []
    for c in stem_table:
        if c.B == 513:
            continue
        inp = TR.inputs(c)
        packed, got = TR.model(c, inp, defect)
        clean = TR.pack_reference(inp["w"], inp["scale"])
        try:
            TR.check(c, got, inp, clean)
        except AssertionError:
            caught.append(c.text)
    print("%s: caught on %d cases" % (defect, len(caught)))
    assert caught
    if defect == "seam_drop":
        assert all(TR.launch(c).Wp > TR.PXS for c in stem_table if c.text in caught)
    if defect == "pad_neighbour":
        assert any(max(c.H, c.W) <= 4 for c in stem_table if c.text in caught)


# ================================================================================================== instance-norm GELU
@pytest.fixture(scope="module")
def inorm_table():
    return IR.cases()


def test_inorm_cases_reach_the_launch_edges(inorm_table):
    assert len({c.text for c in inorm_table}) == len(inorm_table)
    for dt, vn in (("f32", 4), ("bf16", 8)):
        mine = [c for c in inorm_table if c.dtype == dt]
        L = {c.text: IR.launch(c) for c in mine}
        for c in mine:                                          # shape_ok of inorm.hip
            cg = L[c.text].CG
            assert c.C % vn == 0 and cg <= IR.NT and IR.NT % cg == 0 and cg & (cg - 1) == 0 and 0 < c.S <= IR.MAX_S
        assert {1, 256} <= {l.CG for l in L.values()} and (4 in {l.CG for l in L.values()})
        capped = [c for c in mine if L[c.text].capped]
        assert capped and all(L[c.text].CG == 256 and L[c.text].rows == 1 and L[c.text].blocks == 300 > IR.GRID_CAP for c in capped)
        assert any(c.L < L[c.text].rows for c in mine) and any(c.S == 1 for c in mine) and any(c.B == 3 for c in mine)
        assert any(c.S > c.L and L[c.text].sizes.count(0) == 27 for c in mine)
        sizes = {(c.L, c.S): L[c.text].sizes for c in mine}
        assert sizes[(9, 4)] == [3, 3, 3, 0] and sizes[(5, 4)] == [2, 2, 1, 0] and sizes[(10, 4)] == [3, 3, 3, 1]
        assert all(sum(l.sizes) == c.L for c, l in ((c, L[c.text]) for c in mine))
        assert {c.regime for c in mine} == {"plain", "offset", "const", "spike"} and sum(c.chained for c in mine) == 1
        if dt == "f32":
            assert any((c.L, c.C, c.S) == (441, 16, 32) for c in mine) and any((c.B, c.L, c.C, c.S) == (1, 3, 1024, 2) for c in mine)
    assert max(c.B * c.L * c.C * (16 // IR.vn_of(c)) for c in inorm_table) <= 3 * 1000 * 1000           # bytes of the largest operand


def test_inorm_input_regimes_are_what_they_claim(inorm_table):
    for c in inorm_table:
        inp = IR.inputs(c)
        ref, _ = IR.reference_forward(c, inp)
        u = inp["u"].double()
        if c.regime == "offset":
            spread = 1.0 / ref["rstd"]
            assert bool((ref["mean"].abs() > 50 * spread).all()), c.text
        if c.regime == "const":
            assert bool((u[:, :, 1] == 0.75).all()) and bool((ref["rstd"][:, 1] == 1.0 / (IR.EPS ** 0.5)).all())
            assert bool((ref["rstd"][:, 0] < 10).all())
        if c.regime == "spike":
            g = inp["gy"].double().abs()
            assert bool((g.flatten(1).max(dim=1).values == 1000).all()) and float(g.median()) < 1


def test_inorm_clean_model_passes_and_constants_are_the_measured_ones(inorm_table):
    got = IR.measure_c(inorm_table)
    assert set(got) == set(IR.C)
    for key, worst in sorted(got.items()):
        print("%s %s %s: model maximum %.3f, table %.3f, C %.1f" % (key + (worst, IR.MEASURED[key], IR.C[key])))
        assert worst <= IR.C[key] <= 2 * worst + 0.1 + 1e-9, (key, worst)
        assert abs(worst - IR.MEASURED[key]) <= 0.02, "tests/inorm_ref.py's table is out of date: %s measured %.3f" % (key, worst)
    assert IR.format_table(IR.MEASURED) in IR.__doc__
    for c in inorm_table:
        inp = IR.inputs(c)
        IR.check(c, IR.model(c, inp), inp)


def test_inorm_bound_prices_the_fast_erf(inorm_table):
    """erf where the bf16 kernels use Abramowitz & Stegun 7.1.26: inside the same bound - and the two forms do differ in fp32."""
    differ = False
    for c in inorm_table:
        if c.dtype != "bf16":
            continue
        inp = IR.inputs(c)
        IR.check(c, IR.model(c, inp, "exact_erf"), inp)
        v = torch.linspace(-4, 4, 1001)
        fast, exact = IR._gelu_parts(c, v, None)[0], IR._gelu_parts(c, v, "exact_erf")[0]
        d = float((fast.double() - exact.double()).abs().max())
        assert d <= 4.0 * IR.U_F32                               # FAST units
        differ = differ or d > 0.5 * IR.U_F32
    assert differ


@pytest.mark.parametrize("defect", IR.DEFECTS)
def test_inorm_defect_is_caught(inorm_table, defect):
    caught = []
    for c in inorm_table:
        inp = IR.inputs(c)
        try:
            IR.check(c, IR.model(c, inp, defect), inp)
        except AssertionError:
            caught.append(c.text)
    print("%s: caught on %d cases" % (defect, len(caught)))
    assert caught
    by = {c.text: c for c in inorm_table}
    if defect == "one_pass":
        assert any(by[t].regime == "offset" for t in caught)
    if defect in ("merge_unweighted", "empty_as_per"):
        assert all(len(set(IR.launch(by[t]).sizes)) > 1 for t in caught)
    assert {by[t].dtype for t in caught} == {"f32", "bf16"}


def test_inorm_rejected_arguments():
    for dt, C, S, rc in IR.rejected():
        vn = {"f32": 4, "bf16": 8}.get(dt)
        if vn is None:
            assert rc == -2
            continue
        cg = C // vn
        ok = C % vn == 0 and cg <= IR.NT and IR.NT % cg == 0 and cg & (cg - 1) == 0 and S <= IR.MAX_S
        assert not ok and rc == -4
