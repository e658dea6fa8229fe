"""CPU: the case list of the loss and optimizer kernels (tests/loss_ref.py) reaches the launch edges it claims, and the instrument that
tests/test_loss_optim_gpu.py applies to every case - fp64 reference, bound, constants - bites: the clean rounding model passes every
case, the constants are the measured ones, and each injected defect is caught on the smallest and on the largest case it applies to."""
import numpy as np
import pytest
import torch

from tests import loss_ref as R

MAX_BYTES = 40 * 1000 * 1000


@pytest.fixture(scope="module")
def table():
    return R.cases()


def _of(table, family, **kw):
    return [c for c in table if c.family == family and all(getattr(c, k) == v for k, v in kw.items())]


def _ceil(a, b):
    return -(-a // b)


def test_clean_model_passes_every_case(table):
    assert len({c.text for c in table}) == len(table)
    for c in table:
        inp = R.inputs(c)
        R.check(c, R.model(c, inp), inp)


def test_constants_are_the_measured_ones(table):
    """tests/loss_ref.py's table, measured again: every model maximum is inside its C, no C is slack, and the docstring shows the table."""
    got = R.measure_c(table)
    assert set(got) == set(R.C)
    for key, worst in sorted(got.items()):
        print("%s %s %s: model maximum %.3f, table %.3f, C %.1f" % (key + (worst, R.MEASURED[key], R.C[key])))
        assert worst <= R.C[key], (key, worst)
        assert R.C[key] <= 2 * worst + 0.1 + 1e-9, (key, worst, R.C[key])
        assert abs(worst - R.MEASURED[key]) <= 0.02, "tests/loss_ref.py's table is out of date: %s measured %.3f, table %.3f" % (key, worst, R.MEASURED[key])
    assert R.format_table(R.MEASURED) in R.__doc__


# ------------------------------------------------------------------------- the launch arithmetic of losses.hip and optim.hip, written out
def _flat(n, per_block, cap):
    """(blocks, passes, items of the last pass) of a grid-stride loop over n items, `per_block` per block, the grid capped at `cap`."""
    blocks = min(cap, max(1, _ceil(n, per_block)))
    per_pass = blocks * per_block
    return blocks, _ceil(n, per_pass), n - (_ceil(n, per_pass) - 1) * per_pass


def test_sqnorm_cases_reach_the_tail_and_a_partial_third_pass(table):
    sq = _of(table, "sqnorm")
    assert {c.n for c in sq} == {0, 1, 2, 3, 4, 5, 7, 1023, 1024, 1025, 1027, 2 * 2097152 + 1200 + 3}
    assert {c.n & 3 for c in sq} == {0, 1, 2, 3} and any(c.outlier for c in sq)
    big = max(sq, key=lambda c: c.n)
    blocks, passes, last = _flat(big.n // 4, 256, 2048)          # gwd_sqnorm: b = (n / 4 + 255) / 256 capped at 2048; one float4 per thread
    assert (blocks, passes, last, big.n & 3) == (2048, 3, 300, 3)
    assert R.SQNORM_PASS == 2048 * 256
    x = R.inputs(next(c for c in sq if c.outlier))["g"].abs()
    assert 3 <= int((x > 1e3).sum()) <= 8 and float(x.median()) < 1.0
    assert R.SQ_PREFILL != 0


def test_adamw_cases_reach_slices_branches_and_a_partial_third_pass(table):
    ad = _of(table, "adamw")
    big = 2 * 1048576 + 259
    assert {c.n for c in ad} == {1, 255, 256, 257, big}
    for n in (1, 255, 256, 257, big):
        assert {c.off for c in ad if c.n == n} == {0, 1, 3}      # p, g, m, v 4-byte aligned only, p16 2-byte aligned only
    assert _flat(big, 256, 4096) == (4096, 3, 259) and R.ADAMW_PASS == 4096 * 256
    assert _flat(257, 256, 4096)[0] == 2 and _flat(256, 256, 4096)[0] == 1
    plain = [c for c in ad if not c.var and not c.chained and c.n == 257 and c.off == 0]
    assert {(c.ps, c.clip) for c in plain} == {(ps, clip) for ps in R.PSETS for clip in ("on", "off")}
    assert {c.var for c in ad} == {"", "nosq", "mn0", "nop16"} and sum(c.chained for c in ad) >= 1
    ship = {R.PSETS[k] for k in R.PSETS if k.startswith("ship")}
    assert {p[0] for p in ship} == {1e-4, 1e-5} and {p[1] for p in ship} == {1e-4} and {p[2] for p in ship} == {1.0, 0.125} and {p[3] for p in ship} == {1, 3, 1000}
    assert R.PSETS["visible"][:2] == (1e-2, 0.5) and (R.EPS, R.MAX_NORM) == (1e-8, 0.1)
    for c in ad:
        assert R.nbytes(c) <= MAX_BYTES
        if c.n > 1000 and c.off:                                 # (the large inputs are checked once per clip setting)
            continue
        inp, prm = R.inputs(c), R.adamw_params(c)
        total = float(inp["g"].double().norm()) * prm["gs"]
        assert (total > 5 * R.MAX_NORM) if c.clip == "on" else (total < 0.2 * R.MAX_NORM), c.text
        if c.n >= 255:
            zero = (inp["v"] == 0) & (inp["g"] == 0)                             # the denominator is eps alone
            assert int(zero.sum()) >= c.n // 7 and bool((inp["m"][zero] != 0).all())


def test_the_shipped_decay_factor_is_exactly_one():
    """1.0f - lr * wd rounds to 1.0f at the shipped lr 1e-4 / 1e-5 and wd 1e-4 (torch.optim.AdamW multiplies fp32 parameters by the same
    float): the decay is the identity there, bit for bit, and it is not at the visible set."""
    one = np.float32(1.0)
    for name, (lr, wd, _, _) in R.PSETS.items():
        factor = one - np.float32(lr) * np.float32(wd)
        assert (factor == one) == name.startswith("ship"), name
    c = next(c for c in R.cases() if c.family == "adamw" and c.ps == "ship_a" and c.n == 257 and c.clip == "on" and not c.var)
    inp = R.inputs(c)
    assert torch.equal(R.model(c, inp)["p"], R.model(c, inp, "wd_dropped")["p"])


def test_silog_cases_reach_every_launch_form(table):
    sl = _of(table, "silog")
    block = lambda w: 256 if w > 128 else (128 if w > 64 else 64)            # gwd_silog_sums / gwd_silog_backward
    assert {c.w for c in sl if c.h == 5 and c.regime != "invalid"} == {1, 63, 64, 65, 128, 129, 256, 257, 300}
    assert {block(c.w) for c in sl} == {64, 128, 256}
    assert {c.w for c in sl if c.w > block(c.w)} == {257, 300}               # the column loop runs a second, partial time
    assert any((c.h, c.w) == (c.H, c.W) for c in sl)
    big = [c for c in sl if c.B * c.h == 2100]
    assert big and _flat(2100, 1, 512) == (512, 5, 52) and _flat(2100, 1, 2048) == (2048, 2, 52)
    for dt in ("f32", "bf16"):
        for log_err in (0, 1):
            for regime in ("early", "converged"):
                shapes = {(c.B, c.h, c.w, c.H, c.W) for c in sl if (c.dtype, c.log_err, c.regime, c.chained) == (dt, log_err, regime, 0)}
                assert len(shapes) == 13 and (3, 700, 20, 1400, 84) in shapes and (2, 14, 20, 62, 84) in shapes and (2, 21, 21, 93, 93) in shapes
        assert len([c for c in sl if c.dtype == dt and c.regime == "invalid"]) == 1 and len([c for c in sl if c.dtype == dt and c.chained]) == 1
    assert R.GLOSS != 1 and R.LOSS_WEIGHT != 1


def test_float_and_exact_nearest_indices_differ_where_claimed():
    """ATen's float formula min(floorf(dst * ((float)in / (float)out)), in - 1), evaluated here in numpy fp32, is what F.interpolate returns
    and is NOT dst * in // out for the size pairs of the case list."""
    for n_in, n_out, differing in ((62, 14, 1), (84, 20, 1), (93, 21, 2), (11, 5, 0), (1400, 700, 0)):
        dst = np.arange(n_out, dtype=np.float32)
        fl = np.minimum(np.floor(dst * (np.float32(n_in) / np.float32(n_out))).astype(np.int64), n_in - 1)
        oracle = R.nearest_index(n_out, 1, n_in, 1).flatten().numpy()
        exact = np.arange(n_out) * n_in // n_out
        assert (fl == oracle).all(), (n_in, n_out)
        assert int((oracle != exact).sum()) == differing, (n_in, n_out)
    assert int((R.nearest_index(14, 20, 62, 84) != R.exact_index(14, 20, 62, 84)).sum()) == 20 + 14 - 1
    assert int((R.nearest_index(21, 21, 93, 93) != R.exact_index(21, 21, 93, 93)).sum()) == 2 * 21 + 2 * 21 - 4


def test_silog_inputs_hold_the_edges(table):
    sp = R.gt_specials()
    assert float(sp[0]) == float(np.float32(0.2)) and float(sp[1]) < float(sp[0]) and float(sp[2]) == 10.0 and float(sp[3]) < 10.0
    assert R.gt_valid(sp).tolist() == [True, False, False, True, False, False, False, False]
    for c in _of(table, "silog"):
        assert R.nbytes(c) <= MAX_BYTES
        inp = R.inputs(c)
        d, _, valid, _ = R._silog_terms(c, inp)
        lo = inp["gt"].view(c.B, -1)[:, R.nearest_index(c.h, c.w, c.H, c.W).flatten()]
        if c.regime == "invalid":
            assert not valid.any()
            continue
        assert valid.any() and float(valid.double().mean()) > 0.5, c.text           # the valid share stays > 0
        if c.B * c.h * c.w >= 40:
            for v in sp[:7]:
                assert bool((lo == v).any()), (c.text, float(v))
            assert bool(torch.isnan(lo).any())
        if (c.h, c.w) != (c.H, c.W):
            assert bool(torch.isnan(inp["gt"]).sum() > torch.isnan(lo).sum())        # pixels the resize does not pick hold NaN too
        scale = float(d[valid].abs().mean())
        assert (scale < 1e-2) if c.regime == "converged" else (scale > 0.5), (c.text, scale)
        assert bool((inp["pred"].float() > 0).all())


def test_seg_ce_cases(table):
    ce = _of(table, "seg_ce")
    big = 2 * 524288 + 300
    assert {c.P for c in ce} == {1, 255, 256, 257, big}
    assert _flat(big, 256, 2048) == (2048, 3, 300) and R.CE_PASS == 2048 * 256        # flat_grid(): (P + 255) / 256 capped at 2048
    for dt in ("f32", "bf16"):
        small = {(c.P, c.kind, c.target) for c in ce if c.dtype == dt and c.P < 1000}
        assert small == {(P, k, t) for P in (1, 255, 256, 257) for k in ("spread", "gap", "equal") for t in ("zeros", "ones", "mixed")}
        assert {c.kind for c in ce if c.dtype == dt and c.P == big} == {"spread", "gap", "equal"}
    for c in ce:
        assert R.nbytes(c) <= MAX_BYTES
        if c.P > 1000 and c.dtype == "bf16" and c.kind != "gap":
            continue
        inp = R.inputs(c)
        x, t = inp["logits"].double(), inp["target"]
        gap = (x[:, 0] - x[:, 1]).abs()
        if c.kind == "equal":
            assert bool((gap == 0).all())
        elif c.kind == "gap":
            assert bool((gap >= 79).all())
            if c.dtype == "bf16" and c.P > 17:
                assert bool((gap > 1e38).any()) and bool(torch.isfinite(inp["logits"].float()).all())
        if c.P > 1:
            assert set(t.tolist()) == {"zeros": {0}, "ones": {1}, "mixed": {0, 1}}[c.target]
    assert R.CE_PREFILL != 0


def test_anchor_cases_reach_the_lane_segment_idle_threads_and_both_grid_caps(table):
    an = _of(table, "anchor")
    Rs, Ps = (1, 7, 15, 16, 17, 80, 100, 128, 129, 255, 256), (1, 15, 16, 17, 37, 1000)
    for dt in ("f32", "bf16"):
        assert {(c.R, c.P) for c in an if c.dtype == dt and c.B == 3} == {(r, p) for r in Rs for p in Ps}
    assert {r for r in Rs if 256 % r} == {7, 15, 17, 80, 100, 129, 255}              # threads of the backward block without a (slot, channel)
    fwd = lambda P: (min(1024, _ceil(P, 256)), _ceil(P, min(1024, _ceil(P, 256)) * 16))     # blocks (16 pixels each per round), rounds
    assert _ceil(262437, 256) > 1024 and fwd(262437) == (1024, 17) and 262437 - 16 * 1024 * 16 == 293
    assert fwd(15) == (1, 1) and fwd(17) == (1, 2)
    bwd = lambda P, r: _ceil(P, (256 // r) * 16)                                      # blocks before the cap of 512
    assert bwd(8229, 256) == 515 and bwd(1000, 256) == 63 and bwd(262437, 7) == 456
    assert any((c.P, c.R) == (262437, 7) for c in an) and any((c.P, c.R) == (8229, 256) for c in an)
    assert all(R.nbytes(c) <= MAX_BYTES for c in an)
    assert bool((R.pattern(256) != 0).all())


def test_all_cases_stay_under_40_mb(table):
    assert max(R.nbytes(c) for c in table) <= MAX_BYTES


# ------------------------------------------------------------------------------------------- the instrument bites
def _gt_holds_ten(c):
    lo = R.inputs(c)["gt"].view(c.B, -1)[:, R.nearest_index(c.h, c.w, c.H, c.W).flatten()]
    return bool((lo == 10.0).any())


def _p16_moves(c):
    """The defect is visible only where the update moves the bf16 image of at least one parameter."""
    inp = R.inputs(c)
    return not torch.equal(R.reference(c, inp)[0]["p16"], inp["p"].to(torch.bfloat16).double())


def _partial(n, per_pass):
    return n > per_pass and n % per_pass != 0


_live = lambda c: c.family == "silog" and c.regime != "invalid"
DEFECT_NEEDS = {
    "sqnorm_tail": lambda c: c.family == "sqnorm" and c.n % 4 != 0,
    "last_pass_sqnorm": lambda c: c.family == "sqnorm" and _partial(c.n // 4, R.SQNORM_PASS),
    "last_pass_adamw": lambda c: c.family == "adamw" and _partial(c.n, R.ADAMW_PASS),
    "last_pass_seg_ce": lambda c: c.family == "seg_ce" and _partial(c.P, R.CE_PASS),
    "last_pass_silog_rows": lambda c: _live(c) and _partial(c.B * c.h, R.SILOG_BWD_ROWS),
    "silog_col_loop": lambda c: _live(c) and c.w > 256,
    "exact_index": lambda c: _live(c) and not torch.equal(R.nearest_index(c.h, c.w, c.H, c.W), R.exact_index(c.h, c.w, c.H, c.W)),
    "gt_le_10": lambda c: _live(c) and _gt_holds_ten(c),
    "lambda_missing": _live,
    "nonlog_one_missing": lambda c: _live(c) and not c.log_err,
    "ce_no_div_p": lambda c: c.family == "seg_ce" and c.P > 1,
    "wd_dropped": lambda c: c.family == "adamw" and c.ps.startswith("visible"),
    "eps_inside_bc": lambda c: c.family == "adamw" and c.n >= 255,                 # an element with v = 0 and g = 0
    "clip_always": lambda c: c.family == "adamw" and c.clip == "off" and c.var in ("", "nop16"),
    "grad_scale_twice": lambda c: c.family == "adamw" and R.PSETS[c.ps][2] != 1.0,
    "p16_stale": lambda c: c.family == "adamw" and c.var != "nop16" and _p16_moves(c),
    "danchor_overwrite": lambda c: c.family == "anchor",
    "anchor_16_lanes": lambda c: c.family == "anchor" and c.R > 16,
}
assert set(DEFECT_NEEDS) == set(R.DEFECTS)


def _pick(table, defect, big):
    """The smallest, or the largest, case that the defect applies to."""
    order = sorted(table, key=lambda c: (R.nbytes(c), c.text), reverse=big)
    return next(c for c in order if DEFECT_NEEDS[defect](c))


@pytest.mark.parametrize("big", [False, True], ids=["small", "largest"])
@pytest.mark.parametrize("defect", R.DEFECTS)
def test_injected_defect_is_caught(table, defect, big):
    c = _pick(table, defect, big)
    inp = R.inputs(c)
    R.check(c, R.model(c, inp), inp)                          # the clean model passes
    with pytest.raises(AssertionError, match="elements outside"):
        R.check(c, R.model(c, inp, defect), inp)


def test_p16_is_checked_against_the_returned_p(table):
    """A p16 rounded from the fp64 reference instead of from the returned fp32 p differs from it in some element of a large case."""
    c = next(c for c in table if c.family == "adamw" and c.n > 1000 and c.var != "nop16")
    inp = R.inputs(c)
    got = R.model(c, inp)
    got["p16"] = R.reference(c, inp)[0]["p"].to(torch.bfloat16)
    if not torch.equal(got["p16"], got["p"].to(torch.bfloat16)):
        with pytest.raises(AssertionError, match="p16: .* elements outside"):
            R.check(c, got, inp)


def test_sums_fed_to_the_later_kernels_are_the_reference_ones(table):
    """feeds(): the fp64 sums of the reference, and none for the chained cases (they take the device's own)."""
    small = [c for c in table if R.nbytes(c) < 100000 and c.family in ("silog", "adamw")]
    assert any(c.chained for c in small)
    for c in small:
        inp = R.inputs(c)
        fed = R.feeds(c, inp)
        if c.chained or (c.family == "adamw" and c.var == "nosq"):
            assert fed is None
        elif c.family == "silog":
            ref, _ = R.reference(c, inp)
            assert fed["sums"].dtype == torch.float64 and torch.equal(fed["sums"], torch.cat([ref["s0"], ref["s1"], ref["count"]]))
        else:
            assert fed["sq"].dtype == torch.float64 and float(fed["sq"]) == float((inp["g"].double() ** 2).sum())
