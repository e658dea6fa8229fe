"""CPU: the fp64 references, cond expressions and rounding models of tests/attn_ref.py over the case matrix of tests/attn_cases.py.

* every reference agrees with tests/fake_device.py (the fp32 stand-in of the kernels) to fp32 accuracy;
* model.shift_regions agrees with the oracle's dense SW-MSA mask as "different label <=> -100";
* the regime of every case holds (hot scores in 30..60, flat rows uniform, the fill of -100 decisive ...);
* the rounding models stay inside the constants C sized from them (C = twice the models' maxima: tests/attn_ref.py's table)."""
import pytest
import torch

from gw_depth_amd import model as M
from oracle import gwdepth_ref as O
from tests import attn_cases as K
from tests import attn_ref as R
from tests.fake_device import FakeDevice

F32_RTOL = 2e-5      # relative L2 of an fp32 evaluation of a well-conditioned sum against fp64 (hot cases: 45 x 2^-24 in the exponent)


def rel(a, b, cond=None):
    """Relative L2 error; with cond, relative to the size of the terms of the sums (a flat case's dq is a sum of terms that cancel to 0)."""
    a, b = a.double(), b.double()
    return float((a - b).norm() / (b.norm() + (0.0 if cond is None else float(cond[0].norm())) + 1e-30))


def small(cases, limit):
    return [n for n, spec in cases.items() if spec[0] * (spec[1] if len(spec) > 1 else 1) <= limit]


def test_shift_regions_match_the_oracle_mask():
    for Hp, Wp in ((7, 7), (14, 21), (21, 28), (35, 42)):
        reg = M.shift_regions(Hp, Wp, "cpu")
        dense = O.shift_mask(Hp, Wp)
        assert dense.shape == (reg.shape[0], 49, 49)
        differ = reg[:, :, None] != reg[:, None, :]
        assert torch.equal(differ, dense == -100.0) and torch.equal(~differ, dense == 0.0)
        assert torch.equal(R.region_fill(reg, reg.shape[0], reg.shape[0], torch.float32)[:, 0], dense)


def test_region_maps_of_the_cases():
    """shift_regions yields labels 0..8, windows with 1, 2 and 4 distinct labels, and label 8 - the only one in the upper lane half of
    the kernels' one-hot k-step - in the last window; the synthetic map uses 9..15."""
    for Hp, Wp in ((21, 28), (35, 42)):
        reg = K.window_regions(("shift", Hp, Wp))
        assert sorted({len(set(r.tolist())) for r in reg}) == [1, 2, 4]
        assert int(reg.min()) == 0 and int(reg.max()) == 8 and 8 in reg[-1].tolist()
    hi = K.window_regions("high")
    assert int(hi.min()) == 9 and int(hi.max()) == 15 and sorted({len(set(r.tolist())) for r in hi}) == [1, 2, 7]


@pytest.mark.parametrize("name", [n for n, s in K.WINDOW_CASES.items() if s[0] <= 300])
def test_window_reference_agrees_with_fake_device(name):
    c = K.window_case(name, torch.float32)
    K.check_window_regime(c)
    a = (c["q"], c["k"], c["v"], c["bias"], c["region"], c["wpi"], c["scale"], c["go"])
    ref, cond = R.window_ref64(*a), R.window_cond(*a)
    f = lambda t: t.float()
    fake = FakeDevice()
    shape = c["q"].shape
    o, gq, gk, gv = (torch.empty(shape) for _ in range(4))
    table = c["table"] is not None
    bias = f(c["table"] if table else c["bias"])
    rel_index = c["rel"].reshape(-1) if table else None
    db = torch.zeros_like(bias)
    fake.winattn_forward(f(c["q"]), f(c["k"]), f(c["v"]), o, bias, c["region"], c["wpi"], c["scale"], rel_index=rel_index)
    fake.winattn_backward(f(c["q"]), f(c["k"]), f(c["v"]), f(c["go"]), gq, gk, gv, bias, db, c["region"], c["wpi"], c["scale"], rel_index=rel_index)
    want_db = R.table_grad(ref["dbias"], c["rel"], 169) if table else ref["dbias"]
    cond["dbias"] = (R.table_grad(cond["dbias"][0], c["rel"], 169) if table else cond["dbias"][0],)
    for n, x, y in (("o", o, ref["o"]), ("dq", gq, ref["dq"]), ("dk", gk, ref["dk"]), ("dv", gv, ref["dv"]), ("dbias", db, want_db)):
        assert rel(x, y, cond[n]) < F32_RTOL, (name, n, rel(x, y, cond[n]))
    # the explicit formulas behind cond and the models are the autograd gradients
    ex, _ = R._window_explicit(*a, lambda t: t, False)
    for n in ref:
        assert rel(ex[n], ref[n], cond[n]) < 1e-12, (name, n)


@pytest.mark.parametrize("name", [n for n, s in K.TOKEN_CASES.items() if s[0] <= 300])
def test_token_reference_agrees_with_fake_device(name):
    c = K.token_case(name, torch.float32)
    K.check_token_regime(c)
    f = lambda t: t.float()
    fake = FakeDevice()
    ref = R.token_pair_ref64(c["q"], c["q2"], c["k"], c["v"], c["scale"], c["go"], c["go2"])
    cond = R.token_pair_cond(c["q"], c["q2"], c["k"], c["v"], c["scale"], c["go"], c["go2"])
    o, o2, gq, gq2 = (torch.empty(c["q"].shape) for _ in range(4))
    gk, gv = torch.empty(c["k"].shape), torch.empty(c["k"].shape)
    fake.tokattn_pair_forward(f(c["q"]), f(c["q2"]), f(c["k"]), f(c["v"]), o, o2, c["scale"])
    fake.tokattn_pair_backward(f(c["q"]), f(c["q2"]), f(c["k"]), f(c["v"]), f(c["go"]), f(c["go2"]), gq, gq2, gk, gv, c["scale"])
    for n, x in (("o", o), ("o2", o2), ("dq", gq), ("dq2", gq2), ("dk", gk), ("dv", gv)):
        assert rel(x, ref[n], cond[n]) < F32_RTOL, (name, n, rel(x, ref[n], cond[n]))
    ex, _ = R._token_explicit(c["q"], c["k"], c["v"], c["scale"], c["go"], lambda t: t, False)
    one = R.token_ref64(c["q"], c["k"], c["v"], c["scale"], c["go"])
    for n, m in (("o", "o"), ("dq", "dq"), ("dk", "dk_acc"), ("dv", "dv_acc")):
        assert rel(ex[m], one[n], cond[n]) < 1e-12, (name, n)


@pytest.mark.parametrize("name", [n for n, s in K.MHA_CASES.items() if s[1] * s[2] <= 40000])
def test_mha_reference_agrees_with_fake_device(name):
    c = K.mha_case(name, torch.float32)
    K.check_mha_regime(c)
    f = lambda t: None if t is None else t.float()
    fake = FakeDevice()
    a = (c["q"], c["k"], c["v"], c["H"], c["kpm"], c["mult"], c["scale"], c["go"])
    ref, cond = R.mha_ref64(*a), R.mha_cond(*a)
    B, L, S, H, E = c["B"], c["L"], c["S"], c["H"], c["E"]
    out, lse = torch.empty(B, L, E), torch.empty(B, H, L)
    gq, gk, gv = torch.empty(B, L, E), torch.empty(B, S, E), torch.empty(B, S, E)
    fake.mha_flash_forward(f(c["q"]), f(c["k"]), f(c["v"]), c["kpm"], f(c["mult"]), out, lse, H, c["scale"])
    fake.mha_flash_backward(f(c["q"]), f(c["k"]), f(c["v"]), f(c["go"]), out, c["kpm"], f(c["mult"]), lse, None, gq, gk, gv, H, c["scale"])
    for n, x in (("o", out), ("lse", lse), ("dq", gq), ("dk", gk), ("dv", gv)):
        assert rel(x, ref[n], cond[n]) < F32_RTOL, (name, n, rel(x, ref[n], cond[n]))


def test_softmax_reference_agrees_with_fake_device():
    fake = FakeDevice()
    for rows, L, amp in K.softmax_cases(torch.float32):
        for masked in (False, True):
            c = K.softmax_case(rows, L, amp, torch.float32, masked)
            ref = R.softmax_ref64(c["x"], c["gy"], c["scale"], c["mask"], c["rpm"])
            y, gx = torch.empty(rows, L), torch.empty(rows, L)
            fake.softmax_masked_forward(c["x"].float(), c["mask"], y, rows, L, c["rpm"], c["scale"])
            fake.softmax_scaled_backward(c["gy"].float(), y, gx, rows, L, c["scale"])
            # amplitude 1e4: an fp32 exponent carries 1e4 x 2^-24 = 6e-4 of absolute error
            tol = max(F32_RTOL, 4 * amp * 2.0 ** -24)
            cond = R.softmax_cond(c["x"], c["gy"], c["scale"], c["mask"], c["rpm"])
            assert rel(y, ref["y"]) < tol and rel(gx, ref["gx"], cond["gx"]) < tol, (rows, L, amp, masked)
            assert rel(R.softmax_backward_ref64(ref["y"], c["gy"], c["scale"]), ref["gx"]) < 1e-12


@pytest.mark.parametrize("name", list(K.REF_CASES))
def test_reference_point_references_agree_with_fake_device(name):
    c = K.ref_case(name, torch.float32)
    K.check_ref_regime(c)
    f = lambda t: t.float()
    fake = FakeDevice()
    B, nwin, H = c["B"], c["nwin"], c["H"]
    ref = R.ref_scores_ref64(c["q"], c["ref_k"], B, c["scale"], c["g_ra"])
    ra, dq, dk = torch.empty(c["g_ra"].shape), torch.empty(c["q"].shape), torch.empty(c["ref_k"].shape)
    fake.ref_scores_forward(f(c["q"]), f(c["ref_k"]), ra, B, nwin, c["scale"])
    fake.ref_scores_backward(f(c["q"]), f(c["ref_k"]), f(c["g_ra"]), dq, dk, B, nwin, c["scale"])
    for n, x in (("ra", ra), ("dq", dq), ("dk", dk)):
        assert rel(x, ref[n]) < F32_RTOL, (name, n)
    ref = R.ref_mix_ref64(c["ra2"], c["ref_v"], H, c["g_q"])
    q_new, att, d_ra, dv = torch.empty(c["g_q"].shape), torch.empty(c["ra2"].shape), torch.empty(c["ra2"].shape), torch.empty(c["ref_v"].shape)
    fake.ref_mix_forward(f(c["ra2"]), f(c["ref_v"]), q_new, att, H)
    fake.ref_mix_backward(att, f(c["ref_v"]), f(c["g_q"]), d_ra, dv, H)
    cond = R.ref_mix_cond(c["ra2"], c["ref_v"], H, c["g_q"], att_stored=ref["att"])
    for n, x in (("q_new", q_new), ("att", att), ("d_ra", d_ra), ("dv", dv)):
        assert rel(x, ref[n], (cond[n][1],) if n == "d_ra" else None) < F32_RTOL, (name, n, rel(x, ref[n]))
    bw = R.ref_mix_backward_ref64(ref["att"], c["ref_v"], H, c["g_q"])                    # the explicit backward is the autograd one
    assert rel(bw["d_ra"], ref["d_ra"], (cond["d_ra"][1],)) < 1e-12 and rel(bw["dv"], ref["dv"]) < 1e-12


def test_comparator_rules():
    ref = torch.tensor([[1.0, 0.0, 2.0]], dtype=torch.float64)
    cond = (torch.tensor([[1.0, 0.0, 0.0]], dtype=torch.float64), None)
    ok = torch.tensor([[1.0 + 2 * R.U_BF16, 0.0, 2.0]])
    assert R.assert_elementwise(ok, ref, cond, 1.01, ("row", "column"), u=R.U_BF16) <= 1.01
    with pytest.raises(AssertionError, match=r"1 of 3 elements .* \(row 0, column 1\)"):          # a zero bound demands an exact zero
        R.assert_elementwise(torch.tensor([[1.0, 1e-30, 2.0]]), ref, cond, 4.0, ("row", "column"), u=R.U_BF16)
    with pytest.raises(AssertionError, match=r"\(row 0, column 2\)"):                            # one wrong element among many
        R.assert_elementwise(torch.tensor([[1.0, 0.0, 2.1]]), ref, cond, 4.0, ("row", "column"), u=R.U_BF16)
    with pytest.raises(AssertionError):                                                          # NaN never passes
        R.assert_elementwise(torch.tensor([[float("nan"), 0.0, 2.0]]), ref, cond, 4.0, ("row", "column"), u=R.U_BF16)


@pytest.mark.parametrize("op", ["window", "token", "mha", "softmax", "ref"])
def test_rounding_models_stay_inside_their_constants(op):
    """The measurement behind tests/attn_ref.py's table, repeated: largest model ratio per (operation, type, output) <= C, and C is
    not slack either (C <= 2 x the measured maximum + the rounding to one decimal)."""
    got = K.measure_c([op])
    assert got
    for (o, dn, out), (worst, case) in got.items():
        c = R.C[o][dn][out]
        print("%s %s %s: model maximum %.3f (%s), C %.1f" % (o, dn, out, worst, case, c))
        assert worst <= c, (o, dn, out, worst, case)
        assert c <= 2 * worst + 0.1 + 1e-9, (o, dn, out, worst, c)
