"""CPU: the witness table of the row kernels (tests/golden/row_witnesses.txt) is complete and current, and the instrument that
tests/test_row_witnesses_gpu.py applies to every line of it - fp64 reference, bound, constants of tests/row_ref.py - bites."""
import importlib.util
import os
import re

import pytest
import torch

from tests import row_ref as R
from tests import row_witness as W
from tests.test_conv_dispatch import ROOT, kernel_key

# Kernels of rowops.o that no call can reach, as patterns over the mangled name, each with the condition in rowops.hip that bars it.
NOT_DISPATCHED = [
    # launch_ln_fwd_vec<__bf16, 16, PAD>: LN_FWD(64, 2) needs 64 < ld / VEC <= 128 with VEC = 8, i.e. ld > 512, and gwd_layernorm_forward
    # returns -1 for `ld > 64 * MAX_PER_LANE` (= 512) before it selects anything.  Both PAD, both GELU: four kernels.
    r"layernorm_fwd_vec_kernelIDF16bLi64ELi2ELi16ELb[01]ELb[01]E",
    # launch_ln_bwd_vec<__bf16, 16, PAD>: LN_BWD(64, 2) behind the same `ld > 64 * MAX_PER_LANE` of gwd_layernorm_backward; its NWV = 16
    # form is not even instantiated (`LPR * NCH * VEC <= 512` is 1024 <= 512: rows wider than 512 slots), the four NWV = 4 ones are.
    r"layernorm_bwd_vec_kernelIDF16bLi64ELi2ELi16ELi4ELb[01]ELb[01]E",
]


@pytest.fixture(scope="module")
def table():
    return W.load()


@pytest.fixture(scope="module")
def recorder(tmp_path_factory):
    return W.build_recorder(tmp_path_factory.mktemp("row_witness"))


def test_every_witness_still_launches_its_kernel(table, recorder):
    stale = []
    for (kernel, c), rec in zip(table, W.replay(recorder, [c.text for _, c in table])):
        rc, ls = W.launches(rec)
        names = [k for k, _, _ in ls]
        if rc != 0 or (kernel not in names if c.family == "inorm" else names != [kernel]):
            stale.append("%s\n   wants %s\n   record %s" % (c.text, W.short_name(kernel), rec))
    assert not stale, "tests/golden/row_witnesses.txt is out of date (tools/make_row_witnesses.py rewrites it):\n" + "\n".join(stale[:10])


def test_run_time_siblings_launch_the_same_kernel(table, recorder):
    """row_ref.forms(): the other activations of a run-time switch and the one-job batch reach the kernel of their line."""
    pairs = [(kernel, f) for kernel, c in table for f in R.forms(c)[1:]]
    assert len(pairs) >= 4 * 4 + 4 + 1 + 2
    for (kernel, f), rec in zip(pairs, W.replay(recorder, [f.text for _, f in pairs])):
        rc, ls = W.launches(rec)
        assert rc == 0 and [k for k, _, _ in ls] == [kernel], (f.text, rec)


def test_witnesses_cover_every_dispatched_kernel(table):
    kernels = [k for k, _ in table]
    assert len(set(kernels)) == len(kernels), "one line per kernel"
    have = {kernel_key(k) for k in kernels}
    stubs = {kernel_key(s) for s in W.device_stubs()}
    exempt = {k for k in stubs if any(re.search(p, k) for p in NOT_DISPATCHED)}
    assert len(stubs) == 231 and len(exempt) == 4 + 4, (len(stubs), sorted(exempt))
    assert have == stubs - exempt, "without a witness:\n%s\nnot a kernel of the objects:\n%s" % ("\n".join(sorted(stubs - exempt - have)), "\n".join(sorted(have - stubs)))


def test_table_is_what_the_generator_writes():
    spec = importlib.util.spec_from_file_location("make_row_witnesses", os.path.join(ROOT, "tools", "make_row_witnesses.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.build_table()[0] == open(W.FIXTURE).read()


def _ln(table, call=None):
    return [c for _, c in table if c.family == "layernorm" and (call is None or c.call == call)]


def test_witnesses_are_demanding(table):
    """The shapes and the run-time forms the table has to hold (the generator lets the kernels take turns over widths and flags: this is the check)."""
    for _, c in table:
        assert W.nbytes(c) <= W.MAX_BYTES, c.text
    for dt in (W.BF16, W.F32):
        ln = [c for c in _ln(table) if c.dtype == dt]
        widths = {(c.C, c.ld) for c in ln}
        vec = 8 if dt == W.BF16 else 4
        # every (LPR, NCH) bucket of the 16-byte form just above the previous limit and at its own; C = 160; the 8-byte forms; padded rows
        # whose last vector is part real, part padding; the generic kernels (odd C; C = 2 mod 4 above 256 in fp32)
        limits = [8, 16, 32, 64] + ([128] if dt == W.F32 else [])
        want = {(l * vec, 0) for l in limits} | {((l + 1) * vec, 0) for l in limits[:-1]} | {(160, 0), (30, 32), (60, 64), (300, 304)}
        want |= {(60, 0), (120, 0), (300, 0)} if dt == W.BF16 else {(30, 0), (62, 0), (254, 0), (258, 0)}
        assert want <= widths, sorted(want - widths)
        assert any(c.C % 2 == 1 and not c.ld for c in ln)
        for call in ("LF", "LB"):
            sub = [c for c in ln if c.call == call]
            assert {c.affine for c in sub} == {0, 1} and {c.gelu for c in sub} == {0, 1}
            if call == "LF":
                assert {c.residual for c in sub} == {0, 1}
            else:
                assert {c.gskip for c in sub} == {0, 1} and {c.elu for c in sub} == {0, 1} and {c.dgamma for c in sub} == {0, 1}
        ragged = sum(1 for c in ln if c.rows % (4 * R._ln_group(c)))
        assert ragged > len(ln) * 3 // 4
        assert sum(1 for c in ln if c.rows >= 1024) > len(ln) // 2            # the grid-stride loop runs twice
        sm = [c for _, c in table if c.family == "softmax" and c.dtype == dt]
        for c in sm:                                                          # 2048 workgroups of 4 waves, a partial second pass where it fits
            per_row = W.nbytes(c) / c.rows
            assert c.rows % 4 and (c.rows > 8192 or 8193 * per_row > W.MAX_BYTES), c.text
        masked = [c for c in sm if c.call == "SM" and c.mask]
        assert any(c.rpm > 1 for c in masked) and any(c.scaled for c in sm if c.call == "SM") and any(c.scaled for c in sm if c.call == "SS")
        assert {c.call for c in sm} == {"SF", "SM", "SB", "SS"}
        act = [f for _, c in table if c.family == "act" and c.dtype == dt for f in R.forms(c)]
        assert {f.act for f in act} == set(range(5)) and {f.act_scaled for f in act} == {0, 1}
        assert {f.chscale for f in act if f.call == "AB"} == {0, 1} and {f.mult for f in act if f.call == "AC"} == {0, 1}
        cs = [c for _, c in table if c.call in ("CS", "AC") and c.dtype == dt]
        assert any(256 % (c.C // vec) for c in cs if c.C % vec == 0)          # a threadblock tail with slot >= rpb
        (cb,) = [c for _, c in table if c.call == "CB" and c.dtype == dt]
        rpb = lambda C: 256 // (C // vec)
        assert len(cb.jobs) == 16 and len(set(cb.jobs)) == 16 and sum(1 for r, C in cb.jobs if r <= 16 * rpb(C)) >= 4
        ino = [c for _, c in table if c.family == "inorm" and c.dtype == dt]
        assert any(c.L < c.S for c in ino) and any(c.L % c.S and c.L > c.S for c in ino) and any(c.L == 1 for c in ino) and any(c.B > 1 for c in ino)
        assert {1, 256} <= {c.C // vec for c in ino} and any(c.L * (c.C // vec) > 256 * 256 for c in ino)
    assert {c.L for _, c in table if c.family == "softmax"} == {1, 63, 64, 65, 128, 129, 192, 193, 320, 321, 512, 513, 1024, 1025, 1200}
    assert any(c.C == 16 and c.L > 32768 for _, c in table if c.family == "inorm" and c.dtype == W.BF16)


def test_inputs_make_the_bound_bite(table):
    """Offset rows next to zero-mean ones and a constant row, true ELU outputs, hard logits with -inf and the four mask shapes."""
    for dt in (W.BF16, W.F32):
        c = next(c for c in _ln(table, "LF") if c.dtype == dt and c.rows > 100 and c.C >= 60)
        x = R.inputs(c)["x"][:, :c.C].double()
        mean, std = x.mean(1), x.std(1, unbiased=False)
        ulp = mean.abs() * (2.0 ** -7 if dt == W.BF16 else 2.0 ** -23)
        off = mean.abs() >= 10 * std
        assert off.sum() > c.rows // 3 and (~off).sum() > c.rows // 3 and bool((std[off] >= 8 * ulp[off])[std[off] > 0].all())
        assert int((std == 0).sum()) == 1
        u = R.inputs(next(c for _, c in table if c.call == "IF" and c.dtype == dt and c.L > 1000))["u"].double()
        assert bool((u.mean(1).abs() >= 10 * u.std(1, unbiased=False)).any())
        e = next(c for c in _ln(table, "LB") if c.dtype == dt and c.elu and c.rows > 100)
        x = R.inputs(e)["x"][:, :e.C]
        assert bool((x > -1).all()) and bool((x < 0).any()) and bool((x > 0).any()) and bool((x == 0).any())
        m = next(c for _, c in table if c.call == "SM" and c.mask and c.dtype == dt and c.L > 128)
        inp = R.inputs(m)
        mask = inp["mask"].bool()
        assert bool(mask[:, 0].any()) and bool(mask[:, -1].any()) and bool((mask.sum(-1) == m.L - 1).any()) and not mask.all(-1).any()
        assert bool(torch.isinf(inp["x"].float()).any())
        ref, _ = R.reference(m, inp)
        assert bool(torch.isfinite(ref["y"]).all()) and float((ref["y"] < 2.0 ** -126).double().mean()) > 0.5      # most terms underflow fp32 or are masked


def test_constants_are_the_measured_ones(table):
    """tests/row_ref.py's table, measured again: every model maximum is inside its C, no C is slack, and the docstring shows the table."""
    got = R.measure_c(table)
    assert set(got) == set(R.C)
    for key, worst in sorted(got.items()):
        print("%s %s %s: model maximum %.3f, table %.3f, C %.1f" % (key + (worst, R.MEASURED[key], R.C[key])))
        assert worst <= R.C[key], (key, worst)
        assert R.C[key] <= 2 * worst + 0.1 + 1e-9, (key, worst, R.C[key])
        assert abs(worst - R.MEASURED[key]) <= 0.02, "tests/row_ref.py's table is out of date: %s measured %.3f, table %.3f" % (key, worst, R.MEASURED[key])
    assert R.format_table(R.MEASURED) in R.__doc__


# ------------------------------------------------------------------------------------------- the instrument bites
DEFECT_NEEDS = {
    "ragged_unwritten": lambda c: c.family == "layernorm" and c.rows % R._ln_group(c) != 0,
    "onepass_var": lambda c: c.call == "LF" and c.rows >= 2,
    "pad_nonzero": lambda c: c.family == "layernorm" and c.ld > c.C,
    "lanes_beyond_c": lambda c: c.call == "LF" and c.ld > c.C,
    "dgamma_wave": lambda c: c.call == "LB" and c.dgamma,
    "softmax_tail": lambda c: c.call in ("SF", "SM") and c.L > 64,
    "mask_mod": lambda c: c.call == "SM" and c.mask and c.rpm > 1 and c.L > 1,
    "scale_dropped": lambda c: c.call == "SS" and c.scaled and c.L > 1,
    "elu_no_div": lambda c: c.family == "act" and c.act == W.ACT_ELU and c.act_scaled,
    "merge_no_between": lambda c: c.call == "IF" and c.L > c.S,
    "last_slice_short": lambda c: c.family == "inorm" and c.L > 1,
    "block0_off_by_one": lambda c: c.call == "CB" and len(c.jobs) > 1,
}


def _pick(table, defect, big):
    """The smallest, or the largest, witness (run-time siblings included) that the defect applies to."""
    fits = [f for _, c in table for f in R.forms(c) if DEFECT_NEEDS[defect](f)]
    assert fits, defect
    return (max if big else min)(fits, key=lambda f: (W.nbytes(f), f.text))


@pytest.mark.parametrize("big", [False, True], ids=["small", "largest"])
@pytest.mark.parametrize("defect", R.DEFECTS)
def test_injected_defect_is_caught(table, defect, big):
    c = _pick(table, defect, big)
    inp = R.inputs(c)
    R.check(c, R.model(c, inp), inp)                          # the clean model passes
    with pytest.raises(AssertionError, match="elements outside"):
        R.check(c, R.model(c, inp, defect), inp)


def test_dbias_is_checked_against_the_returned_gx(table):
    """A dbias that is the column sum of the UNROUNDED gx is outside the fp32-sum bound on a bf16 witness of a few thousand rows."""
    c = max((c for _, c in table if c.call == "AC" and c.dtype == W.BF16), key=W.nbytes)
    inp = R.inputs(c)
    got = R.model(c, inp)
    exact, _ = R.reference(c, inp)
    got["dbias"] = (R.pattern(c.C).double() + exact["gx"].sum(0)).float()
    with pytest.raises(AssertionError, match="dbias: .* elements outside"):
        R.check(c, got, inp)
