"""CPU: the witness table of the convolution kernels (tests/golden/conv_witnesses.txt) is complete and current, and the instrument
that tests/test_conv_witnesses_gpu.py applies to every line of it - fp64 reference, bound, constants of tests/conv_ref.py - bites."""
import re

import pytest
import torch

from tests import conv_ref as R
from tests import conv_witness as W
from tests.test_conv_dispatch import NOT_DISPATCHED, device_stubs, kernel_key

# kernels of the three objects that are no convolution: test_weight_cache_batch_refresh and test_unpad_add_batch have them
COPY_KERNELS = [r"weight_prep_kernel", r"weight_prep_batch_kernel", r"unpad_add_batch_kernel"]


@pytest.fixture(scope="module")
def table():
    return W.load()


@pytest.fixture(scope="module")
def records(table, tmp_path_factory):
    return W.replay(W.build_recorder(tmp_path_factory.mktemp("witness")), [c.text for _, c in table])


def test_every_witness_still_launches_its_kernel(table, records):
    stale = []
    for (kernel, c), rec in zip(table, records):
        rc, ls = W.launches(rec)
        if rc != 0 or [k for k, _ in ls] != [kernel]:
            stale.append("%s\n   wants %s\n   record %s" % (c.text, W.short_name(kernel), rec))
    assert not stale, "tests/golden/conv_witnesses.txt is out of date (tools/make_conv_witnesses.py rewrites it):\n" + "\n".join(stale[:10])


def test_witnesses_cover_every_dispatched_kernel(table):
    kernels = [k for k, _ in table]
    assert len(set(kernels)) == len(kernels), "one line per kernel"
    have = {kernel_key(k) for k in kernels}
    stubs = {kernel_key(s) for s in device_stubs()}
    exempt = {k for k in stubs if any(re.search(p, k) for p in NOT_DISPATCHED + COPY_KERNELS)}
    assert len(exempt) == 2 + 4, sorted(exempt)              # the two never-launched tconv_wgrad variants, three weight copies, one unpad
    assert have == stubs - exempt, "without a witness:\n%s\nnot a kernel of the objects:\n%s" % ("\n".join(sorted(stubs - exempt - have)), "\n".join(sorted(have - stubs)))


def test_witnesses_are_affordable_and_ragged(table):
    for _, c in table:
        assert W.macs(c) <= W.MAX_MACS, c.text
    # every run-time factor of the epilogues is live: act_scale wherever the kernel admits one, the weight gradient's scale likewise
    assert all(c.act_scale != 1.0 for k, c in table if c.call == "F" and c.kind not in (9, 10) and "thin_dgrad" not in k)
    assert all(c.scaled for k, c in table if c.call != "F" and "thin_wgrad" not in k)
    assert {R.epilogue(c).act for _, c in table if c.call == "F"} >= {R.ACT_NONE, R.ACT_RELU, R.ACT_GELU, R.ACT_ELU, R.ACT_SIGMOID}
    assert {R.epilogue(c).gate for _, c in table if c.call == "F"} >= {R.ACT_RELU, R.ACT_ELU, R.ACT_GELU}
    ragged_m = sum(1 for _, c in table if (c.B * c.Ho * c.Wo) % 64)
    assert ragged_m > len(table) // 2                         # most kernels are met with a partial last row tile


def test_compared_rows_leave_no_block_out(table):
    for _, c in table:
        if c.call == "F":
            rows, skipped = R.compare_rows(c)
            assert skipped == 0 and int(rows.max()) == R.rows_of(c) - 1 and len(torch.unique(rows)) == len(rows), c.text
        else:
            for i in range(c.n):
                j = W.with_batch(c, i)
                blocks = R.wgrad_blocks(j)
                assert {b[0] // 32 for b in blocks} >= set(range((c.Cout + 31) // 32)) or blocks == [(0, c.Cout, 0, c.Cin)]
                assert {b[2] // 32 for b in blocks} >= set(range((c.Cin + 31) // 32)) or blocks == [(0, c.Cout, 0, c.Cin)]


def test_parity_classes_of_a_big_stride2_data_gradient():
    """Sampled rows of a stride-2 transposed gather: two pixels of every (oy % 2, ox % 2) class that occurs, per 256 pixels (a call
    above the whole-output limit; the table's own stride-2 witnesses are compared whole today)."""
    c = W.parse_call("F 8 120 160 256 256 3 2 1 1 1 0 0 1")
    rows, skipped = R.compare_rows(c)
    M = R.rows_of(c)
    assert skipped == 0 and len(rows) < M // 8
    m = torch.arange(M)
    key = lambda r: (r // 256) * 4 + ((r // c.Wo) % c.Ho % 2) * 2 + (r % c.Wo) % 2
    have, want = torch.bincount(key(rows), minlength=4 * ((M + 255) // 256)), torch.bincount(key(m), minlength=4 * ((M + 255) // 256))
    assert bool((have >= want.clamp_max(2)).all())


def test_constants_are_the_measured_ones():
    """tests/conv_ref.py's table, measured again: every model maximum is inside its C, no C is slack, and the docstring shows the table."""
    got = R.measure_c()
    assert set(got) == set(R.C)
    for key, worst in sorted(got.items()):
        print("%s %s %s: model maximum %.3f, table %.3f, C %.1f" % (key + (worst, R.MEASURED[key], R.C[key])))
        assert worst <= R.C[key], (key, worst)
        assert R.C[key] <= 2 * worst + 0.1 + 1e-9, (key, worst, R.C[key])
        assert R.C[key] == R.c_of(R.MEASURED[key])
        assert abs(worst - R.MEASURED[key]) <= 0.02, "tests/conv_ref.py's table is out of date: %s measured %.3f, table %.3f" % (key, worst, R.MEASURED[key])
    assert R.format_table(R.MEASURED) in R.__doc__


# ------------------------------------------------------------------------------------------- the instrument bites
def _forward(c):
    return c.call == "F" and c.kind not in (9, 10)


DEFECT_NEEDS = {
    "k_tile": lambda c: _forward(c) and c.Cout >= 32,
    "tap_shift": lambda c: _forward(c) and c.gather == W.GATHER_CONV and c.k == 3 and c.stride == 1 and c.Wi > 2,
    "row_unwritten": lambda c: _forward(c) and R.rows_of(c) % 64 != 0 and c.kind not in (7, 8),
    "block_swap": lambda c: _forward(c) and R.rows_of(c) >= 128,
    "residual_side": lambda c: _forward(c) and c.kind in (4, 11),
    "tail_nonzero": lambda c: _forward(c) and c.Cin % 32 != 0,
    "split_dropped": lambda c: c.call == "W",
    "act_scale": lambda c: _forward(c) and c.act_scale != 1.0,
    "wgrad_scale": lambda c: c.call == "W" and c.scaled,
}
BIG = 131072


def _pick(table, defect, big):
    """The cheapest witness the defect applies to, small (whole output compared) or big (>= 131 072 rows, sampled rows)."""
    fits = [c for _, c in table if DEFECT_NEEDS[defect](c) and (R.rows_of(c) >= BIG) == big]
    assert fits, (defect, big)
    return min(fits, key=W.macs)


def _check(c, defect):
    if c.call == "F":
        inp = R.Inputs(c)
        rows, skipped = R.compare_rows(c, limit=2e7)
        assert skipped == 0
        ref, cond = R.conv_ref_cond(c, inp, rows)
        got = R.conv_model(c, inp, rows, defect)
        for name in ref:
            R.assert_elementwise(got[name], ref[name], cond[name], R.C[(R.operation(c), name, R.dtype_name(c))], ("row", "channel")[:ref[name].dim()],
                                 u=R.out_unit(c, name), what="%s %s" % (c.text, name))
    else:
        inp = R.Inputs(c)
        blocks = R.wgrad_blocks(c, limit=2e7)[:2]
        ref, cond = R.wgrad_ref_cond(c, inp, blocks)
        got = R.wgrad_model(c, inp, blocks, defect)
        for g, r, cd in zip(got, ref, cond):
            R.assert_elementwise(g, r, cd, R.C[("wgrad", "dw", R.dtype_name(c))], ("n", "tap", "c"), u=R.U_F32, what=c.text)


@pytest.mark.parametrize("big", [False, True], ids=["small", "big"])
@pytest.mark.parametrize("defect", R.DEFECTS)
def test_injected_defect_is_caught(table, defect, big):
    c = _pick(table, defect, big)
    _check(c, None)                                           # the clean model passes
    with pytest.raises(AssertionError, match="elements outside"):
        _check(c, defect)
