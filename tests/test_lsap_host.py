"""csrc/lsap.hip compiled for the CPU (tests/lsap_host.cpp: the kernel's own source, one fiber per lane, barriers and shuffles
emulated; built by tests/lsap_build.py): the matrices no GPU test feeds the kernel.  Finite costs give scipy's assignment in both orientations and both workgroup
sizes; NaN, +inf, -inf and all-NaN matrices end within the barrier count that the kernel's loop bounds allow and return a valid
matching (distinct pairs, min(Q, T) of them) - arbitrary, not optimal, once a non-finite cost has been read as 1e30."""
import numpy as np
import pytest
from scipy.optimize import linear_sum_assignment

from tests import lsap_build
from tests.lsap_build import solve


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return lsap_build.build(tmp_path_factory.mktemp("lsap"))


def barrier_bound(Q, T, waves):
    """__syncthreads() a thread can pass: 1 after the fills, per row `cur` 1 after the reset, (2, or 3 with the cross-wave reduce) per
    search trip and at most cur + 1 trips, 2 around the augmentation; 1 before the output."""
    rows = min(Q, T)
    return 2 + sum(3 + (3 if waves > 1 else 2) * (cur + 1) for cur in range(rows))


def check_valid(q_of_t, Q, T):
    m = q_of_t[q_of_t < Q]
    assert ((q_of_t >= 0) & (q_of_t <= Q)).all() and len(m) == min(Q, T) and len(set(m.tolist())) == len(m)


@pytest.mark.parametrize("Q,sizes,waves", [(12, (9, 12, 0), 1), (9, (12, 1), 1), (40, (5, 37), 1), (9, (12, 7), 4)])
def test_finite_costs_give_scipys_assignment(host, Q, sizes, waves):
    rng = np.random.default_rng(Q)
    cost = (rng.random((Q, sum(sizes) + 3)) * 5 - 1).astype(np.float32)
    out, off, n = solve(host, cost, sizes, 3, waves)
    assert (out[off[-1]:] == Q).all()
    for b, T in enumerate(sizes):
        got = out[off[b]:off[b + 1]]
        check_valid(got, Q, T)
        qi, ti = linear_sum_assignment(cost[:, off[b]:off[b + 1]].astype(np.float64))
        want = np.full(T, Q)
        want[ti] = qi
        assert (got == want).all(), (b, got, want)
    assert n <= max(barrier_bound(Q, T, waves) for T in sizes)


@pytest.mark.parametrize("Q,T,waves", [(12, 9, 1), (9, 12, 1), (10, 10, 4)])
@pytest.mark.parametrize("kind", ["nan_some", "inf_row", "neg_inf_col", "mixed", "all_nan", "all_inf", "all_neg_inf"])
def test_non_finite_costs_end_within_the_bound(host, Q, T, kind, waves):
    rng = np.random.default_rng(Q * 31 + T)
    cost = (rng.random((Q, T)) * 5 - 1).astype(np.float32)
    if kind in ("nan_some", "mixed"):
        cost[rng.random((Q, T)) < 0.4] = np.nan
    if kind in ("inf_row", "mixed"):
        cost[0, :] = np.inf
    if kind in ("neg_inf_col", "mixed"):
        cost[:, 1] = -np.inf
    if kind.startswith("all_"):
        cost[:] = {"all_nan": np.nan, "all_inf": np.inf, "all_neg_inf": -np.inf}[kind]
    out, off, n = solve(host, cost, (T,), 0, waves)
    check_valid(out, Q, T)
    assert n <= barrier_bound(Q, T, waves), (n, barrier_bound(Q, T, waves))
