"""CPU: the launch sequence of the conv-family autograd nodes, dry mode (tests/autograd_trace.py), against the golden trace."""
import os

import pytest

from tests import autograd_trace as A

GOLDEN = A.sections(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "autograd_trace.txt")).read())
CPU_CASES = [c for c in A.CASES if not c.gpu_only]


@pytest.mark.parametrize("case", CPU_CASES, ids=[c.name for c in CPU_CASES])
def test_trace_equals_golden(case):
    assert A.compare(case.name, A.run_case(case, "cpu"), GOLDEN["cpu " + case.name]) is None


def test_golden_has_exactly_the_cases():
    assert sorted(GOLDEN) == sorted(["cpu " + c.name for c in CPU_CASES] + ["gpu " + c.name for c in A.CASES])
    assert len({c.name for c in A.CASES}) == len(A.CASES)
