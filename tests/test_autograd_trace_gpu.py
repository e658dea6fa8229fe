"""GPU: the launch sequence of the conv-family autograd nodes, delegating mode (tests/autograd_trace.py): the real library's answers
decide the path, the x.is_cuda arms and the real declines included."""
import os

import pytest

from gw_depth_amd import hip
from tests import autograd_trace as A

pytestmark = pytest.mark.gpu

GOLDEN = A.sections(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "autograd_trace.txt")).read())


@pytest.fixture(autouse=True)
def _real_library():
    hip.set_library(None)
    assert not getattr(hip.library(), "is_fake", False)
    yield
    hip.set_library(None)


@pytest.mark.parametrize("case", A.CASES, ids=[c.name for c in A.CASES])
def test_trace_equals_golden(case):
    assert A.compare(case.name, A.run_case(case, "cuda"), GOLDEN["gpu " + case.name]) is None
