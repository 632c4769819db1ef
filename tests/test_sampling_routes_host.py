"""Every route of the sampling loops, on the CPU: sampler x RNG x graph x noise-stack budget x entry point (168 cases,
and 24 more for a projecting policy with a condition beyond horizon step 0; ``tests/sampling_routes.py``) against the
traces the loops left before their four copies of the route decisions became one driver
(``tests/golden/sampling_routes.json``, written by ``tests/golden/make_sampling_routes.py``).  A trace is the engine
calls in order with their arguments, the projection strengths in execution order, which buffers of a fused loop are
persistent, the generator's next draw and the result; the GPU suite runs only a handful of these routes."""
import json
import os

import pytest

from tests import sampling_routes as routes

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sampling_routes.json")) as _fh:
    WANT = json.load(_fh)


def test_the_fixture_holds_the_whole_product():
    assert len(routes.CASES) == 168 + 24 and sorted(WANT) == sorted(routes.CASES)


@pytest.mark.parametrize("case", routes.CASES)
def test_route(case):
    assert routes.run_case(case) == WANT[case]
