"""The solve dispatch (csrc/mtg_solve_plan.h) replayed on the GPU: every call of tests/golden/solve_dispatch.json
(recorded by tests/golden/make_solve_dispatch_golden.py before the planner was split out of mtg_capi.hip) must name
the same kernel in mtg_last_solver, character for character."""
import json
import os

import pytest

from golden_util import dispatch_case

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "solve_dispatch.json")))


def test_dispatch_matches_the_recorded_names(engine):
    got = [dispatch_case(engine, case) for case in GOLDEN["cases"]]
    diff = [(case, name) for case, name in zip(GOLDEN["cases"], got) if name != case["solver"]]
    assert not diff, diff
