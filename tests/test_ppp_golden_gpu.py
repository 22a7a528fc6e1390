"""ppp.protassov_test end to end on the GPU against the numbers of the commit before its host path was cut into a plan
and stages (tests/golden/ppp_end_to_end.json, recorded by tests/golden/make_ppp_end_to_end_golden.py): T_obs, every T_sim
and the p-value, bit for bit, in every mode of the observed chains and the refits."""
import json
import os
import warnings

import numpy as np
import pytest

from golden_util import protassov_problem

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
MODES = json.load(open(os.path.join(HERE, "golden", "ppp_end_to_end.json")))["modes"]


def test_the_fixture_holds_the_modes():
    assert sorted(MODES) == ["defaults", "odd_walkers", "refits_sequential", "refits_side_by_side", "refits_unpaired", "reproducible"]
    assert MODES["odd_walkers"]["kwargs"] == {"walkers": 15, "sim_walkers": 16}


@pytest.mark.parametrize("mode", sorted(MODES))
def test_protassov_test_gives_the_numbers_it_gave(mode):
    from mind_the_gaps_amd.ppp import protassov_test
    lc, null, alt, common = protassov_problem()
    want = MODES[mode]
    np.random.seed(20250704)
    np.random.random(3)                                  # (a generator that is in the middle of its stream)
    state = np.random.get_state()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = protassov_test(lc, null, alt, **dict(common, **want["kwargs"]))
    print(mode, float(res["T_obs"]).hex(), [float(v).hex() for v in res["T_sim"]], float(res["p_value"]).hex())
    assert float(res["T_obs"]) == float.fromhex(want["T_obs"])
    assert [float(v) for v in res["T_sim"]] == [float.fromhex(v) for v in want["T_sim"]]
    assert float(res["p_value"]) == float.fromhex(want["p_value"])
    if mode == "odd_walkers":
        # the host-side sampler ran on numpy's global generator, seeded for the chain: it is back where it was
        after = np.random.get_state()
        assert state[0] == after[0] and np.array_equal(state[1], after[1]) and state[2:] == after[2:]
