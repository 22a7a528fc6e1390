#!/usr/bin/env python3
"""Generates tests/golden/ppp_end_to_end.json: T_obs, T_sim and the p-value of ppp.protassov_test on a GPU, per mode,
as hex floats, for tests/test_ppp_golden_gpu.py to hold later versions of the host path to with ``==``.

The problem is golden_util.protassov_problem() (N = 400, five simulated light curves, 16 walkers); the modes are MODES
below.  Record it from a checkout of the commit BEFORE ppp.py got its planner -- the fixture pins the host logic against
that commit, so the recorder refuses to run on a tree whose ppp.py has ``_plan_protassov``.  Every mode runs twice and is
stored only if the two runs agree to the last bit.

Run from the repo root on a machine with an MI355X:  python tests/golden/make_ppp_end_to_end_golden.py [OUT.json]
"""
import json
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

from golden_util import protassov_problem  # noqa: E402
from mind_the_gaps_amd import ppp  # noqa: E402

MODES = {
    "defaults": {},
    "refits_sequential": {"concurrent_refits": False},
    "refits_side_by_side": {"concurrent_refits": True},
    "refits_unpaired": {"concurrent_refits": "unpaired"},
    "reproducible": {"reproducible": True},
    "odd_walkers": {"walkers": 15, "sim_walkers": 16},
}


def run(mode):
    lc, null, alt, common = protassov_problem()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = ppp.protassov_test(lc, null, alt, **dict(common, **MODES[mode]))
    return {"T_obs": float(res["T_obs"]).hex(), "T_sim": [float(v).hex() for v in res["T_sim"]],
            "p_value": float(res["p_value"]).hex()}


def main():
    if hasattr(ppp, "_plan_protassov"):
        raise SystemExit("this tree's ppp.py already has the planner: record the fixture from the commit before it")
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "ppp_end_to_end.json")
    modes = {}
    for mode in MODES:
        first, second = run(mode), run(mode)
        if first != second:
            raise SystemExit("mode %r: two runs of the same commit differ, nothing stored\n%r\n%r" % (mode, first, second))
        assert all(np.isfinite(float.fromhex(v)) for v in first["T_sim"])
        modes[mode] = {"kwargs": MODES[mode], **first}
        print(mode, first, flush=True)
    what = ("ppp.protassov_test on golden_util.protassov_problem(), per mode; hex floats; every mode ran twice with equal "
            "results (tests/golden/make_ppp_end_to_end_golden.py)")
    with open(out, "w") as fh:      # one mode per line
        fh.write('{"what": %s,\n "modes": {\n%s\n }}\n'
                 % (json.dumps(what), ",\n".join("  %s: %s" % (json.dumps(m), json.dumps(v)) for m, v in modes.items())))


if __name__ == "__main__":
    main()
