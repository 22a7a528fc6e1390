#!/usr/bin/env python3
"""Generates tests/golden/solve_dispatch.json (committed fixture): the kernel mtg_last_solver names for a grid of
(model, N, batch, light curves, modes) that takes every branch of the solve dispatch (csrc/mtg_solve_plan.h) on both
sides of its crossovers -- the rank-10 path, the fused and per-structure time-parallel kernels, the pipelined sweep,
the one-launch multi-structure sweep and the per-structure sweep, sorted or not, windowed or not.  One call per case;
tests/test_solve_dispatch_gpu.py replays them and requires the same names character for character.  The paired
pipeline's name depends on timing and is left to the pair tests.

Run on an MI355X from the repo root:  python tests/golden/make_solve_dispatch_golden.py [output.json]
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from golden_util import dispatch_case  # noqa: E402
from mind_the_gaps_amd import synthetic as K  # noqa: E402

MODELS = {
    "white": [K.K_JITTER],                                      # J = 0
    "drw": [K.K_DRW],                                           # J = 1
    "drw_lor": [K.K_DRW, K.K_LORENTZIAN],                       # J = 3, (1, 1), last complex term b = 0
    "real_c4": [K.K_REAL, K.K_COMPLEX4],                        # J = 3, a free b
    "drw_bpl": [K.K_DRW, K.K_BPL],                              # J = 3, a free b
    "null": K.NULL_MODEL,                                       # J = 3, two structures
    "alt": K.ALT_MODEL,                                         # J = 5, two structures, last complex term b = 0
    "drw_c3_c4": [K.K_DRW, K.K_COMPLEX3, K.K_COMPLEX4],         # J = 5, one structure
    "rank6": [K.K_DRW, K.K_COMPLEX4, K.K_COMPLEX3, K.K_REAL],   # J = 6, one structure
    "rank6_sho": [K.K_DRW, K.K_REAL, K.K_SHO, K.K_SHO],         # J = 6, three structures
    "five_sho": [K.K_SHO] * 5,                                  # J = 10, six structures
}


def grid(P):
    """(model, N, B, overrides); P = the pipelined sweep's automatic limit (MTG_PIPE_ROWS_PER_CU x compute units).
    Defaults: L = 4, light-curve index in random order, modes 2 / 2 / 2, with the prior."""
    W = 2 * 256 * 16   # a window of two light curves of 256 samples: the left-over second launch
    return [
        ("drw", 256, 4096, {}), ("drw", 255, 256, {}), ("drw", 4096, 12288, {}), ("drw", 4096, 12289, {}),
        ("drw", 4096, 512, {}), ("drw", 4096, 513, {}),
        ("white", 4096, 256, {}),
        ("drw_lor", 4096, 12288, {}), ("drw_lor", 4096, 12289, {}), ("drw_lor", 256, 4097, {}),
        ("drw_lor", 256, P, {}), ("drw_lor", 256, P + 1, {}), ("drw_lor", 255, 4097, {}), ("drw_lor", 255, 4097, {"pipe": 1}),
        ("drw_lor", 4096, 256, {"tp": 0}), ("drw_lor", 4096, 256, {"tp": 0, "pipe": 0}),
        ("drw_lor", 256, 20000, {"tp": 1}), ("drw_lor", 4096, 256, {"tp": 3}), ("drw_lor", 4096, 20000, {"L": 1}),
        ("drw_lor", 256, 40000, {"sort": 0}), ("drw_lor", 256, 40000, {"sort": 1, "lc": "grouped"}),
        ("drw_lor", 256, 5000, {"window": W}),
        ("null", 4096, 512, {}), ("null", 4096, 513, {}), ("null", 4096, 12289, {}), ("null", 4096, 12289, {"sort": 0}),
        ("null", 256, P + 1, {}), ("null", 256, 5000, {"pipe": 0}), ("null", 4096, 64, {"tp": 0}),
        ("null", 4096, 65, {"tp": 0}), ("null", 4096, 65, {"tp": 0, "lc": "none"}),
        ("null", 256, 5000, {"pipe": 0, "window": W}), ("null", 256, 300, {"tp": 0, "L": 1}),
        ("alt", 4096, 256, {}), ("alt", 4096, 257, {}), ("alt", 4096, 513, {}), ("alt", 4096, 8192, {}),
        ("alt", 4096, 8193, {}), ("alt", 256, 4097, {}), ("alt", 4096, 256, {"tp": 3}),
        ("alt", 4096, 256, {"tp": 0, "sort": 0}),
        ("drw_c3_c4", 4096, 256, {}), ("drw_c3_c4", 4096, 257, {}), ("drw_c3_c4", 4096, 8193, {}),
        ("rank6", 4096, 256, {}), ("rank6", 4096, 8193, {}),
        ("rank6_sho", 4096, 256, {}), ("rank6_sho", 4096, 300, {}), ("rank6_sho", 4096, 8193, {}),
        ("five_sho", 1024, 64, {"L": 2}), ("five_sho", 1023, 64, {"L": 2}), ("five_sho", 1024, 8192, {"L": 2}),
        ("five_sho", 1024, 8193, {"L": 2}), ("five_sho", 1024, 64, {"L": 2, "tp": 3}), ("five_sho", 2048, 16, {"L": 1}),
        ("real_c4", 4096, 256, {"add_prior": False}), ("real_c4", 4096, 256, {}),
        ("drw_bpl", 4096, 256, {"add_prior": False, "pipe": 0}),
    ]


def main():
    import torch
    from mind_the_gaps_amd.engine import Engine
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "solve_dispatch.json")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    eng = Engine(0)
    cases = []
    for model, N, B, over in grid(128 * cus):
        cases.append(dict({"op": "loglike", "model": model, "kinds": [int(k) for k in MODELS[model]], "N": N, "L": 4,
                           "B": B, "lc": "random", "tp": 2, "pipe": 2, "sort": 2, "add_prior": True}, **over))
    for jr, jc in ((1, 1), (0, 0)):
        cases.append({"op": "coeffs", "jr": jr, "jc": jc, "N": 256, "L": 2, "B": 100, "lc": "random",
                      "tp": 2, "pipe": 2, "sort": 2})
    for case in cases:
        case["solver"] = dispatch_case(eng, case)
        print(case, flush=True)
    eng.close()
    with open(out, "w") as fh:
        json.dump({"generator": "tests/golden/make_solve_dispatch_golden.py", "compute_units": cus, "cases": cases},
                  fh, indent=1)
    print("wrote %d cases" % len(cases))


if __name__ == "__main__":
    main()
