"""mtg_lag_sums and mtg_cross_sums against the bits of the commit before their planner, launch validation and host code were
written once for both (csrc/mtg_lag_plan.h, mtg_capi.hip): tests/golden/lag_sweep_parent_bits.npz, made on an MI355X by
tests/golden/make_lag_sweep_parent_bits.py from the build of the commit it names.

The shapes are that file's: the smallest that reach every branch of the two sweeps and their reductions -- four row blocks with idle lanes,
a row block that is, just misses and just exceeds a chunk, the smallest N of each entry; companions of three chunks, of one
and two chunks and of one sample; tiles of one light curve, partly filled, full and ragged; both samplings; a companion row
for all and one per light curve; one bin and 128; late starts and early exits; rows that write only zeros; lags on an
edge; negative and sign-straddling edges; repeated time stamps; every instantiation of both kernels.  The same calls are
made again here on the same inputs, drawn from the same seed, and every output must be the stored 64-bit pattern.  (Slabs
that start above row 0 are held bit for bit to the light curve alone by test_more_than_one_slab of tests/test_lag_gpu.py
and tests/test_cross_gpu.py.)  The file takes about a second.
"""
import importlib.util
import os

import numpy as np
import pytest

from mind_the_gaps_amd.engine import Engine

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_lag_sweep_parent_bits", os.path.join(HERE, "golden", "make_lag_sweep_parent_bits.py"))
maker = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(maker)
FIX = np.load(maker.FIXTURE)


def test_the_inputs_are_the_fixtures():
    inp = maker.draw_inputs()
    assert set(inp) == set(maker.INPUTS)
    for name in maker.INPUTS:
        assert np.array_equal(inp[name].view(np.uint64), FIX[name].view(np.uint64)), name
    assert len(str(FIX["commit"])) == 40


def test_every_output_is_the_parents_bit_for_bit():
    eng = Engine(0)
    try:
        calls = maker.run(eng, {name: FIX[name] for name in maker.INPUTS})
    finally:
        eng.close()
    assert [name for name, _, _ in calls] == [str(n) for n in FIX["names"]]
    assert [solver for _, solver, _ in calls] == [str(s) for s in FIX["solvers"]]
    assert [len(b) for _, _, b in calls] == [int(n) for n in FIX["sizes"]]
    # every instantiation of both sweeps
    assert {solver for _, solver, _ in calls} == ({"mtg_lag_kernel<%d,%d>" % (r, a) for r in (1, 4, 8) for a in (0, 1)} |
                                                  {"mtg_cross_kernel<%d,%d,%d>" % (r, p, a) for r in (1, 4, 8) for p in (0, 1) for a in (0, 1)})
    ends = np.cumsum(FIX["sizes"])
    differing = []
    for (name, _, got), end, size in zip(calls, ends, FIX["sizes"]):
        want = FIX["bits"][end - size:end]
        assert got.dtype == want.dtype == np.uint64
        if not np.array_equal(got, want):
            differing.append("%s: %d of %d words" % (name, int(np.sum(got != want)), len(want)))
    print("\n%d calls, %d words against commit %s" % (len(calls), int(ends[-1]), str(FIX["commit"])[:7]))
    assert not differing, differing
