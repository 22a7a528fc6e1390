"""The per-row GP entries -- predict_at, predict_terms, gp_draw, whiten, gp_cond_draw, loglike_grad -- against the bits of
the commit before the new-time replay (csrc/mtg_pat_replay.h), the forward innovation step (csrc/mtg_factor_step.h) and
the transposed tile (csrc/mtg_device.h) were written once: tests/golden/gp_rows_parent_bits.npz, made on an MI355X by
tests/golden/make_gp_rows_parent_bits.py from the build of the commit it names.

The shapes are that file's: the smallest that reach every branch of the shared code -- N = 2 MTG_PAT_C + 3 (three
checkpoints and a ragged tail, four full tiles and one of 3) and N = 1, 2; B = 67 with a row outside the prior and a row
whose pivot goes non-positive; ranks 0, 1, 2, 3, 10 and an SHO batch with both dampings; both means; both samplings; 70
unsorted new times before, on, between and after the samples and the checkpoints, one twice; every call with and without
its optional outputs, with the caller's normals and with the device's.  The same calls are made again here on the same
inputs, drawn from the same seed, and every output must be the stored 64-bit pattern.  The file takes about a second.
"""
import importlib.util
import os

import numpy as np
import pytest

from mind_the_gaps_amd.engine import Engine

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_gp_rows_parent_bits", os.path.join(HERE, "golden", "make_gp_rows_parent_bits.py"))
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
    assert [name for name, _ in calls] == [str(n) for n in FIX["names"]]
    assert [len(b) for _, b in calls] == [int(n) for n in FIX["sizes"]]
    ends = np.cumsum(FIX["sizes"])
    differing = []
    for (name, got), end, size in zip(calls, ends, FIX["sizes"]):
        want = FIX["bits"][end - size:end]
        assert got.dtype == want.dtype == np.uint64
        if not np.array_equal(got, want):
            differing.append("%s: %d of %d words" % (name, int(np.sum(got != want)), len(want)))
    print("\n%d calls, %d words against commit %s" % (len(calls), int(ends[-1]), str(FIX["commit"])[:7]))
    assert not differing, differing
