"""The Lomb-Scargle entries against the bits of the commit before the tile sweep was written once for one term and K
harmonics (csrc/mtg_ls_tile.h): tests/golden/lomb_scargle_parent_bits.npz, made on an MI355X by
tests/golden/make_lomb_scargle_parent_bits.py from the build of the commit it names.

The shapes are that file's: the smallest that reach every branch of the shared sweep -- a full chunk and a ragged one and
the smallest N of every K; tiles of one light curve, partly filled, full and ragged; both samplings; the 128- and 256-wide
launches with idle lanes; K = 1, 2, 3, 5 and both weightings; the four normalisations; peaks with every call; entries that
are NaN; and the envelope's reductions.  The same calls are made again here on the same inputs, drawn from the same seed,
and every output must be the stored 64-bit pattern.  (Slabs that start above row 0 are held bit for bit to the light curve
alone by tests/test_lomb_scargle_edges_gpu.py and tests/test_lomb_scargle_multi_gpu.py.)  The file takes about a second.
"""
import importlib.util
import os

import numpy as np
import pytest

from mind_the_gaps_amd.engine import Engine

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_lomb_scargle_parent_bits",
                                               os.path.join(HERE, "golden", "make_lomb_scargle_parent_bits.py"))
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
