"""mtg_wwz against the bits of the commit before its chunk walk was written on the pieces of csrc/mtg_ls_tile.h (the lane's
location, the staging of a chunk with a column rule, the per-sample read): tests/golden/wwz_tile_parent_bits.npz, made on
an MI355X by tests/golden/make_wwz_tile_parent_bits.py from the build of the commit it names, recorded twice and equal.

The shapes are that file's, the smallest that reach what tests/golden/resident_calls_parent_bits.npz leaves out: full
tiles and a second and third tile (L = 9 shared: 4 + 4 + 1 weighted, 8 + 1 unweighted), a light curve per lane on
samplings of their own (t_stride = N), three chunks of which the last is ragged (N = 700), a second frequency block with
252 idle lanes (F = 260), and centres and frequencies at which a workgroup keeps all three chunks, only the first, only
the second and only the third.  The maker's host check of those chunk ranges is repeated here; then the same calls are
made on the same inputs and every output must be the stored 64-bit pattern.

Slabs that start above light curve 0 (l0 > 0) need L T F > 2^25 entries, which no fixture of this size can hold: they
stay with test_more_than_one_slab of tests/test_wwz_gpu.py, at its tolerance.  The file takes about two seconds.
"""
import importlib.util
import os

import numpy as np
import pytest

from mind_the_gaps_amd.engine import Engine

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_wwz_tile_parent_bits", os.path.join(HERE, "golden", "make_wwz_tile_parent_bits.py"))
maker = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(maker)
FIX = np.load(maker.FIXTURE)


def test_the_inputs_are_the_fixtures_and_reach_every_chunk_range():
    inp = maker.draw_inputs()
    assert set(inp) == set(maker.INPUTS)
    for name in maker.INPUTS:
        assert np.array_equal(inp[name].view(np.uint64), FIX[name].view(np.uint64)), name
    assert len(str(FIX["commit"])) == 40
    ranges, least = maker.check_grid({name: FIX[name] for name in maker.INPUTS})
    assert set(ranges.values()) == {(0, 3), (0, 1), (1, 2), (2, 3)}
    assert least > 0.0
    assert os.path.getsize(maker.FIXTURE) < 243 * 1024


@pytest.mark.gpu
def test_every_output_is_the_parents_bit_for_bit():
    eng = Engine(0)
    try:
        calls = maker.run(eng, {name: FIX[name] for name in maker.INPUTS})
    finally:
        eng.close()
    assert [name for name, _, _ in calls] == [str(n) for n in FIX["names"]]
    assert [solver for _, solver, _ in calls] == [str(s) for s in FIX["solvers"]]
    assert [len(b) for _, _, b in calls] == [int(n) for n in FIX["sizes"]]
    # both full tiles and the light curve per lane, every one on two frequency blocks of 256 lanes
    assert {solver for _, solver, _ in calls} == {"mtg_wwz_kernel<%s> lanes 256" % rw for rw in ("4,1", "8,0", "1,1")}
    ends = np.cumsum(FIX["sizes"])
    differing = []
    for (name, _, got), end, size in zip(calls, ends, FIX["sizes"]):
        want = FIX["bits"][end - size:end]
        assert got.dtype == want.dtype == np.uint64
        if not np.array_equal(got, want):
            differing.append("%s: %d of %d words" % (name, int(np.sum(got != want)), len(want)))
    print("\n%d calls, %d words against commit %s" % (len(calls), int(ends[-1]), str(FIX["commit"])[:7]))
    assert not differing, differing
