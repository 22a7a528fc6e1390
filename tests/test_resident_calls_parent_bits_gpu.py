"""The entries that work on the resident light curves alone against the commit before their host code was put through one
call shape (mtg_capi.hip: ResidentCall): tests/golden/resident_calls_parent_bits.npz, made on an MI355X by
tests/golden/make_resident_calls_parent_bits.py from the build of the commit it names.

The shapes and the refusals are that file's.  epoch_fold, phase_fold and wwz, which no parent fixture held yet, at the
smallest shapes that reach every plan of their two sweeps -- a full and a ragged chunk, tiles of one, two and four light
curves partly filled and ragged, both samplings, 64, 128 and 256 lanes with idle ones, bins on both sides of the rule that
halves the lanes, every normalisation, statistic and combination of outputs: every output must be the stored 64-bit
pattern and mtg_last_solver the stored string.  Then, for all nine entries, every refusal the entry can make and calls
that are wrong in two ways at once: the code and the whole message must be the stored ones, and the small good call that
follows each on the same context must give the stored bits.  After every good call mtg_last_kernel_ms is finite and
positive.  (Slabs that start above row 0 are held by test_slabs_with_a_start_row_above_zero* and test_more_than_one_slab
of the entries' own files.)  Each test takes about a second.
"""
import importlib.util
import os

import numpy as np
import pytest

from mind_the_gaps_amd.engine import Engine

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_resident_calls_parent_bits", os.path.join(HERE, "golden", "make_resident_calls_parent_bits.py"))
maker = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(maker)
FIX = np.load(maker.FIXTURE)
NAMES = [str(n) for n in FIX["names"]]
FIRST_AFTER = next(i for i, n in enumerate(NAMES) if n.startswith("after "))     # run_bits' calls, then run_refusals'


def inputs():
    return {name: FIX[name] for name in maker.INPUTS}


def hold_to_the_fixture(rec, lo, hi):
    """the calls of `rec` are calls lo .. hi of the fixture: names, kernels, sizes and every word"""
    assert [name for name, _, _ in rec.calls] == NAMES[lo:hi]
    assert [solver for _, solver, _ in rec.calls] == [str(s) for s in FIX["solvers"][lo:hi]]
    assert [len(b) for _, _, b in rec.calls] == [int(n) for n in FIX["sizes"][lo:hi]]
    ends = np.cumsum(FIX["sizes"])
    differing = []
    for (name, _, got), end, size in zip(rec.calls, ends[lo:hi], FIX["sizes"][lo:hi]):
        want = FIX["bits"][end - size:end]
        assert got.dtype == want.dtype == np.uint64
        if not np.array_equal(got, want):
            differing.append("%s: %d of %d words" % (name, int(np.sum(got != want)), len(want)))
    print("\n%d calls, %d words against commit %s" % (len(rec.calls), int(sum(FIX["sizes"][lo:hi])), str(FIX["commit"])[:7]))
    assert not differing, differing
    assert len(rec.ms) == len(rec.calls)
    assert all(np.isfinite(ms) and ms > 0.0 for ms in rec.ms), [(n, ms) for (n, _, _), ms in zip(rec.calls, rec.ms) if not ms > 0.0]


def test_the_inputs_are_the_fixtures():
    inp = maker.draw_inputs()
    assert set(inp) == set(maker.INPUTS)
    for name in maker.INPUTS:
        assert np.array_equal(inp[name].view(np.uint64), FIX[name].view(np.uint64)), name
    assert len(str(FIX["commit"])) == 40


def test_epoch_fold_phase_fold_and_wwz_are_the_parents_bit_for_bit():
    eng = Engine(0)
    try:
        rec = maker.run_bits(eng, inputs())
    finally:
        eng.close()
    hold_to_the_fixture(rec, 0, FIRST_AFTER)
    kernels = {solver for _, solver, _ in rec.calls}
    # every tile and every width of the folding sweep, weighted and not; both weightings of the wavelet sweep
    folds = {k for k in kernels if k.startswith("mtg_epoch_fold_kernel")}
    assert {k.split(" lanes ")[0] for k in folds} == {"mtg_epoch_fold_kernel<%d,%d>" % (r, w) for r in (1, 2, 4) for w in (0, 1)}
    assert {k.split(" lanes ")[1] for k in folds} == {"64", "128", "256"}
    assert {k.split(",")[1][0] for k in kernels if k.startswith("mtg_wwz_kernel")} == {"0", "1"}


def test_every_refusal_is_the_parents_and_the_context_works_after_it():
    eng = Engine(0)
    try:
        refusals, rec = maker.run_refusals(eng, inputs())
    finally:
        eng.close()
    assert [name for name, _, _ in refusals] == [str(n) for n in FIX["refusal_names"]]
    wrong = [(name, code, message, int(c), str(m)) for (name, code, message), c, m in zip(refusals, FIX["refusal_codes"], FIX["refusal_messages"])
             if code != int(c) or message != str(m)]
    assert not wrong, wrong
    for entry in maker.ENTRIES:      # at least three calls that are wrong twice over, per entry
        assert sum(1 for name, _, _ in refusals if name.startswith(entry + ": ") and " + " in name) >= 3, entry
    assert len(rec.calls) == len(refusals)
    hold_to_the_fixture(rec, FIRST_AFTER, len(NAMES))
