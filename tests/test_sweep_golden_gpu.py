"""The serial sweep -- the one-lane kernels mtg_solve_kernel, mtg_solve_kernel_multi and mtg_white_kernel, and their
two-wave pipeline mtg_pipe_kernel -- gives, bit for bit, what it gave before the sample loads and
the epilogue were written once for all of them (csrc/mtg_sweep_step.h): every lnL and every status of
tests/golden/sweep_golden.npz (recorded on an MI355X by tests/golden/make_sweep_golden.py, whose docstring says at which
commit, on which shapes and why those), compared with np.array_equal on the raw bits.

A case is (model, N): seven models, N in {1, 2, 3, 64, 65, 70, 257, 261}, 130 rows, each once with the pipeline off
and once with it forced; a few milliseconds each.
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import make_sweep_golden as G  # noqa: E402

GOLDEN = np.load(os.path.join(HERE, "golden", "sweep_golden.npz"))


def test_the_golden_holds_every_case():
    want = {"%s/%d/%s/%s" % (name, N, dispatch, what) for name in G.MODELS for N in G.LENGTHS for dispatch, _ in G.DISPATCH
            for what in ("lnL", "status")}
    assert set(GOLDEN.files) == want
    for name in G.MODELS:                    # the rows the shapes were chosen for are really there
        st = GOLDEN["%s/261/one_lane/status" % name]
        assert (st == 1).sum() == (0 if name in (G.MODELS[4], G.MODELS[6]) else 4)
        assert list(np.flatnonzero(st == 2)) == (list(G.NOTPD_ROWS) if name == G.MODELS[6] else [])
        assert (st == 0).sum() == G.B - (st == 1).sum() - (st == 2).sum()


@pytest.mark.parametrize("N", G.LENGTHS)
@pytest.mark.parametrize("name", G.MODELS)
def test_bit_for_bit(engine, name, N):
    got, solver = G.run(engine, name, N)
    assert G.dispatch_is_as_meant(name, N, solver), solver
    prefix = "%s/%d/" % (name, N)
    assert sorted(got) == sorted(k for k in GOLDEN.files if k.startswith(prefix))
    for key in sorted(got):
        assert got[key].dtype == GOLDEN[key].dtype and got[key].shape == GOLDEN[key].shape, key
        bits = (lambda a: a.view(np.int64)) if key.endswith("lnL") else (lambda a: a)
        assert np.array_equal(bits(got[key]), bits(GOLDEN[key])), \
            "%s: %d of %d values differ" % (key, int(np.sum(bits(got[key]) != bits(GOLDEN[key]))), got[key].size)
