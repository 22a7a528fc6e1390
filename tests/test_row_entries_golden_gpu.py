"""The per-row entries of the C-ABI -- Engine.predict, predict_at, gp_draw, apply_inverse -- give, bit for bit, what they
gave before their host prologue and their kernels' pivot step were each written once: every array and every status of
tests/golden/row_entries_golden.npz (recorded on an MI355X by tests/golden/make_row_entries_golden.py, whose docstring
says at which commit and on which shapes), compared with np.array_equal(equal_nan=True).

A case is (sampling, model): times per light curve (t_stride = N) or shared (t_stride = 0); a rank-3 model with a
linear mean, an SHO term on either side of Q = 1/2 and a row outside the prior, a white model (rank 0), five complex
terms (rank 10).  L = 2, N = 131, B <= 5, M = 7: a fraction of a second each.
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import make_row_entries_golden as G  # noqa: E402

GOLDEN = np.load(os.path.join(HERE, "golden", "row_entries_golden.npz"))


def test_the_golden_holds_every_call_of_every_case():
    calls = ["predict", "predict_at", "predict_at_mean_only", "predict_at_sorted", "gp_draw_given", "gp_draw_philox"]
    want = set()
    for fixture in G.FIXTURES:
        for name in G.MODELS:
            for call in calls + (["apply_inverse"] if name == G.MODELS[0] else []):
                outs = {"apply_inverse": ("x",), "gp_draw_given": ("y",), "gp_draw_philox": ("y",),
                        "predict_at_mean_only": ("mu",)}.get(call, ("mu", "var"))
                want |= {"%s/%s/%s/%s" % (fixture, name, call, o) for o in outs + ("status",)}
    assert set(GOLDEN.files) == want


@pytest.mark.parametrize("name", G.MODELS)
@pytest.mark.parametrize("fixture", G.FIXTURES)
def test_bit_for_bit(engine, fixture, name):
    got = G.run(engine, fixture, name)
    prefix = "%s/%s/" % (fixture, name)
    assert sorted(got) == sorted(k for k in GOLDEN.files if k.startswith(prefix))
    for key in sorted(got):
        assert got[key].dtype == GOLDEN[key].dtype and got[key].shape == GOLDEN[key].shape, key
        assert np.array_equal(got[key], GOLDEN[key], equal_nan=True), \
            "%s: %d of %d values differ" % (key, int(np.sum(~((got[key] == GOLDEN[key]) | (np.isnan(got[key]) & np.isnan(GOLDEN[key]))))), got[key].size)
    if name == G.MODELS[0]:   # the cases the shapes were chosen for are really there
        assert list(got[prefix + "predict/status"]) == [0, 0, 0, 1, 0]
        assert np.all(np.isnan(got[prefix + "predict_at/mu"][3])) and np.all(np.isnan(got[prefix + "gp_draw_philox/y"][3]))
