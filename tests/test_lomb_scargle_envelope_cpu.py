"""CPU side of mtg_lomb_scargle_envelope (tests/test_lomb_scargle_envelope_gpu.py is the GPU side).

* the planner (csrc/mtg_ls_envelope_plan.h through tests/ls_envelope_plan_driver.cpp): path cut, columns per workgroup and
  slab width at their boundaries, the workspace within the budget on a grid up to 1e6 x 1e6, never a slab of width 0;
* periodogram.envelope_ranks / envelope_levels against np.quantile on random columns with ties and NaN: exactly;
* ppp.periodogram_significance's arithmetic through a stand-in engine that works on a power array in numpy;
* header, EXPORTS and argtypes agree on the new entry.
"""
import collections
import os
import re

import numpy as np
import pytest

from lomb_scargle_envelope_plan import Planner
from mind_the_gaps_amd import engine, periodogram, ppp

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def planner():
    return Planner()


def test_path_cut_and_columns_at_their_boundaries(planner):
    assert planner.lds_keys * 8 <= 160 * 1024 and planner.threads % planner.max_cols == 0
    bounds = planner.boundaries()
    assert bounds[-1] == (planner.lds_keys, "LDS path to segmented sort") and len(bounds) >= 3
    for L, what in bounds:
        lo, hi = planner.plan(L), planner.plan(L + 1)
        if what == "columns per workgroup":
            assert lo["in_lds"] == hi["in_lds"] == 1 and hi["columns"] == lo["columns"] // 2 >= 1
        else:
            assert (lo["in_lds"], hi["in_lds"]) == (1, 0) and lo["columns"] == 1 and hi["columns"] == 0
    for L in list(range(1, 70)) + [L + d for L, _ in bounds for d in (-1, 0, 1)]:
        p = planner.plan(L)
        assert p["pow2"] >= L and p["pow2"] < 2 * L and p["pow2"] & (p["pow2"] - 1) == 0
        if p["in_lds"]:
            c = p["columns"]
            assert 1 <= c <= planner.max_cols and c & (c - 1) == 0 and c * p["pow2"] <= planner.lds_keys
            assert c == planner.max_cols or 2 * c * p["pow2"] > planner.lds_keys      # as many as fit


def test_slab_width_is_within_budget_and_never_zero(planner):
    sizes = [1, 2, 11, 1000, 16384, 16385, 10 ** 5, 10 ** 6]
    cases = [(L, F, Q) for L in sizes for F in sizes for Q in (0, 5, L)]
    for (L, F, Q), p in zip(cases, planner.plans(cases)):
        per_column = 8 * ((1 if p["in_lds"] else 3) * L + Q)
        assert 1 <= p["width"] <= F, (L, F, Q, p)
        assert p["workspace"] == p["width"] * per_column <= planner.budget, (L, F, Q, p)
        # as wide as the budget allows
        assert p["width"] == F or (p["width"] + 1) * per_column > planner.budget, (L, F, Q, p)
    # a budget smaller than one column: one column at a time, the one case over the budget
    assert planner.plan(1000, 50, 3, budget=100)["width"] == 1
    # the exact edge
    assert planner.plan(4, 100, 0, budget=32 * 7)["width"] == 7 and planner.plan(4, 100, 0, budget=32 * 7 - 1)["width"] == 6


def columns_with_ties_and_nan(rng, L, F):
    power = rng.integers(0, 6, size=(L, F)).astype(np.float64) / 4.0 + rng.choice([0.0, 1e-3], size=(L, F))
    power[rng.random((L, F)) < 0.1] = np.nan
    power[:, 0] = np.abs(rng.standard_normal(L))      # a column without NaN or ties
    if F > 1:
        power[:, 1] = np.nan
    return power


@pytest.mark.parametrize("L", [1, 2, 3, 16, 100, 1001])
def test_levels_are_numpys_quantiles_exactly(L):
    rng = np.random.default_rng(L)
    levels = (0.0, 0.5, 0.95, 0.997, 1.0, 1.0 / 3.0, 0.25)
    ranks = periodogram.envelope_ranks(L, levels)
    assert ranks.dtype == np.int64 and np.all(np.diff(ranks) > 0) and ranks[0] >= 0 and ranks[-1] == L - 1
    for F in (1, 9):
        power = columns_with_ties_and_nan(rng, L, F)
        got = periodogram.envelope_levels(np.sort(power, axis=0)[ranks], ranks, L, levels)
        assert np.array_equal(got, np.quantile(power, levels, axis=0), equal_nan=True)
    # ranks in another order, with duplicates and extras
    more = np.concatenate([ranks[::-1], ranks[:1], [0]])
    power = columns_with_ties_and_nan(rng, L, 5)
    assert np.array_equal(periodogram.envelope_levels(np.sort(power, axis=0)[more], more, L, levels),
                          np.quantile(power, levels, axis=0), equal_nan=True)


def test_level_helpers_refuse_what_they_cannot_do():
    with pytest.raises(ValueError):
        periodogram.envelope_ranks(10, (1.5,))
    with pytest.raises(ValueError):
        periodogram.envelope_ranks(0, (0.5,))
    with pytest.raises(ValueError, match="ranks lack"):
        periodogram.envelope_levels(np.zeros((1, 3)), [9], 10, (0.5,))


Envelope = collections.namedtuple("Envelope", "order_stat valid exceed peak_ratio peak_ratio_index")


class FakeEngine:
    """Engine.lomb_scargle_envelope in numpy on a given power array [L][F]; records what it was asked."""

    def __init__(self, power):
        self.power, self.calls = power, []

    def lomb_scargle_envelope(self, freqs, ranks=(), reference=None, scale=None, normalization="standard", weighted=True):
        self.calls.append(dict(F=len(freqs), ranks=list(map(int, ranks)), reference=reference is not None, scale=scale is not None,
                               normalization=normalization, weighted=weighted))
        p = self.power
        order_stat = np.sort(p, axis=0)[np.asarray(ranks, dtype=int)] if len(ranks) else None
        exceed = None if reference is None else np.sum(p >= reference, axis=0)
        pk = ix = None
        if scale is not None:
            assert np.all(np.isfinite(scale) & (scale > 0))
            ratio = np.where(np.isnan(p), -np.inf, p / scale)
            ix = ratio.argmax(axis=1)
            pk = (p / scale)[np.arange(len(p)), ix]
        return Envelope(order_stat, None, exceed, pk, ix)


def test_significance_arithmetic_through_a_fake_engine():
    rng = np.random.default_rng(5)
    L, F = 40, 17
    freqs = np.linspace(0.01, 1.0, F)
    power = rng.exponential(size=(L, F)) / freqs       # red: the raw maximum sits at the lowest frequency
    observed = rng.exponential(size=F) / freqs
    observed[11] *= 12.0                               # a line on the falling part of the spectrum
    eng = FakeEngine(power)
    levels = (0.95, 0.997)
    res = ppp._significance_of_resident_set(eng, observed, freqs, L, levels, "psd", False)
    q = np.quantile(power, (0.5,) + levels, axis=0)
    assert np.array_equal(res["median"], q[0]) and np.array_equal(res["levels"], q[1:])
    assert np.array_equal(res["local_p"], (1.0 + np.sum(power >= observed, axis=0)) / (1.0 + L))
    ratio = power / q[0]
    assert np.array_equal(res["sim_ratio_peaks"], ratio.max(axis=1))
    assert res["observed_ratio_peak"] == (observed / q[0]).max() and res["observed_frequency"] == freqs[11]
    assert res["global_p"] == (1.0 + np.sum(ratio.max(axis=1) >= res["observed_ratio_peak"])) / (1.0 + L)
    assert res["observed_power"] is observed
    # two calls: the ranks of the median and the levels with the reference, then the scale alone
    assert [c["reference"] for c in eng.calls] == [True, False] and [c["scale"] for c in eng.calls] == [False, True]
    assert eng.calls[0]["ranks"] == list(periodogram.envelope_ranks(L, (0.5,) + levels)) and eng.calls[1]["ranks"] == []
    assert all(c["normalization"] == "psd" and c["weighted"] is False and c["F"] == F for c in eng.calls)


def test_significance_names_the_frequency_of_a_bad_median():
    rng = np.random.default_rng(6)
    freqs = np.linspace(0.1, 1.0, 5)
    power = rng.exponential(size=(9, 5))
    for bad in (np.nan, 0.0):
        p = power.copy()
        p[:, 3] = bad
        eng = FakeEngine(p)
        with pytest.raises(ValueError, match=r"frequencies\[3\] = 0.775"):
            ppp._significance_of_resident_set(eng, np.ones(5), freqs, 9, (0.95,), "standard", True)
        assert len(eng.calls) == 1          # the scale never reached the engine
    with pytest.raises(ValueError, match=r"observed power at frequencies\[2\]"):
        ppp._significance_of_resident_set(FakeEngine(power), np.array([1, 1, np.nan, 1, 1.0]), freqs, 9, (0.95,), "standard", True)


def test_entry_is_declared_exported_and_bound():
    text = open(os.path.join(os.path.dirname(HERE), "include", "mtg.h")).read()
    decl = re.search(r"MTG_API\s+int\s+mtg_lomb_scargle_envelope\s*\(([^;]*)\)\s*;", text)
    params = re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).split(",")
    assert "mtg_lomb_scargle_envelope" in engine.EXPORTS
    lib = engine.load_library()
    assert len(lib.mtg_lomb_scargle_envelope.argtypes) == len(params) == 14
    assert callable(engine.Engine.lomb_scargle_envelope) and callable(ppp.periodogram_significance)
    assert "periodogram_significance" in ppp.__all__ and "envelope_levels" in periodogram.__all__
    # no context: an argument error, nothing touched
    assert lib.mtg_lomb_scargle_envelope(None, 1, None, 0, 1, 0, None, None, None, None, None, None, None, None) == engine.E_ARG
