"""mtg_lag_sums on the GPU (include/mtg.h): the sums over the pairs of samples in bins of the time lag.

Accuracy is held against the exact (rational) truth of tests/golden/lag_golden.npz (scripts/make_lag_golden.py), with rho
the error of tests/lag_numpy.py (plain float64) and u = 2^-53: a sum of c pairs is within
    max(10 rho, 64 sqrt(c) u) x (the sum of its terms' magnitudes)
-- the sum itself for lag, sf, cf2 and noise, sum |r_i r_j| for cf -- and count is exact.  The independence properties of
the header are bit for bit.

Measured on the MI355X: the largest ratio to the bound per sum is printed by test_counts_are_exact_and_sums_within_bounds;
the figures of the run that went with this file are in README.md.
"""
import os

import numpy as np
import pytest

import lag_numpy as ln
from mind_the_gaps_amd import engine, timedomain
from mind_the_gaps_amd.engine import Engine, EngineError

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = np.load(os.path.join(HERE, "golden", "lag_golden.npz"))
LS = np.load(os.path.join(HERE, "golden", "lomb_scargle_golden.npz"))
ALL = dict(count=True, lag=True, sf=True, cf=True, cf2=True, noise=True)
VALUES = ("lag", "sf", "cf", "cf2", "noise")


def case(name):
    return tuple(LS["%s/%s" % (name, k)] for k in ("t", "y", "dy"))


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def same(a, b):
    return set(a) == set(b) and all(np.array_equal(a[k], b[k]) for k in a)


def test_counts_are_exact_and_sums_within_bounds(eng):
    worst = {q: (0.0, None) for q in VALUES}
    empty_bins = 0
    for name in ln.CASES:
        t, y, dy = case(name)
        eng.set_lightcurves(t, y, dy)
        for tag in ln.EDGE_SETS:
            key = "%s/%s/" % (name, tag)
            got = eng.lag_sums(FIX[key + "edges"], **ALL)
            count = FIX[key + "count"]
            assert got["count"].dtype == np.int64 and got["count"].shape == (1, len(count))
            assert int(np.sum(got["count"][0] != count)) == 0, (name, tag)
            empty_bins += int(np.sum(count == 0))
            line = []
            for q in VALUES:
                assert np.all(got[q][0][count == 0] == 0.0), (name, tag, q)      # empty bins read exactly 0
                scale = np.abs(FIX[key + ("cfabs" if q == "cf" else q)])
                err = np.abs((got[q][0] - FIX[key + q]) - FIX[key + q + "_lo"])
                b = ln.bound(float(FIX[key + "rho_" + q]), count, scale)
                ratio = float(np.max(np.where(count > 0, err / np.where(b > 0, b, 1.0), 0.0)))
                line.append("%s %.3f" % (q, ratio))
                if ratio > worst[q][0]:
                    worst[q] = (ratio, (name, tag))
                # lag also within 64 sqrt(c) u alone
            lag_err = np.abs((got["lag"][0] - FIX[key + "lag"]) - FIX[key + "lag_lo"])
            assert np.all(lag_err <= 64.0 * np.sqrt(count) * ln.U * FIX[key + "lag"]), (name, tag)
            print("%-5s %-8s |x - truth| / bound: %s" % (name, tag, "  ".join(line)))
    assert "mtg_lag_kernel<1,1>" in eng.last_solver and eng.last_kernel_ms > 0
    assert empty_bins > 0
    for q in VALUES:
        print("largest ratio to the bound, %-5s: %.3f at %s" % (q, worst[q][0], worst[q][1]))
    assert all(worst[q][0] <= 1.0 for q in VALUES), worst


def test_ties_land_in_the_upper_bin(eng):
    for name in ln.CASES:
        t, y, dy = case(name)
        edges, ties = FIX[name + "/ties/edges"], FIX[name + "/ties/tie_pairs"]
        eng.set_lightcurves(t, y, dy)
        whole = eng.lag_sums(edges, count=True, lag=False, sf=False)["count"][0]
        assert np.array_equal(whole, FIX[name + "/ties/count"])
        # each edge moved up by one ulp pushes exactly the pairs that sat on it into the bin below
        for k in range(1, len(edges) - 1):
            moved = edges.copy()
            moved[k] = np.nextafter(edges[k], np.inf)
            on = int(np.sum(ties[:, 2] == k))      # (the fixture lists only pairs whose lag IS an edge)
            got = eng.lag_sums(moved, count=True, lag=False, sf=False)["count"][0]
            assert on >= 1 and got[k - 1] == whole[k - 1] + on and got[k] == whole[k] - on, (name, k)


def test_an_entry_depends_on_its_own_light_curve_and_the_edges_alone(eng):
    t, y, dy = case("n789")
    rng = np.random.default_rng(11)
    for tag in ("wide128", "log32", "short5"):
        edges = FIX["n789/%s/edges" % tag]
        eng.set_lightcurves(t[None, :], y[None, :], dy[None, :])      # alone, the sampling stored per light curve
        alone = eng.lag_sums(edges, **ALL)
        assert "mtg_lag_kernel<1,1>" in eng.last_solver
        # only sf asked for: the lighter kernel
        only = eng.lag_sums(edges, count=False, lag=False, sf=True)
        assert "mtg_lag_kernel<1,0>" in eng.last_solver and np.array_equal(only["sf"], alone["sf"]), tag
        # members 0, 6 and 10 of 11 on shared sampling: a full tile and a partly filled one
        Y = y[None, :] + 0.3 * rng.standard_normal((11, len(t)))
        DY = np.tile(dy, (11, 1)) * rng.uniform(0.5, 2.0, size=(11, 1))
        for m in (0, 6, 10):
            Y[m], DY[m] = y, dy
        eng.set_lightcurves(t, Y, DY)
        among = eng.lag_sums(edges, **ALL)
        assert "mtg_lag_kernel<8,1>" in eng.last_solver
        only = eng.lag_sums(edges, count=False, lag=False, sf=True)
        assert "mtg_lag_kernel<8,0>" in eng.last_solver and np.array_equal(only["sf"], among["sf"]), tag
        for m in (0, 6, 10):
            assert all(np.array_equal(among[q][m], alone[q][0]) for q in ln.SUMS), (tag, m)
        assert not np.array_equal(among["sf"][1], alone["sf"][0])
        # count and lag are the sampling's
        assert np.all(among["count"] == among["count"][0]) and np.all(among["lag"] == among["lag"][0])
        # a tile of four
        eng.set_lightcurves(t, Y[7:11], DY[7:11])
        four = eng.lag_sums(edges, **ALL)
        assert "mtg_lag_kernel<4,1>" in eng.last_solver and all(np.array_equal(four[q], among[q][7:11]) for q in ln.SUMS), tag


def test_more_than_one_slab(eng):
    # 128 bins x 789 rows: 27.5 MB of workspace per tile of 8 (every sum), 4.8 MB per light curve stored on its own
    # sampling, so 1 GiB holds 312 (221) light curves and L = 320 is two slabs; the second starts at a row above zero
    t, y, dy = case("n789")
    edges = FIX["n789/wide128/edges"]
    rng = np.random.default_rng(5)
    L = 320
    Y = y[None, :] + 0.3 * rng.standard_normal((L, len(t)))
    DY = np.tile(dy, (L, 1))
    for m in (0, 100, 319):
        Y[m] = y
    eng.set_lightcurves(t, y, dy)
    alone = eng.lag_sums(edges, **ALL)
    for times in (t, np.tile(t, (L, 1))):
        eng.set_lightcurves(times, Y, DY)
        got = eng.lag_sums(edges, **ALL)
        for m in (0, 100, 319):
            assert all(np.array_equal(got[q][m], alone[q][0]) for q in ln.SUMS), (np.ndim(times), m)
        assert np.all(got["count"].sum(axis=1) == len(t) * (len(t) - 1) // 2)
    # (sf alone fits one slab here: the same rows)
    assert np.array_equal(eng.lag_sums(edges, count=False, lag=False, sf=True)["sf"], got["sf"])


def test_errors_and_a_working_context_afterwards(eng):
    t, y, dy = case("n52")
    edges = FIX["n52/log32/edges"]
    fresh = Engine(0)
    try:
        with pytest.raises(EngineError) as exc:
            fresh.lag_sums(edges)
        assert exc.value.code == engine.E_STATE
        fresh.set_lightcurves(np.array([1.0]), np.array([2.0]), np.array([1.0]))
        with pytest.raises(EngineError) as exc:
            fresh.lag_sums(edges)
        assert exc.value.code == engine.E_ARG and "N = 1" in str(exc.value)
        fresh.set_lightcurves(t, y, dy)
        eng.set_lightcurves(t, y, dy)
        before = fresh.lag_sums(edges, **ALL)
        assert same(before, eng.lag_sums(edges, **ALL))
        bad = [
            (np.linspace(0.0, 1.0, 130), "nbins = 129"), ([0.0, np.nan], "edges[1]"), ([0.0, np.inf], "edges[1]"), ([-np.inf, 1.0], "edges[0]"),
            ([-1e-300, 1.0], "negative"), ([0.0, 1.0, 1.0], "edges[2]"), ([0.0, 2.0, 1.0], "edges[2]"), ([1.0, 0.5], "edges[1]"),
        ]
        for e, word in bad:
            with pytest.raises(EngineError) as exc:
                fresh.lag_sums(e)
            assert exc.value.code == engine.E_ARG and word in str(exc.value), e
            assert same(fresh.lag_sums(edges, **ALL), before)
        # Engine.lag_sums' own checks, and nbins = 0 and every output NULL straight through the C entry
        with pytest.raises(ValueError):
            fresh.lag_sums(edges, count=False, lag=False, sf=False)
        with pytest.raises(ValueError):
            fresh.lag_sums([1.0])
        lib, ctx = fresh._lib, fresh._ctx
        ep, out = engine._ptr(np.ascontiguousarray(edges)), np.zeros(32)
        assert lib.mtg_lag_sums(ctx, 0, ep, None, None, engine._ptr(out), None, None, None) == engine.E_ARG and b"nbins = 0" in lib.mtg_last_error(ctx)
        assert lib.mtg_lag_sums(ctx, 32, ep, None, None, None, None, None, None) == engine.E_ARG and b"NULL" in lib.mtg_last_error(ctx)
        assert same(fresh.lag_sums(edges, **ALL), before)
        # the other entries still run on the same context
        f = np.linspace(0.01, 0.1, 7)
        assert np.array_equal(fresh.lomb_scargle(f), eng.lomb_scargle(f))
    finally:
        fresh.close()


def test_structure_function_and_correlation_classes_on_n216():
    t, y, dy = case("n216")
    edges = timedomain.lag_bins(t, 20, spacing="log")
    want = ln.lag_sums(t, y, dy, edges)
    lag, sf2, count = timedomain.StructureFunction(t, y, dy).sf(edges)
    w_lag, w_sf2, w_count = timedomain.sf_from_sums(want)
    assert lag.shape == sf2.shape == count.shape == (20,) and np.array_equal(count, w_count)
    assert np.allclose(lag, w_lag, rtol=1e-12, equal_nan=True) and np.allclose(sf2, w_sf2, rtol=1e-10, atol=1e-12 * np.nanmax(np.abs(w_sf2)), equal_nan=True)
    raw = timedomain.StructureFunction(t, y).sf(edges)[1]
    assert np.allclose(raw, timedomain.sf_from_sums(want, False)[1], rtol=1e-12, equal_nan=True)
    assert np.allclose(timedomain.StructureFunction(t, y, dy).sf(edges, subtract_noise=False)[1], raw, rtol=0, atol=0, equal_nan=True)
    r = y - y.mean()
    for sub in (True, False):
        lag, dcf, err, count = timedomain.DiscreteCorrelation(t, y, dy).dcf(edges, subtract_noise=sub)
        _, w_dcf, w_err, _ = timedomain.dcf_from_sums(want, np.mean(r * r), np.mean(dy * dy) if sub else 0.0)
        assert np.array_equal(count, w_count) and np.allclose(dcf, w_dcf, rtol=1e-10, atol=1e-12, equal_nan=True)
        assert np.allclose(err, w_err, rtol=1e-7, equal_nan=True) and np.array_equal(np.isnan(err), count < 2)
    # a set of light curves: [L][nbins], row 0 the same bits
    many = timedomain.StructureFunction(t, np.stack([y, y[::-1], 2.0 * y]), dy).sf(edges)
    assert many[1].shape == (3, 20) and np.array_equal(many[1][0], timedomain.StructureFunction(t, y, dy).sf(edges)[1], equal_nan=True)
    # an empty bin is NaN
    empty = timedomain.StructureFunction(t, y, dy).sf([0.0, 1e-9, 1.0])
    assert empty[2][0] == 0 and np.isnan(empty[0][0]) and np.isnan(empty[1][0])


def test_lag_significance_end_to_end_and_reproducible():
    from mind_the_gaps_amd import ppp
    from mind_the_gaps_amd import synthetic as synth
    from mind_the_gaps_amd.gp import get_engine
    from mind_the_gaps_amd.lightcurves import GappyLightcurve
    from mind_the_gaps_amd.models import DampedRandomWalk
    th = synth.truth(synth.ALT_MODEL)
    times, rates, err = synth.make_lightcurves(52, 1, seed=43)
    lc = GappyLightcurve(times, rates[0] + 50.0, err[0], exposures=0.5 * np.diff(times).min())
    edges = timedomain.lag_bins(times, 6)

    def null():
        return DampedRandomWalk(th[0], th[1], bounds=[(-10, 50), (-10, 10)])
    kw = dict(nsims=8, walkers=8, max_steps=60, sigma_noise=0.5, seed=21)
    for stat in ("sf", "dcf"):
        a = ppp.lag_significance(lc, null(), edges, statistic=stat, levels=(0.9, 0.99), **kw)
        b = ppp.lag_significance(lc, null(), edges, statistic=stat, levels=(0.9, 0.99), **kw)
        for k in ("lag", "count", "observed", "median", "share_above", "share_below"):
            assert a[k].shape == (6,) and np.array_equal(a[k], b[k], equal_nan=True), (stat, k)
        for k in ("lower", "upper"):
            assert a[k].shape == (2, 6) and np.array_equal(a[k], b[k], equal_nan=True), (stat, k)
        assert a["sims"].shape == (8, 6) and np.array_equal(a["sims"], b["sims"], equal_nan=True) and a["samples"].shape[0] == 8
        # a bin without pairs is NaN throughout, every other bin a number
        ok = a["count"] > 0
        assert ok.sum() >= 3 and all(np.array_equal(np.isfinite(a[k]), ok) for k in ("observed", "median", "share_above", "share_below", "lag"))
        assert np.all(np.isfinite(a["sims"][:, ok])) and np.all(np.isnan(a["sims"][:, ~ok]))
        assert np.all(a["lower"][1, ok] <= a["lower"][0, ok]) and np.all(a["lower"][0, ok] <= a["median"][ok])
        assert np.all(a["median"][ok] <= a["upper"][0, ok]) and np.all(a["upper"][0, ok] <= a["upper"][1, ok])
        assert np.all((a["share_above"][ok] >= 0) & (a["share_above"][ok] <= 1)) and np.all(a["share_above"][ok] + a["share_below"][ok] >= 1.0)
        # the observed row is a direct call on the observed light curve
        eng = get_engine(0)
        eng.set_lightcurves(np.asarray(lc.times, dtype=np.float64), np.asarray(lc.y, dtype=np.float64), np.asarray(lc.dy, dtype=np.float64))
        eng.bound_to = None
        sums = eng.lag_sums(edges, **ALL)
        if stat == "sf":
            direct = timedomain.sf_from_sums(sums)[1][0]
        else:
            yy, dd = np.asarray(lc.y, dtype=np.float64)[None, :], np.asarray(lc.dy, dtype=np.float64)[None, :]
            direct = timedomain.dcf_from_sums(sums, np.mean((yy - yy.mean(axis=1, keepdims=True)) ** 2, axis=1), np.mean(dd ** 2, axis=1))[1][0]
        assert np.array_equal(a["observed"], direct, equal_nan=True) and np.array_equal(a["count"], sums["count"][0])
