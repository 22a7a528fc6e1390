"""mtg_cross_sums on the GPU (include/mtg.h): the sums over the pairs (resident sample, companion sample) of two series on
different samplings in bins of the signed time lag.

Accuracy is held against the exact (rational) truth of tests/golden/cross_golden.npz (scripts/make_cross_golden.py), with
rho the error of tests/cross_numpy.py (plain float64) and u = 2^-53: a sum of c pairs is within
    max(10 rho, 64 sqrt(c) u) x (the sum of its terms' magnitudes)
-- sum |tau| for lag, sum |r_i s_j| for cf, sum |r_i| and sum |s_j| for sa and sb, the sum itself for cf2, saa and sbb --
and count is exact.  The independence properties of the header and the agreement with mtg_lag_sums are bit for bit.

Measured on the MI355X: the largest ratio to the bound per sum is printed by test_counts_are_exact_and_sums_within_bounds;
the figures of the run that went with this file are in README.md.
"""
import os

import numpy as np
import pytest

import cross_numpy as cn
from mind_the_gaps_amd import engine, timedomain
from mind_the_gaps_amd.engine import Engine, EngineError

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = np.load(os.path.join(HERE, "golden", "cross_golden.npz"))
LAGFIX = np.load(os.path.join(HERE, "golden", "lag_golden.npz"))
LS = np.load(os.path.join(HERE, "golden", "lomb_scargle_golden.npz"))
ALL = {k: True for k in cn.SUMS}
LIGHT = dict(count=True, lag=True, cf=True, cf2=True)


def case(name):
    return tuple(LS["%s/%s" % (name, k)] for k in ("t", "y", "dy")) + (FIX[name + "/t2"], FIX[name + "/y2"])


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def same(a, b):
    return set(a) == set(b) and all(np.array_equal(a[k], b[k]) for k in a)


def test_counts_are_exact_and_sums_within_bounds(eng):
    worst = {q: (0.0, None) for q in cn.VALUES}
    empty_bins = 0
    for name in cn.CASES:
        t, y, dy, t2, y2 = case(name)
        eng.set_lightcurves(t, y, dy)
        for tag in cn.EDGE_SETS:
            key = "%s/%s/" % (name, tag)
            got = eng.cross_sums(t2, y2, FIX[key + "edges"], **ALL)
            count = FIX[key + "count"]
            assert got["count"].dtype == np.int64 and got["count"].shape == (1, len(count))
            assert int(np.sum(got["count"][0] != count)) == 0, (name, tag)
            empty_bins += int(np.sum(count == 0))
            line = []
            for q in cn.VALUES:
                assert np.all(got[q][0][count == 0] == 0.0), (name, tag, q)      # empty bins read exactly 0
                scale = np.abs(FIX[key + cn.SCALE[q]])
                err = np.abs((got[q][0] - FIX[key + q]) - FIX[key + q + "_lo"])
                b = cn.bound(float(FIX[key + "rho_" + q]), count, scale)
                ratio = float(np.max(np.where(count > 0, err / np.where(b > 0, b, 1.0), 0.0)))
                assert np.all(err[(count > 0) & (b == 0)] == 0.0), (name, tag, q)
                line.append("%s %.3f" % (q, ratio))
                if ratio > worst[q][0]:
                    worst[q] = (ratio, (name, tag))
            print("%-5s %-9s |x - truth| / bound: %s" % (name, tag, "  ".join(line)))
    assert "mtg_cross_kernel<1,0,1>" in eng.last_solver and eng.last_kernel_ms > 0
    assert empty_bins > 0
    for q in cn.VALUES:
        print("largest ratio to the bound, %-4s: %.3f at %s" % (q, worst[q][0], worst[q][1]))
    assert all(worst[q][0] <= 1.0 for q in cn.VALUES), worst


def test_ties_land_in_the_upper_bin(eng):
    for name in cn.CASES:
        t, y, dy, t2, y2 = case(name)
        edges, ties = FIX[name + "/ties/edges"], FIX[name + "/ties/tie_pairs"]
        eng.set_lightcurves(t, y, dy)
        whole = eng.cross_sums(t2, y2, edges, count=True, lag=False, cf=False)["count"][0]
        assert np.array_equal(whole, FIX[name + "/ties/count"]) and 0.0 in edges
        # each edge moved up by one ulp pushes exactly the pairs that sat on it into the bin below
        for k in range(1, len(edges) - 1):
            moved = edges.copy()
            moved[k] = np.nextafter(edges[k], np.inf)
            on = int(np.sum(ties[:, 2] == k))      # (the fixture lists only pairs whose lag IS an edge)
            got = eng.cross_sums(t2, y2, moved, count=True, lag=False, cf=False)["count"][0]
            assert on >= 1 and got[k - 1] == whole[k - 1] + on and got[k] == whole[k] - on, (name, k)


@pytest.mark.parametrize("name", cn.CASES)
def test_the_series_against_itself_is_lag_sums_bit_for_bit(eng, name):
    t, y, dy = case(name)[:3]
    eng.set_lightcurves(t, y, dy)
    checked = 0
    for tag in [str(s) for s in LAGFIX["edge_sets"]]:
        edges = LAGFIX["%s/%s/edges" % (name, tag)]
        if not edges[0] > 0:
            continue
        want = eng.lag_sums(edges, count=True, lag=True, sf=False, cf=True, cf2=True)
        got = eng.cross_sums(t, y, edges, **LIGHT)
        assert same(got, want), tag
        full = eng.cross_sums(t, y, edges, **ALL)
        assert all(np.array_equal(full[q], want[q]) for q in want), tag
        checked += 1
    assert checked >= 2


def test_an_entry_depends_on_its_own_pair_of_series_and_the_edges_alone(eng):
    t, y, dy, t2, y2 = case("n789")
    rng = np.random.default_rng(11)
    for tag in ("wide128", "sym8", "short5"):
        edges = FIX["n789/%s/edges" % tag]
        eng.set_lightcurves(t[None, :], y[None, :], dy[None, :])      # alone, the sampling stored per light curve
        alone = eng.cross_sums(t2, y2, edges, **ALL)
        assert "mtg_cross_kernel<1,0,1>" in eng.last_solver
        # no local moment asked for: the lighter kernel; and fewer outputs from either
        light = eng.cross_sums(t2, y2, edges, **LIGHT)
        assert "mtg_cross_kernel<1,0,0>" in eng.last_solver and all(np.array_equal(light[q], alone[q]) for q in LIGHT), tag
        assert np.array_equal(eng.cross_sums(t2, y2, edges, count=False, lag=False, cf=False, saa=True)["saa"], alone["saa"])
        assert np.array_equal(eng.cross_sums(t2, y2[None, :], edges, **ALL)["sb"], alone["sb"])       # [1][M]
        # members 0, 6 and 10 of 11 on shared sampling: a full tile and a partly filled one
        Y = y[None, :] + 0.3 * rng.standard_normal((11, len(t)))
        Y2 = y2[None, :] + 0.3 * rng.standard_normal((11, len(t2)))
        for m in (0, 6, 10):
            Y[m], Y2[m] = y, y2
        eng.set_lightcurves(t, Y, np.tile(dy, (11, 1)))
        among = eng.cross_sums(t2, y2, edges, **ALL)                  # one companion for all
        assert "mtg_cross_kernel<8,0,1>" in eng.last_solver
        light = eng.cross_sums(t2, y2, edges, **LIGHT)
        assert "mtg_cross_kernel<8,0,0>" in eng.last_solver and all(np.array_equal(light[q], among[q]) for q in LIGHT), tag
        repeated = eng.cross_sums(t2, np.tile(y2, (11, 1)), edges, **ALL)   # L2 == L with repeated rows
        assert "mtg_cross_kernel<8,1,1>" in eng.last_solver and same(repeated, among), tag
        per = eng.cross_sums(t2, Y2, edges, **ALL)                    # a companion row per light curve
        light = eng.cross_sums(t2, Y2, edges, **LIGHT)
        assert "mtg_cross_kernel<8,1,0>" in eng.last_solver and all(np.array_equal(light[q], per[q]) for q in LIGHT), tag
        for m in (0, 6, 10):
            assert all(np.array_equal(among[q][m], alone[q][0]) for q in cn.SUMS), (tag, m)
            assert all(np.array_equal(per[q][m], alone[q][0]) for q in cn.SUMS), (tag, m)
        assert not np.array_equal(among["cf"][1], alone["cf"][0]) and not np.array_equal(per["sb"][1], alone["sb"][0])
        # count, lag and, with one companion, sb and sbb are the samplings'
        assert all(np.all(among[q] == among[q][0]) for q in ("count", "lag", "sb", "sbb"))
        # a tile of four
        eng.set_lightcurves(t, Y[7:11], np.tile(dy, (4, 1)))
        four = eng.cross_sums(t2, Y2[7:11], edges, **ALL)
        assert "mtg_cross_kernel<4,1,1>" in eng.last_solver and all(np.array_equal(four[q], per[q][7:11]) for q in cn.SUMS), tag
        four = eng.cross_sums(t2, y2, edges, **ALL)
        assert "mtg_cross_kernel<4,0,1>" in eng.last_solver and all(np.array_equal(four[q], among[q][7:11]) for q in cn.SUMS), tag


def test_more_than_one_slab(eng):
    # 128 bins x 789 rows, every sum: (4 x 8 + 2) arrays of 808 kB per tile of 8, 6 per light curve stored on its own
    # sampling, so 1 GiB holds 312 (221) light curves: L = 313 is the smallest set the planner splits on shared sampling,
    # and the second slab starts at a row above zero either way (tests/test_cross_cpu.py holds these figures to the planner)
    t, y, dy, t2, y2 = case("n789")
    edges = FIX["n789/wide128/edges"]
    rng = np.random.default_rng(5)
    L = 313
    Y = y[None, :] + 0.3 * rng.standard_normal((L, len(t)))
    Y2 = y2[None, :] + 0.3 * rng.standard_normal((L, len(t2)))
    DY = np.tile(dy, (L, 1))
    for m in (0, 100, 312):
        Y[m], Y2[m] = y, y2
    eng.set_lightcurves(t, y, dy)
    alone = eng.cross_sums(t2, y2, edges, **ALL)
    for times in (t, np.tile(t, (L, 1))):
        eng.set_lightcurves(times, Y, DY)
        for companion in (y2, Y2):
            got = eng.cross_sums(t2, companion, edges, **ALL)
            for m in (0, 100, 312):
                assert all(np.array_equal(got[q][m], alone[q][0]) for q in cn.SUMS), (np.ndim(times), np.ndim(companion), m)
            assert np.all(got["count"].sum(axis=1) == len(t) * len(t2))
    # (the light variant fits one slab here: the same rows)
    light = eng.cross_sums(t2, Y2, edges, **LIGHT)
    assert all(np.array_equal(light[q], got[q]) for q in LIGHT)


@pytest.mark.parametrize("name", cn.CASES)
def test_swapping_the_series_reverses_the_counts(eng, name):
    t, y, dy, t2, y2 = case(name)
    tau = cn.pairs(t, t2)[2]
    without_ties = 0
    for tag in cn.EDGE_SETS:
        edges = FIX["%s/%s/edges" % (name, tag)]
        eng.set_lightcurves(t, y, dy)
        ab = eng.cross_sums(t2, y2, edges, count=True, lag=False, cf=False)["count"][0]
        eng.set_lightcurves(t2, y2, np.ones_like(y2))
        ba = eng.cross_sums(t, y, -edges[::-1], count=True, lag=False, cf=False)["count"][0]
        assert np.array_equal(ab, FIX["%s/%s/count" % (name, tag)]), tag
        assert np.array_equal(ba, cn.cross_sums(t2, y2, t, y, -edges[::-1])["count"]), tag
        # fl(t_i - t2_j) = -fl(t2_j - t_i), and the bins are the mirror images but for their closed ends: a pair ON an edge
        # changes sides (sym8 has the edge 0 and the copied times give tau == 0; "ties" is made of such edges)
        if not np.any(np.isin(tau, edges)):
            assert np.array_equal(ab, ba[::-1]), tag
            without_ties += 1
        else:
            assert tag in ("sym8", "ties") and ab.sum() - ba.sum() == np.sum(tau == edges[0]) - np.sum(tau == edges[-1]), tag
    assert without_ties == 4


def test_errors_and_a_working_context_afterwards(eng):
    t, y, dy, t2, y2 = case("n52")
    edges = FIX["n52/sym8/edges"]
    M = len(t2)
    fresh = Engine(0)
    try:
        with pytest.raises(EngineError) as exc:
            fresh.cross_sums(t2, y2, edges)
        assert exc.value.code == engine.E_STATE
        fresh.set_lightcurves(t, np.stack([y, y[::-1], 2.0 * y]), np.tile(dy, (3, 1)))
        eng.set_lightcurves(t, np.stack([y, y[::-1], 2.0 * y]), np.tile(dy, (3, 1)))
        before = fresh.cross_sums(t2, y2, edges, **ALL)
        assert same(before, eng.cross_sums(t2, y2, edges, **ALL))
        resident = fresh.lomb_scargle(np.linspace(0.01, 0.1, 7))
        spoilt = lambda a, k, v: np.concatenate([a[:k], [v], a[k + 1:]])
        bad = [
            (t2, np.tile(y2, (2, 1)), edges, "L2 = 2"),
            (spoilt(t2, 5, np.nan), y2, edges, "t2[5]"), (spoilt(t2, 60, np.inf), y2, edges, "t2[60]"),
            (spoilt(t2, 9, t2[7]), y2, edges, "t2[9]"), (t2[::-1].copy(), y2, edges, "t2[1]"),
            (t2, spoilt(y2, 17, np.nan), edges, "y2[0][17]"), (t2, np.stack([y2, y2, spoilt(y2, 3, -np.inf)]), edges, "y2[2][3]"),
            (t2, y2, np.linspace(-1.0, 1.0, 130), "nbins = 129"), (t2, y2, [0.0, np.nan], "edges[1]"), (t2, y2, [-np.inf, 1.0], "edges[0]"),
            (t2, y2, [-1.0, 1.0, 1.0], "edges[2]"), (t2, y2, [-1.0, -2.0], "edges[1]"),
        ]
        for a, b, e, word in bad:
            with pytest.raises(EngineError) as exc:
                fresh.cross_sums(a, b, e)
            assert exc.value.code == engine.E_ARG and word in str(exc.value), word
            assert same(fresh.cross_sums(t2, y2, edges, **ALL), before)
        # Engine.cross_sums' own checks; M, nbins = 0 and every output NULL straight through the C entry
        with pytest.raises(ValueError):
            fresh.cross_sums(t2, y2, edges, count=False, lag=False, cf=False)
        with pytest.raises(ValueError):
            fresh.cross_sums(t2, y2, [1.0])
        with pytest.raises(ValueError):
            fresh.cross_sums(t2, y2[:-1], edges)
        lib, ctx = fresh._lib, fresh._ctx
        ep, tp, yp, out = engine._ptr(np.ascontiguousarray(edges)), engine._ptr(t2), engine._ptr(y2), np.zeros(3 * 8)
        none = [None] * 8
        assert lib.mtg_cross_sums(ctx, 0, tp, 1, yp, 8, ep, *none[:2], engine._ptr(out), *none[3:]) == engine.E_ARG and b"M = 0" in lib.mtg_last_error(ctx)
        assert lib.mtg_cross_sums(ctx, 1 << 28, tp, 1, yp, 8, ep, *none[:2], engine._ptr(out), *none[3:]) == engine.E_ARG and b"M = 268435456" in lib.mtg_last_error(ctx)
        assert lib.mtg_cross_sums(ctx, M, tp, 1, yp, 0, ep, *none[:2], engine._ptr(out), *none[3:]) == engine.E_ARG and b"nbins = 0" in lib.mtg_last_error(ctx)
        assert lib.mtg_cross_sums(ctx, M, tp, 1, yp, 8, ep, *none) == engine.E_ARG and b"NULL" in lib.mtg_last_error(ctx)
        assert same(fresh.cross_sums(t2, y2, edges, **ALL), before)
        # the resident set was only read, and the other entries still run on the same context
        assert np.array_equal(fresh.lomb_scargle(np.linspace(0.01, 0.1, 7)), resident)
        assert np.array_equal(resident, eng.lomb_scargle(np.linspace(0.01, 0.1, 7)))
        # equal companion times are allowed, and a companion of one sample
        assert fresh.cross_sums(spoilt(t2, 9, t2[8]), y2, edges)["count"].sum() > 0
        one = fresh.cross_sums(t2[:1], y2[:1], [-1e30, 1e30], **ALL)
        assert np.all(one["count"] == len(t)) and np.all(one["cf"] == 0.0) and np.all(one["sb"] == 0.0)
    finally:
        fresh.close()


def test_cross_correlation_finds_a_known_shift():
    # a smooth series and a copy of it delayed by `shift`, each on its own irregular sampling
    rng = np.random.default_rng(2)
    t1 = np.sort(rng.uniform(0.0, 200.0, 400))
    t2 = np.sort(rng.uniform(20.0, 230.0, 310))
    shift = 9.0
    signal = lambda t: np.sin(0.11 * t) + 0.7 * np.sin(0.37 * t + 1.0) + 0.4 * np.sin(0.05 * t + 2.0)
    y1 = 10.0 + signal(t1) + 0.05 * rng.standard_normal(len(t1))
    y2 = 4.0 + 2.0 * signal(t2 - shift) + 0.1 * rng.standard_normal(len(t2))
    edges = timedomain.cross_lag_bins(t1, t2, 25, max_lag=50.0)      # bins of 4: the shift lies in [6, 10)
    home = int(np.searchsorted(edges, shift, side="right") - 1)
    cc = timedomain.CrossCorrelation(t1, y1, t2, y2, dy1=0.05, dy2=0.1)
    lag, ccf, err, count = cc.ccf(edges)
    l_lag, l_ccf, l_err, l_count = cc.ccf(edges, normalization="local")
    assert lag.shape == ccf.shape == err.shape == count.shape == (25,) and np.array_equal(count, l_count) and np.array_equal(lag, l_lag)
    assert np.array_equal(count, cn.cross_sums(t1, y1, t2, y2, edges)["count"]) and count.min() >= 2
    for values in (ccf, l_ccf):
        assert int(np.nanargmax(values)) == home and values[home] > 0.8
        peak, centroid = timedomain.lag_peak_and_centroid(lag, values)
        assert edges[home] <= peak < edges[home + 1] and edges[home] <= centroid < edges[home + 1]
    assert np.all(np.abs(l_ccf) <= 1.0 + 1e-12) and np.all(err > 0) and np.all(l_err > 0)
    assert np.all(np.sign(ccf[home - 1:home + 2]) == np.sign(l_ccf[home - 1:home + 2]))
    # against the plain-numpy sums, and the noise term only scales the global form
    want = timedomain.ccf_from_sums(cn.cross_sums(t1, y1, t2, y2, edges), np.var(y1), np.var(y2), 0.05 ** 2, 0.1 ** 2)
    assert np.allclose(ccf, want[1], rtol=1e-9, atol=1e-12) and np.allclose(err, want[2], rtol=1e-6)
    raw = cc.ccf(edges, subtract_noise=False)[1]
    assert np.allclose(raw / ccf, np.sqrt((np.var(y1) - 0.05 ** 2) * (np.var(y2) - 0.1 ** 2) / (np.var(y1) * np.var(y2))), rtol=1e-12)
    # a set of light curves against one companion and against a companion each: [L][nbins], row 0 the same bits
    many = timedomain.CrossCorrelation(t1, np.stack([y1, y1[::-1]]), t2, y2, dy1=0.05, dy2=0.1).ccf(edges)
    each = timedomain.CrossCorrelation(t1, np.stack([y1, y1[::-1]]), t2, np.stack([y2, y2[::-1]]), dy1=0.05, dy2=0.1).ccf(edges)
    assert many[1].shape == (2, 25) and np.array_equal(many[1][0], ccf) and np.array_equal(each[1][0], ccf)
    # an empty bin is NaN
    empty = cc.ccf([-1e6, -1e5, 0.0])
    assert empty[3][0] == 0 and np.isnan(empty[0][0]) and np.isnan(empty[1][0]) and np.isfinite(empty[1][1])


def test_cross_lag_significance_end_to_end_and_reproducible():
    import types
    from mind_the_gaps_amd import ppp
    from mind_the_gaps_amd import synthetic as synth
    from mind_the_gaps_amd.gp import get_engine
    from mind_the_gaps_amd.lightcurves import GappyLightcurve
    from mind_the_gaps_amd.models import DampedRandomWalk
    th = synth.truth(synth.ALT_MODEL)
    times, rates, err = synth.make_lightcurves(60, 1, seed=43)
    lc = GappyLightcurve(times, rates[0] + 50.0, err[0], exposures=0.5 * np.diff(times).min())
    rng = np.random.default_rng(4)
    span = times[-1] - times[0]
    t2 = np.sort(rng.uniform(times[0] + 0.1 * span, times[-1] + 0.1 * span, 40))
    comp = types.SimpleNamespace(times=t2, y=20.0 + np.interp(t2 - 0.05 * span, times, rates[0]) + 0.1 * rng.standard_normal(40),
                                 dy=np.full(40, 0.1))
    edges = timedomain.cross_lag_bins(times, t2, 6)

    def null():
        return DampedRandomWalk(th[0], th[1], bounds=[(-10, 50), (-10, 10)])
    kw = dict(nsims=8, walkers=8, max_steps=60, sigma_noise=0.5, seed=21)
    for norm in ("global", "local"):
        a = ppp.cross_lag_significance(lc, comp, null(), edges, normalization=norm, levels=(0.9, 0.99), **kw)
        b = ppp.cross_lag_significance(lc, comp, null(), edges, normalization=norm, levels=(0.9, 0.99), **kw)
        for k in ("lag", "count", "observed", "median", "share_above", "share_below"):
            assert a[k].shape == (6,) and np.array_equal(a[k], b[k], equal_nan=True), (norm, k)
        for k in ("lower", "upper"):
            assert a[k].shape == (2, 6) and np.array_equal(a[k], b[k], equal_nan=True), (norm, k)
        for k in ("sims", "sim_peaks", "sim_peak_lags", "samples"):
            assert len(a[k]) == 8 and np.array_equal(a[k], b[k], equal_nan=True), (norm, k)
        assert a["sims"].shape == (8, 6) and (a["peak"], a["peak_lag"], a["p_global"]) == (b["peak"], b["peak_lag"], b["p_global"])
        ok = a["count"] >= 2
        assert ok.sum() >= 3 and np.all(np.isfinite(a["observed"][ok])) and np.all(np.isfinite(a["sims"][:, ok]))
        assert 1.0 / 9.0 <= a["p_global"] <= 1.0
        assert a["p_global"] == (1.0 + np.sum(a["sim_peaks"] >= a["peak"])) / 9.0
        assert a["peak"] == np.nanmax(np.abs(a["observed"])) and a["peak_lag"] == a["lag"][np.nanargmax(np.abs(a["observed"]))]
        assert np.array_equal(a["sim_peaks"], np.nanmax(np.abs(a["sims"]), axis=1))
        assert np.all(a["lower"][0, ok] <= a["median"][ok]) and np.all(a["median"][ok] <= a["upper"][0, ok])
        # the observed row is a direct call on the observed light curve
        eng = get_engine(0)
        y, dy = np.asarray(lc.y, dtype=np.float64), np.asarray(lc.dy, dtype=np.float64)
        eng.set_lightcurves(np.asarray(lc.times, dtype=np.float64), y, dy)
        eng.bound_to = None
        sums = eng.cross_sums(comp.times, comp.y, edges, **ALL)
        s2a = np.mean((y[None, :] - y[None, :].mean(axis=1, keepdims=True)) ** 2, axis=1)
        s2b = float(np.mean((comp.y - comp.y.mean()) ** 2))
        direct = timedomain.ccf_from_sums(sums, s2a, s2b, np.mean(dy[None, :] ** 2, axis=1), float(np.mean(comp.dy ** 2)), norm)[1][0]
        assert np.array_equal(a["observed"], direct, equal_nan=True) and np.array_equal(a["count"], sums["count"][0])
