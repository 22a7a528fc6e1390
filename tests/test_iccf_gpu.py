"""mtg_iccf on the GPU (include/mtg.h): the interpolated cross-correlation function of two series on their own samplings.

Accuracy is held against the exact truth of tests/golden/iccf_golden.npz (scripts/make_iccf_golden.py: rational sums, the
square root at 50 digits), with rho the error of tests/iccf_numpy.py (plain float64) and u = 2^-53: each half is within
    max(10 rho, 64 sqrt(n) u S),   S = Cabs / sqrt(Va Vb) + |r| (Vaabs / Va + Vbabs / Vb) / 2
the combined value within the mean of its halves' bounds, the counts are exact, and the device is NaN exactly where the
truth is.  The independence properties of the header are bit for bit.

Measured on the MI355X: the largest ratio to the bound is printed by test_values_and_counts_against_the_truth; the figure
of the run that went with this file is in README.md.
"""
import os

import numpy as np
import pytest

import iccf_numpy as inp
from mind_the_gaps_amd import engine, timedomain
from mind_the_gaps_amd.engine import Engine, EngineError

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = np.load(os.path.join(HERE, "golden", "iccf_golden.npz"))
LS = np.load(os.path.join(HERE, "golden", "lomb_scargle_golden.npz"))
U = 2.0 ** -53


def case(name):
    return tuple(LS["%s/%s" % (name, k)] for k in ("t", "y", "dy")) + (FIX[name + "/t2"], FIX[name + "/y2"])


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def same(a, b):
    """two Iccf results, bit for bit (NaN equal to NaN)"""
    return all((x is None) == (y is None) and (x is None or np.array_equal(x, y, equal_nan=x.dtype == np.float64)) for x, y in zip(a, b))


def half_bound(key, h):
    return inp.bound(FIX[key + "rho_" + h], FIX[key + "n_" + h], FIX[key + "s_" + h])


def half_error(got, key, h):
    return np.abs((got - FIX[key + "r_" + h]) - FIX[key + "r_%s_lo" % h])


def test_values_and_counts_against_the_truth(eng):
    worst, nans, entries = (0.0, None), 0, 0
    for name in inp.CASES:
        t, y, dy, t2, y2 = case(name)
        eng.set_lightcurves(t, y, dy)
        for tag in inp.LAG_SETS:
            key = "%s/%s/" % (name, tag)
            lags = FIX[key + "lags"]
            got = {mode: eng.iccf(t2, y2, lags, mode=mode, counts=True) for mode in inp.MODES}
            assert got["both"].ccf.shape == (1, len(lags)) and got["both"].n_a.dtype == np.int64
            # counts: exact; 0 for the half a mode does not form
            assert np.array_equal(got["both"].n_a[0], FIX[key + "n_a"]) and np.array_equal(got["both"].n_b[0], FIX[key + "n_b"]), key
            assert np.array_equal(got["companion"].n_a[0], FIX[key + "n_a"]) and np.all(got["companion"].n_b == 0), key
            assert np.array_equal(got["resident"].n_b[0], FIX[key + "n_b"]) and np.all(got["resident"].n_a == 0), key
            ba, bb = half_bound(key, "a"), half_bound(key, "b")
            line = []
            for mode, err, b, truth in (
                    ("companion", half_error(got["companion"].ccf[0], key, "a"), ba, FIX[key + "r_a"]),
                    ("resident", half_error(got["resident"].ccf[0], key, "b"), bb, FIX[key + "r_b"]),
                    ("both", np.abs((got["both"].ccf[0] - 0.5 * (FIX[key + "r_a"] + FIX[key + "r_b"]))
                                    - 0.5 * (FIX[key + "r_a_lo"] + FIX[key + "r_b_lo"])), 0.5 * (ba + bb), FIX[key + "r_a"] + FIX[key + "r_b"])):
                value = got[mode].ccf[0]
                assert np.array_equal(np.isnan(value), np.isnan(truth)) and not np.any(np.isinf(value)), (key, mode)
                fin = np.isfinite(truth)
                nans += int(np.sum(~fin))
                entries += len(truth)
                ratio = float(np.max(err[fin] / b[fin])) if fin.any() else 0.0
                line.append("%s %.3f" % (mode, ratio))
                if ratio > worst[0]:
                    worst = (ratio, (name, tag, mode))
            print("%-5s %-9s |r - truth| / bound: %s" % (name, tag, "  ".join(line)))
    assert "mtg_iccf_kernel<1,0,1>" in eng.last_solver and eng.last_kernel_ms > 0
    assert nans > 0 and entries == 3 * 4 * (65 + 1 + 257 + 29 + 21 + 67)       # no entry is left out
    print("largest ratio to the bound: %.3f at %s" % worst)
    assert worst[0] <= 1.0, worst


def test_ties_land_on_the_node(eng):
    # the lags of "ties" put a shifted resident sample exactly on a companion node, the span's two ends among them: the
    # sample counts (x == t2[0] and x == t2[-1] are inside), its value is the node's -- a companion that is zero but for
    # that node makes it the only large term -- and a lag one ulp away gives what the definition gives there
    for name in inp.CASES:
        t, y, dy, t2, y2 = case(name)
        key = name + "/ties/"
        lags, ties = FIX[key + "lags"], FIX[key + "tie_pairs"]
        eng.set_lightcurves(t, y, dy)
        at_ends = 0
        for k, i, j in ties[:: max(1, len(ties) // 8)].tolist() + [row for row in ties.tolist() if row[2] in (0, len(t2) - 1)][:4]:
            spike = np.zeros(len(t2))
            spike[np.flatnonzero(t2 == t2[j])[-1]] = 1.0
            near = np.array([lags[k], np.nextafter(lags[k], np.inf), np.nextafter(lags[k], -np.inf)])
            got = eng.iccf(t2, spike, near, mode="companion", counts=True)
            want = inp.iccf(t, y, t2, spike, near)
            assert np.array_equal(got.n_a[0], want["n_a"]) and got.n_a[0, 0] == FIX[key + "n_a"][k], (name, k)
            assert np.array_equal(np.isnan(got.ccf[0]), np.isnan(want["r_a"])), (name, k)
            fin = np.isfinite(want["r_a"])
            assert np.all(np.abs(got.ccf[0] - want["r_a"])[fin] <= 1e-9), (name, k)
            at_ends += j in (0, len(t2) - 1)
        assert at_ends >= 2


def test_an_entry_depends_on_its_own_series_its_lag_and_the_mode_alone(eng):
    t, y, dy, t2, y2 = case("n789")
    sym, shuffled, m = FIX["n789/sym65/lags"], FIX["n789/shuffled/lags"], inp.shuffle_map()
    rng = np.random.default_rng(11)
    Y = y[None, :] + 0.3 * rng.standard_normal((11, len(t)))
    Y2 = y2[None, :] + 0.3 * rng.standard_normal((11, len(t2)))
    for k in (0, 6, 10):
        Y[k], Y2[k] = y, y2
    for mode in inp.MODES:
        full = int(mode != "companion")
        eng.set_lightcurves(t[None, :], y[None, :], dy[None, :])      # alone, the sampling stored per light curve
        alone = eng.iccf(t2, y2, sym, mode=mode, counts=True, peak=True)
        assert "mtg_iccf_kernel<1,0,%d>" % full in eng.last_solver
        # the order of the lags, K and duplicates
        mixed = eng.iccf(t2, y2, shuffled, mode=mode, counts=True)
        assert all(np.array_equal(getattr(mixed, q)[0], getattr(alone, q)[0][m], equal_nan=True) for q in ("ccf", "n_a", "n_b")), mode
        one = eng.iccf(t2, y2, sym[17:18], mode=mode, counts=True)
        assert all(np.array_equal(getattr(one, q)[0], getattr(alone, q)[0][17:18]) for q in ("ccf", "n_a", "n_b")), mode
        # which outputs were asked for
        assert np.array_equal(eng.iccf(t2, y2, sym, mode=mode).ccf, alone.ccf)
        only = eng.iccf(t2, y2, sym, mode=mode, values=False, counts=True)
        assert only.ccf is None and np.array_equal(only.n_a, alone.n_a) and np.array_equal(only.n_b, alone.n_b)
        peaks = eng.iccf(t2, y2, sym, mode=mode, values=False, peak=True)
        assert same(peaks[3:], alone[3:]) and peaks.ccf is None and peaks.n_a is None
        assert np.array_equal(eng.iccf(t2, y2[None, :], sym, mode=mode).ccf, alone.ccf)      # [1][M]
        # members 0, 6 and 10 of 11: shared sampling (tiles of four, the last partly filled) and stored per light curve
        for times in (t, np.tile(t, (11, 1))):
            tile = 4 if times.ndim == 1 else 1
            eng.set_lightcurves(times, Y, np.tile(dy, (11, 1)))
            among = eng.iccf(t2, y2, shuffled, mode=mode, counts=True, peak=True)            # one companion for all
            assert "mtg_iccf_kernel<%d,0,%d>" % (tile, full) in eng.last_solver
            repeated = eng.iccf(t2, np.tile(y2, (11, 1)), shuffled, mode=mode, counts=True, peak=True)   # L2 == L, identical rows
            assert "mtg_iccf_kernel<%d,1,%d>" % (tile, full) in eng.last_solver and same(repeated, among), mode
            per = eng.iccf(t2, Y2, shuffled, mode=mode, counts=True, peak=True)              # a companion row per light curve
            for k in (0, 6, 10):
                for got in (among, per):
                    assert all(np.array_equal(getattr(got, q)[k], getattr(alone, q)[0][m], equal_nan=True) for q in ("ccf", "n_a", "n_b")), (mode, k)
            assert not np.array_equal(among.ccf[1], among.ccf[0]) and not np.array_equal(per.ccf[1], among.ccf[1])
            assert np.all(among.n_a == among.n_a[0]) and np.all(among.n_b == among.n_b[0])   # the counts are the samplings'


def test_more_than_one_slab(eng):
    # case n5 at 65536 lags with all three [L][K] arrays: 168 light curves fit 256 MiB on shared sampling, 170 stored per
    # light curve, so L = 173 is cut in two either way (tests/test_iccf_cpu.py holds these figures to the planner)
    t, y, dy, t2, y2 = case("n5")
    K, L = inp.TWO_SLABS["K"], inp.TWO_SLABS["L"]
    lags = np.linspace(-1.2, 1.2, K) * (t[-1] - t[0])
    rng = np.random.default_rng(5)
    Y = y[None, :] + 0.3 * rng.standard_normal((L, len(t)))
    Y2 = y2[None, :] + 0.3 * rng.standard_normal((L, len(t2)))
    for times in (t, np.tile(t, (L, 1))):
        eng.set_lightcurves(times, Y, np.tile(dy, (L, 1)))
        slabbed = eng.iccf(t2, Y2, lags, counts=True, peak=True)                 # three arrays: two slabs
        whole = eng.iccf(t2, Y2, lags)                                           # one array: one slab
        assert np.array_equal(slabbed.ccf, whole.ccf, equal_nan=True) and np.isnan(whole.ccf).any() and np.isfinite(whole.ccf[L - 1]).any()
        # the rows beyond the first slab on their own: the same bits, counts and peaks
        eng.set_lightcurves(times if times.ndim == 1 else times[168:], Y[168:], np.tile(dy, (L - 168, 1)))
        tail = eng.iccf(t2, Y2[168:], lags, counts=True, peak=True)
        assert same(tail, engine.Iccf(*(a[168:] for a in slabbed)))
        fin = np.where(np.isfinite(slabbed.ccf), slabbed.ccf, -np.inf)
        assert np.array_equal(slabbed.peak, fin.max(axis=1)) and np.array_equal(slabbed.peak_index, fin.argmax(axis=1))


@pytest.mark.parametrize("name", inp.CASES)
def test_swapping_the_series_and_the_sign_of_the_lag_exchanges_the_halves(eng, name):
    t, y, dy, t2, y2 = case(name)
    for tag in ("sym65", "beyond", "ties"):
        key = "%s/%s/" % (name, tag)
        lags = FIX[key + "lags"]
        eng.set_lightcurves(t, y, dy)
        ab = eng.iccf(t2, y2, lags, mode="resident", counts=True)
        eng.set_lightcurves(t2, y2, np.ones_like(y2))
        ba = eng.iccf(t, y, -lags, mode="companion", counts=True)
        # the same samples, brackets and sums; the two means come from the pre-pass in exchanged roles: not bit for bit
        assert np.array_equal(ab.n_b, ba.n_a) and np.array_equal(ab.n_b[0], FIX[key + "n_b"]), key
        assert np.array_equal(np.isnan(ab.ccf), np.isnan(ba.ccf)), key
        fin = np.isfinite(FIX[key + "r_b"])
        b = half_bound(key, "b")
        assert np.all(half_error(ba.ccf[0], key, "b")[fin] <= b[fin]) and np.all(np.abs(ab.ccf[0] - ba.ccf[0])[fin] <= 2 * b[fin]), key


def test_peak_and_centroid(eng):
    t, y, dy, t2, y2 = case("n216")
    rng = np.random.default_rng(9)
    Y = np.stack([y, -y, y[::-1], y + rng.standard_normal(len(y))])
    eng.set_lightcurves(t, Y, np.tile(dy, (4, 1)))
    for tag in ("sym65", "fine257", "beyond", "shuffled", "one"):
        lags = FIX["n216/%s/lags" % tag]
        K = len(lags)
        for threshold in (0.8, 0.3, 1.0):
            got = eng.iccf(t2, y2, lags, threshold=threshold, peak=True)
            fin = np.isfinite(got.ccf)
            assert fin.any(axis=1).all()
            masked = np.where(fin, got.ccf, -np.inf)
            assert np.array_equal(got.peak, masked.max(axis=1)) and np.array_equal(got.peak_index, masked.argmax(axis=1)), tag   # the first maximum
            want = timedomain.lag_peak_and_centroid(np.tile(lags, (4, 1)), got.ccf, threshold)[1]
            use = fin & (got.ccf >= threshold * got.peak[:, None])
            den = np.where(use, got.ccf, 0.0).sum(axis=1)
            tol = 4 * K * U * (np.where(use, np.abs(lags[None, :] * got.ccf), 0.0).sum(axis=1) / np.where(den > 0, den, 1.0) + np.abs(want))
            assert np.array_equal(np.isnan(got.centroid), np.isnan(want)), (tag, threshold)
            ok = np.isfinite(want)
            assert np.all(np.abs(got.centroid - want)[ok] <= tol[ok]), (tag, threshold)
    # rows without a finite value: NaN, -1, NaN; a row whose peak is not positive has no centroid
    none = eng.iccf(t2, y2, [1e6, -1e6], peak=True)
    assert np.all(np.isnan(none.peak)) and np.all(none.peak_index == -1) and np.all(np.isnan(none.centroid)) and np.all(np.isnan(none.ccf))
    lags = FIX["n216/sym65/lags"]
    got = eng.iccf(t2, y2, lags, peak=True)
    row, low = np.unravel_index(int(np.argmin(got.ccf[:2])), (2, len(lags)))       # rows 0 and 1 are y and -y: one of them dips below 0
    anti = eng.iccf(t2, y2, lags[low:low + 1], peak=True)
    assert anti.peak[row] == got.ccf[row, low] < 0 and anti.peak_index[row] == 0 and np.isnan(anti.centroid[row])
    assert anti.peak[1 - row] > 0 and anti.centroid[1 - row] == lags[low]


def test_errors_and_a_working_context_afterwards(eng):
    t, y, dy, t2, y2 = case("n52")
    lags = FIX["n52/sym65/lags"]
    M = len(t2)
    fresh = Engine(0)
    try:
        with pytest.raises(EngineError) as exc:
            fresh.iccf(t2, y2, lags)
        assert exc.value.code == engine.E_STATE
        fresh.set_lightcurves(t, np.stack([y, y[::-1], 2.0 * y]), np.tile(dy, (3, 1)))
        eng.set_lightcurves(t, np.stack([y, y[::-1], 2.0 * y]), np.tile(dy, (3, 1)))
        before = fresh.iccf(t2, y2, lags, counts=True, peak=True)
        assert same(before, eng.iccf(t2, y2, lags, counts=True, peak=True))
        resident = fresh.lomb_scargle(np.linspace(0.01, 0.1, 7))
        spoilt = lambda a, k, v: np.concatenate([a[:k], [v], a[k + 1:]])
        bad = [
            (t2, np.tile(y2, (2, 1)), lags, "L2 = 2"),
            (spoilt(t2, 5, np.nan), y2, lags, "t2[5]"), (spoilt(t2, 60, np.inf), y2, lags, "t2[60]"),
            (spoilt(t2, 9, t2[7]), y2, lags, "t2[9]"), (t2[::-1].copy(), y2, lags, "t2[1]"),
            (t2, spoilt(y2, 17, np.nan), lags, "y2[0][17]"), (t2, np.stack([y2, y2, spoilt(y2, 3, -np.inf)]), lags, "y2[2][3]"),
            (t2, y2, spoilt(lags, 33, np.nan), "tau[33]"), (t2, y2, spoilt(lags, 0, np.inf), "tau[0]"), (t2[:1], y2[:1], lags, "M = 1"),
        ]
        for a, b, e, word in bad:
            with pytest.raises(EngineError) as exc:
                fresh.iccf(a, b, e)
            assert exc.value.code == engine.E_ARG and word in str(exc.value), word
            assert same(fresh.iccf(t2, y2, lags, counts=True, peak=True), before)
        # M, K, mode, threshold and every output NULL straight through the C entry
        lib, ctx = fresh._lib, fresh._ctx
        lp, tp, yp, out = engine._ptr(np.ascontiguousarray(lags)), engine._ptr(t2), engine._ptr(y2), np.zeros(3 * 65)
        none = [None] * 5
        call = lambda M_, K_, mode, threshold, first: lib.mtg_iccf(ctx, M_, tp, 1, yp, K_, lp, mode, threshold, first, *none)
        for args, word in (((1 << 28, 65, 0, 0.8, engine._ptr(out)), b"M = 268435456"), ((M, 0, 0, 0.8, engine._ptr(out)), b"K = 0"),
                           ((M, 65537, 0, 0.8, engine._ptr(out)), b"K = 65537"), ((M, 65, 3, 0.8, engine._ptr(out)), b"mode 3"),
                           ((M, 65, -1, 0.8, engine._ptr(out)), b"mode -1"), ((M, 65, 0, 0.0, engine._ptr(out)), b"threshold"),
                           ((M, 65, 0, 1.25, engine._ptr(out)), b"threshold"), ((M, 65, 0, float("nan"), engine._ptr(out)), b"threshold"),
                           ((M, 65, 0, 0.8, None), b"NULL")):
            assert call(*args) == engine.E_ARG and word in lib.mtg_last_error(ctx), word
        assert same(fresh.iccf(t2, y2, lags, counts=True, peak=True), before)
        # a resident set of one sample per light curve: nothing to interpolate between
        short = Engine(0)
        try:
            short.set_lightcurves(t[:1], y[:1], dy[:1])
            with pytest.raises(EngineError) as exc:
                short.iccf(t2, y2, lags)
            assert exc.value.code == engine.E_ARG and "N = 1" in str(exc.value)
        finally:
            short.close()
        # the resident set was only read, and the other entries still run on the same context
        assert np.array_equal(fresh.lomb_scargle(np.linspace(0.01, 0.1, 7)), resident)
        # equal companion times are allowed: the last of the group is the left node
        twin = spoilt(t2, 9, t2[8])
        got = fresh.iccf(twin, y2, lags, counts=True)
        want = inp.iccf(t, y, twin, y2, lags)
        assert np.array_equal(got.n_a[0], want["n_a"]) and np.allclose(got.ccf[0], inp.combine("both", want["r_a"], want["r_b"]), rtol=0, atol=1e-12)
    finally:
        fresh.close()


def test_interpolated_cross_correlation_finds_a_known_shift():
    # a smooth series and a copy of it delayed by `shift`, each on its own irregular sampling
    rng = np.random.default_rng(2)
    t1 = np.sort(rng.uniform(0.0, 200.0, 400))
    t2 = np.sort(rng.uniform(20.0, 230.0, 310))
    shift = 9.0
    signal = lambda t: np.sin(0.11 * t) + 0.7 * np.sin(0.37 * t + 1.0) + 0.4 * np.sin(0.05 * t + 2.0)
    y1 = 10.0 + signal(t1) + 0.02 * rng.standard_normal(len(t1))
    y2 = 4.0 + 2.0 * signal(t2 - shift) + 0.04 * rng.standard_normal(len(t2))
    lags = timedomain.iccf_lags(t1, t2, n=401, max_lag=50.0)                     # a grid step of 0.25
    step = lags[1] - lags[0]
    cc = timedomain.InterpolatedCrossCorrelation(t1, y1, t2, y2)
    for mode in inp.MODES:
        ccf, n_a, n_b = cc.ccf(lags, mode=mode)
        assert ccf.shape == n_a.shape == n_b.shape == (401,) and np.all(np.abs(ccf) <= 1.0 + 1e-12)
        want = inp.iccf(t1, y1, t2, y2, lags)
        assert np.allclose(ccf, inp.combine(mode, want["r_a"], want["r_b"]), rtol=0, atol=1e-11)
        assert np.array_equal(n_a, want["n_a"] if mode != "resident" else 0 * n_a) and np.array_equal(n_b, want["n_b"] if mode != "companion" else 0 * n_b)
        peak_lag, centroid, peak = cc.lag(lags, mode=mode)
        assert abs(peak_lag - shift) <= step and abs(centroid - shift) <= 1.0 and peak > 0.99 and peak == ccf.max() and peak_lag == lags[np.argmax(ccf)]
    # a set of light curves against one companion and against a companion each: [L][K], row 0 the same bits
    ccf = cc.ccf(lags)[0]
    many = timedomain.InterpolatedCrossCorrelation(t1, np.stack([y1, y1[::-1]]), t2, y2)
    each = timedomain.InterpolatedCrossCorrelation(t1, np.stack([y1, y1[::-1]]), t2, np.stack([y2, y2[::-1]]))
    assert many.ccf(lags)[0].shape == (2, 401) and np.array_equal(many.ccf(lags)[0][0], ccf) and np.array_equal(each.ccf(lags)[0][0], ccf)
    at, centroid, peak = many.lag(lags)
    assert at.shape == centroid.shape == peak.shape == (2,) and at[0] == cc.lag(lags)[0]


def test_iccf_significance_end_to_end_and_reproducible():
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
    comp = types.SimpleNamespace(times=t2, y=20.0 + np.interp(t2 - 0.05 * span, times, rates[0]) + 0.1 * rng.standard_normal(40), dy=None)
    lags = timedomain.iccf_lags(times, t2, n=41)

    def null():
        return DampedRandomWalk(th[0], th[1], bounds=[(-10, 50), (-10, 10)])
    kw = dict(nsims=8, walkers=8, max_steps=60, sigma_noise=0.5, seed=21, levels=(0.9, 0.99))
    a = ppp.iccf_significance(lc, comp, null(), lags, **kw)
    b = ppp.iccf_significance(lc, comp, null(), lags, **kw)
    for k in ("lags", "n_a", "n_b", "observed", "median", "share_above", "share_below"):
        assert a[k].shape == (41,) and np.array_equal(a[k], b[k], equal_nan=True), k
    for k in ("lower", "upper"):
        assert a[k].shape == (2, 41) and np.array_equal(a[k], b[k], equal_nan=True), k
    for k in ("sims", "sim_peaks", "sim_peak_lags", "sim_centroids", "samples"):
        assert len(a[k]) == 8 and np.array_equal(a[k], b[k], equal_nan=True), k
    assert a["sims"].shape == (8, 41) and all(a[k] == b[k] for k in ("peak", "peak_lag", "centroid", "p_global", "sim_seed"))
    assert np.all(np.isfinite(a["observed"])) and np.all(np.isfinite(a["sims"])) and a["n_a"].min() >= 2
    assert 1.0 / 9.0 <= a["p_global"] <= 1.0 and a["p_global"] == (1.0 + np.sum(a["sim_peaks"] >= a["peak"])) / 9.0
    assert a["peak"] == a["observed"].max() and a["peak_lag"] == lags[np.argmax(a["observed"])]
    assert np.array_equal(a["sim_peaks"], a["sims"].max(axis=1)) and np.array_equal(a["sim_peak_lags"], lags[np.argmax(a["sims"], axis=1)])
    assert np.all(a["lower"][0] <= a["median"]) and np.all(a["median"] <= a["upper"][0])
    # the observed row is a direct call on the observed light curve
    eng = get_engine(0)
    y, dy = np.asarray(lc.y, dtype=np.float64), np.asarray(lc.dy, dtype=np.float64)
    eng.set_lightcurves(np.asarray(lc.times, dtype=np.float64), y, dy)
    eng.bound_to = None
    direct = eng.iccf(comp.times, comp.y, lags, peak=True)
    assert np.array_equal(a["observed"], direct.ccf[0]) and a["centroid"] == direct.centroid[0]
