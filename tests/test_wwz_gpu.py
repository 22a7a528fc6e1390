"""mtg_wwz on the GPU (include/mtg.h): Foster's weighted wavelet Z-transform of the resident light curves.

Accuracy is held against the 50-digit truth of tests/golden/wwz_golden.npz (scripts/make_wwz_golden.py: Foster's formulas
as written, no cut, no rescaling), with rho the error of tests/wwz_numpy.py (plain float64), u = 2^-53 and kappa the
condition number of the normalised 3 x 3 normal matrix:
    P         within b = max(10 rho, 64 sqrt(N) u kappa)        (the bound of tests/test_lomb_scargle_multi_gpu.py)
    N_eff     within 64 sqrt(N) u, relative
    Z         within b |dZ/dP| + (64 sqrt(N) u) N_eff |dZ/dN_eff|, both at the truth
    amplitude within max(10 rho_A, 64 sqrt(N) u kappa) sqrt(V_x)
Entries whose true N_eff < 4 (at most 10 % of a case, asserted by the generator) are only required to be finite or NaN.
The independence properties of the header are bit for bit.

Measured on the MI355X: the largest ratio to the bound is printed by test_accuracy_against_the_50_digit_truth; the figure
of the run that went with this file is in README.md.
"""
import os

import numpy as np
import pytest

import wwz_numpy as wn
from mind_the_gaps_amd import engine, periodogram
from mind_the_gaps_amd.engine import Engine, EngineError

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = np.load(os.path.join(HERE, "golden", "wwz_golden.npz"))
LS = np.load(os.path.join(HERE, "golden", "lomb_scargle_golden.npz"))
CASES = [str(c) for c in FIX["cases"]]
DECAYS = [float(c) for c in FIX["decays"]]
U = 2.0 ** -53


def case(name):
    return tuple(LS["%s/%s" % (name, k)] for k in ("t", "y", "dy")) + (FIX[name + "/freqs"], FIX[name + "/taus"])


def truth(name, tag, q, ci):
    return FIX["%s/%s_%s" % (name, tag, q)][ci]


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def crowd():
    """n789's light curve at positions 0, 5 and 10 of 11 on its sampling, 300 frequencies from far below 1 / T_span-wide
    windows to beyond the mean Nyquist rate, 16 centres inside, in the widest gap of and outside the span"""
    t, y, dy = (LS["n789/" + k] for k in ("t", "y", "dy"))
    rng = np.random.default_rng(11)
    Y = y[None, :] + 0.3 * rng.standard_normal((11, len(t)))
    DY = np.tile(dy, (11, 1)) * rng.uniform(0.5, 2.0, size=(11, 1))
    for m in (0, 5, 10):
        Y[m], DY[m] = y, dy
    span = t[-1] - t[0]
    f300 = np.geomspace(1.0 / span, 1.2 * 0.5 * len(t) / span, 300)
    gap = int(np.argmax(np.diff(t)))
    taus = np.concatenate([t[0] + span * np.linspace(0.02, 0.98, 13), [0.5 * (t[gap] + t[gap + 1]), t[0] - 0.01 * span, t[-1] + 0.03 * span]])
    return t, y, dy, Y, DY, f300, taus


def test_accuracy_against_the_50_digit_truth(eng):
    worst, left_out = {}, 0
    for name in CASES:
        t, y, dy, f, taus = case(name)
        n = len(t)
        eng.set_lightcurves(t, y, dy)
        for tag, weighted in (("w", True), ("u", False)):
            rho, rho_a = float(FIX["%s/%s_rho" % (name, tag)]), float(FIX["%s/%s_rho_a" % (name, tag)])
            for ci, c in enumerate(DECAYS):
                P, Z, A, ne, vx, kappa = (truth(name, tag, q, ci) for q in ("power", "z", "amplitude", "neff", "vx", "kappa"))
                keep = ne >= 4.0
                assert keep.mean() >= 0.5
                got_p, got_n = eng.wwz(f, taus, decay=c, statistic="power", weighted=weighted, neff=True)
                got_z = eng.wwz(f, taus, decay=c, statistic="z", weighted=weighted)
                got_a = eng.wwz(f, taus, decay=c, statistic="amplitude", weighted=weighted)
                for q, got in (("power", got_p), ("z", got_z), ("amplitude", got_a), ("neff", got_n)):
                    # every entry, the left-out ones included, is finite or NaN; N_eff is a number everywhere
                    assert got.shape == (1, len(taus), len(f)) and not np.any(np.isinf(got)), (name, tag, c, q)
                assert np.all(np.isfinite(got_n)), (name, tag, c)
                left_out += int(np.sum(~keep))
                k = np.where(keep, kappa, 1.0)
                ratios = {
                    "power": np.abs(got_p[0] - P) / wn.bound_power(rho, n, k),
                    "neff": np.abs(got_n[0] - ne) / (wn.bound_neff_rel(n) * ne),
                    "z": np.abs(got_z[0] - Z) / wn.bound_z(rho, n, k, np.where(keep, P, 0.0), ne),
                    "amplitude": np.abs(got_a[0] - A) / wn.bound_amplitude(rho_a, n, k, vx),
                }
                for q, r in ratios.items():
                    assert np.all(np.isfinite(r[keep])), (name, tag, c, q)
                    worst[(name, tag, "%.3g" % c, q)] = float(np.max(r[keep]))
                print("%-8s %s c %-8.3g |x - truth| / bound: %s" % (name, tag, c, "  ".join("%s %.3f" % (q, np.max(r[keep])) for q, r in ratios.items())))
    assert "mtg_wwz_kernel" in eng.last_solver and eng.last_kernel_ms > 0
    assert left_out > 0      # (the fixture has such entries: the check above is not empty)
    print("largest ratio to the bound: %.3f at %s" % (max(worst.values()), max(worst, key=worst.get)))
    assert max(worst.values()) <= 1.0, {k: v for k, v in worst.items() if v > 1.0}


def test_centres_in_a_gap_and_outside_the_span_stay_in_range(eng):
    # without the rescaling by the largest weight every weight underflows there: 0 / 0
    for name in ("n789", "n216"):
        t, y, dy, f, taus = case(name)
        n = len(t)
        eng.set_lightcurves(t, y, dy)
        gap = int(np.argmax(np.diff(t)))
        far = np.array([0.5 * (t[gap] + t[gap + 1]), t[-1] + 0.5 * (t[-1] - t[0])])
        high = f[-3:] * 40.0     # ~ 30 cycles and more to the nearest sample: exp(-z^2 / 2) is below 1e-195, its square 0
        assert np.all(np.exp(-0.5 * (np.min(np.abs(t[None, :] - far[:, None]), axis=1)[:, None] * high[None, :]) ** 2) ** 2 == 0.0)
        for weighted in (True, False):
            for stat in ("power", "z", "amplitude"):
                v, ne = eng.wwz(high, np.concatenate([taus[6:], far]), statistic=stat, weighted=weighted, neff=True)
                assert np.all(np.isfinite(ne)) and np.all(ne >= 1.0 - wn.bound_neff_rel(n)) and np.all(ne <= n), (name, weighted, stat)
                assert not np.any(np.isinf(v)), (name, weighted, stat)
            # the sums themselves are finite: the values at the fixture's own highest frequencies are numbers
            v = eng.wwz(f[-3:], taus[6:], statistic="power", weighted=weighted)
            assert np.all(np.isfinite(v)), (name, weighted)


def test_no_window_is_the_lomb_scargle_power(eng):
    for name in CASES:
        t, y, dy, f, taus = case(name)
        n = len(t)
        eng.set_lightcurves(t, y, dy)
        for tag, weighted in (("w", True), ("u", False)):
            ci = DECAYS.index(0.0)
            b_ls = max(10.0 * float(LS["%s/%s_rho" % (name, tag)]), 64.0 * np.sqrt(n) * U)
            b = wn.bound_power(float(FIX["%s/%s_rho" % (name, tag)]), n, truth(name, tag, "kappa", ci)) + b_ls
            p, ne = eng.wwz(f, taus, decay=0.0, statistic="power", weighted=weighted, neff=True)
            ls = eng.lomb_scargle(f, normalization="standard", weighted=weighted)[0]
            assert np.all(np.abs(p[0] - ls[None, :]) <= b), (name, tag)
            if not weighted:   # (weighted, N_eff = (sum s)^2 / sum s^2 is not N: held against the truth below)
                assert np.all(np.abs(ne - n) <= wn.bound_neff_rel(n) * n), name
            assert np.all(np.abs(ne[0] - truth(name, tag, "neff", ci)) <= wn.bound_neff_rel(n) * truth(name, tag, "neff", ci))


def test_an_entry_depends_on_its_own_light_curve_frequency_and_centre_alone(eng, crowd):
    t, y, dy, Y, DY, f300, taus = crowd
    rng = np.random.default_rng(3)
    fperm, tperm = rng.permutation(300), rng.permutation(16)
    for weighted in (True, False):
        for stat in ("z", "power"):
            eng.set_lightcurves(t, y, dy)
            alone, alone_n = eng.wwz(f300, taus, statistic=stat, weighted=weighted, neff=True)
            assert alone.shape == (1, 16, 300)
            # whole chunks are cut at the higher frequencies (N = 789: three chunks and a ragged one)
            # L = 1 against members 0, 5 and 10 of L = 11 (full tiles and a partly filled one)
            eng.set_lightcurves(t, Y, DY)
            among, among_n = eng.wwz(f300, taus, statistic=stat, weighted=weighted, neff=True)
            for m in (0, 5, 10):
                assert np.array_equal(among[m], alone[0], equal_nan=True), (weighted, stat, m)
                assert np.array_equal(among_n[m], alone_n[0]), (weighted, stat, m)
            # permuted frequencies and centres
            shuffled = eng.wwz(f300[fperm], taus[tperm], statistic=stat, weighted=weighted)
            assert np.array_equal(shuffled, among[:, tperm][:, :, fperm], equal_nan=True), (weighted, stat)
            # a frequency alone in its call against the same one among 299 others, much lower ones included: the
            # workgroup's range of chunks is then another
            for k in (0, 63, 64, 255, 256, 299):
                one = eng.wwz(f300[k:k + 1], taus, statistic=stat, weighted=weighted)
                assert np.array_equal(one[:, :, 0], among[:, :, k], equal_nan=True), (weighted, stat, k)
            # T = 1 against T = 16
            for j in (0, 13, 15):
                one = eng.wwz(f300, taus[j:j + 1], statistic=stat, weighted=weighted)
                assert np.array_equal(one[:, 0], among[:, j], equal_nan=True), (weighted, stat, j)
            # the same times stored per light curve
            eng.set_lightcurves(np.tile(t, (11, 1)), Y, DY)
            per_lc, per_lc_n = eng.wwz(f300, taus, statistic=stat, weighted=weighted, neff=True)
            assert np.array_equal(per_lc, among, equal_nan=True) and np.array_equal(per_lc_n, among_n), (weighted, stat)
    # the default decay really cuts whole chunks at the top of this grid: far fewer than all samples carry weight
    assert np.all(alone_n[0, :13, -1] < 20)


def test_more_than_one_slab(eng):
    # T F = 2^22 entries per light curve: slabs of 2^25 / 2^22 = 8 light curves, so L = 9 is 8 + 1; peaks only -- nothing
    # of size L T F comes to the host.  N = 8 keeps the work small.
    t, y, dy = (LS["n52/" + k][:8] for k in ("t", "y", "dy"))
    rng = np.random.default_rng(5)
    Y = y[None, :] + 0.2 * rng.standard_normal((9, 8))
    span = t[-1] - t[0]
    f = np.geomspace(0.5 / span, 4.0 / span, 1 << 18)
    taus = t[0] + span * np.linspace(0.0, 1.0, 16)
    for weighted in (True, False):
        for times in (t, np.tile(t, (9, 1))):
            eng.set_lightcurves(times, Y, np.tile(dy, (9, 1)))
            peak, at = eng.wwz(f, taus, statistic="power", weighted=weighted, values=False, peak=True)
            eng.set_lightcurves(t, Y[8], dy)
            last, last_p, last_at = eng.wwz(f, taus, statistic="power", weighted=weighted, peak=True)
            assert last_p[0] == np.nanmax(last[0]) and last_at[0] == int(np.nanargmax(last[0].ravel()))
            assert peak[8] == last_p[0] and at[8] == last_at[0], (weighted, np.ndim(times))
            eng.set_lightcurves(t, Y[3], dy)
            mid_p, mid_at = eng.wwz(f, taus, statistic="power", weighted=weighted, values=False, peak=True)
            assert peak[3] == mid_p[0] and at[3] == mid_at[0], (weighted, np.ndim(times))


def test_peaks_are_max_and_first_argmax(eng):
    t, y, dy, f, taus = case("n52")
    rng = np.random.default_rng(5)
    Y = y[None, :] + 0.5 * rng.standard_normal((7, len(t)))
    eng.set_lightcurves(t, Y, np.tile(dy, (7, 1)))
    # every centre twice: the first of the ties is reported
    tt = np.concatenate([taus, taus])
    for stat in ("z", "power", "amplitude"):
        for weighted in (True, False):
            m, peak, at = eng.wwz(f, tt, statistic=stat, weighted=weighted, peak=True)
            flat = m.reshape(7, -1)
            assert np.array_equal(peak, np.nanmax(flat, axis=1)) and np.array_equal(at, np.nanargmax(flat, axis=1))
            assert np.all(at < len(taus) * len(f))
            peak2, at2 = eng.wwz(f, tt, statistic=stat, weighted=weighted, values=False, peak=True)
            assert np.array_equal(peak2, peak) and np.array_equal(at2, at)
    # a map of nothing but NaN: four equal samples' worth of design (every cos and sin the same) has no determinant
    t4 = np.array([0.0, 1.0, 2.0, 3.0])
    eng.set_lightcurves(t4, np.array([1.0, 2.0, 0.5, 1.5]), np.ones(4))
    m, peak, at = eng.wwz([1.0, 2.0], [0.0, 1.0], decay=0.0, peak=True)
    assert np.all(np.isnan(m)) and np.isnan(peak[0]) and at[0] == -1


def test_errors_and_a_working_context_afterwards(eng):
    t, y, dy, f, taus = case("n52")
    fresh = Engine(0)
    try:
        with pytest.raises(EngineError) as exc:
            fresh.wwz([0.1], [0.0])
        assert exc.value.code == engine.E_STATE
        t3 = np.array([0.0, 1.0, 2.5])
        fresh.set_lightcurves(t3, np.array([1.0, 2.0, 0.5]), np.ones(3))
        with pytest.raises(EngineError) as exc:
            fresh.wwz([0.1], [0.0])
        assert exc.value.code == engine.E_ARG and "N = 3" in str(exc.value)
        fresh.set_lightcurves(t, y, dy)
        eng.set_lightcurves(t, y, dy)
        before = fresh.wwz(f, taus)
        assert np.array_equal(before, eng.wwz(f, taus), equal_nan=True)
        bad_calls = [
            (dict(freqs=[], taus=taus), "F >= 1"), (dict(freqs=f, taus=[]), "T >= 1"),
            (dict(freqs=[0.1, np.nan], taus=taus), "freqs[1]"), (dict(freqs=[np.inf], taus=taus), "freqs[0]"),
            (dict(freqs=[0.0], taus=taus), "freqs[0]"), (dict(freqs=[-1.0], taus=taus), "freqs[0]"),
            (dict(freqs=f, taus=[0.0, np.nan]), "taus[1]"), (dict(freqs=f, taus=[np.inf]), "taus[0]"),
            (dict(freqs=f, taus=taus, decay=-1e-3), "decay"), (dict(freqs=f, taus=taus, decay=np.nan), "decay"),
            (dict(freqs=f, taus=taus, decay=np.inf), "decay"), (dict(freqs=f, taus=taus, statistic=3), "statistic 3"),
            (dict(freqs=f, taus=taus, statistic=-1), "statistic -1"),
        ]
        for kwargs, word in bad_calls:
            with pytest.raises(EngineError) as exc:
                fresh.wwz(**kwargs)
            assert exc.value.code == engine.E_ARG and word in str(exc.value), kwargs
        # Engine.wwz's own checks: an unknown statistic by name, and nothing asked for
        with pytest.raises(ValueError, match="statistic"):
            fresh.wwz(f, taus, statistic="psd")
        with pytest.raises(ValueError, match="nothing asked for"):
            fresh.wwz(f, taus, values=False, neff=False, peak=False)
        # every output NULL, and L T F beyond int64 (nothing that large is touched), straight through the C entry
        lib, ctx = fresh._lib, fresh._ctx
        fp, tp = engine._ptr(np.ascontiguousarray(f)), engine._ptr(np.ascontiguousarray(taus))
        assert lib.mtg_wwz(ctx, len(f), fp, len(taus), tp, engine.WWZ_DECAY, engine.WWZ_Z, 1, None, None, None, None) == engine.E_ARG
        assert b"NULL" in lib.mtg_last_error(ctx)
        pk = np.zeros(1)
        assert lib.mtg_wwz(ctx, 1 << 40, fp, 1 << 30, tp, engine.WWZ_DECAY, engine.WWZ_Z, 1, None, None, engine._ptr(pk), None) == engine.E_ARG
        assert b"int64" in lib.mtg_last_error(ctx)
        assert np.array_equal(fresh.wwz(f, taus), before, equal_nan=True)
    finally:
        fresh.close()


def test_periodogram_class_shapes(eng):
    t, y, dy, f, taus = case("n52")
    one = periodogram.WWZ(t, y, dy)
    m = one.power(f, taus)
    assert m.shape == (len(taus), len(f)) and one.neff(f, taus).shape == m.shape
    assert np.array_equal(m, periodogram.WWZ(t, y, dy, statistic="power").power(f, taus, statistic="z"), equal_nan=True)
    Y = np.stack([y, y[::-1], 2.0 * y])
    many = periodogram.WWZ(t, Y)           # dy=None: unweighted
    mm = many.power(f[:5], many.autotau(7))
    assert mm.shape == (3, 7, 5) and many.neff(f[:5], many.autotau(7)).shape == (3, 7, 5)
    assert np.array_equal(mm[0], periodogram.WWZ(t, y).power(f[:5], many.autotau(7)), equal_nan=True)
    ff, tt, auto = one.autopower(n_tau=4, samples_per_peak=1, nyquist_factor=1)
    assert auto.shape == (4, len(ff)) and len(tt) == 4


def test_peak_test_with_the_wwz_statistic_reproduces_for_a_seed():
    from mind_the_gaps_amd import ppp
    from mind_the_gaps_amd import synthetic as synth
    from mind_the_gaps_amd.lightcurves import GappyLightcurve
    from mind_the_gaps_amd.models import DampedRandomWalk
    th = synth.truth(synth.ALT_MODEL)
    times, rates, err = synth.make_lightcurves(60, 1, seed=43)
    T = times[-1] - times[0]
    # a sinusoid that lasts for the second half of the light curve only
    burst = 2.0 * err[0] * np.sin(2.0 * np.pi * 6.0 / T * times) * (times > times[0] + 0.5 * T)
    lc = GappyLightcurve(times, rates[0] + 50.0 + burst, err[0], exposures=0.5 * np.diff(times).min())
    freqs = np.linspace(2.0 / T, 12.0 / T, 12)
    taus = times[0] + T * np.linspace(0.1, 0.9, 6)

    def null():
        return DampedRandomWalk(th[0], th[1], bounds=[(-10, 50), (-10, 10)])
    kw = dict(nsims=6, walkers=8, max_steps=60, sigma_noise=0.5, seed=21)
    a = ppp.periodogram_peak_test(lc, null(), freqs, statistic="wwz", taus=taus, **kw)
    b = ppp.periodogram_peak_test(lc, null(), freqs, statistic="wwz", taus=taus, **kw)
    assert 0.0 <= a["p_value"] <= 1.0 and a["p_value"] == b["p_value"] and np.array_equal(a["sim_peaks"], b["sim_peaks"])
    assert a["observed_peak"] == b["observed_peak"] and len(a["sim_peaks"]) == 6
    assert a["observed_frequency"] in freqs and a["observed_tau"] in taus
    with pytest.raises(ValueError):
        ppp.periodogram_peak_test(lc, null(), freqs, statistic="wwz", nterms=2, **kw)
