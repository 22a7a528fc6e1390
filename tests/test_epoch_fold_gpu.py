"""mtg_epoch_fold and mtg_phase_fold on the GPU (include/mtg.h): the epoch-folding periodogram of the resident light curves
and the folded profiles behind it.

Accuracy is held against the 50-digit truth of tests/golden/epoch_fold_golden.npz (scripts/make_epoch_fold_golden.py; bins
from rational arithmetic): standard power within max(10 rho, 64 sqrt(N) u), u = 2^-53, rho the error of the float64 helper
tests/epoch_fold_numpy.py on the same case; the other normalisations within that times |dP/dp| at the truth.  The bins
are exact: the counts equal the fixture's as integers, the `edges` case included.  Consistency with mtg_phase_fold and
the independence properties of the header are bit for bit.
"""
import os

import numpy as np
import pytest

import epoch_fold_numpy as efn
from mind_the_gaps_amd import engine
from mind_the_gaps_amd.engine import Engine, EngineError

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = np.load(os.path.join(HERE, "golden", "epoch_fold_golden.npz"))
LS = np.load(os.path.join(HERE, "golden", "lomb_scargle_golden.npz"))
CASES = ("n5", "n52", "n216", "n789", "fast216")
ALL_CASES = CASES + ("edges", "edges_neg")
U = 2.0 ** -53


def case(name):
    """t, y, dy, freqs, time_0, nbins"""
    if name.startswith("edges"):
        return tuple(FIX["edges/" + k] for k in ("t", "y", "dy", "freqs")) + (float(FIX[name + "/time_0"]), (2, 8, 10, 32))
    t, y, dy = (LS["%s/%s" % (name, k)] for k in ("t", "y", "dy"))
    return t, y, dy, LS[name + "/freqs"][FIX[name + "/freq_index"]], float(FIX[name + "/time_0"]), (2, 10, 32)


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def test_accuracy_against_the_50_digit_truth(eng):
    worst = {}
    for name in ALL_CASES:
        t, y, dy, f, time_0, nbins = case(name)
        eng.set_lightcurves(t, y, dy)
        for tag, weighted in (("w", True), ("u", False)):
            b = efn.bound(float(FIX["%s/%s_rho" % (name, tag)]), len(t))
            _, _, _, YY, sw = efn.weights(y, dy, weighted)
            for nb in nbins:
                std = FIX["%s/nb%d/%s_standard" % (name, nb, tag)]
                for norm in efn.NORMALIZATIONS:
                    got = eng.epoch_fold(f, nbins=nb, time_0=time_0, normalization=norm, weighted=weighted)[0]
                    want = FIX["%s/nb%d/%s_%s" % (name, nb, tag, norm)]
                    with np.errstate(divide="ignore", invalid="ignore"):
                        err = np.abs(got - want) / (b * efn.dnorm_dstandard(std, YY, sw, norm))
                    err[got == want] = 0.0
                    # a profile that explains everything (standard power 1 as a double): model and log diverge there, and so
                    # must the device's -- a standard power within b of 1 gives |model| >= (1 - b) / b and log >= -log(b),
                    # or NaN where rounding took p past YY
                    full = std == 1.0
                    if norm == "model":
                        assert np.all(np.isnan(got[full]) | (np.abs(got[full]) >= (1.0 - b) / b)), (name, tag, nb)
                        err[full] = 0.0
                    if norm == "log":
                        assert np.all(np.isnan(got[full]) | (got[full] >= -np.log(b))), (name, tag, nb)
                        err[full] = 0.0
                    worst[(name, tag, nb, norm)] = float(np.max(err))
    assert "mtg_epoch_fold_kernel" in eng.last_solver and "lanes" in eng.last_solver and eng.last_kernel_ms > 0
    print("largest ratio to the bound: %.3f at %s" % (max(worst.values()), max(worst, key=worst.get)))
    assert max(worst.values()) <= 1.0, {k: v for k, v in worst.items() if not v <= 1.0}


def test_bins_are_exact(eng):
    differing = 0
    for name in ALL_CASES:
        t, y, dy, f, time_0, nbins = case(name)
        eng.set_lightcurves(t, y, dy)
        for nb in nbins:
            fold = eng.phase_fold(f, nbins=nb, time_0=time_0)
            assert fold.count.dtype == np.int64 and fold.count.shape == (1, len(f), nb)
            differing += int(np.sum(fold.count[0] != FIX["%s/nb%d/count" % (name, nb)]))
            filled = fold.count[0] > 0
            assert np.all(fold.wsum[0][filled] > 0) and np.all(fold.wsum[0][~filled] == 0) and np.all(fold.wrsum[0][~filled] == 0)
    # products just below zero, where nbins frac is just below nbins: the last bin
    t = np.array([-1e-18, -1e-20, -1e-300, 0.0, 1e-300, 1e-20, 0.3, 1.7, 2.9])
    f = np.array([1.0, 0.7, 3.0])
    eng.set_lightcurves(t, np.arange(9.0), np.ones(9))
    for nb in (2, 8, 10, 32):
        want = np.array([np.bincount(efn.exact_bins(v, t, nb), minlength=nb) for v in f])
        assert want[0, nb - 1] >= 3 and np.array_equal(efn.bins(1.0, t, nb), efn.exact_bins(1.0, t, nb))
        differing += int(np.sum(eng.phase_fold(f, nbins=nb, time_0=0.0).count[0] != want))
    assert differing == 0


def test_epoch_fold_is_the_formula_on_phase_fold_bit_for_bit(eng):
    # psd = p (sw / 2) is p itself wherever the factor is exact to form on the host as the device forms it: sw = N
    # unweighted (any N: one product, one rounding on both sides), and weighted with every light curve's dy a constant
    # power of two and N = 512 -- sum sigma^-2 is then a power of two in whatever order it is summed.  Shared sampling,
    # 300 frequencies (256 lanes), nbins 2, 8, 10, 32: tiles of 4, 2 and 1 light curves per lane in either weighting.
    t, y, dy, _, time_0, _ = case("n789")
    f = LS["n789/freqs"][:300]
    rng = np.random.default_rng(11)
    Y = y[None, :] + 0.3 * rng.standard_normal((5, len(t)))
    for n, DY in ((512, np.repeat(np.array([[0.25], [0.5], [1.0], [2.0], [4.0]]), 512, axis=1)),
                  (len(t), np.tile(dy, (5, 1)) * rng.uniform(0.5, 2.0, size=(5, 1)))):
        eng.set_lightcurves(t[:n], Y[:, :n], DY)
        for weighted in ((True, False) if n == 512 else (False,)):
            sw = np.sum(1.0 / DY ** 2, axis=1) if weighted else np.full(5, float(n))
            tiles = set()
            for nb in (2, 8, 10, 32):
                fold = eng.phase_fold(f, nbins=nb, time_0=time_0, weighted=weighted)
                psd = eng.epoch_fold(f, nbins=nb, time_0=time_0, normalization="psd", weighted=weighted)
                tiles.add(int(eng.last_solver.split("<")[1].split(",")[0]))
                assert np.array_equal(psd, efn.reduce_bins(fold.wsum, fold.wrsum) * (0.5 * sw[:, None])), (n, weighted, nb)
                assert np.array_equal(eng.epoch_fold(f, nbins=nb, time_0=time_0, normalization="chi2", weighted=weighted), 2.0 * psd)
                assert np.all(np.abs(np.sum(fold.wsum, axis=2) - 1.0) <= 8 * np.sqrt(n) * U)
            assert tiles == {1, 2, 4}, (weighted, tiles)


@pytest.mark.parametrize("nb", (2, 32))
def test_power_depends_on_its_own_light_curve_and_frequency_alone(eng, nb):
    t, y, dy, _, time_0, _ = case("n789")
    f = LS["n789/freqs"]
    rng = np.random.default_rng(3)
    Y = y[None, :] + 0.3 * rng.standard_normal((11, len(t)))
    DY = np.tile(dy, (11, 1)) * rng.uniform(0.5, 2.0, size=(11, 1))
    for m in (0, 5, 10):
        Y[m], DY[m] = y, dy
    perm = rng.permutation(300)
    f300 = f[:300]
    kw = dict(nbins=nb, time_0=time_0)
    for weighted in (True, False):
        eng.set_lightcurves(t, y, dy)
        alone = eng.epoch_fold(f300, weighted=weighted, **kw)[0]
        eng.set_lightcurves(t, Y, DY)
        among = eng.epoch_fold(f300, weighted=weighted, **kw)
        for m in (0, 5, 10):
            assert np.array_equal(among[m], alone), (weighted, m)
        eng.set_lightcurves(np.tile(t, (11, 1)), Y, DY)
        per_lc = eng.epoch_fold(f300, weighted=weighted, **kw)
        assert np.array_equal(per_lc, among), weighted
        shuffled = eng.epoch_fold(f300[perm], weighted=weighted, **kw)
        assert np.array_equal(shuffled, among[:, perm]), weighted
        for k in (0, 63, 64, 255, 256, 299):
            one = eng.epoch_fold(f300[k:k + 1], weighted=weighted, **kw)
            assert np.array_equal(one[:, 0], among[:, k]), (weighted, k)


@pytest.mark.parametrize("n", (255, 256, 257, 513))
def test_chunk_edges(eng, n):
    t, y, dy, f, time_0, nbins = case("n789")
    t, y, dy = t[:n], y[:n], dy[:n]
    eng.set_lightcurves(t, y, dy)
    b = 64.0 * np.sqrt(n) * U
    for weighted in (True, False):
        for nb in nbins:
            got = eng.epoch_fold(f, nbins=nb, time_0=time_0, weighted=weighted)[0]
            assert np.max(np.abs(got - efn.power(t, y, dy, f, nb, time_0, weighted))) <= b, (weighted, nb)
            assert np.array_equal(eng.phase_fold(f, nbins=nb, time_0=time_0).count[0],
                                  np.array([np.bincount(efn.bins(v, t - time_0, nb), minlength=nb) for v in f]))


def test_slabs_with_a_start_row_above_zero(eng):
    # F = 2^21: slabs of 2^25 / F = 16 light curves, so L = 17 is 16 + 1; a power does not depend on F or L, so the big
    # call equals, bit for bit, a small one at a sample of its frequencies
    rng = np.random.default_rng(17)
    t = np.array([0.0, 0.9, 2.3, 3.1, 4.6, 5.2])
    Y, DY = rng.normal(5.0, 1.0, (17, 6)), rng.uniform(0.5, 1.5, (17, 6))
    f = np.linspace(0.05, 3.0, 1 << 21)
    index = np.unique(rng.integers(0, len(f), 64))
    eng.set_lightcurves(t, Y, DY)
    for weighted in (True, False):
        power, peak, at = eng.epoch_fold(f, nbins=4, weighted=weighted, peak=True)
        assert np.array_equal(power[:, index], eng.epoch_fold(f[index], nbins=4, weighted=weighted))
        assert np.array_equal(peak, power.max(axis=1)) and np.array_equal(at, power.argmax(axis=1))
        assert np.max(np.abs(power[16, index] - efn.power(t, Y[16], DY[16], f[index], 4, 0.0, weighted))) <= 64 * np.sqrt(6) * U


def test_noise_free_square_wave(eng):
    nb, N = 8, 216
    t = np.arange(N) * 0.37 + 0.011          # phases at f0 fall inside the bins, away from their edges
    f = np.linspace(0.05, 1.0, 300)
    f0 = f[97]
    phase = t * f0 % 1                       # folded from time_0 = 0
    assert np.min(np.abs(phase * nb - np.round(phase * nb))) > 1e-6
    y = np.where(phase < 0.5, 3.0, 1.0)      # edges on bin edges 0 and 4 of 8
    eng.set_lightcurves(t, y, np.full(N, 0.1))
    for weighted in (True, False):
        p, peak, at = eng.epoch_fold(f, nbins=nb, time_0=0.0, weighted=weighted, peak=True)
        assert abs(p[0, 97] - 1.0) <= 64.0 * np.sqrt(N) * U and at[0] == 97 and peak[0] == p[0, 97]
        shifted = eng.epoch_fold(f[97:98], nbins=nb, time_0=0.5 / (nb * f0), weighted=weighted)
        assert shifted[0, 0] < p[0, 97]


def test_peaks_and_a_constant_light_curve(eng):
    t, y, dy, _, time_0, _ = case("n52")
    f = LS["n52/freqs"]
    rng = np.random.default_rng(5)
    Y = y[None, :] + rng.standard_normal((9, len(t)))
    eng.set_lightcurves(t, Y, np.tile(dy, (9, 1)))
    for nb in (2, 10, 32):
        power, peak, at = eng.epoch_fold(f, nbins=nb, peak=True)
        assert np.array_equal(peak, power.max(axis=1)) and np.array_equal(at, power.argmax(axis=1))
        peak2, at2 = eng.epoch_fold(f, nbins=nb, power=False, peak=True)
        assert np.array_equal(peak2, peak) and np.array_equal(at2, at)
    # YY = 0: what lomb_scargle does on the same input
    eng.set_lightcurves(np.arange(64.0), np.full(64, 3.0), np.ones(64))
    f = np.linspace(0.01, 0.4, 70)
    for weighted in (True, False):
        ls, ls_peak, ls_at = eng.lomb_scargle(f, weighted=weighted, peak=True)
        ef, ef_peak, ef_at = eng.epoch_fold(f, weighted=weighted, peak=True)
        assert np.array_equal(np.isnan(ef), np.isnan(ls)) and np.array_equal(ef_at, ls_at)
        assert np.array_equal(np.isnan(ef_peak), np.isnan(ls_peak))


def test_errors_leave_the_context_working(eng):
    t, y, dy, f, time_0, _ = case("n52")
    want = FIX["n52/nb10/w_standard"]
    b = efn.bound(float(FIX["n52/w_rho"]), len(t))
    lib, ctx = eng._lib, eng._ctx

    def still_good():
        assert np.max(np.abs(eng.epoch_fold(f, nbins=10, time_0=time_0)[0] - want)) <= b

    fresh = Engine(0)
    for call in (lambda: fresh.epoch_fold(f, time_0=0.0), lambda: fresh.phase_fold(f, time_0=0.0)):
        with pytest.raises(EngineError) as err:
            call()
        assert err.value.code == engine.E_STATE
    fresh.close()
    eng.set_lightcurves(t, y, dy)
    still_good()
    bad = [dict(freqs=[]), dict(freqs=[0.1, np.nan]), dict(freqs=[0.1, np.inf]), dict(freqs=[0.0]), dict(freqs=[-0.1]),
           dict(nbins=1), dict(nbins=33), dict(time_0=np.nan), dict(time_0=np.inf), dict(normalization=7), dict(normalization=-1),
           dict(power=False, peak=False)]
    for kw in bad:
        args = dict(freqs=f, nbins=10, time_0=time_0)
        args.update(kw)
        with pytest.raises(EngineError) as err:
            eng.epoch_fold(**args)
        assert err.value.code == engine.E_ARG, kw
        still_good()
    for kw in (dict(freqs=[]), dict(freqs=[0.1, np.nan]), dict(freqs=[0.1, np.inf]), dict(freqs=[0.0]), dict(freqs=[-1.0]), dict(nbins=1),
               dict(nbins=33), dict(time_0=np.nan), dict(time_0=np.inf)):
        args = dict(freqs=f, nbins=10, time_0=time_0)
        args.update(kw)
        with pytest.raises(EngineError) as err:
            eng.phase_fold(**args)
        assert err.value.code == engine.E_ARG, kw
        still_good()
    # all outputs NULL, and more than the workspace bound (L F nbins > 2^23)
    fp = np.ascontiguousarray(f)
    assert lib.mtg_phase_fold(ctx, len(fp), engine._ptr(fp), 10, time_0, 1, None, None, None, None) == engine.E_ARG
    big = np.linspace(0.1, 1.0, (1 << 23) // 32 + 1)
    with pytest.raises(EngineError) as err:
        eng.phase_fold(big, nbins=32, time_0=time_0)
    assert err.value.code == engine.E_ARG and "exceeds" in str(err.value)
    still_good()
    # N < 2
    eng.set_lightcurves(t[:1], y[:1], dy[:1])
    for call in (lambda: eng.epoch_fold(f, time_0=time_0), lambda: eng.phase_fold(f, time_0=time_0)):
        with pytest.raises(EngineError) as err:
            call()
        assert err.value.code == engine.E_ARG
    eng.set_lightcurves(t, y, dy)
    still_good()


def test_periodogram_phase_fold_is_the_reference_formula(eng):
    from mind_the_gaps_amd import periodogram
    t, y, dy, f, _, _ = case("n216")
    time_0 = 0.0
    k = next(k for k in range(len(f)) if np.array_equal(efn.rounded_bins(f[k], t - time_0, 10), efn.bins(f[k], t - time_0, 10)))
    means, stds, phases = periodogram.phase_fold(t, y, f[k], dy=dy, time_0=time_0, n_bins=10)
    b = np.floor((((t - time_0) * f[k]) % 1) * 10).astype(int)
    tol = 64 * np.sqrt(len(t)) * U * np.max(np.abs(y))
    for i in range(10):
        assert abs(means[i] - y[b == i].mean()) <= tol and abs(stds[i] - np.sqrt(np.sum(dy[b == i] ** 2)) / np.sum(b == i)) <= tol
    assert np.array_equal(means[:10], means[10:]) and np.array_equal(phases, np.hstack([(np.arange(10) + 0.5) / 10, (np.arange(10) + 0.5) / 10 + 1]))
    # empty bins: NaN (5 samples in 32 bins)
    t5, y5, dy5 = (LS["n5/" + v] for v in ("t", "y", "dy"))
    means, stds, _ = periodogram.phase_fold(t5, y5, 0.37, dy=dy5, time_0=t5[0], n_bins=32)
    empty = np.bincount(efn.bins(0.37, t5 - t5[0], 32), minlength=32) == 0
    assert empty.any() and np.array_equal(np.isnan(means[:32]), empty) and np.array_equal(np.isnan(stds[:32]), empty)
    ef = periodogram.EpochFolding(t, y, dy, nbins=10)
    assert np.array_equal(ef.power(f), periodogram.EpochFolding(t, y[None, :], dy, nbins=10, time_0=t[0]).power(f)[0])
    assert np.array_equal(ef.autofrequency(), periodogram.LombScargle(t, y, dy).autofrequency())


def test_periodogram_peak_test_with_epoch_folding():
    from mind_the_gaps_amd import ppp
    from mind_the_gaps_amd import synthetic as synth
    from mind_the_gaps_amd.lightcurves import GappyLightcurve
    from mind_the_gaps_amd.models import DampedRandomWalk
    th = synth.truth(synth.ALT_MODEL)
    times, rates, err = synth.make_lightcurves(60, 1, seed=43)
    T = times[-1] - times[0]
    f0 = 6.0 / T
    dips = -3.0 * err[0] * (((times - times[0]) * f0) % 1 < 0.15)      # a dip train of 15 % duty cycle
    lc = GappyLightcurve(times, rates[0] + 50.0 + dips, err[0], exposures=0.5 * np.diff(times).min())
    freqs = np.linspace(1.0 / T, 20.0 / T, 12)

    def null():
        return DampedRandomWalk(th[0], th[1], bounds=[(-10, 50), (-10, 10)])
    kw = dict(nsims=6, walkers=8, max_steps=60, sigma_noise=0.5, seed=21)
    a = ppp.periodogram_peak_test(lc, null(), freqs, statistic="epoch_fold", nbins=10, **kw)
    b = ppp.periodogram_peak_test(lc, null(), freqs, statistic="epoch_fold", nbins=10, **kw)
    assert 0.0 <= a["p_value"] <= 1.0 and a["p_value"] == b["p_value"] and np.array_equal(a["sim_peaks"], b["sim_peaks"])
    assert a["observed_peak"] == b["observed_peak"] and len(a["sim_peaks"]) == 6
    with pytest.raises(ValueError):
        ppp.periodogram_peak_test(lc, null(), freqs, statistic="epoch_fold", nterms=2, **kw)
    c = ppp.periodogram_peak_test(lc, null(), freqs, **kw)
    d = ppp.periodogram_peak_test(lc, null(), freqs, statistic="lomb_scargle", **kw)
    assert c["p_value"] == d["p_value"] and np.array_equal(c["sim_peaks"], d["sim_peaks"]) and c["observed_peak"] == d["observed_peak"]
