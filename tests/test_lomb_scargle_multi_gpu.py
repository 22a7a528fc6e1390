"""mtg_lomb_scargle_multi and mtg_lomb_scargle_envelope_multi on the GPU (include/mtg.h): the Lomb-Scargle periodogram
with K phase-tied harmonics per frequency, astropy's LombScargle(nterms=K) in its chi2 form.

Accuracy is held against the 50-digit truths of tests/golden/lomb_scargle_multi_golden.npz
(scripts/make_lomb_scargle_multi_golden.py) on the inputs of tests/golden/lomb_scargle_golden.npz: the standard power
within max(10 rho, 64 sqrt(N) u kappa) entry by entry, u = 2^-53, rho the error of plain numpy float64
(tests/lomb_scargle_multi_numpy.py) on the same case, kappa the 2-norm condition number of that entry's
A = sum w x x^T -- the project's bound with the condition number of the solve in it; the other normalisations within the
same bound times |dP/dp| at the truth.  Measured on an MI355X the largest ratio to the bound is 0.003 (n52,
weighted, K = 2).  The independence properties of the header are bit for bit.
"""
import ctypes
import os

import numpy as np
import pytest

import lomb_scargle_multi_numpy
from mind_the_gaps_amd import engine
from mind_the_gaps_amd.engine import Engine, EngineError

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = np.load(os.path.join(HERE, "golden", "lomb_scargle_golden.npz"))
FIX = np.load(os.path.join(HERE, "golden", "lomb_scargle_multi_golden.npz"))
CASES = ("n52", "n216", "n789", "fast216")
NTERMS = (2, 3, 5)
U = 2.0 ** -53


def case(name):
    return tuple(SRC["%s/%s" % (name, k)] for k in ("t", "y", "dy", "freqs"))


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def test_accuracy_against_the_50_digit_truth(eng):
    worst = {}
    for name in CASES:
        t, y, dy, f = case(name)
        eng.set_lightcurves(t, y, dy)
        for tag, weighted in (("w", True), ("u", False)):
            slope = float(FIX["%s/%s_psd_factor" % (name, tag)]) * float(FIX["%s/%s_YY" % (name, tag)])
            for K in NTERMS:
                key = "%s/%s_k%d_" % (name, tag, K)
                b = np.maximum(10.0 * float(FIX[key + "rho"]), 64.0 * np.sqrt(len(t)) * U * FIX[key + "kappa"])
                std = FIX[key + "standard"]
                scale = {"standard": 1.0, "model": 1.0 / (1.0 - std) ** 2, "log": 1.0 / (1.0 - std), "psd": slope}
                for norm in ("standard", "model", "log", "psd"):
                    got = eng.lomb_scargle(f, normalization=norm, weighted=weighted, nterms=K)[0]
                    ratio = float(np.max(np.abs(got - FIX[key + norm]) / (b * scale[norm])))
                    worst[(name, tag, K, norm)] = ratio
                    print("%-8s %s K %d %-8s max |p - truth| / bound = %.3f" % (name, tag, K, norm, ratio))
                assert "mtg_lomb_scargle_multi_kernel<%d,1>" % K == eng.last_solver and eng.last_kernel_ms > 0
    print("largest ratio to the bound: %.3f at %s" % (max(worst.values()), max(worst, key=worst.get)))
    assert max(worst.values()) <= 1.0, {k: v for k, v in worst.items() if not v <= 1.0}


def test_one_term_through_the_new_entries_is_the_one_term_entry(eng):
    t, y, dy, f = case("n216")
    rng = np.random.default_rng(11)
    Y = y[None, :] + 0.3 * rng.standard_normal((9, len(t)))
    eng.set_lightcurves(t, Y, np.tile(dy, (9, 1)))
    L, F = 9, len(f)
    ip = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    ranks = np.array([0, 4, 8], dtype=np.int64)
    for weighted in (True, False):
        want, wpeak, wat = eng.lomb_scargle(f, normalization="psd", weighted=weighted, peak=True)
        got, peak, at = np.full((L, F), np.nan), np.full(L, np.nan), np.full(L, -1, dtype=np.int64)
        rc = eng._lib.mtg_lomb_scargle_multi(eng._ctx, F, dp(f), 1, engine.LS_PSD, int(weighted), dp(got), dp(peak), ip(at))
        assert rc == 0 and "mtg_lomb_scargle_kernel<" in eng.last_solver
        assert np.array_equal(got, want) and np.array_equal(peak, wpeak) and np.array_equal(at, wat)
        env = eng.lomb_scargle_envelope(f, ranks=ranks, reference=want[3], scale=np.full(F, 2.0), normalization="psd", weighted=weighted)
        os_, valid, exceed = np.full((3, F), np.nan), np.zeros(F, dtype=np.int64), np.zeros(F, dtype=np.int64)
        ratio, rat = np.full(L, np.nan), np.full(L, -1, dtype=np.int64)
        scale = np.full(F, 2.0)
        rc = eng._lib.mtg_lomb_scargle_envelope_multi(eng._ctx, F, dp(f), 1, engine.LS_PSD, int(weighted), 3, ip(ranks), dp(os_),
                                                      ip(valid), dp(np.ascontiguousarray(want[3])), ip(exceed), dp(scale), dp(ratio), ip(rat))
        assert rc == 0
        assert np.array_equal(os_, env.order_stat) and np.array_equal(valid, env.valid) and np.array_equal(exceed, env.exceed)
        assert np.array_equal(ratio, env.peak_ratio) and np.array_equal(rat, env.peak_ratio_index)


def test_noise_free_harmonic_signal_has_power_one_from_three_terms_on(eng):
    t, dy = SRC["n216/t"], SRC["n216/dy"]
    T = t[-1] - t[0]
    f = np.linspace(1.0 / T, 216 / T, 300)
    f0 = f[97]
    y = 2.5 + sum(a * np.sin(2.0 * np.pi * k * f0 * t + th) for k, a, th in ((1, 0.7, 0.4), (2, 0.5, 1.3), (3, 0.3, 2.9)))
    eng.set_lightcurves(t, y, dy)
    for weighted in (True, False):
        for K in (3, 5):
            _, kappa = lomb_scargle_multi_numpy.power(t, y, dy if weighted else None, f[97:98], K, return_kappa=True)
            p, peak, at = eng.lomb_scargle(f, weighted=weighted, peak=True, nterms=K)
            print("K %d weighted %d: 1 - p = %.3g, kappa %.3g" % (K, weighted, 1.0 - p[0, 97], kappa[0]))
            assert abs(p[0, 97] - 1.0) <= 64.0 * np.sqrt(216) * U * kappa[0]
            assert at[0] == 97 and peak[0] == p[0, 97]
        for K in (1, 2):
            p, peak, at = eng.lomb_scargle(f, weighted=weighted, peak=True, nterms=K)
            assert p[0, 97] < 1.0 and np.all(p[0] < 1.0) and at[0] == 97


def test_power_depends_on_its_own_light_curve_and_frequency_alone(eng):
    t, y, dy, f = case("n789")
    rng = np.random.default_rng(3)
    Y = y[None, :] + 0.3 * rng.standard_normal((11, len(t)))
    DY = np.tile(dy, (11, 1)) * rng.uniform(0.5, 2.0, size=(11, 1))
    for m in (0, 5, 10):
        Y[m], DY[m] = y, dy
    perm = rng.permutation(300)
    f300 = f[:300]
    for weighted in (True, False):
        eng.set_lightcurves(t, y, dy)
        alone = eng.lomb_scargle(f300, weighted=weighted, nterms=3)[0]
        assert eng.last_solver == "mtg_lomb_scargle_multi_kernel<3,1>"
        # L = 1 against members 0, 5 and 10 of L = 11: full tiles and a partly filled last one (R = 2 weighted, 6 unweighted)
        eng.set_lightcurves(t, Y, DY)
        among = eng.lomb_scargle(f300, weighted=weighted, nterms=3)
        assert eng.last_solver == "mtg_lomb_scargle_multi_kernel<3,%d>" % (2 if weighted else 6)
        for m in (0, 5, 10):
            assert np.array_equal(among[m], alone), (weighted, m)
        # the same times stored per light curve
        eng.set_lightcurves(np.tile(t, (11, 1)), Y, DY)
        per_lc = eng.lomb_scargle(f300, weighted=weighted, nterms=3)
        assert eng.last_solver == "mtg_lomb_scargle_multi_kernel<3,1>"
        assert np.array_equal(per_lc, among), weighted
        # F = 1 against F = 300 permuted
        shuffled = eng.lomb_scargle(f300[perm], weighted=weighted, nterms=3)
        assert np.array_equal(shuffled, among[:, perm]), weighted
        for k in (0, 63, 64, 255, 256, 299):
            one = eng.lomb_scargle(f300[k:k + 1], weighted=weighted, nterms=3)
            assert np.array_equal(one[:, 0], among[:, k]), (weighted, k)


def chunk_edge_case(n):
    """three light curves of n irregular samples, and five frequencies between one and (n - 1) / 4 cycles per span.  Six
    samples carry five parameters: there the sampling is a jittered grid and the frequencies lie around one cycle per six
    samples, where the columns of the design matrix are nearly orthogonal (kappa <= 36 in numpy; random times give 8e6)."""
    rng = np.random.default_rng(100 + n)
    if n == 6:
        t = 58000.0 + 10.0 * np.arange(n) + rng.uniform(-1.0, 1.0, size=n)
        f = np.linspace(0.9, 1.1, 5) / 60.0
    else:
        t = 58000.0 + np.sort(rng.uniform(0.0, 100.0, size=n))
        f = np.linspace(1.0, (n - 1) / 4.0, 5) / (t[-1] - t[0])
    dy = rng.uniform(0.05, 0.3, size=(3, n))
    y = 3.0 + 0.8 * np.sin(2.0 * np.pi * f[2] * t + 0.7)[None, :] + 0.3 * np.sin(4.0 * np.pi * f[2] * t)[None, :] + dy * rng.standard_normal((3, n))
    return t, y, dy, f


@pytest.mark.parametrize("n", [6, 256, 257, 513])
def test_chunk_edges_with_two_terms(eng, n):
    t, y, dy, f = chunk_edge_case(n)
    eng.set_lightcurves(t, y, dy)
    for weighted in (True, False):
        got = eng.lomb_scargle(f, weighted=weighted, nterms=2)
        for l in range(3):
            ref, kappa = lomb_scargle_multi_numpy.power(t, y[l], dy[l] if weighted else None, f, 2, return_kappa=True)
            assert kappa.max() <= 1e6
            ratio = np.abs(got[l] - ref) / (64.0 * np.sqrt(n) * U * kappa)
            print("N %d weighted %d l %d: largest ratio %.3f, kappa up to %.3g" % (n, weighted, l, ratio.max(), kappa.max()))
            assert np.all(ratio <= 1.0)


def test_peaks_are_max_and_first_argmax(eng):
    t, y, dy, f = case("n52")
    rng = np.random.default_rng(5)
    Y = y[None, :] + 0.5 * rng.standard_normal((7, len(t)))
    eng.set_lightcurves(t, Y, np.tile(dy, (7, 1)))
    top = int(np.argmax(eng.lomb_scargle(f, nterms=2)[0]))
    # light curve 0's best frequency twice more, behind and before: the first of the ties is reported
    ff = np.concatenate([f[:10], [f[top]], f[10:], [f[top]]])
    for norm, K in (("standard", 2), ("psd", 5)):
        p, peak, at = eng.lomb_scargle(ff, normalization=norm, peak=True, nterms=K)
        assert np.array_equal(peak, p.max(axis=1)) and np.array_equal(at, p.argmax(axis=1))
        assert p[0, 10] == p[0, -1]
        peak2, at2 = eng.lomb_scargle(ff, normalization=norm, power=False, peak=True, nterms=K)
        assert np.array_equal(peak2, peak) and np.array_equal(at2, at)
    p, peak, at = eng.lomb_scargle(ff, peak=True, nterms=2)
    assert at[0] == (10 if top >= 10 else top)


def test_envelope_is_numpys_sort_and_counts_of_the_same_powers(eng):
    t, y, dy, f = case("n216")
    rng = np.random.default_rng(37)
    L = 37
    Y = y[None, :] + 0.4 * rng.standard_normal((L, len(t)))
    DY = np.tile(dy, (L, 1)) * rng.uniform(0.5, 2.0, size=(L, 1))
    eng.set_lightcurves(t, Y, DY)
    ranks = np.array([0, 18, 35, 36, 18], dtype=np.int64)
    for weighted in (True, False):
        power = eng.lomb_scargle(f, weighted=weighted, nterms=3)
        reference = power[7]
        env = eng.lomb_scargle_envelope(f, ranks=ranks, reference=reference, scale=np.median(power, axis=0), weighted=weighted, nterms=3)
        assert np.array_equal(env.order_stat, np.sort(power, axis=0)[ranks])
        assert np.array_equal(env.valid, np.sum(~np.isnan(power), axis=0))
        assert np.array_equal(env.exceed, np.sum(power >= reference[None, :], axis=0)) and env.exceed.min() >= 1
        ratio = power / np.median(power, axis=0)[None, :]
        assert np.array_equal(env.peak_ratio, ratio.max(axis=1)) and np.array_equal(env.peak_ratio_index, ratio.argmax(axis=1))
        # and not the one-term periodogram's
        assert not np.array_equal(env.order_stat, np.sort(eng.lomb_scargle(f, weighted=weighted), axis=0)[ranks])


def test_errors_and_the_context_afterwards(eng):
    t, y, dy, f = case("n52")
    eng.set_lightcurves(t, y, dy)
    want = eng.lomb_scargle(f, nterms=2)
    fresh = Engine(0)
    try:
        for call in (fresh.lomb_scargle, lambda *a, **k: fresh.lomb_scargle_envelope(*a, ranks=[0], **k)):
            with pytest.raises(EngineError) as exc:
                call(f, nterms=2)                                     # no light curves
            assert exc.value.code == engine.E_STATE and "mtg_set_lightcurves" in str(exc.value)
            fresh.set_lightcurves(t, y, dy)
            for bad in (0, 6):
                with pytest.raises(EngineError) as exc:
                    call(f, nterms=bad)
                assert exc.value.code == engine.E_ARG and "nterms = %d" % bad in str(exc.value)
                assert np.array_equal(fresh.lomb_scargle(f, nterms=2), want)
            t5 = np.array([0.0, 1.0, 2.5, 3.1, 4.7])
            fresh.set_lightcurves(t5, np.array([1.0, 2.0, 0.5, 1.5, 0.7]), np.ones(5))
            with pytest.raises(EngineError) as exc:
                call([0.1], nterms=2)
            assert exc.value.code == engine.E_ARG and "N = 5 < 6" in str(exc.value)
            assert np.all(np.isfinite(fresh.lomb_scargle([0.1, 0.17])))   # one term fits five samples
            fresh.set_lightcurves(t, y, dy)
            assert np.array_equal(fresh.lomb_scargle(f, nterms=2), want)
            fresh.close()
            fresh = Engine(0)
    finally:
        fresh.close()


def test_python_front_end_passes_nterms_on(eng):
    from mind_the_gaps_amd.periodogram import LombScargle
    t, y, dy, f = case("n52")
    eng.set_lightcurves(t, y, dy)
    for K in (3, 5):
        want = eng.lomb_scargle(f, normalization="log", nterms=K)[0]
        assert np.array_equal(LombScargle(t, y, dy, nterms=K, normalization="log").power(f), want)
    unweighted = LombScargle(t, np.stack([y, y + 1.0]), nterms=4).power(f[:9])
    eng.set_lightcurves(t, np.stack([y, y + 1.0]), np.ones((2, len(t))))
    assert np.array_equal(unweighted, eng.lomb_scargle(f[:9], weighted=False, nterms=4))


@pytest.mark.parametrize("K", [4, 5])
def test_full_and_partly_filled_tiles_at_four_and_five_terms(eng, K):
    """L = 1 (the R = 1 kernel the accuracy test holds to the truth at K = 5) against members of L = 11 on shared
    sampling, bit for bit: tiles of 2 (weighted) and 4 / 2 (unweighted) light curves, the last one partly filled."""
    t, y, dy, f = case("n216")
    rng = np.random.default_rng(40 + K)
    Y = y[None, :] + 0.3 * rng.standard_normal((11, len(t)))
    DY = np.tile(dy, (11, 1)) * rng.uniform(0.5, 2.0, size=(11, 1))
    for m in (0, 5, 10):
        Y[m], DY[m] = y, dy
    full = {(4, True): 2, (4, False): 4, (5, True): 1, (5, False): 2}
    for weighted in (True, False):
        eng.set_lightcurves(t, y, dy)
        alone = eng.lomb_scargle(f, weighted=weighted, nterms=K)[0]
        assert eng.last_solver == "mtg_lomb_scargle_multi_kernel<%d,1>" % K
        eng.set_lightcurves(t, Y, DY)
        among = eng.lomb_scargle(f, weighted=weighted, nterms=K)
        assert eng.last_solver == "mtg_lomb_scargle_multi_kernel<%d,%d>" % (K, full[K, weighted])
        for m in (0, 5, 10):
            assert np.array_equal(among[m], alone), (weighted, m)
        # every other member against numpy, within the chunk-edge test's bound
        for m in (1, 10):
            ref, kappa = lomb_scargle_multi_numpy.power(t, Y[m], DY[m] if weighted else None, f[::15], K, return_kappa=True)
            assert np.all(np.abs(among[m, ::15] - ref) <= np.maximum(10.0 * float(FIX["n216/%s_k5_rho" % ("w" if weighted else "u")]),
                                                                     64.0 * np.sqrt(len(t)) * U * kappa))
