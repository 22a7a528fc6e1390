"""The host replay of the simulator's draws and spectra (simulator_replay.py) is the specification the device is held to
(test_simulator_replay_gpu.py), so it is checked first, without a GPU: its Poisson counts follow the exact Poisson law in
both regimes and at the switch, its loop caps and NaN branch do what the kernel's do, its normals, E13 draws and spectra
agree with their mpmath twins -- the worst errors seen are the figures R_draw and R_psd the device tolerances are set
against, printed here -- and it meets no close decision on the Poisson inputs of the GPU test."""
import mpmath
import numpy as np
import pytest
from scipy import stats

import simulator_replay as sr

SEED = 0x5EED0123456789


def _chi_square(counts, lam):
    """chi-square of the sample against the exact pmf over bins of consecutive integers with expected count >= 20
    (the tails folded into the outermost bins) -> (statistic, degrees of freedom, p)"""
    total = counts.size
    lo = int(max(stats.poisson.ppf(1e-13, lam) - 1, 0))
    hi = int(stats.poisson.ppf(1.0 - 1e-13, lam) + 1)
    k = np.arange(lo, hi + 1)
    expect = total * stats.poisson.pmf(k, lam)
    expect[0] = total * stats.poisson.cdf(lo, lam)
    expect[-1] = total * stats.poisson.sf(hi - 1, lam)
    edges, acc = [lo], 0.0            # bin j holds edges[j] <= k < edges[j + 1]
    for kk, e in zip(k, expect):
        acc += e
        if acc >= 20.0:
            edges.append(kk + 1)
            acc = 0.0
    if acc > 0.0:                     # a remainder below 20 joins the last bin
        edges[-1] = hi + 1
    edges = np.array(edges)
    edges[0], edges[-1] = -1, np.iinfo(np.int64).max
    which = np.searchsorted(edges, counts.ravel().astype(np.int64), side="right") - 1
    seen = np.bincount(which, minlength=len(edges) - 1).astype(np.float64)
    cdf = np.concatenate([[0.0], stats.poisson.cdf(edges[1:-1] - 1, lam), [1.0]])
    want = total * np.diff(cdf)
    assert np.all(want >= 19.0) and len(want) >= 2
    stat = float(np.sum((seen - want) ** 2 / want))
    return stat, len(want) - 1, float(stats.chi2.sf(stat, len(want) - 1))


@pytest.mark.parametrize("lam", [0, 0.5, 3, 9.999, 10, 10.001, 30, 1e3, 1e6])
def test_poisson_counts_follow_the_poisson_law(lam):
    """2 10^5 draws per mean, on both sides of the switch at 10 and far into PTRS: p > 1e-4 with the seed fixed, and no
    draw near either loop cap."""
    d = sr.poisson_detail(np.full((400, 500), float(lam)), np.arange(500)[None, :], np.arange(400)[:, None], SEED)
    counts = d["counts"]
    assert not d["capped"].any() and np.all(counts == np.floor(counts)) and np.all(counts >= 0)
    print("lam = %g: most trips %d (caps %d / %d)" % (lam, d["trips"].max(), sr.KNUTH_TRIPS, sr.PTRS_TRIPS))
    assert d["trips"].max() < (sr.KNUTH_TRIPS if lam < 10 else sr.PTRS_TRIPS)
    if lam == 0:
        assert np.all(counts == 0)
        return
    stat, dof, p = _chi_square(counts, float(lam))
    print("lam = %g: chi2 = %.1f over %d degrees of freedom, p = %.3g" % (lam, stat, dof, p))
    assert p > 1e-4


def test_poisson_edges_nan_caps_and_fall_back(monkeypatch):
    """a negative or NaN mean gives NaN and touches no other element; with uniforms that never let a loop end the Knuth
    branch stops at 2 x 63 counts and PTRS falls back to floor(lam + 0.5), as the kernel's loops do"""
    lam = np.array([3.0, -1e-300, np.nan, 12.0, -5.0, 0.0])
    counts, margin = sr.poisson(lam, np.arange(6), 9, SEED)
    alone = [sr.poisson(lam[i], i, 9, SEED)[0] for i in (0, 3, 5)]
    assert np.array_equal(np.isnan(counts), [False, True, True, False, True, False])
    assert [counts[0], counts[3], counts[5]] == [float(a) for a in alone] and counts[5] == 0.0
    assert np.all(margin[[1, 2, 4]] == 1.0)
    # the counters: another epoch, series or seed is another draw
    base = sr.poisson(np.full(200, 7.0), np.arange(200), 3, SEED)[0]
    assert not np.array_equal(base, sr.poisson(np.full(200, 7.0), np.arange(200), 4, SEED)[0])
    assert not np.array_equal(base, sr.poisson(np.full(200, 7.0), np.arange(200) + 1, 3, SEED)[0])
    assert not np.array_equal(base, sr.poisson(np.full(200, 7.0), np.arange(200), 3, SEED + 1)[0])
    monkeypatch.setattr(sr, "block", lambda c0, purpose, series, c3, seed: (np.full(np.shape(c0), 0.999), np.full(np.shape(c0), 0.5)))
    d = sr.poisson_detail(np.array([9.5, 40.2, 40.7]), np.arange(3), 0, SEED)
    # Knuth: the product halves with every block and passes exp(-9.5) after 14 of them
    assert d["counts"][0] == 27.0 and not d["capped"][0]
    # PTRS: us = 0.001 < 0.013 and V = 0.5 > us on every trip
    assert d["capped"][1] and d["capped"][2] and d["counts"][1] == 40.0 and d["counts"][2] == 41.0 and np.all(d["trips"][1:] == sr.PTRS_TRIPS)
    monkeypatch.setattr(sr, "block", lambda c0, purpose, series, c3, seed: (np.full(np.shape(c0), 0.9999), np.full(np.shape(c0), 0.9999)))
    d = sr.poisson_detail(np.array([9.5]), 0, 0, SEED)
    assert d["capped"][0] and d["counts"][0] == 2.0 * sr.KNUTH_TRIPS and d["trips"][0] == sr.KNUTH_TRIPS


def test_margin_sees_a_close_decision():
    """a mean within an ulp of the switch, and a product landing on the limit, are undecided; ordinary draws are not"""
    assert sr.poisson(np.nextafter(10.0, 0.0), 0, 0, SEED)[1] <= sr.DECIDED
    ua, _ = sr.block(5, sr.NOISE, 2, 1, SEED)
    lam = -np.log(float(ua))                       # exp(-lam) = the first uniform, to an ulp
    assert sr.poisson(lam, 5, 2, SEED)[1] <= sr.DECIDED
    _, margin = sr.poisson(np.full((40, 120), 25.0), np.arange(120)[None, :], np.arange(40)[:, None], SEED)
    assert np.all(margin > sr.DECIDED)


def test_normals_and_e13_draws_against_mpmath():
    """R_draw: the replay's float64 draws against their twins at 40 digits, in units of 2^-52 relative.  The normals and
    the uniform kind stay within R_NORMAL and R_UNIFORM; the lognormal's error grows with the exponent |s_ln z| it
    takes exp of: within R_draw(x) = R_DRAW[0] + R_DRAW[1] x over std / mean in [0.2, 1], the range the GPU test works in."""
    ua, ub = sr.block(np.arange(4000), sr.NOISE, 5, 0, SEED)
    g1, g2 = sr.normal2((ua, ub))
    twins = [sr.normal2_mp(a, b) for a, b in zip(ua, ub)]
    worst_n = max(sr.rel_ulps(g1, [t[0] for t in twins]).max(), sr.rel_ulps(g2, [t[1] for t in twins]).max())
    print("R_draw, normal2: %.2f ulp" % worst_n)
    assert worst_n <= sr.R_NORMAL
    # exact at the quadrant points, where a cosine of a rounded 2 pi u would not be
    s, c = sr.sincospi(np.array([0.0, 0.5, 1.0, 1.5]))
    assert np.array_equal(s, [0.0, 1.0, 0.0, -1.0]) and np.array_equal(c, [1.0, 0.0, -1.0, 0.0])
    rng = np.random.default_rng(3)
    worst_a, worst_b, worst_u = 0.0, 0.0, 0.0
    for i, ratio in enumerate(np.concatenate([[0.2, 1.0], rng.uniform(0.2, 1.0, 30)])):
        mean = 25.0
        for kind in (1, 2):
            m = mean if kind == 1 else 100.0                 # (the uniform kind's cases keep mean - sqrt(3) std away from 0)
            std = float(ratio) * (mean if kind == 1 else 25.0)
            x, e = sr.e13_draws(kind, m, std, 301, 11 + i, SEED, with_exponent=True)
            assert x.shape == (301,)                         # the odd tail: 151 blocks, the last one's second element dropped
            u = sr.rel_ulps(x, sr.e13_draws_mp(kind, m, std, 301, 11 + i, SEED))
            if kind == 2:
                worst_u = max(worst_u, u.max())
                continue
            worst_a = max(worst_a, u[e < 0.02].max() if np.any(e < 0.02) else 0.0)
            worst_b = max(worst_b, np.max((u - sr.R_DRAW[0]) / e))
            assert np.all(u <= sr.r_draw(e)), (ratio, u.max())
    print("R_draw, lognormal: %.2f ulp at |s_ln z| < 0.02, slope (err - %.1f) / |s_ln z| at most %.2f; uniform: %.2f ulp"
          % (worst_a, sr.R_DRAW[0], worst_b, worst_u))
    assert worst_u <= sr.R_UNIFORM
    # two series and an even length in one call are the single calls
    both = sr.e13_draws(1, 25.0, np.array([7.0, 9.0]), 64, np.array([3, 4]), SEED)
    assert np.array_equal(both[1], sr.e13_draws(1, 25.0, 9.0, 64, 4, SEED)) and both.shape == (2, 64)
    assert np.array_equal(sr.e13_draws(1, 25.0, 9.0, 63, 4, SEED), both[1][:63])


def test_spectrum_against_mpmath():
    """R_psd: mtg_psd restated in float64 against the model's spectrum at 40 digits, over the rows and lines of the GPU
    test; per model the worst relative error in units of 2^-52 (rows near Q = 1 / 2 cancel: 1 +- 1 / f with f -> 0)."""
    k = np.arange(1, sr.PSD_NFFT // 2 + 1)
    w = sr.grid_omega(k, sr.PSD_NFFT, sr.PSD_DT)
    for name, (kinds, rows) in sr.PSD_MODELS.items():
        assert rows.shape == (6, sum(sr.NPARAMS[kd] for kd in kinds))
        per_row = [sr.rel_ulps(sr.psd_f64(kinds, row, w), sr.psd(kinds, row, w)).max() for row in rows]
        print("R_psd, %s: %.3g ulp (rows: %s)" % (name, max(per_row), " ".join("%.3g" % v for v in per_row)))
        assert max(per_row) == sr.r_psd(name) and np.all(np.array([float(v) for row in rows for v in sr.psd(kinds, row, w)]) > 0)
        if sr.K_SHO in kinds:
            sig = [sr.signature(kinds, row) for row in rows]
            lnq = rows[:, sum(sr.NPARAMS[kd] for kd in kinds[:kinds.index(sr.K_SHO)]) + 1]
            near = np.abs(lnq - np.log(0.5)) < 1e-3
            assert set(sig) == {0, 1} and np.any(near & (np.array(sig) == 1)) and np.any(near & (np.array(sig) == 0))
    # the coefficients are the terms': closed forms of the DRW and of the SHO on either side of Q = 1 / 2
    with mpmath.workdps(sr.DIGITS):
        for row in sr.PSD_MODELS["sho"][1]:
            S0, Q, w0 = [mpmath.exp(mpmath.mpf(float(v))) for v in row]
            for wi, got in zip(w, sr.psd([sr.K_SHO], row, w)):
                ww = mpmath.mpf(float(wi))
                want = mpmath.sqrt(2 / mpmath.pi) * S0 * w0 ** 4 / ((ww ** 2 - w0 ** 2) ** 2 + w0 ** 2 * ww ** 2 / Q ** 2)
                assert abs(got - want) <= mpmath.mpf(10) ** -30 * want
        for row in sr.PSD_MODELS["drw"][1]:
            a, c = [mpmath.exp(mpmath.mpf(float(v))) for v in row]
            for wi, got in zip(w, sr.psd([sr.K_DRW], row, w)):
                want = mpmath.sqrt(2 / mpmath.pi) * a * c / (c ** 2 + mpmath.mpf(float(wi)) ** 2)
                assert abs(got - want) <= mpmath.mpf(10) ** -35 * want
        # a jitter term has no spectrum; a sum is the sum
        kinds, rows = sr.PSD_MODELS["drw+sho+jitter"]
        parts = [a + b for a, b in zip(sr.psd([sr.K_DRW], rows[0][:2], w), sr.psd([sr.K_SHO], rows[0][2:5], w))]
        assert all(abs(a - b) <= mpmath.mpf(10) ** -35 * a for a, b in zip(sr.psd(kinds, rows[0], w), parts))


@pytest.mark.parametrize("name", list(sr.POISSON_CASES) + ["kraft"])
def test_no_undecided_epoch_on_the_gpu_tests_inputs(name):
    """The share of undecided epochs on the Poisson inputs of the GPU test, with the clean rates replayed on the host
    (numpy's irfft: the device's to ~1e-12): none, for these seeds -- the GPU test's cap of 1 in 10^4 has room to spare.
    The cases are what they are meant to be: means around 2 with some clean rates below zero, around 25, and 9 to 11
    with epochs on both sides of the switch."""
    sim, thetas, seed = sr.kraft_simulator() if name == "kraft" else sr.poisson_simulator(name)
    clean = sr.clean_on_host(sim, thetas, seed)
    lam = clean * sim._exposures[None, :] + sim._bkg_counts[None, :]
    d = sr.poisson_detail(lam, np.arange(lam.shape[1])[None, :], np.arange(lam.shape[0])[:, None], seed)
    undecided = np.mean(d["margin"] <= sr.DECIDED)
    print("%s: lam %.2f .. %.2f (mean %.2f), %d negative, undecided share %.3g, most trips %d"
          % (name, lam.min(), lam.max(), lam.mean(), np.sum(lam < 0), undecided, d["trips"].max()))
    assert undecided == 0.0 and not d["capped"].any()
    if name == "knuth-2":
        assert 1.5 < lam.mean() < 2.5 and np.sum(lam < 0) >= 5 and lam.max() < 10
    elif name == "ptrs-25":
        assert 24 < lam.mean() < 26 and lam.min() > 10
    elif name == "switch-10":
        assert lam.min() > 7.5 and lam.max() < 12.5 and np.mean(lam < 10) > 0.2 and np.mean(lam >= 10) > 0.2
    else:
        assert lam.min() > 0 and 12 < lam.mean() < 22        # totals scatter to both sides of the 15 counts of the Kraft table
