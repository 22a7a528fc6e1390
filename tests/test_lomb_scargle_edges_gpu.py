"""mtg_lomb_scargle on the GPU at the shapes where its launcher takes another path (include/mtg.h,
csrc/mtg_lomb_scargle.hip): chunk edges of the 256-sample staging, the smallest N, sampling of its own per light curve,
the R = 4 tile, every fill of the R = 8 / R = 16 tiles, the 64 / 128 / 256-thread launches, slabs of light curves with
a start row above 0 (shared and per-light-curve sampling), and the NaN contract of the entry.

Accuracy is held against the 50-digit truth of tests/golden/lomb_scargle_edges_golden.npz
(scripts/make_lomb_scargle_edges_golden.py; tests/test_lomb_scargle_edges_cpu.py holds the fixture to its conditions)
with the bound of tests/test_lomb_scargle_gpu.py: standard power within max(10 rho, 64 sqrt(N) u), u = 2^-53, rho the
error of plain numpy float64 on the same light curve; the other normalisations within that bound times |dP/dp| at the
truth.  Everything else is bit for bit against the same light curve bound alone (L = 1), which this file and
tests/test_lomb_scargle_gpu.py pin to the truth.

Measured on an MI355X, worst |p - truth| / bound over both weightings and the four normalisations (every test prints
its own):
    chunk edges   edge255 9.4e-4, edge256 1.3e-3, edge257 5.9e-4, edge512 3.4e-4, edge513 3.6e-4; n4 0.024
    perlc3        7.1e-3 (weighted, row 0); every row bit for bit its L = 1 result
    R = 4         8.1e-4 (L = 2, weighted, row 0); every row bit for bit its L = 1 result
    tile fills    row 0 8.1e-4 at L = 5, 8, 9, 16, 17; every row bit for bit its L = 1 result
    launch widths 5.9e-4 in the call of F = 100; F = 64, 65, 128, 129 bit for bit the columns of F = 300
    slabs         row 16 (second slab) 0.17 of the bound from numpy float64, 0.086 from the truth (weighted; 0.033 /
                  0.016 unweighted); rows 0, 15, 16, their peaks and indices bit for bit their L = 1 results
The bound is dominated by 64 sqrt(N) u throughout (rho <= 4e-15).  The two slab tests take 0.34 s and 0.38 s, the
file 1.4 s.
"""
import os

import numpy as np
import pytest

import lomb_scargle_numpy
from mind_the_gaps_amd.engine import Engine

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = np.load(os.path.join(HERE, "golden", "lomb_scargle_edges_golden.npz"))
U = 2.0 ** -53
NORMS = ("standard", "model", "log", "psd")
WEIGHTINGS = (("w", True), ("u", False))


def bound(n, rho):
    return max(10.0 * float(rho), 64.0 * np.sqrt(n) * U)


def stored(name, key, m=None):
    v = FIX["%s/%s" % (name, key)]
    return v if m is None else v[m]


def worst_ratio(eng, name, tag, weighted, m=None, row=0, freqs=None, pick=slice(None)):
    """the resident set's row `row` against the truth of fixture light curve (name, m) in the four normalisations, as
    test_accuracy_against_the_50_digit_truth forms it; `freqs` / `pick`: the call's list and where the fixture's
    frequencies sit in it.  -> largest |p - truth| / (bound |dP/dp|)"""
    b = bound(FIX[name + "/t"].shape[-1], stored(name, tag + "_rho", m))
    std = stored(name, tag + "_standard", m)
    scale = {"standard": 1.0, "model": 1.0 / (1.0 - std) ** 2, "log": 1.0 / (1.0 - std),
             "psd": float(stored(name, tag + "_psd_factor", m))}
    f = FIX[name + "/freqs"] if freqs is None else freqs
    worst = 0.0
    for norm in NORMS:
        got = eng.lomb_scargle(f, normalization=norm, weighted=weighted)[row][pick]
        worst = max(worst, float(np.max(np.abs(got - stored(name, "%s_%s" % (tag, norm), m)) / (b * scale[norm]))))
    return worst


def all_norms(eng, f, weighted):
    return [eng.lomb_scargle(f, normalization=norm, weighted=weighted) for norm in NORMS]


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


@pytest.mark.parametrize("name", ["edge255", "edge256", "edge257", "edge512", "edge513", "n4"])
def test_chunk_edges_and_the_smallest_n_against_truth(eng, name):
    eng.set_lightcurves(FIX[name + "/t"], FIX[name + "/y"], FIX[name + "/dy"])
    worst = {tag: worst_ratio(eng, name, tag, weighted) for tag, weighted in WEIGHTINGS}
    assert eng.last_solver.endswith("<1>")
    print("\n%-8s worst |p - truth| / bound: weighted %.3g, unweighted %.3g" % (name, worst["w"], worst["u"]))
    assert max(worst.values()) <= 1.0, worst


def test_per_light_curve_sampling_against_truth_and_alone(eng):
    t, y, dy, f = (FIX["perlc3/" + k] for k in ("t", "y", "dy", "freqs"))
    assert t.shape == (3, 61)
    worst, among = {}, {}
    eng.set_lightcurves(t, y, dy)
    for tag, weighted in WEIGHTINGS:
        for m in range(3):
            worst[(tag, m)] = worst_ratio(eng, "perlc3", tag, weighted, m=m, row=m)
        assert eng.last_solver.endswith("<1>")
        among[tag] = all_norms(eng, f, weighted)
    print("\nperlc3 worst |p - truth| / bound %.3g at %s" % (max(worst.values()), max(worst, key=worst.get)))
    assert max(worst.values()) <= 1.0, worst
    for m in range(3):
        eng.set_lightcurves(t[m], y[m], dy[m])
        for tag, weighted in WEIGHTINGS:
            for p, q in zip(among[tag], all_norms(eng, f, weighted)):
                assert np.array_equal(p[m], q[0]), (tag, m)


def test_the_r4_tile_against_truth_and_alone(eng):
    t, Y, DY, f = (FIX["tile4/" + k] for k in ("t", "y", "dy", "freqs"))
    rng = np.random.default_rng(41)
    DYS = rng.uniform(0.05, 0.3, size=Y.shape)     # error bars of its own per light curve: weights that differ in shape
    alone = {}
    for m in range(4):
        for key, err in (("fix", DY), ("own", DYS)):
            eng.set_lightcurves(t, Y[m], err[m])
            for tag, weighted in WEIGHTINGS:
                alone[(key, tag, m)] = all_norms(eng, f, weighted)
    worst = {}
    for L in (2, 3, 4):
        eng.set_lightcurves(t, Y[:L], DY[:L])
        for tag, weighted in WEIGHTINGS:
            for m in range(L):
                worst[(L, tag, m)] = worst_ratio(eng, "tile4", tag, weighted, m=m, row=m)
            assert eng.last_solver.endswith("<4>"), eng.last_solver
            for norm, p in enumerate(all_norms(eng, f, weighted)):
                for m in range(L):
                    assert np.array_equal(p[m], alone[("fix", tag, m)][norm][0]), (L, tag, m, norm)
        eng.set_lightcurves(t, Y[:L], DYS[:L])
        for tag, weighted in WEIGHTINGS:
            for norm, p in enumerate(all_norms(eng, f, weighted)):
                for m in range(L):
                    assert np.array_equal(p[m], alone[("own", tag, m)][norm][0]), (L, tag, m, norm)
    print("\ntile4 worst |p - truth| / bound %.3g at (L, weighting, row) %s" % (max(worst.values()), max(worst, key=worst.get)))
    assert max(worst.values()) <= 1.0, {k: v for k, v in worst.items() if v > 1.0}


def test_every_fill_of_the_wide_tiles_equals_the_light_curve_alone(eng):
    t, f = FIX["tile4/t"], FIX["tile4/freqs"]
    rng = np.random.default_rng(42)
    Y = FIX["tile4/y"][0][None, :] + 0.3 * rng.standard_normal((17, len(t)))
    DY = rng.uniform(0.05, 0.3, size=Y.shape)
    Y[0], DY[0] = FIX["tile4/y"][0], FIX["tile4/dy"][0]          # row 0 is the fixture's: held to the truth below
    alone = {}
    for m in range(17):
        eng.set_lightcurves(t, Y[m], DY[m])
        for tag, weighted in WEIGHTINGS:
            alone[(tag, m)] = [eng.lomb_scargle(f, normalization=norm, weighted=weighted)[0] for norm in ("standard", "psd")]
    worst = 0.0
    # 5: a partly filled first tile with a half-filled pair column; 8 / 16: exactly full; 9 / 17: one light curve beyond
    for L in (5, 8, 9, 16, 17):
        eng.set_lightcurves(t, Y[:L], DY[:L])
        for tag, weighted in WEIGHTINGS:
            for i, norm in enumerate(("standard", "psd")):
                p = eng.lomb_scargle(f, normalization=norm, weighted=weighted)
                assert eng.last_solver.endswith("<8>" if weighted else "<16>"), eng.last_solver
                for m in range(L):
                    assert np.array_equal(p[m], alone[(tag, m)][i]), (L, tag, norm, m)
            worst = max(worst, worst_ratio(eng, "tile4", tag, weighted, m=0, row=0))
    print("\ntile fills: row 0 worst |p - truth| / bound %.3g" % worst)
    assert worst <= 1.0


def test_launch_widths(eng):
    t, y, dy, f16 = (FIX["edge257/" + k] for k in ("t", "y", "dy", "freqs"))
    rng = np.random.default_rng(43)
    f300 = np.sort(rng.uniform(f16[0], f16[-1], size=300))
    # the fixture's frequencies scattered over a list of 100: two waves of a 128-thread workgroup
    at = np.sort(rng.choice(100, size=16, replace=False))
    assert at.max() >= 64
    f100 = f300[:100].copy()
    f100[at] = f16
    eng.set_lightcurves(t, y, dy)
    worst = {}
    for tag, weighted in WEIGHTINGS:
        full = eng.lomb_scargle(f300, weighted=weighted)
        for F in (64, 65, 128, 129):           # 64 | 128 | 128 | 256 threads
            assert np.array_equal(eng.lomb_scargle(f300[:F], weighted=weighted), full[:, :F]), (tag, F)
        worst[tag] = worst_ratio(eng, "edge257", tag, weighted, freqs=f100, pick=at)
    print("\nlaunch widths: F = 100 worst |p - truth| / bound: weighted %.3g, unweighted %.3g" % (worst["w"], worst["u"]))
    assert max(worst.values()) <= 1.0, worst


def test_slabs_with_a_start_row_above_zero_on_shared_sampling(eng):
    # F = 2^21: slabs of 2^25 / F = 16 light curves, so L = 17 is 16 + 1 -- two tiles of 8 and one of 1 weighted, one
    # tile of 16 and one of 1 unweighted
    t, f4, F, index = FIX["n4/t"], FIX["n4/freqs"], int(FIX["slab17/F"]), FIX["slab17/index"]
    Y, DY = FIX["slab17/y"], FIX["slab17/dy"]
    f = np.linspace(f4[0], f4[-1], F)
    for tag, weighted in WEIGHTINGS:
        alone = {}
        for m in (0, 15, 16):
            eng.set_lightcurves(t, Y[m], DY[m])
            alone[m] = eng.lomb_scargle(f, weighted=weighted, peak=True)
        eng.set_lightcurves(t, Y, DY)
        power, peak, at = eng.lomb_scargle(f, weighted=weighted, peak=True)
        assert power.shape == (17, F) and eng.last_solver.endswith("<8>" if weighted else "<16>")
        for m in (0, 15, 16):
            p1, peak1, at1 = alone[m]
            assert np.array_equal(power[m], p1[0], equal_nan=True), (tag, m)
            assert peak[m] == peak1[0] and at[m] == at1[0], (tag, m)
        assert np.all(np.isfinite(power).any(axis=1))
        assert np.array_equal(peak, np.nanmax(power, axis=1)) and np.array_equal(at, np.nanargmax(power, axis=1)), tag
        # row 16, the second slab's, against numpy float64 -- and against its 50-digit truth
        b = bound(4, FIX["slab17/%s_rho" % tag])
        ref = lomb_scargle_numpy.power(t, Y[16], DY[16] if weighted else None, f[index])
        e_numpy = float(np.max(np.abs(power[16, index] - ref))) / b
        e_truth = float(np.max(np.abs(power[16, index] - FIX["slab17/%s_standard" % tag]))) / b
        print("\nslabs %s: row 16 at 64 frequencies, |p - numpy| / bound %.3g, |p - truth| / bound %.3g" % (tag, e_numpy, e_truth))
        assert e_numpy <= 1.0 and e_truth <= 1.0
        del power, alone, p1                    # 285 MB and 3 x 17 MB on the host


def test_slabs_with_a_start_row_above_zero_on_per_light_curve_sampling(eng):
    # F = 2^24: slabs of 2 light curves, so L = 3 is 2 + 1; peaks only -- nothing of size L F comes to the host
    t4, f4 = FIX["n4/t"], FIX["n4/freqs"]
    rng = np.random.default_rng(44)
    T = np.stack([t4, 57000.0 + np.sort(rng.uniform(0.0, 900.0, size=4)), 58500.0 + np.sort(rng.uniform(0.0, 700.0, size=4))])
    Y = 3.0 + 0.5 * rng.standard_normal((3, 4))
    DY = rng.uniform(0.05, 0.3, size=(3, 4))
    f = np.linspace(f4[0], f4[-1], 1 << 24)
    for tag, weighted in WEIGHTINGS:
        eng.set_lightcurves(T, Y, DY)
        peak, at = eng.lomb_scargle(f, weighted=weighted, power=False, peak=True)
        assert eng.last_solver.endswith("<1>") and peak.shape == at.shape == (3,)
        assert np.all(np.isfinite(peak)) and np.all((at >= 0) & (at < len(f)))
        for m in range(3):
            eng.set_lightcurves(T[m], Y[m], DY[m])
            peak1, at1 = eng.lomb_scargle(f, weighted=weighted, power=False, peak=True)
            assert peak[m] == peak1[0] and at[m] == at1[0], (tag, m, peak, at, peak1, at1)
        print("\nper-light-curve slabs %s: peaks %s at %s" % (tag, peak, at))
    # (the rows differ: a peak read from another row's slot would not pass)
    assert len(set(at.tolist())) == 3 or len(set(peak.tolist())) == 3


def test_a_non_positive_determinant_gives_nan_and_the_peak_passes_it_over(eng):
    # t = 0 .. 7, weights 1 / 8 (exact).  f = 0.5: every sine is exactly 0, the cosines +-1, so SS = 0 exactly;
    # f = 1.0: every cosine exactly 1, so CC = 0 and SS = 0 exactly.  CC SS - CS^2 is exactly 0: not positive.
    rng = np.random.default_rng(45)
    y = rng.standard_normal(8)
    eng.set_lightcurves(np.arange(8.0), y, np.ones(8))
    f = np.array([0.3, 0.5, 1.0, 0.2])
    for norm in NORMS:
        p, peak, at = eng.lomb_scargle(f, normalization=norm, weighted=False, peak=True)
        assert np.array_equal(np.isnan(p[0]), [False, True, True, False]) and np.all(np.isfinite(p[0, [0, 3]])), (norm, p)
        assert at[0] in (0, 3) and at[0] == np.nanargmax(p[0]) and peak[0] == p[0, at[0]], (norm, p, peak, at)
        p, peak, at = eng.lomb_scargle(f[1:3], normalization=norm, weighted=False, peak=True)
        assert np.all(np.isnan(p)) and np.isnan(peak[0]) and at[0] == -1, (norm, p, peak, at)
        peak, at = eng.lomb_scargle(f[1:3], normalization=norm, weighted=False, power=False, peak=True)
        assert np.isnan(peak[0]) and at[0] == -1
