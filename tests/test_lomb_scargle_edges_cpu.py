"""CPU side of tests/test_lomb_scargle_edges_gpu.py: tests/golden/lomb_scargle_edges_golden.npz
(scripts/make_lomb_scargle_edges_golden.py) holds what the GPU test relies on.

* the layout, and the two conditions on every (case, row, weighting): the 50-digit CC SS - CS^2 >= 0.05 and rho <= 1e-9
  -- for n4 alone 0.02, four points fitting three parameters;
* the tau-free formula in numpy float64 (tests/lomb_scargle_numpy.py) reproduces every truth within the stored rho;
* perlc3 tells its rows apart: the power of rows 1 and 2 on row 0's times (the fixture's `*_standard_row0_times`, 50
  digits too) is more than 1000 bounds of the GPU test away from their truth at most frequencies, so a kernel that read
  the wrong row's times cannot pass there.
"""
import os

import numpy as np
import pytest

import lomb_scargle_numpy

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = np.load(os.path.join(HERE, "golden", "lomb_scargle_edges_golden.npz"))
CASES = [str(c) for c in FIX["cases"]]
U = 2.0 ** -53
# name -> (L, N, F)
SHAPES = {"edge255": (1, 255, 16), "edge256": (1, 256, 16), "edge257": (1, 257, 16), "edge512": (1, 512, 16),
          "edge513": (1, 513, 16), "n4": (1, 4, 4), "perlc3": (3, 61, 40), "tile4": (4, 257, 24)}


def rows(name):
    """-> [(m, t, y, dy)] with m None for a case of one light curve"""
    t, y, dy = (FIX["%s/%s" % (name, k)] for k in ("t", "y", "dy"))
    if y.ndim == 1:
        return [(None, t, y, dy)]
    return [(m, t[m] if t.ndim == 2 else t, y[m], dy[m]) for m in range(len(y))]


def stored(name, key, m):
    v = FIX["%s/%s" % (name, key)]
    return v if m is None else v[m]


def test_fixture_layout_and_conditions():
    assert CASES == list(SHAPES)
    for name, (L, N, F) in SHAPES.items():
        t, y, dy, f = (FIX["%s/%s" % (name, k)] for k in ("t", "y", "dy", "freqs"))
        lead = () if L == 1 else (L,)
        assert y.shape == dy.shape == lead + (N,) and f.shape == (F,) and np.all(f > 0) and np.all(dy > 0)
        assert t.shape == ((L, N) if name == "perlc3" else (N,))
        assert np.all(np.diff(t, axis=-1) > 0) and np.all((57000 < t) & (t < 59500))
        det_floor = 0.02 if name == "n4" else 0.05
        for tag in "wu":
            for key in ("rho", "det_min", "psd_factor"):
                assert FIX["%s/%s_%s" % (name, tag, key)].shape == lead
            assert np.all(FIX["%s/%s_det_min" % (name, tag)] >= det_floor), (name, tag)
            assert np.all(FIX["%s/%s_rho" % (name, tag)] <= 1e-9), (name, tag)
            std = FIX["%s/%s_standard" % (name, tag)]
            assert std.shape == lead + (F,) and np.all((std > 0) & (std < 1))
            factor = FIX["%s/%s_psd_factor" % (name, tag)][..., None]
            # the four normalisations are one truth
            assert np.allclose(FIX["%s/%s_model" % (name, tag)], std / (1 - std), rtol=1e-13)
            assert np.allclose(FIX["%s/%s_log" % (name, tag)], -np.log1p(-std), rtol=1e-13)
            assert np.allclose(FIX["%s/%s_psd" % (name, tag)], std * factor, rtol=1e-13)
    # the grids the issue names
    for name in CASES[:5]:
        t, N = FIX[name + "/t"], SHAPES[name][1]
        T = t[-1] - t[0]
        assert np.array_equal(FIX[name + "/freqs"], np.linspace(1.0 / T, N / T, 16))
    t = FIX["n4/t"]
    assert np.array_equal(FIX["n4/freqs"], np.array([0.4, 0.7, 1.0, 1.3]) / (t[-1] - t[0]))
    t = FIX["perlc3/t"]
    Tmin = np.min(t[:, -1] - t[:, 0])
    assert np.array_equal(FIX["perlc3/freqs"], np.linspace(1.0 / Tmin, 61 / Tmin, 40))
    # times and first epoch differ per row
    assert len({float(v) for v in t[:, 0]}) == 3 and not np.any(t[0] == t[1]) and not np.any(t[0] == t[2])
    # tile4: the error bars of a row are row 0's times a factor in [0.5, 2]; the noise is the row's own
    DY, Y = FIX["tile4/dy"], FIX["tile4/y"]
    factors = DY[:, 0] / DY[0, 0]
    assert np.allclose(DY, factors[:, None] * DY[0], rtol=1e-15) and factors.min() == 0.5 and factors.max() == 2.0
    assert len(set(factors)) == 4 and all(not np.any(Y[a] == Y[b]) for a in range(4) for b in range(a))
    assert os.path.getsize(os.path.join(HERE, "golden", "lomb_scargle_edges_golden.npz")) < 200 * 1024


@pytest.mark.parametrize("name", list(SHAPES))
def test_numpy_tau_free_formula_within_rho(name):
    f = FIX[name + "/freqs"]
    for m, t, y, dy in rows(name):
        for tag, err in (("w", dy), ("u", None)):
            got = lomb_scargle_numpy.power(t, y, err, f)
            rho = float(stored(name, tag + "_rho", m))
            e = float(np.max(np.abs(got - stored(name, tag + "_standard", m))))
            print("\nnumpy %s %s %s: max error %.3g, stored rho %.3g" % (name, m, tag, e, rho))
            assert e <= rho
            for norm in ("model", "log", "psd"):
                ref = stored(name, "%s_%s" % (tag, norm), m)
                assert np.allclose(lomb_scargle_numpy.power(t, y, err, f, norm), ref, rtol=0, atol=1e-8 * np.max(np.abs(ref)))


def test_slab17_row_16_holds_the_n4_conditions_and_numpy_is_within_rho():
    t, f4, F, index = FIX["n4/t"], FIX["n4/freqs"], int(FIX["slab17/F"]), FIX["slab17/index"]
    Y, DY = FIX["slab17/y"], FIX["slab17/dy"]
    assert F == 1 << 21 and Y.shape == DY.shape == (17, 4) and np.all(DY > 0)
    assert index.shape == (64,) and index[0] == 0 and index[-1] == F - 1 and np.all(np.diff(index) > 0)
    f = np.linspace(f4[0], f4[-1], F)[index]
    for tag, err in (("w", DY[16]), ("u", None)):
        rho = float(FIX["slab17/%s_rho" % tag])
        assert FIX["slab17/%s_det_min" % tag] >= 0.02 and rho <= 1e-9
        assert np.max(np.abs(lomb_scargle_numpy.power(t, Y[16], err, f) - FIX["slab17/%s_standard" % tag])) <= rho


def test_perlc3_tells_the_rows_sampling_apart():
    f, t0 = FIX["perlc3/freqs"], FIX["perlc3/t"][0]
    for tag in "wu":
        truth, wrong = FIX["perlc3/%s_standard" % tag], FIX["perlc3/%s_standard_row0_times" % tag]
        assert wrong.shape == truth.shape == (3, 40)
        # row 0 on its own times is its truth; and the stored second truth is what numpy gives on row 0's times
        assert np.array_equal(wrong[0], truth[0])
        for m in (1, 2):
            err = FIX["perlc3/dy"][m] if tag == "w" else None
            assert np.max(np.abs(lomb_scargle_numpy.power(t0, FIX["perlc3/y"][m], err, f) - wrong[m])) <= 1e-9
            bound = max(10.0 * float(FIX["perlc3/%s_rho" % tag][m]), 64.0 * np.sqrt(61) * U)
            far = np.abs(wrong[m] - truth[m]) > 1000.0 * bound
            print("\nperlc3 %s row %d: %d of 40 frequencies further than 1000 bounds (%.3g); median distance %.3g"
                  % (tag, m, far.sum(), 1000.0 * bound, np.median(np.abs(wrong[m] - truth[m]))))
            assert far.sum() > 20
