"""CPU side of the Lomb-Scargle periodogram (mtg_lomb_scargle; tests/test_lomb_scargle_gpu.py is the GPU side).

* the tau-free formula in numpy float64 (tests/lomb_scargle_numpy.py) reproduces a case of
  tests/golden/lomb_scargle_golden.npz (scripts/make_lomb_scargle_golden.py: 50-digit truth by astropy's form) within the
  rho stored there, and the fixture holds what the GPU test relies on;
* periodogram.LombScargle.autofrequency is astropy's grid, and what the device does not do raises NotImplementedError;
* the header's MTG_LS_* are the engine's, the entry is declared, exported and bound with the header's arity.
"""
import os
import re

import numpy as np
import pytest

import lomb_scargle_numpy
from mind_the_gaps_amd import engine
from mind_the_gaps_amd.periodogram import LombScargle

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = np.load(os.path.join(HERE, "golden", "lomb_scargle_golden.npz"))
CASES = [str(c) for c in FIX["cases"]]


def test_fixture_layout():
    assert CASES == ["n5", "n52", "n216", "n789", "fast216"]
    shapes = {c: (len(FIX[c + "/t"]), len(FIX[c + "/freqs"])) for c in CASES}
    assert shapes == {"n5": (5, 7), "n52": (52, 130), "n216": (216, 300), "n789": (789, 400), "fast216": (216, 300)}
    for c in CASES:
        t, f = FIX[c + "/t"], FIX[c + "/freqs"]
        assert np.all(np.diff(t) > 0) and 57000 < t[0] < 59500 and np.all(f > 0)
        assert np.max(np.diff(t)) > 0.1 * (t[-1] - t[0])          # the gap
        for tag in "wu":
            assert FIX["%s/%s_det_min" % (c, tag)] >= 0.05 and FIX["%s/%s_rho" % (c, tag)] <= 1e-9
            std = FIX["%s/%s_standard" % (c, tag)]
            assert std.shape == f.shape and np.all((std > 0) & (std < 1))
            # the four normalisations are one truth
            assert np.allclose(FIX["%s/%s_model" % (c, tag)], std / (1 - std), rtol=1e-13)
            assert np.allclose(FIX["%s/%s_log" % (c, tag)], -np.log1p(-std), rtol=1e-13)
            assert np.allclose(FIX["%s/%s_psd" % (c, tag)], std * FIX["%s/%s_psd_factor" % (c, tag)], rtol=1e-13)
    T = FIX["fast216/t"][-1] - FIX["fast216/t"][0]
    assert 1e5 < FIX["fast216/freqs"].max() * T <= 1e6


@pytest.mark.parametrize("case", ["n216", "fast216"])
def test_numpy_tau_free_formula_within_rho(case):
    t, y, dy, f = (FIX["%s/%s" % (case, k)] for k in ("t", "y", "dy", "freqs"))
    for tag, err in (("w", dy), ("u", None)):
        got = lomb_scargle_numpy.power(t, y, err, f)
        e = float(np.max(np.abs(got - FIX["%s/%s_standard" % (case, tag)])))
        print("\nnumpy %s %s: max error %.3g, stored rho %.3g" % (case, tag, e, FIX["%s/%s_rho" % (case, tag)]))
        assert e <= FIX["%s/%s_rho" % (case, tag)]
        for norm in ("model", "log", "psd"):
            ref = FIX["%s/%s_%s" % (case, tag, norm)]
            assert np.allclose(lomb_scargle_numpy.power(t, y, err, f, norm), ref, rtol=0, atol=1e-8 * np.max(np.abs(ref)))


def test_autofrequency_is_astropys_grid():
    t = np.array([3.0, 4.5, 7.0, 11.0, 23.0])
    ls = LombScargle(t, np.zeros(5))
    T, n = 20.0, 5
    f = ls.autofrequency()
    df = 1.0 / (5 * T)
    assert f[0] == 0.5 * df and np.allclose(np.diff(f), df, rtol=1e-12)
    assert len(f) == int(np.round(1 + (5 * n / (2 * T) - 0.5 * df) / df)) and abs(f[-1] - 5 * n / (2 * T)) <= df
    g = ls.autofrequency(samples_per_peak=10, nyquist_factor=2, minimum_frequency=0.1, maximum_frequency=0.4)
    assert g[0] == 0.1 and np.allclose(np.diff(g), 1.0 / (10 * T), rtol=1e-12) and len(g) == 61


def test_what_the_device_does_not_do_is_refused_by_name():
    t, y = np.arange(6.0), np.zeros(6)
    for kw in (dict(nterms=2), dict(fit_mean=False), dict(center_data=False)):
        with pytest.raises(NotImplementedError, match=list(kw)[0]):
            LombScargle(t, y, **kw)
    with pytest.raises(ValueError):
        LombScargle(t, y, normalization="power")
    with pytest.raises(ValueError):
        LombScargle(t, np.zeros((2, 5)))


def test_entry_is_declared_exported_and_bound():
    text = open(os.path.join(os.path.dirname(HERE), "include", "mtg.h")).read()
    defs = dict(re.findall(r"#define\s+(MTG_LS_\w+)\s+(\d+)", text))
    assert {k: int(v) for k, v in defs.items()} == {"MTG_LS_STANDARD": engine.LS_STANDARD, "MTG_LS_MODEL": engine.LS_MODEL,
                                                    "MTG_LS_LOG": engine.LS_LOG, "MTG_LS_PSD": engine.LS_PSD}
    assert engine.LS_NORMALIZATIONS == {"standard": 0, "model": 1, "log": 2, "psd": 3}
    decl = re.search(r"MTG_API\s+int\s+mtg_lomb_scargle\s*\(([^;]*)\)\s*;", text)
    params = re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).split(",")
    assert "mtg_lomb_scargle" in engine.EXPORTS
    lib = engine.load_library()
    assert lib.mtg_lomb_scargle.argtypes is not None and len(lib.mtg_lomb_scargle.argtypes) == len(params) == 8
    assert callable(engine.Engine.lomb_scargle)
    # no context: an argument error, nothing touched
    assert lib.mtg_lomb_scargle(None, 1, None, 0, 1, None, None, None) == engine.E_ARG
