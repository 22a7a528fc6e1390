#!/usr/bin/env python3
"""Writes tests/golden/lomb_scargle_golden.npz: inputs and 50-digit truths of the floating-mean Lomb-Scargle periodogram
(mtg_lomb_scargle; tests/test_lomb_scargle_cpu.py, tests/test_lomb_scargle_gpu.py).

Every case is a light curve at an absolute epoch of ~58000 with irregular sampling and a gap, a sinusoid plus noise, and
heteroscedastic error bars.  The truth is evaluated with mpmath from exactly the stored doubles by astropy's form
    tan(2 w tau) = 2 CS / (CC - SS),  p = YC_tau^2 / CC_tau + YS_tau^2 / SS_tau
at the ABSOLUTE times -- another algebraic route than the device's tau-free formula at elapsed times -- weighted
(w = dy^-2 / sum dy^-2) and unweighted, in the four normalisations.  rho is the largest error of plain numpy float64
evaluating the tau-free formula at elapsed times (tests/lomb_scargle_numpy.py), standard normalisation.

Two conditions keep the tests from hiding a failure and are asserted here: every CC SS - CS^2 >= 0.05 (no frequency
where the fit is nearly degenerate and every evaluation is poor), and rho <= 1e-9.  A light curve (the "fast" case: its
frequencies, random up to 1e3 cycles per unit of time, f T up to 1e6 cycles) is drawn again until the first holds.

Run on the CPU:  python3 scripts/make_lomb_scargle_golden.py
"""
import os
import sys

import mpmath as mp
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lomb_scargle_numpy  # noqa: E402

mp.mp.dps = 50
SEED = 7
DET_MIN, RHO_MAX = 0.05, 1e-9
# name, n, F, fast
CASES = (("n5", 5, 7, False), ("n52", 52, 130, False), ("n216", 216, 300, False), ("n789", 789, 400, False),
         ("fast216", 216, 300, True))


def lightcurve(rng, n):
    span = 1000.0
    t = np.sort(rng.uniform(0.0, span, size=3 * n))
    t = t[(t < 0.45 * span) | (t > 0.6 * span)]          # a gap
    t = 58000.0 + np.sort(rng.choice(t, size=n, replace=False))
    T = t[-1] - t[0]
    f0 = (0.31 * n) / T
    dy = rng.uniform(0.05, 0.3, size=n)
    y = 3.0 + 0.8 * np.sin(2.0 * np.pi * f0 * t + 0.7) + dy * rng.standard_normal(n)
    return t, y, dy


def det_min_float64(t, dy, freqs):
    w = np.ones(len(t)) if dy is None else dy ** -2.0
    w = w / w.sum()
    x = 2.0 * np.pi * freqs[:, None] * (t - t[0])[None, :]
    c, s = np.cos(x), np.sin(x)
    C, S = c @ w, s @ w
    return float(np.min(((c * c) @ w - C * C) * ((s * s) @ w - S * S) - ((c * s) @ w - C * S) ** 2))


def truth(t, y, dy, freqs):
    """-> dict of [F] float64 per normalisation, min determinant, (YY, sw) as floats"""
    n = len(t)
    tm = [mp.mpf(float(v)) for v in t]
    ym = [mp.mpf(float(v)) for v in y]
    inv = [mp.mpf(1) if dy is None else 1 / mp.mpf(float(v)) ** 2 for v in (t if dy is None else dy)]
    sw = mp.fsum(inv)
    w = [v / sw for v in inv]
    ybar = mp.fsum(wi * yi for wi, yi in zip(w, ym))
    r = [yi - ybar for yi in ym]
    YY = mp.fsum(wi * ri * ri for wi, ri in zip(w, r))
    out = {k: np.empty(len(freqs)) for k in lomb_scargle_numpy.NORMALIZATIONS}
    det_min = mp.inf
    for k, f in enumerate(freqs):
        om = 2 * mp.pi * mp.mpf(float(f))
        c = [mp.cos(om * ti) for ti in tm]
        s = [mp.sin(om * ti) for ti in tm]
        C, S = mp.fsum(wi * ci for wi, ci in zip(w, c)), mp.fsum(wi * si for wi, si in zip(w, s))
        CC = mp.fsum(wi * ci * ci for wi, ci in zip(w, c)) - C * C
        SS = mp.fsum(wi * si * si for wi, si in zip(w, s)) - S * S
        CS = mp.fsum(wi * ci * si for wi, ci, si in zip(w, c, s)) - C * S
        det_min = min(det_min, CC * SS - CS * CS)
        tau = mp.atan2(2 * CS, CC - SS) / (2 * om)
        ct = [mp.cos(om * (ti - tau)) for ti in tm]
        st = [mp.sin(om * (ti - tau)) for ti in tm]
        Ct, St = mp.fsum(wi * ci for wi, ci in zip(w, ct)), mp.fsum(wi * si for wi, si in zip(w, st))
        YCt = mp.fsum(wi * ri * ci for wi, ri, ci in zip(w, r, ct))
        YSt = mp.fsum(wi * ri * si for wi, ri, si in zip(w, r, st))
        CCt = mp.fsum(wi * ci * ci for wi, ci in zip(w, ct)) - Ct * Ct
        SSt = mp.fsum(wi * si * si for wi, si in zip(w, st)) - St * St
        p = YCt * YCt / CCt + YSt * YSt / SSt
        out["standard"][k] = float(p / YY)
        out["model"][k] = float(p / (YY - p))
        out["log"][k] = float(-mp.log(1 - p / YY))
        out["psd"][k] = float(p * sw / 2)
    return out, float(det_min), float(YY), float(sw)


def main():
    rng = np.random.default_rng(SEED)
    store = {}
    for name, n, F, fast in CASES:
        # drawn again until no frequency is nearly degenerate (cheaply, in float64; asserted on the truth below): the
        # light curve with its regular grid, or -- the fast case -- the random frequencies alone
        t, y, dy = lightcurve(rng, n)
        for attempt in range(1000):
            T = t[-1] - t[0]
            freqs = np.sort(rng.uniform(1.0, 1.0e3, size=F)) if fast else np.linspace(1.0 / T, n / T, F)
            if min(det_min_float64(t, dy, freqs), det_min_float64(t, None, freqs)) >= 1.5 * DET_MIN:
                break
            if not fast:
                t, y, dy = lightcurve(rng, n)
        res = {tag: truth(t, y, err, freqs) for tag, err in (("w", dy), ("u", None))}
        for tag, err in (("w", dy), ("u", None)):
            tr, det_min, YY, sw = res[tag]
            rho = float(np.max(np.abs(lomb_scargle_numpy.power(t, y, err, freqs) - tr["standard"])))
            assert det_min >= DET_MIN and rho <= RHO_MAX, (name, tag, det_min, rho)
            print("%-8s %s  n %4d  F %4d  f T max %.3g  min det %.3f  rho %.3g  max standard %.4f" %
                  (name, tag, n, F, freqs.max() * T, det_min, rho, tr["standard"].max()))
            for k, v in tr.items():
                store["%s/%s_%s" % (name, tag, k)] = v
            store["%s/%s_rho" % (name, tag)] = np.float64(rho)
            store["%s/%s_psd_factor" % (name, tag)] = np.float64(0.5 * sw * YY)   # d psd / d standard
            store["%s/%s_det_min" % (name, tag)] = np.float64(det_min)
        for k, v in (("t", t), ("y", y), ("dy", dy), ("freqs", freqs)):
            store["%s/%s" % (name, k)] = v
    store["cases"] = np.array([c[0] for c in CASES])
    path = os.path.join(ROOT, "tests", "golden", "lomb_scargle_golden.npz")
    np.savez_compressed(path, **store)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
