#!/usr/bin/env python3
"""Writes tests/golden/wwz_golden.npz: 50-digit truths of Foster's weighted wavelet Z-transform (mtg_wwz;
tests/test_wwz_cpu.py, tests/test_wwz_gpu.py).

The sampling and data (t, y, dy) are those of the cases n52, n216, n789 and fast216 of
tests/golden/lomb_scargle_golden.npz, which is only read.  Per case
    freqs  twelve frequencies from 1 / T_span to the mean Nyquist rate N / (2 T_span), geometrically spaced, and three
           beyond it (1.15, 1.4 and 1.8 times)
    taus   eight window centres: six spread over the span, the middle of the widest gap, and one 2 % of the span beyond
           the last sample
    decay  1 / (8 pi^2), 0.001 and 0
and both weightings (w: s_n = dy^-2, u: s_n = 1).  mpmath evaluates Foster's formulas as written in include/mtg.h from
te_n = fl(t_n - tau) -- no cut, no rescaling of the weights -- and the file holds, each [3 decays][8 taus][15 freqs],
    <case>/<w|u>_power, _z, _amplitude, _neff, _vx   P, Z, sqrt(a^2 + b^2), N_eff and V_x, rounded to float64
    <case>/<w|u>_kappa       the 2-norm condition number of [[1, C, S], [C, CC, CS], [S, CS, SS]]
    <case>/<w|u>_rho, _rho_a the largest error of tests/wwz_numpy.py (plain float64) in P, and in the amplitude in units
                             of sqrt(V_x), over the entries with N_eff >= 4
Entries whose true N_eff < 4 are left out of the accuracy comparisons (three parameters are fitted, and Z changes sign at
3); this script asserts that they are at most 10 % of any case's entries.

Run on the CPU (a few minutes):  python3 scripts/make_wwz_golden.py
"""
import os
import sys
from concurrent.futures import ProcessPoolExecutor

import mpmath as mp
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import wwz_numpy  # noqa: E402

mp.mp.dps = 50
CASES = ("n52", "n216", "n789", "fast216")
DECAYS = (wwz_numpy.DECAY, 0.001, 0.0)
BEYOND = (1.15, 1.4, 1.8)
QUANTITIES = ("power", "z", "amplitude", "neff", "vx", "kappa")
NEFF_MIN, LEFT_OUT_MAX = 4.0, 0.10


def grid(t):
    """the frequencies and window centres of a case"""
    span = t[-1] - t[0]
    nyquist = 0.5 * len(t) / span
    freqs = np.concatenate([np.geomspace(1.0 / span, nyquist, 12), nyquist * np.array(BEYOND)])
    gap = int(np.argmax(np.diff(t)))
    taus = np.concatenate([t[0] + span * np.array([0.03, 0.21, 0.4, 0.58, 0.77, 0.96]), [0.5 * (t[gap] + t[gap + 1]), t[-1] + 0.02 * span]])
    return freqs, taus


def one_pair(args):
    """one (tau, f) -> {(tag, decay index): (P, Z, A, N_eff, V_x, kappa)} as floats"""
    t, y, dy, tau, f = args
    mp.mp.dps = 50
    te = [mp.mpf(float(v)) for v in (t - tau)]          # fl(t_n - tau): the definition's one IEEE subtraction
    ym = [mp.mpf(float(v)) for v in y]
    fm = mp.mpf(float(f))
    z = [fm * x for x in te]
    co = [mp.cos(2 * mp.pi * v) for v in z]
    si = [mp.sin(2 * mp.pi * v) for v in z]
    out = {}
    for tag in ("w", "u"):
        s = [1 / mp.mpf(float(v)) ** 2 for v in dy] if tag == "w" else [mp.mpf(1)] * len(t)
        ssum = mp.fsum(s)
        ybar = mp.fsum(a * b for a, b in zip(s, ym)) / ssum
        r = [v - ybar for v in ym]
        for ci, c in enumerate(DECAYS):
            k = 4 * mp.pi ** 2 * mp.mpf(float(c))
            w = [sn * mp.exp(-k * v * v) for sn, v in zip(s, z)]
            sw = mp.fsum(w)
            mean = lambda a: mp.fsum(wn * an for wn, an in zip(w, a)) / sw   # noqa: E731
            C, S = mean(co), mean(si)
            CC, CS = mean([v * v for v in co]), mean([a * b for a, b in zip(co, si)])
            SS = 1 - CC
            X, XX = mean(r), mean([v * v for v in r])
            XC, XS = mean([a * b for a, b in zip(r, co)]), mean([a * b for a, b in zip(r, si)])
            neff = sw * sw / mp.fsum(v * v for v in w)
            vx = XX - X * X
            cc, ss, cs, xc, xs = CC - C * C, SS - S * S, CS - C * S, XC - X * C, XS - X * S
            det = cc * ss - cs * cs
            vy = (ss * xc * xc + cc * xs * xs - 2 * cs * xc * xs) / det
            a, b = (ss * xc - cs * xs) / det, (cc * xs - cs * xc) / det
            ev = mp.eigsy(mp.matrix([[1, C, S], [C, CC, CS], [S, CS, SS]]), eigvals_only=True)
            kappa = max(abs(v) for v in ev) / min(abs(v) for v in ev)
            out[tag, ci] = (float(vy / vx), float((neff - 3) * vy / (2 * (vx - vy))), float(mp.sqrt(a * a + b * b)), float(neff),
                            float(vx), float(kappa))
    return out


def main():
    src = np.load(os.path.join(ROOT, "tests", "golden", "lomb_scargle_golden.npz"))
    store = {"cases": np.array(CASES), "decays": np.array(DECAYS)}
    with ProcessPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
        for name in CASES:
            t, y, dy = (src["%s/%s" % (name, k)] for k in ("t", "y", "dy"))
            freqs, taus = grid(t)
            T, F = len(taus), len(freqs)
            res = list(pool.map(one_pair, [(t, y, dy, tau, f) for tau in taus for f in freqs], chunksize=2))
            store["%s/freqs" % name], store["%s/taus" % name] = freqs, taus
            left_out = 0
            for tag, err in (("w", dy), ("u", None)):
                truth = {q: np.empty((len(DECAYS), T, F)) for q in QUANTITIES}
                for ci in range(len(DECAYS)):
                    for e, r in enumerate(res):
                        for qi, q in enumerate(QUANTITIES):
                            truth[q][ci, e // F, e % F] = r[tag, ci][qi]
                keep = truth["neff"] >= NEFF_MIN
                left_out += int(np.sum(~keep))
                rho = rho_a = 0.0
                for ci, c in enumerate(DECAYS):
                    got = wwz_numpy.wwz(t, y, err, freqs, taus, decay=c, weighted=tag == "w")
                    k = keep[ci]
                    rho = max(rho, float(np.max(np.abs(got["power"] - truth["power"][ci])[k])))
                    rho_a = max(rho_a, float(np.max((np.abs(got["amplitude"] - truth["amplitude"][ci]) / np.sqrt(truth["vx"][ci]))[k])))
                for q in QUANTITIES:
                    store["%s/%s_%s" % (name, tag, q)] = truth[q]
                store["%s/%s_rho" % (name, tag)] = np.float64(rho)
                store["%s/%s_rho_a" % (name, tag)] = np.float64(rho_a)
                print("%-8s %s  n %4d  kappa max (kept) %.3g  rho %.3g  rho_a %.3g  neff min %.3g  kept %d / %d" %
                      (name, tag, len(t), truth["kappa"][keep].max(), rho, rho_a, truth["neff"].min(), keep.sum(), keep.size), flush=True)
            share = left_out / (2.0 * len(DECAYS) * T * F)
            print("%-8s left out (N_eff < %g): %.1f %%" % (name, NEFF_MIN, 100 * share), flush=True)
            assert share <= LEFT_OUT_MAX, (name, share)
    path = os.path.join(ROOT, "tests", "golden", "wwz_golden.npz")
    np.savez_compressed(path, **store)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
