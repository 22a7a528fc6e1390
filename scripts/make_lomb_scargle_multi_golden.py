#!/usr/bin/env python3
"""Writes tests/golden/lomb_scargle_multi_golden.npz: 50-digit truths of the multi-harmonic Lomb-Scargle periodogram
(mtg_lomb_scargle_multi; tests/test_lomb_scargle_multi_cpu.py, tests/test_lomb_scargle_multi_gpu.py).

The inputs (t, y, dy, freqs) are those of the cases n52, n216, n789 and fast216 of tests/golden/lomb_scargle_golden.npz,
which is only read.  For K in {2, 3, 5}, weighted (w = dy^-2 / sum dy^-2) and unweighted (w = 1 / N), with
r = y - sum w y, YY = sum w r^2 and phi_n = 2 pi f (t_n - t_0), mpmath evaluates from exactly the stored doubles
    x_n = (1, sin phi_n, cos phi_n, ..., sin K phi_n, cos K phi_n),  A = sum w x x^T,  b = sum w r x,  p = b^T A^-1 b
and the four normalisations of p.  Per (case, weighting, K) the file holds
    <case>/<w|u>_k<K>_<normalisation>  [F] the truth, rounded to float64
    <case>/<w|u>_k<K>_kappa            [F] the 2-norm condition number of A (2K+1 x 2K+1), in the 50-digit arithmetic
    <case>/<w|u>_k<K>_rho              the largest error of tests/lomb_scargle_multi_numpy.py (plain float64: design
                                       matrix, X^T W X, np.linalg.solve), standard normalisation
    <case>/<w|u>_psd_factor, _YY       0.5 sum 1 / sigma^2 (unweighted: 0.5 N) and YY: d psd / d standard is their product
The sums of sin m phi cos m' phi products are formed from C_m = sum w cos m phi, S_m = sum w sin m phi (m <= 2 K) by the
product formulas, which are exact; the float64 reference forms them from the design matrix itself.

Run on the CPU (a few minutes):  python3 scripts/make_lomb_scargle_multi_golden.py
"""
import os
import sys
from concurrent.futures import ProcessPoolExecutor

import mpmath as mp
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lomb_scargle_multi_numpy  # noqa: E402
from lomb_scargle_numpy import NORMALIZATIONS  # noqa: E402

mp.mp.dps = 50
CASES = ("n52", "n216", "n789", "fast216")
NTERMS = (2, 3, 5)
KMAX = max(NTERMS)
KAPPA_MAX, RHO_MAX = 1e6, 1e-9


def matrix(C, S, K):
    """A = sum w x x^T from C_m, S_m (m = 0 .. 2K), x = (1, sin phi, cos phi, ..., sin K phi, cos K phi)"""
    cm = lambda m: C[abs(m)]
    sm = lambda m: S[m] if m >= 0 else -S[-m]
    n = 2 * K + 1
    A = mp.zeros(n, n)
    A[0, 0] = C[0]
    for a in range(1, K + 1):
        A[0, 2 * a - 1] = A[2 * a - 1, 0] = S[a]
        A[0, 2 * a] = A[2 * a, 0] = C[a]
        for b in range(1, K + 1):
            A[2 * a - 1, 2 * b - 1] = (cm(a - b) - cm(a + b)) / 2      # sin a phi sin b phi
            A[2 * a, 2 * b] = (cm(a - b) + cm(a + b)) / 2              # cos a phi cos b phi
            A[2 * a - 1, 2 * b] = (sm(a + b) + sm(a - b)) / 2          # sin a phi cos b phi
            A[2 * b, 2 * a - 1] = A[2 * a - 1, 2 * b]
    return A


def one_frequency(args):
    """-> {(tag, K): (p / YY, p / (YY - p), -log(1 - p / YY), p sw / 2, kappa)} as floats"""
    t, y, dy, f = args
    mp.mp.dps = 50
    n = len(t)
    te = [mp.mpf(float(v)) - mp.mpf(float(t[0])) for v in t]
    ym = [mp.mpf(float(v)) for v in y]
    om = 2 * mp.pi * mp.mpf(float(f))
    # powers of exp(i phi_n): cos m phi_n, sin m phi_n for m = 0 .. 2 KMAX
    cs = []
    for x in te:
        c1, s1 = mp.cos(om * x), mp.sin(om * x)
        row, c, s = [(mp.mpf(1), mp.mpf(0))], mp.mpf(1), mp.mpf(0)
        for _ in range(2 * KMAX):
            c, s = c * c1 - s * s1, s * c1 + c * s1
            row.append((c, s))
        cs.append(row)
    out = {}
    for tag in ("w", "u"):
        inv = [1 / mp.mpf(float(v)) ** 2 for v in dy] if tag == "w" else [mp.mpf(1)] * n
        sw = mp.fsum(inv)
        w = [v / sw for v in inv]
        ybar = mp.fsum(wi * yi for wi, yi in zip(w, ym))
        wr = [wi * (yi - ybar) for wi, yi in zip(w, ym)]
        YY = mp.fsum(wri * (yi - ybar) for wri, yi in zip(wr, ym))
        C = [mp.fsum(wi * row[m][0] for wi, row in zip(w, cs)) for m in range(2 * KMAX + 1)]
        S = [mp.fsum(wi * row[m][1] for wi, row in zip(w, cs)) for m in range(2 * KMAX + 1)]
        YC = [mp.fsum(wi * row[m][0] for wi, row in zip(wr, cs)) for m in range(KMAX + 1)]
        YS = [mp.fsum(wi * row[m][1] for wi, row in zip(wr, cs)) for m in range(KMAX + 1)]
        for K in NTERMS:
            A = matrix(C, S, K)
            b = mp.matrix([YC[0]] + [v for a in range(1, K + 1) for v in (YS[a], YC[a])])
            p = (b.T * mp.lu_solve(A, b))[0]
            ev = mp.eigsy(A, eigvals_only=True)
            kappa = max(abs(v) for v in ev) / min(abs(v) for v in ev)
            out[tag, K] = (float(p / YY), float(p / (YY - p)), float(-mp.log(1 - p / YY)), float(p * sw / 2), float(kappa),
                           float(sw / 2), float(YY))
    return out


def main():
    src = np.load(os.path.join(ROOT, "tests", "golden", "lomb_scargle_golden.npz"))
    store = {}
    with ProcessPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
        for name in CASES:
            t, y, dy, freqs = (src["%s/%s" % (name, k)] for k in ("t", "y", "dy", "freqs"))
            res = list(pool.map(one_frequency, [(t, y, dy, f) for f in freqs], chunksize=4))
            for tag, err in (("w", dy), ("u", None)):
                store["%s/%s_psd_factor" % (name, tag)] = np.float64(res[0][tag, NTERMS[0]][5])
                store["%s/%s_YY" % (name, tag)] = np.float64(res[0][tag, NTERMS[0]][6])
                for K in NTERMS:
                    cols = np.array([r[tag, K][:5] for r in res]).T
                    for k, norm in enumerate(NORMALIZATIONS):
                        store["%s/%s_k%d_%s" % (name, tag, K, norm)] = cols[k]
                    kappa = cols[4]
                    rho = float(np.max(np.abs(lomb_scargle_multi_numpy.power(t, y, err, freqs, K) - cols[0])))
                    assert kappa.max() <= KAPPA_MAX and rho <= RHO_MAX, (name, tag, K, kappa.max(), rho)
                    store["%s/%s_k%d_kappa" % (name, tag, K)] = kappa
                    store["%s/%s_k%d_rho" % (name, tag, K)] = np.float64(rho)
                    print("%-8s %s K %d  n %4d  F %4d  kappa max %.3g  rho %.3g  max standard %.4f" %
                          (name, tag, K, len(t), len(freqs), kappa.max(), rho, cols[0].max()), flush=True)
    store["cases"] = np.array(CASES)
    store["nterms"] = np.array(NTERMS)
    path = os.path.join(ROOT, "tests", "golden", "lomb_scargle_multi_golden.npz")
    np.savez_compressed(path, **store)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
