"""The multi-harmonic floating-mean Lomb-Scargle periodogram in plain numpy float64, as astropy's chi2 method writes it
(fit_mean=True, center_data=True): the design matrix (1, sin phi, cos phi, ..., sin K phi, cos K phi) at elapsed times,
X^T W X, X^T W r and np.linalg.solve.  What scripts/make_lomb_scargle_multi_golden.py measures its rho with and what
tests/test_lomb_scargle_multi_cpu.py holds to the 50-digit fixture.  Not a fallback of the package: tests only."""
import numpy as np

from lomb_scargle_numpy import normalize


def design(t, f, nterms):
    """-> [N][2 nterms + 1]"""
    phi = 2.0 * np.pi * f * (t - t[0])
    cols = [np.ones_like(phi)]
    for m in range(1, nterms + 1):
        cols += [np.sin(m * phi), np.cos(m * phi)]
    return np.stack(cols, axis=1)


def power(t, y, dy, freqs, nterms=1, normalization="standard", return_kappa=False):
    """dy None: unweighted.  -> [F], with return_kappa also the 2-norm condition number of every A = X^T W X [F]"""
    t, y, freqs = (np.asarray(a, dtype=np.float64) for a in (t, y, freqs))
    n = len(t)
    inv = np.ones(n) if dy is None else np.asarray(dy, dtype=np.float64) ** -2.0
    sw = inv.sum()
    w = inv / sw
    r = y - np.sum(w * y)
    YY = np.sum(w * r * r)
    p, kappa = np.empty(len(freqs)), np.empty(len(freqs))
    for k, f in enumerate(freqs):
        X = design(t, f, nterms)
        A = X.T @ (w[:, None] * X)
        b = X.T @ (w * r)
        p[k] = b @ np.linalg.solve(A, b)
        if return_kappa:
            kappa[k] = np.linalg.cond(A, 2)
    out = normalize(p, YY, sw, normalization)
    return (out, kappa) if return_kappa else out
