"""Foster's weighted wavelet Z-transform (1996) in plain float64 numpy: the formulas of include/mtg.h (mtg_wwz) written
down once more, for tests/test_wwz_cpu.py, tests/test_wwz_gpu.py and scripts/make_wwz_golden.py.  Its error against the
50-digit truth of tests/golden/wwz_golden.npz is the rho of the accuracy bounds.

The weights of one (tau, f) are taken relative to the largest of them (every quantity is invariant under a common factor,
and plain float64 would otherwise return 0 / 0 for a centre in a gap); nothing is cut.
"""
import numpy as np

DECAY = 1.0 / (8.0 * np.pi ** 2)
STATISTICS = ("power", "z", "amplitude")
U = 2.0 ** -53


def stat_weights(y, dy, weighted):
    """-> (s [N], ybar): the statistical weights (sigma^-2 / sum sigma^-2, or 1) and the weighted mean of y"""
    y = np.asarray(y, dtype=np.float64)
    if weighted:
        s = np.asarray(dy, dtype=np.float64) ** -2.0
        s = s / s.sum()
        return s, float(np.sum(s * y))
    return np.ones_like(y), float(y.mean())


def wwz(t, y, dy, freqs, taus, decay=DECAY, weighted=True):
    """-> dict of [T][F] arrays: power P, z, amplitude, neff, vx and kappa (the 2-norm condition number of the normalised
    normal matrix [[1, C, S], [C, CC, CS], [S, CS, SS]])"""
    t = np.asarray(t, dtype=np.float64)
    freqs = np.atleast_1d(np.asarray(freqs, dtype=np.float64))
    taus = np.atleast_1d(np.asarray(taus, dtype=np.float64))
    s, ybar = stat_weights(y, dy, weighted)
    r = np.asarray(y, dtype=np.float64) - ybar
    out = {k: np.empty((len(taus), len(freqs))) for k in ("power", "z", "amplitude", "neff", "vx", "kappa")}
    for j, tau in enumerate(taus):
        z = freqs[:, None] * (t - tau)[None, :]
        e = 4.0 * np.pi ** 2 * decay * z * z
        w = s[None, :] * np.exp(-(e - e.min(axis=1, keepdims=True)))
        sw = w.sum(axis=1)
        co, si = np.cos(2.0 * np.pi * z), np.sin(2.0 * np.pi * z)
        mean = lambda a: (w * a).sum(axis=1) / sw   # noqa: E731
        C, S, CC, CS = mean(co), mean(si), mean(co * co), mean(co * si)
        SS = 1.0 - CC
        X, XX, XC, XS = mean(r[None, :]), mean((r * r)[None, :]), mean(r[None, :] * co), mean(r[None, :] * si)
        neff = sw * sw / (w * w).sum(axis=1)
        vx = XX - X * X
        cc, ss, cs, xc, xs = CC - C * C, SS - S * S, CS - C * S, XC - X * C, XS - X * S
        with np.errstate(divide="ignore", invalid="ignore"):
            det = cc * ss - cs * cs
            det = np.where(det > 0, det, np.nan)
            vy = (ss * xc * xc + cc * xs * xs - 2.0 * cs * xc * xs) / det
            a, b = (ss * xc - cs * xs) / det, (cc * xs - cs * xc) / det
            out["power"][j] = np.where(vx > 0, vy / vx, np.nan)
            out["z"][j] = np.where(vx - vy > 0, (neff - 3.0) * vy / (2.0 * (vx - vy)), np.nan)
        out["amplitude"][j] = np.sqrt(a * a + b * b)
        out["neff"][j] = neff
        out["vx"][j] = vx
        for k in range(len(freqs)):
            A = np.array([[1.0, C[k], S[k]], [C[k], CC[k], CS[k]], [S[k], CS[k], SS[k]]])
            out["kappa"][j, k] = np.linalg.cond(A, 2)
    return out


def bound_power(rho, n, kappa):
    """|P - truth| <= max(10 rho, 64 sqrt(N) u kappa): the bound of tests/test_lomb_scargle_multi_gpu.py"""
    return np.maximum(10.0 * rho, 64.0 * np.sqrt(n) * U * np.asarray(kappa))


def bound_neff_rel(n):
    """|N_eff - truth| <= 64 sqrt(N) u N_eff"""
    return 64.0 * np.sqrt(n) * U


def bound_z(rho, n, kappa, P, neff):
    """the bound of P times |dZ / dP| plus the bound of N_eff times |dZ / dN_eff|, both at the truth:
    Z = (N_eff - 3) P / (2 (1 - P))"""
    with np.errstate(divide="ignore", invalid="ignore"):   # (P = 1: no bound; such entries have N_eff < 4 in the fixture)
        dzdp = np.abs(neff - 3.0) / (2.0 * (1.0 - P) ** 2)
        dzdn = np.abs(P / (2.0 * (1.0 - P)))
    return bound_power(rho, n, kappa) * dzdp + bound_neff_rel(n) * neff * dzdn


def bound_amplitude(rho_a, n, kappa, vx):
    """|A - truth| <= max(10 rho_A, 64 sqrt(N) u kappa) sqrt(V_x), rho_A the helper's error in units of sqrt(V_x)"""
    return np.maximum(10.0 * rho_a, 64.0 * np.sqrt(n) * U * np.asarray(kappa)) * np.sqrt(vx)
