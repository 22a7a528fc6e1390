"""The floating-mean Lomb-Scargle periodogram in plain numpy float64, by the tau-free formula of include/mtg.h
(mtg_lomb_scargle) at elapsed times: what scripts/make_lomb_scargle_golden.py measures its rho with and what
tests/test_lomb_scargle_cpu.py holds to it.  Not a fallback of the package: tests only."""
import numpy as np

NORMALIZATIONS = ("standard", "model", "log", "psd")


def power(t, y, dy, freqs, normalization="standard"):
    """dy None: unweighted.  -> [F]"""
    t, y, freqs = (np.asarray(a, dtype=np.float64) for a in (t, y, freqs))
    n = len(t)
    inv = np.ones(n) if dy is None else np.asarray(dy, dtype=np.float64) ** -2.0
    sw = inv.sum()
    w = inv / sw
    r = y - np.sum(w * y)
    YY = np.sum(w * r * r)
    x = 2.0 * np.pi * freqs[:, None] * (t - t[0])[None, :]
    c, s = np.cos(x), np.sin(x)
    C, S = c @ w, s @ w
    YC, YS = c @ (w * r), s @ (w * r)
    CC = (c * c) @ w - C * C
    SS = (s * s) @ w - S * S
    CS = (c * s) @ w - C * S
    p = (SS * YC * YC + CC * YS * YS - 2.0 * CS * YC * YS) / (CC * SS - CS * CS)
    return normalize(p, YY, sw, normalization)


def normalize(p, YY, sw, normalization):
    if normalization == "standard":
        return p / YY
    if normalization == "model":
        return p / (YY - p)
    if normalization == "log":
        return -np.log(1.0 - p / YY)
    if normalization == "psd":
        return p * (0.5 * sw)
    raise ValueError(normalization)
