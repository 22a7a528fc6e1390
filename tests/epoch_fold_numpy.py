"""float64 restatement of mtg_epoch_fold / mtg_phase_fold (include/mtg.h) in numpy, and the exact bin rule in rational
arithmetic.  Sums in the order of the definition (samples ascending into a bin, bins ascending); the bin by the
two-product rule of csrc/mtg_ls_phase.h (mtg_cycles_bin), the products split by Veltkamp / Dekker since numpy has no fma."""
from fractions import Fraction

import numpy as np

U = 2.0 ** -53
NORMALIZATIONS = ("standard", "model", "log", "psd")


def _split(a):
    c = 134217729.0 * a          # 2^27 + 1
    hi = c - (c - a)
    return hi, a - hi


def two_prod(a, b):
    """a b = p + e exactly (no overflow or underflow)"""
    a, b = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64))
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def bins(f, te, nbins):
    """floor(nbins frac(f te)) of every te, the product taken exactly: the device's rule"""
    nb = float(nbins)
    p, pe = two_prod(f, te)
    q = p - np.rint(p)
    hi, lo = two_prod(nb, q)
    n = np.rint(hi)
    s = (hi - n) + (lo + nb * pe)
    b = n.astype(np.int64) - np.where(s < 0.0, 1, 0)
    return np.where(b < 0, b + nbins, b)


def rounded_bins(f, te, nbins):
    """what the rounded product gives: numpy's (te f) % 1"""
    return np.floor(((np.asarray(te) * f) % 1) * nbins).astype(np.int64)


def exact_phase(f, te):
    """frac(f te) of the stored doubles as a Fraction in [0, 1)"""
    x = Fraction(float(f)) * Fraction(float(te))
    return x - (x.numerator // x.denominator)


def exact_bins(f, te, nbins):
    return np.array([int(exact_phase(f, x) * nbins) for x in np.atleast_1d(te)], dtype=np.int64)


def weights(y, dy, weighted):
    """w, ybar, r, YY, sw as mtg_lomb_scargle defines them"""
    y = np.asarray(y, dtype=np.float64)
    if weighted:
        sw = np.sum(1.0 / np.asarray(dy, dtype=np.float64) ** 2)
        w = (1.0 / np.asarray(dy, dtype=np.float64) ** 2) / sw
    else:
        sw = float(len(y))
        w = np.full(len(y), 1.0 / sw)
    ybar = np.sum(w * y)
    r = y - ybar
    return w, ybar, r, np.sum(w * r * r), sw


def fold(t, y, dy, f, nbins, time_0, weighted):
    """count, W_b, S_b of one frequency"""
    w, _, r, _, _ = weights(y, dy, weighted)
    b = bins(f, np.asarray(t, dtype=np.float64) - time_0, nbins)
    return (np.bincount(b, minlength=nbins), np.bincount(b, weights=w, minlength=nbins),
            np.bincount(b, weights=w * r, minlength=nbins))


def reduce_bins(wsum, wrsum):
    """p = sum over the bins with weight of S^2 / W, ascending, one rounding per operation (what the kernel does)"""
    p = np.zeros(np.shape(wsum)[:-1])
    for b in range(np.shape(wsum)[-1]):
        W, S = wsum[..., b], wrsum[..., b]
        with np.errstate(divide="ignore", invalid="ignore"):
            p = np.where(W > 0.0, p + (S * S) / W, p)
    return p


def normalize(p, YY, sw, normalization):
    with np.errstate(divide="ignore", invalid="ignore"):
        if normalization == "standard":
            return p / YY
        if normalization == "model":
            return p / (YY - p)
        if normalization == "log":
            return -np.log(1.0 - p / YY)
        return p * (0.5 * sw)


def dnorm_dstandard(P, YY, sw, normalization):
    """|d normalised / d standard| at standard power P: what an error of the standard power becomes"""
    if normalization == "standard":
        return np.ones_like(P)
    if normalization == "model":
        return 1.0 / (1.0 - P) ** 2
    if normalization == "log":
        return 1.0 / (1.0 - P)
    return np.full_like(P, YY * 0.5 * sw)


def power(t, y, dy, freqs, nbins, time_0, weighted, normalization="standard"):
    _, _, _, YY, sw = weights(y, dy, weighted)
    p = np.array([reduce_bins(*fold(t, y, dy, f, nbins, time_0, weighted)[1:]) for f in np.atleast_1d(freqs)])
    return normalize(p, YY, sw, normalization)


def bound(rho, N):
    """max(10 rho, 64 sqrt(N) u): the error allowed on the standard power"""
    return max(10.0 * rho, 64.0 * np.sqrt(N) * U)
