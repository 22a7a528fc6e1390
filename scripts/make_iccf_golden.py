"""Writes tests/golden/iccf_golden.npz: exact truths of mtg_iccf (include/mtg.h) for the resident series of the
Lomb-Scargle fixture's cases n5, n52, n216 and n789, each against the companion of tests/cross_numpy.py (M = 7, 61, 300,
523), for the six lag sets of tests/iccf_numpy.py.

Every stored number is a double, hence a rational.  x = fl(t + tau) is BY DEFINITION the rounded double, so which samples
a half uses, their brackets and the counts are taken in float64 and are exact.  Everything after that is exact rational
arithmetic (fractions.Fraction for the units, Python integers over a common denominator for the long sums, which saves the
gcd of every addition): the means, the residuals, the interpolated values, the six sums, C, Va and Vb -- so is the decision
whether a half is NaN.  Only r = C / sqrt(Va Vb) is not rational: mpmath at 50 digits, written as the nearest double and
the double nearest to the rest.

Per case and lag set: <case>/<set>/lags; r_a, r_a_lo, r_b, r_b_lo (NaN by the header's rule), n_a, n_b; rho_a, rho_b, the
error of tests/iccf_numpy.py in each entry; s_a, s_b, the scale S = Cabs / sqrt(Va Vb) + |r| (Vaabs / Va + Vbabs / Vb) / 2
that the one-pass formula's rounding grows with; for "ties" the rows (k, i, j) with fl(t_i + lags[k]) == t2_j.
The bound of the tests is max(10 rho, 64 sqrt(n) u S) per half; so that S cannot make it vacuous, in every case and lag
set at least half of the finite entries must have S <= 100 (asserted below; the largest S is printed and stored).

    python scripts/make_iccf_golden.py        (about a minute on one core)
"""
import os
import sys
from fractions import Fraction

import mpmath
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import iccf_numpy as inp  # noqa: E402

mpmath.mp.dps = 50


def scaled(values, k=None):
    """doubles -> (Python integers m, k) with value = m / 2^k exactly"""
    ratios = [float(v).as_integer_ratio() for v in values]
    need = max([d.bit_length() - 1 for _, d in ratios] + [0])
    k = need if k is None else k
    assert k >= need
    return [n * ((1 << k) // d) for n, d in ratios], k


def residuals(y):
    """y -> integers m and the unit u with y_n - mean(y) = m_n u exactly"""
    ym, k = scaled(y)
    total, n = sum(ym), len(ym)
    return [n * v - total for v in ym], Fraction(1, n << k)


def over_common_denominator(groups, which, power):
    """sum over the groups d -> sums of groups[d][which] / d^power, as (numerator, denominator), not reduced"""
    num, den = 0, 1
    for d, sums in groups.items():
        dp = d ** power
        num, den = num * dp + sums[which] * den, den * dp
    return num, den


def exact_half(tw, W, uw, shift, u, Z, uz):
    """One half at one lag, exactly: the walked series (times tw, residuals W uw) against the interpolated one (node times
    u, residuals Z uz) -> (n, None or (C, Va, Vb, Cabs, Vaabs, Vbabs) as Fractions)"""
    x = tw + shift
    ok = np.flatnonzero((x >= u[0]) & (x <= u[-1]))
    n = len(ok)
    if n < 2:
        return n, None
    p = np.searchsorted(u, x[ok], side="right") - 1
    ints, k = scaled(np.concatenate([u, x[ok]]))
    Ui, Xi = ints[:len(u)], ints[len(u):]
    groups = {}                     # bracket width d -> sums of A, A^2, W A, |W A| with the value v = uz A / d
    sw = sww = 0
    for m, (i, b) in enumerate(zip(ok.tolist(), p.tolist())):
        if b == len(u) - 1:
            d, A = 1, Z[b]
        else:
            d = Ui[b + 1] - Ui[b]
            assert d > 0
            A = Z[b] * d + (Xi[m] - Ui[b]) * (Z[b + 1] - Z[b])
        g = groups.setdefault(d, [0, 0, 0, 0])
        g[0] += A
        g[1] += A * A
        g[2] += W[i] * A
        g[3] += abs(W[i] * A)
        sw += W[i]
        sww += W[i] * W[i]
    Sw, Sww = sw * uw, sww * uw * uw
    Sv = Fraction(*over_common_denominator(groups, 0, 1)) * uz
    Svv = Fraction(*over_common_denominator(groups, 1, 2)) * uz * uz
    Swv = Fraction(*over_common_denominator(groups, 2, 1)) * uw * uz
    Sabs = Fraction(*over_common_denominator(groups, 3, 1)) * uw * uz
    C, Va, Vb = Swv - Sw * Sv / n, Sww - Sw * Sw / n, Svv - Sv * Sv / n
    if not (Va > 0 and Vb > 0):
        return n, None
    return n, (C, Va, Vb, Sabs + abs(Sw) * abs(Sv) / n, Sww + Sw * Sw / n, Svv + Sv * Sv / n)


def big(fr):
    return mpmath.mpf(fr.numerator) / mpmath.mpf(fr.denominator)


def finish(parts):
    """-> (r, r_lo, S) of a half; NaN for a half without a value"""
    if parts is None:
        return np.nan, np.nan, np.nan
    C, Va, Vb, Cabs, Vaabs, Vbabs = (big(f) for f in parts)
    root = mpmath.sqrt(Va * Vb)
    r = C / root
    hi = float(r)
    scale = Cabs / root + abs(r) * (Vaabs / Va + Vbabs / Vb) / 2
    return hi, float(r - mpmath.mpf(hi)), float(scale)


def main():
    ls = np.load(os.path.join(ROOT, "tests", "golden", "lomb_scargle_golden.npz"))
    out = {"cases": np.array(inp.CASES), "lag_sets": np.array(inp.LAG_SETS)}
    worst_s = worst_rho = 0.0
    for name in inp.CASES:
        t, y = (np.asarray(ls["%s/%s" % (name, k)], dtype=np.float64) for k in ("t", "y"))
        t2, y2 = inp.companion(name, t, y)
        assert len(t2) == inp.COMPANION_M[name] and np.all(np.diff(t) >= 0) and np.all(np.diff(t2) >= 0)
        out[name + "/t2"], out[name + "/y2"] = t2, y2
        R, ur = residuals(y)
        Sm, us = residuals(y2)
        for tag, lags in inp.lag_sets(t, t2).items():
            key = "%s/%s/" % (name, tag)
            assert 1 <= len(lags) <= 65536 and np.all(np.isfinite(lags))
            helper = inp.iccf(t, y, t2, y2, lags)
            cols = {q: [] for q in ("r_a", "r_a_lo", "s_a", "n_a", "r_b", "r_b_lo", "s_b", "n_b")}
            for tau in lags:
                na, pa = exact_half(t, R, ur, tau, t2, Sm, us)
                nb, pb = exact_half(t2, Sm, us, -tau, t, R, ur)
                for h, n, parts in (("a", na, pa), ("b", nb, pb)):
                    r, lo, scale = finish(parts)
                    cols["r_" + h].append(r); cols["r_%s_lo" % h].append(lo); cols["s_" + h].append(scale); cols["n_" + h].append(n)
            out[key + "lags"] = lags
            for q, v in cols.items():
                out[key + q] = np.array(v, dtype=np.int64 if q[0] == "n" else np.float64)
            for h in "ab":
                r, lo, n, s = (out[key + q] for q in ("r_" + h, "r_%s_lo" % h, "n_" + h, "s_" + h))
                assert np.array_equal(n, helper["n_" + h]) and np.array_equal(np.isnan(r), np.isnan(helper["r_" + h]))
                rho = np.where(np.isnan(r), 0.0, np.abs((helper["r_" + h] - r) - lo))
                out[key + "rho_" + h] = rho
                fin = np.isfinite(r)
                if fin.any():
                    # the condition of the bound: S must not make it vacuous
                    assert np.sum(s[fin] <= 100.0) * 2 >= fin.sum(), (name, tag, h, np.sort(s[fin]))
                    assert np.all(np.abs(r[fin]) <= 1.0 + 1e-12)
                    worst_s, worst_rho = max(worst_s, float(s[fin].max())), max(worst_rho, float(rho.max()))
            if tag == "beyond":
                n_all = np.concatenate([out[key + "n_a"], out[key + "n_b"]])
                assert np.any(n_all == 0) and np.any(n_all == 1) and np.any(np.isnan(out[key + "r_a"])) and np.any(np.isfinite(out[key + "r_a"]))
            if tag == "ties":
                ties = inp.tie_pairs(t, t2, lags)
                assert {0, len(t2) - 1} <= set(ties[:, 2].tolist()) and len(set(ties[:, 0].tolist())) == len(lags)
                out[key + "tie_pairs"] = ties
            fin = np.isfinite(out[key + "r_a"])
            print("%-5s %-9s %3d lags, finite r_a %3d r_b %3d, n_a %d .. %d, largest S %.1f, rho %.1e" % (
                name, tag, len(lags), fin.sum(), np.isfinite(out[key + "r_b"]).sum(), out[key + "n_a"].min(), out[key + "n_a"].max(),
                np.nanmax(np.concatenate([out[key + "s_a"], out[key + "s_b"], [0.0]])), max(out[key + "rho_a"].max(), out[key + "rho_b"].max())))
    out["largest_scale"], out["largest_rho"] = np.float64(worst_s), np.float64(worst_rho)
    path = os.path.join(ROOT, "tests", "golden", "iccf_golden.npz")
    np.savez_compressed(path, **out)
    print("largest S %.3g, largest rho %.3g; %s: %d bytes" % (worst_s, worst_rho, path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
