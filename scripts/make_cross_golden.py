"""Writes tests/golden/cross_golden.npz: exact (rational) truths of the eight sums of mtg_cross_sums for the resident
series of the Lomb-Scargle fixture's cases n5, n52, n216 and n789, each against the companion of tests/cross_numpy.py
(M = 7, 61, 300, 523 on a shifted span), for the six edge sets there.  The method is scripts/make_lag_golden.py's.

Every stored number is a double, so every term of every sum is a rational number: the times and data are scaled to
integers by a power of two, the means are sum y / N and sum y2 / M exactly, and the sums are Python integers -- no rounding
until the result is written, as the nearest double `x` and the double `x_lo` nearest to what is left.  The lag of a pair is
by definition the ROUNDED difference fl(t2_j - t_i) and its bin comes from double comparisons: both are taken in float64.

Per case: <case>/t2, <case>/y2.  Per case and edge set: <case>/<set>/edges, the sums with their _lo parts, the sums of the
terms' magnitudes lagabs, cfabs, saabs, sbabs (the scales of the bounds of lag, cf, sa, sb; the other sums have
non-negative terms), rho_<sum> = the largest error of tests/cross_numpy.py over the bins relative to that scale, and for
"ties" the pairs that sit exactly on an edge as rows (i, j, bin; -1: on the last edge, in no bin).

    python scripts/make_cross_golden.py        (a few seconds on one core)
"""
import os
import sys
from fractions import Fraction

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cross_numpy as cn  # noqa: E402


def scaled(values):
    """doubles -> (Python integers m, k) with value = m / 2^k exactly"""
    fr = [Fraction(float(v)) for v in values]
    k = max(f.denominator.bit_length() - 1 for f in fr)
    return np.array([f.numerator * ((1 << k) // f.denominator) for f in fr], dtype=object), k


def split(fr):
    """a rational -> the nearest double and the double nearest to the rest"""
    hi = float(fr)
    return hi, float(fr - Fraction(hi))


def main():
    ls = np.load(os.path.join(ROOT, "tests", "golden", "lomb_scargle_golden.npz"))
    out = {"cases": np.array(cn.CASES), "edge_sets": np.array(cn.EDGE_SETS)}
    for name in cn.CASES:
        t, y = (np.asarray(ls["%s/%s" % (name, k)], dtype=np.float64) for k in ("t", "y"))
        t2, y2 = cn.companion(name, t, y)
        n, m = len(t), len(t2)
        assert m == cn.COMPANION_M[name] and n * m <= 420000 and np.all(np.diff(t) >= 0) and np.all(np.diff(t2) >= 0)
        out[name + "/t2"], out[name + "/y2"] = t2, y2
        i, j, tau = cn.pairs(t, t2)
        assert np.any(tau == 0) and np.any(tau < 0) and np.any(tau > 0)
        ym, ky = scaled(y)
        zm, kz = scaled(y2)
        tm, kt = scaled(tau)
        rm = n * ym - sum(ym)             # r = rm / (n 2^ky)
        sm = m * zm - sum(zm)             # s = sm / (m 2^kz)
        ur, us = Fraction(1, n << ky), Fraction(1, m << kz)
        p = rm[i] * sm[j]
        terms = {"lag": (tm, Fraction(1, 1 << kt)), "cf": (p, ur * us), "cf2": (p * p, (ur * us) ** 2),
                 "sa": (rm[i], ur), "sb": (sm[j], us), "saa": (rm[i] ** 2, ur ** 2), "sbb": (sm[j] ** 2, us ** 2),
                 "lagabs": (abs(tm), Fraction(1, 1 << kt)), "cfabs": (abs(p), ur * us), "saabs": (abs(rm[i]), ur), "sbabs": (abs(sm[j]), us)}
        for tag, edges in cn.edge_sets(t, t2).items():
            key = "%s/%s/" % (name, tag)
            nb = len(edges) - 1
            assert 1 <= nb <= 128 and np.all(np.diff(edges) > 0) and np.all(np.isfinite(edges))
            b = cn.bin_index(tau, edges)
            members = [np.flatnonzero(b == q) for q in range(nb)]
            helper = cn.cross_sums(t, y, t2, y2, edges)
            count = np.array([len(k) for k in members], dtype=np.int64)
            assert np.array_equal(count, helper["count"])
            out[key + "edges"] = edges
            out[key + "count"] = count
            exact = {}
            for q, (ints, unit) in terms.items():
                exact[q] = [Fraction(sum(ints[k].tolist())) * unit for k in members]
                parts = np.array([split(f) for f in exact[q]])
                out[key + q], out[key + q + "_lo"] = parts[:, 0], parts[:, 1]
            for q in cn.VALUES:
                scale = exact[cn.SCALE[q]]
                out[key + "rho_" + q] = max([float(abs(Fraction(float(helper[q][k])) - exact[q][k]) / scale[k])
                                             for k in range(nb) if scale[k] > 0] + [0.0])
            if tag == "ties":
                on = np.flatnonzero(np.isin(tau, edges))
                assert len(on) >= nb + 1 and 0.0 in edges
                out[key + "tie_pairs"] = np.stack([i[on], j[on], b[on]], axis=1).astype(np.int64)
                # a pair on edge k belongs to bin k, the upper one
                assert all(b[k] == (np.flatnonzero(edges == tau[k])[0] if tau[k] < edges[-1] else -1) for k in on)
            print("%-5s %-9s %3d bins, %6d pairs binned, %3d empty, skipped (late, early, of) %s, rho %s" % (
                name, tag, nb, int(count.sum()), int(np.sum(count == 0)), cn.skipped_chunks(t, t2, edges),
                " ".join("%s %.1e" % (q, out[key + "rho_" + q]) for q in cn.VALUES)))
    path = os.path.join(ROOT, "tests", "golden", "cross_golden.npz")
    np.savez_compressed(path, **out)
    print("%s: %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
