"""Writes tests/golden/lag_golden.npz: exact (rational) truths of the six sums of mtg_lag_sums on the sampling and data of
the Lomb-Scargle fixture's cases n5, n52, n216 and n789, for the six edge sets of tests/lag_numpy.py.

Every stored number is a double, so every term of every sum is a rational number: the times, data and variances are
scaled to integers by a power of two, the mean is sum y / N exactly, and the sums are Python integers -- no rounding until
the result is written, as the nearest double `x` and the double `x_lo` nearest to what is left.  The lag of a pair is by
definition the ROUNDED difference fl(t_j - t_i) and its bin comes from double comparisons: both are taken in float64.

Per case and edge set: <case>/<set>/edges, the sums with their _lo parts, cfabs = sum |r_i r_j| (the scale of cf's
bound), rho_<sum> = the largest error of tests/lag_numpy.py over the bins relative to the sum of the terms' magnitudes,
and for "ties" the pairs that sit exactly on an edge as rows (i, j, bin; -1: on the last edge, in no bin).

    python scripts/make_lag_golden.py        (about a minute on one core)
"""
import os
import sys
from fractions import Fraction

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lag_numpy as ln  # noqa: E402


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
    out = {"cases": np.array(ln.CASES), "edge_sets": np.array(ln.EDGE_SETS)}
    for name in ln.CASES:
        t, y, dy = (np.asarray(ls["%s/%s" % (name, k)], dtype=np.float64) for k in ("t", "y", "dy"))
        n = len(t)
        assert n * (n - 1) // 2 <= 320000 and np.all(np.diff(t) >= 0)
        i, j, tau = ln.pairs(t)
        ym, ky = scaled(y)
        vm, kv = scaled(dy * dy)          # sigma^2 as the engine stores it: the rounded square
        tm, kt = scaled(tau)
        rm = n * ym - sum(ym)             # r = rm / (n 2^ky)
        d2 = (ym[j] - ym[i]) ** 2         # / 2^(2 ky)
        p = rm[i] * rm[j]                 # / (n 2^ky)^2
        terms = {"lag": (tm, Fraction(1, 1 << kt)), "sf": (d2, Fraction(1, 1 << (2 * ky))), "cf": (p, Fraction(1, (n << ky) ** 2)),
                 "cf2": (p * p, Fraction(1, (n << ky) ** 4)), "noise": (vm[i] + vm[j], Fraction(1, 1 << kv)),
                 "cfabs": (abs(p), Fraction(1, (n << ky) ** 2))}
        for tag, edges in ln.edge_sets(t).items():
            key = "%s/%s/" % (name, tag)
            nb = len(edges) - 1
            assert 1 <= nb <= 128 and edges[0] >= 0 and np.all(np.diff(edges) > 0) and np.all(np.isfinite(edges))
            b = ln.bin_index(tau, edges)
            members = [np.flatnonzero(b == q) for q in range(nb)]
            helper = ln.lag_sums(t, y, dy, edges)
            count = np.array([len(m) for m in members], dtype=np.int64)
            assert np.array_equal(count, helper["count"])
            out[key + "edges"] = edges
            out[key + "count"] = count
            exact = {}
            for q, (ints, unit) in terms.items():
                exact[q] = [Fraction(sum(ints[m].tolist())) * unit for m in members]
                parts = np.array([split(f) for f in exact[q]])
                out[key + q], out[key + q + "_lo"] = parts[:, 0], parts[:, 1]
            for q in ("lag", "sf", "cf", "cf2", "noise"):
                scale = exact["cfabs" if q == "cf" else q]
                out[key + "rho_" + q] = max([float(abs(Fraction(float(helper[q][k])) - exact[q][k]) / scale[k])
                                             for k in range(nb) if scale[k] > 0] + [0.0])
            if tag == "ties":
                on = np.flatnonzero(np.isin(tau, edges))
                assert len(on) >= nb + 1
                out[key + "tie_pairs"] = np.stack([i[on], j[on], b[on]], axis=1).astype(np.int64)
                # a pair on edge k belongs to bin k, the upper one
                assert all(b[k] == (np.flatnonzero(edges == tau[k])[0] if tau[k] < edges[-1] else -1) for k in on)
            print("%-5s %-8s %3d bins, %6d pairs binned, %3d empty, rho %s" % (
                name, tag, nb, int(count.sum()), int(np.sum(count == 0)),
                " ".join("%s %.1e" % (q, out[key + "rho_" + q]) for q in ("lag", "sf", "cf", "cf2", "noise"))))
    path = os.path.join(ROOT, "tests", "golden", "lag_golden.npz")
    np.savez_compressed(path, **out)
    print("%s: %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
