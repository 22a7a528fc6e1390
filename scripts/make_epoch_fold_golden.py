#!/usr/bin/env python3
"""Writes tests/golden/epoch_fold_golden.npz: the epoch-folding statistic of mtg_epoch_fold (include/mtg.h) with the bins
from exact rational arithmetic on the stored doubles and the sums in 50-digit mpmath.  CPU only (mpmath, numpy).

Inputs: the five cases of tests/golden/lomb_scargle_golden.npz (read, not copied: a case stores `freq_index` into that
file's frequencies, at most MAXF of them evenly spaced), time_0 = t[0], nbins in NBINS.  Per (case, nbins):
    nb<k>/count [F][k]            the exact counts
    nb<k>/{w,u}_<normalization>   the truths, weighted and unweighted
and per case {w,u}_rho, the largest error of tests/epoch_fold_numpy.py on the standard power, and near_edges [.][3]:
every (frequency index, sample, nbins) with non-zero phase within 2^-40 of a bin edge.

Case `edges` (its own t, y, dy, freqs; time_0 = 0, so te = t exactly) is built for the bin rule, nbins in EDGE_NBINS;
kind_<x> [.][2] lists the (frequency index, sample) pairs of each kind, each property asserted with Fraction:
    a  f te exactly a multiple of 1/32 (the same pairs are multiples of 1/8 and 1/2 where the numerator allows)
    b  fl(f te) exactly a multiple of 1/32 with the exact product just below it: the rounded product picks the wrong bin
    c  the same just above
    e  as b and c at ~ 1e6 cycles
    b10, c10  tenths are no doubles: the exact product below k / 10 with the rounded one at or above it, and the reverse
Case `edges_neg` is the same light curve with time_0 inside the span (kind d: negative te)."""
import os
import sys
from fractions import Fraction

import mpmath
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import epoch_fold_numpy as efn  # noqa: E402

mpmath.mp.dps = 50
CASES = ("n5", "n52", "n216", "n789", "fast216")
NBINS = (2, 10, 32)
EDGE_NBINS = (2, 8, 10, 32)
MAXF = 48


def truth(y, dy, weighted, bins_of, nbins_list):
    """{nbins: {normalization: [F]}} from exact bins [F][N] (as Fractions' floor) in 50 digits"""
    ym = [mpmath.mpf(float(v)) for v in y]
    if weighted:
        iv = [1 / mpmath.mpf(float(v)) ** 2 for v in dy]
        sw = mpmath.fsum(iv)
        w = [v / sw for v in iv]
    else:
        sw = mpmath.mpf(len(y))
        w = [1 / sw] * len(y)
    ybar = mpmath.fsum(a * b for a, b in zip(w, ym))
    r = [v - ybar for v in ym]
    YY = mpmath.fsum(a * b * b for a, b in zip(w, r))
    out = {}
    for nb in nbins_list:
        rows = {k: [] for k in efn.NORMALIZATIONS}
        for b in bins_of[nb]:
            W = [mpmath.mpf(0)] * nb
            S = [mpmath.mpf(0)] * nb
            for n, bn in enumerate(b):
                W[bn] += w[n]
                S[bn] += w[n] * r[n]
            p = mpmath.fsum(S[i] ** 2 / W[i] for i in range(nb) if W[i] > 0)
            rows["standard"].append(float(p / YY))
            rows["model"].append(float(p / (YY - p)))
            rows["log"].append(float(-mpmath.log(1 - p / YY)))
            rows["psd"].append(float(p * sw / 2))
        out[nb] = {k: np.array(v) for k, v in rows.items()}
    return out


def one_case(out, name, t, y, dy, freqs, time_0, nbins_list, edge_case):
    te = t - time_0
    phases = [[efn.exact_phase(f, x) for x in te] for f in freqs]
    bins_of = {nb: np.array([[int(ph * nb) for ph in row] for row in phases], dtype=np.int64) for nb in nbins_list}
    near = []
    for nb in nbins_list:
        for k, f in enumerate(freqs):
            assert np.array_equal(efn.bins(f, te, nb), bins_of[nb][k]), (name, nb, k)
            for n, ph in enumerate(phases[k]):
                x = ph * nb
                d = abs(x - round(x))
                if ph != 0 and d < Fraction(1, 2 ** 40):
                    near.append((k, n, nb))
                elif not edge_case:
                    assert ph == 0 or d >= Fraction(1, 10 ** 9), (name, nb, k, n, float(d))
        out["%s/nb%d/count" % (name, nb)] = np.array([np.bincount(b, minlength=nb) for b in bins_of[nb]], dtype=np.int64)
    out["%s/near_edges" % name] = np.array(near, dtype=np.int64).reshape(-1, 3)
    for tag, weighted in (("w", True), ("u", False)):
        tr = truth(y, dy, weighted, bins_of, nbins_list)
        rho = 0.0
        for nb in nbins_list:
            for k in efn.NORMALIZATIONS:
                out["%s/nb%d/%s_%s" % (name, nb, tag, k)] = tr[nb][k]
            rho = max(rho, float(np.max(np.abs(efn.power(t, y, dy, freqs, nb, time_0, weighted) - tr[nb]["standard"]))))
        assert rho <= 1e-9, (name, tag, rho)
        out["%s/%s_rho" % (name, tag)] = np.float64(rho)
    out["%s/time_0" % name] = np.float64(time_0)
    print("%-10s N %4d F %3d  near edges %3d  rho w %.2e u %.2e" % (name, len(t), len(freqs), len(near), out[name + "/w_rho"],
                                                                   out[name + "/u_rho"]))


def build_edges(rng):
    """times (ascending, te = t), frequencies and the lists of special pairs"""
    want = 36
    pairs = {"a": [], "b": [], "c": [], "e": []}   # (f, te)
    grid_t = np.sort(rng.choice(np.arange(1, 400), size=24, replace=False)) / 8.0
    grid_f = np.sort(rng.choice(np.arange(1, 60), size=6, replace=False)) / 4.0
    for f in grid_f:
        for x in grid_t:
            pairs["a"].append((f, x))
    while min(len(pairs[k]) for k in "bce") < want:
        big = len(pairs["b"]) >= want and len(pairs["c"]) >= want
        edge = (1000000.0 if big else 0.0) + float(rng.integers(1, 32 * 40)) / 32.0
        x = float(rng.uniform(1.0, 50.0))
        f = edge / x
        if f * x != edge:
            continue
        exact = Fraction(f) * Fraction(x)
        if exact == Fraction(edge):
            continue
        kind = "e" if big else ("b" if exact < Fraction(edge) else "c")
        if len(pairs[kind]) < want:
            pairs[kind].append((f, x))
    # tenths are no doubles: the exact and the rounded product on opposite sides of k / 10 (below: exact below the edge)
    pairs["b10"], pairs["c10"] = [], []
    while min(len(pairs["b10"]), len(pairs["c10"])) < want:
        edge = Fraction(int(rng.integers(1, 400)), 10)
        if edge.denominator in (1, 2):
            continue
        x = float(rng.uniform(1.0, 50.0))
        f = float(edge) / x
        rounded, exact = Fraction(f * x), Fraction(f) * Fraction(x)
        kind = "b10" if exact < edge <= rounded else "c10" if rounded < edge <= exact else None
        if kind and len(pairs[kind]) < want:
            pairs[kind].append((f, x))   # (floor(10 frac) of the rounded product is in the bin on the rounded side of the edge)
    t = np.unique(np.array([x for v in pairs.values() for _, x in v]))
    freqs = np.unique(np.array([f for v in pairs.values() for f, _ in v]))
    kinds = {k: np.array([(int(np.searchsorted(freqs, f)), int(np.searchsorted(t, x))) for f, x in v], dtype=np.int64)
             for k, v in pairs.items()}
    for k, n in kinds["a"]:
        assert (Fraction(freqs[k]) * Fraction(t[n]) * 32).denominator == 1
    for kind in "bce":
        for k, n in kinds[kind]:
            rounded, exact = Fraction(freqs[k] * t[n]), Fraction(freqs[k]) * Fraction(t[n])
            assert (rounded * 32).denominator == 1 and exact != rounded
            assert (exact < rounded) == (kind == "b") or kind == "e"
            wrong = [nb for nb in EDGE_NBINS if (rounded * nb).denominator == 1 and exact < rounded]
            for nb in wrong:   # the rounded product sits on the edge, the exact one in the bin below
                assert efn.rounded_bins(freqs[k], t[n:n + 1], nb)[0] != efn.exact_bins(freqs[k], t[n:n + 1], nb)[0]
    assert any(freqs[k] * t[n] > 9e5 for k, n in kinds["e"])
    return t, freqs, kinds


def main():
    src = np.load(os.path.join(ROOT, "tests", "golden", "lomb_scargle_golden.npz"))
    out = {}
    empties = set()
    for name in CASES:
        t, y, dy, freqs = (src["%s/%s" % (name, k)] for k in ("t", "y", "dy", "freqs"))
        index = np.unique(np.round(np.linspace(0, len(freqs) - 1, min(MAXF, len(freqs)))).astype(np.int64))
        out[name + "/freq_index"] = index
        one_case(out, name, t, y, dy, freqs[index], float(t[0]), NBINS, False)
        for nb in NBINS:
            empties.add(bool(np.any(out["%s/nb%d/count" % (name, nb)] == 0)))
    assert empties == {True, False}, "need a (case, nbins) with empty bins and one without"
    assert np.any(out["n5/nb32/count"] == 0)
    rng = np.random.default_rng(20240607)
    t, freqs, kinds = build_edges(rng)
    y = rng.normal(10.0, 2.0, len(t))
    dy = rng.uniform(0.5, 1.5, len(t))
    for name, time_0 in (("edges", 0.0), ("edges_neg", float(t[len(t) // 2]))):
        for k, v in (("t", t), ("y", y), ("dy", dy), ("freqs", freqs)):
            out["%s/%s" % (name, k)] = v
        one_case(out, name, t, y, dy, freqs, time_0, EDGE_NBINS, True)
    assert np.any(t - out["edges_neg/time_0"] < 0)
    for k, v in kinds.items():
        out["edges/kind_" + k] = v
    path = os.path.join(ROOT, "tests", "golden", "epoch_fold_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote %s, %d bytes" % (path, os.path.getsize(path)))
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
