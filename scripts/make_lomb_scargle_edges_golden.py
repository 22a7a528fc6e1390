#!/usr/bin/env python3
"""Writes tests/golden/lomb_scargle_edges_golden.npz: inputs and 50-digit truths for the shapes at which the launcher of
mtg_lomb_scargle takes another path (tests/test_lomb_scargle_edges_cpu.py, tests/test_lomb_scargle_edges_gpu.py).

The light curves, the truth (mpmath on astropy's tau form at the absolute times) and rho (plain numpy float64 on the
tau-free formula, tests/lomb_scargle_numpy.py) are those of scripts/make_lomb_scargle_golden.py, imported from it; that
script and its fixture are not touched, this one has a random stream of its own.  Per case and weighting (w: dy^-2,
u: 1 / N) the file holds the four normalisations, rho, det_min and psd_factor as the first fixture does.

  edge255 .. edge513   N at, one below, one above and two chunks of the kernel's 256-sample staging; L = 1, F = 16,
                       frequencies linspace(1 / T, N / T, 16).
  n4                   the smallest N the entry accepts, frequencies (0.4, 0.7, 1.0, 1.3) / T.
  perlc3               L = 3, N = 61, every light curve drawn separately by lightcurve(): times and first epoch differ
                       per row; one list of F = 40 frequencies, linspace(1 / Tmin, N / Tmin, 40).  t, y, dy are [3][61],
                       truths [3][40], rho / det_min / psd_factor [3].  `{w,u}_standard_row0_times` is the 50-digit
                       power of every row's (y, dy) on ROW 0's times: what a kernel that read the wrong row's sampling
                       would give (tests/test_lomb_scargle_edges_cpu.py shows it is far from the truth).
  tile4                shared sampling, N = 257, four light curves: the lightcurve() signal plus independent noise, the
                       error bars of row j those of row 0 times (1, 0.5, 2, 1.25)[j]; F = 24; truth for every row.
  slab17 (not in `cases`)  y, dy [17][4] on n4's times, for a call with F = 2^21 frequencies linspace over n4's range
                       (two slabs of light curves); for row 16 the truth, rho and det_min at the 64 frequencies
                       `index` of that list -- n4's figures, 0.03 / 0.02, apply.  The other rows have no truth.

Two conditions keep the tests from hiding a failure and are asserted here on every (row, weighting): CC SS - CS^2 >=
0.05 in mpmath, and rho <= 1e-9.  A light curve is drawn again until its float64 determinant is at least 0.075.  n4 alone
has other figures: four points cannot reach 0.05 (three parameters are fitted), so it is drawn again until the float64
determinant is at least 0.03, and 0.02 is asserted on the mpmath value; rho <= 1e-9 stays.

Run on the CPU:  python3 scripts/make_lomb_scargle_edges_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lomb_scargle_numpy  # noqa: E402
from make_lomb_scargle_golden import det_min_float64, lightcurve, truth  # noqa: E402

SEED = 11
DET_MIN, RHO_MAX = 0.05, 1e-9
N4_DET_DRAW, N4_DET_MIN = 0.03, 0.02
EDGES = (255, 256, 257, 512, 513)
TILE4_FACTORS = (1.0, 0.5, 2.0, 1.25)
SLAB_F = 1 << 21
NORMS = lomb_scargle_numpy.NORMALIZATIONS


def dets(t, dy, freqs):
    return min(det_min_float64(t, dy, freqs), det_min_float64(t, None, freqs))


def evaluate(name, t, y, dy, freqs, det_floor):
    """truths of one light curve, conditions asserted -> {"w_standard": [F], ..., "w_rho": float, ...}"""
    out = {}
    for tag, err in (("w", dy), ("u", None)):
        tr, det_min, YY, sw = truth(t, y, err, freqs)
        rho = float(np.max(np.abs(lomb_scargle_numpy.power(t, y, err, freqs) - tr["standard"])))
        assert det_min >= det_floor and rho <= RHO_MAX, (name, tag, det_min, rho)
        print("%-10s %s  n %4d  F %3d  min det %.3f  rho %.3g  max standard %.4f" %
              (name, tag, len(t), len(freqs), det_min, rho, tr["standard"].max()))
        for k in NORMS:
            out["%s_%s" % (tag, k)] = tr[k]
        out["%s_rho" % tag], out["%s_psd_factor" % tag], out["%s_det_min" % tag] = rho, 0.5 * sw * YY, det_min
    return out


def put(store, name, t, y, dy, freqs, rows):
    """rows: one evaluate() dict (L = 1) or a list of them (stacked along a leading axis)"""
    many = isinstance(rows, list)
    for k in (rows[0] if many else rows):
        store["%s/%s" % (name, k)] = np.array([r[k] for r in rows]) if many else np.asarray(rows[k], dtype=np.float64)
    for k, v in (("t", t), ("y", y), ("dy", dy), ("freqs", freqs)):
        store["%s/%s" % (name, k)] = v


def main():
    rng = np.random.default_rng(SEED)
    store, cases = {}, []

    for n in EDGES + (4,):
        name = "edge%d" % n if n > 4 else "n4"
        draw, floor = (1.5 * DET_MIN, DET_MIN) if n > 4 else (N4_DET_DRAW, N4_DET_MIN)
        for attempt in range(10000):
            t, y, dy = lightcurve(rng, n)
            T = t[-1] - t[0]
            freqs = np.linspace(1.0 / T, n / T, 16) if n > 4 else np.array([0.4, 0.7, 1.0, 1.3]) / T
            if dets(t, dy, freqs) >= draw:
                break
        print("%s: draw %d" % (name, attempt + 1))
        put(store, name, t, y, dy, freqs, evaluate(name, t, y, dy, freqs, floor))
        cases.append(name)

    # every light curve on its own times
    n = 61
    for attempt in range(10000):
        lcs = [lightcurve(rng, n) for _ in range(3)]
        Tmin = min(t[-1] - t[0] for t, _, _ in lcs)
        freqs = np.linspace(1.0 / Tmin, n / Tmin, 40)
        if min(dets(t, dy, freqs) for t, _, dy in lcs) >= 1.5 * DET_MIN:
            break
    print("perlc3: draw %d" % (attempt + 1))
    rows = [evaluate("perlc3[%d]" % m, t, y, dy, freqs, DET_MIN) for m, (t, y, dy) in enumerate(lcs)]
    put(store, "perlc3", *(np.stack([lc[i] for lc in lcs]) for i in range(3)), freqs, rows)
    t0 = lcs[0][0]
    for tag in "wu":
        store["perlc3/%s_standard_row0_times" % tag] = np.stack(
            [truth(t0, y, dy if tag == "w" else None, freqs)[0]["standard"] for _, y, dy in lcs])
    cases.append("perlc3")

    # four light curves on shared sampling
    n = 257
    for attempt in range(10000):
        t, y, dy = lightcurve(rng, n)
        T = t[-1] - t[0]
        freqs = np.linspace(1.0 / T, n / T, 24)
        if dets(t, dy, freqs) >= 1.5 * DET_MIN:
            break
    print("tile4: draw %d" % (attempt + 1))
    signal = 3.0 + 0.8 * np.sin(2.0 * np.pi * ((0.31 * n) / T) * t + 0.7)      # lightcurve()'s
    DY = np.stack([dy * s for s in TILE4_FACTORS])
    Y = np.stack([y] + [signal + DY[m] * rng.standard_normal(n) for m in range(1, 4)])
    rows = [evaluate("tile4[%d]" % m, t, Y[m], DY[m], freqs, DET_MIN) for m in range(4)]
    put(store, "tile4", t, Y, DY, freqs, rows)
    cases.append("tile4")

    # 17 light curves on n4's times for the slab test: the data of every row, and for the last one the truth at 64 of the
    # 2^21 frequencies (not a case of the list: no truth for the other rows, whose frequencies may be degenerate)
    t, f4 = store["n4/t"], store["n4/freqs"]
    index = np.linspace(0, SLAB_F - 1, 64).astype(np.int64)
    freqs = np.linspace(f4[0], f4[-1], SLAB_F)[index]
    for attempt in range(10000):
        Y = 3.0 + 0.5 * rng.standard_normal((17, 4))
        DY = rng.uniform(0.05, 0.3, size=(17, 4))
        if dets(t, DY[16], freqs) >= N4_DET_DRAW:
            break
    print("slab17: draw %d" % (attempt + 1))
    for k, v in evaluate("slab17[16]", t, Y[16], DY[16], freqs, N4_DET_MIN).items():
        if k[2:] in ("standard", "rho", "det_min"):
            store["slab17/%s" % k] = np.asarray(v, dtype=np.float64)
    store["slab17/y"], store["slab17/dy"], store["slab17/index"], store["slab17/F"] = Y, DY, index, np.int64(SLAB_F)

    store["cases"] = np.array(cases)
    path = os.path.join(ROOT, "tests", "golden", "lomb_scargle_edges_golden.npz")
    np.savez_compressed(path, **store)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
