#!/usr/bin/env python3
"""What harmonics cost: mtg_lomb_scargle_multi for K = 1, 2, 3, 5 at 2000 light curves x N = 1e4 shared samples x 5000
frequencies (profiles/lomb_scargle_multi_probe.txt), weighted and unweighted.

Per (K, weighting): the kernel time (mtg_last_kernel_ms: pre-pass, powers, peaks) and the whole call (host wall clock
around Engine.lomb_scargle with power=True, peak=True: upload of the frequencies, kernels, the 80 MB copy of the powers),
each the median of 5 calls after 2 warm-ups with the smallest and the largest of the five beside it, and each median
against K = 1 of the same build.  Beside them the operation count
the expectation rests on, in FP64 VALU instructions per (sample, frequency) of a tile of R light curves:
  ~31 for the base (cos, sin) pair, 6 per further harmonic (m = 2 .. 2 K: one complex multiplication),
  4 K per set of trigonometric sums (R sets weighted, one unweighted), 4 K per light curve for the data sums
(K = 1: the one-term kernel's 31, and 7 per light curve weighted / 5 per tile + 2 per light curve unweighted).

Run on a GPU:  python3 scripts/lomb_scargle_multi_probe.py
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mind_the_gaps_amd.engine import Engine  # noqa: E402

ISSUE_RATE = 256 * 4 * 64 / 4 * 2.4e9     # wave-wide FP64 VALU instructions per second, in lanes
SINCOS_OPS = 31


def measure(eng, freqs, weighted, nterms):
    ms, wall = [], []
    for _ in range(7):
        t0 = time.perf_counter()
        eng.lomb_scargle(freqs, weighted=weighted, power=True, peak=True, nterms=nterms)
        wall.append((time.perf_counter() - t0) * 1e3)
        ms.append(eng.last_kernel_ms)
    return np.array(ms[2:]), np.array(wall[2:]), eng.last_solver


def floor_ms(L, N, F, R, K, weighted):
    """the operation count above at the FP64 issue rate"""
    tiles = -(-L // R)
    if K == 1:
        per_tile = SINCOS_OPS + (7 * R if weighted else 5 + 2 * R)
    else:
        per_tile = SINCOS_OPS + 6 * (2 * K - 1) + 4 * K * (R if weighted else 1) + 4 * K * R
    return per_tile * tiles * N * F / ISSUE_RATE * 1e3


def main():
    rng = np.random.default_rng(1)
    L, N, F = 2000, 10_000, 5000
    eng = Engine(0)
    t = np.sort(rng.uniform(0.0, 1000.0, size=N)) + 58000.0
    y = rng.standard_normal((L, N))
    dy = rng.uniform(0.05, 0.3, size=(L, N))
    eng.set_lightcurves(t, y, dy)
    T = t[-1] - t[0]
    freqs = np.linspace(1.0 / T, 0.5 * N / T, F)
    print("L %d N %d F %d, shared sampling; power=True, peak=True" % (L, N, F))
    print("%-9s %2s %10s %17s %8s %10s %17s %8s %10s  %s" % ("weights", "K", "kernel ms", "min - max", "x K=1", "call ms", "min - max",
                                                            "x K=1", "count ms", "kernel"))
    for weighted in (True, False):
        base = None
        for K in (1, 2, 3, 5):
            kms, walls, solver = measure(eng, freqs, weighted, K)
            ms, wall = float(np.median(kms)), float(np.median(walls))
            R = int(solver.rstrip(">").replace("<", ",").split(",")[-1])
            base = base or (ms, wall)
            print("%-9s %2d %10.2f %17s %8.2f %10.2f %17s %8.2f %10.2f  %s" %
                  ("weighted" if weighted else "1/N", K, ms, "%.2f - %.2f" % (kms.min(), kms.max()), ms / base[0], wall,
                   "%.2f - %.2f" % (walls.min(), walls.max()), wall / base[1], floor_ms(L, N, F, R, K, weighted), solver), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
