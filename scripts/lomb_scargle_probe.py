#!/usr/bin/env python3
"""Kernel time of mtg_lomb_scargle (mtg_last_kernel_ms: pre-pass, powers, peaks; median of 5 calls after 2 warm-ups) at
the shapes of profiles/lomb_scargle_probe.txt, beside the floors the work implies:

* FMA floor: 2 (unweighted) or 7 (weighted: w c, C, S, CC, CS, YC, YS) FP64 operations per (light curve, sample,
  frequency) at the 39.3e12 FP64 FMA/s of the vector pipe (256 CUs x 4 SIMDs x 64 lanes / 4 cycles x 2.4 GHz);
* sine/cosine floor: one pair per (tile, sample, frequency), ~31 VALU instructions each (exact product, reduction,
  table rotation, the two short polynomials) at the same issue rate.

Run on a GPU:  python3 scripts/lomb_scargle_probe.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mind_the_gaps_amd.engine import Engine  # noqa: E402

ISSUE_RATE = 256 * 4 * 64 / 4 * 2.4e9     # wave-wide FP64 VALU instructions per second, in lanes
SINCOS_OPS = 31


def measure(eng, freqs, weighted, power):
    ms = []
    for _ in range(7):
        eng.lomb_scargle(freqs, weighted=weighted, power=power, peak=True)
        ms.append(eng.last_kernel_ms)
    return float(np.median(ms[2:])), eng.last_solver


def main():
    rng = np.random.default_rng(1)
    eng = Engine(0)
    print("%-46s %10s %10s %10s  %s" % ("shape", "kernel ms", "FMA floor", "trig floor", "kernel"))
    for L, N, F, cases in ((2000, 10_000, 5000, ((True, True), (False, True), (True, False), (False, False))),
                           (1, 200_000, 100_000, ((True, True), (False, True)))):
        t = np.sort(rng.uniform(0.0, 1000.0, size=N)) + 58000.0
        y = rng.standard_normal((L, N))
        dy = rng.uniform(0.05, 0.3, size=(L, N))
        eng.set_lightcurves(t, y, dy)
        T = t[-1] - t[0]
        freqs = np.linspace(1.0 / T, 0.5 * N / T, F)
        for weighted, power in cases:
            ms, solver = measure(eng, freqs, weighted, power)
            R = int(solver.split("<")[1].rstrip(">"))
            fma = (7 if weighted else 2) * L * N * F / ISSUE_RATE * 1e3
            trig = (SINCOS_OPS + (0 if weighted else 5)) * -(-L // R) * N * F / ISSUE_RATE * 1e3
            print("L %4d N %6d F %6d %-9s power=%-5s %10.2f %10.2f %10.2f  %s  (the two floors together: %.0f %% of it)" %
                  (L, N, F, "weighted" if weighted else "1/N", power, ms, fma, trig, solver, 100.0 * (fma + trig) / ms))
    eng.close()


if __name__ == "__main__":
    main()
