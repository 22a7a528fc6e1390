#!/usr/bin/env python3
"""The numbers of profiles/wwz_probe.txt: mtg_wwz on the headline set (2000 light curves x N = 10^4 on shared sampling,
F = 500 frequencies up to the mean Nyquist rate, T = 100 centres, Foster's decay), both weightings -- kernel time
(mtg_last_kernel_ms), whole-call time with peaks only, and the share of (workgroup, chunk) pairs the kernel skips -- beside
the one-term mtg_lomb_scargle of the same build at F T = 5 x 10^4 frequencies: the same number of (light curve, tau, f)
fits with no window.  One warm-up call, then the median and the range of REPS calls.

    python3 scripts/wwz_probe.py
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mind_the_gaps_amd import synthetic as synth  # noqa: E402
from mind_the_gaps_amd.engine import WWZ_DECAY, Engine  # noqa: E402

N, L, F, T, REPS, CHUNK, LANES = 10000, 2000, 500, 100, 5, 256, 256
CUT = 80.0 * np.log(2.0)


def skipped_share(t, freqs, taus):
    """the kernel's rule restated: a chunk is kept unless its least |t - tau| is cut at the workgroup's lowest frequency"""
    kept = total = 0
    for k0 in range(0, len(freqs), LANES):
        flow = freqs[k0:k0 + LANES].min()
        for tau in taus:
            te = t - tau
            near2 = np.min(te * te)
            for n0 in range(0, len(t), CHUNK):
                a, b = te[n0], te[min(n0 + CHUNK, len(t)) - 1]
                m = a if a >= 0 else -b if b <= 0 else 0.0
                kept += not (4.0 * np.pi ** 2 * WWZ_DECAY * flow * flow * (m * m - near2) > CUT)
                total += 1
    return 1.0 - kept / total


def timed(eng, call):
    call()
    wall, kern = [], []
    for _ in range(REPS):
        t0 = time.perf_counter()
        call()
        wall.append(1e3 * (time.perf_counter() - t0))
        kern.append(eng.last_kernel_ms)
    return "kernel %.1f ms (%.1f .. %.1f), call %.1f ms (%.1f .. %.1f)" % (np.median(kern), min(kern), max(kern), np.median(wall), min(wall), max(wall))


def main():
    t, y, dy = synth.make_lightcurves(N, L, seed=1)
    span = t[-1] - t[0]
    freqs = np.linspace(1.0 / span, 0.5 * N / span, F)
    taus = np.linspace(t[0], t[-1], T)
    many = np.linspace(1.0 / span, 0.5 * N / span, F * T)
    eng = Engine(0)
    eng.set_lightcurves(t, y, dy)
    print("%d light curves x N = %d, shared sampling; F = %d up to the mean Nyquist rate, T = %d, decay 1 / (8 pi^2)" % (L, N, F, T))
    print("chunks skipped: %.1f %% of (workgroup, chunk) pairs" % (100.0 * skipped_share(t, freqs, taus)))
    for weighted in (True, False):
        tag = "weighted" if weighted else "unweighted"
        print("wwz %-10s peaks only: %s  [%s]" % (tag, timed(eng, lambda: eng.wwz(freqs, taus, weighted=weighted, values=False, peak=True)), eng.last_solver))
        print("lomb_scargle %-10s F = %d, peaks only: %s  [%s]" % (tag, F * T, timed(eng, lambda: eng.lomb_scargle(many, weighted=weighted, power=False, peak=True)),
                                                                     eng.last_solver))
    eng.close()


if __name__ == "__main__":
    main()
