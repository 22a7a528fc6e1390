#!/usr/bin/env python3
"""The numbers of profiles/iccf_probe.txt: mtg_iccf on the headline set (2000 light curves x N = 10^4 on shared sampling)
against a companion of M = 10^4 samples on its own sampling, one for all (L2 = 1) and one per light curve (L2 = L), at
K = 500 lags over +- a tenth and over +- half of the span, in mode both and with the companion half alone: kernel time
(mtg_last_kernel_ms) and the whole call.  Beside each setting the light variant of mtg_cross_sums of the same build at 128
bins over the same lag range -- N M pair visits against K (N + M) bracket visits -- and np.interp on the host, timed on a
slice of (light curve, lag, direction) calls and scaled.  The timing method is scripts/cross_probe.py's: one warm-up call,
then the median and the range of REPS calls.

    python3 scripts/iccf_probe.py [output file]
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mind_the_gaps_amd import synthetic as synth  # noqa: E402
from mind_the_gaps_amd.engine import Engine  # noqa: E402

N, M, L, K, REPS = 10000, 10000, 2000, 500, 3
LIGHT = dict(count=True, lag=True, cf=True, cf2=True)


def timed(eng, call):
    call()
    wall, kern = [], []
    for _ in range(REPS):
        t0 = time.perf_counter()
        call()
        wall.append(1e3 * (time.perf_counter() - t0))
        kern.append(eng.last_kernel_ms)
    text = "kernel %.1f ms (%.1f .. %.1f), call %.1f ms (%.1f .. %.1f)" % (np.median(kern), min(kern), max(kern), np.median(wall), min(wall), max(wall))
    return float(np.median(kern)), text


def main():
    out = open(sys.argv[1], "w") if len(sys.argv) > 1 else sys.stdout

    def say(line):
        out.write(line + "\n")
        out.flush()
    t, y, dy = synth.make_lightcurves(N, L, seed=1)
    span = t[-1] - t[0]
    rng = np.random.default_rng(3)
    t2 = np.sort(rng.uniform(t[0], t[-1], M))
    Y2 = rng.standard_normal((L, M))
    eng = Engine(0)
    eng.set_lightcurves(t, y, dy)
    say("%d light curves x N = %d on shared sampling, companion M = %d on its own sampling over the same span, K = %d lags" % (L, N, M, K))
    for name, reach in (("+- a tenth of the span", 0.1 * span), ("+- half the span", 0.5 * span)):
        lags = np.linspace(-reach, reach, K)
        say("K = %d lags over %s" % (K, name))
        ref, text = timed(eng, lambda: eng.cross_sums(t2, Y2[0], np.linspace(-reach, reach, 129), **LIGHT))
        say("  cross_sums L2 = 1, light, 128 bins: %s  [%s]" % (text, eng.last_solver))
        for comp_name, comp in (("L2 = 1", Y2[0]), ("L2 = L", Y2)):
            for mode in ("both", "companion"):
                ms, text = timed(eng, lambda: eng.iccf(t2, comp, lags, mode=mode, peak=True))
                say("  iccf %s, %-10s %s  [%s]  x %.2f of cross_sums" % (comp_name, mode + ":", text, eng.last_solver, ms / ref))
    eng.close()
    # the host: np.interp per (light curve, lag, direction); 4 light curves x 25 lags x 2 directions timed
    lags = np.linspace(-0.5 * span, 0.5 * span, K)[::20]
    t0 = time.perf_counter()
    for row in y[:4]:
        for tau in lags:
            np.interp(t + tau, t2, Y2[0])
            np.interp(t2 - tau, t, row)
    each = (time.perf_counter() - t0) / (4 * len(lags) * 2)
    say("np.interp on the host (the interpolation alone, no sums): %.0f us per call of 10^4 points; x 2 L K = %d calls = %.0f s"
        % (1e6 * each, 2 * L * K, each * 2 * L * K))


if __name__ == "__main__":
    main()
