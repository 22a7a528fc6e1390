#!/usr/bin/env python3
"""The numbers of profiles/lag_probe.txt: mtg_lag_sums on the headline set (2000 light curves x N = 10^4 on shared
sampling) at three bin settings -- 50 log bins to half the span, 50 linear bins to a tenth of the span (the early exit),
128 linear bins over the span -- with the structure function alone and with all six sums: kernel time
(mtg_last_kernel_ms) and the whole call.  Beside them the one-term unweighted mtg_lomb_scargle of the same build at 5000
frequencies (the same number of (row, column) visits, a sine and a cosine each) and tests/lag_numpy.py on ONE light curve
on the host, scaled to the set.  One warm-up call, then the median and the range of REPS calls.

    python3 scripts/lag_probe.py [output file]
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lag_numpy as ln  # noqa: E402
from mind_the_gaps_amd import synthetic as synth  # noqa: E402
from mind_the_gaps_amd import timedomain  # noqa: E402
from mind_the_gaps_amd.engine import Engine  # noqa: E402

N, L, F, REPS = 10000, 2000, 5000, 3


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
    out = open(sys.argv[1], "w") if len(sys.argv) > 1 else sys.stdout

    def say(line):
        out.write(line + "\n")
        out.flush()
    t, y, dy = synth.make_lightcurves(N, L, seed=1)
    span = t[-1] - t[0]
    settings = [("50 log bins to half the span", timedomain.lag_bins(t, 50, spacing="log")),
                ("50 linear bins to a tenth of the span", np.linspace(0.0, 0.1 * span, 51)),
                ("128 linear bins over the span", np.linspace(0.0, span, 129))]
    eng = Engine(0)
    eng.set_lightcurves(t, y, dy)
    say("%d light curves x N = %d, shared sampling: %.3g pairs per light curve" % (L, N, 0.5 * N * (N - 1)))
    freqs = np.linspace(1.0 / span, 0.5 * N / span, F)
    say("lomb_scargle unweighted, F = %d, peaks only: %s  [%s]" % (F, timed(eng, lambda: eng.lomb_scargle(freqs, weighted=False, power=False, peak=True)),
                                                                   eng.last_solver))
    for name, edges in settings:
        say(name)
        say("  sf alone: %s  [%s]" % (timed(eng, lambda: eng.lag_sums(edges, count=False, lag=False, sf=True)), eng.last_solver))
        say("  all six:  %s  [%s]" % (timed(eng, lambda: eng.lag_sums(edges, count=True, lag=True, sf=True, cf=True, cf2=True, noise=True)),
                                      eng.last_solver))
    eng.close()
    t0 = time.perf_counter()
    ln.lag_sums(t, y[0], dy[0], settings[0][1])
    one = time.perf_counter() - t0
    say("numpy helper, one light curve, %s: %.1f s on the host; x %d light curves = %.0f s" % (settings[0][0], one, L, one * L))


if __name__ == "__main__":
    main()
