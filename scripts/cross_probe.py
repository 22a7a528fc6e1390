#!/usr/bin/env python3
"""The numbers of profiles/cross_probe.txt: mtg_cross_sums on the headline set (2000 light curves x N = 10^4 on shared
sampling) against a companion of M = 10^4 samples on its own sampling, one for all (L2 = 1) and one per light curve
(L2 = L), at two bin settings -- 50 linear bins over +- a tenth of the span, 128 over +- the span -- with the light variant
(count, lag, cf, cf2) and with all eight sums: kernel time (mtg_last_kernel_ms) and the whole call.  Beside each the
mtg_lag_sums of the same build on the matching positive-half bins (cf + cf2, and all six), the ratio of the kernel times
beside the ratio of the pairs visited (those whose chunk a workgroup does not skip: N M in the window against N^2 / 2), and
the share of (workgroup, chunk) pairs that late start and early exit skip.  The timing method is scripts/lag_probe.py's:
one warm-up call, then the median and the range of REPS calls.

    python3 scripts/cross_probe.py [output file]
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cross_numpy as cn  # noqa: E402
from mind_the_gaps_amd import synthetic as synth  # noqa: E402
from mind_the_gaps_amd.engine import Engine  # noqa: E402

N, M, L, REPS = 10000, 10000, 2000, 3
LIGHT = dict(count=True, lag=True, cf=True, cf2=True)
FULL = dict(LIGHT, sa=True, sb=True, saa=True, sbb=True)


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


def lag_visited(t, edges):
    """pairs in the chunks the lag sweep visits: a row block walks from its own chunk to its early exit"""
    total = 0
    for row0 in range(0, len(t), 256):
        rows = min(256, len(t) - row0)
        last = t[row0 + rows - 1]
        for n0 in range(row0, len(t), 256):
            if t[n0] - last >= edges[-1]:
                break
            total += rows * min(256, len(t) - n0)
    return total


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
    settings = [("50 linear bins over +- a tenth of the span", np.linspace(-0.1 * span, 0.1 * span, 51), np.linspace(0.0, 0.1 * span, 26)),
                ("128 linear bins over +- the span", np.linspace(-span, span, 129), np.linspace(0.0, span, 65))]
    eng = Engine(0)
    eng.set_lightcurves(t, y, dy)
    say("%d light curves x N = %d on shared sampling, companion M = %d on its own sampling over the same span" % (L, N, M))
    for name, edges, half in settings:
        late, early, total = cn.skipped_chunks(t, t2, edges)
        visited = 256.0 * 256.0 * (total - late - early)        # (whole chunks: an upper bound that is tight at these sizes)
        lag_pairs = lag_visited(t, half)
        say(name)
        say("  (workgroup, chunk) pairs skipped: %.1f %% by late start, %.1f %% by early exit; pairs visited per light curve %.3g, "
            "lag_sums on the positive half (%d bins) %.3g: ratio %.2f" % (100.0 * late / total, 100.0 * early / total, visited, len(half) - 1,
                                                                        lag_pairs, visited / lag_pairs))
        ref = {}
        for label, want in (("cf + cf2", dict(count=True, lag=True, sf=False, cf=True, cf2=True)),
                            ("all six", dict(count=True, lag=True, sf=True, cf=True, cf2=True, noise=True))):
            ref[label], text = timed(eng, lambda: eng.lag_sums(half, **want))
            say("  lag_sums %-9s %s  [%s]" % (label + ":", text, eng.last_solver))
        for comp_name, comp in (("L2 = 1", Y2[0]), ("L2 = L", Y2)):
            for label, want, against in (("light", LIGHT, "cf + cf2"), ("all eight", FULL, "all six")):
                ms, text = timed(eng, lambda: eng.cross_sums(t2, comp, edges, **want))
                say("  cross_sums %s, %-10s %s  [%s]  x %.2f of lag_sums %s" % (comp_name, label + ":", text, eng.last_solver, ms / ref[against], against))
    eng.close()
    t0 = time.perf_counter()
    cn.cross_sums(t[:2000], y[0][:2000], t2[:2000], Y2[0][:2000], settings[0][1])
    one = (time.perf_counter() - t0) * (N / 2000.0) * (M / 2000.0)
    say("numpy helper, one light curve, %s: %.1f s on the host (2000 x 2000 samples scaled by the pairs); x %d light curves = %.0f s"
        % (settings[0][0], one, L, one * L))


if __name__ == "__main__":
    main()
