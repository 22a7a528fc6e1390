#!/usr/bin/env python3
"""Three routes to the per-frequency envelope of the periodograms of 2000 light curves x N = 1e4 at 5000 frequencies (the
shape of scripts/lomb_scargle_probe.py), weighted and 1/N -- the median, three levels and the count of simulations at
or above a reference, per frequency:

1. before mtg_lomb_scargle_envelope: ``Engine.lomb_scargle(power=True)`` with its 80 MB copy back, then ``np.quantile``
   for the median and three levels and a ``>=`` count on the host;
2. ``Engine.lomb_scargle_envelope`` with the ranks of those quantiles and the reference (``envelope_levels`` included);
3. ``Engine.lomb_scargle(power=False, peak=True)``: the floor the periodogram itself sets.

Wall time of the whole route (time.perf_counter around the call, which ends with the stream drained), median of 5 after
2 warm-ups, on an otherwise idle GPU; beside it the device span of the call (mtg_last_kernel_ms: pre-pass to the last
slab's kernels, the copies of earlier slabs inside it).  The column kernel's own time is the difference of the spans of
route 2 and of the same slabs without column work (a call that asks for ratio peaks only), both measured here.

Run on a GPU:  python3 scripts/lomb_scargle_envelope_probe.py [output file]
"""
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mind_the_gaps_amd.engine import Engine  # noqa: E402
from mind_the_gaps_amd.periodogram import envelope_levels, envelope_ranks  # noqa: E402

LEVELS = (0.5, 0.95, 0.997, 0.9999)


def timed(fn, eng):
    wall, span = [], []
    for _ in range(7):
        t0 = time.perf_counter()
        out = fn()
        wall.append((time.perf_counter() - t0) * 1e3)
        span.append(eng.last_kernel_ms)
    return float(np.median(wall[2:])), float(np.median(span[2:])), out


def main():
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    try:
        head = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        head = ""
    say("mtg_lomb_scargle_envelope against the host route, MI355X, scripts/lomb_scargle_envelope_probe.py; on commit %s" % (head or "unknown"))
    say("L 2000 x N 10000 x F 5000, shared sampling; median, 0.95, 0.997, 0.9999 levels and the exceedance count per frequency.")
    say("wall = whole route on the host clock, span = mtg_last_kernel_ms of its device call; median of 5 after 2 warm-ups, ms.")
    say("")
    rng = np.random.default_rng(1)
    L, N, F = 2000, 10_000, 5000
    t = np.sort(rng.uniform(0.0, 1000.0, size=N)) + 58000.0
    y = rng.standard_normal((L, N))
    dy = rng.uniform(0.05, 0.3, size=(L, N))
    eng = Engine(0)
    eng.set_lightcurves(t, y, dy)
    T = t[-1] - t[0]
    freqs = np.linspace(1.0 / T, 0.5 * N / T, F)
    ranks = envelope_ranks(L, LEVELS)
    say("%-10s %-62s %10s %10s" % ("weights", "route", "wall", "span"))
    for weighted in (True, False):
        tag = "weighted" if weighted else "1/N"
        reference = eng.lomb_scargle(freqs, weighted=weighted)[0]          # light curve 0 plays the observed one

        def host_route():
            power = eng.lomb_scargle(freqs, weighted=weighted)
            return np.quantile(power, LEVELS, axis=0), np.sum(power >= reference, axis=0)

        def host_route_sort():
            power = eng.lomb_scargle(freqs, weighted=weighted)
            return envelope_levels(np.sort(power, axis=0)[ranks], ranks, L, LEVELS), np.sum(power >= reference, axis=0)

        def device_route():
            env = eng.lomb_scargle_envelope(freqs, ranks=ranks, reference=reference, weighted=weighted)
            return envelope_levels(env.order_stat, ranks, L, LEVELS), env.exceed

        w1, s1, r1 = timed(host_route, eng)
        w1s, s1s, r1s = timed(host_route_sort, eng)
        w2, s2, r2 = timed(device_route, eng)
        solver = eng.last_solver
        assert np.array_equal(r1[0], r2[0]) and np.array_equal(r1[1], r2[1]) and np.array_equal(r1s[0], r2[0])
        w3, s3, _ = timed(lambda: eng.lomb_scargle(freqs, weighted=weighted, power=False, peak=True), eng)
        w4, s4, _ = timed(lambda: eng.lomb_scargle_envelope(freqs, scale=np.ones(F), weighted=weighted), eng)
        say("%-10s %-62s %10.2f %10.2f" % (tag, "1  lomb_scargle(power=True) + np.quantile + >= count", w1, s1))
        say("%-10s %-62s %10.2f %10.2f" % (tag, "1' the same with np.sort in place of np.quantile", w1s, s1s))
        say("%-10s %-62s %10.2f %10.2f" % (tag, "2  lomb_scargle_envelope(ranks, reference) + envelope_levels", w2, s2))
        say("%-10s %-62s %10.2f %10.2f" % (tag, "3  lomb_scargle(power=False, peak=True)", w3, s3))
        say("%-10s %-62s %10.2f %10.2f" % (tag, "   lomb_scargle_envelope(scale): the slabs without column work", w4, s4))
        say("%-10s route 1 / route 2 = %.1f (wall); results equal bit for bit; %s: span 2 - span without column work = %.2f ms"
            % (tag, w1 / w2, solver, s2 - s4))
        say("")
    eng.close()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
