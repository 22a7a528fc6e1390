#!/usr/bin/env python3
"""Times of mtg_epoch_fold at the headline shape (2000 light curves x N = 10^4 x 5000 frequencies, shared sampling) for
nbins 10 and 32, weighted and unweighted: kernel time (mtg_last_kernel_ms: pre-pass, sweeps, peaks) and whole-call time,
powers and peaks-only, each the median of 5 calls after 2 warm-ups with the spread (min .. max) beside it.  For
comparison mtg_lomb_scargle of the same build at the same shape, and the host route -- np.bincount per frequency, timed
on a slice of SLICE_L light curves x SLICE_F frequencies and SCALED to the shape (the line says so).

Every step runs in a child process under a time limit of its own; the first that fails ends the run.  Writes
profiles/epoch_fold_probe.txt.

Run on a GPU:  python3 scripts/epoch_fold_probe.py
"""
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

L, N, F = 2000, 10_000, 5000
SLICE_L, SLICE_F = 4, 50
STEPS = [("ef %d %d" % (nb, w), 240) for nb in (10, 32) for w in (1, 0)] + [("ls 0 1", 120), ("ls 0 0", 120), ("host 10 0", 120)]


def data():
    rng = np.random.default_rng(1)
    t = np.sort(rng.uniform(0.0, 1000.0, size=N)) + 58000.0
    T = t[-1] - t[0]
    return t, rng.standard_normal((L, N)), rng.uniform(0.05, 0.3, size=(L, N)), np.linspace(1.0 / T, 0.5 * N / T, F)


def timed(call, eng):
    kernel, whole = [], []
    for _ in range(7):
        t0 = time.perf_counter()
        call()
        whole.append((time.perf_counter() - t0) * 1e3)
        kernel.append(eng.last_kernel_ms)
    k, w = np.array(kernel[2:]), np.array(whole[2:])
    return "kernel %8.1f ms (%.1f .. %.1f)  call %8.1f ms (%.1f .. %.1f)" % (np.median(k), k.min(), k.max(), np.median(w), w.min(), w.max())


def step(kind, nb, weighted):
    t, y, dy, freqs = data()
    if kind == "host":
        w = np.full(N, 1.0 / N)
        t0 = time.perf_counter()
        for l in range(SLICE_L):
            r = w * (y[l] - y[l].mean())
            for f in freqs[:SLICE_F]:
                b = np.floor((((t - t[0]) * f) % 1) * nb).astype(np.int64)
                W, S = np.bincount(b, weights=w, minlength=nb), np.bincount(b, weights=r, minlength=nb)
                np.sum(S[W > 0] ** 2 / W[W > 0])
        ms = (time.perf_counter() - t0) * 1e3
        print("host route (np.bincount per frequency, rounded-product bins, one core), nbins %d: %.1f ms for %d x %d, SCALED to "
              "%d x %d: %.0f s" % (nb, ms, SLICE_L, SLICE_F, L, F, ms * (L / SLICE_L) * (F / SLICE_F) / 1e3))
        return
    from mind_the_gaps_amd.engine import Engine
    eng = Engine(0)
    eng.set_lightcurves(t, y, dy)
    for power in (True, False):
        if kind == "ef":
            line = timed(lambda: eng.epoch_fold(freqs, nbins=nb, weighted=bool(weighted), power=power, peak=True), eng)
            name = "epoch_fold nbins %2d" % nb
        else:
            line = timed(lambda: eng.lomb_scargle(freqs, weighted=bool(weighted), power=power, peak=True), eng)
            name = "lomb_scargle       "
        print("%s %-9s %-11s %s  %s" % (name, "weighted" if weighted else "1/N", "powers+peaks" if power else "peaks only", line, eng.last_solver))
    eng.close()


def main():
    if len(sys.argv) > 1:
        return step(sys.argv[1], int(sys.argv[2]), int(sys.argv[3]))
    out = os.path.join(ROOT, "profiles", "epoch_fold_probe.txt")
    lines = ["mtg_epoch_fold at L = %d light curves x N = %d samples x F = %d frequencies, shared sampling (scripts/epoch_fold_probe.py):" % (L, N, F),
             "median of 5 calls after 2 warm-ups (min .. max); kernel = mtg_last_kernel_ms, call = the whole call with its copies.", ""]
    for args, limit in STEPS:
        r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args.split(), capture_output=True, text=True, timeout=limit)
        lines += r.stdout.splitlines()
        print(r.stdout, end="", flush=True)
        if r.returncode != 0:
            lines.append("step %r failed (exit %d): %s" % (args, r.returncode, r.stderr.strip()[-400:]))
            break
    floor = L * N * F * 17.0 / 64.0 / (256 * 2.4e9) * 1e3
    lines += ["", "Where the time is suspected to go (reasoning from the documented LDS rates; no counters were collected, so this is a", "hypothesis, not a measurement): per (sample, frequency, light",
              "curve) the sweep does one 16-byte LDS read-modify-write, 4 + 13 LDS cycles per wave instruction pair on a CU's one",
              "LDS: %.0f ms at this shape if the LDS never idled, against 2 to 7 FMAs for one-term Lomb-Scargle.  The read -> add ->" % floor,
              "write chain of one sample must finish before the next sample of the same bin, and the waves that could hide it are",
              "bounded by the LDS itself: 160 KiB / (1 KiB x nbins x tile) waves per CU, 12 at nbins = 10 and 4 at nbins = 32 --",
              "which would explain why 32 bins cost more than 10 at the same number of read-modify-writes.  Nothing here was tuned."]
    with open(out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return 1 if r.returncode else 0


if __name__ == "__main__":
    sys.exit(main())
