"""Cost of the per-term prediction (Engine.predict_terms) beside Engine.predict_at of the same build on the same shapes:
the headline model (DRW + SHO + Lorentzian, rank 5) with variance,

    B = 256, N = M = 1e4, T = 1 and T = 3        B = 1, N = 2e5, M = 1e6, T = 3.

Whole-call times as the host sees them (uploads, kernels, the copy back: predict_terms returns T times as many doubles):
one warm-up call, then the median and the range of five.  Kernel times from `rocprofv3 --kernel-trace --stats` over a
child process per (entry, shape) that makes one warm-up call and three more: the average and the range of the
factorisation kernel and of the evaluation kernel over those calls.  The design intends the evaluation of T = 3 to cost
close to that of T = 1, and both close to mtg_predict_at's: the replay is done once.  Writes
profiles/predict_terms_probe.txt.

    python scripts/predict_terms_probe.py"""
import csv
import glob
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mind_the_gaps_amd import synthetic as synth  # noqa: E402
from mind_the_gaps_amd.engine import Engine  # noqa: E402

SHAPES = ((10000, 10000, 256), (200000, 1000000, 1))
CONFIGS = ((0, 0), (0, 1), (0, 3), (1, 0), (1, 3))          # (shape, T); T = 0: predict_at


def bind(eng, shape):
    N, M, B = SHAPES[shape]
    kinds = synth.ALT_MODEL
    theta = synth.truth(kinds)
    P = len(theta)
    t, y, dy = synth.make_lightcurves(N, 1, seed=N)
    eng.set_lightcurves(t, y, dy + 1e-12, y_offset=y.mean(axis=1))
    eng.set_model(kinds, np.concatenate([theta, [0.0]]), np.arange(P, dtype=np.int32), np.tile([-np.inf, np.inf], (P + 1, 1)))
    ts = np.sort(np.random.default_rng(M).uniform(t[0] - 10.0, t[-1] + 10.0, M))
    return np.tile(theta, (B, 1)), ts


def call_of(eng, th, ts, T):
    if T == 0:
        return lambda: eng.predict_at(th, ts)
    masks = [1, 2, 4][:T]
    return lambda: eng.predict_terms(th, masks, ts)


def child(shape, T):
    eng = Engine(0)
    th, ts = bind(eng, shape)
    call = call_of(eng, th, ts, T)
    for _ in range(4):
        call()
    eng.close()


def kernel_times(shape, T):
    """{'factor' | 'eval': (average, min, max) in ms} of one call, from the profiler's statistics"""
    out = tempfile.mkdtemp(prefix="mtg_predict_terms_probe_")
    subprocess.check_call(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--", sys.executable,
                           os.path.abspath(__file__), "--child", str(shape), str(T)], stdout=subprocess.DEVNULL,
                          stderr=subprocess.DEVNULL, timeout=900)
    found = {}
    for path in glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            for key, tag in (("factor", "mtg_predict_at_factor_kernel"), ("eval", "_eval_kernel")):
                if tag in row["Name"]:
                    found[key] = (float(row["AverageNs"]) * 1e-6, float(row["MinNs"]) * 1e-6, float(row["MaxNs"]) * 1e-6)
    return found


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        return child(int(sys.argv[2]), int(sys.argv[3]))
    kern = {cfg: kernel_times(*cfg) for cfg in CONFIGS}          # (before this process opens the device)
    eng = Engine(0)
    lines = ["predict_terms beside predict_at, headline model (rank 5), with variance (scripts/predict_terms_probe.py)",
             "whole call: median [min, max] of 5 after a warm-up, ms, copies included (predict_terms copies back T x as much)",
             "kernels: average [min, max] over 4 calls under rocprofv3 --kernel-trace --stats, ms",
             "%8s %8s %5s %-14s %26s %26s %26s" % ("N", "M", "B", "entry", "whole call", "factor kernel", "eval kernel")]
    base = {}
    for shape, T in CONFIGS:
        N, M, B = SHAPES[shape]
        th, ts = bind(eng, shape)
        call = call_of(eng, th, ts, T)
        call()
        times = []
        for _ in range(5):
            t0 = time.perf_counter()
            call()
            times.append(1e3 * (time.perf_counter() - t0))
        k = kern[(shape, T)]
        fmt = lambda v: "%9.2f [%6.2f, %6.2f]" % v
        lines.append("%8d %8d %5d %-14s %26s %26s %26s" % (
            N, M, B, "predict_at" if T == 0 else "terms T = %d" % T, fmt((np.median(times), min(times), max(times))),
            fmt(k.get("factor", (np.nan,) * 3)), fmt(k.get("eval", (np.nan,) * 3))))
        print(lines[-1], flush=True)
        if T == 0:
            base[shape] = (np.median(times), k.get("eval", (np.nan,))[0])
        else:
            lines.append("%37s ratio to predict_at: whole call %.2f, eval kernel %.2f" % (
                "", np.median(times) / base[shape][0], k.get("eval", (np.nan,))[0] / base[shape][1]))
            print(lines[-1], flush=True)
    eng.close()
    with open(os.path.join(ROOT, "profiles", "predict_terms_probe.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
