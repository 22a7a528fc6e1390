#!/usr/bin/env python3
"""Times the prediction at new times: Engine.predict_at (mtg_predict_at: checkpointed factorisation, linear in N and M)
against the method it replaces in GP.predict -- the dense cross-covariance K_* [M][N] built on the host, sent as M + 1
right-hand sides of Engine.apply_inverse and multiplied back on the host (reproduced here; apply_inverse is unchanged).

N = 1e4, DRW + SHO + Lorentzian, B = 1, M in {48, 1e3, 1e4}: both methods, every shape warmed up, the two alternated
within one process, a host clock around calls that end in a stream synchronisation.  Then Engine.predict_at alone for
(B, M) in {(1, 1e6), (256, 1e4)} and for N = 2e5 with five SHO terms (J = 10), M = 1e6.  Reported per shape: the
median and the spread (max - min) of the repeats.  The one condition: at none of the three compared shapes is the new
method slower than the old one by more than the old one's own spread.

    python scripts/predict_at_probe.py [--out profiles/predict_at_probe.txt] [--repeats 7]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mind_the_gaps_amd import synthetic as synth  # noqa: E402
from mind_the_gaps_amd.engine import Engine  # noqa: E402
from oracle import dense  # noqa: E402


def old_method(eng, kinds, th, t, resid, ts):
    """GP.predict(y, t=ts, return_var=True) as it was assembled on the host"""
    co = dense.build_coeffs(kinds, th)
    kxs = dense.kernel_value(co, ts[:, None] - t[None, :])
    sol, status = eng.apply_inverse(th, np.column_stack([resid, kxs.T]))
    assert status == 0
    return kxs @ sol[:, 0], dense.kernel_value(co, 0.0) - np.sum(kxs.T * sol[:, 1:], axis=0)


def clock(fn, eng):
    eng.synchronize()
    started = time.perf_counter()
    out = fn()
    eng.synchronize()
    return time.perf_counter() - started, out


def stats(v):
    return float(np.median(v)), float(np.max(v) - np.min(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    eng = Engine(0)
    kinds = synth.ALT_MODEL
    N = 10000
    t, y, dy = synth.make_lightcurves(N, 1, seed=3)
    full, free, bounds = synth.model_spec(kinds, y, per_lc_mean=True)
    eng.set_lightcurves(t, y, dy + 1e-12, y_offset=y.mean(axis=1))
    eng.set_model(kinds, full, free, bounds)
    th = synth.truth(kinds)
    resid = y[0] - y[0].mean()
    span = t[-1] - t[0]
    say("predict at new times, N = %d, DRW + SHO + Lorentzian (J = 6), B = 1: seconds, median (spread = max - min) of the repeats" % N)
    say("%8s %8s %24s %24s %8s  %s" % ("M", "repeats", "host assembly (old)", "mtg_predict_at (new)", "old/new", "condition"))
    verdict = True
    for M in (48, 1000, 10000):
        ts = np.linspace(t[0] - 0.01 * span, t[-1] + 0.01 * span, M)
        reps = args.repeats if M < 10000 else max(3, args.repeats // 2)
        a = old_method(eng, kinds, th, t, resid, ts)            # warm-up of both, and a check that they agree
        mu, var, st = eng.predict_at(th[None, :], ts)
        assert st[0] == 0 and np.allclose(mu[0], a[0], rtol=0, atol=1e-8 * np.max(np.abs(a[0])))
        assert np.allclose(var[0], a[1], rtol=0, atol=1e-8 * dense.kernel_value(dense.build_coeffs(kinds, th), 0.0))
        old, new = [], []
        for _ in range(reps):
            old.append(clock(lambda: old_method(eng, kinds, th, t, resid, ts), eng)[0])
            new.append(clock(lambda: eng.predict_at(th[None, :], ts), eng)[0])
        (mo, so), (mn, sn) = stats(old), stats(new)
        ok = mn <= mo + so
        verdict = verdict and ok
        say("%8d %8d %14.4f (%7.4f) %14.4f (%7.4f) %8.1f  %s" % (M, reps, mo, so, mn, sn, mo / mn,
                                                                "holds" if ok else "FAILS: new > old + spread"))
    say("condition (new <= old + spread of old at all three shapes): %s" % ("holds" if verdict else "FAILS"))
    say("")
    say("mtg_predict_at alone: seconds, median (spread)")
    for B, M in ((1, 1000000), (256, 10000)):
        ts = np.linspace(t[0] - 0.01 * span, t[-1] + 0.01 * span, M)
        theta = synth.draw_thetas(kinds, B, seed=B, percent=0.05) if B > 1 else th[None, :]
        eng.predict_at(theta, ts)
        v = [clock(lambda: eng.predict_at(theta, ts), eng)[0] for _ in range(max(3, args.repeats // 2))]
        say("N = %6d J = 6  B = %4d M = %8d   %.4f (%.4f)" % (N, B, M, *stats(v)))
        v = [clock(lambda: eng.predict_at(theta, ts, return_var=False), eng)[0] for _ in range(max(3, args.repeats // 2))]
        say("N = %6d J = 6  B = %4d M = %8d   %.4f (%.4f)   mean only" % (N, B, M, *stats(v)))
    # the largest configuration of BASELINE.json: N = 2e5, five SHO terms
    kinds5 = [synth.K_SHO] * 5
    N5, M5 = 200000, 1000000
    t5, y5, dy5 = synth.make_lightcurves(N5, 1, seed=20250709)
    full5, free5, bounds5 = synth.model_spec(kinds5, y5, per_lc_mean=True)
    eng.set_lightcurves(t5, y5, dy5 + 1e-12, y_offset=y5.mean(axis=1))
    eng.set_model(kinds5, full5, free5, bounds5)
    th5 = synth.truth(kinds5)
    span5 = t5[-1] - t5[0]
    for M in (48, M5):
        ts = np.linspace(t5[0] - 0.01 * span5, t5[-1] + 0.01 * span5, M)
        mu, var, st = eng.predict_at(th5[None, :], ts)
        assert st[0] == 0
        v = [clock(lambda: eng.predict_at(th5[None, :], ts), eng)[0] for _ in range(3)]
        say("N = %6d J = 10 B = %4d M = %8d   %.4f (%.4f)%s" % (
            N5, 1, M, *stats(v), "   (the factorisation stage, one serial lane, is nearly all of it)" if M == 48 else ""))
    eng.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
