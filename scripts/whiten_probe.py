#!/usr/bin/env python3
"""Times mtg_whiten on the headline model (DRW + SHO + Lorentzian) and measures the device's erfc.

Sweep cost: whiten (residuals only, from a given y) against gp_draw with given normals -- the same step functions and
the same tile traffic -- at B = 256, N = 1e4; B = 2000 rows over 2000 resident light curves, N = 1e4; B = 1, N = 2e5.
Diagnostics: the whole residual-diagnostics call (stats and K = N / 4 lags, no [B][N] array copied back) at B = 2000,
N = 1e4 against the host route on the same q (q copied back, then ks_1samp and np.correlate per row; timed on 20 rows and
scaled); and the stats-only call (one sweep, nothing of size N stored) against loglike of the same rows.
Host clock around the whole call, warm-up first, the variants interleaved, median and (min .. max) of REPEATS.

erfc: with one sample per light curve stats[6] = D- IS Phi(q) = erfc(-q / sqrt 2) / 2 as the device rounds it, so
2 stats[6] is the device's erfc at a = fl(-q 0.7071067811865476), an argument the host forms with the same single
rounding.  E, the figure the KS bound (2 E + 8) u of tests/test_whiten_gpu.py takes, is the worst
|erfc_device(a) - erfc(a)| in ulp of erfc(a) against mpmath at 30 digits, over the q the device itself returns for the
rows of that test (tests/whiten_replay.ks_case, N = 257 and 1000: 3771 values).  Next to it the same figure and the
absolute error of Phi in u = 2^-53 over 4096 other values of q in [-8, 8].

The sweep's kernel time: mtg_whiten records its kernels' time (last_kernel_ms); mtg_gp_draw records none, so its kernel
time is estimated as its call minus what whiten's call spends outside its kernel (the same uploads and downloads of
[B][N] doubles) -- labelled as an estimate.

    python scripts/whiten_probe.py            -> profiles/whiten_probe.txt
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))      # whiten_replay.ks_case: the rows of the KS test

from mind_the_gaps_amd import synthetic as synth  # noqa: E402
from mind_the_gaps_amd.engine import Engine  # noqa: E402

REPEATS = 5


def race(jobs):
    for fn in jobs.values():
        fn()
    times = {k: [] for k in jobs}
    for _ in range(REPEATS):
        for k, fn in jobs.items():
            t0 = time.perf_counter()
            fn()
            times[k].append(time.perf_counter() - t0)
    return {k: (float(np.median(v)), min(v), max(v)) for k, v in times.items()}


def show(r):
    return "%.4f s (%.4f .. %.4f)" % r


def device_phi(eng, q):
    """Phi(q) as the device rounds it, through D- of one-sample rows under a white model of unit variance (q = y exactly)"""
    eng.set_lightcurves(np.zeros(1), np.zeros((1, 1)), np.ones((1, 1)))
    eng.set_model([synth.K_JITTER], np.array([-40.0, 0.0]), np.array([0], dtype=np.int32), np.tile([-np.inf, np.inf], (2, 1)))
    qd, _, st, status = eng.whiten(np.full((len(q), 1), -40.0), y=np.asarray(q)[:, None])
    assert np.all(status == 0) and np.array_equal(qd[:, 0], q)
    return st[:, 6]


def erfc_errors(eng, q):
    """(worst error of the device's erfc at fl(-q / sqrt 2) in ulp of the value, worst absolute error of Phi(q) in u)"""
    import mpmath as mp
    phi = device_phi(eng, q)
    arg = -np.asarray(q) * 0.70710678118654752440
    worst_ulp = worst_abs = 0.0
    with mp.workdps(30):
        for x, a, p in zip(q, arg, phi):
            true = mp.erfc(mp.mpf(float(a)))
            worst_ulp = max(worst_ulp, float(abs(2 * mp.mpf(float(p)) - true) / mp.mpf(float(np.spacing(float(true))))))
            worst_abs = max(worst_abs, float(abs(mp.mpf(float(p)) - mp.ncdf(mp.mpf(float(x)))) / mp.mpf(2) ** -53))
    return worst_ulp, worst_abs


def ks_rows_q(eng):
    """the q the device returns for the rows of the KS test, N = 257 and 1000"""
    import whiten_replay as WR
    out = []
    for N in (257, 1000):
        t, y, dy, theta, data = WR.ks_case(N)
        eng.set_lightcurves(t, y, dy + 1e-12, y_offset=np.zeros(1))
        eng.set_model([synth.K_JITTER], np.array([-0.3, 0.0]), np.array([0], dtype=np.int32), np.tile([-np.inf, np.inf], (2, 1)))
        q, _, _, status = eng.whiten(theta, y=data, stats=False)
        assert np.all(status == 0)
        out.append(q.ravel())
    return np.concatenate(out)


def main():
    kinds = synth.ALT_MODEL
    eng = Engine(0)
    lines = ["whiten_probe: headline model %s, median (min .. max) of %d interleaved repeats, host clock around the call" % (kinds, REPEATS)]
    q_test = ks_rows_q(eng)
    e_ulp, e_abs = erfc_errors(eng, q_test)
    lines.append("E: device erfc against mpmath at the %d q of the KS test's rows (|q| <= %.2f): worst %.2f ulp of the value; "
                 "Phi worst %.2f u absolute" % (len(q_test), np.max(np.abs(q_test)), e_ulp, e_abs))
    other = np.concatenate([np.linspace(-8.0, 8.0, 3072), np.random.default_rng(1).standard_normal(1024)])
    e_ulp, e_abs = erfc_errors(eng, other)
    lines.append("   the same over 4096 other q in [-8, 8]: worst %.2f ulp of the value; Phi worst %.2f u absolute" % (e_ulp, e_abs))
    for B, N, L in ((256, 10000, 1), (2000, 10000, 2000), (1, 200000, 1)):
        t, y, dy = synth.make_lightcurves(N, L, seed=1)
        full, free, bounds = synth.model_spec(kinds, y, per_lc_mean=True)
        eng.set_lightcurves(t, y, dy + 1e-12, y_offset=y.mean(axis=1))
        eng.set_model(kinds, full, free, bounds)
        theta = synth.draw_thetas(kinds, B, seed=B, percent=0.02)
        lc = (np.arange(B) % L).astype(np.int32)
        q = np.random.default_rng(B).standard_normal((B, N))
        data, _ = eng.gp_draw(theta, lc_index=lc, normals=q)
        kernel_ms = []

        def whiten():
            eng.whiten(theta, lc_index=lc, y=data, stats=False)
            kernel_ms.append(eng.last_kernel_ms)

        r = race({"draw": lambda: eng.gp_draw(theta, lc_index=lc, normals=q), "whiten": whiten})
        kms = float(np.median(kernel_ms[1:]))         # of the timed calls
        draw_kms = 1e3 * r["draw"][0] - (1e3 * r["whiten"][0] - kms)
        lines.append("B = %-5d N = %-7d L = %-5d whole call: gp_draw given %s | whiten given y, residuals only %s | ratio %.2f"
                     % (B, N, L, show(r["draw"]), show(r["whiten"]), r["whiten"][0] / r["draw"][0]))
        lines.append("    kernel alone: whiten %.3f ms (recorded) | gp_draw %.3f ms (estimate: its call minus whiten's copies) | ratio %.2f"
                     % (kms, draw_kms, kms / draw_kms))
        if B == 2000:
            from scipy.stats import ks_1samp, norm
            K = N // 4
            qd = eng.whiten(theta, lc_index=lc, stats=False)[0]

            def host_rows(rows=20):
                for b in range(rows):
                    ks_1samp(qd[b], norm.cdf)
                    full_ = np.correlate(qd[b], qd[b], mode="full")
                    full_[N:N + K] / full_[N - 1]

            r = race({"device": lambda: eng.whiten(theta, lc_index=lc, residuals=False, lags=K),
                      "copy": lambda: eng.whiten(theta, lc_index=lc, stats=False),
                      "host20": host_rows,
                      "sums": lambda: eng.whiten(theta, lc_index=lc, residuals=False, ks=False),
                      "loglike": lambda: eng.loglike(theta, lc, add_prior=False)})
            host = r["copy"][0] + r["host20"][0] * B / 20.0
            lines.append("    diagnostics, K = %d: device %s | host route: q copied back %s + ks_1samp and np.correlate %.2f s (20 rows scaled) "
                         "= %.2f s: %.1f x" % (K, show(r["device"]), show(r["copy"]), r["host20"][0] * B / 20.0, host, host / r["device"][0]))
            lines.append("    stats only %s | loglike %s (%s) | ratio %.2f"
                         % (show(r["sums"]), show(r["loglike"]), eng.last_solver, r["sums"][0] / r["loglike"][0]))
    eng.close()
    text = "\n".join(lines) + "\n"
    print(text)
    out = os.path.join(ROOT, "profiles", "whiten_probe.txt")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
