#!/usr/bin/env python3
"""Generates tests/golden/quad_golden.json: the quad-precision truth (oracle/celerite_quad.c) of the likelihood at
the shapes the kernels run -- N up to 2e5, every regime where the device code branches -- for
tests/test_accuracy_vs_quad_gpu.py.

Light curves are not stored: each group names its recipe (synthetic.make_lightcurves(N, L, seed, offset), then an
optional edit of the sampling) and the SHA-256 of the float64 bytes of t, y, dy, which the tests check before use.
Per row: the full parameter vector (kernel parameters, then the mean: a constant, which the kernels see as the light
curve's y_offset, or -- mean_kind 1 -- a fitted (slope, intercept) line with no y_offset), the quad lnL as a double pair, the float64 coefficients oracle.dense.build_coeffs makes of theta
with their own quad truth (lnL_raw: the same likelihood with the builders' rounding in its inputs), the error scale S, the forward / reversed disagreement of the
quad sweep, celerite's float64 value and status (oracle_logprob_batch, its two-sweep algorithm) and d * max dx.
Rows the float64 oracle does not call positive definite, and rows whose two quad sweeps disagree by more than 1e-3 of
the row's tolerance, are dropped (and counted); every group must keep all its rows -- a lost row is replaced by
changing the recipe, never kept.

Run from the repo root:  python tests/golden/make_quad_golden.py   (~1 minute on 8 cores; deterministic)
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

from mind_the_gaps_amd import synthetic as synth  # noqa: E402
from oracle import celerite as oracle_c  # noqa: E402
from oracle import dense  # noqa: E402
from oracle import quad  # noqa: E402
from golden_util import lightcurve_sha256 as sha, quad_lightcurve as lightcurve  # noqa: E402

K = synth
U = 2.0 ** -53
NULL, ALT, FIVE = K.NULL_MODEL, K.ALT_MODEL, [K.K_SHO] * 5
CONFIG5 = np.array([v for i in range(5) for v in (np.log(20.0 + 10 * i), np.log([3.0, 8.0, 10.0, 1.0, 0.8][i]),
                                                  np.log(2 * np.pi / (5.0 + 6 * i)))])


def around(kinds, B, seed, spread=0.25):
    rng = np.random.default_rng(seed)
    th = synth.truth(kinds)
    return th + spread * np.abs(th) * rng.uniform(-1.0, 1.0, (B, len(th)))


def priors_ok(kinds, th):
    return dense.log_prior(kinds, np.concatenate([th, [0.0]]), np.tile([-np.inf, np.inf], (len(th) + 1, 1))) == 0.0


def groups():
    """(name, regime, kinds, lightcurve recipe, theta [B][P], tags per row)"""
    out = []

    def add(name, regime, kinds, rec, thetas, tags=None, mean_kind=0):
        thetas = np.atleast_2d(np.asarray(thetas, dtype=np.float64))
        out.append((name, regime, [int(k) for k in kinds], rec, thetas,
                    tags if tags is not None else [[] for _ in range(len(thetas))], mean_kind))

    def linear(kinds, B, seed, rec, slope):
        """kernel parameters 25 % around the tutorial values, then a fitted linear mean (slope, intercept): slopes
        around `slope`, the line through the light curve's average at mid-span (mean_models.py LinearModel)"""
        rng = np.random.default_rng(seed)
        t, y, _ = lightcurve(rec)
        sl = slope * (1.0 + 0.25 * rng.uniform(-1.0, 1.0, B))
        return np.hstack([around(kinds, B, seed + 1000), sl[:, None], (y.mean() - sl * t[len(t) // 2])[:, None]])

    lc = lambda N, seed, L=1, offset=0.0, edit=None: dict(N=N, L=L, seed=seed, offset=offset, edit=edit)
    # typical: 25 % around the tutorial values
    add("typical/null", "typical", NULL, lc(4096, 101), around(NULL, 12, 1))
    add("typical/alt", "typical", ALT, lc(4096, 101), around(ALT, 12, 2))
    add("typical/null_n64", "typical", NULL, lc(64, 102), around(NULL, 8, 3))
    add("typical/alt_n65", "typical", ALT, lc(65, 103), around(ALT, 8, 4))
    bm = [K.K_BPL, K.K_MATERN32]
    add("typical/bpl+matern32", "typical", bm, lc(1000, 104), [r for r in around(bm, 20, 5) if priors_ok(bm, r)][:8])
    cjs = [K.K_COSINUS, K.K_JITTER, K.K_SHO]
    add("typical/cosinus+jitter+sho", "typical", cjs, lc(4095, 105), around(cjs, 8, 6))
    c4r = [K.K_COMPLEX4, K.K_REAL]
    add("typical/complex4+real", "typical", c4r, lc(1000, 106), [r for r in around(c4r, 40, 7) if priors_ok(c4r, r)][:8])
    rng = np.random.default_rng(8)
    add("typical/5sho", "typical", FIVE, lc(10000, 107), CONFIG5 + 0.25 * np.abs(CONFIG5) * rng.uniform(-1, 1, (6, 15)))
    add("typical/jitter_only", "typical", [K.K_JITTER], lc(20011, 108), around([K.K_JITTER], 6, 9))
    # signatures: SHO quality factors straddling 1/2 in one batch, two light curves
    sig = [K.K_DRW, K.K_SHO, K.K_SHO]
    th = np.repeat(around(sig, 4, 10, spread=0.1), 5, axis=0)
    qs = np.log([0.3, 0.49, 0.4999, 0.5001, 0.51] * 4)
    th[:, 3] = qs
    th[::2, 6] = qs[::2][::-1]
    add("signatures", "signatures", sig, lc(4096, 110, L=2), th,
        [["Q=%.4g/%.4g" % (np.exp(r[3]), np.exp(r[6]))] for r in th])
    # long memory: c median(dx) from 1e-6 down to 1e-9, amplitudes e^10 .. e^20 (DRW and a complex term)
    rows, tags = [], []
    for i, (cm, amp) in enumerate([(1e-6, 10.0), (1e-7, 15.0), (1e-8, 20.0), (1e-9, 12.0), (1e-9, 20.0), (1e-7, 18.0)]):
        r = synth.truth([K.K_DRW, K.K_COMPLEX3]).copy()
        r[0], r[1] = amp, np.log(cm / 0.74)
        r[2], r[3] = amp - 2.0 * (i % 2), np.log(cm / 0.74)
        rows.append(r); tags.append(["c*dx=%g" % cm, "amp=e^%g" % amp])
    add("long_memory", "long_memory", [K.K_DRW, K.K_COMPLEX3], lc(10000, 111), rows, tags)
    # short memory: c dx across the exp underflow (700 .. 745) and far beyond, duplicate epochs and a 1e6 gap
    rows, tags = [], []
    for cdx in (700.0, 720.0, 745.0, 760.0, 1.0e4):
        r = synth.truth(NULL).copy()
        r[1] = np.log(cdx / 0.74)
        rows.append(r); tags.append(["c*dx=%g" % cdx])
    add("short_memory", "short_memory", NULL, lc(1000, 112, edit="dup_gap"), rows, tags)
    # phase: d max(dx) across the switches of the table reduction (1e5 tp_big fast, 1e12 MTG_TRIG_FAST_MAX)
    targets = (1e2, 0.9e5, 1.1e5, 1e8, 0.9e12, 1.1e12)
    rec = lc(10000, 113)
    dxmax = float(np.max(np.diff(lightcurve(rec)[0])))
    rows = []
    for x in targets:
        r = np.array([np.log(2.0), np.log(0.3), np.log(x / dxmax), np.log(1.5), np.log(0.2)])
        rows.append(r)
    add("phase/j3", "phase", [K.K_COMPLEX3, K.K_DRW], rec, rows, [["d*dxmax=%g" % x] for x in targets])
    rec = lc(20011, 114)
    dxmax = float(np.max(np.diff(lightcurve(rec)[0])))
    rows = []
    for x in targets:
        r = np.array([v for i in range(5) for v in (np.log(20.0 + 5 * i), np.log(0.05 + 0.02 * i), np.log(0.3 + 0.4 * i))])
        r[2] = np.log(x / dxmax)
        rows.append(r)
    add("phase/j10", "phase", [K.K_COMPLEX3] * 5, rec, rows, [["d*dxmax=%g" % x] for x in targets])
    # extreme: amplitude e^40 against unit noise, Q = 8000
    rows = []
    for i in range(6):
        r = CONFIG5.copy()
        if i % 2 == 0:
            r[3 * (i // 2)] = 40.0
        else:
            r[3 * (i // 2) + 1] = np.log(8000.0)
        rows.append(r)
    add("extreme/5sho", "extreme", FIVE, lc(10000, 115), rows, [["amp=e^40"] if i % 2 == 0 else ["Q=8000"] for i in range(6)])
    r = around(NULL, 4, 11)
    r[:2, 0], r[2:, 1] = 40.0, np.log(8000.0)
    add("extreme/null", "extreme", NULL, lc(4096, 116), r, [["amp=e^40"]] * 2 + [["Q=8000"]] * 2)
    # time offsets: MJD and seconds
    add("offset/mjd", "time_offset", ALT, lc(4096, 117, offset=5.9e4), around(ALT, 6, 12))
    add("offset/seconds", "time_offset", NULL, lc(1000, 118, offset=1.0e9), around(NULL, 6, 13))
    # a fitted linear mean (mean_kind 1, no y_offset): at t ~ 1e3 days, and at t ~ 1e9 s where slope * t ~ 2e3
    rec = lc(4096, 119)
    add("linear_mean/null", "linear_mean", NULL, rec, linear(NULL, 8, 15, rec, 2e-3), mean_kind=1)
    rec = lc(4096, 120, offset=1.0e9)
    add("linear_mean/null_seconds", "linear_mean", NULL, rec, linear(NULL, 8, 16, rec, 2e-6), mean_kind=1)
    j3 = [K.K_COMPLEX3, K.K_DRW]
    rec = lc(10000, 121, offset=1.0e9)
    add("linear_mean/j3_seconds", "linear_mean", j3, rec, linear(j3, 6, 17, rec, 2e-6), mean_kind=1)
    dr = [K.K_DRW, K.K_REAL]                     # no phase: celerite's own error stays at rounding level at t ~ 1e9
    rec = lc(10000, 123, offset=1.0e9)
    add("linear_mean/drw+real_seconds", "linear_mean", dr, rec, linear(dr, 6, 19, rec, 2e-6), mean_kind=1)
    rec = lc(10000, 122, offset=5.9e4)
    add("linear_mean/5sho_mjd", "linear_mean", FIVE, rec, linear(FIVE, 6, 18, rec, 1e-3), mean_kind=1)
    # rank 10 at the configs[4] size
    rng = np.random.default_rng(14)
    r = CONFIG5 + 0.05 * np.abs(CONFIG5) * rng.standard_normal((4, 15))
    r[3, 4] = np.log(0.3)                        # an over-damped oscillator: a second structure
    add("rank10/config5", "typical", FIVE, lc(200000, 20250709), r)
    return out


def dmaxdx(kinds, th, t):
    co = dense.build_coeffs(kinds, th)
    d = np.max(np.abs(co[5])) if len(co[5]) else 0.0
    return float(d * np.max(np.diff(t))) if len(t) > 1 else 0.0


def main():
    doc = {"generator": "tests/golden/make_quad_golden.py", "u": U,
           "truth": "oracle/celerite_quad.c (coefficients built from theta in quad); c64: oracle_logprob_batch",
           "groups": []}
    dropped = 0
    for name, regime, kinds, rec, thetas, tags, mean_kind in groups():
        t, y, dy = lightcurve(rec)
        L, N = y.shape
        lc = (np.arange(len(thetas)) % L).astype(np.int32)
        if mean_kind == 1:          # theta already ends with (slope, intercept); nothing subtracted at upload
            means = np.zeros(L)
            full, nm = thetas, 2
        else:                       # the frozen mean: the light curve's average, the kernels' y_offset
            means = y.mean(axis=1)
            full, nm = np.hstack([thetas, means[lc][:, None]]), 1
        hi, lo, S, st = quad.loglike(t, y, dy, kinds, full, lc_index=lc, mean_kind=mean_kind)
        rhi, rlo, _, rst = quad.loglike(t, y, dy, kinds, full, lc_index=lc, mean_kind=mean_kind, reverse=True)
        c64, cst = oracle_c.logprob_batch(t, y, dy, kinds, full, lc_index=lc, mean_kind=mean_kind,
                                          nthreads=quad.default_threads())
        rows = []
        for b in range(len(thetas)):
            if cst[b] != 0 or st[b] != 0 or rst[b] != 0:
                dropped += 1
                print("  dropped (not positive definite)", name, b, flush=True)
                continue
            fr = abs((hi[b] - rhi[b]) + (lo[b] - rlo[b]))
            e64 = abs((c64[b] - hi[b]) - lo[b])
            tol = max(10.0 * e64, 64.0 * np.sqrt(N) * U * S[b])
            if not fr < 1e-3 * tol:
                dropped += 1
                print("  dropped (forward / reverse %.3g against tolerance %.3g)" % (fr, tol), name, b, flush=True)
                continue
            # the truth of the float64 coefficients the builders round to (what Engine.loglike_coeffs is handed, and
            # what celerite's float64 run works from)
            kernel = full[b, :-nm]
            co = dense.build_coeffs(kinds, kernel)
            ch, cl, _, cs = quad.loglike_coeffs(t, y[lc[b]], dy[lc[b]], *(np.asarray(a)[None] for a in co[:6]),
                                                jitter=co[6], mean_kind=mean_kind, mean_params=[full[b, -nm:]])
            assert cs[0] == 0
            rows.append({"theta": [float(v) for v in full[b]], "lc": int(lc[b]), "lnL": float(hi[b]),
                         "coeffs": [[float(v) for v in a] for a in co[:6]] + [float(co[6])],
                         "lnL_raw": float(ch[0]), "lnL_raw_lo": float(cl[0]),
                         "lnL_lo": float(lo[b]), "S": float(S[b]), "fwd_rev": float(fr), "c64": float(c64[b]),
                         "c64_status": int(cst[b]), "d_dxmax": dmaxdx(kinds, kernel, t), "tags": tags[b]})
        doc["groups"].append({"name": name, "regime": regime, "kinds": kinds, "lightcurve": rec, "mean_kind": mean_kind,
                              "sha256": sha(t, y, dy), "y_offset": [float(v) for v in means], "rows": rows})
        print("%-28s N=%-6d rows %d/%d" % (name, N, len(rows), len(thetas)), flush=True)
    if dropped:
        raise SystemExit("%d rows dropped: change the recipe" % dropped)
    with open(os.path.join(HERE, "quad_golden.json"), "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
