#!/usr/bin/env python3
"""Generates tests/golden/tp_fallback_golden.json: rows on both sides of the time-parallel kernels' per-row decision
(`good` in mtg_timeparallel.h, its twin in mtg_tp_scan.hip) with their quad-precision truth (oracle/celerite_quad.c),
for tests/test_tp_fallback_gpu.py and tests/test_tp_fallback_cpu.py.

Every group is one model on one pair of light curves (recipe "quiet_spike" of golden_util.quad_lightcurve: the scatter
of y and the errors are ~0.15, so that ln 2 pi D_n is negative where the model fits; light curve 1 equals light curve
0 but for one interior sample y = 1e160).  Light curves are not stored: the recipe and the SHA-256 of t, y, dy are.
Three classes of rows, each checked here and the checks recorded:

* healthy      light curve 0; every other row theta 25 % around the tutorial values (make_quad_golden.py's `around`:
               S / |T| ~ 1), the others with amplitudes at the light curve's scatter and one parameter bisected to
               lnL = -N / 2 (S / |T| 3 to 4: kept, yet the scan's and the filter's sums differ in their last bits).  The
               float64 oracle gives status 0 and S / |T| <= 10: the scanned likelihood is kept.
* cancelling   the amplitudes brought down to the light curve's scatter, then ONE parameter bisected in the quad oracle
               until |T| <= 1e-6 S (T the quad lnL, S the row's error scale): the positive and negative halves of the
               sum cancel, the kernels' guard (magnitudes <= 1e3 |lnL|) fails by three orders of magnitude and the row
               is redone by the filter pass whatever its last bits are.  The float64 oracle gives status 0.
* nonfinite    the healthy thetas on light curve 1: the squared residual of the 1e160 sample overflows, the float64
               oracle returns -inf with status 3 as celerite does.

Per status-0 row: the full parameter vector (the frozen mean last), the quad lnL as a double pair, S, the forward /
reversed disagreement of the quad sweep, celerite's float64 value (oracle_logprob_batch).  A row that fails a check
stops the run: the recipe is changed, the row is never kept.

Run from the repo root:  python tests/golden/make_tp_fallback_golden.py   (~3 minutes on 8 cores; deterministic)
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
from make_quad_golden import CONFIG5, around, priors_ok  # noqa: E402

K = synth
U = 2.0 ** -53
SPIKE = 1.0e160
J3, J4, NULL, ALT, FIVE = [K.K_DRW, K.K_LORENTZIAN], [K.K_BPL, K.K_MATERN32], K.NULL_MODEL, K.ALT_MODEL, [K.K_SHO] * 5
# (model, N, healthy rows, cancelling rows, columns of SHO quality factors put below 1/2 in every other row)
GROUPS = [("j3", J3, N, 12, 24, []) for N in (70, 1000, 4096, 4097)]
GROUPS += [("j4", J4, N, 12, 24, []) for N in (70, 1000, 4096, 4097)]
GROUPS += [("null", NULL, N, 12, 24, [3]) for N in (1000, 4096)]
GROUPS += [("alt", ALT, 4096, 12, 24, [3])]
GROUPS += [("5sho", FIVE, 1024, 12, 33, [4, 10]), ("5sho", FIVE, 8192, 12, 33, [])]


def recipe(N):
    return dict(N=N, L=1, seed=300 + N, offset=0.0, edit="quiet_spike", scale=0.15, spike=N // 2, spike_value=SPIKE)


def draw(kinds, B, seed, overdamp):
    """B rows 25 % around the tutorial values that pass the model's own prior; every other row over-damped"""
    if kinds == FIVE:
        rng = np.random.default_rng(seed)
        th = CONFIG5 + 0.25 * np.abs(CONFIG5) * rng.uniform(-1, 1, (4 * B, 15))
    else:
        th = around(kinds, 4 * B, seed)
    th = np.array([r for r in th if priors_ok(kinds, r)][:B])
    assert len(th) == B
    for col in overdamp:
        th[::2, col] = np.log(0.3)
    return th


def quieten(kinds, th, rng):
    """The amplitudes of every term but the first brought down to a variance of ~0.003 (x 0.5 .. 2); returns the index
    of the parameter that is bisected (the first term's amplitude; BPL + Matern32: the Matern32 sigma, so that the
    BPL's a >= b, its prior, is kept by moving both together)."""
    th = th.copy()
    off, first = 0, True
    for k in kinds:
        var = 0.003 * 2.0 ** rng.uniform(-1.0, 1.0)
        if k == K.K_BPL:
            th[off + 1] += np.log(var) - th[off]
            th[off] = np.log(var)
        elif not first:
            if k == K.K_SHO:       # variance S0 w0 Q
                th[off] = np.log(var) - th[off + 1] - th[off + 2]
            elif k == K.K_MATERN32:
                th[off] = 0.5 * np.log(var)
            else:
                th[off] = np.log(var)
        off += synth.NPARAMS[k]
        first = False
    return th, (synth.NPARAMS[K.K_BPL] if kinds[0] == K.K_BPL else 0)


def bisect_to(t, y, dy, kinds, full, idx, target=0.0):
    """full[:, idx] moved until the quad lnL of every row is ~target: the float64 oracle brackets the root, the quad
    oracle bisects inside the bracket"""
    B = len(full)
    lc = np.zeros(B, dtype=np.int32)
    nt = quad.default_threads()

    def f64(x):
        p = full.copy(); p[:, idx] = x
        v, st = oracle_c.logprob_batch(t, y, dy, kinds, p, lc_index=lc, nthreads=nt)
        assert np.all(st == 0), st
        return v - target

    def fq(x):
        p = full.copy(); p[:, idx] = x
        hi, lo, _, st = quad.loglike(t, y, dy, kinds, p, lc_index=lc)
        assert np.all(st == 0), st
        return (hi - target) + lo

    lo, hi = np.full(B, -25.0), np.full(B, np.log(1.0e3))
    assert np.all(f64(lo) > 0.0) and np.all(f64(hi) < 0.0), "no sign change: change the recipe"
    for _ in range(48):
        mid = 0.5 * (lo + hi)
        pos = f64(mid) > 0.0
        lo, hi = np.where(pos, mid, lo), np.where(pos, hi, mid)
    x = 0.5 * (lo + hi)
    lo, hi = x - 1.0e-7, x + 1.0e-7
    assert np.all(fq(lo) > 0.0) and np.all(fq(hi) < 0.0), "the quad root is not within 1e-7 of the float64 one"
    for _ in range(20):
        mid = 0.5 * (lo + hi)
        pos = fq(mid) > 0.0
        lo, hi = np.where(pos, mid, lo), np.where(pos, hi, mid)
    out = full.copy()
    out[:, idx] = 0.5 * (lo + hi)
    return out


def truth_rows(name, cls, t, y, dy, kinds, full, N):
    """quad truth, float64 oracle and the forward / reversed check of make_quad_golden.py for status-0 rows on lc 0"""
    B = len(full)
    lc = np.zeros(B, dtype=np.int32)
    hi, lo, S, st = quad.loglike(t, y, dy, kinds, full, lc_index=lc)
    rhi, rlo, _, rst = quad.loglike(t, y, dy, kinds, full, lc_index=lc, reverse=True)
    c64, cst = oracle_c.logprob_batch(t, y, dy, kinds, full, lc_index=lc, nthreads=quad.default_threads())
    rows = []
    for b in range(B):
        assert cst[b] == 0 and st[b] == 0 and rst[b] == 0, (name, cls, b, cst[b], st[b], rst[b])
        fr = abs((hi[b] - rhi[b]) + (lo[b] - rlo[b]))
        tol = max(10.0 * abs((c64[b] - hi[b]) - lo[b]), 64.0 * np.sqrt(N) * U * S[b])
        assert fr < 1e-3 * tol, (name, cls, b, fr, tol)
        T = abs(hi[b] + lo[b])
        if cls == "healthy":
            assert S[b] <= 10.0 * T, (name, b, S[b], T)
        else:
            assert T <= 1.0e-6 * S[b], (name, b, S[b], T)
        rows.append({"cls": cls, "theta": [float(v) for v in full[b]], "lc": 0, "lnL": float(hi[b]),
                     "lnL_lo": float(lo[b]), "S": float(S[b]), "fwd_rev": float(fr), "c64": float(c64[b]),
                     "c64_status": int(cst[b]), "T_over_S": float(T / S[b])})
    return rows


def main():
    doc = {"generator": "tests/golden/make_tp_fallback_golden.py", "u": U,
           "truth": "oracle/celerite_quad.c (coefficients built from theta in quad); c64: oracle_logprob_batch",
           "checks": {"healthy": "c64_status 0, S <= 10 |T|", "cancelling": "c64_status 0, |T| <= 1e-6 S",
                      "nonfinite": "c64_status 3 and -inf on light curve 1 (one sample 1e160)",
                      "all status-0 rows": "forward and reversed quad sweeps agree to 1e-3 of the row's tolerance"},
           "groups": []}
    for model, kinds, N, nh, ncan, overdamp in GROUPS:
        name = "%s/n%d" % (model, N)
        rec = recipe(N)
        t, y, dy = lightcurve(rec)
        assert y.shape == (2, N) and np.sum(y[0] != y[1]) == 1 and np.array_equal(dy[0], dy[1])
        mean = float(y[0].mean())
        seed = 1000 * len(kinds) + N
        rng = np.random.default_rng(seed + 1)
        # half of the healthy rows as the quad fixture draws them: lnL is all log-determinant on this quiet light curve,
        # which the scan and the filter both get to the last bit; the other half with amplitudes at the light curve's
        # scatter and lnL = -N / 2, where S / |T| is 3 to 4: kept (magnitudes ~|lnL|), but with enough cancellation that
        # the scan's and the filter's sums differ in their last bits
        fit = [quieten(kinds, r, rng) for r in draw(kinds, nh - nh // 2, seed + 3, overdamp)]
        fit = bisect_to(t, y, dy, kinds, np.hstack([np.array([q[0] for q in fit]), np.full((len(fit), 1), mean)]),
                        fit[0][1], target=-0.5 * N)
        healthy = np.vstack([np.hstack([draw(kinds, nh // 2, seed, overdamp), np.full((nh // 2, 1), mean)]), fit])
        healthy = healthy[np.arange(nh).reshape(2, -1).T.ravel()]     # interleaved
        base = draw(kinds, ncan, seed + 2, overdamp)
        quiet = [quieten(kinds, r, rng) for r in base]
        idx = quiet[0][1]
        cancel = bisect_to(t, y, dy, kinds, np.hstack([np.array([q[0] for q in quiet]), np.full((ncan, 1), mean)]),
                                idx)
        for r in list(cancel) + list(healthy):
            assert priors_ok(kinds, r[:-1])
        rows = truth_rows(name, "healthy", t, y, dy, kinds, healthy, N)
        rows += truth_rows(name, "cancelling", t, y, dy, kinds, cancel, N)
        c64, cst = oracle_c.logprob_batch(t, y, dy, kinds, healthy, lc_index=np.ones(nh, dtype=np.int32))
        for b in range(nh):
            assert cst[b] == 3 and c64[b] == -np.inf, (name, b, cst[b], c64[b])
            rows.append({"cls": "nonfinite", "theta": [float(v) for v in healthy[b]], "lc": 1, "c64_status": int(cst[b])})
        doc["groups"].append({"name": name, "kinds": [int(k) for k in kinds], "lightcurve": rec, "sha256": sha(t, y, dy),
                              "y_offset": [mean, mean], "bisected": int(idx), "rows": rows})
        worst = max(r["T_over_S"] for r in rows if r["cls"] == "cancelling")
        print("%-12s rows %d  worst cancelling |T|/S %.2e  worst healthy S/|T| %.2f" % (
            name, len(rows), worst, 1.0 / min(r["T_over_S"] for r in rows if r["cls"] == "healthy")), flush=True)
    with open(os.path.join(HERE, "tp_fallback_golden.json"), "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
