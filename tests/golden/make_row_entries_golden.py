#!/usr/bin/env python3
"""Generates tests/golden/row_entries_golden.npz: what the per-row entries of the C-ABI -- Engine.predict, predict_at,
gp_draw and apply_inverse -- returned at the commit BEFORE their host prologue (index check, reserves, uploads,
prepare, argument head) and the pivot step of their kernels were each written once (3bcea26, "Draw light curves from
the GP on the device").  tests/test_row_entries_golden_gpu.py holds every later commit to these arrays bit for bit.

The shapes are the smallest that reach every branch of those entries: L = 2 light curves of N = 131 samples (past two
checkpoints of 64 of the new-time prediction and past four tiles of 32 of the draw, each with a ragged tail), once
with times of their own per light curve and once with shared times; a rank-3 model with a linear mean whose rows have
an SHO term on either side of Q = 1/2 and one row outside the prior, a white model (rank 0) and five complex terms
(rank 10, the last compiled rank).  Inputs are regenerated from seeded numpy generators; only results are stored.

Needs an MI355X and uses nothing newer than that commit's API.  Run from the root of a checkout of that commit, with
this file copied into it:
    python tests/golden/make_row_entries_golden.py
and commit the resulting file here.  A few seconds.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

L, N = 2, 131
SEED, STREAM_BASE = 12345, 1000
FIXTURES = ("per_lc_times", "shared_times")
MODELS = ("real+sho+jitter+line", "jitter", "5complex3")


def lightcurves(fixture):
    """(t [L][N] or [N], y [L][N], dy [L][N]): irregular sampling, about one sample per day"""
    rng = np.random.default_rng(20251017)
    t = 100.0 + np.cumsum(rng.uniform(0.3, 1.7, (L, N)), axis=1)
    y = 10.0 + rng.standard_normal((L, N))
    dy = rng.uniform(0.1, 0.3, (L, N))
    return (t if fixture == "per_lc_times" else t[0].copy()), y, dy


def new_times(fixture):
    """M = 7 unsorted times: before the first sample, after the last one, a sample time (of light curve 0) and a
    duplicate among them"""
    t = lightcurves(fixture)[0]
    t0 = t[0] if t.ndim == 2 else t
    return np.array([150.3, t0[0] - 1.3, t0[40], 197.7, 150.3, t0[-1] + 2.1, 112.9])


def model(name):
    """(kinds, full, free, bounds, mean_kind, theta [B][P], lc [B])"""
    from mind_the_gaps_amd import engine as E
    if name == "real+sho+jitter+line":
        kinds = [E.TERM_REAL, E.TERM_SHO, E.TERM_JITTER]
        # log a, log c | log S0, log Q, log w0 | log sigma | slope, intercept
        base = np.array([-0.5, -1.5, 0.2, np.log(2.0), np.log(0.8), -2.0, 1.0e-3, -0.1])
        theta = np.tile(base, (5, 1)) + 0.05 * np.random.default_rng(1).uniform(-1.0, 1.0, (5, len(base)))
        theta[2, 3] = np.log(0.3)        # over-damped: this row's SHO term expands to two real terms
        theta[3, 0] = 11.0               # outside the prior
        bounds = np.vstack([np.tile([-10.0, 10.0], (6, 1)), np.tile([-np.inf, np.inf], (2, 1))])
        return kinds, base, np.arange(8, dtype=np.int32), bounds, E.MEAN_LINEAR, theta, np.array([1, 0, 1, 0, 1], dtype=np.int32)
    if name == "jitter":
        theta = np.array([[-0.3], [0.1]])
        return ([E.TERM_JITTER], np.array([-0.3, 0.0]), np.array([0], dtype=np.int32), np.tile([-np.inf, np.inf], (2, 1)),
                E.MEAN_CONSTANT, theta, np.array([0, 1], dtype=np.int32))
    # five complex terms (log a, log c, log d each), periods from 3 to 40 days
    base = np.concatenate([[-1.0 - 0.2 * k, -2.0 - 0.1 * k, np.log(2.0 * np.pi / p)] for k, p in enumerate((3.0, 5.5, 9.0, 17.0, 40.0))])
    theta = np.tile(base, (2, 1)) + 0.05 * np.random.default_rng(2).uniform(-1.0, 1.0, (2, len(base)))
    P = len(base)
    return ([E.TERM_COMPLEX3] * 5, np.concatenate([base, [0.0]]), np.arange(P, dtype=np.int32),
            np.tile([-np.inf, np.inf], (P + 1, 1)), E.MEAN_CONSTANT, theta, np.array([1, 0], dtype=np.int32))


def run(engine, fixture, name):
    """every call of the case -> {key: array}"""
    t, y, dy = lightcurves(fixture)
    kinds, full, free, bounds, mean_kind, theta, lc = model(name)
    engine.set_lightcurves(t, y, dy + 1e-12, y_offset=None if mean_kind else y.mean(axis=1))
    engine.set_model(kinds, full, free, bounds, mean_kind=mean_kind)
    B = len(theta)
    out = {}

    def keep(call, names, values):
        for n, v in zip(names, values):
            if v is not None:
                out["%s/%s/%s/%s" % (fixture, name, call, n)] = np.asarray(v)

    keep("predict", ("mu", "var", "status"), engine.predict(theta, lc))
    ts = new_times(fixture)
    keep("predict_at", ("mu", "var", "status"), engine.predict_at(theta, ts, lc))
    keep("predict_at_mean_only", ("mu", "var", "status"), engine.predict_at(theta, ts, lc, return_var=False))
    keep("predict_at_sorted", ("mu", "var", "status"), engine.predict_at(theta, np.sort(ts), lc))
    q = np.random.default_rng(3).standard_normal((B, N))
    keep("gp_draw_given", ("y", "status"), engine.gp_draw(theta, lc, normals=q))
    engine.set_stream_base(STREAM_BASE)
    try:
        keep("gp_draw_philox", ("y", "status"), engine.gp_draw(theta, lc, seed=SEED))
    finally:
        engine.set_stream_base(0)
    if name == MODELS[0]:
        rhs = np.random.default_rng(4).standard_normal((N, 3))
        x, status = engine.apply_inverse(theta[0], rhs, lc_index=1)
        keep("apply_inverse", ("x", "status"), (x, np.int32(status)))
    return out


def main():
    from mind_the_gaps_amd.engine import Engine
    engine = Engine(0)
    arr = {}
    for fixture in FIXTURES:
        for name in MODELS:
            got = run(engine, fixture, name)
            again = run(engine, fixture, name)
            assert all(np.array_equal(got[k], again[k], equal_nan=True) for k in got), "not reproducible: %s %s" % (fixture, name)
            arr.update(got)
    engine.close()
    a = "%s/%s/" % (FIXTURES[0], MODELS[0])
    assert list(arr[a + "predict/status"]) == [0, 0, 0, 1, 0] and np.all(np.isnan(arr[a + "gp_draw_given/y"][3]))
    assert all(np.all(v == 0) for k, v in arr.items() if k.endswith("status") and MODELS[0] not in k)
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "row_entries_golden.npz")
    np.savez_compressed(out, **arr)
    print("wrote %s: %d arrays, %d bytes" % (out, len(arr), os.path.getsize(out)))


if __name__ == "__main__":
    main()
