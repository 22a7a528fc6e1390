#!/usr/bin/env python3
"""Generates tests/golden/sweep_golden.npz: lnL (float64) and status (int32) of Engine.loglike from the serial sweep --
the one-lane kernels (mtg_solve_kernel, mtg_solve_kernel_multi, mtg_white_kernel) and their two-wave pipeline
(mtg_pipe_kernel) -- at the commit BEFORE their sample loads and their epilogue were
written once (237d629, "Share one row-batch prologue and pivot step across the GP entries").
tests/test_sweep_golden_gpu.py holds every later commit to these arrays bit for bit.

The shapes are the smallest that reach every branch of the shared code.  N in {1, 2, 3, 64, 65, 70, 257, 261}: odd N
takes the tail step of the one-lane loop; 64 is the pipeline's shortest light curve, and lengths on either side of a
whole number of chunks of 4 and of trips of 12 samples take the consumer's remainder loop with every count of samples
left, the renormalisation of an odd last sample included.  130 rows: two workgroups of the pipeline, the second with
two live rows; three waves of the one-lane kernel.  Models: DRW (rank 1, no pipeline); DRW + SHO with rows on both
sides of Q = 1/2 (two structures in one launch); DRW + SHO + Lorentzian (the last complex term with b = 0); the same
with a JitterTerm, a fitted linear mean and times per light curve (the MEAN variants); ComplexTerm + DRW on times with
a gap that takes one row's phase step out of the table sincos' range (the libm variants of sweep and producer);
JitterTerm alone (the white kernel); RealTerm + four-parameter ComplexTerm with rows whose b is too large for a
positive definite covariance (without the prior, which forbids them).  Rows outside the prior box in every other model
with a box.  Each case once with the pipeline off and once with it forced, the time-parallel kernels off, the sort at
its default.
Inputs are regenerated from seeded numpy generators; only results are stored.

Needs an MI355X and uses nothing newer than that commit's API.  Run from the root of a checkout of that commit, with
this file copied into it:
    python tests/golden/make_sweep_golden.py
and commit the resulting file here.  A few seconds.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

LENGTHS = (1, 2, 3, 64, 65, 70, 257, 261)
B, L = 130, 3
MODELS = ("drw", "drw_sho", "drw_sho_lorentzian", "drw_sho_lorentzian_jitter_line", "complex3_drw_wide_phase", "jitter",
          "real_complex4_notpd")
PIPED = MODELS[1:5] + MODELS[6:]                    # the models mtg_kernels_pipe.hip is compiled for
DISPATCH = (("one_lane", 0), ("pipeline", 1))       # name, mtg_set_pipeline mode
WIDE_ROW, NOTPD_ROWS = 70, (5, 69, 128)


def case(name, N):
    """(t, y, dy, y_offset, kinds, full, free, bounds, mean_kind, theta [B][P], lc [B], add_prior)"""
    from mind_the_gaps_amd import engine as E
    from mind_the_gaps_amd import synthetic as S
    rng = np.random.default_rng(1000 * MODELS.index(name) + N)
    t, y, dy = S.make_lightcurves(N, L, seed=77 + N)
    lc = rng.integers(0, L, B).astype(np.int32)
    if name == "complex3_drw_wide_phase":
        t = np.cumsum(rng.exponential(0.5, N))
        t[N // 2:] += 2.0e8 if N > 1 else 0.0
        y, dy = rng.standard_normal((L, N)), rng.uniform(0.2, 0.5, (L, N))
        kinds = [S.K_COMPLEX3, S.K_DRW]
        base = np.array([np.log(2.0), np.log(0.3), np.log(3.0), np.log(1.5), np.log(0.2)])
        theta = base + 0.01 * rng.standard_normal((B, 5))
        theta[WIDE_ROW, 2] = np.log(9000.0)         # d dx = 1.8e12 in the second group of 64 rows
        return (t, y, dy, None, kinds, np.concatenate([base, [0.0]]), np.arange(5, dtype=np.int32),
                np.tile([-np.inf, np.inf], (6, 1)), E.MEAN_CONSTANT, theta, lc, False)
    if name == "drw_sho_lorentzian_jitter_line":
        kinds = S.ALT_MODEL + [S.K_JITTER]
        t = np.cumsum(0.05 + rng.exponential(1.0, (L, N)), axis=1)
        full, free, bounds = S.model_spec(kinds, y, mean_kind=E.MEAN_LINEAR, fit_mean=True)
        theta = np.tile(full, (B, 1)) + 0.05 * rng.standard_normal((B, len(full)))
        theta[:, -2] = 1e-3 * rng.standard_normal(B)             # slope
        theta[::4, 3] = np.log(0.2)                              # over-damped rows
        theta[::43, 0] = 60.0                                    # outside the prior box
        return t, y, dy, None, kinds, full, free, bounds, E.MEAN_LINEAR, theta, lc, True
    kinds = {"drw": [S.K_DRW], "drw_sho": S.NULL_MODEL, "drw_sho_lorentzian": S.ALT_MODEL, "jitter": [S.K_JITTER],
             "real_complex4_notpd": [S.K_REAL, S.K_COMPLEX4]}[name]
    full, free, bounds = S.model_spec(kinds, y, per_lc_mean=True)
    theta = S.draw_thetas(kinds, B, seed=N + 1, percent=0.15)
    if S.K_SHO in kinds:
        theta[::3, 3] = np.log(0.3)                              # over-damped: the SHO term expands to two real terms
    if name == "real_complex4_notpd":
        theta[NOTPD_ROWS, 3] += 8.0                              # log b of the complex term: b >> a c / d
    theta[::43, 0] = 60.0                                        # outside the prior box
    # (the four-parameter ComplexTerm's own prior forbids the b that is not positive definite: that model without prior)
    return t, y, dy, y.mean(axis=1), kinds, full, free, bounds, E.MEAN_CONSTANT, theta, lc, name != "real_complex4_notpd"


def run(engine, name, N):
    """both dispatches of the case -> ({key: array}, {dispatch: kernel name})"""
    t, y, dy, y_offset, kinds, full, free, bounds, mean_kind, theta, lc, add_prior = case(name, N)
    engine.set_lightcurves(t, y, dy + 1e-12, y_offset=y_offset)
    engine.set_model(kinds, full, free, bounds, mean_kind=mean_kind)
    out, solver = {}, {}
    engine.set_time_parallel(0)
    try:
        for dispatch, mode in DISPATCH:
            engine.set_pipeline(mode)
            lnl, status = engine.loglike(theta, lc, add_prior=add_prior)
            out["%s/%d/%s/lnL" % (name, N, dispatch)] = np.asarray(lnl, dtype=np.float64)
            out["%s/%d/%s/status" % (name, N, dispatch)] = np.asarray(status, dtype=np.int32)
            solver[dispatch] = engine.last_solver
    finally:
        engine.set_pipeline(2)
        engine.set_time_parallel(2)
    return out, solver


def dispatch_is_as_meant(name, N, solver):
    """the kernels the case was chosen for really ran"""
    return ("mtg_pipe_kernel" not in solver["one_lane"]
            and ("mtg_white_kernel" in solver["one_lane"]) == (name == "jitter")
            and ("mtg_pipe_kernel" in solver["pipeline"]) == (name in PIPED and N >= 64)
            and ("mtg_solve_kernel_multi" in solver["one_lane"]) == ("sho" in name))


def main():
    from mind_the_gaps_amd.engine import Engine
    engine = Engine(0)
    arr = {}
    for name in MODELS:
        for N in LENGTHS:
            got, solver = run(engine, name, N)
            again, _ = run(engine, name, N)
            assert all(np.array_equal(got[k], again[k]) for k in got), "not reproducible: %s %d" % (name, N)
            assert dispatch_is_as_meant(name, N, solver), (name, N, solver)
            print("%-32s N = %3d  %s | %s  status counts %s" % (name, N, solver["one_lane"], solver["pipeline"],
                  np.bincount(got["%s/%d/one_lane/status" % (name, N)], minlength=4)))
            arr.update(got)
    engine.close()
    for name in MODELS:
        st = arr["%s/261/one_lane/status" % name]
        assert (st == 0).sum() > B // 2, name
        assert (st == 1).sum() == (0 if name in (MODELS[4], MODELS[6]) else 4), name
        assert ((st == 2).sum() > 0) == (name == MODELS[6]), name
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "sweep_golden.npz")
    np.savez_compressed(out, **arr)
    print("wrote %s: %d arrays, %d bytes" % (out, len(arr), os.path.getsize(out)))


if __name__ == "__main__":
    main()
