#!/usr/bin/env python3
"""Generates tests/golden/posterior_sims_golden.npz: what GPModelling.generate_from_posteriors(nsims=4) -- the default,
Timmer & Koenig route -- returned under np.random.seed(5) at the commit BEFORE the method= keyword existed, for the
light curve, kernel and posterior samples of case() below.  tests/test_gp_draw_gpu.py holds the default route of every
later commit to these arrays bit for bit (the TK95 route is reproducible for a seed: Philox counters on the device, the
host's draws from numpy's seeded generator).

Needs an MI355X and uses nothing newer than that commit's API.  Run from the root of a checkout of that commit
(3d94ba1, "Predict at new times in linear time on the device"), with this file copied into it:
    python tests/golden/make_posterior_sims_golden.py
and commit the resulting file here.  A few seconds.
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

NSIMS, SEED = 4, 5


def case():
    """(GPModelling with 64 posterior samples, its light curve): 300 epochs one day apart with exposures of 0.2 d,
    DRW + Lorentzian"""
    from mind_the_gaps_amd.gpmodelling import GPModelling
    from mind_the_gaps_amd.lightcurves import GappyLightcurve
    from mind_the_gaps_amd.models import DampedRandomWalk, Lorentzian
    rng = np.random.default_rng(20250712)
    kernel = DampedRandomWalk(1.0, -1.0, bounds=[(-5.0, 5.0), (-5.0, 5.0)]) + \
        Lorentzian(0.5, 1.0, -0.5, bounds=[(-5.0, 5.0), (-2.0, 4.0), (-4.0, 2.0)])
    times = np.arange(300) * 1.0 + 0.5
    lc = GappyLightcurve(times, 50.0 + rng.standard_normal(300), rng.uniform(0.2, 0.5, 300), exposures=0.2)
    model = GPModelling(lc, kernel)
    P = len(model.gp.get_parameter_vector())
    model._mcmc_samples = model.gp.get_parameter_vector()[None, :] + 0.01 * rng.standard_normal((64, P))
    return model, lc


def default_route(model):
    """y [NSIMS][N], dy [NSIMS][N] of generate_from_posteriors(nsims=NSIMS) under np.random.seed(SEED)"""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        np.random.seed(SEED)
        sims = model.generate_from_posteriors(nsims=NSIMS)
    return np.array([s.y for s in sims]), np.array([s.dy for s in sims])


def main():
    model, lc = case()
    y, dy = default_route(model)
    y2, dy2 = default_route(model)
    assert np.array_equal(y, y2) and np.array_equal(dy, dy2), "the default route is not reproducible for a seed"
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "posterior_sims_golden.npz")
    np.savez(out, y=y, dy=dy, times=lc.times, samples=model._mcmc_samples)
    print("wrote %s: y %s, dy %s" % (out, y.shape, dy.shape))


if __name__ == "__main__":
    main()
