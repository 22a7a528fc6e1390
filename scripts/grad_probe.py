#!/usr/bin/env python3
"""Measures the analytic gradient (mtg_loglike_grad) against the forward differences it replaces.

Timing: kernel time (HIP events on the context's stream, mtg_last_kernel_ms; median of REPEATS = 3 calls after a
warm-up) at two shapes.  What is inside each number: for loglike_grad the coefficient-tangent kernel and the tangent
sweep, NOT the expansion theta -> coefficients that precedes them (one launch of B lanes, microseconds); for the
finite-difference batch of P + 1 rows per point through mtg_loglike_batch that expansion AND the solve.  Uploads and
downloads are outside both.  The shapes: 250 light curves x N = 1e4 with the
alternative model (DRW + SHO + Lorentzian, P = 8, one point per light curve) and one light curve at N = 1e6.
Fit quality: the end point's -lnL and the iteration count of GPModelling.fit in both modes at N = 1e6.
Resources (registers and scratch per instantiated rank): profiles/grad_resources.txt, from
hipcc -Rpass-analysis=kernel-resource-usage on csrc/mtg_loglike_grad.hip.

    python scripts/grad_probe.py [out]      -> profiles/grad_probe.txt
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mind_the_gaps_amd import synthetic as synth  # noqa: E402
from mind_the_gaps_amd import terms  # noqa: E402
from mind_the_gaps_amd.engine import Engine  # noqa: E402
from mind_the_gaps_amd.gpmodelling import GPModelling  # noqa: E402
from mind_the_gaps_amd.lightcurves import GappyLightcurve  # noqa: E402
from mind_the_gaps_amd.models import DampedRandomWalk, Lorentzian  # noqa: E402

REPEATS = 3
AMP, OTHER = (-10, 50), (-10, 10)


def median_ms(eng, call):
    call()
    ms = []
    for _ in range(REPEATS):
        call()
        ms.append(eng.last_kernel_ms)
    return float(np.median(ms))


def timing(eng, N, L, lines):
    kinds = synth.ALT_MODEL
    t, y, dy = synth.make_lightcurves(N, L, seed=1)
    full, free, bounds = synth.model_spec(kinds, y, per_lc_mean=True)
    eng.set_lightcurves(t, y, dy + 1e-12, y_offset=y.mean(axis=1))
    eng.set_model(kinds, full, free, bounds)
    P = len(free)
    theta = synth.draw_thetas(kinds, L, seed=2, percent=0.05)
    lc = np.arange(L, dtype=np.int32)
    pts = np.repeat(theta[:, None, :], P + 1, axis=1)
    pts[:, 1:, :] += 1e-8 * np.eye(P)[None]
    lc_fd = np.repeat(lc, P + 1)
    grad_ms = median_ms(eng, lambda: eng.loglike_grad(theta, lc))
    grad_solver = eng.last_solver
    fd_ms = median_ms(eng, lambda: eng.loglike(pts.reshape(-1, P), lc_fd, add_prior=False))
    lines.append("L = %d light curves x N = %d, P = %d: loglike_grad %.3f ms (%s, %d lanes); forward differences %.3f ms "
                 "(%s, %d rows); ratio %.2f" % (L, N, P, grad_ms, grad_solver, L * P, fd_ms, eng.last_solver, L * (P + 1),
                                                grad_ms / fd_ms))


def fit_quality(N, lines):
    t, y, dy = synth.make_lightcurves(N, 1, seed=7)
    th = synth.truth(synth.ALT_MODEL)
    for mode in ("fd", "analytic"):
        k = (DampedRandomWalk(th[0], th[1], bounds=[AMP, OTHER]) + terms.SHOTerm(th[2], th[3], th[4], bounds=[AMP, OTHER, OTHER])
             + Lorentzian(th[5], th[6], th[7], bounds=[AMP, OTHER, OTHER]))
        g = GPModelling(GappyLightcurve(t, y[0], dy[0]), k)
        sol = g.fit(gradient=mode)
        lines.append("fit(gradient=%r) at N = %d: -lnL = %.6f after %d iterations, %d evaluations (%s)"
                     % (mode, N, sol.fun, sol.nit, sol.nfev, sol.message if isinstance(sol.message, str) else sol.message.decode()))


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "grad_probe.txt")
    lines = []

    class Echo(list):
        def append(self, line):
            super().append(line)
            print(line, flush=True)
    lines = Echo()
    eng = Engine(0)
    timing(eng, 10000, 250, lines)
    timing(eng, 1000000, 1, lines)
    eng.close()
    fit_quality(1000000, lines)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
