#!/usr/bin/env python3
"""Times mtg_gp_draw on the headline model (DRW + SHO + Lorentzian) at N = 1e4 for B in {256, 2000, 32000}: the caller's
normals and the device's (Philox), next to mtg_simulate_tk95 for the same B at the workflow's grid (Simulator on the same
epochs, exposures of 0.04 d, extension_factor 2, Gaussian noise; in blocks of 2000 series as the Protassov test cuts
them), mtg_predict for the same B (B <= 2000: its workspace is B N (3 J + 2) doubles) and a device-to-device copy of
B N 8 bytes.  Host clock around the whole C-ABI call (upload of theta and normals,
kernels, download of the draws), warm-up first, the variants interleaved, median of REPEATS.

    python scripts/gp_draw_probe.py            -> profiles/gp_draw_probe.txt
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mind_the_gaps_amd import synthetic as synth  # noqa: E402
from mind_the_gaps_amd import terms  # noqa: E402
from mind_the_gaps_amd.engine import Engine  # noqa: E402
from mind_the_gaps_amd.models import DampedRandomWalk, Lorentzian  # noqa: E402
from mind_the_gaps_amd.simulator import Simulator  # noqa: E402

REPEATS = 5
N = 10000


def clock(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def main():
    import torch
    kinds = synth.ALT_MODEL
    t, y, dy = synth.make_lightcurves(N, 1, seed=1)
    full, free, bounds = synth.model_spec(kinds, y, per_lc_mean=True)
    eng = Engine(0)
    eng.set_lightcurves(t, y, dy + 1e-12, y_offset=y.mean(axis=1))
    eng.set_model(kinds, full, free, bounds)
    th = synth.truth(kinds)
    amp, other = (-10.0, 50.0), (-10.0, 10.0)
    kernel = DampedRandomWalk(th[0], th[1], bounds=[amp, other]) + terms.SHOTerm(th[2], th[3], th[4], bounds=[amp, other, other]) \
        + Lorentzian(th[5], th[6], th[7], bounds=[amp, other, other])
    sim = Simulator(kernel, t, 0.04, 100.0, "Gaussian", sigma_noise=1.0, extension_factor=2, random_state=3)
    lines = ["gp_draw_probe: headline model %s, N = %d, median of %d interleaved repeats, host clock around the call" % (kinds, N, REPEATS),
             "tk95: Simulator.simulate on a grid of %d points, step %.4g d, blocks of 2000 series" % (sim.fftndatapoints, sim.sim_dt),
             "%8s %14s %14s %14s %14s %14s" % ("B", "draw given s", "draw philox s", "tk95 s", "predict s", "d2d copy s")]
    for B in (256, 2000, 32000):
        theta = synth.draw_thetas(kinds, B, seed=B, percent=0.02)
        q = np.random.default_rng(B).standard_normal((B, N))
        src = torch.empty(B * N, dtype=torch.float64, device="cuda")
        dst = torch.empty_like(src)

        def copy():
            dst.copy_(src)
            torch.cuda.synchronize()

        def tk95():
            for b0 in range(0, B, 2000):
                sim.simulate(theta[b0:b0 + 2000], seed=1, index_base=b0, pair_series=True)

        jobs = {"given": lambda: eng.gp_draw(theta, normals=q), "philox": lambda: eng.gp_draw(theta, seed=1), "tk95": tk95,
                "copy": copy}
        if B <= 2000:
            jobs["predict"] = lambda: eng.predict(theta)
        for fn in jobs.values():
            fn()
        times = {k: [] for k in jobs}
        for _ in range(REPEATS):
            for k, fn in jobs.items():
                times[k].append(clock(fn))
        med = {k: float(np.median(v)) for k, v in times.items()}
        lines.append("%8d %14.4f %14.4f %14.4f %14s %14.6f" % (B, med["given"], med["philox"], med["tk95"],
                                                         "%.4f" % med["predict"] if "predict" in med else "-", med["copy"]))
        del src, dst
    eng.close()
    text = "\n".join(lines) + "\n"
    print(text)
    out = os.path.join(ROOT, "profiles", "gp_draw_probe.txt")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
