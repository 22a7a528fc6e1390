"""Cost of the conditional draw (Engine.gp_cond_draw) beside the two entries it is made of, on the same shapes from the
same build: Engine.predict_at with return_var=False (the mean-only form the conditional draw runs) and Engine.gp_draw.
256 draws at N = 1e4, M = 1e4 and one draw at N = 2e5, M = 1e6, the rank-5 alternative model, device normals.

Times are those of the whole call as the host sees it -- uploads, kernels, the copy of the result back -- not kernel times,
the best of three after one warm-up call.  The calls copy back different volumes: gp_cond_draw and the mean-only
predict_at B M doubles each, gp_draw B N; the baseline therefore copies B (M + N) doubles where the new entry copies
B M.  Writes profiles/gp_cond_draw_probe.txt.

    python scripts/gp_cond_draw_probe.py"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mind_the_gaps_amd import synthetic as synth  # noqa: E402
from mind_the_gaps_amd.engine import Engine  # noqa: E402


def best_of(call, n=3):
    call()
    out = []
    for _ in range(n):
        t0 = time.perf_counter()
        call()
        out.append(time.perf_counter() - t0)
    return min(out)


def main():
    kinds = synth.ALT_MODEL
    theta = synth.truth(kinds)
    P = len(theta)
    eng = Engine(0)
    lines = ["conditional draw beside mean-only predict_at + gp_draw: whole-call times in ms (copies included: cond_draw and",
             "predict_at return B M doubles each, gp_draw B N), best of 3 (scripts/gp_cond_draw_probe.py)",
             "%8s %8s %5s %12s %12s %12s %8s" % ("N", "M", "B", "cond_draw", "pat_mean", "gp_draw", "ratio")]
    for N, M, B in ((10000, 10000, 256), (200000, 1000000, 1)):
        t, y, dy = synth.make_lightcurves(N, 1, seed=N)
        eng.set_lightcurves(t, y, dy + 1e-12, y_offset=y.mean(axis=1))
        eng.set_model(kinds, np.concatenate([theta, [0.0]]), np.arange(P, dtype=np.int32), np.tile([-np.inf, np.inf], (P + 1, 1)))
        ts = np.sort(np.random.default_rng(M).uniform(t[0] - 10.0, t[-1] + 10.0, M))
        th = np.tile(theta, (B, 1))
        cond = best_of(lambda: eng.gp_cond_draw(th, ts, seed=1))
        assert eng.last_solver == "mtg_gp_cond_draw_kernel<5>", eng.last_solver
        pat = best_of(lambda: eng.predict_at(th, ts, return_var=False))
        draw = best_of(lambda: eng.gp_draw(th, seed=1))
        lines.append("%8d %8d %5d %12.2f %12.2f %12.2f %8.2f" % (N, M, B, 1e3 * cond, 1e3 * pat, 1e3 * draw, cond / (pat + draw)))
        print(lines[-1], flush=True)
    eng.close()
    with open(os.path.join(ROOT, "profiles", "gp_cond_draw_probe.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
