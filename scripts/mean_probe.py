"""Writes profiles/mean_probe.txt: what the sweep under the profile means (csrc/mtg_kernels_mean.hip) takes and costs.

    make -C mind_the_gaps_amd/csrc HIPFLAGS="<the Makefile's> -Rpass-analysis=kernel-resource-usage" 2> remarks.log
    python scripts/mean_probe.py --resources remarks.log [--out profiles/mean_probe.txt]

Resources: VGPRs, AGPRs, scratch, occupancy and LDS of every new instantiation from the compiler's remarks, and of the
plain sweep's instantiations that use scratch, for comparison.  Timings (needs the GPU): the headline shape (N = 1e4,
DRW + SHO + Lorentzian, 2000 light curves x 256 rows in their own sorted order) and 250 x 128; per shape and mean kind
3 warm-up calls, then the median and the spread of 10 timed calls of mtg_loglike_batch_device's solver launches (HIP
events around them: Engine.last_kernel_ms), time-parallel and pipelined forms off so that the linear mean runs the
one-lane sweep too; then each kind's ratio to the linear mean."""
import argparse
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mind_the_gaps_amd import engine as _engine, synthetic as synth

MEANS = {"linear": (_engine.MEAN_LINEAR, [0.0, 0.0]), "sine": (_engine.MEAN_SINE, [0.0, 0.5, 0.37, 0.7]),
         "two sines": (_engine.MEAN_TWOSINE, [0.0, 0.5, 0.7, 0.2, -1.1, 0.37]), "gaussian": (_engine.MEAN_GAUSSIAN, [5000.0, 300.0, 900.0, 0.0])}


KINDS = {"2": "sine", "3": "two sines", "4": "gaussian"}


def resources(log):
    """the remarks of a build as table lines: the mean kernels, and the plain sweeps that spill"""
    rows, plain = [], []
    for block in re.split(r"remark: Function Name: ", open(log).read())[1:]:
        name = block.split()[0]

        def field(key):
            m = re.search(key + r": (\d+)", block)
            return int(m.group(1)) if m else -1
        v = (field("VGPRs"), field("AGPRs"), field(r"ScratchSize \[bytes/lane\]"), field(r"Occupancy \[waves/SIMD\]"),
             field(r"LDS Size \[bytes/block\]"))
        m = re.search(r"mtg_solve_mean_kernelILi(\d+)ELi(\d+)ELi(\d+)E14MtgMeanProfileILi(\d)", name)
        w = re.search(r"mtg_white_mean_kernelI14MtgMeanProfileILi(\d)", name)
        q = re.search(r"Z16mtg_solve_kernelILi(\d+)ELi(\d+)ELi(\d+)EEv", name)
        if m:
            nr, nc, b0, k = (int(g) for g in m.groups())
            rows.append((KINDS[str(k)], nr + 2 * nc, nr, nc, b0) + v)
        elif w:
            rows.append((KINDS[w.group(1)], 0, 0, 0, 0) + v)
        elif q and v[2] > 0:
            nr, nc, b0 = (int(g) for g in q.groups())
            plain.append(("linear", nr + 2 * nc, nr, nc, b0) + v)
    fmt = "%-9s %2d  %2d %2d %2d  %5d %5d %15d %21d %6d"
    out = ["mean       J  NR NC B0  VGPRs AGPRs scratch[B/lane] occupancy[waves/SIMD] LDS[B]"]
    out += [fmt % r for r in sorted(set(rows))]
    spill = [r for r in rows if r[1] <= 6 and r[7] > 0]
    out += ["", "new instantiations: %d; of rank <= 6 with scratch: %d" % (len(set(rows)), len(spill)), "",
            "the plain sweep's instantiations (mtg_solve_kernel<NR,NC,B0>) that use scratch, same build:"]
    out += [fmt % r for r in sorted(set(plain))]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "mean_probe.txt"))
    ap.add_argument("--resources", default=None, help="compiler output of a build with -Rpass-analysis=kernel-resource-usage")
    args = ap.parse_args()
    import torch
    lines = ["scripts/mean_probe.py", ""]
    if args.resources:
        lines += resources(args.resources) + [""]
    lines += ["timings (ms, solver launches only; one-lane sweep for every mean, time-parallel and pipelined forms off)"]
    eng = _engine.Engine(0)
    eng.set_time_parallel(0)
    eng.set_pipeline(0)
    kinds = synth.ALT_MODEL
    for L, W in ((2000, 256), (250, 128)):
        N = 10000
        t, y, dy = synth.make_lightcurves(N, L, seed=1)
        y = y - y.mean(axis=1, keepdims=True)
        eng.set_lightcurves(t, y, dy + 1e-12)
        kth = synth.draw_thetas(kinds, L * W, seed=2)
        lc = np.repeat(np.arange(L, dtype=np.int32), W)
        ms = {}
        for name, (kind, mean) in MEANS.items():
            full = np.concatenate([kth[0], mean])
            P = len(full)
            eng.set_model(kinds, full, np.arange(P, dtype=np.int32), np.tile([-np.inf, np.inf], (P, 1)), mean_kind=kind)
            theta = torch.as_tensor(np.hstack([kth, np.tile(mean, (L * W, 1))]), device="cuda")
            lcd = torch.as_tensor(lc, device="cuda")
            out = torch.empty(L * W, dtype=torch.float64, device="cuda")
            st = torch.empty(L * W, dtype=torch.int32, device="cuda")
            times = []
            for it in range(13):
                eng.loglike_device(L * W, theta.data_ptr(), lcd.data_ptr(), out.data_ptr(), st.data_ptr(), add_prior=False)
                eng.synchronize()
                if it >= 3:
                    times.append(eng.last_kernel_ms)
            assert int((st != 0).sum()) == 0, "%s: rows with a status" % name
            ms[name] = float(np.median(times))
            lines.append("%4d x %3d  %-10s %-36s median %8.3f ms  (min %.3f, max %.3f, 10 calls)" % (
                L, W, name, eng.last_solver, ms[name], min(times), max(times)))
        for name in ("sine", "two sines", "gaussian"):
            lines.append("%4d x %3d  %-10s / linear = %.3f" % (L, W, name, ms[name] / ms["linear"]))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    open(args.out, "w").write(text)


if __name__ == "__main__":
    main()
