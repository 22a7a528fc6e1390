#!/usr/bin/env python3
"""The Lomb-Scargle entries' outputs, bit for bit, at the smallest shapes that reach every branch of the tile sweep the
one-term and the K-harmonic kernels share (csrc/mtg_ls_tile.h) -> tests/golden/lomb_scargle_parent_bits.npz, which
tests/test_lomb_scargle_parent_bits_gpu.py holds every later build to.

Only public Engine calls, so that this file runs unchanged on the commit before the sweep was written once (where the
fixture was made; `commit` in the fixture) and on every commit after it.

    N       MTG_LS_CHUNK + 3 = 259 (a full chunk and a ragged one) and the smallest allowed: 4 (K = 1), 2 K + 2
    L       shared sampling 1 (tile 1), 3 (the R = 4 tile of K = 1 and the full tiles, partly filled), 19 (full tiles and a
            ragged last one for every (K, weighted)); sampling of its own per light curve: 3
    F       70 (a 128-wide workgroup with idle lanes), 260 (two 256-wide ones, the second nearly idle)
    K       1, 2, 3, 5, weighted and not; all four normalisations at L = 3, F = 70, the standard one elsewhere
    peaks   with every call; one set whose determinant is not positive at two frequencies (NaN, passed over)
    envelope  L = 19, F = 70, three ranks, valid, exceed and the ratio peaks, K = 1 and K = 3

Every output is stored as its 64-bit pattern, all calls one after the other in `bits` (`names`, `sizes`: whose and how
many).  Run on a GPU:  python3 tests/golden/make_lomb_scargle_parent_bits.py --commit $(git rev-parse HEAD)
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "lomb_scargle_parent_bits.npz")
SEED = 20261020
N_BIG, L_BIG = 259, 19
NTERMS = (1, 2, 3, 5)
NORMS = ("standard", "model", "log", "psd")
INPUTS = ("t", "t_own", "y", "dy", "f70", "f260", "nan_y", "reference", "scale")


def draw_inputs():
    """every call's inputs from SEED: the sets are leading slices of one draw"""
    rng = np.random.default_rng(SEED)
    t = np.sort(rng.uniform(0.0, 40.0, size=N_BIG)) + 100.0
    t_own = np.sort(rng.uniform(0.0, 40.0, size=(3, N_BIG)), axis=-1) + 100.0
    y = rng.standard_normal((L_BIG, N_BIG)) + np.sin(0.9 * t) + 0.5 * np.cos(2.7 * t)
    dy = rng.uniform(0.1, 0.5, size=(L_BIG, N_BIG))
    # (the inputs of test_a_non_positive_determinant_gives_nan_and_the_peak_passes_it_over)
    nan_y = np.random.default_rng(45).standard_normal(8)
    return dict(t=t, t_own=t_own, y=y, dy=dy, f70=np.linspace(0.02, 3.0, 70), f260=np.linspace(0.02, 3.0, 260), nan_y=nan_y,
                reference=rng.uniform(0.01, 0.1, size=70), scale=rng.uniform(0.5, 2.0, size=70))


def bits(*arrays):
    return np.concatenate([np.ascontiguousarray(a).ravel().view(np.uint64) for a in arrays])


def run(eng, inp):
    """-> [(name, uint64 bits)] of every call, in a fixed order"""
    out = []

    def periodogram(name, f, K, weighted, norm="standard"):
        p, peak, at = eng.lomb_scargle(f, normalization=norm, weighted=weighted, power=True, peak=True, nterms=K)
        out.append(("%s/k%d_%s_%s" % (name, K, "w" if weighted else "u", norm), bits(p, peak, at)))

    def resident(L, N, own=False):
        eng.set_lightcurves(inp["t_own"][:, :N] if own else inp["t"][:N], inp["y"][:L, :N], inp["dy"][:L, :N])

    for L, F, own in ((1, 260, False), (3, 70, False), (19, 70, False), (3, 70, True)):
        resident(L, N_BIG, own)
        for K in NTERMS:
            for weighted in (True, False):
                for norm in (NORMS if (L == 3 and not own) else NORMS[:1]):
                    periodogram("%s%d_n%d_f%d" % ("own" if own else "shared", L, N_BIG, F), inp["f%d" % F], K, weighted, norm)
    for K in NTERMS:
        n = 4 if K == 1 else 2 * K + 2
        resident(3, n)
        for weighted in (True, False):
            periodogram("shared3_n%d_f70" % n, inp["f70"], K, weighted)
    eng.set_lightcurves(np.arange(8.0), inp["nan_y"], np.ones(8))
    for K in (1, 2, 3):
        periodogram("nan_n8_f4", np.array([0.3, 0.5, 1.0, 0.2]), K, False)
    resident(L_BIG, N_BIG)
    for K in (1, 3):
        env = eng.lomb_scargle_envelope(inp["f70"], ranks=(0, 9, 18), reference=inp["reference"], scale=inp["scale"], nterms=K)
        out.append(("envelope19_n%d_f70/k%d_w_standard" % (N_BIG, K), bits(*env)))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--commit", required=True, help="the commit the library was built from")
    ap.add_argument("--out", default=FIXTURE)
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from mind_the_gaps_amd.engine import Engine
    inp = draw_inputs()
    eng = Engine(0)
    calls = run(eng, inp)
    eng.close()
    np.savez_compressed(args.out, commit=np.array(args.commit), names=np.array([n for n, _ in calls]),
                        sizes=np.array([len(b) for _, b in calls], dtype=np.int64), bits=np.concatenate([b for _, b in calls]), **inp)
    print("%d calls, %d words -> %s (%d bytes)" % (len(calls), sum(len(b) for _, b in calls), args.out, os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
