#!/usr/bin/env python3
"""The outputs of mtg_lag_sums and mtg_cross_sums, bit for bit, at the smallest shapes that reach every branch of the two
lag-bin sweeps (csrc/mtg_lag.hip, csrc/mtg_cross.hip), of their reductions and of the planner and host code the two entries
share (csrc/mtg_lag_plan.h, mtg_capi.hip) -> tests/golden/lag_sweep_parent_bits.npz, which
tests/test_lag_sweep_parent_bits_gpu.py holds every later build to.

Only public Engine calls, so that this file runs unchanged on the commit before the planner and the host code were written
once (where the fixture was made; `commit` in the fixture) and on every commit after it.

    N       789 (four row blocks, the last partly filled with idle lanes), 255, 256, 257 (a row block against a chunk),
            2 (lag's smallest) and 1 (cross alone)
    M       523 (three chunks, the last ragged), 257, 256, 1
    L       shared sampling 1 (tile 1), 3 and 4 (tile 4, partly filled and full), 8 and 11 (tile 8, full and ragged);
            sampling of its own per light curve: 3 (tile 1, t_stride = N)
    L2      1 and L (one companion row for all, a row per light curve)
    edges   one bin; 128 bins wider than the span; five short bins (lag: early exits; cross: late starts too); bins wholly
            beyond the span (only zeros); edges that ARE pairs' lags, 0 among them; for cross negative and
            sign-straddling ones and bins wholly below the span
    times   repeated stamps in the resident and in the companion series, and companion stamps copied from the resident's
    sums    lag: sf alone and all six; cross: count, lag, cf, cf2 and all eight; count, noise and saa alone

Every output is stored as its 64-bit pattern, all calls one after the other in `bits` (`names`, `sizes`: whose and how
many; `solvers`: the kernel of every call).  Run on a GPU:
    python3 tests/golden/make_lag_sweep_parent_bits.py --commit $(git rev-parse HEAD)
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "lag_sweep_parent_bits.npz")
SEED = 20261021
N_BIG, M_BIG, L_BIG = 789, 523, 11
INPUTS = ("t", "t_own", "y", "dy", "t2", "y2")
LAG_ALL = ("count", "lag", "sf", "cf", "cf2", "noise")
CROSS_LIGHT = ("count", "lag", "cf", "cf2")
CROSS_ALL = CROSS_LIGHT + ("sa", "sb", "saa", "sbb")


def draw_inputs():
    """every call's inputs from SEED: the sets are leading slices of one draw"""
    rng = np.random.default_rng(SEED)
    t = np.sort(rng.uniform(0.0, 40.0, size=N_BIG)) + 100.0
    t[11] = t[10]                           # repeated stamps: pairs with tau == 0
    t[401] = t[402] = t[400]
    t_own = np.sort(rng.uniform(0.0, 40.0, size=(3, N_BIG)), axis=-1) + 100.0
    t_own[1, 300] = t_own[1, 299]
    y = rng.standard_normal((L_BIG, N_BIG)) + np.sin(0.9 * t) + 0.5 * np.cos(2.7 * t)
    dy = rng.uniform(0.1, 0.5, size=(L_BIG, N_BIG))
    t2 = rng.uniform(-10.0, 30.0, size=M_BIG) + 100.0      # the spans overlap only partly
    t2[:6] = t[[0, 10, 100, 256, 400, 500]]                # lags that are exactly 0, and exactly a resident pair's lag
    t2[6] = t2[7]
    t2 = np.sort(t2)
    y2 = rng.standard_normal((L_BIG, M_BIG)) + np.sin(0.9 * (t2 - 1.5))
    return dict(t=t, t_own=t_own, y=y, dy=dy, t2=t2, y2=y2)


def lag_edges(t):
    span = t[-1] - t[0]
    ties = np.unique([0.0, t[12] - t[10], t[300] - t[100], t[256] - t[255], t[700] - t[256], t[788] - t[0]])
    return dict(one=np.array([0.5, 20.0]), wide128=np.linspace(0.0, 1.2 * span, 129), short5=np.linspace(0.02 * span, 0.1 * span, 6),
                beyond=np.array([2.0, 3.0, 4.0]) * span, ties=ties)


def cross_edges(t, t2):
    span = t[-1] - t[0]
    ties = np.unique([0.0, t2[0] - t[788], t2[200] - t[300], t2[256] - t[255], t2[522] - t[0], t2[300] - t[10], t2[100] - t[400]])
    return dict(one=np.array([-5.0, 5.0]), wide128=np.linspace(-1.2 * span, 1.2 * span, 129), short5=np.linspace(0.02 * span, 0.1 * span, 6),
                negative6=np.linspace(-0.3 * span, -0.05 * span, 7), straddle3=np.array([-0.07, -0.01, 0.0, 0.05]) * span,
                beyond=np.array([2.0, 3.0, 4.0]) * span, below=np.array([-4.0, -3.0]) * span, ties=ties)


def bits(arrays):
    return np.concatenate([np.ascontiguousarray(a).ravel().view(np.uint64) for a in arrays])


def run(eng, inp):
    """-> [(name, kernel, uint64 bits)] of every call, in a fixed order"""
    out = []
    le, ce = lag_edges(inp["t"]), cross_edges(inp["t"], inp["t2"])

    def resident(L, N, own=False):
        eng.set_lightcurves(inp["t_own"][:, :N] if own else inp["t"][:N], inp["y"][:L, :N], inp["dy"][:L, :N])
        return "%s%d_n%d" % ("own" if own else "shared", L, N)

    def lag(where, tag, sums):
        got = eng.lag_sums(le[tag], **{k: k in sums for k in LAG_ALL})
        out.append(("lag/%s/%s/%s" % (where, tag, "+".join(sums)), eng.last_solver.split(" ")[0], bits([got[k] for k in sums])))

    def cross(where, M, L2, tag, sums):
        y2 = inp["y2"][0, :M] if L2 == 1 else inp["y2"][:L2, :M]
        got = eng.cross_sums(inp["t2"][:M], y2, ce[tag], **{k: k in sums for k in CROSS_ALL})
        out.append(("cross/%s_m%d_x%d/%s/%s" % (where, M, L2, tag, "+".join(sums)), eng.last_solver.split(" ")[0], bits([got[k] for k in sums])))

    few = ("one", "short5", "beyond", "ties")
    for L, own, lag_tags, cross_tags in ((11, False, few, few + ("negative6", "straddle3", "below")), (8, False, ("short5", "ties"), ("short5", "ties")),
                                         (4, False, ("short5", "ties"), ("short5", "ties")), (3, False, tuple(le), tuple(ce)),
                                         (3, True, ("one", "short5", "wide128"), ("short5", "negative6", "wide128")),
                                         (1, False, tuple(le), ("one", "short5", "negative6", "below", "ties"))):
        where = resident(L, N_BIG, own)
        for tag in lag_tags:
            lag(where, tag, ("sf",))
            lag(where, tag, LAG_ALL)
        for tag in cross_tags:
            for L2 in sorted({1, L}):
                if tag == "wide128" and not own:          # (the largest outputs once per kernel variant)
                    cross(where, M_BIG, L2, tag, CROSS_LIGHT if L2 == 1 else CROSS_ALL)
                    continue
                cross(where, M_BIG, L2, tag, CROSS_LIGHT)
                cross(where, M_BIG, L2, tag, CROSS_ALL)
        if L == 11:
            lag(where, "wide128", ("sf",))
        if L == 3 and not own:
            lag(where, "short5", ("count",))
            lag(where, "ties", ("noise",))
            cross(where, M_BIG, 1, "straddle3", ("count",))
            cross(where, M_BIG, 3, "short5", ("saa",))
            for M in (257, 256, 1):
                for tag in ("one", "short5", "negative6", "straddle3"):
                    for L2 in (1, 3):
                        cross(where, M, L2, tag, CROSS_ALL)
                    cross(where, M, 1, tag, CROSS_LIGHT)
    for N in (257, 256, 255, 2, 1):
        where = resident(3, N)
        for tag in ("one", "short5", "ties"):
            if N >= 2:
                lag(where, tag, ("sf",))
                lag(where, tag, LAG_ALL)
            cross(where, M_BIG, 3, tag, CROSS_ALL)
            cross(where, M_BIG, 1, tag, CROSS_LIGHT)
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
    np.savez_compressed(args.out, commit=np.array(args.commit), names=np.array([n for n, _, _ in calls]),
                        solvers=np.array([s for _, s, _ in calls]), sizes=np.array([len(b) for _, _, b in calls], dtype=np.int64),
                        bits=np.concatenate([b for _, _, b in calls]), **inp)
    print("%d calls, %d words, %d kernels -> %s (%d bytes)" % (len(calls), sum(len(b) for _, _, b in calls), len({s for _, s, _ in calls}),
                                                                args.out, os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
