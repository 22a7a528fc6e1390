#!/usr/bin/env python3
"""The per-row GP entries' outputs, bit for bit, at the smallest shapes that reach every branch of the code they share
(csrc/mtg_pat_replay.h, csrc/mtg_factor_step.h, the transposed tile of csrc/mtg_device.h): predict_at, predict_terms,
gp_draw, whiten, gp_cond_draw and loglike_grad -> tests/golden/gp_rows_parent_bits.npz, which
tests/test_gp_rows_parent_bits_gpu.py holds every later build to.

Only public Engine calls, so that this file runs unchanged on the commit before the replay and the innovation step were
written once (where the fixture was made; `commit` in the fixture) and on every commit after it.

    N       2 MTG_PAT_C + 3 = 131 (checkpoints at 0, 64, 128 and a ragged tail; four full MTG_DRAW_T tiles and one of 3),
            and the smallest: 1 and 2 (no entry refuses an N)
    rows    B = 67 (a full workgroup and one of 3) at the rank-3 model, with row 5 outside its prior bounds (rejected
            before the sweep) and row 13 not positive definite (a real term of amplitude e^80, c = e^-40: the pivot goes
            non-positive inside the sweep); B = 3 elsewhere
    ranks   0 (jitter), 1 (real), 2 (complex), 3 (real + complex), SHO with an under- and an over-damped row in one
            batch (NR differs per row), 10 = MTG_MAX_J (two real + four complex); constant and linear mean
    curves  shared sampling with L = 1; sampling per light curve with L = 3, lc_index over all three
    times   M = 70 (a block of 64 and a ragged one), unsorted, one duplicate: two before the first sample, t_0, t_63,
            t_64, t_127, t_128, t_{N-1}, one strictly between t_63 and t_64, two after the last sample, the rest inside;
            at N = 1, 2: one before, one between (N = 2), one after
    calls   predict_at with and without the variance; predict_terms with {each term, all, all | TERMS_MEAN, none}, with
            and without the variance (at B = 67 without it: the first 16 rows); gp_draw with given normals and with a seed; whiten of the resident data and of a
            given y, each as residuals + lags = 5 + KS and as the sums alone; gp_cond_draw with given normals and with a
            seed; loglike_grad at ranks 0, 3, 6 = MTG_GRAD_MAX_J and 10 (refused: its error code is what is stored)

Every output is stored as its 64-bit pattern (statuses and codes as int64), all calls one after the other in `bits`
(`names`, `sizes`: whose and how many).  Run on a GPU:
    python3 tests/golden/make_gp_rows_parent_bits.py --commit $(git rev-parse HEAD)
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "gp_rows_parent_bits.npz")
SEED = 20261021
N_BIG, B_BIG, M_BIG = 131, 67, 70
K_REAL, K_COMPLEX4, K_SHO, K_JITTER = 0, 2, 3, 5      # include/mtg.h, MTG_TERM_*
MEAN_CONSTANT, MEAN_LINEAR = 0, 1
TERMS_MEAN = 1 << 31
SEED_DRAW, SEED_COND = 0x123456789ABCDEF, 77

REAL = [0.0, -1.0]                                    # log a, log c
COMPLEX = [[0.0, -5.0, -1.0, 0.5], [-0.5, -5.0, -0.5, 1.2], [-1.0, -5.0, 0.0, 0.0], [0.3, -5.0, -1.5, -0.8]]
# name -> (kinds, mean kind, kernel parameters of the base row)
MODELS = {
    "j0": ([K_JITTER], MEAN_LINEAR, [-1.0]),
    "j1": ([K_REAL], MEAN_CONSTANT, REAL),
    "j2": ([K_COMPLEX4], MEAN_CONSTANT, COMPLEX[0]),
    "j3": ([K_REAL, K_COMPLEX4], MEAN_LINEAR, REAL + COMPLEX[0]),
    "sho": ([K_SHO], MEAN_CONSTANT, [0.0, 0.5, 0.5]),  # log S0, log Q, log omega0; the rows' log Q alternate sides of Q = 1/2
    "j6": ([K_COMPLEX4] * 3, MEAN_CONSTANT, COMPLEX[0] + COMPLEX[1] + COMPLEX[2]),
    "j10": ([K_REAL, K_REAL] + [K_COMPLEX4] * 4, MEAN_CONSTANT, REAL + [-0.7, 0.3] + sum(COMPLEX, [])),
}
INPUTS = ("t", "t_own", "y", "dy", "ts", "ts_own", "ts_small", "normals", "new_normals") + tuple(
    "theta_" + name for name in MODELS) + ("theta_big",)


def new_times(t, rng):
    """M_BIG times around and among the samples t [N_BIG], shuffled, one of them twice"""
    span = t[-1] - t[0]
    special = [t[0] - 0.3 * span, t[0] - 1e-3, t[0], t[63], t[64], t[127], t[128], t[-1], 0.5 * (t[63] + t[64]),
               t[-1] + 1e-3, t[-1] + 0.3 * span]
    assert t[63] < special[8] < t[64]
    inside = rng.uniform(t[0], t[-1], size=M_BIG - len(special) - 1)
    ts = np.concatenate([special, inside, inside[:1]])
    return ts[rng.permutation(M_BIG)]


def thetas(name, B, rng):
    kinds, mean_kind, base = MODELS[name]
    mean = [1e-3, 0.1] if mean_kind == MEAN_LINEAR else [0.1]
    rows = np.tile(np.asarray(base + mean, dtype=np.float64), (B, 1))
    rows += 0.05 * rng.uniform(-1.0, 1.0, size=rows.shape) * np.where(np.abs(rows[0]) == 1e-3, 1e-3, 1.0)   # (the slope stays small)
    if name == "sho":
        rows[:, 1] = np.where(np.arange(B) & 1, -1.2, 0.5)
    return rows


def draw_inputs():
    """every call's inputs from SEED"""
    rng = np.random.default_rng(SEED)
    t = np.sort(rng.uniform(0.0, 40.0, size=N_BIG)) + 100.0
    t_own = np.sort(rng.uniform(0.0, 40.0, size=(3, N_BIG)), axis=-1) + 100.0
    y = rng.standard_normal((3, N_BIG)) + np.sin(0.9 * t) + 0.1
    dy = rng.uniform(0.1, 0.5, size=(3, N_BIG))
    inp = dict(t=t, t_own=t_own, y=y, dy=dy, ts=new_times(t, rng), ts_own=new_times(t_own[1], rng),
               ts_small=np.array([t[1] + 1.0, t[0] - 1.0, 0.5 * (t[0] + t[1])]),
               normals=rng.standard_normal((B_BIG, N_BIG)), new_normals=rng.standard_normal((B_BIG, M_BIG)))
    for name in MODELS:
        inp["theta_" + name] = thetas(name, 3, rng)
    big = thetas("j3", B_BIG, rng)
    big[5, 2] = 101.0            # outside the box of bind()
    big[13, :2] = 80.0, -40.0    # not positive definite in float64
    inp["theta_big"] = big
    return inp


def bits(*arrays):
    """64-bit patterns of doubles; integers (statuses, codes) as int64; None (an output not asked for) as nothing"""
    out = []
    for a in arrays:
        if a is None:
            continue
        a = np.ascontiguousarray(a)
        if a.dtype != np.float64:
            a = a.astype(np.int64)
        out.append(a.ravel().view(np.uint64))
    return np.concatenate(out)


def bind(eng, name, t, y, dy):
    kinds, mean_kind, base = MODELS[name]
    PF = len(base) + (2 if mean_kind == MEAN_LINEAR else 1)
    bounds = np.tile([-100.0, 100.0], (PF, 1))
    full = np.asarray(base + [0.0] * (PF - len(base)))
    eng.set_lightcurves(t, y, dy)
    eng.set_model(kinds, full, np.arange(PF, dtype=np.int32), bounds, mean_kind=mean_kind)
    return len(kinds)


def run(eng, inp):
    """-> [(name, uint64 bits)] of every call, in a fixed order"""
    from mind_the_gaps_amd.engine import EngineError
    out = []

    def rows_calls(tag, nterms, theta, lc, ts, N, lags, terms_rows=None):
        B, M = len(theta), len(ts)
        for var in (True, False):
            out.append(("%s/predict_at_var%d" % (tag, var), bits(*eng.predict_at(theta, ts, lc, return_var=var))))
        full = (1 << nterms) - 1
        masks = [1 << k for k in range(nterms)] + [full, full | TERMS_MEAN, 0]
        out.append((tag + "/predict_terms_var1", bits(*eng.predict_terms(theta, masks, ts, lc, return_var=True))))
        out.append((tag + "/predict_terms_var0", bits(*eng.predict_terms(theta[:terms_rows], masks, ts, lc, return_var=False))))
        normals = np.ascontiguousarray(inp["normals"][:B, :N])
        out.append((tag + "/gp_draw_given", bits(*eng.gp_draw(theta, lc, normals=normals))))
        out.append((tag + "/gp_draw_seed", bits(*eng.gp_draw(theta, lc, seed=SEED_DRAW))))
        for label, yg in (("resident", None), ("given", 0.7 * normals[::-1] + 0.1)):
            out.append(("%s/whiten_%s_full" % (tag, label), bits(*eng.whiten(theta, lc, y=yg, residuals=True, lags=lags, ks=True))))
            out.append(("%s/whiten_%s_sums" % (tag, label), bits(*eng.whiten(theta, lc, y=yg, residuals=False, lags=0, ks=False))))
        cn = np.ascontiguousarray(np.concatenate([normals[:, ::-1], inp["new_normals"][:B, :M]], axis=1))
        out.append((tag + "/gp_cond_draw_given", bits(*eng.gp_cond_draw(theta, ts, lc, normals=cn))))
        out.append((tag + "/gp_cond_draw_seed", bits(*eng.gp_cond_draw(theta, ts, lc, seed=SEED_COND))))

    def grad(tag, theta, lc, add_prior):
        try:
            out.append((tag + "/loglike_grad", bits(*eng.loglike_grad(theta, lc, add_prior=add_prior))))
        except EngineError as exc:                     # a rank beyond the tangent sweep's: refused, by this code
            out.append((tag + "/loglike_grad_refused", bits(np.array([exc.code]))))

    shared = (inp["t"], inp["y"][0], inp["dy"][0])
    own = (inp["t_own"], inp["y"], inp["dy"])
    lc3 = np.array([2, 0, 1], dtype=np.int32)
    # B = 67 at rank 3, shared sampling (the variance-free components: the first 16 rows, rows 5 and 13 among them --
    # a lane of its own per (row, time), and the factor stage without the variance runs on all 67 under predict_at)
    nterms = bind(eng, "j3", *shared)
    rows_calls("big_j3", nterms, inp["theta_big"], None, inp["ts"], N_BIG, 5, terms_rows=16)
    grad("big_j3", inp["theta_big"], None, True)
    # B = 3 at every rank: shared sampling, or sampling per light curve
    for name, sampling in (("j0", "shared"), ("j0", "own"), ("j1", "shared"), ("j2", "shared"), ("j3", "own"), ("sho", "shared"),
                           ("sho", "own"), ("j10", "shared")):
        nterms = bind(eng, name, *(own if sampling == "own" else shared))
        rows_calls("%s_%s" % (sampling, name), nterms, inp["theta_" + name], lc3 if sampling == "own" else None,
                   inp["ts_own"] if sampling == "own" else inp["ts"], N_BIG, 5)
    for name in ("j0", "j3", "sho", "j6", "j10"):
        bind(eng, name, *own)
        grad("own_" + name, inp["theta_" + name], lc3, False)
    # the smallest N at rank 3: a time before, one between (N = 2), one after
    for n in (1, 2):
        nterms = bind(eng, "j3", inp["t"][:n], inp["y"][0, :n], inp["dy"][0, :n])
        rows_calls("n%d_j3" % n, nterms, inp["theta_j3"], None, inp["ts_small"][:n + 1], n, n - 1)
        grad("n%d_j3" % n, inp["theta_j3"], None, False)
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
    for name, b in calls:
        if name in ("big_j3/gp_draw_given", "big_j3/whiten_given_sums", "big_j3/gp_cond_draw_given", "big_j3/loglike_grad"):
            print(name, "statuses != 0:", {int(i): int(v) for i, v in enumerate(b[-B_BIG:].view(np.int64)) if v})
    print("%d calls, %d words -> %s (%d bytes)" % (len(calls), sum(len(b) for _, b in calls), args.out, os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
