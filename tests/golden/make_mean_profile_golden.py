"""Writes tests/golden/mean_profile_golden.npz: inputs and expected values for the profile means (MTG_MEAN_SINE,
MTG_MEAN_TWOSINE, MTG_MEAN_GAUSSIAN) of tests/test_mean_profile_gpu.py.  Runs on the CPU:

    python tests/golden/make_mean_profile_golden.py

Per row the truth lnL has the mean evaluated by mpmath at 50 digits from the double inputs (the reference's formulas,
mind_the_gaps/models/mean_models.py) and subtracted from y in mpmath; for N <= 129 that residual goes through a dense
mpmath Cholesky (oracle.dense's arithmetic, its residual left in mpmath), for longer rows the quad oracle
(oracle.quad.loglike) takes the residual rounded to double.  Stored with it: delta_np, the largest difference between
numpy's float64 evaluation of the same formula and the mpmath mean; w1 = |K^-1 r|_1 (oracle.predict.apply_inverse);
S, the likelihood's error scale, and c64, celerite's float64 value, both on the rounded residual, as
tests/test_accuracy_vs_quad_gpu.py uses them; max |mean| and max |r|.  The file ends by checking that numpy's float64
mean pushed through the quad oracle stays inside the test's bound on every row.
"""
import json
import os
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle import celerite as oracle_c, dense, predict as oracle_p, quad  # noqa: E402

U = 2.0 ** -53
SINE, TWOSINE, GAUSSIAN = 2, 3, 4
REAL, SHO, JITTER, DRW, LORENTZIAN = 0, 3, 5, 6, 7
# rank families: kinds and kernel parameters (logs, in the order of include/mtg.h)
FAMILIES = {
    "j0": ([JITTER], [-1.0]),
    "j1": ([DRW], [0.3, -1.2]),
    "j2c": ([SHO], [0.1, 1.1, 0.4]),                 # Q = e^1.1 > 1/2: one complex term
    "j2r": ([SHO], [0.1, -1.6, 0.4]),                # Q = e^-1.6 < 1/2: two real terms
    "j5": ([DRW, SHO, LORENTZIAN], [0.3, -1.2, -0.4, 0.9, 0.2, -0.7, 2.3, 1.1]),
    "j6": ([DRW, SHO, LORENTZIAN, REAL], [0.3, -1.2, -0.4, 0.9, 0.2, -0.7, 2.3, 1.1, -0.9, 0.6]),
}
SIZES = [1, 2, 3, 64, 65, 129, 4097]


def lightcurve(N, seed, L=1, per_lc=False):
    rng = np.random.RandomState(seed)
    t = 50.0 + np.cumsum(rng.uniform(0.2, 1.8, size=(L if per_lc else 1, N)), axis=1)
    y = 3.0 + rng.normal(0.0, 1.0, size=(L, N))
    dy = rng.uniform(0.05, 0.3, size=(L, N))
    return (t if per_lc else t[0]), y, dy


def mean_params(kind, t, i):
    """the i-th deterministic choice of a kind's parameters on the sampling t"""
    t0, t1 = float(t[0]), float(t[-1])
    span = max(t1 - t0, 1.0)
    if kind in (SINE, TWOSINE):
        phase_at_end = 10.0 ** (5.0 * ((i * 7) % 11) / 10.0)        # frequency t_max from 1 to 1e5 rad
        w = phase_at_end / t1
        if kind == SINE:
            return [2.9 + 0.01 * i, 0.8 + 0.1 * (i % 3), w, 0.7 + 0.3 * (i % 5)]
        return [2.9 + 0.01 * i, 0.8, 0.7 + 0.3 * (i % 5), 0.35, -1.1 + 0.2 * (i % 4), w]
    centre = [0.5 * (t0 + t1), t0, t1 + 0.3 * span, t0 - 2.0 * span][i % 4]     # inside, at the edge, outside
    sigma = span * 10.0 ** (-3.0 + 4.0 * ((i * 3) % 7) / 6.0)                   # 1e-3 to 10 durations
    return [centre, sigma, 4.0 * sigma, 3.1]


def mean_np(kind, p, x):
    """numpy's float64 evaluation of the reference's formulas, operation for operation"""
    if kind == SINE:
        return p[0] + p[1] * np.sin(p[2] * x + p[3])
    if kind == TWOSINE:
        return p[0] + p[1] * np.sin(p[5] * x + p[2]) + p[3] * np.sin(2 * p[5] * x + p[4])
    return p[2] / (2 * np.pi * p[1]) * np.exp(-(x - p[0]) ** 2 / (2 * p[1] ** 2)) + p[3]


def mean_mp(kind, p, x):
    q = [mp.mpf(float(v)) for v in p]
    out = []
    for xv in x:
        xv = mp.mpf(float(xv))
        if kind == SINE:
            out.append(q[0] + q[1] * mp.sin(q[2] * xv + q[3]))
        elif kind == TWOSINE:
            out.append(q[0] + q[1] * mp.sin(q[5] * xv + q[2]) + q[3] * mp.sin(2 * q[5] * xv + q[4]))
        else:
            out.append(q[2] / (2 * mp.pi * q[1]) * mp.exp(-(xv - q[0]) ** 2 / (2 * q[1] ** 2)) + q[3])
    return out


def dense_mp(t, r, dy, coeffs):
    """oracle.dense.dense_loglike_mp with the residual r already in mpmath"""
    ar, cr, ac, bc, cc, dc, jitter = coeffs
    tt = [mp.mpf(float(v)) for v in t]
    n = len(tt)
    K = mp.matrix(n, n)
    for i in range(n):
        for j in range(i + 1):
            tau = abs(tt[i] - tt[j])
            k = mp.mpf(0)
            for a, c in zip(ar, cr):
                k += mp.mpf(float(a)) * mp.exp(-mp.mpf(float(c)) * tau)
            for a, b, c, d in zip(ac, bc, cc, dc):
                k += mp.exp(-mp.mpf(float(c)) * tau) * (mp.mpf(float(a)) * mp.cos(mp.mpf(float(d)) * tau)
                                                        + mp.mpf(float(b)) * mp.sin(mp.mpf(float(d)) * tau))
            K[i, j] = k
            K[j, i] = k
        K[i, i] += mp.mpf(float(np.float64(dy[i]) + np.float64(1e-12))) ** 2 + mp.mpf(float(jitter))
    Lc = mp.cholesky(K)
    z = dense._forward_sub(Lc, mp.matrix(r), n)
    dot = sum(zv * zv for zv in z)
    logdet = 2 * sum(mp.log(Lc[i, i]) for i in range(n))
    return float(-(dot + logdet + n * mp.log(2 * mp.pi)) / 2)


def make_row(t, y, dy, kinds, kpar, kind, mpar):
    """truth and error scales of one (light curve, theta) pair"""
    with mp.workdps(50):
        mu = mean_mp(kind, mpar, t)
        r_mp = [mp.mpf(float(yv)) - m for yv, m in zip(y, mu)]
        mu_np = mean_np(kind, np.asarray(mpar), t)
        delta = max(abs(float(mp.mpf(float(a)) - b)) for a, b in zip(mu_np, mu))
        r = np.array([float(v) for v in r_mp])
        full0 = np.concatenate([kpar, [0.0]])
        hi, lo, scale, st = quad.loglike(t, r, dy, kinds, full0)
        assert st[0] == 0
        truth = dense_mp(t, r_mp, dy, dense.build_coeffs(kinds, kpar)) if len(t) <= 129 else float(hi[0] + lo[0])
    c64 = float(oracle_c.logprob_batch(t, r, dy, kinds, full0)[0][0])
    w1 = float(np.sum(np.abs(oracle_p.apply_inverse(t, dy, kinds, full0, r).x)))
    # numpy's float64 mean through the quad oracle: what the bound must hold
    hn, ln, _, _ = quad.loglike(t, y - mu_np, dy, kinds, full0)
    return dict(lnL=truth, delta_np=delta, w1=w1, S=float(scale[0]), c64=c64, max_mean=float(np.max(np.abs(mu_np))),
                max_r=float(np.max(np.abs(r))), lnL_np=float(hn[0] + ln[0]))


def bound(row, N):
    like = max(10.0 * abs(row["c64"] - row["lnL"]), 64.0 * np.sqrt(N) * U * row["S"])
    return like + row["w1"] * (4.0 * row["delta_np"] + 4.0 * U * row["max_mean"] + U * row["max_r"])


def main():
    cases, arrays = [], {}

    def add(name, t, y, dy, kinds, kind, fulls, lc, per_lc=False, free=None):
        i = len(cases)
        t, y, dy = np.asarray(t), np.atleast_2d(y), np.atleast_2d(dy)
        nk = len(fulls[0]) - {SINE: 4, TWOSINE: 6, GAUSSIAN: 4}[kind]
        rows = [make_row(t[l] if per_lc else t, y[l], dy[l], kinds, np.asarray(f[:nk]), kind, list(f[nk:]))
                for f, l in zip(fulls, lc)]
        for r in rows:
            assert abs(r["lnL_np"] - r["lnL"]) <= bound(r, y.shape[1]), (name, r, bound(r, y.shape[1]))
        arrays.update({"c%d_t" % i: t, "c%d_y" % i: y, "c%d_dy" % i: dy, "c%d_full" % i: np.asarray(fulls, dtype=np.float64),
                       "c%d_lc" % i: np.asarray(lc, dtype=np.int32)})
        for key in ("lnL", "delta_np", "w1", "S", "c64", "max_mean", "max_r"):
            arrays["c%d_%s" % (i, key)] = np.array([r[key] for r in rows])
        cases.append(dict(name=name, kinds=[int(k) for k in kinds], mean_kind=int(kind), per_lc=bool(per_lc), nk=int(nk),
                          free=list(range(len(fulls[0]))) if free is None else [int(v) for v in free]))
        print("%-28s N %5d rows %3d worst numpy/bound %.3g" % (
            name, y.shape[1], len(rows), max(abs(r["lnL_np"] - r["lnL"]) / bound(r, y.shape[1]) for r in rows)), flush=True)

    n = 0
    for fam, (kinds, kpar) in FAMILIES.items():
        for kind in (SINE, TWOSINE, GAUSSIAN):
            for N in SIZES:
                if N == 4097 and kind != (SINE, TWOSINE, GAUSSIAN)[list(FAMILIES).index(fam) % 3]:
                    continue            # one long row per family, the kinds taking turns
                t, y, dy = lightcurve(N, 100 + n)
                add("%s/kind%d/n%d" % (fam, kind, N), t, y, dy, kinds, kind, [kpar + mean_params(kind, t, n)], [0])
                n += 1
    # a libm-variant row: the Lorentzian's d max(dx) = e^29.5 x 1.8 > MTG_TRIG_FAST_MAX = 1e12, beside a table row
    kinds, kpar = FAMILIES["j5"]
    t, y, dy = lightcurve(64, 7)
    big = list(kpar)
    big[7] = 29.5
    add("j5/libm", t, y, dy, kinds, SINE, [big + mean_params(SINE, t, 3), kpar + mean_params(SINE, t, 4)], [0, 0])
    # batches: two light curves through lc_index, B = 5 and 67; both sides of Q = 1/2 in one batch
    t, y, dy = lightcurve(65, 8, L=2)
    rng = np.random.RandomState(9)
    fulls = [[0.1, float(rng.uniform(-2.0, 1.5)), 0.4] + mean_params(SINE, t, b) for b in range(67)]
    add("batch/sho_mixed_b67", t, y, dy, [SHO], SINE, fulls, [b % 2 for b in range(67)])
    fulls = [[0.3, -1.2 + 0.1 * b] + mean_params(TWOSINE, t, b) for b in range(5)]
    add("batch/drw_b5", t, y, dy, [DRW], TWOSINE, fulls, [0, 1, 1, 0, 1])
    # per-light-curve sampling, and a batch with part of the mean frozen (sigma and constant of the Gaussian)
    t, y, dy = lightcurve(65, 10, L=2, per_lc=True)
    base = mean_params(GAUSSIAN, t[0], 0)
    fulls = [list(FAMILIES["j5"][1]) + [base[0] + 0.7 * b, base[1], base[2] * (1.0 + 0.1 * b), base[3]] for b in range(5)]
    add("batch/per_lc_frozen_b5", t, y, dy, FAMILIES["j5"][0], GAUSSIAN, fulls, [0, 1, 0, 1, 1], per_lc=True,
        free=list(range(8)) + [8, 10])
    arrays["cases"] = np.array(json.dumps(cases))
    np.savez_compressed(os.path.join(HERE, "mean_profile_golden.npz"), **arrays)
    print("wrote %d cases" % len(cases))


if __name__ == "__main__":
    main()
