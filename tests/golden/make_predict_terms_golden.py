"""Makes tests/golden/predict_terms_golden.npz: the truth for mtg_predict_terms -- the conditional mean and variance
of every COMPONENT k_c of a sum kernel given the data,

    mu_c(t*) = k_c(t*, t) K^-1 r,        var_c(t*) = k_c(0) - k_c,*^T K^-1 k_c,*,       K of the whole model,

from the dense expression in mpmath at 50 digits (Cholesky of K, coefficients expanded from theta in mpmath too), on
the CPU.  Run from the repository root:  python tests/golden/make_predict_terms_golden.py   (under a minute).

Per group: the light curve (t, y, yerr as the GP sees it), kinds, extra, theta (kernel parameters, then the mean's),
mean_kind, the 48 new times ts, the masks (every single term, every pair, all terms, 0) and per (mask, time)
    mu, var               the truth, rounded to float64 (mu WITHOUT the mean; mean_ts holds the mean at ts)
    mu_c64err, var_c64err |float64 dense expression - truth| (numpy / scipy Cholesky of the float64 K)
    mu_scale, var_scale   s_mu = sum_n |k_c,*(n) (K^-1 r)_n| (the test adds |mean| where the mean is added),
                          s_var = k_c(0) + |k_c,*^T K^-1 k_c,*|
Every row is checked here to be positive definite in float64 (the dense Cholesky succeeds): status 0, nothing to skip.
Light curves: N = 150 (forward checkpoints at 0, 64, 128), one of N = 1 and one of N = 65.
"""
import itertools
import json
import os
import sys

import mpmath as mp
import numpy as np
from scipy.linalg import cho_factor, cho_solve

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from mind_the_gaps_amd import synthetic as synth  # noqa: E402
from oracle import dense  # noqa: E402

mp.mp.dps = 50
K = synth
M_NEW = 48


def term_mp(kind, p, extra):
    """one term's (real [(a, c)], complex [(a, b, c, d)], jitter) in mpmath -- oracle.dense.build_coeffs restated"""
    p = [mp.mpf(float(v)) for v in p]
    e = [mp.exp(v) for v in p]
    if kind == K.K_REAL:
        return [(e[0], e[1])], [], mp.mpf(0)
    if kind == K.K_DRW:
        return [(e[0], e[1])], [], mp.mpf(0)
    if kind == K.K_SHO:
        S0, Q, w0 = e
        if Q < mp.mpf(1) / 2:
            f = mp.sqrt(1 - 4 * Q * Q)
            return [(S0 * w0 * Q * (1 + 1 / f) / 2, w0 / Q * (1 - f) / 2), (S0 * w0 * Q * (1 - 1 / f) / 2, w0 / Q * (1 + f) / 2)], [], mp.mpf(0)
        f = mp.sqrt(4 * Q * Q - 1)
        return [], [(S0 * w0 * Q, S0 * w0 * Q / f, w0 / Q / 2, w0 / Q * f / 2)], mp.mpf(0)
    if kind == K.K_LORENTZIAN:
        return [], [(e[0], mp.mpf(0), e[2] / e[1] / 2, e[2])], mp.mpf(0)
    if kind == K.K_MATERN32:
        eps = mp.mpf(float(extra))
        w0 = mp.sqrt(3) * mp.exp(-p[1])
        S0 = mp.exp(2 * p[0]) / w0
        return [], [(w0 * S0, w0 * w0 * S0 / eps, w0, eps)], mp.mpf(0)
    if kind == K.K_JITTER:
        return [], [], mp.exp(2 * p[0])
    raise ValueError(kind)


def k_mp(term, tau):
    tau = abs(tau)
    s = mp.mpf(0)
    for a, c in term[0]:
        s += a * mp.exp(-c * tau)
    for a, b, c, d in term[1]:
        s += mp.exp(-c * tau) * (a * mp.cos(d * tau) + b * mp.sin(d * tau))
    return s


def new_times(t, rng):
    """3 before the first sample, 3 after the last, 6 equal to epochs (the first, the last, 64 and 128 among them where
    they exist), the rest between epochs with two duplicates; shuffled"""
    N = len(t)
    span = max(t[-1] - t[0], 10.0)
    before = t[0] - span * np.array([1e-3, 0.05, 1.0])
    after = t[-1] + span * np.array([1e-3, 0.05, 1.0])
    on = [0, N - 1] + [n for n in (64, 128) if n < N - 1]
    while len(on) < 6:
        on.append(int(rng.integers(N)))
    rest = M_NEW - 12 - 2
    if N > 1:
        i = rng.integers(N - 1, size=rest)
        between = t[i] + rng.uniform(0.1, 0.9, rest) * (t[i + 1] - t[i])
    else:
        between = t[0] + span * rng.uniform(-0.5, 0.5, rest)
    ts = np.concatenate([before, after, t[on], between])
    ts = np.concatenate([ts, ts[[14, 3]]])
    return ts[rng.permutation(len(ts))]


def masks_of(nterms):
    single = [1 << k for k in range(nterms)]
    pairs = [(1 << i) | (1 << j) for i, j in itertools.combinations(range(nterms), 2)]
    return sorted(set(single + pairs + [(1 << nterms) - 1])) + [0]


def solve_group(g):
    kinds, extra, theta, t, y, yerr, ts = g["kinds"], g["extra"], g["theta"], g["t"], g["y"], g["yerr"], g["ts"]
    N, nk = len(t), dense.n_kernel_params(kinds)
    mean_p = theta[nk:]
    masks = masks_of(len(kinds))
    # ---- float64 dense expression ----------------------------------------------------------------------------
    offs = np.concatenate([[0], np.cumsum([K.NPARAMS[k] for k in kinds])])
    co64 = [dense.build_coeffs([k], theta[offs[i]:offs[i + 1]], [extra[i]]) for i, k in enumerate(kinds)]
    mean64 = (lambda x: mean_p[0] * x + mean_p[1]) if g["mean_kind"] == 1 else (lambda x: np.zeros_like(x) + mean_p[0])
    K64 = sum(dense.kernel_value(c, t[:, None] - t[None, :]) for c in co64) + np.diag(yerr ** 2 + sum(c[6] for c in co64))
    cf = cho_factor(K64, lower=True)             # raises if not positive definite: every row has status 0
    x64 = cho_solve(cf, y - mean64(t))
    ks64 = [dense.kernel_value(c, ts[:, None] - t[None, :]) for c in co64]          # [term][M][N]
    k064 = [float(dense.kernel_value(c, 0.0)) for c in co64]
    # ---- the truth ---------------------------------------------------------------------------------------------
    tm, tsm = [mp.mpf(float(v)) for v in t], [mp.mpf(float(v)) for v in ts]
    terms = [term_mp(k, theta[offs[i]:offs[i + 1]], extra[i]) for i, k in enumerate(kinds)]
    jit = sum(tr[2] for tr in terms)
    if g["mean_kind"] == 1:
        mean = lambda x: mp.mpf(float(mean_p[0])) * x + mp.mpf(float(mean_p[1]))
    else:
        mean = lambda x: mp.mpf(float(mean_p[0]))
    L = [[mp.mpf(0)] * N for _ in range(N)]
    for i in range(N):
        for j in range(i + 1):
            kij = sum(k_mp(tr, tm[i] - tm[j]) for tr in terms)
            if i == j:
                kij += mp.mpf(float(yerr[i])) ** 2 + jit
            s = kij - mp.fdot(L[i][:j], L[j][:j])
            L[i][j] = mp.sqrt(s) if i == j else s / L[j][j]
    def fwd(b):
        z = []
        for i in range(N):
            z.append((b[i] - mp.fdot(L[i][:i], z)) / L[i][i])
        return z
    z = fwd([mp.mpf(float(y[n])) - mean(tm[n]) for n in range(N)])
    x = [mp.mpf(0)] * N
    for i in range(N - 1, -1, -1):
        x[i] = (z[i] - sum(L[j][i] * x[j] for j in range(i + 1, N))) / L[i][i]
    k0 = [k_mp(tr, mp.mpf(0)) for tr in terms]
    T, M = len(masks), len(ts)
    out = {k: np.zeros((T, M)) for k in ("mu", "var", "mu_c64err", "var_c64err", "mu_scale", "var_scale")}
    for m in range(M):
        rows = [[k_mp(tr, tsm[m] - tm[n]) for n in range(N)] for tr in terms]
        zs = [fwd(r) for r in rows]
        for c, mask in enumerate(masks):
            sel = [i for i in range(len(kinds)) if mask >> i & 1]
            kc = [sum(rows[i][n] for i in sel) for n in range(N)]
            zc = [sum(zs[i][n] for i in sel) for n in range(N)]
            mu = mp.fdot(kc, x)
            quad = mp.fdot(zc, zc)
            kc0 = sum((k0[i] for i in sel), mp.mpf(0))
            var = kc0 - quad
            k64 = sum((ks64[i][m] for i in sel), np.zeros(N))
            mu64 = float(k64 @ x64)
            var64 = float(sum(k064[i] for i in sel) - k64 @ cho_solve(cf, k64))
            out["mu"][c, m], out["var"][c, m] = float(mu), float(var)
            out["mu_c64err"][c, m], out["var_c64err"][c, m] = float(abs(mu64 - mu)), float(abs(var64 - var))
            out["mu_scale"][c, m] = float(sum(abs(kc[n] * x[n]) for n in range(N)))
            out["var_scale"][c, m] = float(kc0 + abs(quad))
    out["mean_ts"] = np.array([float(mean(v)) for v in tsm])
    out["masks"] = np.array(masks, dtype=np.uint32)
    return out


def main():
    rng = np.random.default_rng(20240)
    lcs = {}
    for name, N, seed in (("n150", 150, 61), ("n1", 1, 62), ("n65", 65, 63)):
        t, y, dy = synth.make_lightcurves(N, 1, seed=seed)
        lcs[name] = (t, y[0], dy[0] + 1e-12, new_times(t, rng))
    ln = np.log
    drw, lor, real = synth.TRUTH[K.K_DRW], synth.TRUTH[K.K_LORENTZIAN], synth.TRUTH[K.K_REAL]
    sho = lambda Q: [ln(50.0), ln(Q), ln(2 * np.pi / 7.0)]
    sho2 = lambda Q: [ln(20.0), ln(Q), ln(2 * np.pi / 3.0)]
    headline = [K.K_DRW, K.K_SHO, K.K_LORENTZIAN]
    th_head = drw + sho(3.0) + lor
    groups = [
        ("real", "n150", [K.K_REAL], real, 0, None),
        ("headline", "n150", headline, th_head, 0, None),
        ("sho_over_first", "n150", [K.K_SHO, K.K_SHO, K.K_DRW], sho(0.3) + sho2(5.0) + drw, 0, None),
        ("sho_over_second", "n150", [K.K_SHO, K.K_SHO, K.K_DRW], sho(5.0) + sho2(0.3) + drw, 0, None),
        ("matern_jitter_real", "n150", [K.K_MATERN32, K.K_JITTER, K.K_REAL], synth.TRUTH[K.K_MATERN32] + synth.TRUTH[K.K_JITTER] + real, 0, None),
        ("headline_linear", "n150", headline, th_head, 1, [0.013, 98.5]),
        ("headline_n1", "n1", headline, th_head, 0, None),
        ("headline_n65", "n65", headline, th_head, 0, None),
    ]
    arrays, manifest = {}, []
    for name, lc, kinds, th, mean_kind, mean_p in groups:
        t, y, yerr, ts = lcs[lc]
        # a constant mean travels as the light curve's y_offset (the model's own constant is frozen at 0): here it is the
        # mean parameter, and mu excludes it either way
        theta = np.array(list(th) + (list(mean_p) if mean_kind == 1 else [float(np.mean(y))]), dtype=np.float64)
        g = dict(kinds=kinds, extra=[0.01 if k == K.K_MATERN32 else 0.0 for k in kinds], theta=theta, t=t, y=y, yerr=yerr,
                 ts=ts, mean_kind=mean_kind)
        out = solve_group(g)
        if mean_kind == 0:
            out["mean_ts"] = np.zeros(len(ts))      # the y_offset is excluded from mu
        for k, v in dict(out, t=t, y=y, yerr=yerr, ts=ts, theta=theta).items():
            arrays["%s/%s" % (name, k)] = v
        manifest.append(dict(name=name, kinds=[int(k) for k in kinds], extra=g["extra"], mean_kind=mean_kind, N=int(len(t))))
        rho = np.max(out["mu_c64err"] / np.where(out["mu_scale"] > 0, out["mu_scale"], 1.0))
        print("%-20s N = %3d  masks %s  worst c64err / s: mu %.2e var %.2e" % (
            name, len(t), list(out["masks"]), rho, np.max(out["var_c64err"] / np.where(out["var_scale"] > 0, out["var_scale"], 1.0))),
            flush=True)
    arrays["manifest"] = np.frombuffer(json.dumps(dict(groups=manifest)).encode(), dtype=np.uint8)
    np.savez_compressed(os.path.join(HERE, "predict_terms_golden.npz"), **arrays)


if __name__ == "__main__":
    main()
