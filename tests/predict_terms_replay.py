"""tests/predict_terms_replay.py -- TEST INFRASTRUCTURE: the conditional mean and variance of COMPONENTS of the sum
kernel at new times, in numpy float64 for one parameter vector: the executable specification of
mind_the_gaps_amd/csrc/mtg_predict_terms.hip, on top of tests/predict_at_replay.py (same recurrences, same notation,
every S_n, f_n, G_n, g_n kept).  The factorisation is that of the whole K; for component c only the generators at t*
and k(0) are restricted to the slots of its terms:

    Um = U* on the slots of the selected terms, 0 elsewhere;  Vm likewise;  k_c(0) = sum of a over those slots
    q = S* Um,  Wt = Vm - q
    mu_c*  = [mean(t*)] + Um^T f* + Wt^T g*
    var_c* = k_c(0) - Um^T q - Wt^T X* Wt

With every term selected and the mean added the operations are predict_at_replay.predict_at's, in its order: the results
are equal bit for bit.
"""
import numpy as np

from predict_at_replay import generators


def slot_owners(term_coeffs):
    """the term of every slot, in the generators' order (real slots, then the two slots of every complex pair), from
    the coefficients of each term alone, ``term_coeffs[k]`` as oracle.dense.build_coeffs([kind_k], ...) returns them;
    also the concatenated coefficients of the whole model"""
    real = [k for k, c in enumerate(term_coeffs) for _ in c[0]]
    comp = [k for k, c in enumerate(term_coeffs) for _ in c[2]]
    whole = tuple(np.concatenate([np.asarray(c[i], dtype=np.float64) for c in term_coeffs]) for i in range(6))
    whole += (float(sum(c[6] for c in term_coeffs)),)
    return np.array(real + [k for k in comp for _ in (0, 1)], dtype=np.int64), whole


def predict_terms(t, y, yerr, coeffs, mean, ts, owner, masks, add_mean):
    """mu [T][M], var [T][M]: component c is the sum of the terms k with bit k of masks[c] set, ``owner`` the term of
    every slot (slot_owners); ``add_mean`` adds mean(t*) to every mu.  Otherwise as predict_at_replay.predict_at."""
    t, y, yerr = (np.asarray(v, dtype=np.float64) for v in (t, y, yerr))
    ts = np.atleast_1d(np.asarray(ts, dtype=np.float64))
    N = len(t)
    U, V, c = generators(coeffs, t, t[0])
    J = len(c)
    NR = len(coeffs[0])
    a_slot = np.zeros(J)                      # what a slot adds to k(0): a of a real slot and of the first of a pair
    a_slot[:NR], a_slot[NR::2] = coeffs[0], coeffs[2]
    k0 = float(np.sum(coeffs[0]) + np.sum(coeffs[2]))
    d = yerr ** 2 + coeffs[6]
    r = y - mean(t)
    phi = np.exp(-c[None, :] * np.diff(t, prepend=t[0])[:, None])
    S, f = np.zeros((N, J, J)), np.zeros((N, J))
    W, D, z = np.zeros((N, J)), np.zeros(N), np.zeros(N)
    Sc, fc = np.zeros((J, J)), np.zeros(J)
    for n in range(N):
        if n > 0:
            Sc = np.outer(phi[n], phi[n]) * (Sc + D[n - 1] * np.outer(W[n - 1], W[n - 1]))
            fc = phi[n] * (fc + W[n - 1] * z[n - 1])
        S[n], f[n] = Sc, fc
        q = Sc @ U[n]
        D[n] = d[n] + k0 - U[n] @ q
        if not D[n] > 0.0:
            raise np.linalg.LinAlgError("not positive definite at sample %d" % n)
        W[n] = (V[n] - q) / D[n]
        z[n] = r[n] - U[n] @ fc
    G, g, x = np.zeros((N + 1, J, J)), np.zeros((N + 1, J)), np.zeros(N)
    eye = np.eye(J)
    for n in range(N - 1, -1, -1):
        if n < N - 1:
            g[n] = phi[n + 1] * (g[n + 1] + U[n + 1] * x[n + 1])
            X = np.outer(phi[n + 1], phi[n + 1]) * G[n + 1]
        else:
            X = np.zeros((J, J))
        x[n] = z[n] / D[n] - W[n] @ g[n]
        A = eye - np.outer(U[n], W[n])
        G[n] = np.outer(U[n], U[n]) / D[n] + A @ X @ A.T
    Us, Vs, _ = generators(coeffs, ts, t[0])
    mu, var = np.empty((len(masks), len(ts))), np.empty((len(masks), len(ts)))
    for m, tm in enumerate(ts):
        n0 = int(np.searchsorted(t, tm, side="right")) - 1
        if n0 >= 0:
            p = np.exp(-c * (tm - t[n0]))
            Ss = np.outer(p, p) * (S[n0] + D[n0] * np.outer(W[n0], W[n0]))
            fs = p * (f[n0] + W[n0] * z[n0])
        else:
            Ss, fs = np.zeros((J, J)), np.zeros(J)
        if n0 < N - 1:
            p = np.exp(-c * (t[n0 + 1] - tm))
            Xs = np.outer(p, p) * G[n0 + 1]
            gs = p * (g[n0 + 1] + U[n0 + 1] * x[n0 + 1])
        else:
            Xs, gs = np.zeros((J, J)), np.zeros(J)
        for k, mask in enumerate(masks):
            sel = ((int(mask) >> owner) & 1).astype(bool)
            Um, Vm = np.where(sel, Us[m], 0.0), np.where(sel, Vs[m], 0.0)
            k0c = float(np.sum(a_slot[:NR][sel[:NR]]) + np.sum(a_slot[NR::2][sel[NR::2]]))
            q = Ss @ Um
            Wt = Vm - q
            mean_here = float(mean(np.array([tm]))[0]) if add_mean else 0.0
            mu[k, m] = mean_here + Um @ fs + Wt @ gs
            var[k, m] = k0c - Um @ q - Wt @ (Xs @ Wt)
    return mu, var
