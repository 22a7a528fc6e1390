"""tests/predict_at_replay.py -- TEST INFRASTRUCTURE: the conditional mean and variance at NEW times from the
semiseparable factorisation, in numpy float64 for one parameter vector.  It is the executable specification of
mind_the_gaps_amd/csrc/mtg_predict_at.hip (same recurrences, same notation, no checkpoints: every S_n, f_n, G_n, g_n
is kept) and the second side of tests/test_predict_at_cpu.py.

Notation of mtg_predict_kernel (W normalised by D):

    forward    S_n = phi_n phi_n^T o (S_{n-1} + D_{n-1} W_{n-1} W_{n-1}^T),  f_n = phi_n o (f_{n-1} + W_{n-1} z_{n-1})
               W_n = (V_n - S_n U_n) / D_n,  D_n = d_n + k(0) - U_n^T S_n U_n,  z_n = r_n - U_n^T f_n
    backward   g_n = phi_{n+1} o (g_{n+1} + U_{n+1} x_{n+1}),  x_n = z_n / D_n - W_n^T g_n          (x = K^-1 r)
               G_n = U_n U_n^T / D_n + (I - U_n W_n^T) X_n (I - W_n U_n^T),  X_n = phi_{n+1} phi_{n+1}^T o G_{n+1}

and for a new time t* with n0 the last sample at or before it (-1: before the first)

    phi* = exp(-c (t* - t_n0)),   S* = phi* phi*^T o (S_n0 + D_n0 W_n0 W_n0^T),  f* = phi* o (f_n0 + W_n0 z_n0)
    psi  = exp(-c (t_{n0+1} - t*)), X* = psi psi^T o G_{n0+1},                   g* = psi o (g_{n0+1} + U_{n0+1} x_{n0+1})
    q = S* U*,  Wt = V* - q
    mu*  = mean(t*) + U*^T f* + Wt^T g*
    var* = k(0) - U*^T q - Wt^T X* Wt

(S*, f* are 0 for n0 = -1; X*, g* are 0 for n0 = N - 1).  The factors are those of the unchanged matrix K.
"""
import numpy as np


def generators(coeffs, t, t_first):
    """U [..][J], V [..][J] at times t (phase at the elapsed time t - t_first) and the decay rates c [J]"""
    ar, cr, ac, bc, cc, dc = [np.asarray(v, dtype=np.float64) for v in coeffs[:6]]
    t = np.atleast_1d(np.asarray(t, dtype=np.float64))
    NR, NC = len(ar), len(ac)
    J = NR + 2 * NC
    U, V, c = np.empty(t.shape + (J,)), np.empty(t.shape + (J,)), np.empty(J)
    U[..., :NR], V[..., :NR], c[:NR] = ar, 1.0, cr
    ph = (t - t_first)[..., None] * dc
    cn, sn = np.cos(ph), np.sin(ph)
    U[..., NR::2], U[..., NR + 1::2] = ac * cn + bc * sn, ac * sn - bc * cn
    V[..., NR::2], V[..., NR + 1::2] = cn, sn
    c[NR::2], c[NR + 1::2] = cc, cc
    return U, V, c


def predict_at(t, y, yerr, coeffs, mean, ts):
    """mu [M], var [M] at times ts; ``coeffs`` as oracle.dense.build_coeffs returns them, ``mean`` a function of
    time (the whole mean), yerr the standard deviations as the GP sees them.  Raises if K is not positive definite."""
    t, y, yerr = (np.asarray(v, dtype=np.float64) for v in (t, y, yerr))
    ts = np.atleast_1d(np.asarray(ts, dtype=np.float64))
    N = len(t)
    U, V, c = generators(coeffs, t, t[0])
    J = len(c)
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
    mu, var = np.empty(len(ts)), np.empty(len(ts))
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
        q = Ss @ Us[m]
        Wt = Vs[m] - q
        mu[m] = float(mean(np.array([tm]))[0]) + Us[m] @ fs + Wt @ gs
        var[m] = k0 - Us[m] @ q - Wt @ (Xs @ Wt)
    return mu, var
