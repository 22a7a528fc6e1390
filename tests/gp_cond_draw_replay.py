"""Host replay of the conditional draw (csrc/mtg_gp_cond_draw.hip): Matheron's rule in float64 numpy from the two replays
it is made of, the same by dense linear algebra, and the conditional covariance in mpmath.

    merged series   the N epochs and the unique new times in ascending order, a new time equal to an epoch after it;
                    diagonal sigma_n^2 + jitter at an epoch, 0 at a new time
    joint draw      z = L sqrt(D) q on the merged series (gp_draw_replay.factor / draw): y~ at the epochs, f* at the new times
    condition       y* = f* + mu(t*), mu the conditional mean of predict_at_replay.predict_at for the data y - y~

The caller's normals q [N + M]: the epochs' in epoch order, then one per entry of ts; a time given more than once takes
the normal of its first entry.  The device's: Philox4x32-10, counter (k, purpose, low word, high word of the draw's global
index), purpose 13 for the pair of epochs (2k, 2k + 1), 14 for the pair of unique new times of rank (2k, 2k + 1)."""
import numpy as np

import gp_draw_replay as R
import philox_replay
import predict_at_replay
from oracle import dense

PURPOSE_EPOCH, PURPOSE_NEW = 13, 14


def merge(t, ts):
    """-> tu [Mu] unique new times ascending, first [Mu] index in ts of the first entry with that time, inv [M] index into
    tu of every entry of ts, order [N + Mu] the merged series as indices into (epochs, then tu), is_new [N + Mu]"""
    t, ts = np.asarray(t, dtype=np.float64), np.atleast_1d(np.asarray(ts, dtype=np.float64))
    tu, first, inv = np.unique(ts, return_index=True, return_inverse=True)
    pos = np.searchsorted(t, tu, side="right")                   # epochs at or before each new time
    key = np.concatenate([2.0 * np.arange(len(t)), 2.0 * pos - 1.0])      # after epoch pos - 1, before epoch pos
    order = np.argsort(key, kind="stable")                       # equal keys: new times in one gap, ascending as tu is
    return tu, first, inv.ravel(), order, order >= len(t)


def merged_normals(q, N, first, order):
    """the caller's normals q [B][N + M] in merged order [B][N + Mu]"""
    return np.atleast_2d(np.asarray(q, dtype=np.float64))[:, np.concatenate([np.arange(N), N + first])[order]]


def joint_factor(t, yerr, coeffs, tu, order):
    diag = np.concatenate([np.asarray(yerr, dtype=np.float64) ** 2 + coeffs[6], np.zeros(len(tu))])[order]
    return R.factor(np.concatenate([t, tu])[order], diag, coeffs)


def draw(t, y, yerr, coeffs, mean, ts, q):
    """float64 replay: q [N + M] -> y* [M]; ``mean`` a function of time (the whole mean), yerr the standard deviations as
    the GP sees them"""
    t, y = np.asarray(t, dtype=np.float64), np.asarray(y, dtype=np.float64)
    N = len(t)
    tu, first, inv, order, is_new = merge(t, ts)
    z = R.draw(None, None, coeffs, merged_normals(q, N, first, order)[0], factors=joint_factor(t, yerr, coeffs, tu, order))
    mu, _ = predict_at_replay.predict_at(t, y - z[~is_new], yerr, coeffs, mean, tu)
    return (mu + z[is_new])[inv]


def dense_parts(t, yerr, coeffs, ts):
    """the dense float64 pieces: K [N][N] with its diagonal, C = K_* K^-1 [Mu][N], Lj the Cholesky factor of the merged
    covariance, and the merge"""
    t = np.asarray(t, dtype=np.float64)
    m = merge(t, ts)
    tu, order = m[0], m[3]
    tm = np.concatenate([t, tu])[order]
    K = dense.kernel_value(coeffs, t[:, None] - t[None, :])
    K[np.diag_indices_from(K)] += np.asarray(yerr, dtype=np.float64) ** 2 + coeffs[6]
    Ks = dense.kernel_value(coeffs, tu[:, None] - t[None, :])
    C = np.linalg.solve(K, Ks.T).T
    Kj = dense.kernel_value(coeffs, tm[:, None] - tm[None, :])
    Kj[np.diag_indices_from(Kj)] += np.concatenate([np.asarray(yerr, dtype=np.float64) ** 2 + coeffs[6], np.zeros(len(tu))])[order]
    return K, Ks, C, np.linalg.cholesky(Kj), m


def dense_draw(t, y, yerr, coeffs, mean, ts, q):
    """the dense Matheron formula in float64 numpy: q [B][N + M] or [N + M] -> (y* [B][M], scale s [B][M]), s the sum of
    the magnitudes that enter each value: |mean| + sum |Lj q| at the new time + sum_n |C_n| (|y_n - mean_n| + sum |Lj q| at
    epoch n)"""
    t, y = np.asarray(t, dtype=np.float64), np.asarray(y, dtype=np.float64)
    K, Ks, C, Lj, (tu, first, inv, order, is_new) = dense_parts(t, yerr, coeffs, ts)
    qm = merged_normals(q, len(t), first, order)
    z, za = qm @ Lj.T, np.abs(qm) @ np.abs(Lj).T
    r = y - mean(t)
    out = mean(tu)[None, :] + z[:, is_new] + (r[None, :] - z[:, ~is_new]) @ C.T
    s = np.abs(mean(tu))[None, :] + za[:, is_new] + (np.abs(r)[None, :] + za[:, ~is_new]) @ np.abs(C).T
    out, s = out[:, inv], s[:, inv]
    return (out, s) if np.ndim(q) == 2 else (out[0], s[0])


def dense_map(t, yerr, coeffs, ts):
    """A [Mu][N + Mu] with y* - E y* = A q_merged in float64, and a = |Lj_new| + |C| |Lj_epochs|, the magnitudes its
    entries are made of"""
    K, Ks, C, Lj, m = dense_parts(t, yerr, coeffs, ts)
    is_new = m[4]
    return Lj[is_new] - C @ Lj[~is_new], np.abs(Lj[is_new]) + np.abs(C) @ np.abs(Lj[~is_new])


def cond_cov(t, yerr, coeffs, ts):
    """K_** - K_* K^-1 K_*^T at the unique new times in float64 numpy, and the scale |K_**| + |K_*| |K^-1 K_*^T|"""
    K, Ks, C, Lj, m = dense_parts(t, yerr, coeffs, ts)
    tu = m[0]
    Kss = dense.kernel_value(coeffs, tu[:, None] - tu[None, :])
    X = np.linalg.solve(K, Ks.T)
    return Kss - Ks @ X, np.abs(Kss) + np.abs(Ks) @ np.abs(X)


def mp_cond_cov(t, yerr, coeffs, ts, dps=50):
    """the same in mpmath at ``dps`` digits, rounded to float64"""
    import mpmath as mp
    with mp.workdps(dps):
        f64 = lambda x: mp.mpf(float(x))
        ar, cr, ac, bc, cc, dc, jitter = coeffs
        terms = [(f64(a), mp.mpf(0), f64(c), mp.mpf(0)) for a, c in zip(ar, cr)]
        terms += [(f64(a), f64(b), f64(c), f64(d)) for a, b, c, d in zip(ac, bc, cc, dc)]

        def k(x, y):
            tau = abs(x - y)
            return sum((mp.exp(-c * tau) * (a * mp.cos(d * tau) + b * mp.sin(d * tau)) for a, b, c, d in terms), mp.mpf(0))

        tt = [f64(x) for x in t]
        tu = [f64(x) for x in np.unique(np.asarray(ts, dtype=np.float64))]
        N, M = len(tt), len(tu)
        K = mp.matrix(N, N)
        for i in range(N):
            for j in range(N):
                K[i, j] = k(tt[i], tt[j])
            K[i, i] += f64(yerr[i]) ** 2 + f64(jitter)
        Ks = mp.matrix(M, N)
        for i in range(M):
            for j in range(N):
                Ks[i, j] = k(tu[i], tt[j])
        X = [mp.lu_solve(K, Ks[j, :].T) for j in range(M)]         # column j of K^-1 K_*^T
        return np.array([[float(k(tu[i], tu[j]) - (Ks[i, :] * X[j])[0]) for j in range(M)] for i in range(M)])


def philox_normals(seed, draw_index, n, purpose):
    """Box-Muller on the replayed blocks (gp_draw_replay.philox_normals with this entry's counter word): n normals"""
    g = int(draw_index) & 0xFFFFFFFFFFFFFFFF
    r = philox_replay.philox(np.arange((n + 1) // 2, dtype=np.uint64), purpose, g & 0xFFFFFFFF, g >> 32, int(seed))
    u1, u2 = 1.0 - philox_replay.u01(r[0], r[1]), philox_replay.u01(r[2], r[3])
    rad = np.sqrt(-2.0 * np.log(u1))
    q = np.empty(2 * len(u1))
    q[0::2], q[1::2] = rad * R.cospi(2.0 * u2), rad * R.sinpi(2.0 * u2)
    return q[:n], np.repeat(rad, 2)[:n]


def device_normals(seed, draw_index, N, ts):
    """what the device draws for this call, laid out as the caller's normals [N + M] (a repeated time: its normal at
    every entry), and the Box-Muller radius of each"""
    tu, first, inv = np.unique(np.atleast_1d(np.asarray(ts, dtype=np.float64)), return_index=True, return_inverse=True)
    qe, re = philox_normals(seed, draw_index, N, PURPOSE_EPOCH)
    qn, rn = philox_normals(seed, draw_index, len(tu), PURPOSE_NEW)
    return np.concatenate([qe, qn[inv.ravel()]]), np.concatenate([re, rn[inv.ravel()]])
