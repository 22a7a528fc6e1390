"""Host replay of the whitening sweep (csrc/mtg_whiten.hip), the counterpart of tests/gp_draw_replay.py whose
factorisation it shares: with K = L diag(D) L^T, L = I + tril(U W^T) and r = y - mean,

    f_n = phi_n o (f_{n-1} + W_{n-1} v_{n-1}),  v_n = r_n - U_n^T f_n,  q_n = v_n / sqrt(D_n)        (q = D^-1/2 L^-1 r)

in float64 numpy (whiten), the eight sums of a row and its autocorrelation as the device defines them (row_stats, acf),
the same sweep in mpmath with the scale of every sample and the sums' truths (mp_whiten), and the two dense routes: numpy's
Cholesky (dense_whiten) and mpmath's (mp_dense_whiten), where q solves chol(K) q = r by forward substitution."""
import math

import numpy as np

import gp_draw_replay as R

NSTATS = 8


def factor(t, diag, coeffs, phase="elapsed"):
    """gp_draw_replay.factor with its compensated accumulations; a white model (J = 0) has nothing to accumulate"""
    return R.factor(t, diag, coeffs, phase=phase, compensated=len(R.slots(coeffs)) > 0)


def whiten(t, dy, coeffs, y, mean=0.0, phase="elapsed", factors=None):
    """float64 replay: y [B][N] or [N] -> q of the same shape (gp_draw_replay.whiten); mean: scalar or [N]"""
    return R.whiten(t, dy, coeffs, y, mean=mean, phase=phase, factors=factors)


def ks_distances(q):
    """(D+, D-) of the one-sample KS test of q against the standard normal, Phi(x) = erfc(-x / sqrt 2) / 2"""
    x = np.sort(np.asarray(q, dtype=np.float64))
    N = len(x)
    cdf = np.array([0.5 * math.erfc(-v * 0.7071067811865476) for v in x])
    i = np.arange(1, N + 1, dtype=np.float64)
    return float(np.max(i / N - cdf)), float(np.max(cdf - (i - 1.0) / N))


def row_stats(q, D):
    """the eight slots of mtg_whiten's stats for one row: sum q, sum q^2, sum ln D, sum q^3, sum q^4, D+, D-, max |q|"""
    q = np.asarray(q, dtype=np.float64)
    dp, dm = ks_distances(q)
    return np.array([np.sum(q), np.sum(q * q), np.sum(np.log(D)), np.sum(q ** 3), np.sum(q ** 4), dp, dm, np.max(np.abs(q))])


def acf(q, K):
    """acf[k - 1] = sum_{n < N - k} q_n q_{n+k} / sum_n q_n^2, k = 1 .. K (matplotlib's acorr), through np.correlate"""
    q = np.asarray(q, dtype=np.float64)
    N = len(q)
    full = np.correlate(q, q, mode="full")          # lag k at index N - 1 + k
    return full[N:N + K] / full[N - 1]


def ks_case(N):
    """the rows of the KS test of tests/test_whiten_gpu.py (scripts/whiten_probe.py measures the device's erfc at their
    q): a white model with log sigma = -0.3 on synthetic.make_lightcurves(N, 1, seed=33); row 0 standard normals through
    it, row 1 a constant q = 0.37, row 2 the light curve's own scatter at 1.3 sigma -> (t, y, dy, theta [3][1], data [3][N])"""
    from mind_the_gaps_amd import synthetic as synth
    t, y, dy = synth.make_lightcurves(N, 1, seed=33)
    sd = np.sqrt((dy[0] + 1e-12) ** 2 + np.exp(2.0 * -0.3))
    data = np.vstack([sd * np.random.default_rng(N).standard_normal(N), 0.37 * sd, (y[0] - 100.0) / 10.0 * sd * 1.3])
    return t, y, dy, np.full((3, 1), -0.3), data


def dense_whiten(t, dy, coeffs, y, mean=0.0):
    """the dense float64 route: chol(K) q = y - mean, and ln det K = 2 sum ln diag(chol)"""
    from oracle import dense
    t = np.asarray(t, dtype=np.float64)
    K = dense.kernel_value(coeffs, t[:, None] - t[None, :])
    K[np.diag_indices_from(K)] += R.diagonal(dy, coeffs)
    Lc = np.linalg.cholesky(K)
    r = np.asarray(y, dtype=np.float64) - mean
    q = np.empty(len(t))
    for n in range(len(t)):                         # forward substitution
        q[n] = (r[n] - Lc[n, :n] @ q[:n]) / Lc[n, n]
    return q, 2.0 * float(np.sum(np.log(np.diag(Lc))))


# ---- mpmath ---------------------------------------------------------------------------------------------------------

def mp_whiten(t, dy, coeffs, y, mean_kind=0, mean_params=(0.0,), dps=40):
    """the recurrence in mpmath at ``dps`` digits, phases at the absolute time (exact there) -> dict of float64 arrays:
    q [N] the truth; scale [N], s_n = (|r_n| + sum_i |U_ni f_ni|) / sqrt(D_n); D [N]; and the truths of the two sums the
    likelihood is made of with the sums of their terms' magnitudes: sum2, logdet, logdet_abs (sum2 is its own);
    and the status: 0, or 2 when a pivot is not positive"""
    import mpmath as mp
    with mp.workdps(dps):
        f64 = lambda x: mp.mpf(float(x))
        sl = [(f64(a), f64(b), f64(c), f64(d), kind) for a, b, c, d, kind in R.slots(coeffs)]
        J, N = len(sl), len(t)
        tt = [f64(x) for x in t]
        k0 = sum((f64(a) for a in coeffs[0]), mp.mpf(0)) + sum((f64(a) for a in coeffs[2]), mp.mpf(0))
        jit = f64(coeffs[6])
        S = [[mp.mpf(0)] * J for _ in range(J)]
        f, Wp, Dp, vp = [mp.mpf(0)] * J, [mp.mpf(0)] * J, mp.mpf(1), mp.mpf(0)
        q, scale, Dout = np.empty(N), np.empty(N), np.empty(N)
        sum1 = sum2 = sum3 = sum4 = logdet = logdet_abs = mp.mpf(0)
        for n in range(N):
            dx = tt[n] - tt[n - 1] if n > 0 else mp.mpf(0)
            ph, U, V = [None] * J, [None] * J, [None] * J
            for i, (a, b, c, d, kind) in enumerate(sl):
                if kind == 0:
                    ph[i], U[i], V[i] = mp.exp(-c * dx), a, mp.mpf(1)
                elif kind == 1:
                    cn, sn = mp.cos(d * tt[n]), mp.sin(d * tt[n])
                    e = mp.exp(-c * dx)
                    ph[i], U[i], V[i] = e, a * cn + b * sn, cn
                    ph[i + 1], U[i + 1], V[i + 1] = e, a * sn - b * cn, sn
            for i in range(J):
                for j in range(i + 1):
                    S[i][j] = S[j][i] = ph[i] * ph[j] * (S[i][j] + Dp * Wp[i] * Wp[j])
                f[i] = ph[i] * (f[i] + Wp[i] * vp)
            SU = [mp.fdot(S[i], U) for i in range(J)]
            D = (f64(np.float64(dy[n]) + np.float64(1e-12))) ** 2 + jit + k0 - mp.fdot(U, SU)
            if not D > 0:
                return None, 2
            Wp = [(V[i] - SU[i]) / D for i in range(J)]
            mean = f64(mean_params[0]) * tt[n] + f64(mean_params[1]) if mean_kind == 1 else f64(mean_params[0])
            r = f64(y[n]) - mean
            vp = r - mp.fdot(U, f)
            root = mp.sqrt(D)
            qn = vp / root
            q[n], Dout[n] = float(qn), float(D)
            scale[n] = float((abs(r) + sum((abs(U[i] * f[i]) for i in range(J)), mp.mpf(0))) / root)
            sum1 += qn; sum2 += qn * qn; sum3 += qn ** 3; sum4 += qn ** 4
            logdet += mp.log(D); logdet_abs += abs(mp.log(D))
            Dp = D
        return dict(q=q, scale=scale, D=Dout, sum1=float(sum1), sum2=float(sum2), sum3=float(sum3), sum4=float(sum4),
                    logdet=float(logdet), logdet_abs=float(logdet_abs)), 0


def mp_dense_whiten(t, dy, coeffs, y, mean_kind=0, mean_params=(0.0,), dps=50):
    """mpmath dense Cholesky of K (small N): q from chol(K) q = y - mean by forward substitution, rounded to float64 (K
    is built as gp_draw_replay.mp_dense_draw builds it: the functions of t_i - t_j from their values at t_i and t_j)"""
    import mpmath as mp
    with mp.workdps(dps):
        f64 = lambda x: mp.mpf(float(x))
        N = len(t)
        tt = [f64(x) for x in t]
        K = [[mp.mpf(0)] * (i + 1) for i in range(N)]
        ar, cr, ac, bc, cc, dc, jitter = coeffs
        terms = [(f64(a), mp.mpf(0), f64(c), mp.mpf(0)) for a, c in zip(ar, cr)]
        terms += [(f64(a), f64(b), f64(c), f64(d)) for a, b, c, d in zip(ac, bc, cc, dc)]
        for a, b, c, d in terms:
            E = [mp.exp(-c * (x - tt[0])) for x in tt]
            Ei = [1 / e for e in E]
            C = [mp.cos(d * x) for x in tt]
            Sn = [mp.sin(d * x) for x in tt]
            for i in range(N):
                row = K[i]
                for j in range(i + 1):
                    cosd = C[i] * C[j] + Sn[i] * Sn[j]
                    sind = Sn[i] * C[j] - C[i] * Sn[j]
                    row[j] += E[i] * Ei[j] * (a * cosd + b * sind)
        for i in range(N):
            K[i][i] += f64(np.float64(dy[i]) + np.float64(1e-12)) ** 2 + f64(jitter)
        Lc = [[mp.mpf(0)] * (i + 1) for i in range(N)]
        for i in range(N):
            for j in range(i + 1):
                s = K[i][j] - mp.fdot(Lc[i][:j], Lc[j][:j])
                Lc[i][j] = mp.sqrt(s) if i == j else s / Lc[j][j]
        q = []
        for i in range(N):
            mean = f64(mean_params[0]) * tt[i] + f64(mean_params[1]) if mean_kind == 1 else f64(mean_params[0])
            q.append((f64(y[i]) - mean - mp.fdot(Lc[i][:i], q)) / Lc[i][i])
        return np.array([float(v) for v in q])
