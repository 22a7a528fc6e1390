"""Host replay of the GP draw (csrc/mtg_gp_draw.hip): y = mean + L sqrt(D) q from celerite's factorisation
K = L diag(D) L^T, L = I + tril(U W^T), in float64 numpy (the factorisation's accumulations optionally as float64 pairs:
factor), and the same in mpmath; the Philox counters and the Box-Muller
pairs of the device-drawn normals (integer-exact blocks, philox_replay.philox); the inverse (L sqrt(D))^-1.

    S_n = phi_n phi_n^T o (S_{n-1} + D_{n-1} W_{n-1} W_{n-1}^T),  W_n = (V_n - S_n U_n) / D_n,
    D_n = diag_n + k(0) - U_n^T S_n U_n,                           diag_n = sigma_n^2 + jitter
    f_n = phi_n o (f_{n-1} + W_{n-1} v_{n-1}),  v_n = sqrt(D_n) q_n,  y_n = mean_n + v_n + U_n^T f_n

Coefficients are celerite's (oracle.dense.build_coeffs); slots are the real terms, then (cos, sin) pairs of the complex
ones.  The phases are those of the elapsed time t_n - t_0 (phase="elapsed", what the device does) or of the absolute
time (phase="absolute", celerite's own: the float64 baseline c64 of tests/golden/gp_draw_golden.npz)."""
import numpy as np

import philox_replay

PURPOSE_GP_DRAW = 12


def slots(coeffs):
    """(a, b, c, d, kind) per slot: kind 0 real, 1 the cos slot of a complex term, 2 its sin slot"""
    ar, cr, ac, bc, cc, dc, _ = coeffs
    out = [(a, 0.0, c, 0.0, 0) for a, c in zip(ar, cr)]
    for a, b, c, d in zip(ac, bc, cc, dc):
        out += [(a, b, c, d, 1), (a, b, c, d, 2)]
    return out


def _two_prod(a, b):
    """a b = p + e exactly (Dekker's product on Veltkamp splits: no fused multiply-add in numpy)"""
    p = a * b
    ca, cb = 134217729.0 * a, 134217729.0 * b
    ah, bh = ca - (ca - a), cb - (cb - b)
    al, bl = a - ah, b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def reduced_phase(d, th):
    """d th modulo 2 pi, reduced BEFORE it is rounded, as the device's mtg_elapsed_sincos does: the product exactly as
    p + e, k = rint(p / 2 pi), then p - k C1 - k C2 + e with C1 + C2 = 2 pi to 106 bits.  (Formed plainly, d th is
    rounded at its own magnitude: 3e-14 rad at 400 rad, 250 u in the generators.)"""
    th = np.asarray(th, dtype=np.float64)
    p, e = _two_prod(np.float64(d), th)
    k = np.rint(p * 0.15915494309189535)
    h, l = _two_prod(k, np.float64(6.283185307179586))
    return ((p - h) - l) - k * 2.4492935982947064e-16 + e


def generators(coeffs, t, phase="elapsed"):
    """U [N][J], V [N][J], c [J] in float64"""
    t = np.asarray(t, dtype=np.float64)
    sl = slots(coeffs)
    U, V = np.empty((len(t), len(sl))), np.empty((len(t), len(sl)))
    for i, (a, b, c, d, kind) in enumerate(sl):
        if kind == 0:
            U[:, i], V[:, i] = a, 1.0
            continue
        arg = reduced_phase(d, t - t[0]) if phase == "elapsed" else d * t      # t - t[0] is exact
        cn, sn = np.cos(arg), np.sin(arg)
        if kind == 1:
            U[:, i], V[:, i] = a * cn + b * sn, cn
        else:
            U[:, i], V[:, i] = a * sn - b * cn, sn
    return U, V, np.array([s[2] for s in sl], dtype=np.float64)


def k0_of(coeffs):
    return float(np.sum(coeffs[0]) + np.sum(coeffs[2]))


def diagonal(dy, coeffs):
    """sigma^2 + jitter with sigma = dy + 1e-12 (what GP.compute is given)"""
    return (np.asarray(dy, dtype=np.float64) + 1e-12) ** 2 + coeffs[6]


# float64 pairs (hi, lo), hi + lo the value: error-free sums and products of float64 numbers (Dekker, Knuth)
def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _norm(h, l):
    s = h + l
    return s, l - (s - h)


def _dd_add(a, b):
    s, e = _two_sum(a[0], b[0])
    return _norm(s, e + (a[1] + b[1]))


def _dd_mul(a, b):
    p, e = _two_prod(a[0], b[0])
    return _norm(p, e + (a[0] * b[1] + a[1] * b[0]))


def _dd_div(a, b):
    q1 = a[0] / b[0]
    r = _dd_add(a, tuple(-x for x in _dd_mul(b, (q1, 0.0))))
    return _norm(q1, r[0] / b[0])


def _dd_sum(a, axis):
    """sum of the pairs a = (hi, lo) along an axis (a handful of terms: the rank J)"""
    h, l = np.moveaxis(a[0], axis, 0), np.moveaxis(a[1], axis, 0)
    out = (h[0], l[0])
    for i in range(1, len(h)):
        out = _dd_add(out, (h[i], l[i]))
    return out


def factor(t, diag, coeffs, phase="elapsed", compensated=True):
    """factorisation -> U [N][J], W [N][J] (normalised by D), ph [N][J], D [N], all float64.

    compensated=False is the recurrence as written, in float64: what celerite and the device compute (the float64
    baseline c64 of tests/golden/gp_draw_golden.npz).  Its pivot D_n = diag_n + k(0) - U_n^T S_n U_n takes the rounding
    of every entry of S times |U_i U_j|: with celerite's Matern-3/2 term (b / a = w0 / eps = 22 at eps = 0.01, |U|^2 =
    470 k(0)) D_n carries 2000 u where the dense Cholesky of K carries 10 u.  compensated=True (the replay the tests hold
    the device to) carries S, S U, D and W as float64 pairs with error-free sums and products, so that what is left is
    the rounding of the generators themselves; the results are rounded to float64."""
    t = np.asarray(t, dtype=np.float64)
    U, V, c = generators(coeffs, t, phase)
    N, J = U.shape
    dx = np.concatenate([[0.0], np.diff(t)])
    ph = np.exp(-c[None, :] * dx[:, None])
    k0 = k0_of(coeffs)
    W, D = np.empty((N, J)), np.empty(N)
    if not compensated:
        S, Wp, Dp = np.zeros((J, J)), np.zeros(J), 1.0
        for n in range(N):
            S = np.outer(ph[n], ph[n]) * (S + Dp * np.outer(Wp, Wp))
            SU = S @ U[n]
            D[n] = diag[n] + k0 - U[n] @ SU
            W[n] = (V[n] - SU) / D[n]
            Wp, Dp = W[n], D[n]
        return U, W, ph, D
    z = np.zeros((J, J))
    S, Wp, Dp = (z, z.copy()), (np.zeros(J), np.zeros(J)), (np.float64(1.0), np.float64(0.0))
    with np.errstate(under="ignore"):
        for n in range(N):
            PP = _two_prod(ph[n][:, None], ph[n][None, :])
            WW = _dd_mul((Wp[0][:, None], Wp[1][:, None]), (Wp[0][None, :], Wp[1][None, :]))
            S = _dd_mul(PP, _dd_add(S, _dd_mul(Dp, WW)))
            SU = _dd_sum(_dd_mul(S, (U[n][None, :], 0.0)), 1)
            UtSU = _dd_sum(_dd_mul(SU, (U[n], 0.0)), 0)
            Dp = _dd_add(_two_sum(np.float64(diag[n]), np.float64(k0)), (-UtSU[0], -UtSU[1]))
            Wp = _dd_div(_dd_add((V[n], np.zeros(J)), (-SU[0], -SU[1])), Dp)
            D[n], W[n] = Dp[0], Wp[0]
    return U, W, ph, D


def draw(t, dy, coeffs, q, mean=0.0, phase="elapsed", factors=None):
    """float64 replay: q [B][N] or [N] standard normals -> y of the same shape; mean: scalar or [N]"""
    q2 = np.atleast_2d(np.asarray(q, dtype=np.float64))
    U, W, ph, D = factors if factors is not None else factor(t, diagonal(dy, coeffs), coeffs, phase)
    N, J = U.shape
    v = np.sqrt(D)[None, :] * q2
    y = np.empty_like(q2)
    f = np.zeros((q2.shape[0], J))
    for n in range(N):
        if n > 0:
            f = ph[n][None, :] * (f + W[n - 1][None, :] * v[:, n - 1][:, None])
        y[:, n] = v[:, n] + f @ U[n]
    y = np.broadcast_to(np.asarray(mean, dtype=np.float64), (N,))[None, :] + y
    return y if np.ndim(q) == 2 else y[0]


def whiten(t, dy, coeffs, y, mean=0.0, phase="elapsed", factors=None):
    """the inverse (L sqrt(D))^-1 (y - mean): the normals a draw was made from"""
    y2 = np.atleast_2d(np.asarray(y, dtype=np.float64)) - np.broadcast_to(np.asarray(mean, dtype=np.float64), (len(t),))[None, :]
    U, W, ph, D = factors if factors is not None else factor(t, diagonal(dy, coeffs), coeffs, phase)
    N, J = U.shape
    v = np.empty_like(y2)
    f = np.zeros((y2.shape[0], J))
    for n in range(N):
        if n > 0:
            f = ph[n][None, :] * (f + W[n - 1][None, :] * v[:, n - 1][:, None])
        v[:, n] = y2[:, n] - f @ U[n]
    q = v / np.sqrt(D)[None, :]
    return q if np.ndim(y) == 2 else q[0]


def scale_at(t, coeffs, factors, q, idx):
    """s_n = sum_m |L_nm sqrt(D_m) q_m| at the samples idx, L_nm = sum_i U_ni W_mi exp(-c_i (t_n - t_m)) (m < n), 1 (m = n);
    q [N] -> [len(idx)]"""
    t = np.asarray(t, dtype=np.float64)
    U, W, ph, D = factors
    c = np.array([s[2] for s in slots(coeffs)], dtype=np.float64)
    v = np.sqrt(D) * np.asarray(q, dtype=np.float64)
    out = np.empty(len(idx))
    for k, n in enumerate(idx):
        n = int(n)
        with np.errstate(under="ignore"):
            L = np.einsum("i,mi,mi->m", U[n], W[:n], np.exp(-c[None, :] * (t[n] - t[:n])[:, None]))
        out[k] = abs(v[n]) + np.sum(np.abs(L * v[:n]))
    return out


def dense_draw(t, dy, coeffs, q, mean=0.0):
    """the dense float64 route: np.linalg.cholesky(K) @ q + mean, and the scale s_n = sum_m |chol_nm q_m|"""
    from oracle import dense
    t = np.asarray(t, dtype=np.float64)
    K = dense.kernel_value(coeffs, t[:, None] - t[None, :])
    K[np.diag_indices_from(K)] += diagonal(dy, coeffs)
    Lc = np.linalg.cholesky(K)
    q = np.asarray(q, dtype=np.float64)
    return Lc @ q + mean, np.abs(Lc * q[None, :]).sum(axis=1)


# ---- mpmath ---------------------------------------------------------------------------------------------------------

def mp_draw(t, dy, coeffs, q, mean_kind=0, mean_params=(0.0,), dps=40, keep=None):
    """the recurrence in mpmath at ``dps`` digits, phases at the absolute time (exact there) -> y [N] rounded to
    float64 (keep: only these samples), and the status: 0, or 2 when a pivot is not positive"""
    import mpmath as mp
    with mp.workdps(dps):
        f64 = lambda x: mp.mpf(float(x))
        sl = [(f64(a), f64(b), f64(c), f64(d), kind) for a, b, c, d, kind in slots(coeffs)]
        J, N = len(sl), len(t)
        tt = [f64(x) for x in t]
        k0 = sum((f64(a) for a in coeffs[0]), mp.mpf(0)) + sum((f64(a) for a in coeffs[2]), mp.mpf(0))
        jit = f64(coeffs[6])
        S = [[mp.mpf(0)] * J for _ in range(J)]
        f, Wp, Dp, vp = [mp.mpf(0)] * J, [mp.mpf(0)] * J, mp.mpf(1), mp.mpf(0)
        out = np.empty(N)
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
            vp = mp.sqrt(D) * f64(q[n])
            mean = f64(mean_params[0]) * tt[n] + f64(mean_params[1]) if mean_kind == 1 else f64(mean_params[0])
            out[n] = float(mean + vp + mp.fdot(U, f))
            Dp = D
        return (out if keep is None else out[np.asarray(keep)]), 0


def mp_dense_draw(t, dy, coeffs, q, mean_kind=0, mean_params=(0.0,), dps=50):
    """mpmath dense Cholesky of K (small N): chol(K) q + mean, rounded to float64.  exp(-c (t_i - t_j)) and the
    trigonometric functions of d (t_i - t_j) come from their values at t_i and t_j (exact identities; mpmath's exponent
    range has no underflow)."""
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
        qq = [f64(x) for x in q]
        out = np.empty(N)
        for i in range(N):
            mean = f64(mean_params[0]) * tt[i] + f64(mean_params[1]) if mean_kind == 1 else f64(mean_params[0])
            out[i] = float(mean + mp.fdot(Lc[i], qq[:i + 1]))
        return out


# ---- the device's normals --------------------------------------------------------------------------------------------

def philox_blocks(seed, draw_index, N):
    """the four 32-bit words of the blocks of samples (2k, 2k + 1), k = 0 .. ceil(N / 2) - 1, of the draw with global
    index draw_index: counter (k, PURPOSE_GP_DRAW, low word, high word of draw_index), key = seed"""
    k = np.arange((N + 1) // 2, dtype=np.uint64)
    g = int(draw_index) & 0xFFFFFFFFFFFFFFFF
    return philox_replay.philox(k, PURPOSE_GP_DRAW, g & 0xFFFFFFFF, g >> 32, int(seed))


def philox_normals(seed, draw_index, N):
    """Box-Muller on the replayed blocks: u1 = 1 - u01(r0, r1) in (0, 1], u2 = u01(r2, r3); q_2k = rad cos(2 pi u2),
    q_2k+1 = rad sin(2 pi u2), rad = sqrt(-2 ln u1)"""
    r = philox_blocks(seed, draw_index, N)
    u1 = 1.0 - philox_replay.u01(r[0], r[1])
    u2 = philox_replay.u01(r[2], r[3])
    rad = np.sqrt(-2.0 * np.log(u1))
    q = np.empty(2 * len(u1))
    # sin / cos of 2 pi u2 with the argument reduced to [-1/4, 1/4] turns first: exact, as sincospi does it
    q[0::2], q[1::2] = rad * cospi(2.0 * u2), rad * sinpi(2.0 * u2)
    return q[:N]


def _reduce(x):
    """x (turns of pi) -> (r, quadrant) with x pi = r pi + quadrant pi / 2, |r| <= 1/4: exact in float64"""
    k = np.rint(2.0 * x)
    return x - 0.5 * k, k.astype(np.int64) & 3


def sinpi(x):
    r, k = _reduce(np.asarray(x, dtype=np.float64))
    s, c = np.sin(np.pi * r), np.cos(np.pi * r)
    return np.choose(k, [s, c, -s, -c])


def cospi(x):
    r, k = _reduce(np.asarray(x, dtype=np.float64))
    s, c = np.sin(np.pi * r), np.cos(np.pi * r)
    return np.choose(k, [c, -s, -c, s])
