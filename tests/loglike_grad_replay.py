"""Host replay of the analytic gradient of the log-likelihood (csrc/mtg_loglike_grad.hip) in float64 numpy: the
coefficient tangents of csrc/mtg_prepare_tangent.h and the tangent recurrence of csrc/mtg_factor_step_tangent.h, all
free parameters of a row at once (the device gives each a lane).

Notation of csrc/mtg_gp_draw.hip (W normalised by D), dots for d/dtheta_p:

    S_n = phi phi^T o (S_{n-1} + D_{n-1} W_{n-1} W_{n-1}^T),   f_n = phi o (f_{n-1} + W_{n-1} z_{n-1})
    D_n = sigma_n^2 + asum - U^T S U,   W_n = (V - S U) / D_n,   z_n = y_n - mean(t_n) - U^T f_n
    lnL = -1/2 sum (z^2 / D + ln D) - N/2 ln 2 pi

    phi' = -(c' dx) phi,   D' = asum' - 2 U'^T S U - U^T S' U,   W' = (V' - S' U - S U' - W D') / D
    z' = -mean' - U'^T f - U^T f',   dlnL/dtheta_p = -1/2 sum (2 z z' / D - z^2 D' / D^2 + D' / D)

A frequency d enters the generators of its (cos, sin) pair through the phase d (t_n - t_0), so its tangent carries the
elapsed time as a factor: x' = x~ + d' (t_n - t_0) R x for every vector x of the pair (U, V, f, W, rows and columns of
S), R the quarter turn (x_cos, x_sin) -> (-x_sin, x_cos).  The scalars D and z do not turn, so these terms cancel in
every sample's contribution -- after having been formed at a size of (t_n - t_0) / lag times what is left.  Two forms:

    frame="elapsed"   x' itself is carried, U' and V' with the elapsed time in them
    frame="rotated"   x~ is carried (the device's form): U~ and V~ hold only a', b', and each step turns the carried
                      tangents by the lag alone, f~ -= d' dx R f, S~ -= d' dx (R S + S R^T)

Both give the same derivative; they differ in rounding (tests/test_loglike_grad_cpu.py measures both).

The error scale of component p is G_p = 1/2 sum_n (|2 z z' / D| + |z^2 D' / D^2| + |D' / D|): a scale, never an
expected value."""
import numpy as np

import gp_draw_replay
from oracle.dense import (K_BPL, K_COMPLEX3, K_COMPLEX4, K_COSINUS, K_DRW, K_JITTER, K_LORENTZIAN, K_MATERN32, K_REAL,
                          K_SHO, NPARAMS)

KEYS = ("ar", "cr", "ac", "bc", "cc", "dc")


def coefficients(kinds, full, mean_kind=0, extra=None):
    """full [PF] (kernel parameters, then the mean's) -> (coef, dcoef): coef a dict of ar, cr (real slots), ac, bc,
    cc, dc (complex slots), asum (sum a + jitter), jit, slope, icpt in the device's slot order (a Lorentzian's empty
    real term is not expanded); dcoef the same keys with a leading axis [PF], the derivative by every parameter."""
    full = np.asarray(full, dtype=np.float64)
    PF = len(full)
    val = {k: [] for k in KEYS}
    der = {k: [] for k in KEYS}          # per slot: {parameter index: derivative}
    jit, djit = 0.0, {}
    off = 0
    for i, kind in enumerate(kinds):
        o = off
        p = full[o:o + NPARAMS[kind]]
        off += NPARAMS[kind]

        def real(a, c, da, dc):
            val["ar"].append(a); val["cr"].append(c); der["ar"].append(da); der["cr"].append(dc)

        def comp(a, b, c, d, da, db, dc, dd):
            for k, v, dv in (("ac", a, da), ("bc", b, db), ("cc", c, dc), ("dc", d, dd)):
                val[k].append(v); der[k].append(dv)

        if kind in (K_REAL, K_DRW):
            a, c = np.exp(p[0]), (np.exp(p[1]) if kind == K_REAL else 0.5 * np.exp(p[1]) / 0.5)
            real(a, c, {o: a}, {o + 1: c})
        elif kind == K_COMPLEX3:
            a, c, d = np.exp(p)
            comp(a, 0.0, c, d, {o: a}, {}, {o + 1: c}, {o + 2: d})
        elif kind == K_COMPLEX4:
            a, b, c, d = np.exp(p)
            comp(a, b, c, d, {o: a}, {o + 1: b}, {o + 2: c}, {o + 3: d})
        elif kind == K_SHO:
            S0, Q, w0 = np.exp(p)
            if Q < 0.5:
                f = np.sqrt(1.0 - 4.0 * Q * Q)
                h = 0.5 * S0 * w0 * Q
                a1, a2 = h * (1.0 + 1.0 / f), h * (1.0 - 1.0 / f)
                c1, c2 = 0.5 * w0 / Q * (1.0 - f), 0.5 * w0 / Q * (1.0 + f)
                g = 4.0 * Q * Q / f                   # -df/dlnQ; d(1/f)/dlnQ = g / f^2
                real(a1, c1, {o: a1, o + 1: a1 + h * g / (f * f), o + 2: a1}, {o + 1: -c1 + 0.5 * w0 / Q * g, o + 2: c1})
                real(a2, c2, {o: a2, o + 1: a2 - h * g / (f * f), o + 2: a2}, {o + 1: -c2 - 0.5 * w0 / Q * g, o + 2: c2})
            else:
                f = np.sqrt(4.0 * Q * Q - 1.0)
                a = S0 * w0 * Q
                b, c = a / f, 0.5 * w0 / Q
                d = c * f
                g = 4.0 * Q * Q / (f * f)             # dlnf/dlnQ
                comp(a, b, c, d, {o: a, o + 1: a, o + 2: a}, {o: b, o + 1: b * (1.0 - g), o + 2: b},
                     {o + 1: -c, o + 2: c}, {o + 1: d * (g - 1.0), o + 2: d})
        elif kind == K_MATERN32:
            eps = 0.01 if extra is None else extra[i]
            w0 = np.sqrt(3.0) * np.exp(-p[1])
            S0 = np.exp(2.0 * p[0]) / w0
            a, b = w0 * S0, w0 * w0 * S0 / eps
            comp(a, b, w0, eps, {o: 2.0 * a}, {o: 2.0 * b, o + 1: -b}, {o + 1: -w0}, {})
        elif kind == K_JITTER:
            jv = np.exp(2.0 * p[0])
            jit += jv
            djit[o] = djit.get(o, 0.0) + 2.0 * jv
        elif kind == K_LORENTZIAN:
            a, w0 = np.exp(p[0]), np.exp(p[2])
            c = 0.5 * w0 / np.exp(p[1])
            comp(a, 0.0, c, w0, {o: a}, {}, {o + 1: -c, o + 2: c}, {o + 2: w0})
        elif kind == K_COSINUS:
            a, d = np.exp(p)
            comp(a, 0.0, 0.0, d, {o: a}, {}, {}, {o + 1: d})
        elif kind == K_BPL:
            a, b, w0 = np.exp(p)
            comp(a, b, w0, w0, {o: a}, {o + 1: b}, {o + 2: w0}, {o + 2: w0})
        else:
            raise ValueError("unknown term kind %r" % (kind,))
    nk = off
    coef = {k: np.asarray(v, dtype=np.float64) for k, v in val.items()}
    dcoef = {}
    for k in KEYS:
        dcoef[k] = np.zeros((PF, len(val[k])))
        for s, dv in enumerate(der[k]):
            for q, x in dv.items():
                dcoef[k][q, s] = x
    coef["jit"] = jit
    dcoef["jit"] = np.zeros(PF)
    for q, x in djit.items():
        dcoef["jit"][q] = x
    coef["asum"] = float(np.sum(coef["ar"]) + np.sum(coef["ac"]) + jit)
    dcoef["asum"] = dcoef["ar"].sum(axis=1) + dcoef["ac"].sum(axis=1) + dcoef["jit"]
    dcoef["slope"], dcoef["icpt"] = np.zeros(PF), np.zeros(PF)
    if mean_kind == 1:
        coef["slope"], coef["icpt"] = float(full[nk]), float(full[nk + 1])
        dcoef["slope"][nk], dcoef["icpt"][nk + 1] = 1.0, 1.0
    else:
        coef["slope"], coef["icpt"] = 0.0, float(full[nk])
        dcoef["icpt"][nk] = 1.0
    return coef, dcoef


def as_dense(coef):
    """the tuple oracle.dense.build_coeffs returns (without a Lorentzian's empty real term)"""
    return tuple(coef[k] for k in KEYS) + (coef["jit"],)


def _slots(coef, dcoef, free_index):
    """per slot (real slots, then (cos, sin) pairs): a, b, c, d [J], their tangents [P][J], sg [J] (-1 cos, +1 sin,
    0 real) and pi [J], the slot's partner: R x = sg * x[pi]"""
    nr, nc = len(coef["ar"]), len(coef["ac"])
    J = nr + 2 * nc
    P = len(free_index)
    v = {k: np.zeros(J) for k in "abcd"}
    dv = {k: np.zeros((P, J)) for k in "abcd"}
    sg, pi = np.zeros(J), np.arange(J)
    v["a"][:nr], v["c"][:nr] = coef["ar"], coef["cr"]
    dv["a"][:, :nr], dv["c"][:, :nr] = dcoef["ar"][free_index], dcoef["cr"][free_index]
    for q in range(nc):
        for s in (0, 1):
            i = nr + 2 * q + s
            for k in "abcd":
                v[k][i] = coef[k + "c"][q]
                dv[k][:, i] = dcoef[k + "c"][free_index, q]
            sg[i], pi[i] = (-1.0, i + 1) if s == 0 else (1.0, i - 1)
    return v, dv, sg, pi


def loglike_grad(t, y, dy, kinds, full, free_index, mean_kind=0, extra=None, frame="rotated"):
    """-> (lnL, grad [P], G [P], status): y is the light curve as the device holds it (its y_offset taken off), dy as
    given to the reference (sigma = dy + 1e-12); status 2 and (-inf, NaN, NaN) at a non-positive pivot."""
    if frame not in ("rotated", "elapsed"):
        raise ValueError(frame)
    t, y = np.asarray(t, dtype=np.float64), np.asarray(y, dtype=np.float64)
    free_index = np.asarray(free_index, dtype=np.int64)
    coef, dcoef = coefficients(kinds, full, mean_kind, extra)
    v, dv, sg, pi = _slots(coef, dcoef, free_index)
    a, b, c, d = (v[k] for k in "abcd")
    da, db, dc, dd = (dv[k] for k in "abcd")
    dasum, dslope, dicpt = (dcoef[k][free_index] for k in ("asum", "slope", "icpt"))
    N, J, P = len(t), len(a), len(free_index)
    diag = (np.asarray(dy, dtype=np.float64) + 1e-12) ** 2
    cn, sn = np.ones((N, J)), np.zeros((N, J))
    for i in range(J):
        if sg[i] != 0.0:
            arg = gp_draw_replay.reduced_phase(d[i], t - t[0])
            cn[:, i], sn[:, i] = np.cos(arg), np.sin(arg)
    S, f, Wp, Dp, zp = np.zeros((J, J)), np.zeros(J), np.zeros(J), 1.0, 0.0
    dS, df, dWp, dDp, dzp = np.zeros((P, J, J)), np.zeros((P, J)), np.zeros((P, J)), np.zeros(P), np.zeros(P)
    lnL, grad, G = 0.0, np.zeros(P), np.zeros(P)
    with np.errstate(under="ignore"):
        for n in range(N):
            dx = t[n] - t[n - 1] if n > 0 else 0.0
            ph = np.exp(-c * dx)
            # generators: V = (1 | cos | sin), U = (a | a cos + b sin | a sin - b cos)
            V = np.where(sg == 0.0, 1.0, np.where(sg < 0.0, cn[n], sn[n]))
            U = a * V - sg * b * V[pi]
            dU = da * V - sg * db * V[pi]
            dV = np.zeros((P, J))
            if frame == "elapsed":
                turn = dd * (t[n] - t[0])
                dU = dU + turn * sg * U[pi]
                dV = turn * sg * V[pi]
            # forward step
            WW = np.outer(Wp, Wp)
            T = S + Dp * WW
            dT = dS + dDp[:, None, None] * WW + Dp * (dWp[:, :, None] * Wp[None, None, :] + Wp[None, :, None] * dWp[:, None, :])
            PP = np.outer(ph, ph)
            rate = -(dc * dx)
            dS = PP * ((rate[:, :, None] + rate[:, None, :]) * T + dT)
            S = PP * T
            g = f + Wp * zp
            df = ph * (rate * g + df + dWp * zp + Wp[None, :] * dzp[:, None])
            f = ph * g
            if frame == "rotated":
                lag = dd * dx
                RS = sg[:, None] * S[pi, :]
                dS = dS - (lag[:, :, None] * RS[None] + lag[:, None, :] * RS.T[None])
                df = df - lag * (sg * f[pi])
            # pivot
            q = S @ U
            dq = dS @ U + dU @ S
            D = diag[n] + coef["asum"] - U @ q
            dD = dasum - dU @ q - dq @ U
            if not D > 0.0:
                return -np.inf, np.full(P, np.nan), np.full(P, np.nan), 2
            W = (V - q) / D
            dW = (dV - dq - W[None, :] * dD[:, None]) / D
            z = y[n] - (coef["slope"] * t[n] + coef["icpt"]) - U @ f
            dz = -(dslope * t[n] + dicpt) - dU @ f - df @ U
            lnL += z * z / D + np.log(D)
            t1, t2, t3 = 2.0 * z * dz / D, z * z * dD / (D * D), dD / D
            grad += t1 - t2 + t3
            G += np.abs(t1) + np.abs(t2) + np.abs(t3)
            Wp, Dp, zp, dWp, dDp, dzp = W, D, z, dW, dD, dz
    return -0.5 * lnL - 0.5 * N * np.log(2.0 * np.pi), -0.5 * grad, 0.5 * G, 0


def quad_gradient(t, y, dy, kinds, full, free_index, mean_kind=0, extra=None, step=1e-10):
    """the truth: central differences of the quad-precision oracle, its two parts differenced separately;
    y is the light curve with its y_offset taken off (the oracle is handed a mean that includes none)"""
    from oracle import quad
    full = np.asarray(full, dtype=np.float64)
    P = len(free_index)
    pts = np.tile(full, (2 * P, 1))
    for p, k in enumerate(free_index):
        pts[2 * p, k] += step
        pts[2 * p + 1, k] -= step
    hi, lo, _, status = quad.loglike(t, y, dy, kinds, pts, mean_kind=mean_kind, extra=extra)
    assert np.all(status == 0), status
    h = np.array([pts[2 * p, k] - pts[2 * p + 1, k] for p, k in enumerate(free_index)])
    return ((hi[0::2] - hi[1::2]) + (lo[0::2] - lo[1::2])) / h
