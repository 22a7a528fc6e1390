"""Host replay of the simulator's random draws and spectra (csrc/mtg_simulate.hip, csrc/mtg_e13.hip): the same Philox
counters (philox_replay.py), the kernels' float64 arithmetic restated in numpy branch for branch, and mpmath twins of the
draws and of the spectrum at 40 digits.  The replay is the specification the device is held to
(test_simulator_replay_gpu.py); test_simulator_replay_cpu.py checks the replay itself.

Counters: (c0, purpose, global series index, c3).  Noise (purpose 10): c0 = epoch, c3 = 0 for the Gaussian draw and
1, 2, ... for the trips of the Poisson loops.  E13's own draws (purpose 11): c0 = pair index, c3 = its high word."""
import mpmath
import numpy as np
from scipy.special import gammaln

import philox_replay

NOISE, E13 = 10, 11
KNUTH_TRIPS, PTRS_TRIPS = 63, 255        # `ctr < 64`, `ctr < 256` from ctr = 1
DIGITS = 40
EPS = 2.0 ** -52

# term kinds of mind_the_gaps_amd.synthetic / csrc/mtg_prepare.h
K_REAL, K_COMPLEX3, K_COMPLEX4, K_SHO, K_MATERN32, K_JITTER, K_DRW, K_LORENTZIAN = range(8)
NPARAMS = {K_REAL: 2, K_COMPLEX3: 3, K_COMPLEX4: 4, K_SHO: 3, K_MATERN32: 2, K_JITTER: 1, K_DRW: 2, K_LORENTZIAN: 3}
MATERN_EPS = 0.01                        # mtg_set_model's default `extra` of a Matern-3/2 term


# ---- uniforms and normals -------------------------------------------------------------------------------------------
def block(c0, purpose, series, c3, seed):
    """One Philox block per element of the broadcast counters -> (ua, ub): the two uniforms in [0, 1) of u01."""
    r = philox_replay.philox(c0, purpose, series, c3, seed)
    return philox_replay.u01(r[0], r[1]), philox_replay.u01(r[2], r[3])


def sincospi(x):
    """sin(pi x), cos(pi x) for x in [0, 2] as a correctly reduced sincospi gives them: x = q / 2 + r with |r| <= 1 / 4
    exactly, so that the only roundings are pi r and the two functions on [-pi / 4, pi / 4]."""
    x = np.asarray(x, dtype=np.float64)
    q = np.rint(2.0 * x)
    r = x - 0.5 * q
    s, c = np.sin(np.pi * r), np.cos(np.pi * r)
    q = q.astype(np.int64) & 3
    return np.choose(q, [s, c, -s, -c]), np.choose(q, [c, -s, -c, s])


def normal2(blk):
    """Box-Muller as the kernels write it: blk = (ua, ub) -> (g1, g2) with u1 = 1 - ua in (0, 1]."""
    ua, ub = blk
    rad = np.sqrt(-2.0 * np.log(1.0 - ua))
    s, c = sincospi(2.0 * ub)
    return rad * c, rad * s


def normal2_mp(ua, ub):
    """normal2 of ONE block in mpmath (the uniforms are exact binary fractions)."""
    with mpmath.workdps(DIGITS):
        rad = mpmath.sqrt(-2 * mpmath.log(1 - mpmath.mpf(float(ua))))
        return rad * mpmath.cospi(2 * mpmath.mpf(float(ub))), rad * mpmath.sinpi(2 * mpmath.mpf(float(ub)))


def gaussian_noise(epoch, series, seed):
    """g1 of block (epoch, 10, series, 0): what the observe kernel scales by sigma."""
    return normal2(block(epoch, NOISE, series, 0, seed))[0]


# ---- Poisson counts -------------------------------------------------------------------------------------------------
def _distance(a, b, *also):
    """|a - b| over the largest magnitude among the two sides (and of the summands they were made of, `also`); two sides
    that are not both finite and differ are as far apart as can be."""
    big = np.maximum(np.abs(a), np.abs(b))
    for v in also:
        big = np.maximum(big, np.abs(v))
    with np.errstate(invalid="ignore", divide="ignore"):
        d = np.abs(a - b) / big
    d = np.where(big == 0.0, 0.0, d)
    return np.where(np.isfinite(a) & np.isfinite(b), d, 1.0)


def _to_integer(x):
    """distance of a floor's argument from the integers on either side of it, over the argument's magnitude"""
    with np.errstate(invalid="ignore"):
        f = x - np.floor(x)
        d = np.minimum(f, 1.0 - f) / np.maximum(np.abs(x), 1.0)
    return np.where(np.isfinite(x), d, 1.0)


def poisson_detail(lam, epoch, series, seed):
    """tk95_poisson for every element of the broadcast (lam, epoch, series) -> dict(counts, margin, capped, trips).
    ``margin``: the smallest relative distance by which a decision on the way was taken -- lam against 10, prod <= limit,
    every floor's argument from the next integer, us against 0.07 and 0.013, V against vr and us, the two sides of the log
    inequality (scaled by the largest of their summands as well: that is where their rounding comes from) -- each one
    only where the kernel's short-circuit order evaluates it.  ``capped``: the loop ran out of trips."""
    lam, epoch, series = np.broadcast_arrays(np.asarray(lam, dtype=np.float64), np.asarray(epoch), np.asarray(series))
    shape = lam.shape
    lam, epoch, series = lam.ravel(), epoch.ravel().astype(np.uint64), series.ravel().astype(np.uint64)
    total = lam.size
    counts = np.full(total, np.nan)
    margin = np.full(total, np.inf)
    capped = np.zeros(total, dtype=bool)
    trips = np.zeros(total, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        valid = lam >= 0.0
    margin[valid] = _distance(lam[valid], 10.0)
    margin[~valid] = 1.0

    # Knuth's multiplication below 10: two uniforms per block
    at = np.flatnonzero(valid & (lam < 10.0))
    limit = np.exp(-lam[at])
    prod = np.ones(len(at))
    kcount = np.zeros(len(at))
    live = np.ones(len(at), dtype=bool)
    for ctr in range(1, KNUTH_TRIPS + 1):
        if not live.any():
            break
        i = np.flatnonzero(live)
        ua, ub = block(epoch[at[i]], NOISE, series[at[i]], ctr, seed)
        trips[at[i]] = ctr
        for half in (0, 1):
            p = prod[i] * (ua if half == 0 else ub)
            prod[i] = p
            margin[at[i]] = np.minimum(margin[at[i]], _distance(p, limit[i]))
            stop = p <= limit[i]
            live[i[stop]] = False
            i, ub = i[~stop], ub[~stop]
            kcount[i] += 1.0
    counts[at] = kcount
    capped[at[live]] = True

    # Hoermann's PTRS from 10 up
    at = np.flatnonzero(valid & ~(lam < 10.0))
    L = lam[at]
    slam, loglam = np.sqrt(L), np.log(L)
    b = 0.931 + 2.53 * slam
    a = -0.059 + 0.02483 * b
    invalpha = 1.1239 + 1.1328 / (b - 3.4)
    vr = 0.9277 - 3.6224 / (b - 2.0)
    out = np.floor(L + 0.5)
    live = np.ones(len(at), dtype=bool)
    for ctr in range(1, PTRS_TRIPS + 1):
        if not live.any():
            break
        i = np.flatnonzero(live)
        ua, V = block(epoch[at[i]], NOISE, series[at[i]], ctr, seed)
        trips[at[i]] = ctr
        U = ua - 0.5
        us = 0.5 - np.abs(U)
        with np.errstate(divide="ignore", invalid="ignore"):
            arg = (2.0 * a[i] / us + b[i]) * U + L[i] + 0.43
            kf = np.floor(arg)
            m = np.minimum(_to_integer(arg), _distance(us, 0.07))
            wide = us >= 0.07
            m = np.where(wide, np.minimum(m, _distance(V, vr[i])), m)
            quick = wide & (V <= vr[i])
            rest = ~quick
            narrow = us < 0.013
            m = np.where(rest & (kf >= 0.0), np.minimum(m, _distance(us, 0.013)), m)
            m = np.where(rest & (kf >= 0.0) & narrow, np.minimum(m, _distance(V, us)), m)
            skip = rest & ((kf < 0.0) | (narrow & (V > us)))
            test = rest & ~skip
            t1, t2, t3 = np.log(V), np.log(invalpha[i]), np.log(a[i] / (us * us) + b[i])
            r2, r3 = kf * loglam[i], gammaln(kf + 1.0)
            lhs, rhs = t1 + t2 - t3, -L[i] + r2 - r3
            m = np.where(test, np.minimum(m, _distance(lhs, rhs, t1, t2, t3, L[i], r2, r3)), m)
            slow = test & (lhs <= rhs)
        margin[at[i]] = np.minimum(margin[at[i]], m)
        take = quick | slow
        out[i[take]] = kf[take]
        live[i[take]] = False
    fell = at[live]
    margin[fell] = np.minimum(margin[fell], _to_integer(lam[fell] + 0.5))
    counts[at] = out
    capped[fell] = True
    return dict(counts=counts.reshape(shape), margin=margin.reshape(shape), capped=capped.reshape(shape), trips=trips.reshape(shape))


def poisson(lam, epoch, series, seed):
    """-> (counts, margin); an epoch is decided when margin > DECIDED."""
    d = poisson_detail(lam, epoch, series, seed)
    return d["counts"], d["margin"]


DECIDED = 1e-9


# ---- E13's own draws ------------------------------------------------------------------------------------------------
def e13_draws(kind, mean, std, n, series, seed, with_exponent=False):
    """mtg_e13_draw_kernel: x[series][n] from one block (pair, 11, series, pair >> 32) per pair of elements, the second
    of the last pair dropped when n is odd.  kind 1: lognormal, 2: uniform; ``std``, ``series``: scalars or [S].
    ``with_exponent``: also |s_ln z| per element (zeros for the uniform kind), what the lognormal's error grows with."""
    sd = np.atleast_1d(np.asarray(std, dtype=np.float64))[:, None]
    sg = np.atleast_1d(np.asarray(series)).astype(np.uint64)[:, None]
    p = np.arange((n + 1) // 2, dtype=np.uint64)[None, :]
    ua, ub = block(p, E13, sg, p >> np.uint64(32), seed)
    var = sd * sd
    if kind == 1:
        rad = np.sqrt(-2.0 * np.log(1.0 - ua))
        sn, cs = sincospi(2.0 * ub)
        sl = np.sqrt(np.log(var / (mean * mean) + 1.0))
        scale = mean * mean / np.sqrt(var + mean * mean)
        e0, e1 = sl * rad * cs, sl * rad * sn
        v0, v1 = scale * np.exp(e0), scale * np.exp(e1)
    else:
        hw = np.sqrt(3.0) * sd
        v0 = mean - hw + 2.0 * hw * ua
        v1 = mean - hw + 2.0 * hw * ub
        e0 = e1 = np.zeros_like(v0)
    x = np.stack([v0, v1], axis=2).reshape(len(sd), -1)[:, :n]
    expo = np.abs(np.stack([e0, e1], axis=2).reshape(len(sd), -1)[:, :n])
    if np.ndim(std) == 0 and np.ndim(series) == 0:
        x, expo = x[0], expo[0]
    return (x, expo) if with_exponent else x


def e13_draws_mp(kind, mean, std, n, series, seed):
    """e13_draws of ONE series in mpmath: a list of n mpf (mean and std taken as the doubles they are)."""
    p = np.arange((n + 1) // 2, dtype=np.uint64)
    ua, ub = block(p, E13, int(series), p >> np.uint64(32), seed)
    out = []
    with mpmath.workdps(DIGITS):
        mean, sd = mpmath.mpf(float(mean)), mpmath.mpf(float(std))
        var = sd * sd
        sl = mpmath.sqrt(mpmath.log(var / (mean * mean) + 1))
        scale = mean * mean / mpmath.sqrt(var + mean * mean)
        hw = mpmath.sqrt(3) * sd
        for a, b in zip(ua, ub):
            if kind == 1:
                g1, g2 = normal2_mp(a, b)
                out += [scale * mpmath.exp(sl * g1), scale * mpmath.exp(sl * g2)]
            else:
                out += [mean - hw + 2 * hw * mpmath.mpf(float(a)), mean - hw + 2 * hw * mpmath.mpf(float(b))]
    return out[:n]


def e13_host_loop(segment, draws, max_iter=400, tie=1e-9):
    """The reference's adjustment loop (Simulator._adjust_pdf) started from ``draws`` -> (series, closest): ``closest`` is
    the smallest gap between two neighbouring adjusted values met at any iteration, relative to the larger of the two --
    below ``tie`` the ranks, and with them the order the loop ends on, are not the arithmetic's to decide."""
    n = len(segment)
    amplitudes = np.abs(np.fft.rfft(segment))
    current = np.array(draws, dtype=np.float64)
    values = np.sort(current)[::-1]
    closest = np.inf
    for _ in range(max_iter + 1):
        adjusted = np.fft.irfft(amplitudes * np.exp(1j * np.angle(np.fft.rfft(current))), n=n)
        ranked = np.sort(adjusted)
        gap = np.diff(ranked) / np.maximum(np.abs(ranked[1:]), np.abs(ranked[:-1]))
        closest = min(closest, float(np.min(gap)))
        new = np.empty(n)
        new[np.argsort(-adjusted)] = values
        if np.allclose(new, current, rtol=1e-4):
            return new, closest
        current = new
    return current, closest


# ---- the spectrum ---------------------------------------------------------------------------------------------------
def coefficients(kinds, row, exp, sqrt, one=1.0, matern_eps=MATERN_EPS):
    """theta -> celerite coefficients as mtg_prepare_from writes them, in its order and with its expressions, in the
    arithmetic of ``exp`` / ``sqrt`` (numpy's: float64 as the device; mpmath's: the truth).  ``row``: the terms'
    parameters in the order of ``kinds`` (anything behind them, the mean, is ignored).
    -> (reals [(a, c)], complexes [(a, b, c, d)]); a jitter term has no spectrum."""
    reals, comps = [], []
    o = 0
    for kind in kinds:
        th = [one * row[o + i] for i in range(NPARAMS[kind])]
        o += NPARAMS[kind]
        if kind == K_REAL:
            reals.append((exp(th[0]), exp(th[1])))
        elif kind == K_COMPLEX3:
            comps.append((exp(th[0]), 0 * one, exp(th[1]), exp(th[2])))
        elif kind == K_COMPLEX4:
            comps.append((exp(th[0]), exp(th[1]), exp(th[2]), exp(th[3])))
        elif kind == K_SHO:
            S0, Q, w0 = exp(th[0]), exp(th[1]), exp(th[2])
            if Q < 0.5:
                f = sqrt(1 - 4 * Q * Q)
                reals.append((0.5 * S0 * w0 * Q * (1 + 1 / f), 0.5 * w0 / Q * (1 - f)))
                reals.append((0.5 * S0 * w0 * Q * (1 - 1 / f), 0.5 * w0 / Q * (1 + f)))
            else:
                f = sqrt(4 * Q * Q - 1)
                av = S0 * w0 * Q
                comps.append((av, av / f, 0.5 * w0 / Q, 0.5 * w0 / Q * f))
        elif kind == K_MATERN32:
            eps = one * matern_eps
            w0 = sqrt(3 * one) * exp(-th[1])
            S0 = exp(2 * th[0]) / w0
            comps.append((w0 * S0, w0 * w0 * S0 / eps, w0, eps))
        elif kind == K_JITTER:
            pass
        elif kind == K_DRW:
            reals.append((exp(th[0]), 0.5 * exp(th[1]) / 0.5))
        elif kind == K_LORENTZIAN:
            w0 = exp(th[2])
            comps.append((exp(th[0]), 0 * one, 0.5 * w0 / exp(th[1]), w0))
        else:
            raise ValueError("term kind %r has no replay" % (kind,))
    return reals, comps


def signature(kinds, row):
    """number of over-damped SHO terms of the row: the kernel's nr = nr0 + 2 sig, nc = nc0 - sig"""
    o, sig = 0, 0
    for kind in kinds:
        if kind == K_SHO and np.exp(np.float64(row[o + 1])) < 0.5:
            sig += 1
        o += NPARAMS[kind]
    return sig


def psd_f64(kinds, row, omega):
    """mtg_psd operation for operation in float64 (numpy scalars), at the angular frequencies ``omega``."""
    reals, comps = coefficients(kinds, np.asarray(row, dtype=np.float64), np.exp, np.sqrt, np.float64(1.0))
    w = np.asarray(omega, dtype=np.float64)
    w2 = w * w
    p = np.zeros_like(w)
    for a, c in reals:
        p = p + a * c / (c * c + w2)
    for a, b, c, d in comps:
        w02 = c * c + d * d
        p = p + ((a * c + b * d) * w02 + (a * c - b * d) * w2) / (w2 * w2 + 2.0 * (c * c - d * d) * w2 + w02 * w02)
    return 0.79788456080286535588 * p


def psd(kinds, row, omega):
    """The spectrum of the model at ``omega`` in mpmath (40 digits): celerite's sum over the coefficients of
    ``coefficients``, sqrt(2 / pi) in front.  -> list of mpf."""
    with mpmath.workdps(DIGITS):
        reals, comps = coefficients(kinds, [float(v) for v in row], mpmath.exp, mpmath.sqrt, mpmath.mpf(1))
        out = []
        for w in np.atleast_1d(omega):
            w2 = mpmath.mpf(float(w)) ** 2
            p = mpmath.mpf(0)
            for a, c in reals:
                p += a * c / (c * c + w2)
            for a, b, c, d in comps:
                w02 = c * c + d * d
                p += ((a * c + b * d) * w02 + (a * c - b * d) * w2) / (w2 * w2 + 2 * (c * c - d * d) * w2 + w02 * w02)
            out.append(mpmath.sqrt(2 / mpmath.pi) * p)
        return out


def grid_omega(k, nfft, dt):
    """the spectrum kernel's angular frequency of line k"""
    return 6.28318530717958647692 * np.asarray(k, dtype=np.float64) / (float(nfft) * dt)


def rel_ulps(got, truth):
    """|got - truth| / |truth| in units of 2^-52, ``truth`` a list of mpf"""
    with mpmath.workdps(DIGITS):
        return np.array([float(abs(mpmath.mpf(float(g)) - t) / abs(t)) if t != 0 else (0.0 if g == 0 else np.inf)
                         for g, t in zip(np.ravel(got), truth)]) / EPS


# ---- the cases of test_simulator_replay_gpu.py, shared with the CPU test ---------------------------------------------
# (a) name -> (mean rate, variance of the DRW, exposure, seed): ~2 counts per epoch with some clean rates below zero, ~25
# (PTRS only), 9-11 (both sides of the switch at 10).  The exposure is a power of two: counts = rates * exposure exactly.
POISSON_CASES = {"knuth-2": (4.0, 4.0, 0.5, 1001), "ptrs-25": (50.0, 4.0, 0.5, 1002), "switch-10": (20.0, 1.0, 0.5, 1003)}
POISSON_S, POISSON_EPOCHS = 40, 120
KRAFT_SEED = 31

# (d) the rows of theta, six per model; in the SHO batches ln Q lies on both sides of ln(1 / 2) and once within 1e-3 of it
_LNQ = np.log(0.5) + np.array([-1.2, 7e-4, 1.5, -6e-4, 0.4, -0.3])
PSD_MODELS = {
    "drw": ([K_DRW], np.column_stack([np.log([100.0, 3.0, 40.0, 0.5, 900.0, 7.0]), np.log([0.3, 1.0, 0.05, 2.5, 0.7, 0.11])])),
    "sho": ([K_SHO], np.column_stack([np.log([50.0, 2.0, 9.0, 30.0, 0.8, 120.0]), _LNQ, np.log([0.9, 0.3, 1.7, 0.6, 2.4, 0.2])])),
    "matern32": ([K_MATERN32], np.column_stack([np.log([5.0, 1.5, 12.0, 0.4, 30.0, 2.2]), np.log([8.0, 1.0, 0.5, 3.0, 20.0, 1.7])])),
    "complex4": ([K_COMPLEX4], np.column_stack([np.log([20.0, 5.0, 60.0, 1.2, 9.0, 33.0]), np.log([1.0, 0.4, 2.0, 0.05, 0.1, 1.5]),
                                                np.log([0.05, 0.3, 0.1, 0.6, 0.02, 0.2]), np.log([0.7, 1.1, 0.4, 2.0, 0.9, 1.6])])),
    "drw+sho+jitter": ([K_DRW, K_SHO, K_JITTER], np.column_stack([
        np.log([100.0, 3.0, 40.0, 0.5, 900.0, 7.0]), np.log([0.3, 1.0, 0.05, 2.5, 0.7, 0.11]),
        np.log([50.0, 2.0, 9.0, 30.0, 0.8, 120.0]), _LNQ[::-1], np.log([0.9, 0.3, 1.7, 0.6, 2.4, 0.2]),
        np.log([0.7, 0.1, 1.3, 0.5, 2.0, 0.9])])),
}
PSD_NFFT, PSD_DT = 64, 0.5


def poisson_simulator(name):
    """-> (Simulator, thetas [S][2], seed) of a case of POISSON_CASES: 120 regular epochs, a DRW, Poisson noise"""
    from mind_the_gaps_amd.models import DampedRandomWalk
    from mind_the_gaps_amd.simulator import Simulator
    mean, variance, exposure, seed = POISSON_CASES[name]
    times = np.arange(0.5, POISSON_EPOCHS, 1.0)
    kernel = DampedRandomWalk(np.log(variance), np.log(0.3), bounds=[(-10, 50), (-10, 10)])
    sim = Simulator(kernel, times, exposure, mean, "Gaussian", extension_factor=2, random_state=1)
    return sim, np.tile(kernel.get_parameter_vector(), (POISSON_S, 1)), seed


def kraft_simulator():
    """the simulator of test_simulator_gpu.py's Kraft test -> (Simulator, thetas [S][2], seed)"""
    from mind_the_gaps_amd import synthetic as synth
    from mind_the_gaps_amd.models import DampedRandomWalk
    from mind_the_gaps_amd.simulator import Simulator
    times = synth.make_times(150, np.random.default_rng(4))
    kernel = DampedRandomWalk(np.log(900.0), np.log(2 * np.pi / 12), bounds=[(-10, 50), (-10, 10)])
    sim = Simulator(kernel, times, 0.04, 400.0, "Gaussian", bkg_rate=30.0, bkg_rate_err=2.0, extension_factor=2, random_state=1)
    return sim, np.tile(kernel.get_parameter_vector(), (POISSON_S, 1)), KRAFT_SEED


def clean_on_host(sim, thetas, seed, base=0):
    """The noise-free rates of a DRW simulator with numpy's irfft and the replayed draws: the device's `clean` to the
    rounding of the transform (~1e-12), good enough to ask how often the Poisson replay meets a close decision."""
    nfft, dt = sim.fftndatapoints, sim.sim_dt
    k = np.arange(1, nfft // 2 + 1)
    out = np.empty((len(thetas), len(sim.win_lo)))
    for s, th in enumerate(thetas):
        g1, g2 = normal2(block(k, 8, s + base, k >> 32, seed))
        X = np.zeros(nfft // 2 + 1, dtype=complex)
        X[1:] = (g1 + 1j * g2) * np.sqrt(0.5 * psd_f64([K_DRW], th, grid_omega(k, nfft, dt)))
        if nfft % 2 == 0:
            X[-1] = X[-1].real
        rate = np.fft.irfft(X, n=nfft) * np.sqrt(nfft * dt * np.sqrt(2 * np.pi)) / dt + sim.mean
        span = (nfft - 1) - sim.seg_len
        j0 = int(np.ceil(float(block(0, 9, s + base, 0, seed)[0]) * span)) if span > 0 else 0
        j0 = max(0, min(j0, nfft - sim.seg_len))
        seg = rate[j0:j0 + sim.seg_len]
        out[s] = [seg[a:b].mean() for a, b in zip(sim.win_lo, sim.win_hi)]
    return out


# ---- the replay's own error against its mpmath twins (test_simulator_replay_cpu.py measures and holds them) ----------
R_NORMAL = 2.0            # normal2, units of 2^-52 relative
R_UNIFORM = 2.0           # e13_draws, uniform kind
R_DRAW = (2.0, 1.0)       # e13_draws, lognormal kind: R_draw(x) = R_DRAW[0] + R_DRAW[1] x at exponent x = |s_ln z|, std / mean in [0.2, 1]


def r_draw(exponent):
    return R_DRAW[0] + R_DRAW[1] * np.asarray(exponent)


_R_PSD = {}


def r_psd(name):
    """R_psd of a model of PSD_MODELS: the worst relative error of psd_f64 against psd over its six rows and the lines
    1 .. nfft / 2, in units of 2^-52"""
    if name not in _R_PSD:
        kinds, rows = PSD_MODELS[name]
        w = grid_omega(np.arange(1, PSD_NFFT // 2 + 1), PSD_NFFT, PSD_DT)
        _R_PSD[name] = max(rel_ulps(psd_f64(kinds, row, w), psd(kinds, row, w)).max() for row in rows)
    return _R_PSD[name]
