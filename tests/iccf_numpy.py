"""mtg_iccf (include/mtg.h) in plain numpy float64: searchsorted for the bracket, the formulas as written -- the
definition as one would write it on the host, the yardstick whose own error rho the fixture records -- and the cases, lag
sets and bounds that scripts/make_iccf_golden.py, tests/test_iccf_cpu.py and tests/test_iccf_gpu.py share."""
import numpy as np

from cross_numpy import CASES, COMPANION_M, companion  # noqa: F401  (the resident series and their companions)

LAG_SETS = ("sym65", "one", "fine257", "beyond", "ties", "shuffled")
MODES = ("both", "companion", "resident")
U = 2.0 ** -53
# the set of the GPU test's two slabs: case n5 at K lags, L light curves (tests/test_iccf_cpu.py holds it to the planner)
TWO_SLABS = dict(K=65536, L=173)


def interpolate(u, z, x):
    """I(series, x) of include/mtg.h for u[0] <= x <= u[-1]: the left node is the LAST index with u <= x"""
    p = np.searchsorted(u, x, side="right") - 1
    end = p == len(u) - 1
    q = np.where(end, p, p + 1)
    w = (x - u[p]) / np.where(end, 1.0, u[q] - u[p])
    return np.where(end, z[p], w * (z[q] - z[p]) + z[p]), p


def half(tw, a, shift, u, z):
    """One half at one lag: the walked series (times tw, residuals a) shifted by ``shift`` against the interpolated one
    (u, z) -> (r, n, S): the correlation, the samples used, and the scale the rounding of the one-pass formula grows with"""
    x = tw + shift
    ok = (x >= u[0]) & (x <= u[-1])
    n = int(ok.sum())
    if n < 2:
        return np.nan, n, np.nan
    w = a[ok]
    v = interpolate(u, z, x[ok])[0]
    sw, sv = w.sum(), v.sum()
    c = (w * v).sum() - sw * sv / n
    va = (w * w).sum() - sw * sw / n
    vb = (v * v).sum() - sv * sv / n
    if not (va > 0 and vb > 0):
        return np.nan, n, np.nan
    r = c / np.sqrt(va * vb)
    if not np.isfinite(r):
        return np.nan, n, np.nan
    cabs = np.abs(w * v).sum() + abs(sw) * abs(sv) / n
    scale = cabs / np.sqrt(va * vb) + 0.5 * abs(r) * (((w * w).sum() + sw * sw / n) / va + ((v * v).sum() + sv * sv / n) / vb)
    return r, n, scale


def iccf(t, y, t2, y2, lags):
    """dict r_a, r_b [K] (NaN by the header's rule), n_a, n_b [K] int64, s_a, s_b [K] of one light curve and one companion row"""
    t, y, t2, y2, lags = (np.asarray(a, dtype=np.float64) for a in (t, y, t2, y2, lags))
    r, s = y - np.mean(y), y2 - np.mean(y2)
    a = [half(t, r, tau, t2, s) for tau in lags]
    b = [half(t2, s, -tau, t, r) for tau in lags]
    col = lambda rows, k, dtype: np.array([row[k] for row in rows], dtype=dtype)
    return dict(r_a=col(a, 0, np.float64), n_a=col(a, 1, np.int64), s_a=col(a, 2, np.float64),
                r_b=col(b, 0, np.float64), n_b=col(b, 1, np.int64), s_b=col(b, 2, np.float64))


def combine(mode, r_a, r_b):
    """the ccf of a mode from its halves"""
    return {"both": 0.5 * (r_a + r_b), "companion": r_a, "resident": r_b}[mode]


def shuffle_map(K=65):
    """shuffled[k] = sym65[shuffle_map()[k]]: a seeded permutation of the K lags with two of them repeated at the end"""
    perm = np.random.default_rng(65).permutation(K)
    return np.concatenate([perm, perm[[3, 40]]])


def lag_sets(t, t2):
    """name -> lags of the six sets the fixture holds for the samplings t and t2"""
    t, t2 = np.asarray(t, dtype=np.float64), np.asarray(t2, dtype=np.float64)
    half_span = 0.5 * min(t[-1] - t[0], t2[-1] - t2[0])
    sym = np.linspace(-half_span, half_span, 65)
    lo, hi = t2[0] - t[-1], t2[-1] - t[0]            # the lags at which the overlap of half A begins and ends
    w = hi - lo
    beyond = np.concatenate([np.linspace(lo - 0.1 * w, hi + 0.1 * w, 23),
                             [lo, hi, t2[0] - 0.5 * (t[-1] + t[-2]), t2[-1] - 0.5 * (t[0] + t[1]),    # half A keeps one sample
                              t2[0] - t[-2], t2[-2] - t[0]]])
    # lags equal to a pair's own t2_j - t_i that put the shifted resident sample exactly on the companion's node
    js = sorted({0, len(t2) // 3, len(t2) // 2, len(t2) - 1})
    picks = np.unique(np.linspace(0, len(t) - 1, 5).astype(int))
    ties = [0.0] + [t2[j] - t[i] for j in js for i in picks if t[i] + (t2[j] - t[i]) == t2[j]]
    return {"sym65": sym, "one": np.array([0.25 * half_span]), "fine257": np.linspace(-0.25 * half_span, 0.25 * half_span, 257),
            "beyond": beyond, "ties": np.array(ties), "shuffled": sym[shuffle_map()]}


def tie_pairs(t, t2, lags):
    """rows (k, i, j) with fl(t_i + lags[k]) == t2_j exactly"""
    out = [(k, i, j) for k, tau in enumerate(lags) for i, x in enumerate(t + tau) for j in np.flatnonzero(t2 == x)]
    return np.array(out, dtype=np.int64).reshape(-1, 3)


def bound(rho, n, scale):
    """|error| allowed for one half of n samples: the project's usual form, on the scale of the one-pass formula"""
    return np.maximum(10.0 * rho, 64.0 * np.sqrt(n) * U * scale)
