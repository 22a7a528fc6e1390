"""mtg_lag_sums (include/mtg.h) in plain numpy float64: outer subtraction, searchsorted, bincount with weights -- the
definition as one would write it on the host, the yardstick whose own error rho the fixture records -- and the edge sets
and bounds that scripts/make_lag_golden.py, tests/test_lag_cpu.py and tests/test_lag_gpu.py share."""
import numpy as np

SUMS = ("count", "lag", "sf", "cf", "cf2", "noise")
CASES = ("n5", "n52", "n216", "n789")
EDGE_SETS = ("linear8", "log32", "one", "short5", "wide128", "ties")
U = 2.0 ** -53


def pairs(t):
    """(i, j, tau) of every pair i < j, row by row with j ascending; tau = fl(t_j - t_i)"""
    i, j = np.triu_indices(len(t), k=1)
    return i, j, t[j] - t[i]


def bin_index(tau, edges):
    """the bin of every lag: edges[b] <= tau < edges[b + 1]; -1 for no bin"""
    b = np.searchsorted(edges, tau, side="right") - 1
    return np.where((b >= 0) & (b < len(edges) - 1), b, -1)


def lag_sums(t, y, dy, edges):
    """dict of the six sums [nbins] of one light curve, and "cfabs" = sum |r_i r_j|, the scale of cf's bound"""
    t, y, dy, edges = (np.asarray(a, dtype=np.float64) for a in (t, y, dy, edges))
    nb = len(edges) - 1
    i, j, tau = pairs(t)
    b = bin_index(tau, edges)
    keep = b >= 0
    i, j, tau, b = i[keep], j[keep], tau[keep], b[keep]
    r = y - np.mean(y)
    v = dy * dy
    p = r[i] * r[j]
    tot = lambda w: np.bincount(b, weights=w, minlength=nb)
    return dict(count=np.bincount(b, minlength=nb).astype(np.int64), lag=tot(tau), sf=tot((y[j] - y[i]) ** 2), cf=tot(p), cf2=tot(p * p),
                noise=tot(v[i] + v[j]), cfabs=tot(np.abs(p)))


def edge_sets(t):
    """name -> edges of the six sets the fixture holds for the sampling t"""
    t = np.asarray(t, dtype=np.float64)
    span = t[-1] - t[0]
    steps = np.diff(t)
    min_lag = float(steps[steps > 0].min())
    taus = np.unique(pairs(t)[2])
    lo = min(1.5 * min_lag, 0.05 * span)
    pick = np.unique(np.linspace(0, len(taus) - 1, 7).astype(int))
    return {
        "linear8": np.linspace(0.0, span, 9),                       # the largest lag sits on the last edge: in no bin
        "log32": np.geomspace(min_lag, 0.5 * span, 33),
        "one": np.array([0.0, 0.75 * span]),
        "short5": np.linspace(lo, 0.1 * span, 6),                   # early exit, and pairs below the first edge
        # 16 bins narrower than any lag present, then 112 of which the last third lies beyond the span
        "wide128": np.concatenate([np.linspace(0.0, 0.5 * min_lag, 17)[:-1], np.linspace(0.5 * min_lag, 1.5 * span, 113)]),
        "ties": taus[pick],                                          # every edge is the lag of an actual pair
    }


def bound(rho, count, scale):
    """|error| allowed for a sum of `count` terms whose magnitudes add up to `scale`: the project's usual bound"""
    return np.maximum(10.0 * rho, 64.0 * np.sqrt(count) * U) * scale
