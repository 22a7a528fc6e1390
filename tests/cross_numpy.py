"""mtg_cross_sums (include/mtg.h) in plain numpy float64: outer subtraction, searchsorted, bincount with weights -- the
definition as one would write it on the host, the yardstick whose own error rho the fixture records -- and the cases, edge
sets and bounds that scripts/make_cross_golden.py, tests/test_cross_cpu.py and tests/test_cross_gpu.py share."""
import numpy as np

SUMS = ("count", "lag", "cf", "cf2", "sa", "sb", "saa", "sbb")
VALUES = SUMS[1:]
# the sum of the terms' magnitudes, the scale of a sum's bound: the sum itself where every term is >= 0
SCALE = dict(lag="lagabs", cf="cfabs", cf2="cf2", sa="saabs", sb="sbabs", saa="saa", sbb="sbb")
CASES = ("n5", "n52", "n216", "n789")           # the resident series: those of lomb_scargle_golden.npz
COMPANION_M = dict(n5=7, n52=61, n216=300, n789=523)
EDGE_SETS = ("sym8", "one", "negative6", "short5", "wide128", "ties")
U = 2.0 ** -53


def companion(name, t, y):
    """(t2, y2) of the case: M samples over a span shifted against the resident one (it starts 0.3 spans in and ends 0.2
    spans past the end), a few of its times copied from the resident times so that tau == 0 occurs; a seeded generator."""
    M = COMPANION_M[name]
    rng = np.random.default_rng(1000 + len(t))
    span = t[-1] - t[0]
    t2 = np.sort(rng.uniform(t[0] + 0.3 * span, t[-1] + 0.2 * span, M))
    inside = np.flatnonzero(t >= t2[0])
    for k in inside[np.linspace(0, len(inside) - 1, 1 if len(t) < 10 else 3).astype(int)]:
        t2[np.argmin(np.abs(t2 - t[k]))] = t[k]
    t2 = np.sort(t2)
    y2 = 3.0 * np.mean(np.abs(y)) + np.std(y) * (np.sin(7.0 * (t2 - t[0]) / span) + 0.5 * rng.standard_normal(M))
    return t2, y2


def pairs(t, t2):
    """(i, j, tau) of every pair, row by row with j ascending; tau = fl(t2_j - t_i)"""
    i, j = np.divmod(np.arange(len(t) * len(t2)), len(t2))
    return i, j, t2[j] - t[i]


def bin_index(tau, edges):
    """the bin of every lag: edges[b] <= tau < edges[b + 1]; -1 for no bin"""
    b = np.searchsorted(edges, tau, side="right") - 1
    return np.where((b >= 0) & (b < len(edges) - 1), b, -1)


def cross_sums(t, y, t2, y2, edges):
    """dict of the eight sums [nbins] of one light curve and one companion row, and the scales lagabs, cfabs, saabs, sbabs"""
    t, y, t2, y2, edges = (np.asarray(a, dtype=np.float64) for a in (t, y, t2, y2, edges))
    nb = len(edges) - 1
    i, j, tau = pairs(t, t2)
    b = bin_index(tau, edges)
    keep = b >= 0
    i, j, tau, b = i[keep], j[keep], tau[keep], b[keep]
    r = y - np.mean(y)
    s = y2 - np.mean(y2)
    p = r[i] * s[j]
    tot = lambda w: np.bincount(b, weights=w, minlength=nb)
    # a row's partial of sa is r_i times its pair count in the bin, of saa the rounded r_i^2 times it
    c = np.bincount(i * nb + b, minlength=len(t) * nb).reshape(len(t), nb).astype(np.float64)
    return dict(count=np.bincount(b, minlength=nb).astype(np.int64), lag=tot(tau), cf=tot(p), cf2=tot(p * p),
                sa=(r[:, None] * c).sum(axis=0), sb=tot(s[j]), saa=((r * r)[:, None] * c).sum(axis=0), sbb=tot(s[j] * s[j]),
                lagabs=tot(np.abs(tau)), cfabs=tot(np.abs(p)), saabs=(np.abs(r)[:, None] * c).sum(axis=0), sbabs=tot(np.abs(s[j])))


def edge_sets(t, t2):
    """name -> edges of the six sets the fixture holds for the samplings t and t2"""
    t, t2 = np.asarray(t, dtype=np.float64), np.asarray(t2, dtype=np.float64)
    span = t[-1] - t[0]
    taus = np.unique(pairs(t, t2)[2])
    lo, hi = taus[0], taus[-1]
    half = 0.5 * min(span, t2[-1] - t2[0])
    pick = np.unique(np.linspace(0, len(taus) - 1, 7).astype(int))
    return {
        "sym8": np.linspace(-half, half, 9),
        "one": np.array([-0.25 * span, 0.5 * span]),
        "negative6": np.linspace(-0.6 * span, -0.01 * span, 7),
        "short5": np.linspace(0.05 * span, 0.15 * span, 6),        # late start and early exit; pairs on both sides of it
        "wide128": np.linspace(lo - 0.25 * (hi - lo), hi + 0.25 * (hi - lo), 129),   # empty bins at both ends
        "ties": np.unique(np.concatenate([taus[pick], [0.0]])),    # every edge is the lag of an actual pair, 0 included
    }


def skipped_chunks(t, t2, edges, lanes=256, chunk=256):
    """(late, early, total): the (row block, chunk) pairs a workgroup skips before its first chunk and from its early exit
    on, and all of them -- the rule of csrc/mtg_cross.hip restated"""
    late = early = total = 0
    for row0 in range(0, len(t), lanes):
        first, last = t[row0], t[min(row0 + lanes, len(t)) - 1]
        starts = list(range(0, len(t2), chunk))
        total += len(starts)
        k = 0
        while k < len(starts) and not t2[min(starts[k] + chunk, len(t2)) - 1] - first >= edges[0]:
            k += 1
        late += k
        while k < len(starts) and not t2[starts[k]] - last >= edges[-1]:
            k += 1
        early += len(starts) - k
    return late, early, total


def bound(rho, count, scale):
    """|error| allowed for a sum of `count` terms whose magnitudes add up to `scale`: the project's usual bound"""
    return np.maximum(10.0 * rho, 64.0 * np.sqrt(count) * U) * scale
