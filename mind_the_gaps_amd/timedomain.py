"""The time-lag view of a light curve on the device: the structure function and the discrete correlation function of
Edelson & Krolik (1988) in bins of the lag ``tau = t_j - t_i`` over the pairs ``i < j`` of the samples -- what one plots to
read off a break timescale or to see a QPO as a dip and a bump, and compares with the model's ``2 (k(0) - k(tau))``.
Defined on the pairs: gaps cost nothing and nothing is interpolated.

The sums over the pairs come from ``Engine.lag_sums`` (``mtg_lag_sums``, include/mtg.h) on the GPU, for one light curve
or a whole set on shared sampling in one call; this module bins, normalises and models.  There is no CPU fallback, as
elsewhere in the package.

The lag between TWO series on different samplings -- one energy band against another -- is ``CrossCorrelation`` on
``Engine.cross_sums`` (``mtg_cross_sums``): every pair of a sample of each, signed lags, positive when the second lags.

    >>> edges = lag_bins(t, 20, spacing="log")
    >>> tau, sf2, count = StructureFunction(t, y, dy).sf(edges)
    >>> model = model_structure_function(kernel, tau)
"""
import numpy as np

from .engine import ICCF_MAX_LAGS, LAG_MAX_BINS

__all__ = ["lag_bins", "StructureFunction", "DiscreteCorrelation", "model_structure_function", "sf_from_sums", "dcf_from_sums",
           "cross_lag_bins", "ccf_from_sums", "CrossCorrelation", "lag_peak_and_centroid"]


def lag_bins(t, nbins, spacing="linear", min_lag=None, max_lag=None):
    """``nbins + 1`` ascending edges for ``Engine.lag_sums``: ``"linear"`` or ``"log"`` spacing from ``min_lag`` (None: the
    smallest positive spacing of ``t``) to ``max_lag`` (None: half the span).  Bin b holds ``edges[b] <= tau < edges[b + 1]``."""
    t = np.asarray(t, dtype=np.float64)
    if t.ndim != 1 or len(t) < 2:
        raise ValueError("t must be [N] with N >= 2")
    if nbins not in range(1, LAG_MAX_BINS + 1):
        raise ValueError("nbins must lie in 1 .. %d" % LAG_MAX_BINS)
    if spacing not in ("linear", "log"):
        raise ValueError("spacing must be 'linear' or 'log'")
    if min_lag is None:
        steps = np.diff(np.sort(t))
        steps = steps[steps > 0]
        if len(steps) == 0:
            raise ValueError("all times are equal: there is no positive lag")
        min_lag = float(steps.min())
    if max_lag is None:
        max_lag = 0.5 * float(t.max() - t.min())
    if not (np.isfinite(min_lag) and np.isfinite(max_lag)) or min_lag < 0 or not min_lag < max_lag:
        raise ValueError("need finite 0 <= min_lag < max_lag, got %r and %r" % (min_lag, max_lag))
    if spacing == "log":
        if min_lag <= 0:
            raise ValueError("log spacing needs min_lag > 0")
        edges = np.geomspace(min_lag, max_lag, nbins + 1)
    else:
        edges = np.linspace(min_lag, max_lag, nbins + 1)
    if not np.all(np.diff(edges) > 0):
        raise ValueError("%d bins between %r and %r are narrower than the numbers resolve" % (nbins, min_lag, max_lag))
    return edges


def _per_pair(total, count):
    """total / count, NaN where the bin is empty"""
    count = np.asarray(count, dtype=np.float64)
    return np.where(count > 0, np.asarray(total) / np.where(count > 0, count, 1.0), np.nan)


def sf_from_sums(sums, subtract_noise=True):
    """``lag_sums``' ``count, lag, sf`` (and ``noise``) -> (mean lag, SF^2 = sf / count - noise / count, count); an empty bin
    gives NaN."""
    count = sums["count"]
    sf2 = _per_pair(sums["sf"], count)
    if subtract_noise:
        sf2 = sf2 - _per_pair(sums["noise"], count)
    return _per_pair(sums["lag"], count), sf2, count


def dcf_from_sums(sums, s2, e2=0.0):
    """``lag_sums``' ``count, lag, cf, cf2`` -> (mean lag, DCF, its error, count) with the variance ``s2`` = sum r^2 / N
    and the mean measurement variance ``e2`` of each light curve ([L] or scalars):
    ``DCF_b = cf_b / (count_b (s2 - e2))`` and Edelson & Krolik's error
    ``sqrt(cf2_b - cf_b^2 / count_b) / ((count_b - 1) (s2 - e2))``, NaN for fewer than two pairs."""
    count = np.asarray(sums["count"])
    c = count.astype(np.float64)
    norm = np.asarray(s2, dtype=np.float64) - np.asarray(e2, dtype=np.float64)
    norm = norm[..., None] if np.ndim(norm) else norm
    cf, cf2 = np.asarray(sums["cf"]), np.asarray(sums["cf2"])
    dcf = _per_pair(cf, count) / norm
    two = count >= 2
    safe = np.where(two, c, 2.0)
    spread = np.sqrt(np.maximum(cf2 - cf * cf / safe, 0.0))      # (a negative difference is rounding)
    err = np.where(two, spread / ((safe - 1.0) * norm), np.nan)
    return _per_pair(sums["lag"], count), dcf, err, count


class _LagStatistic:
    """What ``StructureFunction`` and ``DiscreteCorrelation`` share: the data and the sums through the process-wide engine."""

    def __init__(self, t, y, dy=None, device=0):
        self.t = np.ascontiguousarray(t, dtype=np.float64)
        self.y = np.ascontiguousarray(y, dtype=np.float64)
        if self.t.ndim != 1 or self.y.ndim not in (1, 2) or self.y.shape[-1] != len(self.t):
            raise ValueError("t must be [N] and y [N] or [L][N]")
        if len(self.t) < 2:
            raise ValueError("a lag needs N >= 2 samples")
        if np.any(np.diff(self.t) < 0):
            raise ValueError("t must ascend")
        self.dy = None if dy is None else np.ascontiguousarray(np.broadcast_to(np.asarray(dy, dtype=np.float64), self.y.shape))
        self.device = device

    def _sums(self, edges, **want):
        from .gp import get_engine
        eng = get_engine(self.device)
        y = np.atleast_2d(self.y)
        eng.set_lightcurves(self.t, y, np.ones_like(y) if self.dy is None else np.atleast_2d(self.dy))
        eng.bound_to = None      # the process-wide engine holds this object's light curves now, nobody's evaluator's
        return eng.lag_sums(edges, **dict(dict(count=True, lag=True, sf=False), **want))

    def _shaped(self, arrays):
        return tuple(a.reshape(self.y.shape[:-1] + a.shape[-1:]) for a in arrays)


class StructureFunction(_LagStatistic):
    """``StructureFunction(t, y, dy=None)``: ``t`` [N] ascending, ``y`` [N] or [L][N] on the sampling ``t``, ``dy`` None
    (no noise term), a scalar, [N] or [L][N]."""

    def sf(self, edges, subtract_noise=True):
        """-> (mean lag, SF^2, count), each [nbins] or [L][nbins]: ``SF^2 = <(y_j - y_i)^2> - <sigma_i^2 + sigma_j^2>`` over
        the pairs of each bin of ``edges`` (``lag_bins``); without ``subtract_noise`` or ``dy`` the first term alone.  An
        empty bin gives NaN."""
        noise = bool(subtract_noise) and self.dy is not None
        sums = self._sums(edges, sf=True, **({"noise": True} if noise else {}))
        return self._shaped(sf_from_sums(sums, noise))


class DiscreteCorrelation(_LagStatistic):
    """``DiscreteCorrelation(t, y, dy=None)``: the discrete autocorrelation function of Edelson & Krolik (1988); arguments
    as ``StructureFunction``."""

    def dcf(self, edges, subtract_noise=True):
        """-> (mean lag, DCF, error, count), each [nbins] or [L][nbins]: ``DCF_b = sum r_i r_j / (count_b (s^2 - e^2))`` with
        ``r = y - mean(y)``, ``s^2 = sum r^2 / N`` and ``e^2`` the mean of ``dy^2`` (0 without ``subtract_noise`` or
        ``dy``), and Edelson & Krolik's error (NaN for fewer than two pairs).  An empty bin gives NaN."""
        sums = self._sums(edges, cf=True, cf2=True)
        y = np.atleast_2d(self.y)
        s2 = np.mean((y - y.mean(axis=1, keepdims=True)) ** 2, axis=1)
        e2 = np.mean(np.atleast_2d(self.dy) ** 2, axis=1) if subtract_noise and self.dy is not None else np.zeros(len(y))
        return self._shaped(dcf_from_sums(sums, s2, e2))


def cross_lag_bins(t1, t2, nbins, max_lag=None):
    """``nbins + 1`` linear edges from ``-max_lag`` to ``max_lag`` for ``Engine.cross_sums`` (None: half the shorter of the
    two spans).  Bin b holds ``edges[b] <= t2_j - t1_i < edges[b + 1]``."""
    t1, t2 = (np.asarray(t, dtype=np.float64) for t in (t1, t2))
    if t1.ndim != 1 or t2.ndim != 1 or len(t1) < 1 or len(t2) < 1:
        raise ValueError("t1 and t2 must be [N] and [M] with at least one sample each")
    if nbins not in range(1, LAG_MAX_BINS + 1):
        raise ValueError("nbins must lie in 1 .. %d" % LAG_MAX_BINS)
    if max_lag is None:
        max_lag = 0.5 * min(float(t1.max() - t1.min()), float(t2.max() - t2.min()))
    if not np.isfinite(max_lag) or not max_lag > 0:
        raise ValueError("need a finite max_lag > 0, got %r" % (max_lag,))
    edges = np.linspace(-max_lag, max_lag, nbins + 1)
    if not np.all(np.diff(edges) > 0):
        raise ValueError("%d bins within +-%r are narrower than the numbers resolve" % (nbins, max_lag))
    return edges


def ccf_from_sums(sums, s2a, s2b, e2a=0.0, e2b=0.0, normalization="global"):
    """``cross_sums``' sums -> (mean lag, CCF, its error, count), each shaped like the sums.

    ``"global"`` (Edelson & Krolik 1988), from ``count, lag, cf, cf2``: ``cf / (count sqrt((s2a - e2a)(s2b - e2b)))`` with
    the variances ``s2`` = sum r^2 / N of the two series and their mean measurement variances ``e2`` ([L] or scalars), and
    the error ``sqrt(cf2 - cf^2 / count) / ((count - 1) sqrt(...))`` as in ``dcf_from_sums``.
    ``"local"`` (Lehar et al. 1992, Welsh 1999), from all eight sums: with c = count,
    ``(cf/c - (sa/c)(sb/c)) / sqrt((saa/c - (sa/c)^2)(sbb/c - (sb/c)^2))`` -- the means and variances of the samples that
    contribute to the bin -- and the same spread of the products over ``(c - 1)`` times that root as the error.
    A bin with fewer than two pairs gives NaN in CCF and error; so does a variance (product) that is not positive."""
    if normalization not in ("global", "local"):
        raise ValueError("normalization must be 'global' or 'local'")
    count = np.asarray(sums["count"])
    c = count.astype(np.float64)
    two = count >= 2
    safe = np.where(two, c, 2.0)
    cf, cf2 = np.asarray(sums["cf"]), np.asarray(sums["cf2"])
    if normalization == "global":
        va = np.asarray(s2a, dtype=np.float64) - np.asarray(e2a, dtype=np.float64)
        vb = np.asarray(s2b, dtype=np.float64) - np.asarray(e2b, dtype=np.float64)
        va, vb = (np.broadcast_to(v[..., None] if np.ndim(v) else v, cf.shape) for v in (va, vb))
        top = cf / safe
    else:
        ma, mb = np.asarray(sums["sa"]) / safe, np.asarray(sums["sb"]) / safe
        va, vb = np.asarray(sums["saa"]) / safe - ma * ma, np.asarray(sums["sbb"]) / safe - mb * mb
        top = cf / safe - ma * mb
    ok = two & (va > 0) & (vb > 0)
    var = np.where(ok, va * vb, 1.0)
    root = np.sqrt(np.where(ok, var, 1.0))
    spread = np.sqrt(np.maximum(cf2 - cf * cf / safe, 0.0))      # (a negative difference is rounding)
    ccf = np.where(ok, top / root, np.nan)
    err = np.where(ok, spread / ((safe - 1.0) * root), np.nan)
    return _per_pair(sums["lag"], count), ccf, err, count


def lag_peak_and_centroid(lag, ccf, threshold=0.8):
    """The reverberation-mapping summary of a cross-correlation function: per row of ``ccf`` ([nbins] or [L][nbins], with
    the bins' mean lags ``lag`` of the same shape) -> (the lag of the highest finite CCF value, the CCF-weighted centroid
    ``sum lag ccf / sum ccf`` of the bins at or above ``threshold`` x that peak).  A row without a finite value gives NaN
    for both; so does a centroid whose weights do not add up to a positive number (a peak <= 0)."""
    lag, ccf = np.asarray(lag, dtype=np.float64), np.asarray(ccf, dtype=np.float64)
    if lag.shape != ccf.shape or ccf.ndim not in (1, 2):
        raise ValueError("lag and ccf must have the same shape, [nbins] or [L][nbins]")
    if not 0 < threshold <= 1:
        raise ValueError("threshold must lie in (0, 1]")
    L2, C2 = np.atleast_2d(lag), np.atleast_2d(ccf)
    ok = np.isfinite(C2) & np.isfinite(L2)
    any_ok = ok.any(axis=1)
    at = np.argmax(np.where(ok, C2, -np.inf), axis=1)            # (the first maximum)
    rows = np.arange(len(C2))
    top = np.where(any_ok, C2[rows, at], np.nan)
    peak = np.where(any_ok, L2[rows, at], np.nan)
    use = ok & (C2 >= threshold * top[:, None])
    w = np.where(use, C2, 0.0)
    total = w.sum(axis=1)
    good = any_ok & (total > 0)
    centroid = np.where(good, (w * np.where(use, L2, 0.0)).sum(axis=1) / np.where(good, total, 1.0), np.nan)
    if ccf.ndim == 1:
        return float(peak[0]), float(centroid[0])
    return peak, centroid


class CrossCorrelation:
    """``CrossCorrelation(t1, y1, t2, y2, dy1=None, dy2=None)``: the discrete cross-correlation function of two series on
    their own samplings.  ``t1`` [N] ascending with ``y1`` [N] or [L][N], ``t2`` [M] ascending with ``y2`` [M] (one
    companion for every row of ``y1``) or [L][M]; ``dy1``, ``dy2`` None, scalars or shaped like their series.  A positive
    lag means the second series lags the first."""

    def __init__(self, t1, y1, t2, y2, dy1=None, dy2=None, device=0):
        self.t1, self.y1 = np.ascontiguousarray(t1, dtype=np.float64), np.ascontiguousarray(y1, dtype=np.float64)
        self.t2, self.y2 = np.ascontiguousarray(t2, dtype=np.float64), np.ascontiguousarray(y2, dtype=np.float64)
        if self.t1.ndim != 1 or self.y1.ndim not in (1, 2) or self.y1.shape[-1] != len(self.t1):
            raise ValueError("t1 must be [N] and y1 [N] or [L][N]")
        if self.t2.ndim != 1 or self.y2.ndim not in (1, 2) or self.y2.shape[-1] != len(self.t2):
            raise ValueError("t2 must be [M] and y2 [M] or [L][M]")
        if len(self.t1) < 1 or len(self.t2) < 1:
            raise ValueError("each series needs at least one sample")
        if np.any(np.diff(self.t1) < 0) or np.any(np.diff(self.t2) < 0):
            raise ValueError("t1 and t2 must ascend")
        if self.y2.ndim == 2 and (self.y1.ndim != 2 or len(self.y2) != len(self.y1)):
            raise ValueError("y2 [L][M] needs y1 [L][N] with the same L")
        self.dy1 = None if dy1 is None else np.ascontiguousarray(np.broadcast_to(np.asarray(dy1, dtype=np.float64), self.y1.shape))
        self.dy2 = None if dy2 is None else np.ascontiguousarray(np.broadcast_to(np.asarray(dy2, dtype=np.float64), self.y2.shape))
        self.device = device

    def ccf(self, edges, normalization="global", subtract_noise=True):
        """-> (mean lag, CCF, error, count), each [nbins] or [L][nbins], in the bins of ``edges`` (``cross_lag_bins``):
        ``ccf_from_sums`` with ``s^2 = sum r^2 / N`` of each series and, for ``"global"`` with ``subtract_noise``, the
        means of ``dy1^2`` and ``dy2^2`` taken off them.  An empty bin gives NaN."""
        if normalization not in ("global", "local"):
            raise ValueError("normalization must be 'global' or 'local'")
        from .gp import get_engine
        eng = get_engine(self.device)
        y1 = np.atleast_2d(self.y1)
        eng.set_lightcurves(self.t1, y1, np.ones_like(y1) if self.dy1 is None else np.atleast_2d(self.dy1))
        eng.bound_to = None      # the process-wide engine holds this object's light curves now, nobody's evaluator's
        local = normalization == "local"
        sums = eng.cross_sums(self.t2, self.y2, edges, count=True, lag=True, cf=True, cf2=True, sa=local, sb=local, saa=local, sbb=local)
        y2 = np.atleast_2d(self.y2)
        s2a = np.mean((y1 - y1.mean(axis=1, keepdims=True)) ** 2, axis=1)
        s2b = np.mean((y2 - y2.mean(axis=1, keepdims=True)) ** 2, axis=1)
        e2a = np.mean(np.atleast_2d(self.dy1) ** 2, axis=1) if subtract_noise and self.dy1 is not None else 0.0
        e2b = np.mean(np.atleast_2d(self.dy2) ** 2, axis=1) if subtract_noise and self.dy2 is not None else 0.0
        out = ccf_from_sums(sums, s2a, s2b, e2a, e2b, normalization)
        return tuple(a.reshape(self.y1.shape[:-1] + a.shape[-1:]) for a in out)


def iccf_lags(t1, t2, n=201, max_lag=None):
    """``n`` uniform lags from ``-max_lag`` to ``max_lag`` for ``Engine.iccf`` (None: half the shorter of the two spans):
    a symmetric grid, with lag 0 on it when ``n`` is odd."""
    t1, t2 = (np.asarray(t, dtype=np.float64) for t in (t1, t2))
    if t1.ndim != 1 or t2.ndim != 1 or len(t1) < 2 or len(t2) < 2:
        raise ValueError("t1 and t2 must be [N] and [M] with at least two samples each")
    if n not in range(1, ICCF_MAX_LAGS + 1):
        raise ValueError("n must lie in 1 .. %d" % ICCF_MAX_LAGS)
    if max_lag is None:
        max_lag = 0.5 * min(float(t1.max() - t1.min()), float(t2.max() - t2.min()))
    if not np.isfinite(max_lag) or not max_lag > 0:
        raise ValueError("need a finite max_lag > 0, got %r" % (max_lag,))
    return np.linspace(-max_lag, max_lag, n)


class InterpolatedCrossCorrelation:
    """``InterpolatedCrossCorrelation(t1, y1, t2, y2)``: the interpolated cross-correlation function (Gaskell & Peterson
    1987; White & Peterson 1994) of two series on their own samplings, on a lag grid finer than any bin of
    ``CrossCorrelation`` could be.  ``t1`` [N] ascending with ``y1`` [N] or [L][N], ``t2`` [M] ascending with ``y2`` [M]
    (one companion for every row of ``y1``) or [L][M].  A positive lag means the second series lags the first.  One series
    is linearly interpolated at the other's shifted times: across a gap that invents data, so read the counts and
    calibrate with ``ppp.iccf_significance``."""

    def __init__(self, t1, y1, t2, y2, device=0):
        self.t1, self.y1 = np.ascontiguousarray(t1, dtype=np.float64), np.ascontiguousarray(y1, dtype=np.float64)
        self.t2, self.y2 = np.ascontiguousarray(t2, dtype=np.float64), np.ascontiguousarray(y2, dtype=np.float64)
        if self.t1.ndim != 1 or self.y1.ndim not in (1, 2) or self.y1.shape[-1] != len(self.t1):
            raise ValueError("t1 must be [N] and y1 [N] or [L][N]")
        if self.t2.ndim != 1 or self.y2.ndim not in (1, 2) or self.y2.shape[-1] != len(self.t2):
            raise ValueError("t2 must be [M] and y2 [M] or [L][M]")
        if len(self.t1) < 2 or len(self.t2) < 2:
            raise ValueError("each series needs at least two samples")
        if np.any(np.diff(self.t1) < 0) or np.any(np.diff(self.t2) < 0):
            raise ValueError("t1 and t2 must ascend")
        if self.y2.ndim == 2 and (self.y1.ndim != 2 or len(self.y2) != len(self.y1)):
            raise ValueError("y2 [L][M] needs y1 [L][N] with the same L")
        self.device = device

    def _engine(self):
        from .gp import get_engine
        eng = get_engine(self.device)
        y1 = np.atleast_2d(self.y1)
        eng.set_lightcurves(self.t1, y1, np.ones_like(y1))
        eng.bound_to = None      # the process-wide engine holds this object's light curves now, nobody's evaluator's
        return eng

    def ccf(self, lags, mode="both"):
        """-> (ccf, n_a, n_b), each [K] or [L][K]: the function at ``lags`` (``iccf_lags``) and the samples each half
        used; ``mode`` "both", "companion" (the second series interpolated) or "resident" (the first)."""
        got = self._engine().iccf(self.t2, self.y2, lags, mode=mode, values=True, counts=True)
        return tuple(a.reshape(self.y1.shape[:-1] + a.shape[-1:]) for a in (got.ccf, got.n_a, got.n_b))

    def lag(self, lags, mode="both", threshold=0.8):
        """-> (peak lag, centroid, peak value), per row of ``y1`` (floats for one series): the lag of the largest finite
        value, the centroid of the lags at or above ``threshold`` x peak (Peterson et al. 1998), reduced on the device."""
        lags = np.ascontiguousarray(np.atleast_1d(lags), dtype=np.float64).ravel()
        got = self._engine().iccf(self.t2, self.y2, lags, mode=mode, threshold=threshold, values=False, peak=True)
        at = np.where(got.peak_index >= 0, lags[np.maximum(got.peak_index, 0)], np.nan)
        if self.y1.ndim == 1:
            return float(at[0]), float(got.centroid[0]), float(got.peak[0])
        return at, got.centroid, got.peak


def model_structure_function(kernel, lags, jitter=0.0):
    """The curve one overplots: ``SF^2(tau) = 2 (k(0) - k(tau)) + 2 jitter^2`` of a kernel of ``terms`` (on the host,
    through its ``get_value``); ``jitter`` is a white-noise standard deviation not subtracted from the data."""
    lags = np.asarray(lags, dtype=np.float64)
    return 2.0 * (kernel.get_value(np.zeros(())) - kernel.get_value(lags)) + 2.0 * float(jitter) ** 2
