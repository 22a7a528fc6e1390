"""The time-lag view of a light curve on the device: the structure function and the discrete correlation function of
Edelson & Krolik (1988) in bins of the lag ``tau = t_j - t_i`` over the pairs ``i < j`` of the samples -- what one plots to
read off a break timescale or to see a QPO as a dip and a bump, and compares with the model's ``2 (k(0) - k(tau))``.
Defined on the pairs: gaps cost nothing and nothing is interpolated.

The sums over the pairs come from ``Engine.lag_sums`` (``mtg_lag_sums``, include/mtg.h) on the GPU, for one light curve
or a whole set on shared sampling in one call; this module bins, normalises and models.  There is no CPU fallback, as
elsewhere in the package.

    >>> edges = lag_bins(t, 20, spacing="log")
    >>> tau, sf2, count = StructureFunction(t, y, dy).sf(edges)
    >>> model = model_structure_function(kernel, tau)
"""
import numpy as np

from .engine import LAG_MAX_BINS

__all__ = ["lag_bins", "StructureFunction", "DiscreteCorrelation", "model_structure_function", "sf_from_sums", "dcf_from_sums"]


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


def model_structure_function(kernel, lags, jitter=0.0):
    """The curve one overplots: ``SF^2(tau) = 2 (k(0) - k(tau)) + 2 jitter^2`` of a kernel of ``terms`` (on the host,
    through its ``get_value``); ``jitter`` is a white-noise standard deviation not subtracted from the data."""
    lags = np.asarray(lags, dtype=np.float64)
    return 2.0 * (kernel.get_value(np.zeros(())) - kernel.get_value(lags)) + 2.0 * float(jitter) ** 2
