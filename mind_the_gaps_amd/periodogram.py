"""Lomb-Scargle periodogram on the device: the part of ``astropy.timeseries.LombScargle`` the reference's workflow uses
(``lomb_scargle_biases.ipynb``: ``LombScargle(t, y, fit_mean=True, nterms=1, center_data=True, normalization=...)`` and
``.power(frequencies)``), for one light curve or for a whole set on shared sampling in one call -- and ``nterms`` up to 5 (not 2: see the class),
the batched form of the reference's ``utils.fit_sines`` (phase-tied harmonics at one frequency) over a frequency grid.

``envelope_ranks`` / ``envelope_levels`` turn the order statistics of ``Engine.lomb_scargle_envelope`` into the quantiles
``np.quantile(power, levels, axis=0)`` would give, without the [L][F] power array.

The periodogram is the generalised (floating-mean) one of Zechmeister & Kuerster (2009), evaluated by ``mtg_lomb_scargle``
(include/mtg.h) on the GPU.  There is no CPU fallback, as elsewhere in the package.
"""
import numpy as np

from .engine import EF_MAX_BINS, LS_MAX_TERMS, LS_NORMALIZATIONS, WWZ_DECAY, WWZ_STATISTICS

__all__ = ["LombScargle", "EpochFolding", "WWZ", "phase_fold", "envelope_ranks", "envelope_levels"]


class _Periodogram:
    """What ``LombScargle`` and ``EpochFolding`` share: the data, astropy's automatic frequency grid, and ``power`` through
    the process-wide engine.  A statistic says in ``_powers(engine, frequencies, normalization)`` which entry it calls."""

    def _set_data(self, t, y, dy, device):
        self.t = np.ascontiguousarray(t, dtype=np.float64)
        self.y = np.ascontiguousarray(y, dtype=np.float64)
        if self.t.ndim != 1 or self.y.ndim not in (1, 2) or self.y.shape[-1] != len(self.t):
            raise ValueError("t must be [N] and y [N] or [L][N]")
        self.dy = None if dy is None else np.ascontiguousarray(np.broadcast_to(np.asarray(dy, dtype=np.float64), self.y.shape))
        self.device = device

    def autofrequency(self, samples_per_peak=5, nyquist_factor=5, minimum_frequency=None, maximum_frequency=None):
        """astropy's automatic grid: spacing ``1 / (samples_per_peak T)`` from half a spacing (or ``minimum_frequency``) up
        to ``nyquist_factor`` times the average Nyquist frequency ``N / (2 T)`` (or ``maximum_frequency``)."""
        baseline = self.t.max() - self.t.min()
        n_samples = len(self.t)
        df = 1.0 / baseline / samples_per_peak
        if minimum_frequency is None:
            minimum_frequency = 0.5 * df
        if maximum_frequency is None:
            maximum_frequency = nyquist_factor * (0.5 * n_samples / baseline)
        nf = int(np.round(1 + (maximum_frequency - minimum_frequency) / df))
        return minimum_frequency + df * np.arange(nf)

    def _bound_engine(self):
        from .gp import get_engine
        eng = get_engine(self.device)
        y = np.atleast_2d(self.y)
        eng.set_lightcurves(self.t, y, np.ones_like(y) if self.dy is None else np.atleast_2d(self.dy))
        eng.bound_to = None      # the process-wide engine holds this object's light curves now, nobody's evaluator's
        return eng

    def power(self, frequency, normalization=None):
        """The periodogram at ``frequency`` (cycles per unit of ``t``) -> [F], or [L][F] for a set."""
        frequency = np.asarray(frequency, dtype=np.float64)
        out = self._powers(self._bound_engine(), frequency.ravel(), normalization or self.normalization)
        return out.reshape(self.y.shape[:-1] + frequency.shape)

    def autopower(self, **kwargs):
        frequency = self.autofrequency(**kwargs)
        return frequency, self.power(frequency)


class LombScargle(_Periodogram):
    """``LombScargle(t, y, dy=None, fit_mean=True, center_data=True, nterms=1, normalization="standard")``.

    ``t`` [N] (ascending), ``y`` [N] or [L][N] (L light curves on the sampling ``t``), ``dy`` None (unweighted), a scalar,
    [N] or [L][N].  ``nterms`` = 1, 3, 4 or 5 harmonics (beyond one: astropy's ``chi2`` method, N >= 2 nterms + 2 samples);
    ``nterms=2`` raises ``NotImplementedError`` here and runs through ``Engine.lomb_scargle(nterms=2)``.  Only astropy's
    defaults ``fit_mean=True, center_data=True`` exist on the device; anything else raises ``NotImplementedError``."""

    def __init__(self, t, y, dy=None, fit_mean=True, center_data=True, nterms=1, normalization="standard", device=0):
        for name, value, only in (("fit_mean", fit_mean, True), ("center_data", center_data, True)):
            if value != only:
                raise NotImplementedError("LombScargle(%s=%r): only %s=%r runs on the device" % (name, value, name, only))
        if nterms == 2:
            raise NotImplementedError("LombScargle(nterms=2): this class takes nterms = 1, 3, 4, 5; two harmonics run through "
                                      "Engine.lomb_scargle(nterms=2)")
        if nterms not in range(1, LS_MAX_TERMS + 1):
            raise NotImplementedError("LombScargle(nterms=%r): nterms = 1 .. %d run on the device" % (nterms, LS_MAX_TERMS))
        if normalization not in LS_NORMALIZATIONS:
            raise ValueError("normalization must be one of %s" % sorted(LS_NORMALIZATIONS))
        self._set_data(t, y, dy, device)
        self.normalization = normalization
        self.nterms = int(nterms)

    def _powers(self, eng, frequency, normalization):
        return eng.lomb_scargle(frequency, normalization=normalization, weighted=self.dy is not None, nterms=self.nterms)


class EpochFolding(_Periodogram):
    """``EpochFolding(t, y, dy=None, nbins=10, time_0=None, normalization="standard")``: the epoch-folding periodogram of
    Leahy et al. (1983) with ``LombScargle``'s interface -- ``power``, ``autofrequency``, ``autopower``.  ``nbins`` phase
    bins (2 .. 32) counted from ``time_0`` (None: ``t[0]``); ``normalization`` one of ``LombScargle``'s or ``"chi2"``
    (Leahy's statistic, twice ``"psd"``).  ``Engine.epoch_fold`` has the definition."""

    def __init__(self, t, y, dy=None, nbins=10, time_0=None, normalization="standard", device=0):
        if nbins not in range(2, EF_MAX_BINS + 1):
            raise ValueError("nbins must lie in 2 .. %d" % EF_MAX_BINS)
        if normalization != "chi2" and normalization not in LS_NORMALIZATIONS:
            raise ValueError("normalization must be one of %s" % sorted(list(LS_NORMALIZATIONS) + ["chi2"]))
        self._set_data(t, y, dy, device)
        self.normalization = normalization
        self.nbins = int(nbins)
        self.time_0 = None if time_0 is None else float(time_0)

    def _powers(self, eng, frequency, normalization):
        return eng.epoch_fold(frequency, nbins=self.nbins, time_0=self.time_0, normalization=normalization, weighted=self.dy is not None)


class WWZ(_Periodogram):
    """``WWZ(t, y, dy=None, decay=1 / (8 pi^2), statistic="z")``: Foster's weighted wavelet Z-transform (1996), the
    time-frequency map of a light curve (or of a set [L][N] on the sampling ``t``) -- when was a periodicity there, and did
    its period move?  ``dy=None`` is unweighted, as in ``LombScargle``; ``decay`` is Foster's c, the window
    ``exp(-4 pi^2 c (f (t - tau))^2)``; ``statistic`` one of ``"z"``, ``"power"``, ``"amplitude"``.  ``power(frequency,
    tau)`` and ``neff(frequency, tau)`` return [T][F] (a set: [L][T][F]); ``autofrequency`` is ``LombScargle``'s and
    ``autotau(n)`` spreads n centres evenly over the time span.  ``Engine.wwz`` has the definition."""

    def __init__(self, t, y, dy=None, decay=WWZ_DECAY, statistic="z", device=0):
        if statistic not in WWZ_STATISTICS:
            raise ValueError("statistic must be one of %s" % sorted(WWZ_STATISTICS))
        if not (np.isfinite(decay) and decay >= 0):
            raise ValueError("decay must be finite and >= 0")
        self._set_data(t, y, dy, device)
        self.decay = float(decay)
        self.statistic = statistic

    def autotau(self, n=50):
        """``n`` window centres evenly spaced from the first to the last time"""
        if n < 1:
            raise ValueError("n must be at least 1")
        return np.linspace(self.t.min(), self.t.max(), int(n))

    def _map(self, frequency, tau, statistic, **what):
        frequency = np.asarray(frequency, dtype=np.float64)
        tau = np.asarray(tau, dtype=np.float64)
        if statistic not in WWZ_STATISTICS:
            raise ValueError("statistic must be one of %s" % sorted(WWZ_STATISTICS))
        out = self._bound_engine().wwz(frequency.ravel(), tau.ravel(), decay=self.decay, statistic=statistic,
                                       weighted=self.dy is not None, **what)
        return out.reshape(self.y.shape[:-1] + (tau.size, frequency.size))

    def power(self, frequency, tau, statistic=None):
        """The map at ``frequency`` [F] and the centres ``tau`` [T] -> [T][F], or [L][T][F] for a set."""
        return self._map(frequency, tau, statistic or self.statistic, values=True)

    def neff(self, frequency, tau):
        """Foster's effective number of samples under the window of every ``(tau, frequency)``: shapes as ``power``."""
        return self._map(frequency, tau, self.statistic, values=False, neff=True)

    def autopower(self, n_tau=50, **kwargs):
        """-> ``(frequency, tau, map)`` on ``autofrequency(**kwargs)`` and ``autotau(n_tau)``"""
        frequency, tau = self.autofrequency(**kwargs), self.autotau(n_tau)
        return frequency, tau, self.power(frequency, tau)


def phase_fold(timestamps, y, folding_frequency, dy=None, time_0=0, n_bins=10, device=0):
    """The reference's ``utils.phase_fold``: the light curve folded at ``folding_frequency`` from ``time_0`` into ``n_bins``
    phase bins -> ``(bin_means, bin_stds, two_phase_bins)``, each over two cycles: the unweighted mean of every bin, its
    error ``sqrt(sum dy^2) / count`` (NaN without ``dy``) and the bins' phases.  Computed on the device
    (``Engine.phase_fold``), with a sample's bin taken from the exact product ``f (t - time_0)``.  Two departures from the
    reference: the phases returned are the bin centres ``(bins + 0.5) / n_bins`` (the reference's ``bins / n_bins + 0.05``
    is the centre only for ten bins), and an empty bin is NaN in both arrays without a warning (the reference averages an
    empty slice, which warns)."""
    t = np.ascontiguousarray(timestamps, dtype=np.float64)
    y = np.ascontiguousarray(y, dtype=np.float64)
    if t.ndim != 1 or y.shape != t.shape:
        raise ValueError("timestamps and y must be [N]")
    fold = EpochFolding(t, y, dy=dy, nbins=n_bins, device=device)
    count, wsum, wrsum, varsum = (a[0, 0] for a in fold._bound_engine().phase_fold([float(folding_frequency)], nbins=fold.nbins,
                                                                                   time_0=float(time_0), weighted=False))
    filled = count > 0
    bin_means = np.full(fold.nbins, np.nan)
    bin_stds = np.full(fold.nbins, np.nan)
    bin_means[filled] = y.mean() + wrsum[filled] / wsum[filled]
    if dy is not None:
        bin_stds[filled] = np.sqrt(varsum[filled]) / count[filled]
    bins = (np.arange(fold.nbins) + 0.5) / fold.nbins
    return np.hstack([bin_means, bin_means]), np.hstack([bin_stds, bin_stds]), np.hstack([bins, bins + 1])


def _virtual_index(L, levels):
    """numpy's position of a quantile in a sorted sample of L (method "linear": (L - 1) q, as numpy 2 forms it), with the
    two neighbouring ranks: beyond the last rank the last one."""
    levels = np.atleast_1d(np.asarray(levels, dtype=np.float64))
    if levels.ndim != 1 or not np.all((levels >= 0) & (levels <= 1)):
        raise ValueError("levels must lie in [0, 1]")
    virtual = (L - 1) * levels
    lower = np.floor(virtual).astype(np.int64)
    upper = lower + 1
    upper[upper > L - 1] = L - 1
    lower[lower > L - 1] = L - 1
    lower[lower < 0] = 0
    return virtual, lower, upper


def envelope_ranks(L, levels):
    """The ranks ``Engine.lomb_scargle_envelope`` has to return for ``envelope_levels(..., L, levels)``: the two
    neighbours of every level's position in a sorted sample of L, and the last rank L - 1, which tells whether a column
    holds a NaN -> ascending int64, without duplicates."""
    L = int(L)
    if L < 1:
        raise ValueError("L must be at least 1")
    _, lower, upper = _virtual_index(L, levels)
    return np.unique(np.concatenate([lower, upper, [L - 1]])).astype(np.int64)


def envelope_levels(order_stat, ranks, L, levels):
    """``np.quantile(power, levels, axis=0)`` (numpy's default "linear" rule) from order statistics alone:
    ``order_stat[q]`` is the row of rank ``ranks[q]`` of ``np.sort(power, axis=0)``, ``L = len(power)``.  -> [len(levels)][F];
    a column with a NaN gives NaN, as numpy's does.  ``ranks`` must hold ``envelope_ranks(L, levels)``.  The interpolation is
    written as numpy writes it (``a + (b - a) t``, and ``b - (b - a) (1 - t)`` from t = 1/2 on), so the result is numpy's
    bit for bit."""
    order_stat = np.atleast_2d(np.asarray(order_stat, dtype=np.float64))
    where = {int(r): q for q, r in enumerate(np.atleast_1d(ranks))}
    L = int(L)
    virtual, lower, upper = _virtual_index(L, levels)
    missing = sorted(set(map(int, np.concatenate([lower, upper, [L - 1]]))) - set(where))
    if missing:
        raise ValueError("ranks lack %s (envelope_ranks gives what is needed)" % missing)
    a = order_stat[[where[int(r)] for r in lower]]
    b = order_stat[[where[int(r)] for r in upper]]
    t = (virtual - lower).reshape(-1, 1)
    diff = b - a
    out = a + diff * t
    np.subtract(b, diff * (1 - t), out=out, where=t >= 0.5)
    out[:, np.isnan(order_stat[where[L - 1]])] = np.nan
    return out
