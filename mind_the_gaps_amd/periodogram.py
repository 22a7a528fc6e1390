"""Lomb-Scargle periodogram on the device: the part of ``astropy.timeseries.LombScargle`` the reference's workflow uses
(``lomb_scargle_biases.ipynb``: ``LombScargle(t, y, fit_mean=True, nterms=1, center_data=True, normalization=...)`` and
``.power(frequencies)``), for one light curve or for a whole set on shared sampling in one call.

The periodogram is the generalised (floating-mean) one of Zechmeister & Kuerster (2009), evaluated by ``mtg_lomb_scargle``
(include/mtg.h) on the GPU.  There is no CPU fallback, as elsewhere in the package.
"""
import numpy as np

from .engine import LS_NORMALIZATIONS

__all__ = ["LombScargle"]


class LombScargle:
    """``LombScargle(t, y, dy=None, fit_mean=True, center_data=True, nterms=1, normalization="standard")``.

    ``t`` [N] (ascending), ``y`` [N] or [L][N] (L light curves on the sampling ``t``), ``dy`` None (unweighted), a scalar,
    [N] or [L][N].  Only astropy's defaults ``fit_mean=True, center_data=True, nterms=1`` exist on the device; anything
    else raises ``NotImplementedError``."""

    def __init__(self, t, y, dy=None, fit_mean=True, center_data=True, nterms=1, normalization="standard", device=0):
        for name, value, only in (("fit_mean", fit_mean, True), ("center_data", center_data, True), ("nterms", nterms, 1)):
            if value != only:
                raise NotImplementedError("LombScargle(%s=%r): only %s=%r runs on the device" % (name, value, name, only))
        if normalization not in LS_NORMALIZATIONS:
            raise ValueError("normalization must be one of %s" % sorted(LS_NORMALIZATIONS))
        self.t = np.ascontiguousarray(t, dtype=np.float64)
        self.y = np.ascontiguousarray(y, dtype=np.float64)
        if self.t.ndim != 1 or self.y.ndim not in (1, 2) or self.y.shape[-1] != len(self.t):
            raise ValueError("t must be [N] and y [N] or [L][N]")
        self.dy = None if dy is None else np.ascontiguousarray(np.broadcast_to(np.asarray(dy, dtype=np.float64), self.y.shape))
        self.normalization = normalization
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
        out = self._bound_engine().lomb_scargle(frequency.ravel(), normalization=normalization or self.normalization,
                                                weighted=self.dy is not None)
        return out.reshape(self.y.shape[:-1] + frequency.shape)

    def autopower(self, **kwargs):
        frequency = self.autofrequency(**kwargs)
        return frequency, self.power(frequency)
