"""Mean functions (API of /root/reference/mind_the_gaps/models/mean_models.py:6-31).

Through its ``meanmodel`` strings ``GPModelling`` reaches the constant and the linear mean only
(gpmodelling.py:27,83-111); every class here is evaluated inside the kernels (``mtg_mean_kind``: MTG_MEAN_LINEAR,
MTG_MEAN_SINE, MTG_MEAN_TWOSINE, MTG_MEAN_GAUSSIAN of include/mtg.h) and can be fitted with the kernel, by handing
``GP`` / ``GPModelling`` an instance.  ``get_value`` is the reference's formula, operation for operation.
"""
import numpy as np

from .. import engine as _engine
from ..modeling import Model

__all__ = ["LinearModel", "GaussianModel", "SineModel", "TwoSineModel"]


class LinearModel(Model):
    """slope * t + intercept, fitted on the device (mean_models.py:24-31)."""

    parameter_names = ("slope", "intercept")
    mtg_mean_kind = _engine.MEAN_LINEAR

    def get_value(self, x):
        return np.add(np.multiply(self.slope, x), self.intercept)

    def compute_gradient(self, x):
        x = np.asarray(x, dtype=np.float64)
        return np.vstack([x, np.ones_like(x)])          # d/d slope, d/d intercept


class GaussianModel(Model):
    """Gaussian bump on a constant level; note the reference's normalisation
    amplitude / (2 pi sigma) (mean_models.py:9-10), kept as is."""

    parameter_names = ("mean", "sigma", "amplitude", "constant")
    mtg_mean_kind = _engine.MEAN_GAUSSIAN

    def get_value(self, x):
        x = np.asarray(x, dtype=np.float64)
        return self.amplitude / (2 * np.pi * self.sigma) * np.exp(-(x - self.mean) ** 2 / (2 * self.sigma ** 2)) + self.constant


class SineModel(Model):
    """constant + amplitude sin(frequency t + phase) (mean_models.py:12-16)."""

    parameter_names = ("constant", "amplitude", "frequency", "phase")
    mtg_mean_kind = _engine.MEAN_SINE

    def get_value(self, x):
        return self.constant + self.amplitude * np.sin(np.multiply(self.frequency, x) + self.phase)


class TwoSineModel(Model):
    """constant + amplitude0 sin(frequency t + phase0) + amplitude1 sin(2 frequency t + phase1): a fundamental and its
    first harmonic (mean_models.py:18-22)."""

    parameter_names = ("constant", "amplitude0", "phase0", "amplitude1", "phase1", "frequency")
    mtg_mean_kind = _engine.MEAN_TWOSINE

    def get_value(self, x):
        x = np.asarray(x, dtype=np.float64)
        return (self.constant + self.amplitude0 * np.sin(self.frequency * x + self.phase0)
                + self.amplitude1 * np.sin(2 * self.frequency * x + self.phase1))
