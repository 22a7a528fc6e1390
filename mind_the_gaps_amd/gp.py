"""``GP``: the celerite.GP interface of the hot path, evaluated on MI355X.

Host-side mirror of what /root/reference/mind_the_gaps/gpmodelling.py does with
``celerite.GP`` (third-party; semantics restated in SURVEY.md Appendix A.1/A.2):

    gp = GP(kernel, mean=meanmodel, fit_mean=fit_mean)        gpmodelling.py:51
    gp.compute(times, dy + 1e-12)                             gpmodelling.py:54
    gp.get_parameter_vector() / set_parameter_vector(theta)   gpmodelling.py:55,147
    gp.log_prior(); gp.log_likelihood(y)                      gpmodelling.py:149-152
    gp.get_parameter_bounds() / get_parameter_names()         gpmodelling.py:193,454

Every likelihood value comes from the HIP kernels through the C-ABI
(engine.Engine).  There is no host fallback: without libmtg_hip.so or a GPU the
first evaluation raises ``EngineUnavailable``.

Beyond celerite's one-theta-at-a-time calls, ``LogProbEvaluator`` exposes the
batched form the ensemble sampler and the finite-difference gradient use:
``evaluate(theta[B, P], lc_index[B]) -> (lnP[B], status[B])`` over L resident
light curves.
"""
import numpy as np

from . import engine as _engine
from .modeling import ConstantModel, Model, ModelSet
from .terms import Term

__all__ = ["GP", "LinAlgError", "LogProbEvaluator", "DeviceModel", "get_engine"]


class LinAlgError(Exception):
    """The covariance matrix is not positive definite (celerite.solver.LinAlgError)."""


_engines = {}


def get_engine(device=0):
    """Process-wide engine (one ``mtg_ctx``) per GPU."""
    eng = _engines.get(device)
    if eng is None:
        eng = _engine.Engine(device)
        eng.bound_to = None
        _engines[device] = eng
    return eng


_side_engines = {}


def get_side_engine(device=0, k=0):
    """The k-th extra context of a GPU, kept for the life of the process: work that runs BESIDE the process-wide engine's
    (or beside another side engine's) from another host thread -- the two models of the Protassov test.  Kept and reused
    rather than made per call: HIP deals its streams round the hardware queues in the order they are created (four queues
    by default), and two contexts whose streams land on the same queue run their kernels strictly one after the other
    (measured: the refits of a 250-light-curve block side by side 3.56 s, on one queue 4.09 s = one after the other)."""
    key = (device, int(k))
    eng = _side_engines.get(key)
    if eng is None:
        eng = _engine.Engine(device)
        eng.bound_to = None
        _side_engines[key] = eng
    return eng


def _inf_bounds(bounds):
    out = np.empty((len(bounds), 2), dtype=np.float64)
    for i, (lo, hi) in enumerate(bounds):
        out[i, 0] = -np.inf if lo is None else lo
        out[i, 1] = np.inf if hi is None else hi
    return out


class DeviceModel:
    """Flattened (kernel, mean) description handed to ``mtg_set_model``.

    ``device_terms`` is False when some term has no ``mtg_kind`` (a user-defined
    Python term): coefficients are then evaluated on the host per theta and sent
    through ``mtg_loglike_coeffs``.
    """

    def __init__(self, kernel, mean, mean_unfrozen):
        self.terms = list(kernel.terms)
        self.kinds = [t.mtg_kind for t in self.terms]
        self.device_terms = all(k is not None for k in self.kinds)
        self.extra = [float(t.mtg_extra()) for t in self.terms]
        if isinstance(mean, ConstantModel):
            self.mean_kind = _engine.MEAN_CONSTANT
        elif getattr(mean, "mtg_mean_kind", None) is not None:
            self.mean_kind = mean.mtg_mean_kind
        else:
            self.mean_kind = None  # host-evaluated mean: only a frozen one is supported
        kfull = kernel.get_parameter_vector(include_frozen=True)
        kmask = np.atleast_1d(kernel.unfrozen_mask).astype(bool)
        kbounds = kernel.get_parameter_bounds(include_frozen=True)
        if self.mean_kind is None:
            mfull, mmask, mbounds = np.zeros(1), np.zeros(1, dtype=bool), [(None, None)]
        else:
            mfull = mean.get_parameter_vector(include_frozen=True)
            mmask = np.atleast_1d(mean_unfrozen).astype(bool)
            mbounds = mean.get_parameter_bounds(include_frozen=True)
        self.nk = len(kfull)
        self.full = np.concatenate([kfull, mfull]).astype(np.float64)
        self.mask = np.concatenate([kmask, mmask])
        self.free_index = np.flatnonzero(self.mask).astype(np.int32)
        self.bounds = _inf_bounds(list(kbounds) + list(mbounds))
        # A frozen constant mean -- the reference default, ConstantModel(lightcurve.mean)
        # with fit_mean=False (gpmodelling.py:83-87) -- is subtracted from y once at upload
        # (mtg_set_lightcurves y_offset); the device model then carries a mean of exactly 0
        # and its bounds move with it, so the box prior still vetoes an out-of-range value.
        self.y_offset = None
        if self.mean_kind == _engine.MEAN_CONSTANT and not self.mask[self.nk]:
            self.y_offset = float(self.full[self.nk])
            self.bounds[self.nk] -= self.y_offset
            self.full[self.nk] = 0.0

    def signature(self):
        frozen = self.full[~self.mask]
        return (tuple(-1 if k is None else k for k in self.kinds), tuple(self.extra), self.mean_kind,
                self.mask.tobytes(), frozen.tobytes(), self.bounds.tobytes(), self.y_offset)


class LogProbEvaluator:
    """L light curves resident on one GPU + one model; batched lnP / lnL.

    ``t``: [N] shared sampling (gpmodelling.py:538 gives every simulated light
    curve the observed ``times``) or [L][N]; ``y``, ``yerr``: [N] or [L][N];
    ``yerr`` is what the reference passes to ``gp.compute``, i.e. ``dy + 1e-12``
    (gpmodelling.py:54); the device squares it.
    """

    def __init__(self, t, y, yerr, device=0, y_offset=None, own_engine=False):
        """``y_offset``: [L] frozen per-light-curve means; when None a model with a frozen
        constant mean supplies its value for every light curve.  ``own_engine``: a context of its own instead of
        the process-wide one of ``get_engine`` (for work that runs beside other work on the same GPU, from another
        host thread; ``close()`` frees it)."""
        self.t = np.ascontiguousarray(t, dtype=np.float64)
        self.y = np.atleast_2d(np.ascontiguousarray(y, dtype=np.float64))
        self.yerr = np.atleast_2d(np.ascontiguousarray(yerr, dtype=np.float64))
        if self.yerr.shape != self.y.shape:
            raise ValueError("dimension mismatch")
        self.device = device
        self.y_offset = None if y_offset is None else np.ascontiguousarray(y_offset, dtype=np.float64)
        self._model_sig = None
        self._bound_offset = None
        self._token = object()
        self._own = None
        self._own_is_mine = False
        if isinstance(own_engine, tuple) and own_engine and own_engine[0] == "side":
            self._own = get_side_engine(device, own_engine[1])      # ("side", k): the process's k-th extra context, reused
        elif own_engine:     # True, or (part, parts): a context of its own on that slice of the compute units
            self._own = _engine.Engine(device, cu_slice=None if own_engine is True else tuple(own_engine))
            self._own.bound_to = None
            self._own_is_mine = True

    def close(self):
        if self._own is not None:
            if self._own_is_mine:
                self._own.close()
            elif self._own.bound_to is self._token:
                self._own.bound_to = None       # a side engine goes back to the pool; its resident set is nobody's now
            self._own = None

    @property
    def n_lightcurves(self):
        return self.y.shape[0]

    def _bind_lightcurves(self):
        """The engine with these light curves resident and no particular model (tabulated spectra)."""
        class _NoModel:
            device_terms = ()
        return self._bind(_NoModel())

    def _bind(self, model):
        eng = self._own if self._own is not None else get_engine(self.device)
        offset = self.y_offset if self.y_offset is not None else getattr(model, "y_offset", None)
        key = None if offset is None else np.asarray(offset, dtype=np.float64).tobytes()
        if eng.bound_to is not self._token or key != self._bound_offset:
            eng.set_lightcurves(self.t, self.y, self.yerr, y_offset=offset)
            eng.bound_to = self._token
            self._bound_offset = key
            self._model_sig = None
        if model.device_terms:
            sig = model.signature()
            if sig != self._model_sig:
                eng.set_model(model.kinds, model.full, model.free_index, model.bounds,
                              mean_kind=model.mean_kind, extra=model.extra)
                self._model_sig = sig
        return eng

    def evaluate(self, model, theta, lc_index=None, add_prior=True):
        """theta [B][P] -> (lnP [B], status [B]); ``model`` is a DeviceModel."""
        if not model.device_terms:
            raise ValueError("batched evaluation needs device-expandable terms")
        if model.mean_kind is None:
            raise NotImplementedError("a mean model without mtg_mean_kind does not run on the device")
        eng = self._bind(model)
        return eng.loglike(theta, lc_index, add_prior=add_prior)

    def evaluate_coefficients(self, model, coeffs, jitter, mean_params, lc_index=None):
        """Host-evaluated celerite coefficients [B][j]; mean_params [B][engine.MEAN_NPARAMS[kind]] are the
        device-side mean parameters (0 for a frozen constant mean, see DeviceModel)."""
        eng = self._bind(model)
        ar, cr, ac, bc, cc, dc = coeffs
        return eng.loglike_coeffs(ar, cr, ac, bc, cc, dc, jitter=jitter, mean_kind=model.mean_kind,
                                  mean_params=mean_params, lc_index=lc_index)


class GP(ModelSet):
    """celerite.GP look-alike; parameters are ``kernel:*`` then ``mean:*``."""

    def __init__(self, kernel, mean=0.0, fit_mean=False, log_white_noise=None, fit_white_noise=False, device=0, own_engine=False):
        if not isinstance(kernel, Term):
            raise TypeError("kernel must be a mind_the_gaps_amd Term")
        if log_white_noise is not None:
            # celerite's extra diagonal model; the reference never passes one (its notebooks give fit_white_noise=False
            # with the default None, docs/notebooks/poisson_level.ipynb cell 5): white noise goes in as a JitterTerm
            raise NotImplementedError("log_white_noise: add a JitterTerm to the kernel instead")
        try:
            mean = ConstantModel(float(mean))
        except TypeError:
            if not isinstance(mean, Model):
                raise
        if not fit_mean:
            mean.freeze_all_parameters()
        super().__init__([("kernel", kernel), ("mean", mean)])
        self.device = device
        self._own_engine = own_engine    # a device context of this GP's own (work that runs beside other work, from another thread)
        self._t = None
        self._yerr = None
        self._evaluator = None
        self._y_bound = None

    # -- celerite.GP API ---------------------------------------------------------
    @property
    def mean(self):
        return self.models["mean"]

    @property
    def kernel(self):
        return self.models["kernel"]

    @property
    def computed(self):
        return self._t is not None

    def compute(self, t, yerr=1.123e-12, check_sorted=True):
        """Bind the sampling ``t`` and the per-point standard deviations ``yerr``."""
        t = np.atleast_1d(np.asarray(t, dtype=np.float64))
        if t.ndim != 1:
            raise ValueError("dimension mismatch")
        if check_sorted and np.any(np.diff(t) < 0.0):
            raise ValueError("the input coordinates must be sorted")
        self._t = t
        self._yerr = np.empty_like(t)
        self._yerr[:] = yerr
        self._evaluator = None

    def _device_model(self):
        return DeviceModel(self.kernel, self.mean, self.mean.unfrozen_mask)

    def release_engine(self):
        """Give a context of this GP's own back (``own_engine=True``); later calls use the process-wide engine."""
        self._own_engine = False
        if self._evaluator is not None:
            self._evaluator.close()

    def _ensure_evaluator(self, y):
        if self._t is None:
            raise RuntimeError("you must call 'compute' first")
        y = np.asarray(y, dtype=np.float64)
        if y.shape != self._t.shape:
            raise ValueError("dimension mismatch")
        if self._evaluator is None or self._y_bound is None or not np.array_equal(self._y_bound, y):
            if self._evaluator is not None:
                self._evaluator.close()
            self._evaluator = LogProbEvaluator(self._t, y, self._yerr, device=self.device, own_engine=self._own_engine)
            self._y_bound = y.copy()
        return self._evaluator

    def log_likelihood(self, y, quiet=False):
        """ln L of the current parameter vector (gpmodelling.py:152,169)."""
        ev = self._ensure_evaluator(y)
        model = self._device_model()
        if model.mean_kind is None:
            raise NotImplementedError("a mean model without mtg_mean_kind does not run on the device")
        if model.device_terms:
            out, status = ev.evaluate(model, model.full[model.free_index][None, :], add_prior=False)
        else:
            coeffs = tuple(c[None, :] for c in self.kernel.coefficients)
            out, status = ev.evaluate_coefficients(
                model, coeffs, np.array([self.kernel.jitter]), model.full[model.nk:][None, :])
        if status[0] == _engine.ST_NOTPD:
            if quiet:
                return -np.inf
            raise LinAlgError("failed to factorize or solve matrix")
        return float(out[0])

    def grad_log_likelihood(self, y, quiet=False):
        """``(lnL, d lnL / d theta)`` of the current parameter vector, the gradient by the free parameters in
        ``get_parameter_vector``'s order (celerite.GP.grad_log_likelihood): analytic, from one launch of the device's
        tangent sweep (``Engine.loglike_grad``).  A covariance that is not positive definite raises ``LinAlgError``, or
        with ``quiet`` returns ``(-inf, zeros)`` as celerite does.  The tangent sweep knows the constant and the linear
        mean: a profile mean (sine, two sines, Gaussian) raises ``NotImplementedError``."""
        eng, model = self._bound_engine(y)
        out, grad, status = eng.loglike_grad(model.full[model.free_index][None, :], add_prior=False)
        if status[0] == _engine.ST_NOTPD:
            if quiet:
                return -np.inf, np.zeros(len(model.free_index))
            raise LinAlgError("failed to factorize or solve matrix")
        return float(out[0]), grad[0]

    def log_probability_grad_batch(self, theta, y, add_prior=True):
        """lnP and its gradient for B free-parameter vectors at once -> (lnP[B], grad[B][P], status[B]); the box prior
        is flat, so it only rejects rows (-inf, a gradient of NaN).  Pure in theta."""
        eng, _ = self._bound_engine(y)
        return eng.loglike_grad(np.atleast_2d(np.asarray(theta, dtype=np.float64)), add_prior=add_prior)

    def log_probability_batch(self, theta, y, add_prior=True):
        """lnP of B free-parameter vectors at once -> (lnP[B], status[B]); pure in theta."""
        ev = self._ensure_evaluator(y)
        theta = np.atleast_2d(np.asarray(theta, dtype=np.float64))
        model = self._device_model()
        if model.device_terms:
            return ev.evaluate(model, theta, add_prior=add_prior)
        return self._host_coefficient_batch(ev, model, theta, add_prior)

    def _host_coefficient_batch(self, ev, model, theta, add_prior):
        """User-defined Python terms: coefficients on the host, recurrence on the device."""
        saved = self.get_parameter_vector()
        B = theta.shape[0]
        rows, jit, means, keep = [], [], [], np.ones(B, dtype=bool)
        try:
            for b in range(B):
                self.set_parameter_vector(theta[b])
                if add_prior and not np.isfinite(self.log_prior()):
                    keep[b] = False
                    continue
                rows.append(self.kernel.coefficients)
                jit.append(self.kernel.jitter)
                mvec = self.mean.get_parameter_vector(include_frozen=True).copy()
                if model.y_offset is not None:
                    mvec[0] = 0.0      # folded into y at upload
                means.append(mvec)
        finally:
            self.set_parameter_vector(saved)
        out = np.full(B, -np.inf)
        status = np.full(B, _engine.ST_PRIOR, dtype=np.int32)
        if rows:
            shapes = {tuple(len(c) for c in r) for r in rows}
            if len(shapes) != 1:
                raise ValueError("host-evaluated terms must keep one structure across the batch")
            coeffs = tuple(np.array([r[i] for r in rows]).reshape(len(rows), -1) for i in range(6))
            o, s = ev.evaluate_coefficients(model, coeffs, np.array(jit), np.array(means))
            out[keep], status[keep] = o, s
        return out, status

    def _bound_engine(self, y, profile_ok=False):
        """(engine with ``y`` and the model bound, the model).  ``profile_ok``: the caller's device entry works under a
        profile mean too (``apply_inverse``, which does not read the mean); the others know the constant and the linear
        mean only, and ``predict`` / ``sample`` go through ``_zero_mean_engine`` instead."""
        ev = self._ensure_evaluator(y)
        model = self._device_model()
        if not model.device_terms or model.mean_kind is None:
            raise NotImplementedError("needs device-expandable terms and a mean model with mtg_mean_kind")
        if model.mean_kind in _engine.PROFILE_MEANS and not profile_ok:
            raise NotImplementedError("not available on the device with the %s mean; it evaluates the likelihood, chains, "
                                      "predict() and sample() only" % type(self.mean).__name__)
        return ev._bind(model), model

    def _has_profile_mean(self):
        return getattr(self.mean, "mtg_mean_kind", None) in _engine.PROFILE_MEANS

    def _zero_mean_engine(self, y):
        """A profile mean (sine, two sines, Gaussian) under the device entries that read the mean and know only the
        constant and the linear one: the residual ``y - mean(t)`` at the current parameters is bound with a frozen
        constant mean of zero, and the caller adds ``mean.get_value`` back on the host.  -> (engine, that model)."""
        if self._t is None:
            raise RuntimeError("you must call 'compute' first")
        y = np.zeros(len(self._t)) if y is None else np.asarray(y, dtype=np.float64)
        ev = self._ensure_evaluator(y - self.mean.get_value(self._t))
        zero = ConstantModel(0.0)
        zero.freeze_all_parameters()
        model = DeviceModel(self.kernel, zero, zero.unfrozen_mask)
        if not model.device_terms:
            raise NotImplementedError("needs device-expandable terms")
        return ev._bind(model), model

    def _mean_engine(self, y):
        """-> (engine, model, what to add to a device mean at times x)"""
        if self._has_profile_mean():
            eng, model = self._zero_mean_engine(y)
            return eng, model, self.mean.get_value
        eng, model = self._bound_engine(y)
        return eng, model, lambda x: model.y_offset or 0.0

    @staticmethod
    def _raise_for(status):
        if status == _engine.ST_NOTPD:
            raise LinAlgError("failed to factorize or solve matrix")
        if status == _engine.ST_PRIOR:
            raise ValueError("the current parameter vector has zero prior probability")

    def apply_inverse(self, y):
        """``K^-1 y`` for ``y`` of shape (N,) or (N, nrhs) (celerite.GP.apply_inverse), K the
        covariance at the current parameters: O(N J^2 + N J nrhs) on the device."""
        y = np.asarray(y, dtype=np.float64)
        if y.shape[0] != len(self._t):
            raise ValueError("dimension mismatch")
        eng, model = self._bound_engine(self._y_bound if self._y_bound is not None else np.zeros(len(self._t)), profile_ok=True)
        x, status = eng.apply_inverse(model.full[model.free_index], y)
        self._raise_for(status)
        return x

    def whiten(self, y):
        """Whitened (one-step-ahead) residuals of ``y`` at the current parameters, ``q = D^-1/2 L^-1 (y - mean)`` with
        ``K = L diag(D) L^T`` -> ``[N]``: ``q_n`` is ``y_n`` minus its prediction from the samples before it, over the
        standard deviation of that prediction.  Under the model the ``q_n`` are independent standard normals -- what a
        KS test or an autocorrelation band assumes -- and ``sample`` with the normals ``q`` gives ``y`` back
        (``Engine.whiten``, O(N J^2) on the device).  Under a profile mean the device sees ``y - mean(t)`` with a zero
        mean, as in ``predict``."""
        eng, model, _ = self._mean_engine(y)
        q, _, _, status = eng.whiten(model.full[model.free_index][None, :], stats=False)
        self._raise_for(status[0])
        return q[0]

    def sample(self, size=None, seed=None):
        """Realisations of the process at the computed times, ``y ~ N(mean, K)`` with the measurement errors and the
        jitter on the diagonal (celerite.GP.sample -> solver.dot_L): ``[N]`` for ``size=None``, else ``[size][N]``.
        The draw is ``mean + L sqrt(D) q`` on the device, O(N J^2) each (``Engine.gp_draw``).  ``seed=None``: the
        normals ``q`` are ``np.random.randn(size, N)`` of numpy's global generator, celerite's own semantics
        (``np.random.seed`` reproduces a draw); an integer ``seed``: the device draws them itself (Philox4x32-10 keyed
        by the seed and the draw's index)."""
        if self._t is None:
            raise RuntimeError("you must call 'compute' first")
        n = 1 if size is None else int(size)
        if n == 0:
            return np.empty((0, len(self._t)))          # celerite: an empty [0][N] array
        # (a profile mean: drawn around zero, the mean added on the host; only sigma^2 of the bound light curve is read)
        if self._has_profile_mean():
            eng, model, mean_at = self._mean_engine(None)
        else:
            eng, model, mean_at = self._mean_engine(self._y_bound if self._y_bound is not None else np.zeros(len(self._t)))
        theta = np.tile(model.full[model.free_index][None, :], (n, 1))
        normals = np.random.randn(n, len(self._t)) if seed is None else None
        y, status = eng.gp_draw(theta, seed=0 if seed is None else int(seed), normals=normals)
        self._raise_for(status[0])                      # every row has the same theta, hence the same status
        y += mean_at(self._t)
        return y[0] if size is None else y

    def sample_conditional(self, y, t=None, size=None, seed=None):
        """Realisations of the process given the data ``y``, at times ``t`` (celerite.GP.sample_conditional; ``t=None``:
        the computed times, where the draw is of the latent process, without measurement noise, as celerite's is):
        ``[M]`` for ``size=None``, else ``[size][M]``.  celerite draws from the dense conditional covariance of
        ``predict``; here each draw is Matheron's rule on the device, linear in N and M (``Engine.gp_cond_draw``).
        ``seed`` as in ``sample``: None takes the normals from numpy's global generator, an integer lets the device
        draw them.  Under a profile mean the device sees ``y - mean(t)`` with a zero mean and ``mean.get_value`` is
        added back, as in ``predict``."""
        eng, model, mean_at = self._mean_engine(y)
        xs = self._t if t is None else np.atleast_1d(np.asarray(t, dtype=np.float64))
        n = 1 if size is None else int(size)
        if n == 0:
            return np.empty((0, len(xs)))
        theta = np.tile(model.full[model.free_index][None, :], (n, 1))
        normals = np.random.randn(n, len(self._t) + len(xs)) if seed is None else None
        out, status = eng.gp_cond_draw(theta, xs, seed=0 if seed is None else int(seed), normals=normals)
        self._raise_for(status[0])                      # every row has the same theta, hence the same status
        out += mean_at(xs)
        return out[0] if size is None else out

    def _term_mask(self, kernel):
        """``kernel`` -- one top-level term of this GP's sum, or a sum of several -- as the bit mask of
        ``Engine.predict_terms``; the terms are matched by identity"""
        mine = self.kernel.terms
        parts = kernel.terms if isinstance(kernel, Term) else None
        mask = 0
        for part in parts or ():
            where = [k for k, term in enumerate(mine) if term is part]
            if not where:
                parts = None
                break
            mask |= 1 << where[0]
        if not parts:
            raise ValueError("kernel= must be one of the terms of this GP's kernel (gp.kernel.terms[k]) or a sum of them")
        return mask

    def predict(self, y, t=None, return_cov=True, return_var=False, kernel=None):
        """Conditional mean and (co)variance, celerite.GP.predict.

        ``kernel``: None, or a component of this GP's kernel -- ``gp.kernel.terms[k]`` or a sum of such terms, matched
        by identity; anything else (a term inside a product, a foreign object) raises ``ValueError``.  Then the mean and
        the variance are those of that component given the data, ``mean + k_c,* K^-1 r`` and
        ``k_c(0) - k_c,*^T K^-1 k_c,*`` with K the covariance of the whole kernel (celerite adds the mean here too), at
        ``t`` or at the computed times, from one device call that shares the factorisation and the replay of
        ``Engine.predict_at`` (``Engine.predict_terms``).  With ``return_cov=True`` the dense covariance of the
        component is assembled on the host over ``apply_inverse``, as the new-time covariance below is.

        At the training times (``t=None``) with ``return_var=True`` -- the reference's call,
        gpmodelling.py:366 -- mean and variance both come from the O(N J^2) factorisation on the
        device (celerite forms the dense N x N cross-covariance for the variance).  At other times the
        mean and the variance come from the same factorisation, checkpointed along the light curve
        (``Engine.predict_at``: linear in N and in the number of new times, no cross-covariance
        ``K_*`` is formed -- celerite's is dense, N_* x N).  Only the full covariance, a dense
        N_* x N_* object by definition, is assembled on the host from celerite's own expression
        ``cov = K_** - K_* K^-1 K_*^T`` over ``apply_inverse`` (one device call with 1 + N_*
        right-hand sides).  Like celerite's, the variances are those of the noise-free process (no
        jitter, no measurement errors).  Under a profile mean (sine, two sines, Gaussian) the device sees the residual
        ``y - mean(t)`` with a zero mean and ``mean.get_value`` is added back here."""
        mask = None if kernel is None else self._term_mask(kernel)
        eng, model, mean_at = self._mean_engine(y)
        if mask is not None and (return_var or not return_cov):
            xs = self._t if t is None else np.atleast_1d(np.asarray(t, dtype=np.float64))
            mu, var, status = eng.predict_terms(model.full[model.free_index][None, :], [mask | _engine.TERMS_MEAN], xs,
                                                return_var=return_var)
            self._raise_for(status[0])
            mu = mu[0, 0] + mean_at(xs)
            return (mu, var[0, 0]) if return_var else mu
        if t is None and (return_var or not return_cov):
            mu, var, status = eng.predict(model.full[model.free_index][None, :])
            self._raise_for(status[0])
            mu = mu[0] + mean_at(self._t)
            return (mu, var[0]) if return_var else mu
        if return_var or not return_cov:
            xs = np.atleast_1d(np.asarray(t, dtype=np.float64))
            mu, var, status = eng.predict_at(model.full[model.free_index][None, :], xs, return_var=return_var)
            self._raise_for(status[0])
            mu = mu[0] + mean_at(xs)
            return (mu, var[0]) if return_var else mu
        y = np.asarray(y, dtype=np.float64)
        xs = self._t if t is None else np.atleast_1d(np.asarray(t, dtype=np.float64))
        resid = y - self.mean.get_value(self._t)
        part = self.kernel if kernel is None else kernel
        kxs = part.get_value(xs[:, None] - self._t[None, :])                       # [N_*][N]
        sol, status = eng.apply_inverse(model.full[model.free_index], np.column_stack([resid, kxs.T]))
        self._raise_for(status)
        mu = self.mean.get_value(xs) + kxs @ sol[:, 0]
        return mu, part.get_value(xs[:, None] - xs[None, :]) - kxs @ sol[:, 1:]
