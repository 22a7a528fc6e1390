"""``GPModelling``: the reference's workflow facade on the MI355X engine.

Drop-in mirror of /root/reference/mind_the_gaps/gpmodelling.py:23-539 for the
log-likelihood hot path: same constructor, method names, defaults, attributes
and error behaviour; every likelihood comes from the HIP kernels (gp.GP ->
engine.Engine -> libmtg_hip.so).  What changes underneath:

* ``_log_probability`` / ``_neg_log_like`` accept one theta (P,) -> float exactly
  like the reference, or a batch (B, P) -> array, which is one GPU launch;
* ``fit`` gives L-BFGS-B the value and the forward-difference gradient from ONE
  batched launch of P + 1 evaluations (scipy's own serial finite differences,
  gpmodelling.py:192, cost P + 1 sequential likelihood calls);
* ``derive_posteriors`` runs the stretch move with the whole half-ensemble per
  launch; ``cores`` (a multiprocessing.Pool size in the reference,
  gpmodelling.py:245) is accepted and ignored.
"""
import time
import warnings
from typing import List, Tuple

import numpy as np
from scipy.optimize import minimize

from . import engine as _engine
from . import walkers as _walkers
from .gp import GP, LinAlgError
from .lightcurves import GappyLightcurve
from .modeling import ConstantModel, Model
from .models import GaussianModel, LinearModel
from .device_sampler import DeviceEnsembleSampler
from .sampler import EnsembleSampler

__all__ = ["GPModelling"]


def whiten_diagnostics(stats, acf, N):
    """The host arithmetic of ``GPModelling.residual_diagnostics``: ``Engine.whiten``'s stats [B][8] and acf [B][K] of
    series of N samples -> the dict it returns, arrays over the B rows."""
    from scipy.stats import chi2 as _chi2, kstwo
    stats, acf = np.atleast_2d(np.asarray(stats, dtype=np.float64)), np.atleast_2d(np.asarray(acf, dtype=np.float64))
    K = acf.shape[1]
    s1, s2, s3, s4 = (stats[:, k] for k in (_engine.WHITEN_SUM, _engine.WHITEN_SUM2, _engine.WHITEN_SUM3, _engine.WHITEN_SUM4))
    ks = np.maximum(stats[:, _engine.WHITEN_KS_PLUS], stats[:, _engine.WHITEN_KS_MINUS])
    # ks_1samp(method="auto") always takes the exact distribution of the two-sided statistic, and clips
    pvalue = np.clip(kstwo.sf(ks, N), 0.0, 1.0)
    # central moments (biased, scipy.stats.skew / kurtosis defaults) from the power sums
    m = s1 / N
    m2 = s2 / N - m * m
    m3 = s3 / N - 3.0 * m * s2 / N + 2.0 * m ** 3
    m4 = s4 / N - 4.0 * m * s3 / N + 6.0 * m * m * s2 / N - 3.0 * m ** 4
    lb = N * (N + 2.0) * np.sum(acf * acf / (N - np.arange(1, K + 1, dtype=np.float64))[None, :], axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):      # a constant series has no shape: NaN
        skewness, kurtosis = m3 / m2 ** 1.5, m4 / (m2 * m2) - 3.0
    return dict(ks_statistic=ks, ks_pvalue=pvalue, chi2=s2.copy(), skewness=skewness, excess_kurtosis=kurtosis,
                acf=acf, ljung_box=lb, ljung_box_pvalue=_chi2.sf(lb, K), max_abs=stats[:, _engine.WHITEN_MAXABS].copy(),
                acf_band=1.96 / np.sqrt(N))


class GPModelling:
    """The interface for Gaussian Process (GP) modelling on MI355X."""

    meanmodels = ["linear", "constant", "gaussian"]

    def __init__(self, lightcurve: GappyLightcurve, kernel, mean_model: str = None, device: int = 0,
                 quiet: bool = False, random_state=None, own_engine: bool = False, meanmodel=None):
        """GP of ``kernel`` (a ``mind_the_gaps_amd.terms.Term``) on ``lightcurve``, factorised once with
        ``yerr = dy + 1e-12`` as the reference does (gpmodelling.py:54).

        ``mean_model``: None keeps the mean frozen at the light curve's average; "constant", "linear" or
        "gaussian" name a mean that is fitted along with the kernel (the table in ``_build_mean_model``).
        New and optional: ``mean_model`` (or, by the name ``_build_mean_model`` gives it, ``meanmodel``) may also be a
        mean-model INSTANCE -- ``models.SineModel``, ``TwoSineModel``, ``GaussianModel``, ``LinearModel`` --, which is
        then fitted along with the kernel from its own starting values within its own bounds; ``device`` = GPU ordinal; ``quiet`` = a covariance that is not positive definite gives
        -inf instead of ``LinAlgError`` (the reference raises, gpmodelling.py:152); ``random_state`` = a
        ``numpy.random.RandomState`` for the walkers' starting points and the device sampler's key instead of numpy's
        global generator (the reference's and emcee's source; a private one lets two models be sampled from two threads
        with the numbers ``np.random.seed`` would have given each); ``own_engine`` = a device context of this object's
        own (``gp.release_engine()`` gives it back)."""
        self._lightcurve = lightcurve
        if meanmodel is not None and mean_model is not None:
            raise ValueError("give the mean model once, as mean_model or as meanmodel")
        meanmodel, fit_mean = self._build_mean_model(mean_model if meanmodel is None else meanmodel)
        self.gp = GP(kernel, mean=meanmodel, fit_mean=fit_mean, device=device, own_engine=own_engine)
        self._random = random_state
        self.gp.compute(self._lightcurve.times, np.asarray(self._lightcurve.dy, dtype=np.float64) + 1e-12)
        self.initial_params = self.gp.get_parameter_vector()
        self._ndim = len(self.initial_params)
        self._autocorr = []
        self._loglikelihoods = None
        self._mcmc_samples = None
        self._quiet = quiet
        self._fit_evaluations = 1   # fit() resets it: only the first evaluation of a fit may raise LinAlgError
        self._y = np.asarray(self._lightcurve.y, dtype=np.float64)

    # mean kind -> (model factory taking the light curve, fitted?).  The contract of gpmodelling.py:62-124: without a
    # name the mean is a ConstantModel frozen at the light curve's average, boxed by the data's range; a name selects a
    # fitted mean -- "constant" the same model, "linear" LinearModel(slope 0, intercept 1.5) without bounds (the
    # reference works slope estimates out and then does not use them), "gaussian" a bump centred on the middle epoch,
    # half the duration wide.  The reference hands GaussianModel three values for its four parameters, so that branch
    # raises ValueError there and here -- kept, not fixed.
    @staticmethod
    def _constant_mean(lc):
        return ConstantModel(lc.mean, bounds=[(np.min(lc.y), np.max(lc.y))])

    @staticmethod
    def _linear_mean(lc):
        return LinearModel(0, 1.5, bounds=[(-np.inf, np.inf)] * 2)

    @staticmethod
    def _gaussian_mean(lc):
        span, top, root2pi = lc.duration, np.max(lc.y), np.sqrt(2 * np.pi)
        width = span / 2
        return GaussianModel(lc.times[len(lc.times) // 2], width, (top - np.min(lc.y)) * root2pi * width,
                             bounds=[(lc.times[0], lc.times[-1]), (0, span), (top * root2pi * span, 50 * top * root2pi * span)])

    _MEAN_KINDS = {None: ("_constant_mean", False), "constant": ("_constant_mean", True),
                   "linear": ("_linear_mean", True), "gaussian": ("_gaussian_mean", True)}

    def _build_mean_model(self, meanmodel: str = None):
        """(mean model, fit_mean) for a mean kind (see the table above), or for a mean-model instance: itself, fitted."""
        if isinstance(meanmodel, Model):
            return meanmodel, True
        kind = meanmodel if meanmodel is None else meanmodel.lower()
        if kind not in self._MEAN_KINDS:
            raise ValueError("Input mean model %s not implemented! Only \n %s \n are available"
                             % (meanmodel, "\t".join(GPModelling.meanmodels)))
        factory, fitted = self._MEAN_KINDS[kind]
        return getattr(self, factory)(self._lightcurve), fitted

    # -- the hot path --------------------------------------------------------------
    def _batch(self, params, add_prior):
        theta = np.asarray(params, dtype=np.float64)
        single = theta.ndim == 1
        out, status = self.gp.log_probability_batch(np.atleast_2d(theta), self._y, add_prior=add_prior)
        if not self._quiet and np.any(status == _engine.ST_NOTPD):
            raise LinAlgError("failed to factorize or solve matrix")
        return (float(out[0]) if single else out)

    def _log_probability(self, params):
        """Logarithm of the posterior: box prior + GP log-likelihood
        (gpmodelling.py:127-152).  ``params``: (P,) -> float or (B, P) -> array."""
        return self._batch(params, add_prior=True)

    def _neg_log_like(self, params):
        """Negative log-likelihood, no prior (gpmodelling.py:155-169)."""
        r = self._batch(params, add_prior=False)
        return -r

    def _neg_log_like_and_grad(self, x, lower, upper, step=1e-8):
        """-lnL and its forward-difference gradient from one batched launch.

        Same scheme scipy applies for L-BFGS-B without a jacobian (absolute step
        ``eps`` = 1e-8, flipped or shrunk where x + h would leave the bounds)."""
        x = np.asarray(x, dtype=np.float64)
        h = np.full_like(x, step)
        room_up, room_dn = upper - x, x - lower
        out_of_box = x + h > upper
        flip = out_of_box & (np.abs(h) <= np.maximum(room_dn, room_up))
        h[flip] *= -1.0
        shrink = out_of_box & ~flip
        h[shrink & (room_up >= room_dn)] = room_up[shrink & (room_up >= room_dn)]
        h[shrink & (room_up < room_dn)] = -room_dn[shrink & (room_up < room_dn)]
        pts = np.vstack([x[None, :], x[None, :] + np.diag(h)])
        # Inside the optimiser a numerically singular corner of the box (e.g. log_S0 at its
        # upper bound) is a very bad point, not a fatal one: celerite's LinAlgError would
        # abort the reference's fit there; here the line search simply backs off.
        out, status = self.gp.log_probability_batch(pts, self._y, add_prior=False)
        vals = np.where(status == _engine.ST_OK, -out, np.inf)
        f0 = float(vals[0])
        if not np.isfinite(f0):
            if self._fit_evaluations == 0 and not self._quiet:
                # the STARTING point itself cannot be factorised: returning a plateau would make
                # L-BFGS-B "converge" there at once; the reference raises here (gpmodelling.py:192)
                raise LinAlgError("failed to factorize or solve matrix")
            self._fit_evaluations += 1
            return 1e300, np.zeros_like(x)
        self._fit_evaluations += 1
        dx = pts[1:].diagonal() - x
        with np.errstate(divide="ignore", invalid="ignore"):
            grad = np.where((dx != 0.0) & np.isfinite(vals[1:]), (vals[1:] - f0) / dx, 0.0)
        return f0, grad

    def _neg_log_like_and_grad_analytic(self, x, lower, upper):
        """-lnL and its analytic gradient from one launch of the device's tangent sweep (``Engine.loglike_grad``);
        a point that cannot be factorised is treated as in ``_neg_log_like_and_grad``."""
        x = np.asarray(x, dtype=np.float64)
        out, grad, status = self.gp.log_probability_grad_batch(x[None, :], self._y, add_prior=False)
        if status[0] != _engine.ST_OK or not np.isfinite(out[0]):
            if self._fit_evaluations == 0 and not self._quiet:
                raise LinAlgError("failed to factorize or solve matrix")
            self._fit_evaluations += 1
            return 1e300, np.zeros_like(x)
        self._fit_evaluations += 1
        return -float(out[0]), -grad[0]

    def _analytic_gradient_usable(self, x):
        """None when ``fit(gradient="analytic")`` can run on this model, else why not"""
        model = self.gp._device_model()
        if not model.device_terms:
            return "a term has no device expansion"
        if model.mean_kind is None:
            return "the mean model is evaluated on the host"
        if model.mean_kind in _engine.PROFILE_MEANS:
            return "the device's tangent sweep has no gradient by the parameters of the %s mean" % type(self.gp.mean).__name__
        try:
            self.gp.log_probability_grad_batch(np.asarray(x, dtype=np.float64)[None, :], self._y, add_prior=False)
        except _engine.EngineError as exc:
            if exc.code != _engine.E_UNSUPPORTED:
                raise
            return "the model's rank is beyond the device's tangent sweep"
        return None

    def fit(self, initial_params=None, gradient="fd"):
        """L-BFGS-B minimisation of the negative log-likelihood within the
        parameter bounds (gpmodelling.py:172-194).  Returns scipy's OptimizeResult.

        ``gradient`` (new, optional): "fd", the default, gives L-BFGS-B forward differences of step 1e-8 from one
        batched launch; "analytic" the exact gradient from the device's tangent sweep (one launch of one lane per
        free parameter): free of the differences' rounding noise, u |lnL| / 1e-8, but 50 to 740 times their kernel
        time (profiles/grad_probe.txt).  It does not by itself end the search higher: at N = 1e6 scipy's default
        ``ftol`` (a relative reduction of 2.2e-9, 8e-3 in -lnL there) stops both modes first, the analytic run 3.6
        above the other in -lnL.  A model the sweep does not cover (a host-evaluated term or mean, a rank
        it is not compiled for) warns and uses "fd"."""
        if gradient not in ("fd", "analytic"):
            raise ValueError("gradient must be 'fd' or 'analytic', not %r" % (gradient,))
        if initial_params is None:
            initial_params = self.initial_params
        fun = self._neg_log_like_and_grad
        if gradient == "analytic":
            why_not = self._analytic_gradient_usable(initial_params)
            if why_not is None:
                fun = self._neg_log_like_and_grad_analytic
            else:
                warnings.warn("fit(gradient='analytic'): %s; using finite differences" % why_not)
        bounds = self.gp.get_parameter_bounds()
        lower = np.array([-np.inf if b[0] is None else b[0] for b in bounds], dtype=np.float64)
        upper = np.array([np.inf if b[1] is None else b[1] for b in bounds], dtype=np.float64)
        self._fit_evaluations = 0
        solution = minimize(fun, initial_params, args=(lower, upper), jac=True,
                            method="L-BFGS-B", bounds=bounds)
        if not np.isfinite(solution.fun) or solution.fun >= 1e300:   # quiet mode: say so instead of "success"
            solution.success = False
            solution.message = "the covariance could not be factorised at the starting point"
            warnings.warn("fit(): " + solution.message)
        return solution

    def derive_posteriors(self, initial_chain_params=None, fit: bool = True, converge: bool = True,
                          max_steps: int = 10000, convergence_steps: int = 500, walkers: int = 12,
                          cores: int = 6, progress: bool = True, device_sampler: bool = None,
                          shard_walkers: bool = False, group=None):
        """Derive GP posteriors (gpmodelling.py:197-286): optional fit, walker
        spreading, stretch-move MCMC with an autocorrelation-time convergence check
        every ``convergence_steps`` iterations, then burn-in and thinning.

        ``device_sampler`` (new, optional): keep walkers, random numbers and the
        accept/reject step on the GPU (``mtg_ensemble_*``); the host only sees the chain
        every ``convergence_steps`` iterations.  Needs an even number of walkers and terms the
        device can expand.  Default (None): on whenever that holds -- 2-3x the iteration rate of
        the host-side sampler; like emcee's, the run is reproducible from ``np.random.seed``
        (the Philox key is drawn from numpy's global generator).  False: the host-side sampler
        with emcee's own use of numpy's global generator.

        ``shard_walkers`` (new, optional): inside a ``torch.distributed`` job (one process per
        GPU, every rank holding this light curve and calling this method with the same
        arguments) split every half-ensemble across the ranks: each GPU evaluates its rows,
        one all-gather of the log-probabilities per half-step (``group``: the process group,
        default the world), identical accept/reject everywhere -- every rank ends with the
        same chain.  With the device sampler the exchange is an ``ncclAllGather`` on the engine's
        stream (``mtg_ensemble_shard_rccl``; a host-staged exchange over ``group`` when its backend
        is not nccl); with the host-side sampler (``device_sampler=False``) it is
        ``distributed.WalkerShardedLogProb``.  Rank 0's starting ensemble and random state / seed are
        broadcast first."""
        if device_sampler is None:
            model = self.gp._device_model()
            device_sampler = walkers % 2 == 0 and bool(model.device_terms) and model.mean_kind is not None
        if initial_chain_params is None:
            if not fit:
                initial_params = self.initial_params
            else:
                solution = self.fit(self.initial_params)
                initial_params = solution.x
            initial_chain_params = self.spread_walkers(walkers, initial_params,
                                                       np.array(self.gp.get_parameter_bounds()))
        every_samples = convergence_steps
        old_tau = np.inf
        self.converged = False
        tau = None
        started = time.perf_counter()
        if device_sampler:
            sampler = self._device_sampler(walkers, shard_group=group if shard_walkers else False)
            first, done = initial_chain_params, 0

            def iterations():
                nonlocal first, done
                while done < max_steps:
                    chunk = min(every_samples - done % every_samples, max_steps - done)
                    sampler.run_mcmc(first, chunk)
                    if not self._quiet and sampler.state["n_not_pd"]:
                        raise LinAlgError("failed to factorize or solve matrix")
                    first, done = None, done + chunk
                    yield done
            steps_iter = iterations()
        else:
            log_prob_fn = self._log_probability
            if shard_walkers:
                from .distributed import WalkerShardedLogProb, lockstep
                log_prob_fn = WalkerShardedLogProb(self._log_probability, group=group)
            sampler = EnsembleSampler(walkers, self._ndim, log_prob_fn, vectorize=True)
            if shard_walkers:
                initial_chain_params = lockstep(sampler, initial_chain_params, group=group)
            steps_iter = sampler.sample(initial_chain_params, iterations=max_steps, progress=progress)
        for sample in steps_iter:
            if sampler.iteration % every_samples:
                continue
            # tol=0: always get an estimate, even an untrustworthy one
            tau = sampler.get_autocorr_time(tol=0)
            if shard_walkers and not device_sampler:   # (the device sampler broadcasts rank 0's value itself)
                from .distributed import broadcast_array
                tau = broadcast_array(tau, group)
            self.autocorr.append(np.mean(tau))
            if np.all(tau * 100 < sampler.iteration) and np.all(np.abs(old_tau - tau) / tau < 0.01) and converge:
                print("Convergence reached after %d samples!" % sampler.iteration)
                self.converged = True
                break
            old_tau = tau
        if tau is None:
            # max_steps < convergence_steps: the reference hits a NameError here
            # (SURVEY.md Appendix C.1); estimate once from the chain we have
            tau = sampler.get_autocorr_time(tol=0)
        self._tau = tau
        mean_tau = np.mean(tau)
        if not np.isfinite(mean_tau):
            # a parameter that never moved (very short chains) has an undefined autocorrelation
            # time; the reference would crash on int(nan) below
            warnings.warn("The autocorrelation time could not be estimated; keeping every sample")
            mean_tau = 0.0
        if not self.converged:
            warnings.warn(f"The chains did not converge after {sampler.iteration} iterations!")
            thin = int(mean_tau / 4)
            discard = int(mean_tau) * 5
        else:
            discard = int(mean_tau * 40)
            if discard > max_steps:
                discard = int(mean_tau * 10)
            thin = int(mean_tau / 2)
        thin = max(thin, 1)  # int(mean_tau / k) can be 0 for short chains (Appendix C.1)
        discard = min(max(discard, 0), max(sampler.iteration - thin, 0))
        self._loglikelihoods = sampler.get_log_prob(discard=discard, thin=thin, flat=True)
        self._mcmc_samples = sampler.get_chain(discard=discard, thin=thin, flat=True)
        self._sampler = sampler
        # metrics: log-probability evaluations per second of this run, convergence checks included
        self.evals_per_second = sampler.iteration * walkers / max(time.perf_counter() - started, 1e-12)

    def _device_sampler(self, walkers, shard_group=False):
        """One device-resident ensemble on this light curve (see device_sampler.py)."""
        ev = self.gp._ensure_evaluator(self._y)
        model = self.gp._device_model()
        if not model.device_terms or model.mean_kind is None:
            raise ValueError("the device sampler needs device-expandable terms and a mean model with mtg_mean_kind")
        seed = None if self._random is None else int(self._random.randint(0, 2 ** 62))   # (None: numpy's global generator)
        return DeviceEnsembleSampler(lambda: ev._bind(model), walkers, self._ndim, n_ensembles=1,
                                     shard_group=shard_group, seed=seed)

    def spread_walkers(self, walkers: int, parameters, bounds: List[Tuple[float, float]],
                       percent: float = 0.1, max_attempts: int = 20):
        """Spread the walkers with a Gaussian around ``parameters`` (gpmodelling.py:289-350).
        Draws from numpy's global generator in the reference's order (walker by walker,
        ``walkers.spread_reference_order``): after ``np.random.seed(k)`` the array returned is
        the reference's, value for value (tests/golden/spread_golden.npz, made by the
        reference's function; tests/test_spread_golden.py)."""
        bounds = np.array([(-np.inf if lower is None else lower, np.inf if upper is None else upper)
                           for lower, upper in bounds], dtype=np.float64)
        normal = np.random.normal if getattr(self, "_random", None) is None else self._random.normal
        return _walkers.spread_reference_order(normal, np.asarray(parameters, dtype=np.float64), bounds[:, 0],
                                               bounds[:, 1], walkers, percent=percent, max_attempts=max_attempts)

    def standarized_residuals(self, include_noise: bool = True):
        """Standardised residuals (gpmodelling.py:353-370) need ``GP.predict`` -- outside
        the log-likelihood hot path.  These are smoothing residuals, each sample
        against its prediction from ALL the data: correlated, and not of unit variance even under the true model; to
        test for whiteness (KS against the normal, autocorrelation) use ``whitened_residuals``, whose entries are
        independent standard normals under the model."""
        pred_mean, pred_var = self.gp.predict(self._lightcurve.y, return_var=True, return_cov=False)
        if include_noise:
            pred_var += self.gp.kernel.jitter
        return (self._lightcurve.y - pred_mean) / np.sqrt(pred_var)

    def _whiten_rows(self, parameters, residuals, lags, stats):
        """``Engine.whiten`` of the light curve at ``parameters`` (as in ``predict_at``) -> (q, acf, stats, one vector?)"""
        if parameters is None:
            parameters = self.max_parameters if self._mcmc_samples is not None else self.gp.get_parameter_vector()
        parameters = np.asarray(parameters, dtype=np.float64)
        theta = np.atleast_2d(parameters)
        if self.gp._has_profile_mean():
            # one vector at a time, as predict_at: the residual y - mean(t) at that vector bound with a zero mean
            saved = self.gp.get_parameter_vector()
            try:
                rows = []
                for b in range(len(theta)):
                    self.gp.set_parameter_vector(theta[b])
                    eng, model, _ = self.gp._mean_engine(self._lightcurve.y)
                    out = eng.whiten(model.full[model.free_index][None, :], residuals=residuals, lags=lags, stats=stats)
                    self.gp._raise_for(out[3][0])
                    rows.append(out[:3])
            finally:
                self.gp.set_parameter_vector(saved)
            q, acf, st = (None if rows[0][k] is None else np.vstack([r[k] for r in rows]) for k in range(3))
        else:
            eng, model = self.gp._bound_engine(self._lightcurve.y)
            q, acf, st, status = eng.whiten(theta, residuals=residuals, lags=lags, stats=stats)
            for s in status:
                self.gp._raise_for(s)
        return q, acf, st, parameters.ndim == 1

    def whitened_residuals(self, parameters=None):
        """Whitened (one-step-ahead) residuals of the light curve, ``q_n = (y_n - E[y_n | y_1 .. y_n-1]) /
        sqrt(Var[y_n | y_1 .. y_n-1])`` (Kelly et al. 2014; ``GP.whiten``): independent standard normals under the model,
        so that ``ks_1samp(q, norm.cdf)`` and ``plt.acorr(q)`` test what they claim to.  ``parameters`` as in
        ``predict_at``: None -- the maximum-posterior sample if posteriors were derived, else the GP's current vector
        -- or one vector [P], or [B][P] posterior samples, evaluated in one launch.  Returns [N] or [B][N]."""
        q, _, _, one = self._whiten_rows(parameters, True, 0, False)
        return q[0] if one else q

    def residual_diagnostics(self, parameters=None, lags=None):
        """Goodness of fit of the whitened residuals at ``parameters`` (as in ``whitened_residuals``), computed on the
        device next to the light curve -- only [B] and [B][lags] numbers come back -> a dict of arrays over the B rows
        (scalars and [lags] for one vector): ``ks_statistic`` and ``ks_pvalue`` (scipy's ``ks_1samp(q, norm.cdf)``),
        ``chi2`` = sum q^2, ``skewness``, ``excess_kurtosis``, ``acf`` at lags 1 .. ``lags`` (``plt.acorr``'s
        definition; None: N // 4, the tutorial's), ``ljung_box`` = N (N + 2) sum_k acf_k^2 / (N - k) with its chi^2
        p-value ``ljung_box_pvalue``, ``max_abs``, and the 95 per cent band of a white series ``acf_band`` =
        1.96 / sqrt(N).  The KS p-value is the textbook one: it is biased towards large values once parameters were
        fitted to the same data, so compare it over posterior samples or simulated light curves, not to 0.05."""
        N = len(self._lightcurve.times)
        K = N // 4 if lags is None else int(lags)
        if K < 1:
            raise ValueError("lags must be at least 1")
        _, acf, st, one = self._whiten_rows(parameters, False, K, True)
        out = whiten_diagnostics(st, acf, N)
        return {k: (v[0] if one and np.ndim(v) > 0 else v) for k, v in out.items()}

    def predict_at(self, times, parameters=None, include_noise: bool = False):
        """Model curve and its variance at ``times`` [M] (new; celerite users loop ``gp.predict(y, t, return_var=True)``
        over posterior samples): conditional mean and variance of the process given the light curve, from the
        factorisation in time linear in N and M (``Engine.predict_at``).  ``parameters``: None -- the
        maximum-posterior sample if posteriors were derived, else the GP's current vector -- or one vector [P], or
        [B][P] posterior samples, evaluated in one launch.  Returns ``(mu, var)`` of shape [M] or [B][M]; the variance
        is that of the noise-free process unless ``include_noise`` adds each vector's ``kernel.jitter``, as
        ``standarized_residuals`` does."""
        if parameters is None:
            parameters = self.max_parameters if self._mcmc_samples is not None else self.gp.get_parameter_vector()
        parameters = np.asarray(parameters, dtype=np.float64)
        theta = np.atleast_2d(parameters)
        if self.gp._has_profile_mean():
            # the device's entry knows the constant and the linear mean: one vector at a time, the residual
            # y - mean(t) at that vector bound with a zero mean and the mean added back (GP.predict)
            saved = self.gp.get_parameter_vector()
            try:
                rows = []
                for b in range(len(theta)):
                    self.gp.set_parameter_vector(theta[b])
                    rows.append(self.gp.predict(self._lightcurve.y, t=times, return_var=True))
            finally:
                self.gp.set_parameter_vector(saved)
            mu, var = np.array([r[0] for r in rows]), np.array([r[1] for r in rows])
        else:
            eng, model = self.gp._bound_engine(self._lightcurve.y)
            mu, var, status = eng.predict_at(theta, times)
            for st in status:
                self.gp._raise_for(st)
            mu += model.y_offset or 0.0
        if include_noise:
            saved = self.gp.get_parameter_vector()
            try:
                for b in range(len(theta)):
                    self.gp.set_parameter_vector(theta[b])
                    var[b] += self.gp.kernel.jitter
            finally:
                self.gp.set_parameter_vector(saved)
        return (mu[0], var[0]) if parameters.ndim == 1 else (mu, var)

    def predict_components(self, t=None, parameters=None):
        """The fitted curve taken apart: ``{term name: (mu, var)}`` with one entry per term of the kernel, the
        conditional mean and variance of that term alone given the light curve (``GP.predict(kernel=term)``; the mean
        model is added to every ``mu``), at times ``t`` (None: the observed epochs).  The names are the parameter
        prefixes of the sum, ``terms[k]``, or ``kernel`` for a kernel of one term.  ``parameters``: None -- the
        maximum-posterior sample if posteriors were derived, else the GP's current vector -- or one vector [P].  All
        terms come from one device call sharing one factorisation (``Engine.predict_terms``), except under a profile
        mean, where ``GP.predict`` is called per term."""
        if parameters is None:
            parameters = self.max_parameters if self._mcmc_samples is not None else self.gp.get_parameter_vector()
        times = self._lightcurve.times if t is None else np.atleast_1d(np.asarray(t, dtype=np.float64))
        parts = self.gp.kernel.terms
        names = ["terms[%d]" % k for k in range(len(parts))] if len(parts) > 1 else ["kernel"]
        saved = self.gp.get_parameter_vector()
        try:
            self.gp.set_parameter_vector(np.asarray(parameters, dtype=np.float64))
            if self.gp._has_profile_mean():
                return {name: self.gp.predict(self._lightcurve.y, t=times, return_var=True, return_cov=False, kernel=part)
                        for name, part in zip(names, parts)}
            eng, model = self.gp._bound_engine(self._lightcurve.y)
            masks = [(1 << k) | _engine.TERMS_MEAN for k in range(len(parts))]
            mu, var, status = eng.predict_terms(model.full[model.free_index][None, :], masks, times)
            self.gp._raise_for(status[0])
            return {name: (mu[0, k] + (model.y_offset or 0.0), var[0, k]) for k, name in enumerate(names)}
        finally:
            self.gp.set_parameter_vector(saved)

    def sample_conditional(self, times=None, nsims: int = 1, parameters=None, seed=None):
        """``nsims`` light curves drawn from the process given the data, at ``times`` [M] (None: the observed epochs) ->
        [nsims][M]: what fills a gap with realisations consistent with both the data and the fitted kernel
        (``GP.sample_conditional``, linear in N and M).  ``parameters``: None -- ``nsims`` vectors drawn from the stored
        posterior samples as ``generate_from_posteriors`` draws them, one light curve each -- or one vector [P], used
        for every draw.  ``seed``: None takes the choice of samples and the device's seed from numpy's global
        generator; an integer makes the call reproducible by itself."""
        rng = np.random if seed is None else np.random.RandomState(int(seed))
        if parameters is None:
            if self._mcmc_samples is None:
                raise RuntimeError(self._NOT_DERIVED)
            theta = self._mcmc_samples[rng.randint(len(self._mcmc_samples), size=nsims)]
        else:
            theta = np.tile(np.asarray(parameters, dtype=np.float64)[None, :], (nsims, 1))
        dev_seed = int(rng.randint(0, 2 ** 31 - 1))
        times = self._lightcurve.times if times is None else np.atleast_1d(np.asarray(times, dtype=np.float64))
        if self.gp._has_profile_mean():
            # one vector at a time, as predict_at: the residual y - mean(t) at that vector bound with a zero mean
            saved = self.gp.get_parameter_vector()
            try:
                rows = []
                for b in range(nsims):
                    self.gp.set_parameter_vector(theta[b])
                    rows.append(self.gp.sample_conditional(self._lightcurve.y, t=times, seed=dev_seed + b))
            finally:
                self.gp.set_parameter_vector(saved)
            return np.array(rows)
        eng, model = self.gp._bound_engine(self._lightcurve.y)
        y, status = eng.gp_cond_draw(theta, times, seed=dev_seed)
        for st in status:
            self.gp._raise_for(st)
        return y + (model.y_offset or 0.0)

    def get_rstat(self, burnin: int = None):
        """Gelman-Rubin-like statistic as the reference computes it
        (gpmodelling.py:373-403): within-chain over total variance."""
        if getattr(self, "_sampler", None) is None:
            raise ValueError("Posteriors have not been derived. Please run derive_posteriors prior to "
                             "populate the attributes.")
        if burnin is None:
            burnin = int(np.mean(self.tau)) * 10
        samples = self._sampler.get_chain(discard=burnin)
        whithin_chain_variances = np.var(samples, axis=0)
        samples = self._sampler.get_chain(flat=True, discard=burnin)
        between_chain_variances = np.var(samples, axis=0)
        return whithin_chain_variances / between_chain_variances[np.newaxis, :]

    # -- result accessors (gpmodelling.py:405-475) -----------------------------------
    _NOT_DERIVED = ("Posteriors have not been derived. Please run derive_posteriors prior to "
                    "populate the attributes.")

    @property
    def loglikelihoods(self):
        if self._loglikelihoods is None:
            raise AttributeError(self._NOT_DERIVED)
        return self._loglikelihoods

    @property
    def autocorr(self):
        return self._autocorr

    @property
    def sampler(self):
        if self._loglikelihoods is None:
            raise AttributeError(self._NOT_DERIVED)
        return self._sampler

    @property
    def mcmc_samples(self):
        if self._mcmc_samples is None:
            raise AttributeError(self._NOT_DERIVED)
        return self._mcmc_samples

    @property
    def max_loglikelihood(self):
        if self._loglikelihoods is None:
            raise AttributeError(self._NOT_DERIVED)
        return np.max(self._loglikelihoods)

    @property
    def best_loglikelihood(self):
        """Largest log-posterior over EVERYTHING the chains stored, burn-in included (new; the
        reference has only ``max_loglikelihood``, the maximum over the burned-in, thinned chain).  It
        is the estimator the lock-step refits of ``ppp.derive_posteriors_batch`` keep when they do not
        store chains, so a likelihood-ratio test compares like with like (``ppp.protassov_test``)."""
        if self._loglikelihoods is None:
            raise AttributeError(self._NOT_DERIVED)
        best = float(np.max(self._sampler.get_log_prob(flat=True)))
        state = getattr(self._sampler, "state", None)
        if isinstance(state, dict) and "best_log_prob" in state:   # the device sampler also saw the starting ensemble
            best = max(best, float(np.max(state["best_log_prob"])))
        return best

    @property
    def max_parameters(self):
        if self._mcmc_samples is None:
            raise AttributeError(self._NOT_DERIVED)
        return self._mcmc_samples[np.argmax(self._loglikelihoods)]

    @property
    def median_parameters(self):
        if self._mcmc_samples is None:
            raise AttributeError(self._NOT_DERIVED)
        return np.median(self._mcmc_samples, axis=0)

    @property
    def parameter_names(self):
        return self.gp.get_parameter_names()

    @property
    def k(self) -> int:
        return self._ndim

    @property
    def tau(self):
        if self._mcmc_samples is None:
            raise AttributeError(self._NOT_DERIVED)
        return self._tau

    def generate_from_posteriors(self, nsims: int = 10, cpus: int = 8, pdf: str = "Gaussian",
                                 extension_factor: int = 2, sigma_noise=None, method: str = "tk95"):
        """Light curves drawn from the MCMC posteriors (gpmodelling.py:478-539): ``nsims``
        random posterior samples, one Timmer & Koenig realisation each on this light
        curve's sampling, noise and error bars from its exposures (or ``sigma_noise``).
        All simulations run in one device call (``cpus`` is accepted and ignored).

        ``method="gp"``: each posterior sample (kernel and mean parameters) gives one exact draw of the
        GP itself at the observed epochs, ``y ~ N(mean, K + diag(dy^2))`` (``Engine.gp_draw``, no grid and
        no window averages), returned with the observed error bars; Gaussian flux PDF only."""
        if method not in ("tk95", "gp"):
            raise ValueError("method must be 'tk95' or 'gp', not %r" % (method,))
        if method == "gp" and pdf != "Gaussian":
            raise ValueError("method='gp' draws from the Gaussian process itself: pdf must be 'Gaussian', not %r" % (pdf,))
        if self._mcmc_samples is None:
            raise RuntimeError("Posteriors have not been derived. Please run derive_posteriors prior to "
                               "calling this method.")
        if nsims >= len(self._mcmc_samples):
            warnings.warn("The number of simulation requested (%d) is higher than the number of posterior "
                          "samples (%d), so many samples will be drawn more than once"
                          % (nsims, len(self._mcmc_samples)))
        from .simulator import Simulator
        param_samples = self._mcmc_samples[np.random.randint(len(self._mcmc_samples), size=nsims)]
        lc = self._lightcurve
        if method == "gp":
            eng, model = self.gp._bound_engine(lc.y)
            y, status = eng.gp_draw(param_samples, seed=np.random.randint(0, 2 ** 31 - 1))
            for st in status:
                self.gp._raise_for(st)
            y += model.y_offset or 0.0
            return [GappyLightcurve(lc.times, y[i], lc.dy) for i in range(nsims)]
        simulator = Simulator(self.gp.kernel, lc.times, lc.exposures, lc.mean, pdf, lc.bkg_rate, lc.bkg_rate_err,
                              sigma_noise=sigma_noise, extension_factor=extension_factor,
                              random_state=np.random.randint(0, 2 ** 31 - 1), device=self.gp.device)
        nk = self.gp.kernel.vector_size               # the PSD depends on the kernel parameters only
        out = simulator.simulate(param_samples[:, :nk])
        return [GappyLightcurve(lc.times, out["rates"][i], out["dy"][i]) for i in range(nsims)]
