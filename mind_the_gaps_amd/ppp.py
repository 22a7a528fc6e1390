"""Lock-step posteriors for MANY light curves: the Protassov loop as a batch axis.

The reference refits every simulated light curve one after the other
(/root/reference/docs/notebooks/tutorial_ppp.ipynb:326-343):

    for lc in lcs:
        gpm = GPModelling(lc, kernel)
        gpm.derive_posteriors(fit=True, max_steps=500, walkers=2 * cpus, cores=cpus)
        likelihoods.append(gpm.max_loglikelihood)

Every light curve is an independent problem of identical shape, so here all L
ensembles advance together: one stretch-move half-step of every ensemble is ONE
launch of L * W/2 evaluations (`LogProbEvaluator.evaluate` over the L resident
light curves).  The move, the acceptance rule, the autocorrelation estimate and
the burn-in / thinning arithmetic are those of `sampler.EnsembleSampler` and
`GPModelling.derive_posteriors` (gpmodelling.py:197-286), applied per light curve;
random numbers come from one vectorised generator instead of L private streams.
"""
import time
import warnings

import numpy as np

from . import engine as _engine
from . import walkers as _walkers
from ._ppp_plan import BLOCK_SEED_STRIDE, REPRODUCIBLE_TP_ROWS, _plan_protassov, _reproducible_is_free, _split_by_model  # noqa: F401
from .gp import DeviceModel, LinAlgError, LogProbEvaluator
from .modeling import ConstantModel
from .sampler import integrated_time

__all__ = ["EnsembleBatchSampler", "BatchPosteriors", "derive_posteriors_batch", "batched_minimize",
           "protassov_test", "periodogram_peak_test", "periodogram_significance", "derive_posteriors_sharded"]


class PhaseTimer:
    """Wall time by named phase: ``mark(name)`` closes the phase that began at the previous mark (or at construction)."""

    def __init__(self):
        self.seconds = {}
        self._last = time.perf_counter()

    def mark(self, name, seconds=None):
        """``seconds``: book that much instead of the time since the last mark (which it does not move)."""
        if seconds is None:
            now = time.perf_counter()
            seconds, self._last = now - self._last, now
        self.seconds[name] = seconds


class EnsembleBatchSampler:
    """L independent affine-invariant ensembles (stretch move, a = 2) in lock-step.

    ``log_prob_fn(coords[B, ndim], lc_index[B]) -> lnP[B]``.  ``store_chain=False`` keeps
    only the running best sample of every light curve (what the LRT needs) instead of
    the [steps, L, W, ndim] chain.
    """

    def __init__(self, nlc, nwalkers, ndim, log_prob_fn, seed=None, a=2.0, store_chain=True):
        if nwalkers < 2 * ndim:
            raise RuntimeError("It is unadvisable to use a red-blue move with fewer walkers than "
                               "twice the number of dimensions.")
        if nwalkers % 2:
            raise ValueError("the lock-step sampler needs an even number of walkers")
        self.L, self.W, self.ndim = int(nlc), int(nwalkers), int(ndim)
        self.log_prob_fn = log_prob_fn
        self.a = float(a)
        self.rng = np.random.default_rng(seed)
        self.store_chain = store_chain
        self.iteration = 0
        self._chain = []
        self._lnp = []
        self.coords = None
        self.lnp = None
        self.best_lnp = np.full(self.L, -np.inf)
        self.best_coords = np.full((self.L, self.ndim), np.nan)
        self.n_accepted = np.zeros((self.L, self.W))

    def _evaluate(self, coords):
        """coords [L, K, ndim] -> lnP [L, K] in one call."""
        L, K, _ = coords.shape
        flat = coords.reshape(L * K, self.ndim)
        if not np.all(np.isfinite(flat)):
            raise ValueError("At least one parameter value was infinite or NaN")
        lc = np.repeat(np.arange(L, dtype=np.int32), K)
        lnp = np.asarray(self.log_prob_fn(flat, lc), dtype=np.float64)
        if np.any(np.isnan(lnp)):
            raise ValueError("Probability function returned NaN")
        return lnp.reshape(L, K)

    def _track_best(self):
        j = np.argmax(self.lnp, axis=1)
        cand = self.lnp[np.arange(self.L), j]
        better = cand > self.best_lnp
        self.best_lnp[better] = cand[better]
        self.best_coords[better] = self.coords[np.arange(self.L), j][better]

    def run(self, initial_state, steps, progress=False):
        """Advance every ensemble ``steps`` iterations from ``initial_state`` [L, W, ndim]
        (or continue when it is None)."""
        L, W, ndim, half = self.L, self.W, self.ndim, self.W // 2
        if initial_state is not None:
            p0 = np.array(initial_state, dtype=np.float64)
            if p0.shape != (L, W, ndim):
                raise ValueError("incompatible input dimensions {0}".format(p0.shape))
            self.coords = p0
            self.lnp = self._evaluate(p0)
            self._track_best()
        rows = np.arange(L)[:, None]
        for _ in range(int(steps)):
            # red/blue split, independently shuffled for every light curve
            order = np.argsort(self.rng.random((L, W)), axis=1)
            red, blue = order[:, :half], order[:, half:]
            for first, other in ((red, blue), (blue, red)):
                s = self.coords[rows, first]                                   # [L, half, ndim]
                zz = ((self.a - 1.0) * self.rng.random((L, half)) + 1.0) ** 2 / self.a
                partner = other[rows, self.rng.integers(half, size=(L, half))]
                c = self.coords[rows, partner]
                q = c - (c - s) * zz[:, :, None]
                new_lnp = self._evaluate(q)                                    # <- ONE launch
                lnpdiff = (ndim - 1.0) * np.log(zz) + new_lnp - self.lnp[rows, first]
                accept = lnpdiff > np.log(self.rng.random((L, half)))
                li, wi = np.nonzero(accept)
                tgt = first[li, wi]
                self.coords[li, tgt] = q[li, wi]
                self.lnp[li, tgt] = new_lnp[li, wi]
                self.n_accepted[li, tgt] += 1
            self.iteration += 1
            self._track_best()
            if self.store_chain:
                self._chain.append(self.coords.copy())
                self._lnp.append(self.lnp.copy())
        return self.coords, self.lnp

    # -- per-light-curve views -------------------------------------------------------
    def get_chain(self, lc=None):
        chain = np.asarray(self._chain)                     # [steps, L, W, ndim]
        return chain if lc is None else chain[:, lc]

    def get_log_prob(self, lc=None):
        lnp = np.asarray(self._lnp)
        return lnp if lc is None else lnp[:, lc]

    def get_autocorr_time(self, tol=0):
        """tau[L, ndim]: integrated autocorrelation time per light curve and parameter."""
        chain = self.get_chain()
        return np.array([integrated_time(chain[:, l], tol=tol, quiet=True) for l in range(self.L)])

    @property
    def acceptance_fraction(self):
        return self.n_accepted / float(max(self.iteration, 1))


def batched_minimize(fun, x0, lower, upper, max_iter=60, history=8, fd_step=1e-6, gtol=1e-5, ftol=1e-10, value_and_grad=None):
    """Projected L-BFGS for L independent box-constrained problems in lock-step.

    ``fun(X[M, P], lc[M]) -> f[M]``; ``x0`` [L, P]; ``lower``/``upper`` [P].  Each
    iteration costs one launch for the forward-difference gradients (L * (P + 1)
    evaluations) plus one per backtracking round (L evaluations).  It plays the role of
    ``scipy.optimize.minimize(method="L-BFGS-B")`` in GPModelling.fit (gpmodelling.py:192)
    for the lock-step driver: a good starting point for the walkers, not a bit-identical
    optimiser path.  Returns (x[L, P], f[L], iterations).

    ``value_and_grad``: an optional callable ``(x[L, P]) -> (f[L], g[L, P])``, row l on problem l, used in place of
    the forward differences (an analytic gradient: one launch of L rows); ``fun`` then serves the line search alone.
    """
    x = np.clip(np.array(x0, dtype=np.float64), lower, upper)
    L, P = x.shape
    lcs = np.arange(L, dtype=np.int32)

    def forward_differences(x):
        h = np.where(x + fd_step > upper, -fd_step, fd_step)            # step inward at the upper bound
        pts = np.repeat(x[:, None, :], P + 1, axis=1)                   # [L, P+1, P]
        pts[:, 1:, :] += np.eye(P)[None] * h[:, None, :]
        vals = fun(pts.reshape(-1, P), np.repeat(lcs, P + 1)).reshape(L, P + 1)
        return vals[:, 0], (vals[:, 1:] - vals[:, :1]) / h

    if value_and_grad is None:
        value_and_grad = forward_differences
    f, g = value_and_grad(x)
    S, Y = [], []
    active = np.ones(L, dtype=bool)
    it = 0
    for it in range(1, max_iter + 1):
        # projected gradient: components pushing out of the box are dropped
        blocked = ((x <= lower) & (g > 0)) | ((x >= upper) & (g < 0))
        pg = np.where(blocked, 0.0, g)
        active &= np.max(np.abs(pg), axis=1) > gtol
        if not active.any():
            break
        # two-loop recursion, vectorised over the L problems
        q = pg.copy()
        alphas = []
        for s, yv in zip(reversed(S), reversed(Y)):
            rho = 1.0 / np.maximum(np.einsum("lp,lp->l", yv, s), 1e-300)
            a = rho * np.einsum("lp,lp->l", s, q)
            q -= a[:, None] * yv
            alphas.append((a, rho))
        if S:
            sy = np.einsum("lp,lp->l", S[-1], Y[-1])
            yy = np.maximum(np.einsum("lp,lp->l", Y[-1], Y[-1]), 1e-300)
            q *= np.where(sy > 0, sy / yy, 1.0)[:, None]
        for (a, rho), s, yv in zip(reversed(alphas), S, Y):
            b = rho * np.einsum("lp,lp->l", yv, q)
            q += (a - b)[:, None] * s
        d = -np.where(blocked, 0.0, q)
        bad_dir = np.einsum("lp,lp->l", d, pg) >= 0                      # not a descent direction
        d[bad_dir] = -pg[bad_dir]
        # backtracking (Armijo) on the projected path: steps 1, 1/2, 1/4, ... (twenty of them), every problem takes
        # the first that passes.  The steps are tried in THREE launches, not twenty -- 1; then 1/2, 1/4, 1/8 for whoever
        # failed; then all the rest for the stubborn few -- because a round is a launch of a handful of rows (a
        # latency, ~0.2 ms) and the stragglers of 250 light curves kept 13 rounds per iteration going: 715 of the 775
        # launches of a fit.  Same trial points, same test, same choice as one step per round.
        x_new, f_new = x.copy(), f.copy()
        todo = active.copy()
        for ks in ((0,), (1, 2, 3), tuple(range(4, 20))):
            if not todo.any():
                break
            idx = np.flatnonzero(todo)
            steps = 0.5 ** np.asarray(ks, dtype=np.float64)
            trial = np.clip(x[idx, None, :] + steps[None, :, None] * d[idx, None, :], lower, upper)      # [rows, steps, P]
            ft = fun(trial.reshape(-1, P), np.repeat(lcs[idx], len(ks))).reshape(len(idx), len(ks))
            ok = np.isfinite(ft) & (ft <= f[idx, None] + 1e-4 * np.einsum("lp,lkp->lk", pg[idx], trial - x[idx, None, :]))
            passed = ok.any(axis=1)
            first = np.argmax(ok, axis=1)                                 # the largest step that passes
            rows = np.flatnonzero(passed)
            x_new[idx[rows]] = trial[rows, first[rows]]
            f_new[idx[rows]] = ft[rows, first[rows]]
            todo[idx[rows]] = False
        active &= ~todo                                                   # line search failed: stop there
        f_old = f
        g_old = g
        f_try, g_try = value_and_grad(x_new)
        # The line search and the gradient batch differ in size and may run on different solver families (time-parallel
        # scan / serial sweep), which can disagree on positive-definiteness at the very edge: a point the line search
        # accepted and the gradient batch rejects is not taken.
        lost = ~np.isfinite(f_try) | ~np.all(np.isfinite(g_try), axis=1)
        if lost.any():
            x_new[lost], f_try[lost], g_try[lost] = x[lost], f[lost], g[lost]
        moved = np.any(x_new != x, axis=1)
        s_vec, y_vec = x_new - x, g_try - g_old
        good = np.einsum("lp,lp->l", s_vec, y_vec) > 1e-12
        S.append(np.where(good[:, None], s_vec, 0.0))
        Y.append(np.where(good[:, None], y_vec, 0.0))
        if len(S) > history:
            S.pop(0), Y.pop(0)
        x, f, g = x_new, f_try, g_try
        active &= moved & (np.abs(f_old - f) > ftol * np.maximum(np.abs(f), 1.0))
    return x, f, it


class BatchPosteriors:
    """Per-light-curve results of :func:`derive_posteriors_batch` (the accessors of
    GPModelling, gpmodelling.py:405-475, with a leading light-curve axis)."""

    def __init__(self, sampler, tau, discard, thin, fit_params, fit_loglike, parameter_names):
        self.sampler = sampler
        self.tau = tau                              # [L, ndim]
        self.discard, self.thin = discard, thin     # [L]
        self.fit_parameters = fit_params            # [L, ndim] or None
        self.fit_loglikelihood = fit_loglike        # [L] or None
        self.parameter_names = parameter_names
        L = sampler.L
        if sampler.store_chain:
            lnp = sampler.get_log_prob()            # [steps, L, W]
            chain = sampler.get_chain()
            self.max_loglikelihood = np.empty(L)
            self.max_parameters = np.empty((L, sampler.ndim))
            self.median_parameters = np.empty((L, sampler.ndim))
            for l in range(L):
                sl = slice(discard[l] + thin[l] - 1, None, thin[l])
                lp = lnp[sl, l].reshape(-1)
                ch = chain[sl, l].reshape(-1, sampler.ndim)
                k = int(np.argmax(lp))
                self.max_loglikelihood[l] = lp[k]
                self.max_parameters[l] = ch[k]
                self.median_parameters[l] = np.median(ch, axis=0)
        else:
            self.max_loglikelihood = sampler.best_lnp.copy()
            self.max_parameters = sampler.best_coords.copy()
            self.median_parameters = None


def _spread(rng, centers, lower, upper, walkers, percent=0.1, max_attempts=20):
    """spread_walkers (gpmodelling.py:289-350) for every light curve at once."""
    return _walkers.spread(rng.normal, centers, lower, upper, walkers, percent=percent, max_attempts=max_attempts)


class _DeviceBatch:
    """Adapter giving DeviceEnsembleSampler the read surface BatchPosteriors uses."""

    def __init__(self, dev):
        self.dev = dev
        self.L, self.W, self.ndim = dev.E, dev.nwalkers, dev.ndim
        self.store_chain = dev.store_chain
        self.iteration = dev.iteration
        self.best_lnp = dev.state["best_log_prob"]
        self.best_coords = dev.state["best_coords"]
        self.n_accepted = dev.state["naccept"]

    def get_chain(self, lc=None):
        return self.dev._chain if lc is None else self.dev._chain[:, lc]

    def get_log_prob(self, lc=None):
        return self.dev._log_prob if lc is None else self.dev._log_prob[:, lc]

    def get_autocorr_time(self, tol=0):
        from .device_sampler import _autocorr_time_where_it_is_cheapest
        return _autocorr_time_where_it_is_cheapest(self.dev._bind(), self.dev._chain, dict(tol=tol, quiet=True))

    @property
    def acceptance_fraction(self):
        return self.n_accepted / float(max(self.iteration, 1))


def derive_posteriors_batch(times, Y, DY, kernel, walkers=12, max_steps=500, fit=True, seed=None,
                            device=0, store_chain=True, initial_params=None, quiet=False,
                            evaluate=None, device_sampler=True, own_engine=False, index_base=None, before_sampling=None,
                            total_lightcurves=None, fit_gradient="fd"):
    """GPModelling(lc, kernel).derive_posteriors(...) for L light curves at once.

    times [N] (shared sampling, gpmodelling.py:538); Y, DY [L, N]; ``kernel`` a
    mind_the_gaps_amd Term (its current parameter vector is the common starting point,
    as in the tutorial loop).  The mean of every light curve is frozen at its own average
    (the reference default, gpmodelling.py:83-87).  ``evaluate`` overrides the engine call
    ``(theta[B, P], lc[B], add_prior) -> (lnP, status)`` (used by the multi-GPU driver);
    ``device_sampler`` keeps the L ensembles on the GPU between iterations
    (``mtg_ensemble_*``) instead of proposing and accepting on the host.  ``own_engine``: a device context for this
    call alone (closed before it returns), so that several calls can run side by side from different host threads.

    ``before_sampling``: called once, between the starting fit and the chains (two calls that run side by side meet there,
    so that their chains -- the long, regular part -- overlap from the first iteration to the last).

    ``index_base`` (an integer; needs ``seed`` and the device sampler): these are light curves [index_base,
    index_base + L) of a larger set that is being fitted in blocks, and every one of them must get the result it
    would get in ONE call for the whole set, bit for bit -- whatever the blocks.  Three things then stop depending on
    L: the walkers' starting points (one generator per light curve, keyed by seed and global index), the sampler's
    random numbers (Philox counters by global ensemble index, ``mtg_set_stream_base``) and the kernels (the number
    of rows in a batch otherwise picks between kernels whose sums differ in the last bits: the starting fit runs on
    the one-wave time-parallel kernel whatever the batch; the chains on the one-lane sweep and its pipelined form,
    which agree bit for bit -- or, when the WHOLE set is small, on that one-wave kernel as well;
    ``mtg_set_time_parallel`` 3 and 0).  ``total_lightcurves``: the size of the whole set, which is what that choice
    may depend on (not L, the block's): up to ``REPRODUCIBLE_TP_ROWS`` rows per half-step of the whole set every
    block, whatever the split, is inside the range where the time-parallel kernel is the fast one (0.35-3.6 ms against
    2.4-3.4 ms for the sweep at N = 1e4); unknown or larger, the sweep.  Models of rank above 6 keep the sweep in
    either mode (their time-parallel path sizes its chunks by the batch).

    ``fit_gradient``: "fd" (default), the starting fit's forward differences; "analytic", the exact gradient of every
    light curve's -lnL from one launch of the evaluator's engine (``Engine.loglike_grad``; needs this call's own
    evaluator, ``evaluate=None``).  A model of a rank the tangent sweep is not compiled for warns and uses "fd".
    """
    if fit_gradient not in ("fd", "analytic"):
        raise ValueError("fit_gradient must be 'fd' or 'analytic', not %r" % (fit_gradient,))
    if fit_gradient == "analytic" and evaluate is not None:
        raise ValueError("fit_gradient='analytic' runs on this call's own evaluator: evaluate must be None")
    Y = np.atleast_2d(np.asarray(Y, dtype=np.float64))
    DY = np.atleast_2d(np.asarray(DY, dtype=np.float64))
    L = Y.shape[0]
    model = DeviceModel(kernel, ConstantModel(0.0), np.zeros(1, dtype=bool))
    if not model.device_terms:
        raise ValueError("the lock-step driver needs device-expandable terms")
    model.y_offset = None                         # offsets are per light curve, owned by the evaluator
    timer = PhaseTimer()
    ev = None
    if evaluate is None:
        ev = LogProbEvaluator(times, Y, DY + 1e-12, device=device, y_offset=Y.mean(axis=1), own_engine=own_engine)
        timer.mark("upload")

        def evaluate(theta, lc, add_prior):
            return ev.evaluate(model, theta, lc, add_prior=add_prior)

    def checked(theta, lc, add_prior):
        out, status = evaluate(theta, lc, add_prior)
        if not quiet and np.any(status == _engine.ST_NOTPD):
            raise LinAlgError("failed to factorize or solve matrix")
        return out

    def analytic(x):            # -lnL and its gradient, row l on light curve l
        out, grad, status = ev._bind(model).loglike_grad(x, np.arange(len(x), dtype=np.int32), add_prior=False)
        if not quiet and np.any(status == _engine.ST_NOTPD):
            raise LinAlgError("failed to factorize or solve matrix")
        return -out, -grad

    P = len(model.free_index)
    lower, upper = model.bounds[model.free_index, 0], model.bounds[model.free_index, 1]
    start = model.full[model.free_index] if initial_params is None else np.asarray(initial_params, float)
    centers = np.broadcast_to(start, (L, P)).copy()
    fit_x = fit_f = None
    block_free = index_base is not None
    if block_free and (seed is None or ev is None or not device_sampler):
        raise ValueError("index_base needs a seed and the device-resident sampler on this call's own evaluator")

    def kernels(mode):          # which kernel family the evaluator's engine may pick from (see the docstring)
        if block_free:
            ev._bind(model).set_time_parallel(mode)

    chain_mode = 3 if (total_lightcurves is not None
                       and int(total_lightcurves) * (walkers // 2) <= REPRODUCIBLE_TP_ROWS) else 0

    try:
        if fit:
            kernels(3)
            hook = analytic if fit_gradient == "analytic" else None
            if hook is not None:
                try:
                    hook(centers)       # a model the tangent sweep is not compiled for (rank above 6) says so here
                except _engine.EngineError as exc:
                    if exc.code != _engine.E_UNSUPPORTED:
                        raise
                    warnings.warn("derive_posteriors_batch(fit_gradient='analytic'): the model's rank is beyond the device's "
                                  "tangent sweep; using finite differences")
                    hook = None
            fit_x, fit_f, _ = batched_minimize(lambda x, lc: -checked(x, lc, False), centers, lower, upper, value_and_grad=hook)
            centers, fit_f = fit_x, -fit_f
            timer.mark("fit")
        kernels(chain_mode)
        if block_free:
            p0 = np.concatenate([_spread(np.random.default_rng([int(seed), 1, int(index_base) + l]), centers[l:l + 1],
                                         lower, upper, walkers) for l in range(L)])
            sampler_seed = int(np.random.default_rng([int(seed), 2]).integers(0, 2 ** 62))
        else:
            rng = np.random.default_rng(seed)
            p0 = _spread(rng, centers, lower, upper, walkers)
        timer.mark("spread")
        if before_sampling is not None:
            before_sampling()
            timer.mark("wait")
        if device_sampler and ev is not None:
            from .device_sampler import DeviceEnsembleSampler
            dev = DeviceEnsembleSampler(lambda: ev._bind(model), walkers, P, n_ensembles=L,
                                        seed=sampler_seed if block_free else int(rng.integers(0, 2 ** 62)),
                                        store_chain=store_chain, index_base=index_base or 0)
            dev.run_mcmc(p0, max_steps)
            if not quiet and dev.state["n_not_pd"]:
                raise LinAlgError("failed to factorize or solve matrix")
            sampler = _DeviceBatch(dev)
        else:
            sampler = EnsembleBatchSampler(L, walkers, P, lambda x, lc: checked(x, lc, True), seed=rng,
                                           store_chain=store_chain)
            sampler.run(p0, max_steps)
    finally:
        kernels(2)
    timer.mark("sample")
    if store_chain:
        tau = sampler.get_autocorr_time(tol=0)
        mean_tau = np.mean(tau, axis=1)
        # not-converged branch of gpmodelling.py:272-276 (a fixed-length PPP run never "converges")
        thin = np.maximum((mean_tau / 4).astype(int), 1)
        discard = np.minimum(mean_tau.astype(int) * 5, np.maximum(max_steps - thin, 0))
    else:
        tau = None
        thin = np.ones(L, dtype=int)
        discard = np.zeros(L, dtype=int)
    names = tuple("kernel:" + n for n in kernel.get_parameter_names())
    res = BatchPosteriors(sampler, tau, discard, thin, fit_x, fit_f, names)
    if own_engine and ev is not None:
        ev.close()      # (everything BatchPosteriors needs has been copied to the host by now)
    timer.mark("collect")
    res.seconds = timer.seconds     # wall time of each phase
    return res


def protassov_test(lightcurve, null_kernel, alt_kernel, nsims=100, walkers=12, max_steps=500, sim_walkers=None,
                   sim_steps=500, sigma_noise=None, extension_factor=2, seed=None, device=0, progress=False,
                   sharded=False, group=None, concurrent_refits="auto", split="auto", reproducible=None,
                   observed_side_by_side=True, observed_split=True, pdf="Gaussian", max_iter=400):
    """The whole posterior-predictive likelihood-ratio test of the reference's workflow
    (README.md:38-41, docs/notebooks/tutorial_ppp.ipynb) on the GPU:

    1. posteriors of the null and the alternative kernel on the observed light curve,
       ``T_obs = -2 (max lnL_null - max lnL_alt)``;
    2. ``nsims`` light curves simulated from the null posteriors (device TK95);
    3. both kernels refitted to every simulated light curve in lock-step;
    4. p-value of ``T_obs`` in the simulated distribution.

    Who does what is decided first, in one value (``_ppp_plan._plan_protassov``); the steps then run as the stages of
    ``_ProtassovRun`` over that plan, on random numbers drawn in the order ``_seed_schedule`` states.

    Returns dict(T_obs, T_sim[nsims], p_value ((1 + #{T_sim >= T_obs}) / (1 + nsims)), p_value_percentile (the tutorial's own
    ``1 - percentileofscore(T_sim, T_obs) / 100``), null, alt, sim_null, sim_alt, lightcurves, seconds, split, reproducible) --
    ``seconds``:
    wall time of the observed chains, the simulation and the two refits on this process.

    ``concurrent_refits``: the null and the alternative refits of step 3 side by side on the device (two contexts, two
    host threads) instead of one after the other; the results are the same either way (``seconds`` then gives the two
    refits' common wall time under "refit_null" and 0 under "refit_alt").  "auto" (default): side by side when a
    half-step leaves the GPU room -- at most ~40 000 rows, e.g. one GPU's 250 light curves x 128 proposals at 8 GPUs,
    where the two models' launches interleave and their tails and sampler kernels overlap (7.1 ms per iteration of both
    against 8.1 ms one after the other); with the GPU full (2000 x 128 rows) there is nothing to gain (26.30 s against
    26.36 s) and the refits run one after the other.  For measurements: "unpaired" = side by side without
    ``mtg_pair_contexts`` (each context launches its own pipelined half-steps), "slices" = each context on its own half of
    the compute units (``mtg_create_on_slice``); same results all ways.

    ``observed_side_by_side`` (default on; even walker counts): the observed light curve's two chains of step 1 from two
    host threads, each model on a device context and a random generator of its own -- two single-light-curve chains
    leave the GPU nearly empty; the chains are the ones that running them one after the other gives.

    ``sharded`` (inside a ``torch.distributed`` job, one process per GPU, every rank calling with the same
    arguments and its own ``device``; BASELINE configs[3]): steps 2 and 3 -- the loop over simulated light curves
    of tutorial_ppp.ipynb:326-343 -- are cut into contiguous blocks, one per rank (``distributed.LightcurveShard``):
    rank r simulates and refits only its block, nothing is exchanged meanwhile, and ONE all-gather per model of the
    maxima of lnL (8 bytes per light curve) gives every rank the whole ``T_sim``.  Step 1 is split by model
    (``observed_split``, two ranks or more): rank 0 runs the null model's chain on the observed light curve, rank 1 the
    alternative's, nobody else any; rank 1's maximum and rank 0's maximum, posterior samples and seeds are broadcast,
    so that all ranks test the same thing -- the chains are the ones one process runs (each model has a generator of its
    own), hence the same ``T_obs`` to the last bit.  **The returned ``null`` is then rank 0's alone and ``alt`` rank 1's
    (``None`` on every other rank** -- a caller that reads ``res["null"].sampler`` on all ranks passes
    ``observed_split=False``); a chain that fails on rank 0 or 1 raises on every rank (a ``RuntimeError`` naming the rank
    on the others); ``observed_split=False``: every rank runs both and keeps both, rank 0's are everybody's test.
    ``sim_null``, ``sim_alt`` and ``lightcurves`` hold the rank's own block.  ``split``: "lightcurves" as just described,
    "models" -- the first half of the ranks refits the null model, the second half the alternative, each over all the
    light curves (a rank then holds ``sim_null`` or ``sim_alt``, not both) --, "auto" picks by the rows a half-step
    leaves each rank (``_split_by_model``).

    ``reproducible`` (default: on when ``sharded`` and it costs nothing, see below): ``T_sim`` and the p-value do not
    depend on the number of ranks or on the split -- a run on 8 GPUs can be CHECKED against a run on one, bit for bit.  Every simulated light curve
    is then a function of (seed, its global index) alone: the simulator's noise stream and each refit's Philox
    counters are keyed by global index (``mtg_set_stream_base``), the walkers start from a generator of the light
    curve's own, and the refits keep to kernels whose results do not depend on the batch a row travels in
    (``derive_posteriors_batch(index_base=..., total_lightcurves=nsims)``; what the host draws -- Kraft noise, a
    non-Gaussian flux PDF -- comes from a generator per light curve as well).  Off, every block draws from a stream of
    its own and every batch takes whichever kernel is fastest for its size: the same statistics, not the same numbers.
    The price of "on" is the kernel choice: a set beyond ``REPRODUCIBLE_TP_ROWS`` rows per half-step keeps its chains
    on the sweep, which a rank whose own share is small (under ~8000 rows: the time-parallel kernels' range) pays
    with 2.4-3.4 ms per half-step instead of 0.35-1.8 ms at N = 1e4.  The default is therefore "on" only where that
    does not happen -- the set is small enough for the batch-independent time-parallel kernel everywhere, or every
    rank's share is beyond the time-parallel range anyway (BASELINE configs[3]: 250 x 128 rows per rank) -- and the
    returned dict says which it was (``reproducible``).  (The observed light curve's chains are rank 0's either way.)
    """
    from .simulator import Simulator
    from .stats import lrt_pvalue, lrt_pvalue_percentile, lrt_statistic
    shard = None
    if sharded:
        from .distributed import LightcurveShard
        shard = LightcurveShard(nsims, group=group)
    plan = _plan_protassov(nsims, walkers, sim_walkers, shard.rank if sharded else 0, shard.world if sharded else 1,
                           sharded, split, reproducible, observed_split, observed_side_by_side, concurrent_refits)
    run = _ProtassovRun(plan, lightcurve, (null_kernel, alt_kernel), device, group)
    timer = PhaseTimer()
    # the simulator's transform plan is built beside the observed chains (its grid depends on the sampling alone)
    # (``pdf``: the flux PDF of the simulated light curves, simulator.py:149-150 -- "Lognormal" / "Uniform" go through the
    # E13 adjustment on the device, csrc/mtg_e13.hip, ``max_iter`` iterations at most: the loop still never leaves the GPU)
    sim = Simulator(null_kernel, lightcurve.times, lightcurve.exposures, lightcurve.mean, pdf,
                    lightcurve.bkg_rate, lightcurve.bkg_rate_err, sigma_noise=sigma_noise,
                    extension_factor=extension_factor, max_iter=max_iter, random_state=0, device=device)
    sim.warm_up()
    seeds = _seed_schedule(seed, nsims)
    null, alt = run.observed_chains(next(seeds), walkers, max_steps, progress)
    timer.mark("observed_chains")
    picks, sim_seed, fit_seeds = seeds.send(null)
    t_obs, samples, sim_seed, fit_seeds = run.exchange_head(null, alt, picks, sim_seed, fit_seeds)
    out, fits, pair_stats, failure = None, [None, None], None, None
    if plan.hi > plan.lo:
        try:
            out = run.simulate(sim, samples, sim_seed)
            timer.mark("simulate")
            fits, pair_stats = run.refit(out, fit_seeds, sim_steps, timer)
        except BaseException as exc:     # (simulation or refits: one process raises at once, a rank says it to the others first)
            failure = exc
            if not sharded:
                raise
    t_sim = lrt_statistic(*run.gather(fits, out, failure))
    if plan.hi > plan.lo:                # (a rank without a block reports its observed chains only)
        timer.mark("gather")
    return dict(T_obs=t_obs, T_sim=t_sim, p_value=lrt_pvalue(t_obs, t_sim), p_value_percentile=lrt_pvalue_percentile(t_obs, t_sim), null=null, alt=alt,
                sim_null=fits[0], sim_alt=fits[1], lightcurves=out, seconds=timer.seconds, reproducible=plan.reproducible,
                paired_launches=pair_stats, split=plan.split)


def periodogram_peak_test(lightcurve, null_kernel, frequencies, nsims=100, walkers=12, max_steps=500, sigma_noise=None,
                          extension_factor=2, normalization="standard", weighted=True, seed=None, device=0, progress=False,
                          pdf="Gaussian", max_iter=400, nterms=1, statistic="lomb_scargle", nbins=10, taus=None,
                          decay=_engine.WWZ_DECAY):
    """The classic companion of the LRT p-value of ``protassov_test``: is the highest Lomb-Scargle peak of the observed
    light curve unusual among light curves of the null model?

    1. posterior of ``null_kernel`` on the observed light curve (the chain ``protassov_test`` runs for its null model);
    2. ``nsims`` posterior samples, one light curve simulated from each on the observed sampling (device TK95, the path
       ``protassov_test`` takes) and left resident on the device;
    3. the generalised Lomb-Scargle periodogram of every simulated light curve at ``frequencies``, reduced to its peak on
       the device (``Engine.lomb_scargle(power=False, peak=True)``), and the same of the observed light curve.

    Returns dict(observed_peak, observed_frequency, sim_peaks[nsims], p_value = (1 + #{sim >= obs}) / (1 + nsims), null,
    samples[nsims][P], sim_seed, lightcurves) -- the last three are what step 2 drew and made.  One GPU.  Every random number
    comes from ``default_rng(seed)`` in a fixed order (the chain's seed, the picks, the simulator's seed): the same seed gives
    the same result bit for bit.  ``weighted``: by the error bars, the simulated light curves' own included -- Poisson noise
    at a few counts per epoch leaves epochs with ``dy = 0`` that take all the weight; pass ``weighted=False`` there.
    ``nterms``: harmonics per frequency of every periodogram (``Engine.lomb_scargle``), for profiles that are not sinusoidal.
    ``statistic="epoch_fold"``: the peaks of the epoch-folding periodogram instead (``Engine.epoch_fold`` with ``nbins``
    phase bins counted from the first observed time; ``nterms`` must be 1) -- for dips, eclipses and narrow pulses.
    ``statistic="wwz"``: the highest value of Foster's Z over the whole time-frequency map (``Engine.wwz`` at
    ``frequencies`` and the window centres ``taus``, None: 50 evenly spaced over the observed span, with the decay constant
    ``decay``; ``nterms`` must be 1, ``normalization`` is not used) -- for a periodicity that lasts for part of the light
    curve only.  No map leaves the device; ``observed_frequency`` is the ridge's frequency and ``observed_tau`` its centre."""
    if statistic not in ("lomb_scargle", "epoch_fold", "wwz"):
        raise ValueError("statistic must be 'lomb_scargle', 'epoch_fold' or 'wwz'")
    if statistic in ("epoch_fold", "wwz") and nterms != 1:
        raise ValueError("statistic=%r has no harmonics: nterms must be 1" % statistic)
    frequencies = np.ascontiguousarray(np.atleast_1d(frequencies), dtype=np.float64).ravel()
    eng, null, samples, sim_seed, out = _simulate_null_set(lightcurve, null_kernel, nsims, walkers, max_steps, sigma_noise,
                                                           extension_factor, seed, device, progress, pdf, max_iter)
    times = np.asarray(lightcurve.times, dtype=np.float64)
    if statistic == "wwz":
        taus = np.linspace(times.min(), times.max(), 50) if taus is None else np.ascontiguousarray(np.atleast_1d(taus), dtype=np.float64).ravel()

        def peaks(weighted):
            return eng.wwz(frequencies, taus, decay=decay, statistic="z", weighted=weighted, values=False, peak=True)
    elif statistic == "epoch_fold":
        def peaks(weighted):
            return eng.epoch_fold(frequencies, nbins=nbins, time_0=float(times[0]), normalization=normalization, weighted=weighted,
                                  power=False, peak=True)
    else:
        def peaks(weighted):
            return eng.lomb_scargle(frequencies, normalization=normalization, weighted=weighted, power=False, peak=True,
                                    **_harmonics(nterms))
    sim_peaks, _ = peaks(weighted)
    y = np.asarray(lightcurve.y, dtype=np.float64)
    dy = np.ones_like(y) if lightcurve.dy is None else np.asarray(lightcurve.dy, dtype=np.float64)
    eng.set_lightcurves(times, y, dy)
    eng.bound_to = None
    obs, at = peaks(weighted and lightcurve.dy is not None)
    observed_peak = float(obs[0])
    p_value = (1.0 + float(np.sum(sim_peaks >= observed_peak))) / (1.0 + nsims)
    res = dict(observed_peak=observed_peak, observed_frequency=float(frequencies[at[0] % len(frequencies)]) if at[0] >= 0 else float("nan"),
               sim_peaks=sim_peaks, p_value=p_value, null=null, samples=samples, sim_seed=sim_seed, lightcurves=out)
    if statistic == "wwz":
        res["observed_tau"] = float(taus[at[0] // len(frequencies)]) if at[0] >= 0 else float("nan")
    return res


def _harmonics(nterms):
    """The keyword of the engine's periodogram calls for ``nterms`` harmonics: none for one term, so that an engine-like
    object with the one-term signature serves the default."""
    return {} if nterms == 1 else {"nterms": nterms}


def _simulate_null_set(lightcurve, null_kernel, nsims, walkers, max_steps, sigma_noise, extension_factor, seed, device,
                       progress, pdf, max_iter):
    """Steps 1 and 2 of ``periodogram_peak_test`` and ``periodogram_significance``: the null model's chain on the observed
    light curve, ``nsims`` posterior samples, one light curve simulated from each and left resident on the device's
    engine -> (engine, null, samples, sim_seed, lightcurves).  Every random number comes from ``default_rng(seed)`` in a
    fixed order (the chain's seed, the picks, the simulator's seed)."""
    from .gp import get_engine
    from .gpmodelling import GPModelling
    from .simulator import Simulator
    sim = Simulator(null_kernel, lightcurve.times, lightcurve.exposures, lightcurve.mean, pdf,
                    lightcurve.bkg_rate, lightcurve.bkg_rate_err, sigma_noise=sigma_noise,
                    extension_factor=extension_factor, max_iter=max_iter, random_state=0, device=device)
    sim.warm_up()
    rng = np.random.default_rng(seed)
    chain_seed = int(rng.integers(0, 2 ** 31 - 1))
    on_device = walkers % 2 == 0
    null = GPModelling(lightcurve, null_kernel, device=device, random_state=np.random.RandomState(chain_seed) if on_device else None)
    state = np.random.get_state()
    if not on_device:
        np.random.seed(chain_seed)
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            null.derive_posteriors(fit=True, max_steps=max_steps, walkers=walkers, progress=progress, device_sampler=on_device)
    finally:
        if not on_device:
            np.random.set_state(state)
    samples = null.mcmc_samples[rng.integers(len(null.mcmc_samples), size=nsims)][:, :null_kernel.vector_size]
    sim_seed = int(rng.integers(0, 2 ** 31 - 1))
    eng = get_engine(device)
    out = sim.simulate(samples, make_resident=True, seed=sim_seed)      # (the process-wide engine of the device holds them now)
    return eng, null, samples, sim_seed, out


def _observed_power(eng, lightcurve, frequencies, normalization, weighted, nterms=1):
    """The observed light curve made resident (nobody's evaluator's afterwards), and its periodogram [F]."""
    y = np.asarray(lightcurve.y, dtype=np.float64)
    dy = np.ones_like(y) if lightcurve.dy is None else np.asarray(lightcurve.dy, dtype=np.float64)
    eng.set_lightcurves(np.asarray(lightcurve.times, dtype=np.float64), y, dy)
    eng.bound_to = None
    return eng.lomb_scargle(frequencies, normalization=normalization, weighted=weighted and lightcurve.dy is not None,
                            **_harmonics(nterms))[0]


def _significance_of_resident_set(eng, observed_power, frequencies, nsims, levels, normalization, weighted, nterms=1):
    """Steps 4 to 6 of ``periodogram_significance`` on an engine that holds the ``nsims`` simulated light curves: the two
    envelope calls and the arithmetic on what comes back (tests drive it with a stand-in engine on the CPU)."""
    from .periodogram import envelope_levels, envelope_ranks
    levels = tuple(float(v) for v in np.atleast_1d(levels))
    harmonics = _harmonics(nterms)
    if not np.all(np.isfinite(observed_power)):
        k = int(np.flatnonzero(~np.isfinite(observed_power))[0])
        raise ValueError("periodogram_significance: the observed power at frequencies[%d] = %g is not finite" % (k, frequencies[k]))
    ranks = envelope_ranks(nsims, (0.5,) + levels)
    env = eng.lomb_scargle_envelope(frequencies, ranks=ranks, reference=observed_power, normalization=normalization, weighted=weighted,
                                    **harmonics)
    quantiles = envelope_levels(env.order_stat, ranks, nsims, (0.5,) + levels)
    median = quantiles[0]
    bad = ~(np.isfinite(median) & (median > 0))
    if bad.any():
        k = int(np.flatnonzero(bad)[0])
        raise ValueError("periodogram_significance: the median power of the simulated light curves at frequencies[%d] = %g is %g, "
                         "not finite and positive" % (k, frequencies[k], median[k]))
    peaks = eng.lomb_scargle_envelope(frequencies, scale=median, normalization=normalization, weighted=weighted, **harmonics)
    ratio = observed_power / median
    at = int(np.argmax(ratio))                     # (finite over finite and positive: no NaN; the first maximum)
    observed_ratio_peak = float(ratio[at])
    return dict(observed_power=observed_power, median=median, levels=quantiles[1:],
                local_p=(1.0 + env.exceed) / (1.0 + nsims),
                observed_ratio_peak=observed_ratio_peak, observed_frequency=float(frequencies[at]),
                sim_ratio_peaks=peaks.peak_ratio,
                global_p=(1.0 + float(np.sum(peaks.peak_ratio >= observed_ratio_peak))) / (1.0 + nsims))


def periodogram_significance(lightcurve, null_kernel, frequencies, nsims=100, levels=(0.95, 0.997), walkers=12, max_steps=500,
                             sigma_noise=None, extension_factor=2, normalization="standard", weighted=True, seed=None, device=0,
                             progress=False, pdf="Gaussian", max_iter=400, nterms=1):
    """What a red-noise periodicity search reports (Vaughan 2005): the significance of the observed Lomb-Scargle power
    frequency by frequency, against light curves of the null model.  ``periodogram_peak_test`` compares highest RAW peaks,
    which for red-noise nulls sit at the lowest frequencies whatever the data hold; this compares every frequency with the
    null's own distribution there, and corrects for the trials with the highest RATIO of power to the null's median.

    1. the observed light curve's periodogram at ``frequencies``;
    2. and 3. the null chain, the ``nsims`` posterior picks and the simulated set of ``periodogram_peak_test``: the same
       ones for the same seed, left resident on the device;
    4. one ``Engine.lomb_scargle_envelope`` call on that set: the order statistics for the median and ``levels`` (numpy's
       "linear" quantiles, ``periodogram.envelope_levels``) and, per frequency, the simulations at or above the observed power;
    5. a second call with ``scale=median``: every simulation's highest power / median;
    6. the same ratio peak of the observed light curve, on the host.
    The [nsims][F] powers never leave the device.

    Returns dict(observed_power[F], median[F], levels[len(levels)][F], local_p[F] = (1 + exceed) / (1 + nsims),
    observed_ratio_peak, observed_frequency, sim_ratio_peaks[nsims], global_p = (1 + #{sim >= obs}) / (1 + nsims), null,
    samples[nsims][P], sim_seed, lightcurves).  A median that is not finite and positive at some frequency raises a
    ValueError naming it.  One GPU; the same seed gives the same result bit for bit.  ``weighted``: by the error bars, the
    simulated light curves' own included -- Poisson noise at a few counts per epoch leaves epochs with ``dy = 0`` that
    take all the weight; pass ``weighted=False`` there.  ``nterms``: harmonics per frequency of every periodogram
    (``Engine.lomb_scargle``)."""
    from .gp import get_engine
    frequencies = np.ascontiguousarray(np.atleast_1d(frequencies), dtype=np.float64).ravel()
    observed_power = _observed_power(get_engine(device), lightcurve, frequencies, normalization, weighted, nterms)
    eng, null, samples, sim_seed, out = _simulate_null_set(lightcurve, null_kernel, nsims, walkers, max_steps, sigma_noise,
                                                           extension_factor, seed, device, progress, pdf, max_iter)
    res = _significance_of_resident_set(eng, observed_power, frequencies, nsims, levels, normalization, weighted, nterms)
    res.update(null=null, samples=samples, sim_seed=sim_seed, lightcurves=out)
    return res


def _lag_statistic(eng, Y, DY, edges, statistic, subtract_noise):
    """The structure function or the discrete correlation function [L][nbins] of the light curves resident on ``eng``
    (``Y``, ``DY`` [L][N]: the same ones on the host, for the variances the correlation function is normalised by)."""
    from .timedomain import dcf_from_sums, sf_from_sums
    if statistic == "sf":
        sums = eng.lag_sums(edges, count=True, lag=True, sf=True, noise=subtract_noise)
        return sf_from_sums(sums, subtract_noise)[1]
    sums = eng.lag_sums(edges, count=True, lag=True, sf=False, cf=True, cf2=True)
    s2 = np.mean((Y - Y.mean(axis=1, keepdims=True)) ** 2, axis=1)
    e2 = np.mean(DY ** 2, axis=1) if subtract_noise else np.zeros(len(Y))
    return dcf_from_sums(sums, s2, e2)[1]


def _lag_levels(observed, sims, levels):
    """The host arithmetic of ``lag_significance``: ``observed`` [nbins] against ``sims`` [nsims][nbins] -> dict(median,
    lower, upper, share_above, share_below).  A bin in which the observed value or any simulation is NaN (an empty bin) is
    NaN in every output."""
    levels = np.atleast_1d(np.asarray(levels, dtype=np.float64))
    if np.any(levels <= 0.5) or np.any(levels >= 1.0):
        raise ValueError("levels must lie in (0.5, 1)")
    ok = np.isfinite(observed) & np.all(np.isfinite(sims), axis=0)
    safe = np.where(ok[None, :], sims, 0.0)
    blank = lambda a: np.where(ok, a, np.nan)
    return dict(median=blank(np.quantile(safe, 0.5, axis=0)), lower=blank(np.quantile(safe, 1.0 - levels, axis=0)),
                upper=blank(np.quantile(safe, levels, axis=0)),
                share_above=blank(np.mean(safe >= np.where(ok, observed, 0.0)[None, :], axis=0)),
                share_below=blank(np.mean(safe <= np.where(ok, observed, 0.0)[None, :], axis=0)))


def lag_significance(lightcurve, null_kernel, edges, statistic="sf", nsims=100, levels=(0.95, 0.997), walkers=12, max_steps=500,
                     sigma_noise=None, extension_factor=2, subtract_noise=True, seed=None, device=0, progress=False,
                     pdf="Gaussian", max_iter=400):
    """``periodogram_significance`` in the time-lag view: is the observed structure function (``statistic="sf"``) or
    discrete correlation function (``"dcf"``) in the lag bins ``edges`` (``timedomain.lag_bins``) unusual, bin by bin,
    among light curves of the null model?

    1. the observed light curve's statistic (``Engine.lag_sums``, normalised by ``timedomain``);
    2. and 3. the null chain, the ``nsims`` posterior picks and the simulated set of ``periodogram_peak_test``: the same
       ones for the same seed, left resident on the device;
    4. one ``Engine.lag_sums`` call on that set, and ``np.quantile`` over the [nsims][nbins] values on the host.

    Returns dict(lag[nbins] the mean lag of each bin, count[nbins], observed[nbins], median[nbins], lower[len(levels)][nbins]
    and upper[len(levels)][nbins] -- the quantiles ``1 - level`` and ``level`` --, share_above[nbins] and share_below[nbins]
    -- the shares of simulations at or above and at or below the observed value --, sims[nsims][nbins], null,
    samples[nsims][P], sim_seed, lightcurves).  A bin without pairs is NaN throughout.  ``subtract_noise``: the
    measurement-noise term of either statistic, from the error bars (the simulated light curves' own included).  There is
    no trial-corrected p-value over the bins.  One GPU; the same seed gives the same result bit for bit."""
    from .gp import get_engine
    from .timedomain import sf_from_sums
    if statistic not in ("sf", "dcf"):
        raise ValueError("statistic must be 'sf' or 'dcf'")
    edges = np.ascontiguousarray(np.atleast_1d(edges), dtype=np.float64).ravel()
    times = np.asarray(lightcurve.times, dtype=np.float64)
    y = np.asarray(lightcurve.y, dtype=np.float64)
    noise = bool(subtract_noise) and lightcurve.dy is not None
    dy = np.ones_like(y) if lightcurve.dy is None else np.asarray(lightcurve.dy, dtype=np.float64)
    eng = get_engine(device)
    eng.set_lightcurves(times, y, dy)
    eng.bound_to = None
    observed = _lag_statistic(eng, y[None, :], dy[None, :], edges, statistic, noise)[0]
    lag, _, count = sf_from_sums(eng.lag_sums(edges, count=True, lag=True, sf=True), False)
    eng, null, samples, sim_seed, out = _simulate_null_set(lightcurve, null_kernel, nsims, walkers, max_steps, sigma_noise,
                                                           extension_factor, seed, device, progress, pdf, max_iter)
    sims = _lag_statistic(eng, np.asarray(out["rates"], dtype=np.float64), np.asarray(out["dy"], dtype=np.float64), edges,
                          statistic, bool(subtract_noise))
    res = dict(lag=lag[0], count=count[0], observed=observed, sims=sims, null=null, samples=samples, sim_seed=sim_seed, lightcurves=out)
    res.update(_lag_levels(observed, sims, levels))
    return res


def _cross_statistic(eng, Y, DY, t2, y2, dy2, edges, normalization, subtract_noise):
    """(mean lag, CCF, count), each [L][nbins], of the light curves resident on ``eng`` (``Y``, ``DY`` [L][N]: the same ones
    on the host, for the variances of the global normalisation) against the one companion ``t2, y2, dy2`` (``dy2`` None:
    no noise term): one ``cross_sums`` call."""
    from .timedomain import ccf_from_sums
    local = normalization == "local"
    sums = eng.cross_sums(t2, y2, edges, count=True, lag=True, cf=True, cf2=True, sa=local, sb=local, saa=local, sbb=local)
    s2a = np.mean((Y - Y.mean(axis=1, keepdims=True)) ** 2, axis=1)
    s2b = float(np.mean((y2 - y2.mean()) ** 2))
    e2a = np.mean(DY ** 2, axis=1) if subtract_noise else np.zeros(len(Y))
    e2b = float(np.mean(dy2 ** 2)) if subtract_noise and dy2 is not None else 0.0
    lag, ccf, _, count = ccf_from_sums(sums, s2a, s2b, e2a, e2b, normalization)
    return lag, ccf, count


def _cross_peaks(lag, ccf):
    """Per row of ``ccf`` [L][nbins]: (the largest |CCF| over the finite bins, the mean lag of that bin: the first such
    bin); NaN for a row without a finite bin."""
    mag = np.where(np.isfinite(ccf), np.abs(ccf), -1.0)
    at = np.argmax(mag, axis=1)
    rows = np.arange(len(ccf))
    none = mag[rows, at] < 0
    return np.where(none, np.nan, mag[rows, at]), np.where(none, np.nan, lag[rows, at])


def _cross_global_p(observed_peak, sim_peaks):
    """``(1 + #{simulations whose peak is at or above the observed one}) / (1 + nsims)``: a simulation without a finite
    bin (NaN) does not count as above; an observed CCF without one gives NaN."""
    sim_peaks = np.asarray(sim_peaks, dtype=np.float64)
    if not np.isfinite(observed_peak):
        return float("nan")
    return (1.0 + float(np.sum(sim_peaks >= observed_peak))) / (1.0 + len(sim_peaks))


def cross_lag_significance(lightcurve, companion, null_kernel, edges, nsims=100, levels=(0.95, 0.997), normalization="global",
                           walkers=12, max_steps=500, sigma_noise=None, extension_factor=2, subtract_noise=True, seed=None, device=0,
                           progress=False, pdf="Gaussian", max_iter=400):
    """Is the cross-correlation of ``lightcurve`` with ``companion`` (a second light curve on its own sampling: ``times``,
    ``y``, ``dy`` or None) in the signed lag bins ``edges`` (``timedomain.cross_lag_bins``; positive: the companion lags)
    unusual if the light curve is red noise of ``null_kernel``, INDEPENDENT of the companion?

    1. the observed CCF (``Engine.cross_sums``, normalised by ``timedomain.ccf_from_sums``, ``normalization`` "global" or
       "local");
    2. and 3. the null chain, the ``nsims`` posterior picks and the simulated set of ``lag_significance``: the same ones for
       the same seed, left resident on the device;
    4. ONE ``Engine.cross_sums`` call of that set against the observed companion, and ``np.quantile`` over the
       [nsims][nbins] values on the host, bin by bin;
    5. over the bins: ``peak`` = the largest ``|CCF|`` of the finite bins, of the observation and of every simulation, and
       ``p_global = (1 + #{simulations with peak >= observed}) / (1 + nsims)`` -- the trial-corrected significance.

    Returns dict(lag[nbins], count[nbins], observed[nbins], median, lower[len(levels)][nbins], upper, share_above,
    share_below as ``lag_significance``; peak, peak_lag the observation's; sim_peaks[nsims], sim_peak_lags[nsims];
    p_global; sims[nsims][nbins], null, samples[nsims][P], sim_seed, lightcurves).  A bin with fewer than two pairs is NaN
    throughout.  ``subtract_noise``: the measurement-noise terms of the global normalisation, from the error bars (the
    simulated light curves' own included).  One GPU; the same seed gives the same result bit for bit."""
    from .gp import get_engine
    if normalization not in ("global", "local"):
        raise ValueError("normalization must be 'global' or 'local'")
    edges = np.ascontiguousarray(np.atleast_1d(edges), dtype=np.float64).ravel()
    times = np.asarray(lightcurve.times, dtype=np.float64)
    y = np.asarray(lightcurve.y, dtype=np.float64)
    noise = bool(subtract_noise) and lightcurve.dy is not None
    dy = np.ones_like(y) if lightcurve.dy is None else np.asarray(lightcurve.dy, dtype=np.float64)
    t2 = np.ascontiguousarray(companion.times, dtype=np.float64)
    y2 = np.ascontiguousarray(companion.y, dtype=np.float64)
    dy2 = None if getattr(companion, "dy", None) is None else np.asarray(companion.dy, dtype=np.float64)
    if t2.ndim != 1 or y2.shape != t2.shape:
        raise ValueError("the companion must be one series: times [M] and y [M]")
    eng = get_engine(device)
    eng.set_lightcurves(times, y, dy)
    eng.bound_to = None
    lag, observed, count = _cross_statistic(eng, y[None, :], dy[None, :], t2, y2, dy2, edges, normalization, noise)
    peak, peak_lag = _cross_peaks(lag, observed)
    eng, null, samples, sim_seed, out = _simulate_null_set(lightcurve, null_kernel, nsims, walkers, max_steps, sigma_noise,
                                                           extension_factor, seed, device, progress, pdf, max_iter)
    sim_lag, sims, _ = _cross_statistic(eng, np.asarray(out["rates"], dtype=np.float64), np.asarray(out["dy"], dtype=np.float64), t2, y2,
                                        dy2, edges, normalization, bool(subtract_noise))
    sim_peaks, sim_peak_lags = _cross_peaks(sim_lag, sims)
    res = dict(lag=lag[0], count=count[0], observed=observed[0], sims=sims, peak=float(peak[0]), peak_lag=float(peak_lag[0]),
               sim_peaks=sim_peaks, sim_peak_lags=sim_peak_lags, p_global=_cross_global_p(float(peak[0]), sim_peaks),
               null=null, samples=samples, sim_seed=sim_seed, lightcurves=out)
    res.update(_lag_levels(observed[0], sims, levels))
    return res


def iccf_significance(lightcurve, companion, null_kernel, lags, nsims=100, levels=(0.95, 0.997), mode="both", threshold=0.8,
                      walkers=12, max_steps=500, sigma_noise=None, extension_factor=2, seed=None, device=0, progress=False,
                      pdf="Gaussian", max_iter=400):
    """``cross_lag_significance`` for the interpolated cross-correlation function: is the ICCF of ``lightcurve`` with
    ``companion`` (``times``, ``y``) at ``lags`` (``timedomain.iccf_lags``; positive: the companion lags) unusual if the
    light curve is red noise of ``null_kernel``, INDEPENDENT of the companion?  Linear interpolation across the gaps of
    either sampling invents data; the simulated light curves live on the same gappy sampling and are interpolated the
    same way, which is what makes the comparison fair.

    1. the observed ICCF, its peak and its centroid (``Engine.iccf``; ``mode``, ``threshold`` as there);
    2. and 3. the null chain, the ``nsims`` posterior picks and the simulated set of ``cross_lag_significance``: the same
       ones for the same seed, left resident on the device;
    4. ONE ``Engine.iccf`` call of that set against the observed companion, and ``np.quantile`` over the [nsims][K]
       values on the host, lag by lag;
    5. ``p_global = (1 + #{simulations whose peak r >= the observed peak r}) / (1 + nsims)``.

    Returns dict(lags[K], n_a[K], n_b[K], observed[K], median, lower[len(levels)][K], upper, share_above, share_below as
    ``lag_significance``; peak, peak_lag, centroid the observation's; sim_peaks[nsims], sim_peak_lags[nsims],
    sim_centroids[nsims]; p_global; sims[nsims][K], null, samples[nsims][P], sim_seed, lightcurves).  A lag at which a
    half has fewer than two samples is NaN throughout.  One GPU; the same seed gives the same result bit for bit."""
    from .engine import ICCF_MODES
    from .gp import get_engine
    if mode not in ICCF_MODES:
        raise ValueError("mode must be one of %s" % sorted(ICCF_MODES))
    if not 0.0 < threshold <= 1.0:
        raise ValueError("threshold must lie in (0, 1]")
    lags = np.ascontiguousarray(np.atleast_1d(lags), dtype=np.float64).ravel()
    times = np.asarray(lightcurve.times, dtype=np.float64)
    y = np.asarray(lightcurve.y, dtype=np.float64)
    dy = np.ones_like(y) if lightcurve.dy is None else np.asarray(lightcurve.dy, dtype=np.float64)
    t2 = np.ascontiguousarray(companion.times, dtype=np.float64)
    y2 = np.ascontiguousarray(companion.y, dtype=np.float64)
    if t2.ndim != 1 or y2.shape != t2.shape:
        raise ValueError("the companion must be one series: times [M] and y [M]")
    lag_at = lambda index: np.where(index >= 0, lags[np.maximum(index, 0)], np.nan)
    eng = get_engine(device)
    eng.set_lightcurves(times, y, dy)
    eng.bound_to = None
    obs = eng.iccf(t2, y2, lags, mode=mode, threshold=threshold, values=True, counts=True, peak=True)
    eng, null, samples, sim_seed, out = _simulate_null_set(lightcurve, null_kernel, nsims, walkers, max_steps, sigma_noise,
                                                           extension_factor, seed, device, progress, pdf, max_iter)
    sim = eng.iccf(t2, y2, lags, mode=mode, threshold=threshold, values=True, counts=False, peak=True)
    peak = float(obs.peak[0])
    res = dict(lags=lags, n_a=obs.n_a[0], n_b=obs.n_b[0], observed=obs.ccf[0], sims=sim.ccf, peak=peak, peak_lag=float(lag_at(obs.peak_index)[0]),
               centroid=float(obs.centroid[0]), sim_peaks=sim.peak, sim_peak_lags=lag_at(sim.peak_index), sim_centroids=sim.centroid,
               p_global=_cross_global_p(peak, sim.peak), null=null, samples=samples, sim_seed=sim_seed, lightcurves=out)
    res.update(_lag_levels(obs.ccf[0], sim.ccf, levels))
    return res


def _seed_schedule(seed, nsims):
    """Every random number protassov_test itself draws, from ONE ``default_rng(seed)``, in the order every bit-for-bit
    guarantee of the sharded run rests on.  A generator of two steps: ``next`` gives the two chain seeds, ``send(null)``
    -- the null model's observed chain, or None where another rank runs it -- gives (picks or None, sim_seed, fit_seeds).

    1. two ``integers(0, 2**31 - 1)``: the seeds of the null and the alternative model's observed chain;
    2. the caller runs the observed chains; they do not touch this generator;
    3. ``integers(len(null.mcmc_samples), size=nsims)``, the posterior samples to simulate from -- ONLY where the null
       chain is held (under the observed split that is rank 0);
    4. one ``integers(0, 2**31 - 1)``: the simulator's seed;
    5. two ``integers(0, 2**52)``: the seeds of the null and the alternative refits (below 2^52: they travel as float64).

    Ranks that skipped 3 are one draw behind from there on, and every rank's chains left it a different step 3 anyway:
    rank 0's values of 3 to 5 replace everybody's in ``_ProtassovRun.exchange_head``."""
    rng = np.random.default_rng(seed)
    null = yield [int(rng.integers(0, 2 ** 31 - 1)) for _ in range(2)]
    picks = rng.integers(len(null.mcmc_samples), size=nsims) if null is not None else None
    sim_seed = int(rng.integers(0, 2 ** 31 - 1))
    fit_seeds = [int(rng.integers(0, 2 ** 52)) for _ in range(2)]
    yield picks, sim_seed, fit_seeds


def _raise_together(plan, failure, what, group):
    """Say it to everybody before the next collective: every rank tells whether ``what`` failed here (``failure``: the
    exception or None); the rank it failed on raises its own error, the others a RuntimeError naming the rank(s) --
    nobody may wait in a broadcast or a gather for values that will not come."""
    from .distributed import all_gather_rows
    failed = all_gather_rows(np.array([0.0 if failure is None else 1.0]), np.ones(plan.world, dtype=int), group)
    if failure is not None:
        raise failure
    if failed.any():
        raise RuntimeError("protassov_test: %s failed on rank(s) %s" % (what, np.flatnonzero(failed).tolist()))


def _refit_side_by_side(refit, paired, device):
    """``refit(k, before_sampling)`` of both models from two host threads (the library calls release the GIL), each on a
    context and a stream of its own -> ([null's, alternative's], pair statistics or None).  Measured at configs[3]'s
    sizes: 26.30 s side by side against 8.40 + 17.96 s one after the other -- both sweeps are bound by FP64 issue and a
    half-step leaves no idle issue slots for the other model to fill; on a block that leaves the GPU room (a rank's 250
    light curves at 8 GPUs) the two chains interleave and gain 16 %: "auto" (protassov_test's docstring).

    The threads meet between their starting fits and their chains, so that the chains -- the long, regular part --
    overlap from the first iteration to the last.  ``paired``: from there on the two contexts' pipelined half-steps go out
    in ONE launch (mtg_pair_contexts: eight waves per compute unit on one table set, two per SIMD -- a pipelined sweep
    alone takes the whole compute unit, so unpaired launches alternate rather than share SIMDs); not before, because the
    fits' batches come at each model's own pace and must not wait for each other.  A refit that fails aborts the barrier
    (no timeout: its partner must not wait there for it) and it is that refit's error that is raised, not the partner's
    broken barrier."""
    import threading
    from concurrent.futures import ThreadPoolExecutor
    from .gp import get_side_engine
    meet = threading.Barrier(2)

    def meet_then_pair():
        first = meet.wait() == 0
        if paired:
            if first:
                for k in (0, 1):
                    get_side_engine(device, k).unpair()      # (whatever an interrupted run may have left)
                get_side_engine(device, 0).pair_with(get_side_engine(device, 1))
            meet.wait()

    def guarded(k):
        try:
            return refit(k, meet_then_pair)
        except BaseException:
            meet.abort()
            raise

    pair_stats = None
    try:
        with ThreadPoolExecutor(max_workers=2) as pool:
            futures = [pool.submit(guarded, k) for k in (0, 1)]
    finally:
        if paired:     # (both threads have returned: nobody is inside a paired call)
            pair_stats = get_side_engine(device, 0).pair_stats()
            get_side_engine(device, 0).unpair()
    errors = [f.exception() for f in futures if f.exception() is not None]
    if errors:
        real = [e for e in errors if not isinstance(e, threading.BrokenBarrierError)]
        raise (real or errors)[0]
    return [f.result() for f in futures], pair_stats


class _ProtassovRun:
    """One rank's run of a Protassov test: the stages of protassov_test, in its order, over a ProtassovPlan."""

    def __init__(self, plan, lightcurve, kernels, device, group):
        self.plan, self.lightcurve, self.kernels, self.device, self.group = plan, lightcurve, kernels, device, group

    def observed_chains(self, seeds, walkers, max_steps, progress):
        """Step 1 -> [null, alt]: GPModelling of the observed light curve per model, None for a chain another rank runs."""
        from .gpmodelling import GPModelling
        plan = self.plan

        def chain(k, own_engine=False):
            """Model k's chain from a generator of its own (the stream np.random.seed(seed) would give: nothing here
            touches numpy's global generator unless the walkers are odd -- the host-side sampler copies the global
            state, as emcee does -- and then it is put back as it was)."""
            on_device = plan.observed_device_sampler
            g = GPModelling(self.lightcurve, self.kernels[k], device=self.device, own_engine=own_engine,
                            random_state=np.random.RandomState(seeds[k]) if on_device else None)
            state = np.random.get_state()
            if not on_device:
                np.random.seed(seeds[k])
            try:
                g.derive_posteriors(fit=True, max_steps=max_steps, walkers=walkers, progress=progress, device_sampler=on_device)
            finally:
                if not on_device:
                    np.random.set_state(state)
            return g

        chains = [None, None]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            if plan.observed == "by_model":
                failure = None
                try:
                    for k in plan.observed_models:
                        chains[k] = chain(k)
                except Exception as exc:
                    failure = exc
                _raise_together(plan, failure, "the observed light curve's chain", self.group)
            elif plan.observed == "side_by_side":
                from concurrent.futures import ThreadPoolExecutor
                with ThreadPoolExecutor(max_workers=2) as pool:
                    chains = list(pool.map(lambda k: chain(k, own_engine=("side", k)), (0, 1)))
                for g in chains:
                    g.gp.release_engine()
            else:
                chains = [chain(0), chain(1)]
        return chains

    def exchange_head(self, null, alt, picks, sim_seed, fit_seeds):
        """The test every rank works on -> (T_obs, samples[nsims], sim_seed, fit_seeds): one process's own; sharded, rank
        0's (every rank drew its own from its own chains' state; under the model split two ranks must simulate the SAME
        light curves), sent as ONE float64 array ``[null_best, sim_seed, fit_seeds[0], fit_seeds[1], t_obs, samples...]``.
        Under the observed split T_obs is rank 0's null maximum with rank 1's alternative maximum (its own broadcast)."""
        from .stats import lrt_statistic
        plan = self.plan
        # one estimator on both sides of the test: the largest log-posterior over everything the chains
        # visited (the refits store no chains and keep exactly that; the maximum over the burned-in,
        # thinned chain is systematically smaller, the more so the more parameters a model has)
        if plan.observed == "by_model":
            from .distributed import broadcast_array
            alt_best = float(broadcast_array(np.array([alt.best_loglikelihood if alt is not None else 0.0]), self.group, src=1)[0])
            null_best = float(null.best_loglikelihood) if null is not None else 0.0
            samples = null.mcmc_samples[picks] if null is not None else np.zeros((plan.nsims, self.kernels[0].vector_size))
        else:
            null_best, alt_best = float(null.best_loglikelihood), float(alt.best_loglikelihood)
            samples = null.mcmc_samples[picks]
        t_obs = float(lrt_statistic(null_best, alt_best))
        if plan.sharded:
            from .distributed import broadcast_array
            head = broadcast_array(np.concatenate([[null_best, float(sim_seed)], np.asarray(fit_seeds, dtype=np.float64),
                                                   [t_obs], samples.ravel()]), self.group)
            sim_seed, fit_seeds = int(head[1]), [int(head[2]), int(head[3])]
            t_obs = float(lrt_statistic(float(head[0]), alt_best)) if plan.observed == "by_model" else float(head[4])
            samples = head[5:].reshape(samples.shape)
            if not plan.reproducible:
                # independent noise on every block (the two ranks of a block under the model split draw the same)
                sim_seed = (sim_seed + BLOCK_SEED_STRIDE * plan.block) % (2 ** 31 - 1)
                fit_seeds = [f + BLOCK_SEED_STRIDE * plan.block for f in fit_seeds]
        return t_obs, samples, sim_seed, fit_seeds

    def simulate(self, sim, samples, sim_seed):
        """Step 2 -> the block's light curves, dict(rates[hi - lo][N], dy, ...) (plan.sim_lo .. keep: the pair partners)."""
        plan = self.plan
        sim.random_state = np.random.RandomState(sim_seed)
        out = sim.simulate(samples[plan.sim_lo:plan.sim_hi, :self.kernels[0].vector_size], index_base=plan.sim_index_base,
                           pair_series=plan.pair_series)
        return {k: (v[plan.keep] if v is not None else None) for k, v in out.items()}

    def refit(self, out, fit_seeds, sim_steps, timer):
        """Step 3 -> ([BatchPosteriors of the null refit or None, of the alternative's or None], pair statistics or None)."""
        plan = self.plan

        def one(k, before_sampling=None):
            return derive_posteriors_batch(self.lightcurve.times, out["rates"], out["dy"], self.kernels[k],
                                           walkers=plan.sim_walkers, max_steps=sim_steps, fit=True, seed=fit_seeds[k],
                                           device=self.device, store_chain=False, quiet=True, own_engine=plan.own_engine[k],
                                           index_base=plan.fit_index_base, total_lightcurves=plan.total_lightcurves,
                                           before_sampling=before_sampling)

        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            if plan.refits_meet:
                fits, pair_stats = _refit_side_by_side(one, plan.paired, self.device)
                timer.mark("refit_null")          # the two refits' common wall time
                timer.mark("refit_alt", 0.0)
                return fits, pair_stats
            fits = [None, None]
            for k in (0, 1):
                if k in plan.models:
                    fits[k] = one(k)
                timer.mark(("refit_null", "refit_alt")[k])
            return fits, None

    def gather(self, fits, out, failure):
        """-> [max lnL of the null refits [nsims], of the alternative's]: the only exchange of the loop, one all-gather per
        model (plan.counts).  A rank whose simulation or refits failed says so first (``failure``)."""
        plan = self.plan
        best = [np.empty(0) if f is None else f.max_loglikelihood for f in fits]
        if not plan.sharded:
            return best
        from .distributed import all_gather_rows
        _raise_together(plan, failure, "the refits", self.group)
        if plan.split == "models":
            # the null rank and the alternative rank of a block pair lnL values of what must be the same light curves,
            # simulated on two GPUs: a checksum per rank says so, or the test stops here (a block without light curves
            # -- fewer of them than pairs of ranks -- has nothing to compare)
            half, bounds = plan.world // 2, plan.bounds
            mine = np.array([float(np.sum(out["rates"])) + float(np.sum(out["dy"])) if out is not None else 0.0])
            sums = all_gather_rows(mine, np.ones(plan.world, dtype=int), self.group)
            for b in range(half):
                if bounds[b + 1] > bounds[b] and sums[b] != sums[b + half]:
                    raise RuntimeError("ranks %d and %d simulated different light curves for block %d (checksums %r, %r)"
                                       % (b, b + half, b, sums[b], sums[b + half]))
        return [all_gather_rows(best[k], plan.counts[k], self.group) for k in (0, 1)]


def derive_posteriors_sharded(times, Y, DY, kernel, group=None, device=None, **kwargs):
    """:func:`derive_posteriors_batch` with the light curves sharded over the ranks of a
    ``torch.distributed`` job (one process per GPU; BASELINE configs[3]: 2000 simulated light
    curves over the 8 GPUs of a node).

    Every rank calls this with the SAME ``Y, DY`` [L, N]; rank r fits only its contiguous block
    of light curves (``distributed.LightcurveShard``) on its own GPU -- the ensembles are
    independent, so nothing is exchanged while sampling -- and ONE all-gather of
    ``max_loglikelihood`` (8 bytes per light curve, RCCL over xGMI) gives every rank the full
    vector for the LRT.  Returns (max_loglikelihood[L], local BatchPosteriors, shard).
    ``kwargs`` go to derive_posteriors_batch; a ``seed`` is offset by the rank.
    """
    from .distributed import LightcurveShard
    Y = np.atleast_2d(np.asarray(Y, dtype=np.float64))
    DY = np.atleast_2d(np.asarray(DY, dtype=np.float64))
    shard = LightcurveShard(Y.shape[0], group=group)
    if kwargs.get("seed") is not None:
        kwargs["seed"] = int(kwargs["seed"]) + BLOCK_SEED_STRIDE * shard.rank
    local = None
    best = np.empty(0)
    if len(shard):
        local = derive_posteriors_batch(times, Y[shard.lo:shard.hi], DY[shard.lo:shard.hi], kernel, **kwargs)
        best = local.max_loglikelihood
    return shard.gather(best, device=device), local, shard
