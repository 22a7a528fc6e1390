"""The profile means -- MTG_MEAN_SINE, MTG_MEAN_TWOSINE, MTG_MEAN_GAUSSIAN -- on the device: the one-lane sweep of
csrc/mtg_kernels_mean.hip against tests/golden/mean_profile_golden.npz (made on the CPU by
tests/golden/make_mean_profile_golden.py: mpmath means, dense mpmath / quad likelihoods).

Per fixture row, |lnL - truth| <= bound with
    bound = max(10 |c64 - T|, 64 sqrt(N) u S)                           the likelihood bound of test_accuracy_vs_quad_gpu.py
          + w1 (4 delta_np + 4 u max|mean| + u max|r|)                  first order in the mean's error, w1 = |K^-1 r|_1
delta_np being the error of numpy's float64 evaluation of the reference's formula: the device may be four times as far
off as numpy (it orders frequency t + phase differently), plus the truth's rounded residual.  No row is left out.

Largest measured error / bound over the fixture on an MI355X: 0.0436 (j2r/kind3/n3, the two sines on an over-damped
SHO at N = 3); the batches of 67 and 5 rows stay below 0.007.
"""
import json
import os
import warnings

import numpy as np
import pytest

from mind_the_gaps_amd import engine as _engine
from oracle import dense

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
U = 2.0 ** -53
GOLD = np.load(os.path.join(HERE, "golden", "mean_profile_golden.npz"))
CASES = json.loads(str(GOLD["cases"]))
NAMES = {_engine.MEAN_SINE: "MTG_MEAN_SINE", _engine.MEAN_TWOSINE: "MTG_MEAN_TWOSINE", _engine.MEAN_GAUSSIAN: "MTG_MEAN_GAUSSIAN"}


def arr(i, key):
    return GOLD["c%d_%s" % (i, key)]


def index(name):
    return next(i for i, c in enumerate(CASES) if c["name"] == name)


def like_bound(i, b):
    N = arr(i, "y").shape[1]
    return max(10.0 * abs(arr(i, "c64")[b] - arr(i, "lnL")[b]), 64.0 * np.sqrt(N) * U * arr(i, "S")[b])


def bound(i, b):
    return like_bound(i, b) + arr(i, "w1")[b] * (4.0 * arr(i, "delta_np")[b] + 4.0 * U * arr(i, "max_mean")[b]
                                                  + U * arr(i, "max_r")[b])


def setup(engine, i, lo=None, hi=None):
    """the case's light curves and model bound; -> (theta [B][P], lc [B])"""
    c, full = CASES[i], arr(i, "full")
    free = np.asarray(c["free"], dtype=np.int32)
    engine.set_lightcurves(arr(i, "t"), arr(i, "y"), arr(i, "dy") + 1e-12)
    bounds = np.tile([-np.inf, np.inf], (full.shape[1], 1))
    if lo is not None:
        bounds[:, 0], bounds[:, 1] = lo, hi
    engine.set_model(c["kinds"], full[0], free, bounds, mean_kind=c["mean_kind"])
    return np.ascontiguousarray(full[:, free]), arr(i, "lc")


@pytest.fixture()
def eng(engine):
    yield engine
    engine.set_time_parallel(2)
    engine.set_pipeline(2)
    engine.set_sort(2)
    engine.set_window_bytes(2 ** 32 - 1)


def test_every_fixture_row_within_the_bound(eng):
    worst, where = 0.0, None
    for i, c in enumerate(CASES):
        theta, lc = setup(eng, i)
        out, st = eng.loglike(theta, lc, add_prior=True)
        assert "mean_kernel" in eng.last_solver, "%s: dispatched to %s" % (c["name"], eng.last_solver)
        assert np.all(st == _engine.ST_OK), "%s: statuses %s" % (c["name"], st)
        for b in range(len(out)):
            e, tol = abs(out[b] - arr(i, "lnL")[b]), bound(i, b)
            print("%-28s row %2d  |lnL - T| %.3e  bound %.3e  ratio %.3g" % (c["name"], b, e, tol, e / tol))
            if e / tol > worst:
                worst, where = e / tol, "%s row %d" % (c["name"], b)
            assert e <= tol, "%s row %d: |lnL - T| = %.3e > %.3e" % (c["name"], b, e, tol)
    print("\nmean profile: worst error / bound %.3g (%s)" % (worst, where))


def test_libm_variant_row_is_in_the_fixture():
    i = index("j5/libm")
    t, full = arr(i, "t"), arr(i, "full")
    assert np.exp(full[0, 7]) * np.max(np.diff(t)) > 1.0e12 > np.exp(full[1, 7]) * np.max(np.diff(t))


def test_same_row_any_batch(eng):
    """a row's bits: alone, in the batch of 67 (both sides of Q = 1/2, two light curves), under every sort and
    time-parallel mode, and through the left-over launch of a window that reaches one light curve only"""
    i = index("batch/sho_mixed_b67")
    theta, lc = setup(eng, i)
    eng.set_time_parallel(0)
    ref, st = eng.loglike(theta, lc, add_prior=True)
    assert np.all(st == 0)
    for b in (0, 1, 17, 66):
        one, _ = eng.loglike(theta[b:b + 1], lc[b:b + 1], add_prior=True)
        assert one[0] == ref[b], "row %d alone" % b
    for sort in (0, 1):
        for tp in (0, 1, 2):
            eng.set_sort(sort)
            eng.set_time_parallel(tp)
            out, _ = eng.loglike(theta, lc, add_prior=True)
            assert "mean_kernel" in eng.last_solver, eng.last_solver
            assert np.array_equal(out, ref), "sort %d, time-parallel %d" % (sort, tp)
    eng.set_sort(0)
    eng.set_window_bytes(arr(i, "y").shape[1] * 16)      # rows on light curve 1 of a wave that starts on 0: left over
    out, _ = eng.loglike(theta, lc, add_prior=True)
    assert np.array_equal(out, ref), "left-over launch"


@pytest.mark.parametrize("kind", [_engine.MEAN_SINE, _engine.MEAN_GAUSSIAN])
def test_zero_amplitude_is_the_constant_mean(eng, kind):
    i = index("j5/kind%d/n65" % kind)
    c, full = CASES[i], arr(i, "full")[0].copy()
    nk = c["nk"]
    level = 3.05
    mean = [level, 0.0, full[nk + 2], full[nk + 3]] if kind == _engine.MEAN_SINE else [full[nk], full[nk + 1], 0.0, level]
    eng.set_lightcurves(arr(i, "t"), arr(i, "y"), arr(i, "dy") + 1e-12)
    v = np.concatenate([full[:nk], mean])
    eng.set_model(c["kinds"], v, np.arange(len(v), dtype=np.int32), np.tile([-np.inf, np.inf], (len(v), 1)), mean_kind=kind)
    got, st = eng.loglike(v[None, :], add_prior=False)
    w = np.concatenate([full[:nk], [level]])
    eng.set_model(c["kinds"], w, np.arange(len(w), dtype=np.int32), np.tile([-np.inf, np.inf], (len(w), 1)))
    eng.set_time_parallel(0)
    want, st2 = eng.loglike(w[None, :], add_prior=False)
    assert st[0] == 0 and st2[0] == 0
    # |lnL| <= S: no wider than the likelihood's floor 64 sqrt(N) u S
    assert abs(got[0] - want[0]) <= 64.0 * np.sqrt(65) * U * abs(want[0])


def test_coefficient_entry_agrees(eng):
    for name in ("j1/kind2/n65", "j5/kind3/n65", "j6/kind4/n64", "j0/kind4/n3", "batch/drw_b5"):
        i = index(name)
        c, full = CASES[i], arr(i, "full")
        theta, lc = setup(eng, i)
        want, _ = eng.loglike(theta, lc, add_prior=False)
        co = [dense.build_coeffs(c["kinds"], f[:c["nk"]]) for f in full]
        cols = [np.array([np.atleast_1d(k[j]) for k in co]).reshape(len(full), -1) for j in range(6)]
        got, st = eng.loglike_coeffs(*cols, jitter=np.array([k[6] for k in co]), mean_kind=c["mean_kind"],
                                     mean_params=full[:, c["nk"]:], lc_index=lc)
        assert "mean_kernel" in eng.last_solver and np.all(st == 0)
        for b in range(len(full)):
            assert abs(got[b] - want[b]) <= like_bound(i, b), "%s row %d: %.3e" % (name, b, abs(got[b] - want[b]))


def test_statuses(eng):
    i = index("j5/kind4/n65")
    c, full = CASES[i], arr(i, "full")[0]
    nk, P = c["nk"], len(full)
    lo, hi = np.full(P, -np.inf), np.full(P, np.inf)
    lo[nk + 2], hi[nk + 2] = 0.0, 2.0 * abs(full[nk + 2])          # the Gaussian's amplitude
    theta, lc = setup(eng, i, lo, hi)
    rows = np.repeat(theta[:1], 3, axis=0)
    rows[1, nk + 2] = 3.0 * abs(full[nk + 2])                       # outside the box
    rows[2, nk + 1] = 0.0                                           # sigma = 0: the mean is not finite
    out, st = eng.loglike(rows, add_prior=True)
    assert list(st) == [_engine.ST_OK, _engine.ST_PRIOR, _engine.ST_NONFINITE] and out[1] == -np.inf and out[2] == -np.inf
    out, st = eng.loglike(rows[:2], add_prior=False)
    assert list(st) == [_engine.ST_OK, _engine.ST_OK] and np.all(np.isfinite(out))
    # a covariance that is not positive definite (ComplexTerm with b d > a c, no prior) under a sine mean
    v = np.concatenate([np.log([1.0, 50.0, 0.01, 1.0]), [3.0, 0.5, 0.3, 0.2]])
    eng.set_model([_engine.TERM_COMPLEX4], v, np.arange(8, dtype=np.int32), np.tile([-np.inf, np.inf], (8, 1)),
                  mean_kind=_engine.MEAN_SINE)
    out, st = eng.loglike(v[None, :], add_prior=False)
    assert st[0] == _engine.ST_NOTPD and out[0] == -np.inf


def sampler_problem(eng):
    i = index("j1/kind2/n65")
    theta, _ = setup(eng, i)
    rng = np.random.RandomState(5)
    return theta[0] + 1e-3 * rng.normal(size=(1, 16, theta.shape[1]))


def test_device_sampler(eng):
    start = sampler_problem(eng)
    eng.ensemble_init(start, seed=11)
    chain, lnp = eng.ensemble_run(20, store_chain=True)
    assert "mean_kernel" in eng.last_solver, eng.last_solver
    again, st = eng.loglike(chain.reshape(-1, chain.shape[-1]), add_prior=True)
    assert np.array_equal(np.where(st == 0, again, -np.inf), lnp.reshape(-1)), "lnp_chain is not mtg_loglike_batch's"
    eng.ensemble_init(start, seed=11)
    chain2, lnp2 = eng.ensemble_run(20, store_chain=True)
    assert np.array_equal(chain, chain2) and np.array_equal(lnp, lnp2)
    # ten steps, the state saved and put back, ten more
    eng.ensemble_init(start, seed=11)
    first, lfirst = eng.ensemble_run(10, store_chain=True)
    state = eng.ensemble_state()
    eng.ensemble_init(state["coords"], seed=11)
    eng.ensemble_restore(state["iteration"], log_prob=state["log_prob"], naccept=state["naccept"],
                         best_log_prob=state["best_log_prob"], best_coords=state["best_coords"])
    second, lsecond = eng.ensemble_run(10, store_chain=True)
    assert np.array_equal(np.concatenate([first, second]), chain) and np.array_equal(np.concatenate([lfirst, lsecond]), lnp)


def test_refusals_name_the_mean_kind(eng):
    for kind in NAMES:
        i = index("j1/kind%d/n3" % kind)
        theta, _ = setup(eng, i)
        for call in (lambda: eng.predict(theta), lambda: eng.predict_at(theta, np.array([51.0, 52.5])),
                     lambda: eng.gp_draw(theta, seed=1), lambda: eng.loglike_grad(theta)):
            with pytest.raises(_engine.EngineError) as err:
                call()
            assert err.value.code == _engine.E_UNSUPPORTED and NAMES[kind] in str(err.value), str(err.value)


def python_problem(N):
    from mind_the_gaps_amd.models import DampedRandomWalk, SineModel
    i = index("j1/kind2/n%d" % N)
    full = arr(i, "full")[0]
    kernel = DampedRandomWalk(log_S0=full[0], log_omega0=full[1], bounds=[(-10, 10), (-10, 10)])
    mean = SineModel(*full[2:], bounds=[(0.0, 6.0), (0.0, 5.0), (0.5 * full[4], 2.0 * full[4]), (-4.0, 4.0)])
    return i, kernel, mean


def test_python_gp(eng):
    from mind_the_gaps_amd.gp import GP
    i, kernel, mean = python_problem(65)
    t, y, dy = arr(i, "t"), arr(i, "y")[0], arr(i, "dy")[0]
    gp = GP(kernel, mean=mean, fit_mean=True)
    gp.compute(t, dy + 1e-12)
    assert abs(gp.log_likelihood(y) - arr(i, "lnL")[0]) <= bound(i, 0)
    with pytest.raises(NotImplementedError, match="SineModel"):
        gp.grad_log_likelihood(y)
    zero = GP(kernel, mean=0.0)
    zero.compute(t, dy + 1e-12)
    r, ts = y - mean.get_value(t), np.linspace(t[0] - 1.0, t[-1] + 1.0, 23)
    for got, want in ((gp.predict(y, return_var=True), zero.predict(r, return_var=True)),
                      (gp.predict(y, t=ts, return_var=True), zero.predict(r, t=ts, return_var=True))):
        add = mean.get_value(t if len(got[0]) == len(t) else ts)
        np.testing.assert_allclose(got[0], want[0] + add, rtol=1e-12, atol=0)
        np.testing.assert_allclose(got[1], want[1], rtol=1e-12, atol=0)
    np.testing.assert_allclose(gp.sample(seed=3), zero.sample(seed=3) + mean.get_value(t), rtol=1e-12, atol=0)


def test_python_gpmodelling(eng):
    from mind_the_gaps_amd.device_sampler import DeviceEnsembleSampler
    from mind_the_gaps_amd.gpmodelling import GPModelling
    from mind_the_gaps_amd.lightcurves import GappyLightcurve
    i, kernel, mean = python_problem(129)
    lc = GappyLightcurve(arr(i, "t"), arr(i, "y")[0], arr(i, "dy")[0])
    np.random.seed(4)
    model = GPModelling(lc, kernel, meanmodel=mean)
    with pytest.warns(UserWarning, match="SineModel"):
        solution = model.fit(gradient="analytic")
    assert np.isfinite(solution.fun) and len(solution.x) == 6
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model.derive_posteriors(walkers=16, max_steps=40, convergence_steps=20, progress=False)
    assert isinstance(model._sampler, DeviceEnsembleSampler)
    assert np.all(np.isfinite(model.standarized_residuals()))
    # the model curve at new times, for the current vector: GP.predict's, through the zero-mean binding
    ts = np.linspace(arr(i, "t")[0], arr(i, "t")[-1], 17)
    mu, var = model.predict_at(ts, parameters=model.gp.get_parameter_vector())
    want = model.gp.predict(lc.y, t=ts, return_var=True)
    assert np.array_equal(mu, want[0]) and np.array_equal(var, want[1]) and np.all(np.isfinite(mu))
