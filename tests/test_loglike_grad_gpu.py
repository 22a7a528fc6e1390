"""Engine.loglike_grad / GP.grad_log_likelihood / GPModelling.fit(gradient="analytic") (mtg_loglike_grad_kernel: one
lane per row and free parameter carries the factorisation and its tangent) on the device.

Truth for gradients: T = central differences of the quad-precision oracle (oracle.quad.loglike, step 1e-10, its two
parts differenced separately: both error terms below 1e-15 relative).  Error scale per component, from the float64
replay tests/loglike_grad_replay.py: G_p = 1/2 sum_n (|2 z z'/D| + |z^2 D'/D^2| + |D'/D|), a scale, never an expected
value.  u = 2^-53.

Tolerance C.  The worst |g_replay - T| / (sqrt(N) u G_p) over the rows of tests 1 and 3 below (the replay is the
float64 formulation, the quad oracle the reference; ``python tests/loglike_grad_cases.py`` prints it).  Test 3 runs
EVERY group of the fixture with J <= 6 and N <= 1e4, 18 groups.  Over all their rows the replay's worst ratio is
2.2e12, so one constant for all of them would say nothing.  The rows fall into four regimes by a rule on the row
(tests/loglike_grad_cases.py, where each rule and its reason are written down), measured worst replay ratio:

    common        all others (122 fixture rows, every row of test 1)               70.96   (typical/alt_n65)
    critical      an SHO term within 1e-3 of Q = 1/2 in ln Q (12 rows, signatures)   1.68e4
    long_memory   the group long_memory, a / sigma^2 to e^20, c dx to 1e-9 (6 rows)  1.04e6
    phase         phase/j3 beyond 1e4 rad per step (5 rows)                          2.2e12

C = 8 x 70.96 = 568, rounded up to a power of two: C = 1024 for the common rows; the smallest shapes reach 55.7 (a
fitted line at N = 2: y - mean cancels), bpl+matern32 42.8 (b / a = 1 / eps).  The factor 8 covers the device's
exp / sincos differing from numpy's by a few ulp per sample.  "critical" and "long_memory" rows are NOT within C: the
float64 formulation, which is also the device's, loses 1e7 u and 1e10 u there (relative errors of 3e-9 and 2e-8 in a
gradient of 10 to 1e4).  They are held to constants derived in the same way from their own replay ratios, 2^18 and
2^23: the device may be no worse than its formulation, which is all a test can ask until the conditioning is mended
(it sits in the expansion near Q = 1/2 and in celerite's pivot for long memory; the likelihood shares both).  "phase"
rows have no gradient bound: the truth builds d in quad, a float64 d turns the phases by up to a radian, and no
float64 evaluation follows it; their status and finiteness are checked and their figures printed.  Measured on the
device: common 69.5, critical 3.2e4, long_memory 5.3e5, phase 2.2e12.  A bound is
C sqrt(N) u G_p plus the resolution of the truth itself, 1e-32 |lnL| / 1e-10 (components of 1e-20 and below: decays
that underflow, an amplitude of e^40 beside the other terms).  A device error beyond a bound where the replay is inside
is a finding about the kernel.

The replay and the kernel carry the tangents in the frame rotated per step (csrc/mtg_factor_step_tangent.h): the
plain form, with the elapsed time in U' and V', has a worst replay ratio of 59.6 at N = 1000 against 12.4 rotated, and
59.6 against 1.07 without the Matern-3/2 model (tests/test_loglike_grad_cpu.py)."""
import warnings

import numpy as np
import pytest

import loglike_grad_cases as cases
from mind_the_gaps_amd import engine as _engine
from mind_the_gaps_amd import synthetic as synth
from mind_the_gaps_amd import terms
from mind_the_gaps_amd.gpmodelling import GPModelling
from mind_the_gaps_amd.lightcurves import GappyLightcurve
from mind_the_gaps_amd.models import DampedRandomWalk
from oracle.dense import K_COMPLEX4, K_DRW, K_SHO

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
C = 1024
AMP, OTHER = (-10, 50), (-10, 10)


def check_case(engine, case):
    case.bind(engine)
    out, grad, status = engine.loglike_grad(case.theta, case.lc)
    J = sum({0: 1, 6: 1, 5: 0}.get(k, 2) for k in case.kinds)
    assert engine.last_solver == "mtg_loglike_grad_kernel<%d>" % J
    assert np.all(status == 0) and np.all(np.isfinite(out)) and np.all(np.isfinite(grad))
    ll, st = engine.loglike(case.theta, case.lc, add_prior=False)
    assert np.all(st == 0)
    _, S = case.lnl_truth
    # (on "phase" and "long_memory" rows the likelihood kernels are themselves held only to celerite's own error,
    # tests/test_accuracy_vs_quad_gpu.py: two of them need not agree to this; the figure is printed)
    followed = ~np.isin(case.regime, ("phase", "long_memory"))
    print(case.name, "lnL: worst |out - loglike| / (64 sqrt(N) u S) = %.3g" % np.max(np.abs(out - ll) / (64 * np.sqrt(case.N) * U * S)))
    assert np.all((np.abs(out - ll) <= 64 * np.sqrt(case.N) * U * S)[followed])
    g_replay = case.replayed[1]
    for regime in sorted(set(case.regime)):
        rows = case.regime == regime
        print(case.name, regime or "common", "gradient: worst |g - T| / (sqrt(N) u G) = %.3g, replay %.3g"
              % (np.max(cases.ratios(case, grad)[rows]), cases.replay_ratio(case, regime)))
        if regime == "phase":
            continue
        bound = case.bound(C if regime == "" else cases.REGIME_C[regime])[rows]
        assert np.all(np.abs(grad - case.truth)[rows] <= bound)
        assert np.all(np.abs(grad - g_replay)[rows] <= bound)
    return out, grad


@pytest.mark.parametrize("N", cases.SMALL_N)
@pytest.mark.parametrize("name", sorted(cases.SMALL))
def test_smallest_shapes(engine, name, N):
    """ranks 0, 1, 2, 3 and 6; (B, P) = (5, 3) and (23, 7); two light curves through lc_index, a y_offset, two
    parameters frozen in the middle of the vector, SHO rows on both sides of Q = 1/2 in one batch"""
    case = cases.small(name, N)
    kinds, _, _, free_index, B = cases.SMALL[name]
    assert case.theta.shape == (B, len(free_index)) and set(case.lc) == {0, 1}
    if K_SHO in kinds:
        off = [sum(cases.NPARAMS[k] for k in kinds[:i]) + 1 for i, k in enumerate(kinds) if k == K_SHO]
        sides = np.exp(case.full_rows[:, off]) < 0.5
        assert sides.any() and (~sides).any() and len({tuple(r) for r in sides}) == min(B, 2 ** len(off))
    check_case(engine, case)


def test_statuses_and_their_neighbours(engine):
    """a row outside the box and a row whose covariance is not positive definite among good ones: their status, -inf
    and a gradient of NaN; the good rows' values are those of a batch without them, bit for bit.  (A kernel the prior
    accepts is positive definite, so the second kind of row needs a batch evaluated without the prior.)"""
    N = 65
    t, y, dy = synth.make_lightcurves(N, 2, seed=31)
    engine.set_lightcurves(t, y, dy + 1e-12, y_offset=y.mean(axis=1))
    full = np.array([0.0, -5.0, 0.0, 0.0, 1.0, -1.0, 0.0])
    bounds = np.array([(-10.0, 10.0)] * 6 + [(-np.inf, np.inf)])
    engine.set_model([K_COMPLEX4, K_DRW], full, np.arange(6, dtype=np.int32), bounds)
    rng = np.random.default_rng(4)
    good = full[None, :6] + 0.1 * rng.standard_normal((9, 6))
    lc = (np.arange(9) % 2).astype(np.int32)
    for add_prior, bad_row, want in ((True, np.array([0.0, -5.0, 11.0, 0.0, 1.0, -1.0]), _engine.ST_PRIOR),
                                     (False, np.concatenate([np.log([1.0, 50.0, 0.01, 1.0]), [-30.0, -1.0]]), _engine.ST_NOTPD)):
        ref_out, ref_grad, ref_st = engine.loglike_grad(good, lc, add_prior=add_prior)
        assert np.all(ref_st == 0) and np.all(np.isfinite(ref_grad))
        theta = np.insert(good, 4, bad_row, axis=0)
        out, grad, status = engine.loglike_grad(theta, np.insert(lc, 4, 1), add_prior=add_prior)
        assert status[4] == want and np.isneginf(out[4]) and np.all(np.isnan(grad[4]))
        keep = np.arange(10) != 4
        assert np.all(status[keep] == 0)
        assert np.array_equal(out[keep], ref_out) and np.array_equal(grad[keep], ref_grad)
        _, st = engine.loglike(theta, np.insert(lc, 4, 1), add_prior=add_prior)
        assert st[4] == want


class _FitStub:
    """what GPModelling._neg_log_like_and_grad reads of its object, bound to an engine that holds a fixture's model"""

    def __init__(self, engine, lc):
        self._fit_evaluations, self._quiet, self._y = 1, True, None
        self.gp = self
        self._engine, self._lc = engine, lc

    def log_probability_batch(self, pts, y, add_prior=True):
        return self._engine.loglike(pts, np.full(len(pts), self._lc, dtype=np.int32), add_prior=add_prior)


@pytest.mark.parametrize("name", cases.FIXTURE_GROUPS)
def test_fixture_rows(engine, name):
    """every row and component within C sqrt(N) u G_p of the quad truth; per row the analytic gradient's largest error
    at least 100 times smaller than that of GPModelling._neg_log_like_and_grad's forward differences (step 1e-8) on the
    same row.  The forward differences are off by about u |lnL| / 1e-8; a row where they happen to be within the
    analytic bound is exempt, at most one row in ten.  The comparison is made on the rows of the common tolerance; the
    figures of the others are printed"""
    case = cases.fixture(name)
    _, grad = check_case(engine, case)
    P = len(case.free_index)
    inf = np.full(P, np.inf)
    exempt, rows = 0, int((case.regime == "").sum())
    for b in range(len(case.lc)):
        f, fd = GPModelling._neg_log_like_and_grad(_FitStub(engine, case.lc[b]), case.theta[b], -inf, inf)
        assert np.isfinite(f)
        e_fd = np.abs(-fd - case.truth[b])
        e_an = np.abs(grad[b] - case.truth[b])
        print(name, b, case.regime[b] or "common", "largest error: analytic %.3g, forward differences %.3g" % (e_an.max(), e_fd.max()))
        if case.regime[b] != "":
            continue
        if np.all(e_fd <= case.bound(C)[b]):
            exempt += 1
            continue
        assert e_an.max() * 100 <= e_fd.max()
    assert exempt * 10 <= rows


def test_fit_with_the_analytic_gradient_ends_higher(engine):
    """the DRW + SHO case of test_gpmodelling_gpu.test_fit_improves_and_matches_oracle_at_optimum"""
    import loglike_grad_replay as replay
    N = 600
    t, y, dy = synth.make_lightcurves(N, 1, seed=12)
    y, dy = y[0], dy[0]
    th = synth.truth(synth.NULL_MODEL)

    def model():
        k = DampedRandomWalk(th[0], th[1], bounds=[AMP, OTHER]) + terms.SHOTerm(th[2], th[3], th[4], bounds=[AMP, OTHER, OTHER])
        return GPModelling(GappyLightcurve(t, y, dy), k)

    g_fd, g_an = model(), model()
    sol_fd = g_fd.fit()
    sol_an = g_an.fit(gradient="analytic")
    print("-lnL: fd %.12g (%d iterations), analytic %.12g (%d iterations)" % (sol_fd.fun, sol_fd.nit, sol_an.fun, sol_an.nit))
    assert sol_an.fun <= sol_fd.fun
    lo, hi = np.array(g_an.gp.get_parameter_bounds(), dtype=np.float64).T

    def projected(x):
        full = np.concatenate([x, [0.0]])
        grad = -replay.quad_gradient(t, y - np.mean(y), dy, synth.NULL_MODEL, full, np.arange(5))      # of -lnL
        blocked = ((x <= lo) & (grad > 0)) | ((x >= hi) & (grad < 0))
        return np.max(np.abs(np.where(blocked, 0.0, grad)))

    p_fd, p_an = projected(sol_fd.x), projected(sol_an.x)
    print("projected gradient in quad: fd %.3g, analytic %.3g" % (p_fd, p_an))
    assert p_an < p_fd
    g_an.gp.set_parameter_vector(sol_an.x)
    value, grad = g_an.gp.grad_log_likelihood(y)
    assert value == -sol_an.fun and np.array_equal(grad, -sol_an.jac)


def test_unsupported_rank_says_so_and_fit_falls_back(engine):
    """ranks 7 to 10 are not compiled (their tangent state needs scratch): MTG_E_UNSUPPORTED, and
    fit(gradient="analytic") warns and completes on forward differences"""
    N = 60
    t, y, dy = synth.make_lightcurves(N, 1, seed=3)
    kinds = [K_DRW, K_SHO, K_SHO, K_SHO]                          # rank 7
    full = np.array([1.0, -1.0, 1.0, 0.5, 0.5, 0.5, 1.0, -0.5, 0.0, 0.7, 1.2, 0.0])
    engine.set_lightcurves(t, y, dy + 1e-12, y_offset=y.mean(axis=1))
    engine.set_model(kinds, full, np.arange(11, dtype=np.int32), np.tile([-np.inf, np.inf], (12, 1)))
    with pytest.raises(_engine.EngineError) as info:
        engine.loglike_grad(full[None, :11])
    assert info.value.code == _engine.E_UNSUPPORTED
    k = DampedRandomWalk(1.0, -1.0, bounds=[AMP, OTHER])
    for i in range(3):
        k = k + terms.SHOTerm(1.0 - 0.3 * i, 0.5, 0.5 * i, bounds=[AMP, OTHER, OTHER])
    g = GPModelling(GappyLightcurve(t, y[0], dy[0]), k)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        sol = g.fit(gradient="analytic")
    assert any("finite differences" in str(w.message) for w in caught)
    assert np.isfinite(sol.fun) and sol.fun <= g._neg_log_like(g.initial_params)


def test_lock_step_fit_with_the_analytic_gradient(engine, monkeypatch):
    """ppp.derive_posteriors_batch(fit_gradient="analytic"): the starting fit of every light curve takes its gradients
    from Engine.loglike_grad (one launch of L rows, never the L (P + 1) rows of the differences) and ends where the
    finite-difference fit ends; a model of rank 7 warns and fits with finite differences"""
    from mind_the_gaps_amd import ppp
    t, y, dy = synth.make_lightcurves(80, 3, seed=17)
    th = synth.truth([K_DRW])

    def run(kernel, mode, walkers=4):
        calls = []
        real = _engine.Engine.loglike_grad
        monkeypatch.setattr(_engine.Engine, "loglike_grad", lambda self, theta, *a, **k: (calls.append(len(theta)), real(self, theta, *a, **k))[1])
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            res = ppp.derive_posteriors_batch(t, y, dy, kernel, walkers=walkers, max_steps=20, seed=5, fit_gradient=mode, store_chain=False)
        monkeypatch.setattr(_engine.Engine, "loglike_grad", real)
        return res, calls, [str(w.message) for w in caught]

    drw = lambda: DampedRandomWalk(th[0], th[1], bounds=[AMP, OTHER])
    fd, calls_fd, _ = run(drw(), "fd")
    an, calls_an, _ = run(drw(), "analytic")
    assert not calls_fd and calls_an and set(calls_an) == {3}
    print("fit lnL: fd", fd.fit_loglikelihood, "analytic", an.fit_loglikelihood)
    assert np.all(np.isfinite(an.fit_loglikelihood))
    # both stop at a projected gradient of 1e-5 (batched_minimize's gtol): the same top to well within 1e-6 in lnL
    assert np.all(np.abs(an.fit_loglikelihood - fd.fit_loglikelihood) <= 1e-6)
    k = drw()
    for i in range(3):
        k = k + terms.SHOTerm(1.0 - 0.3 * i, 0.5, 0.5 * i, bounds=[AMP, OTHER, OTHER])
    res, calls, messages = run(k, "analytic", walkers=24)
    assert any("finite differences" in m for m in messages)
    assert np.all(np.isfinite(res.fit_loglikelihood))
