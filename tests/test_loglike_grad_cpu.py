"""CPU tests of the analytic gradient (mtg_loglike_grad): the float64 replay tests/loglike_grad_replay.py against the
quad-precision truth, the coefficient tangents against differences of oracle.dense.build_coeffs, and the host-side
hooks (ppp.batched_minimize's value_and_grad, GPModelling.fit's gradient).

Truth: central differences of oracle.quad.loglike with a step of 1e-10, its two parts differenced separately (both
error terms of that difference are below 1e-15 relative).  Bound: C sqrt(N) u G_p with the C = 1024 of
tests/test_loglike_grad_gpu.py (where it is derived) and G_p the replay's error scale.

Which frame.  The replay carries the tangents either plainly (frame="elapsed": U' and V' with the elapsed time
t_n - t_0 as a factor) or in the frame rotated per step (frame="rotated").  Worst |g - T| / (sqrt(N) u G_p) over the
models below, measured here:

    N = 65     elapsed 271   rotated 123  (bpl+matern32; without it 171 against 3.6)
    N = 1000   elapsed 59.6  rotated 12.4 (bpl+matern32; without it 59.6 against 1.07)

The elapsed-time terms decide the plain form's error (they cancel down to lags inside each sample's contribution), so
the rotated form is the one the device carries; test_rotated_frame_is_the_more_accurate keeps that on record.  What is
left in the rotated form is the Matern-3/2 term's own conditioning (b / a = 1 / eps: the pivot's rounding, as in
tests/gp_draw_replay.py)."""
import numpy as np
import pytest

import loglike_grad_cases as cases
import loglike_grad_replay as replay
from mind_the_gaps_amd import engine, ppp
from mind_the_gaps_amd import synthetic as synth
from oracle import dense
from oracle.dense import (K_BPL, K_COMPLEX3, K_COMPLEX4, K_COSINUS, K_DRW, K_JITTER, K_LORENTZIAN, K_MATERN32, K_REAL,
                          K_SHO)

U = 2.0 ** -53
C = 1024

# name -> (kinds, kernel parameters, mean_kind)
MODELS = {
    "drw": ([K_DRW], [4.0, -1.0], 0),
    "sho_under": ([K_SHO], [2.0, 1.0, 0.5], 0),
    "sho_over": ([K_SHO], [2.0, -1.5, 0.5], 0),
    "drw+sho+lorentzian": ([K_DRW, K_SHO, K_LORENTZIAN], [4.6, -0.9, 3.2, 1.3, -0.1, 2.0, 1.5, 0.3], 0),
    "bpl+matern32": ([K_BPL, K_MATERN32], [3.0, 2.0, -0.5, 1.0, 1.5], 0),
    "complex4+real": ([K_COMPLEX4, K_REAL], [3.0, 1.0, -0.5, 0.2, 2.0, -1.0], 0),
    "cosinus+jitter+sho": ([K_COSINUS, K_JITTER, K_SHO], [1.0, 0.3, -0.5, 2.0, 0.8, 0.2], 0),
    "linear_mean": ([K_DRW, K_SHO], [4.0, -1.0, 2.0, 1.0, 0.5], 1),
    "white": ([K_JITTER], [0.3], 0),
}


@pytest.fixture(autouse=True)
def the_kernel_the_replay_mirrors_exists():
    assert "mtg_loglike_grad" in engine.EXPORTS and hasattr(engine.Engine, "loglike_grad")


def problem(name, N):
    kinds, th, mean_kind = MODELS[name]
    t, y, dy = synth.make_lightcurves(N, 1, seed=5)
    full = np.array(th + ([1e-3, 0.1] if mean_kind == 1 else [0.05]))
    return t, y[0] - y[0].mean(), dy[0], kinds, full, np.arange(len(full)), mean_kind


@pytest.mark.parametrize("N", [1, 2, 3, 65, 1000])
@pytest.mark.parametrize("name", sorted(MODELS))
def test_replay_against_quad_truth(name, N):
    t, y, dy, kinds, full, free, mean_kind = problem(name, N)
    T = replay.quad_gradient(t, y, dy, kinds, full, free, mean_kind)
    lnl, g, G, status = replay.loglike_grad(t, y, dy, kinds, full, free, mean_kind)
    assert status == 0
    from oracle import quad
    hi, _, S, _ = quad.loglike(t, y, dy, kinds, full[None, :], mean_kind=mean_kind)
    assert abs(lnl - hi[0]) <= 64 * np.sqrt(N) * U * S[0]
    err, bound = np.abs(g - T), C * np.sqrt(N) * U * G
    print(name, N, "worst ratio %.3g" % np.max(err / np.where(G > 0, np.sqrt(N) * U * G, np.inf)))
    assert np.all(err <= bound), (err, bound)


def test_a_frozen_parameter_leaves_the_others_alone():
    t, y, dy, kinds, full, free, mean_kind = problem("drw+sho+lorentzian", 65)
    _, g, G, _ = replay.loglike_grad(t, y, dy, kinds, full, free, mean_kind)
    keep = np.array([0, 2, 3, 6, 8])                     # non-contiguous
    _, gk, Gk, _ = replay.loglike_grad(t, y, dy, kinds, full, keep, mean_kind)
    assert np.array_equal(gk, g[keep]) and np.array_equal(Gk, G[keep])


def test_rotated_frame_is_the_more_accurate():
    """the measurement behind the choice of the rotated frame (module docstring), at N = 1000"""
    worst = {"elapsed": 0.0, "rotated": 0.0}
    for name in ("sho_under", "drw+sho+lorentzian", "complex4+real", "cosinus+jitter+sho"):
        t, y, dy, kinds, full, free, mean_kind = problem(name, 1000)
        T = replay.quad_gradient(t, y, dy, kinds, full, free, mean_kind)
        for frame in worst:
            _, g, G, _ = replay.loglike_grad(t, y, dy, kinds, full, free, mean_kind, frame=frame)
            worst[frame] = max(worst[frame], np.max(np.abs(g - T) / (np.sqrt(1000) * U * G)))
    print(worst)
    assert worst["rotated"] < worst["elapsed"] / 4


TANGENT_CASES = {
    "real": ([K_REAL], [0.7, -0.4]),
    "complex3": ([K_COMPLEX3], [0.7, -0.4, 0.9]),
    "complex4": ([K_COMPLEX4], [0.7, -0.2, -0.4, 0.3]),
    "sho_under": ([K_SHO], [0.5, 0.4, -0.3]),
    "sho_over": ([K_SHO], [0.5, -1.1, -0.3]),
    "matern32": ([K_MATERN32], [0.3, 1.2]),
    "jitter": ([K_JITTER], [-0.6]),
    "drw": ([K_DRW], [0.7, -0.4]),
    "lorentzian": ([K_LORENTZIAN], [0.7, 1.1, 0.2]),
    "cosinus": ([K_COSINUS], [0.7, 0.2]),
    "bpl": ([K_BPL], [0.9, 0.1, -0.5]),
    "all": ([K_DRW, K_SHO, K_LORENTZIAN, K_SHO, K_MATERN32, K_JITTER, K_BPL, K_REAL, K_COSINUS, K_COMPLEX3, K_COMPLEX4, K_JITTER],
            [0.7, -0.4, 0.5, 0.4, -0.3, 0.7, 1.1, 0.2, 0.5, -1.1, -0.3, 0.3, 1.2, -0.6, 0.9, 0.1, -0.5, 0.2, 0.1, 0.7, 0.2,
             0.7, -0.4, 0.9, 0.7, -0.2, -0.4, 0.3, -1.0]),
}


def dense_slots(kinds, params):
    """oracle.dense.build_coeffs in the device's slot order: without the empty real term of a Lorentzian"""
    ar, cr, ac, bc, cc, dc, jit = dense.build_coeffs(kinds, params)
    keep, i, off = [], 0, 0
    for kind in kinds:
        if kind in (K_REAL, K_DRW):
            keep.append(i); i += 1
        elif kind == K_LORENTZIAN:
            i += 1
        elif kind == K_SHO and np.exp(params[off + 1]) < 0.5:
            keep += [i, i + 1]; i += 2
        off += dense.NPARAMS[kind]
    return ar[keep], cr[keep], ac, bc, cc, dc, jit


@pytest.mark.parametrize("mean_kind", [0, 1])
@pytest.mark.parametrize("name", sorted(TANGENT_CASES))
def test_coefficient_tangents_against_central_differences(name, mean_kind):
    kinds, th = TANGENT_CASES[name]
    th = np.asarray(th, dtype=np.float64)
    full = np.concatenate([th, [0.3, -2.0] if mean_kind == 1 else [1.5]])
    coef, dcoef = replay.coefficients(kinds, full, mean_kind)
    for got, want in zip(replay.as_dense(coef), dense_slots(kinds, th)):
        assert np.allclose(got, want, rtol=4 * U, atol=0)
    h = 1e-5
    for k in range(len(th)):
        up, dn = th.copy(), th.copy()
        up[k] += h
        dn[k] -= h
        cu, cd = dense_slots(kinds, up), dense_slots(kinds, dn)
        for key, vu, vd, v in zip(replay.KEYS + ("jit",), cu, cd, replay.as_dense(coef)):
            fd = (np.asarray(vu) - np.asarray(vd)) / (up[k] - dn[k])
            d = dcoef[key][k]
            assert np.all(np.abs(d - fd) <= 1e-7 * np.maximum(np.abs(v), np.abs(d))), (name, key, k, d, fd)
        fd_asum = ((np.sum(cu[0]) + np.sum(cu[2]) + cu[6]) - (np.sum(cd[0]) + np.sum(cd[2]) + cd[6])) / (up[k] - dn[k])
        assert abs(dcoef["asum"][k] - fd_asum) <= 1e-7 * max(abs(coef["asum"]), abs(dcoef["asum"][k]))
        assert dcoef["slope"][k] == 0.0 and dcoef["icpt"][k] == 0.0
    # the mean's own parameters: mean(t) = slope t + icpt, a constant mean is the intercept
    nk = len(th)
    for key in replay.KEYS + ("jit", "asum"):
        assert not np.any(dcoef[key][nk:])
    if mean_kind == 1:
        assert (coef["slope"], coef["icpt"]) == (0.3, -2.0)
        assert np.array_equal(dcoef["slope"][nk:], [1.0, 0.0]) and np.array_equal(dcoef["icpt"][nk:], [0.0, 1.0])
    else:
        assert (coef["slope"], coef["icpt"]) == (0.0, 1.5)
        assert np.array_equal(dcoef["slope"][nk:], [0.0]) and np.array_equal(dcoef["icpt"][nk:], [1.0])


def test_fixture_groups_leave_the_forward_differences_no_room():
    """the rows of tests/test_loglike_grad_gpu.py's fixture test, with the oracle alone: on every chosen row the rounding of lnL in a forward difference of step 1e-8,
    u |lnL| / 1e-8, is beyond the analytic bound of at least one component -- none is exempt by construction"""
    for name in cases.FIXTURE_GROUPS:
        case = cases.fixture(name)
        lnl, _ = case.lnl_truth
        common = case.regime == ""
        assert (U * np.abs(lnl)[:, None] / 1e-8 > 100 * case.bound(C))[common].any(axis=1).all(), name


def test_batched_minimize_takes_a_gradient_callable():
    """a quadratic toy problem: the hook reaches the minimum the forward differences reach, and ``fun`` then serves
    the line search alone -- it never sees the L (P + 1) rows of a finite-difference batch"""
    L, P = 6, 4
    rng = np.random.default_rng(3)
    centre = rng.uniform(-1.0, 1.0, (L, P))
    weight = rng.uniform(0.5, 3.0, (L, P))
    lower, upper = np.full(P, -0.5), np.full(P, 2.0)          # some minima lie on the box
    calls = []

    def fun(x, lc):
        calls.append(len(x))
        return np.sum(weight[lc] * (x - centre[lc]) ** 2, axis=1)

    def value_and_grad(x):
        assert x.shape == (L, P)
        return np.sum(weight * (x - centre) ** 2, axis=1), 2.0 * weight * (x - centre)

    x0 = np.zeros((L, P))
    x_fd, f_fd, _ = ppp.batched_minimize(fun, x0, lower, upper)
    assert L * (P + 1) in calls
    calls.clear()
    x_an, f_an, _ = ppp.batched_minimize(fun, x0, lower, upper, value_and_grad=value_and_grad)
    assert calls and L * (P + 1) not in calls
    best = np.clip(centre, lower, upper)
    assert np.allclose(x_an, best, atol=1e-5) and np.allclose(x_fd, best, atol=1e-4)
    assert np.allclose(f_an, f_fd, atol=1e-8) and np.all(f_an <= f_fd + 1e-12)


def test_fit_rejects_an_unknown_gradient():
    from mind_the_gaps_amd.gpmodelling import GPModelling
    from mind_the_gaps_amd.lightcurves import GappyLightcurve
    from mind_the_gaps_amd.models import DampedRandomWalk
    t = np.arange(50.0)
    g = GPModelling(GappyLightcurve(t, np.sin(t), np.full(50, 0.1)), DampedRandomWalk(0.0, 0.0, bounds=[(-5, 5), (-5, 5)]))
    for bad in ("numeric", "FD", None):
        with pytest.raises(ValueError):
            g.fit(gradient=bad)
    with pytest.raises(ValueError):
        ppp.derive_posteriors_batch(t, np.sin(t)[None], np.full((1, 50), 0.1), DampedRandomWalk(0.0, 0.0, bounds=[(-5, 5), (-5, 5)]),
                                    fit_gradient="numeric")
