"""Per-term conditional mean and variance at any times (mtg_predict_terms: mind_the_gaps_amd/csrc/mtg_predict_terms.hip)
against the 50-digit dense truth of tests/golden/predict_terms_golden.npz (tests/golden/make_predict_terms_golden.py).

The bound is the project's (tests/test_predict_vs_quad_gpu.py: bound), not fitted to a run: with T the truth, c64 the
dense expression in float64, s the cancellation scale and u = 2^-53, per (row, mask)

    |out - T| <= max(10 rho, 64 sqrt(N) u) s,   rho = worst |c64 - T| / s over the times,
    s_mu = [|mean|] + sum_n |k_c,*(n) (K^-1 r)_n|,   s_var = k_c(0) + |k_c,*^T K^-1 k_c,*|.

Also: all terms with MTG_TERMS_MEAN is mtg_predict_at bit for bit; a mask of 0 or of a jitter term gives 0; single-term
means add up to the all-terms mean; the two orderings of an over- and an under-damped SHO term give each term its own
component, alone and in one batch; every (row, time, mask) is bit for bit the same whatever B, M, T, the order of ts,
the order of the masks and the slab it travels in; argument errors; GP.predict(kernel=) and
GPModelling.predict_components.
"""
import json
import os

import numpy as np
import pytest

import test_predict_at_vs_quad_gpu as tpat
import test_predict_vs_quad_gpu as tq
from mind_the_gaps_amd import engine as _engine
from mind_the_gaps_amd import terms
from mind_the_gaps_amd.engine import MEAN_LINEAR, TERMS_MEAN
from mind_the_gaps_amd.gp import GP
from mind_the_gaps_amd.gpmodelling import GPModelling
from mind_the_gaps_amd.lightcurves import GappyLightcurve
from mind_the_gaps_amd.models import DampedRandomWalk, Lorentzian
from oracle import dense
from test_predict_vs_quad_gpu import bound, report

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
U = 2.0 ** -53
FIX = np.load(os.path.join(HERE, "golden", "predict_terms_golden.npz"))
GROUPS = {g["name"]: g for g in json.loads(bytes(FIX["manifest"]))["groups"]}


def arrays(name):
    return {k[len(name) + 1:]: FIX[k] for k in FIX.files if k.startswith(name + "/")}


def same(x, y):
    return np.array_equal(x, y, equal_nan=True)


def setup(engine, name):
    """binds the group's light curve and model -> (arrays, the free parameters [1][P]); a constant mean travels as the
    light curve's y_offset, frozen at 0 in the model"""
    g, a = GROUPS[name], arrays(name)
    nk = dense.n_kernel_params(g["kinds"])
    if g["mean_kind"] == 1:
        engine.set_lightcurves(a["t"], a["y"], a["yerr"])
        engine.set_model(g["kinds"], a["theta"], np.arange(nk + 2, dtype=np.int32), np.tile([-np.inf, np.inf], (nk + 2, 1)),
                         mean_kind=MEAN_LINEAR, extra=g["extra"])
        return a, a["theta"][None, :]
    engine.set_lightcurves(a["t"], a["y"], a["yerr"], y_offset=a["theta"][nk:])
    engine.set_model(g["kinds"], np.concatenate([a["theta"][:nk], [0.0]]), np.arange(nk, dtype=np.int32),
                     np.tile([-np.inf, np.inf], (nk + 1, 1)), extra=g["extra"])
    return a, a["theta"][None, :nk]


def full_mask(name):
    return (1 << len(GROUPS[name]["kinds"])) - 1


@pytest.mark.parametrize("name", list(GROUPS))
def test_components_against_the_dense_truth(engine, name):
    """every mask of the fixture at its 48 times, without and with the mean: mu and var within the bound, status 0"""
    a, theta = setup(engine, name)
    N = len(a["t"])
    worst, failures = {}, []
    for flag, label in ((0, ""), (TERMS_MEAN, " + mean")):
        mu, var, status = engine.predict_terms(theta, a["masks"] | np.uint32(flag), a["ts"])
        assert status[0] == 0 and "mtg_predict_terms_eval_kernel<" in engine.last_solver
        truth = a["mu"] + (a["mean_ts"] if flag else 0.0)
        scale = a["mu_scale"] + (np.abs(a["mean_ts"]) if flag else 0.0)
        for v, out, T, s in (("mu", mu[0], truth, scale), ("var", var[0], a["var"], a["var_scale"])):
            try:
                worst["%s %s%s" % (name, v, label)] = bound("predict_terms %s%s / %s" % (v, label, name), N, out, T,
                                                            a[v + "_c64err"], s)
            except AssertionError as exc:
                failures.append(str(exc))
    report("predict_terms", worst)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("name", list(GROUPS))
def test_all_terms_is_predict_at_bit_for_bit(engine, name):
    a, theta = setup(engine, name)
    full = full_mask(name)
    m0, v0, s0 = engine.predict_at(theta, a["ts"])
    mu, var, status = engine.predict_terms(theta, [full | TERMS_MEAN, full, 0, TERMS_MEAN], a["ts"])
    assert status[0] == 0 and s0[0] == 0
    assert same(mu[:, 0], m0) and same(var[:, 0], v0), "all terms + mean differs from mtg_predict_at"
    assert same(var[:, 1], v0), "all terms without the mean: the variance differs from mtg_predict_at"
    only, none, st = engine.predict_terms(theta, [full | TERMS_MEAN], a["ts"], return_var=False)
    assert none is None and same(only[:, 0], m0)
    # nothing selected: the mean or 0, and no variance
    assert np.all(mu[:, 2] == 0.0) and np.all(var[:, 2] == 0.0) and np.all(var[:, 3] == 0.0)
    assert same(mu[0, 3], a["mean_ts"]) if GROUPS[name]["mean_kind"] == 1 else np.all(mu[:, 3] == 0.0)


def test_a_jitter_term_contributes_nothing(engine):
    a, theta = setup(engine, "matern_jitter_real")
    assert GROUPS["matern_jitter_real"]["kinds"][1] == dense.K_JITTER
    mu, var, status = engine.predict_terms(theta, [2, 1, 3], a["ts"])
    assert status[0] == 0 and np.all(mu[0, 0] == 0.0) and np.all(var[0, 0] == 0.0)
    assert same(mu[0, 1], mu[0, 2]) and same(var[0, 1], var[0, 2])        # Matern32 with and without the jitter term


@pytest.mark.parametrize("name", list(GROUPS))
def test_single_term_means_add_up(engine, name):
    """mu is linear in the generators: nothing but rounding may separate the sum of the single-term means from the
    all-terms mean, 64 sqrt(N) u s_mu"""
    a, theta = setup(engine, name)
    nt = len(GROUPS[name]["kinds"])
    mu, var, status = engine.predict_terms(theta, [1 << k for k in range(nt)] + [full_mask(name)], a["ts"])
    s = a["mu_scale"][list(a["masks"]).index(full_mask(name))]
    e = np.abs(np.sum(mu[0, :nt], axis=0) - mu[0, nt])
    tol = 64.0 * np.sqrt(len(a["t"])) * U * s
    print("\nadditivity %-20s worst e/tol %.3g" % (name, np.max(e / np.where(tol > 0, tol, 1.0))))
    assert np.all(e <= tol)


def test_each_sho_term_owns_its_own_slots(engine):
    """SHO (Q = 0.3) + SHO (Q = 5) + DRW and the same with the two Q swapped: the over-damped term holds two real slots,
    the other a complex pair, whichever comes first.  Each named term against its own truth (a swapped map misses by
    orders of magnitude), and both patterns alternating in one batch against each row alone."""
    alone, thetas = {}, {}
    for name in ("sho_over_first", "sho_over_second"):
        a, theta = setup(engine, name)
        mu, var, status = engine.predict_terms(theta, a["masks"], a["ts"])
        assert status[0] == 0
        for k in (0, 1):
            c = list(a["masks"]).index(1 << k)
            for v, out in (("mu", mu), ("var", var)):
                bound("%s term %d %s" % (name, k, v), len(a["t"]), out[0, c][None, :], a[v][c][None, :],
                      a[v + "_c64err"][c][None, :], a[v + "_scale"][c][None, :])
        alone[name], thetas[name] = (mu[0], var[0]), theta[0]
    # same kinds, same light curve: the damping side is a property of the row
    rows = np.array([thetas["sho_over_first"], thetas["sho_over_second"]] * 35)[:69]
    mu, var, status = engine.predict_terms(rows, a["masks"], a["ts"])
    assert np.all(status == 0)
    for b in range(69):
        m1, v1 = alone["sho_over_first" if b % 2 == 0 else "sho_over_second"]
        assert same(mu[b], m1) and same(var[b], v1), "row %d differs in the alternating batch" % b


def test_every_row_time_and_mask_is_invariant_bit_for_bit(engine):
    """the batch of 37 of the mtg_predict_at tests (two light curves, two rows outside the prior, one not positive
    definite): statuses and NaN as mtg_predict_at gives them; every row alone; ts shuffled; masks permuted; T = 1 and
    T = 32; single times"""
    g, a, t, y, dy, P, bounds, theta, want, lc = tpat.batch_of_37()
    engine.set_lightcurves(t, y, dy + 1e-12, y_offset=y.mean(axis=1))
    engine.set_model(g["kinds"], np.concatenate([a["theta"][0][:P], [0.0]]), np.arange(P, dtype=np.int32), bounds)
    ts = tpat.golden_util.new_times(t, 4242)
    masks = np.array([1, 2 | TERMS_MEAN, 3, 0, 3 | TERMS_MEAN, 2], dtype=np.uint32)
    mu, var, status = engine.predict_terms(theta, masks, ts, lc_index=lc)
    m0, v0, s0 = engine.predict_at(theta, ts, lc_index=lc)
    assert list(status) == want == list(s0)
    bad = np.array(want) != _engine.ST_OK
    assert np.all(np.isnan(mu[bad])) and np.all(np.isnan(var[bad]))
    assert np.all(np.isfinite(mu[~bad])) and np.all(np.isfinite(var[~bad]))
    assert same(mu[:, 4], m0) and same(var[:, 4], v0)
    on = int(np.flatnonzero(np.isin(ts, t))[0])
    singles = [0, on, int(np.flatnonzero((ts > t[0]) & (ts < t[-1]) & ~np.isin(ts, t))[3]), len(ts) - 1]
    for b in range(37):
        m1, v1, s1 = engine.predict_terms(theta[b:b + 1], masks, ts, lc_index=lc[b:b + 1])
        assert s1[0] == status[b] and same(m1[0], mu[b]) and same(v1[0], var[b]), "row %d differs alone" % b
        for k in singles:
            m1, v1, s1 = engine.predict_terms(theta[b:b + 1], masks[2:3], ts[k:k + 1], lc_index=lc[b:b + 1])
            assert m1.shape == (1, 1, 1) and same(m1[0, 0, 0], mu[b, 2, k]) and same(v1[0, 0, 0], var[b, 2, k]), (b, k)
    perm = np.random.default_rng(11).permutation(len(ts))
    m2, v2, s2 = engine.predict_terms(theta, masks, ts[perm], lc_index=lc)
    assert same(m2, mu[:, :, perm]) and same(v2, var[:, :, perm]) and list(s2) == want
    order = np.random.default_rng(12).permutation(len(masks))
    m3, v3, s3 = engine.predict_terms(theta, masks[order], ts, lc_index=lc)
    assert same(m3, mu[:, order]) and same(v3, var[:, order])
    m32, v32, s32 = engine.predict_terms(theta, np.tile(masks, 6)[:32], ts, lc_index=lc)
    for c in range(32):
        assert same(m32[:, c], mu[:, c % 6]) and same(v32[:, c], var[:, c % 6]), "mask %d of 32" % c
    for c in range(len(masks)):
        m1, v1, s1 = engine.predict_terms(theta, masks[c:c + 1], ts, lc_index=lc)
        assert same(m1[:, 0], mu[:, c]) and same(v1[:, 0], var[:, c]), "mask %d alone (T = 1)" % c
    m4, v4, s4 = engine.predict_terms(theta, masks, ts, lc_index=lc, return_var=False)
    assert v4 is None and same(m4, mu)


def test_rows_in_slabs_are_the_rows_alone(engine):
    """more than one slab by the means of the mtg_predict_at test: phase/j10 (N = 20011, J = 10: 5.3 MB a row), 210
    rows; every row is bit for bit one of the four distinct rows evaluated alone, and all terms are mtg_predict_at"""
    name = "phase/j10"
    a = tpat.arrays(name)
    t, y, dy = tq.setup(engine, name, a["theta"][0])
    rows = np.array([tq.free(name, r) for r in a["theta"]])
    assert 210 * len(t) * 33 * 8 > 1 << 30
    nt = len(tq.GROUPS[name]["kinds"])
    masks = [1, (1 << nt) - 1 | TERMS_MEAN, 1 << (nt - 1) | 2]
    pick = np.arange(210) % len(rows)
    mu, var, status = engine.predict_terms(rows[pick], masks, a["ts"])
    m1, v1, s1 = engine.predict_terms(rows, masks, a["ts"])
    m0, v0, s0 = engine.predict_at(rows, a["ts"])
    assert np.all(status == 0) and np.all(s1 == 0) and np.all(s0 == 0)
    assert same(mu, m1[pick]) and same(var, v1[pick])
    assert same(m1[:, 1], m0) and same(v1[:, 1], v0)


def test_argument_errors(engine):
    a, theta = setup(engine, "headline")
    ts = a["ts"]
    for masks, times in (([], ts), ([1] * 33, ts), ([1 << 3], ts), ([1 << 30], ts), ([1], np.array([1.0, np.nan])),
                         ([1], np.array([np.inf])), ([1], np.empty(0))):
        with pytest.raises(_engine.EngineError) as err:
            engine.predict_terms(theta, masks, times)
        assert err.value.code == _engine.E_ARG, (masks, times)
    engine.predict_terms(theta, [1 << 2 | TERMS_MEAN] * 32, ts[:1])
    # a profile mean: as mtg_predict_at
    nk = theta.shape[1]
    engine.set_model(GROUPS["headline"]["kinds"], np.concatenate([theta[0], [0.0, 1.0, 0.1, 0.0]]), np.arange(nk, dtype=np.int32),
                     np.tile([-np.inf, np.inf], (nk + 4, 1)), mean_kind=_engine.MEAN_SINE)
    with pytest.raises(_engine.EngineError) as err:
        engine.predict_terms(theta, [1], ts)
    assert err.value.code == _engine.E_UNSUPPORTED


def host_gp():
    a = arrays("headline")
    th = a["theta"]
    kernel = DampedRandomWalk(th[0], th[1]) + terms.SHOTerm(th[2], th[3], th[4]) + Lorentzian(th[5], th[6], th[7])
    return a, kernel


def test_gp_predict_with_a_kernel():
    a, kernel = host_gp()
    t, y, ts = a["t"], a["y"], a["ts"]
    gp = GP(kernel, mean=float(np.mean(y)))
    gp.compute(t, a["yerr"])
    before = gp.predict(y, t=ts, return_var=True, return_cov=False)
    before_t = gp.predict(y, return_var=True, return_cov=False)
    eng, model = gp._bound_engine(y)
    theta = model.full[model.free_index][None, :]
    for k, part in enumerate(gp.kernel.terms):
        mu, var = gp.predict(y, t=ts, return_var=True, return_cov=False, kernel=part)
        m, v, st = eng.predict_terms(theta, [1 << k | TERMS_MEAN], ts)
        assert st[0] == 0 and same(mu, m[0, 0] + (model.y_offset or 0.0)) and same(var, v[0, 0])
        assert same(gp.predict(y, t=ts, return_cov=False, kernel=part), mu)
        # the component against the fixture's truth (the mean is the light curve's average)
        c = list(a["masks"]).index(1 << k)
        bound("GP.predict kernel=terms[%d] mu" % k, len(t), (mu - np.mean(y))[None, :], a["mu"][c][None, :],
              a["mu_c64err"][c][None, :], (a["mu_scale"][c] + abs(np.mean(y)))[None, :])
        bound("GP.predict kernel=terms[%d] var" % k, len(t), var[None, :], a["var"][c][None, :], a["var_c64err"][c][None, :],
              a["var_scale"][c][None, :])
    two = gp.kernel.terms[0] + gp.kernel.terms[2]
    mu, var = gp.predict(y, t=ts, return_var=True, kernel=two)
    m, v, st = eng.predict_terms(theta, [5 | TERMS_MEAN], ts)
    assert same(mu, m[0, 0] + (model.y_offset or 0.0)) and same(var, v[0, 0])
    # the dense covariance of a component: its diagonal and mean against the linear-time ones, within both bounds
    mu_d, cov = gp.predict(y, t=ts, kernel=two)
    c = list(a["masks"]).index(5)
    for v_, out, ref, extra in (("mu", mu_d - np.mean(y), mu - np.mean(y), abs(np.mean(y))), ("var", np.diag(cov), var, 0.0)):
        rho = np.max(a[v_ + "_c64err"][c] / a[v_ + "_scale"][c])
        tol = 2.0 * max(10.0 * rho, 64.0 * np.sqrt(len(t)) * U) * (a[v_ + "_scale"][c] + extra)
        assert np.all(np.abs(out - ref) <= tol), v_
    with pytest.raises(ValueError):
        gp.predict(y, t=ts, kernel=Lorentzian(1.0, 2.0, 0.5))
    # kernel=None is what it was before the new entry ran in this process
    after = gp.predict(y, t=ts, return_var=True, return_cov=False)
    after_t = gp.predict(y, return_var=True, return_cov=False)
    assert same(before[0], after[0]) and same(before[1], after[1]) and same(before_t[0], after_t[0]) and same(before_t[1], after_t[1])
    m0, v0, s0 = eng.predict_at(theta, ts)
    assert same(after[0], m0[0] + (model.y_offset or 0.0)) and same(after[1], v0[0])


def test_gpmodelling_predict_components():
    a, kernel = host_gp()
    t, y = a["t"], a["y"]
    g = GPModelling(GappyLightcurve(t, y, a["yerr"] - 1e-12), kernel)
    current = g.gp.get_parameter_vector()
    comps = g.predict_components()
    assert list(comps) == ["terms[0]", "terms[1]", "terms[2]"] and np.array_equal(g.gp.get_parameter_vector(), current)
    at = g.predict_components(t=a["ts"])
    for k, name in enumerate(comps):
        assert comps[name][0].shape == (len(t),) and comps[name][1].shape == (len(t),) and at[name][0].shape == (48,)
        m, v = g.gp.predict(y, t=a["ts"], return_var=True, kernel=g.gp.kernel.terms[k])
        assert same(at[name][0], m) and same(at[name][1], v)
    # at the epochs the components and the mean add up to predict(y)'s mean: the new-time replay against the
    # training-time kernel, each within the bound (rho of the fixture's all-terms row; scales formed here in float64)
    mean = float(np.mean(y))
    total = mean + sum(comps[name][0] - mean for name in comps)
    mu0 = g.gp.predict(y, return_var=True, return_cov=False)[0]
    x = g.gp.apply_inverse(y - mean)
    kx = np.abs(g.gp.kernel.get_value(t[:, None] - t[None, :]) * x[None, :]).sum(axis=1)
    c = list(a["masks"]).index(7)
    rho = np.max(a["mu_c64err"][c] / a["mu_scale"][c])
    r = y - mean
    tol = max(10.0 * rho, 64.0 * np.sqrt(len(t)) * U) * ((abs(mean) + kx) + (np.abs(r) + np.abs(r - (mu0 - mean))))
    e = np.abs(total - mu0)
    print("\ncomponents + mean against predict(y): worst e/tol %.3g" % np.max(e / tol))
    assert np.all(e <= tol)
