"""The prediction at NEW times from the factorisation (mtg_predict_at: mind_the_gaps_amd/csrc/mtg_predict_at.hip)
against the quad-precision truth of tests/golden/predict_at_golden.npz (made by tests/golden/make_predict_at_golden.py
from oracle/predict_sweep.h's predict_at in __float128) for EVERY group of quad_golden.json plus noise_dominated, N up
to 2e5 with J = 10.

The bound is the project's, imported from tests/test_predict_vs_quad_gpu.py and not fitted to a run: with T the truth,
c64 celerite's dense expression in float64, s the cancellation scale and u = 2^-53,

    |out - T| <= max(10 rho, 64 sqrt(N) u) s,   rho = the row's worst |c64 - T| / s,
    s_mu = |mean| + sum |k_* K^-1 r|,  s_var = k(0) + |k_*^T K^-1 k_*|,

rows of d max(dx) >= 1e4 rad held to factor 1 instead of 10 (phase_rows).  Status 0 wherever celerite's is.

Also: every (row, t*) is bit for bit the same alone, in a batch of 37 rows with a mixed lc_index (rows outside the prior
or not positive definite keep their status and read back NaN), with ts shuffled, embedded among other times and without
the variance; on samples the result agrees with Engine.predict; a grid of 1e6 times on N = 2e5, J = 10 (the dense
cross-covariance would take 1.6 TB) runs; per-light-curve times, an over-damped SHO row and slabs of rows; and
GPModelling.predict_at.
"""
import json
import os
import time

import numpy as np
import pytest

import golden_util
import test_predict_vs_quad_gpu as tq
from mind_the_gaps_amd import engine as _engine
from mind_the_gaps_amd import synthetic as synth
from mind_the_gaps_amd import terms
from mind_the_gaps_amd.gp import GP
from mind_the_gaps_amd.gpmodelling import GPModelling
from mind_the_gaps_amd.lightcurves import GappyLightcurve
from mind_the_gaps_amd.models import DampedRandomWalk, Lorentzian
from oracle import dense
from oracle import predict as oracle_predict
from test_predict_vs_quad_gpu import bound, free, linear, phase_rows, report, setup

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
U = 2.0 ** -53
FIX = np.load(os.path.join(HERE, "golden", "predict_at_golden.npz"))
GROUPS = {g["name"]: g for g in json.loads(bytes(FIX["manifest"]))["groups"]}


def arrays(name):
    key = name.replace("/", ".") + "/"
    return {k[len(key):]: FIX[k] for k in FIX.files if k.startswith(key)}


def whole_mean(name, a, mu):
    """the kernel's mu plus what it leaves out: the per-light-curve constant mean (y_offset)"""
    if linear(name):
        return mu
    return mu + np.asarray(GROUPS[name]["y_offset"])[a["lc"]][:, None]


def test_fixture_groups_are_the_training_time_fixtures():
    assert list(GROUPS) == list(tq.GROUPS)
    for name, g in GROUPS.items():
        assert g["sha256"] == tq.GROUPS[name]["sha256"] and g["kinds"] == tq.GROUPS[name]["kinds"]


@pytest.mark.parametrize("name", list(GROUPS))
def test_predict_at_against_quad_truth(engine, name):
    """Engine.predict_at at the 48 stored times of every row: mu and var within the bound, status 0"""
    a = arrays(name)
    theta = a["theta"]
    t, y, dy = setup(engine, name, theta[0])
    N = len(t)
    mu, var, status = engine.predict_at(np.array([free(name, r) for r in theta]), a["ts"], lc_index=a["lc"])
    assert np.all(status == 0), "%s: statuses %s (celerite: 0)" % (name, status)
    mu = whole_mean(name, a, mu)
    worst = {}
    phase = phase_rows(name, theta, t)
    failures = []
    for v, out in (("mu", mu), ("var", var)):
        try:
            worst["%s %s" % (name, v)] = bound("predict_at %s / %s" % (v, name), N, out, a[v], a[v + "_c64err"],
                                               a[v + "_scale"])
            if phase.any():
                w = bound("predict_at %s / %s (phase claim)" % (v, name), N, out[phase], a[v][phase],
                          a[v + "_c64err"][phase], a[v + "_scale"][phase], factor=1.0)
                worst["%s %s phase" % (name, v)] = w
        except AssertionError as exc:
            failures.append(str(exc))
    report("predict_at", worst)
    assert not failures, "\n".join(failures)


def batch_of_37():
    """the recipe of test_predict_vs_quad_gpu.test_predict_rows_are_batch_invariant"""
    name = "typical/complex4+real"
    g, a = tq.GROUPS[name], tq.arrays(name)
    rec = dict(g["lightcurve"], L=2)
    t, y, dy = golden_util.quad_lightcurve(rec)
    P = len(a["theta"][0]) - 1
    bounds = np.vstack([np.tile([-100.0, 100.0], (P, 1)), [[-np.inf, np.inf]]])
    base = a["theta"][:, :P]
    rows, want = [], []
    rng = np.random.default_rng(7)
    for i in range(37):
        r = base[i % len(base)] + 0.05 * rng.uniform(-1.0, 1.0, P)
        st = _engine.ST_OK
        if i in (5, 22):
            r[i % P] = 101.0 + i                    # outside the box
            st = _engine.ST_PRIOR
        elif i == 13:
            r[4], r[5] = 80.0, -40.0                # real term a = e^80, c = e^-40: K = a 1 1^T + noise in float64
            st = _engine.ST_NOTPD
        rows.append(r)
        want.append(st)
    lc = (np.arange(37) * 7 % 3 % 2).astype(np.int32)
    return g, a, t, y, dy, P, bounds, np.array(rows), want, lc


def same(x, y):
    return np.array_equal(x, y, equal_nan=True)


def test_every_row_and_time_is_invariant_bit_for_bit(engine):
    g, a, t, y, dy, P, bounds, theta, want, lc = batch_of_37()
    engine.set_lightcurves(t, y, dy + 1e-12, y_offset=y.mean(axis=1))
    engine.set_model(g["kinds"], np.concatenate([a["theta"][0][:P], [0.0]]), np.arange(P, dtype=np.int32), bounds)
    ts = golden_util.new_times(t, 4242)
    mu, var, status = engine.predict_at(theta, ts, lc_index=lc)
    assert list(status) == want, "statuses %s, expected %s" % (list(status), want)
    bad = np.array(want) != _engine.ST_OK
    assert np.all(np.isnan(mu[bad])) and np.all(np.isnan(var[bad]))
    assert np.all(np.isfinite(mu[~bad])) and np.all(np.isfinite(var[~bad]))
    # alone: every row with all the times, and every row with single times (before, on a sample, between, after)
    on = int(np.flatnonzero(np.isin(ts, t))[0])
    singles = [0, on, int(np.flatnonzero((ts > t[0]) & (ts < t[-1]) & ~np.isin(ts, t))[3]), len(ts) - 1]
    for b in range(37):
        m1, v1, s1 = engine.predict_at(theta[b:b + 1], ts, lc_index=lc[b:b + 1])
        assert s1[0] == status[b]
        assert same(m1[0], mu[b]) and same(v1[0], var[b]), "row %d differs alone and in the batch of 37" % b
        for k in singles:
            m1, v1, s1 = engine.predict_at(theta[b:b + 1], ts[k:k + 1], lc_index=lc[b:b + 1])
            assert s1[0] == status[b] and m1.shape == (1, 1)
            assert same(m1[0, 0], mu[b, k]) and same(v1[0, 0], var[b, k]), "row %d, time %d differs alone (B = M = 1)" % (b, k)
    # shuffled
    perm = np.random.default_rng(11).permutation(len(ts))
    m2, v2, s2 = engine.predict_at(theta, ts[perm], lc_index=lc)
    assert same(m2, mu[:, perm]) and same(v2, var[:, perm]) and list(s2) == want
    # embedded among M times in any order
    rng = np.random.default_rng(12)
    span = t[-1] - t[0]
    for M in (1, 63, 64, 65, 4097):
        other = rng.uniform(t[0] - 0.3 * span, t[-1] + 0.3 * span, M)
        k = min(M, len(ts))
        where = rng.choice(M, k, replace=False)
        which = rng.choice(len(ts), k, replace=False)
        other[where] = ts[which]
        m3, v3, s3 = engine.predict_at(theta, other, lc_index=lc)
        assert list(s3) == want
        assert same(m3[:, where], mu[:, which]) and same(v3[:, where], var[:, which]), "M = %d" % M
    # mean only
    m4, v4, s4 = engine.predict_at(theta, ts, lc_index=lc, return_var=False)
    assert v4 is None and list(s4) == want and same(m4, mu)
    # duplicates allowed
    m5, v5, s5 = engine.predict_at(theta, np.concatenate([ts, ts[::-1]]), lc_index=lc)
    assert same(m5[:, :len(ts)], mu) and same(m5[:, len(ts):], mu[:, ::-1]) and same(v5[:, len(ts):], var[:, ::-1])
    # a non-finite time is an argument error
    with pytest.raises(_engine.EngineError):
        engine.predict_at(theta, np.array([1.0, np.nan]), lc_index=lc)


def test_rows_in_slabs_are_the_rows_alone(engine):
    """B N (3 J + 3) 8 bytes beyond the workspace budget of 1 GiB: phase/j10 (N = 20011, J = 10: 5.3 MB a row), 210 rows
    -> two slabs; every row is bit for bit one of the four distinct rows evaluated alone"""
    name = "phase/j10"
    a = arrays(name)
    t, y, dy = setup(engine, name, a["theta"][0])
    rows = np.array([free(name, r) for r in a["theta"]])
    assert 210 * len(t) * 33 * 8 > 1 << 30
    pick = np.arange(210) % len(rows)
    mu, var, status = engine.predict_at(rows[pick], a["ts"])
    m0, v0, s0 = engine.predict_at(rows, a["ts"])
    assert np.all(status == 0) and np.all(s0 == 0)
    assert same(mu, m0[pick]) and same(var, v0[pick])


@pytest.mark.parametrize("name", [n for n in GROUPS if GROUPS[n]["N"] <= 20011])
def test_on_samples_agrees_with_training_time_predict(engine, name):
    """At ts = t[idx] the noise-free conditional law is that of the training times: k(0) - k_n^T K^-1 k_n =
    d - d^2 (K^-1)_nn and mean + k_n^T K^-1 r = mean + r - d (K^-1 r)_n analytically.  The two kernels agree within
    the SUM of their quad bounds.  New times: rho of the fixture's row, scales s_mu = |mean| + sum |k_* K^-1 r| and
    s_var = k(0) + |k_*^T K^-1 k_*| taken at the fixture's on-sample times.  Training times: rho of predict_golden.npz's
    row, scales s_mu = |r| + d |K^-1 r| = |r| + |r - (mu - mean)| and s_var = d + d^2 (K^-1)_nn = 2 d - var formed
    from the outputs themselves (their error is of second order in the bound)."""
    g, a, at = GROUPS[name], arrays(name), tq.arrays(name)
    theta = a["theta"]
    assert np.array_equal(theta, at["theta"])
    t, y, dy = setup(engine, name, theta[0])
    N = len(t)
    on = np.flatnonzero(np.isin(a["ts"], t))
    assert len(on) >= 12
    idx = np.searchsorted(t, a["ts"][on], side="right") - 1
    rows = np.array([free(name, r) for r in theta])
    mu, var, status = engine.predict_at(rows, a["ts"][on], lc_index=a["lc"])
    mu0, var0, status0 = engine.predict(rows, lc_index=a["lc"])
    assert np.all(status == 0) and np.all(status0 == 0)
    nk = dense.n_kernel_params(g["kinds"])
    worst = 0.0
    for b, row in enumerate(theta):
        l = a["lc"][b]
        mean = row[nk] * t[idx] + row[nk + 1] if linear(name) else np.zeros(len(idx))
        r = (y[l] - (0.0 if linear(name) else g["y_offset"][l]))[idx] - mean
        jit = dense.build_coeffs(g["kinds"], row[:nk])[6]
        d = (dy[l][idx] + 1e-12) ** 2 + jit
        floor = 64.0 * np.sqrt(N) * U
        for v, new, old, s_old in (("mu", mu[b], mu0[b][idx], np.abs(r) + np.abs(r - (mu0[b][idx] - mean))),
                                   ("var", var[b], var0[b][idx], 2.0 * d - var0[b][idx])):
            def rho(arr, v=v):
                e, s = arr[v + "_c64err"][b].astype(np.float64), arr[v + "_scale"][b].astype(np.float64)
                return float(np.max(np.where(s > 0, e / np.where(s > 0, s, 1.0), 0.0)))
            tol = max(10.0 * rho(a), floor) * a[v + "_scale"][b][on].astype(np.float64) + max(10.0 * rho(at), floor) * s_old
            e = np.abs(new - old)
            ok = np.where(tol > 0, e <= tol, e == 0)
            k = int(np.argmax(e - tol))
            assert np.all(ok), "%s row %d %s on samples: |new - training| = %.3e > %.3e" % (name, b, v, e[k], tol[k])
            worst = max(worst, float(np.max(np.where(tol > 0, e / np.where(tol > 0, tol, 1.0), 0.0))))
    print("\non-sample consistency %-28s worst e/(tol_at + tol_train) %.3g" % (name, worst))


def test_a_million_times_on_rank10_config5(engine):
    """The shape the dense path cannot run: N = 2e5, five SHO terms, a uniform grid of 1e6 times over the span
    stretched by 1 % on both sides with the fixture's 48 times merged in.  Every value finite, the variance within
    [0, k(0)] to tol = 64 sqrt(N) u 2 k(0), the 48 embedded values bit for bit those of the 48-point call.  The wall
    time is printed, not asserted."""
    name = "rank10/config5"
    g, a = GROUPS[name], arrays(name)
    t, y, dy = setup(engine, name, a["theta"][0])
    N = len(t)
    row = free(name, a["theta"][0])[None, :]
    span = t[-1] - t[0]
    grid = np.linspace(t[0] - 0.01 * span, t[-1] + 0.01 * span, 1000000)
    both = np.concatenate([grid, a["ts"]])
    order = np.argsort(both, kind="stable")
    ts = both[order]
    where = np.empty(len(both), dtype=np.int64)
    where[order] = np.arange(len(both))
    m48, v48, s48 = engine.predict_at(row, a["ts"], lc_index=a["lc"][:1])
    engine.synchronize()
    started = time.perf_counter()
    mu, var, status = engine.predict_at(row, ts, lc_index=a["lc"][:1])
    wall = time.perf_counter() - started
    print("\npredict_at N = %d, J = 10, M = %d: %.3f s wall (host to host)" % (N, len(ts), wall))
    assert status[0] == 0 and s48[0] == 0
    assert np.all(np.isfinite(mu)) and np.all(np.isfinite(var))
    k0 = g["k0"][0]
    tol = 64.0 * np.sqrt(N) * U * 2.0 * k0
    assert np.min(var) >= -tol and np.max(var) <= k0 + tol, (np.min(var), np.max(var), k0, tol)
    emb = where[len(grid):]
    assert np.array_equal(mu[0, emb], m48[0]) and np.array_equal(var[0, emb], v48[0])


def quad_bounds(label, N, t, y, dy, kinds, full, ts, outs):
    """each (mu, var) pair of ``outs`` within the module's bound of the quad truth computed here (small N); returns the
    tolerances [2][M]"""
    q = oracle_predict.predict_at(t, y, dy, kinds, full, ts)
    c = oracle_predict.predict_at(t, y, dy, kinds, full, ts, c64=True)
    assert q.status == 0 and c.status == 0
    tols = []
    for i, (v, s) in enumerate((("mu", "s_mu"), ("var", "s_var"))):
        T, S = getattr(q, v), getattr(q, s)
        e64 = np.abs((getattr(c, v) - T) - getattr(q, v + "_lo"))
        for k, out in enumerate(outs):
            bound("%s %s route %d" % (label, v, k), N, out[i][None, :], T[None, :], e64[None, :], S[None, :])
        tols.append(np.maximum(10.0 * np.max(e64 / S), 64.0 * np.sqrt(N) * U) * S)
    return tols


def test_an_over_damped_sho_row_against_the_dense_assembly():
    """a model whose row expands an SHO term with Q < 1/2 into two real terms (signature 1):
    GP.predict(return_var=True) -- the new kernel -- against the mean and the diagonal of GP.predict(return_cov=True) --
    the dense assembly over apply_inverse that stays -- within the sum of both bounds, each within its own of the quad
    truth"""
    N = 400
    t, y, dy = synth.make_lightcurves(N, 1, seed=31)
    y, dy = y[0], dy[0]
    th = np.array([np.log(np.var(y)), np.log(0.2), np.log(np.var(y)), np.log(0.3), np.log(1.5)])
    gp = GP(DampedRandomWalk(th[0], th[1]) + terms.SHOTerm(th[2], th[3], th[4]), mean=float(np.mean(y)))
    gp.compute(t, dy + 1e-12)
    ts = golden_util.new_times(t, 77)
    mu, var = gp.predict(y, t=ts, return_var=True, return_cov=False)
    mu_d, cov = gp.predict(y, t=ts, return_cov=True)
    only = gp.predict(y, t=ts, return_cov=False)
    assert np.array_equal(only, mu)
    tols = quad_bounds("over-damped", N, t, y, dy, [synth.K_DRW, synth.K_SHO], np.append(th, np.mean(y)), ts,
                       [(mu, var), (mu_d, np.diag(cov))])
    assert np.all(np.abs(mu - mu_d) <= 2.0 * tols[0]) and np.all(np.abs(var - np.diag(cov)) <= 2.0 * tols[1])


def test_per_lightcurve_times(engine):
    """t_per_lc = 1, L = 2: every row searches and replays its own light curve's times; against the dense assembly over
    Engine.apply_inverse and the quad truth"""
    N = 300
    ta, ya, dya = synth.make_lightcurves(N, 1, seed=41)
    tb, yb, dyb = synth.make_lightcurves(N, 1, seed=42)
    t = np.vstack([ta, 1.7 * tb + 3.0])
    y, dy = np.vstack([ya[0], yb[0]]), np.vstack([dya[0], dyb[0]])
    assert not np.array_equal(t[0], t[1])
    kinds = synth.NULL_MODEL
    th = synth.truth(kinds)
    P = len(th)
    engine.set_lightcurves(t, y, dy + 1e-12, y_offset=y.mean(axis=1))
    engine.set_model(kinds, np.concatenate([th, [0.0]]), np.arange(P, dtype=np.int32), np.tile([-np.inf, np.inf], (P + 1, 1)))
    ts = np.sort(np.concatenate([golden_util.new_times(t[0], 5), golden_util.new_times(t[1], 6)]))
    lc = np.array([1, 0, 1], dtype=np.int32)
    mu, var, status = engine.predict_at(np.tile(th, (3, 1)), ts, lc_index=lc)
    assert np.all(status == 0)
    co = dense.build_coeffs(kinds, th)
    for b, l in enumerate(lc):
        kxs = dense.kernel_value(co, ts[:, None] - t[l][None, :])
        sol, st = engine.apply_inverse(th, np.column_stack([y[l] - y[l].mean(), kxs.T]), lc_index=int(l))
        assert st == 0
        mu_d = y[l].mean() + kxs @ sol[:, 0]
        var_d = dense.kernel_value(co, 0.0) - np.sum(kxs.T * sol[:, 1:], axis=0)
        out = (mu[b] + y[l].mean(), var[b])
        tols = quad_bounds("per-lc times row %d" % b, N, t[l], y[l], dy[l], kinds, np.append(th, y[l].mean()), ts,
                           [out, (mu_d, var_d)])
        assert np.all(np.abs(out[0] - mu_d) <= 2.0 * tols[0]) and np.all(np.abs(out[1] - var_d) <= 2.0 * tols[1])


def test_gpmodelling_predict_at_is_one_launch_of_gp_predict():
    """GPModelling.predict_at with [B][P] parameter vectors (draws around the truth, as a slice of a chain is) equals B
    separate GP.predict(t=ts, return_var=True) calls bit for bit; include_noise adds each vector's kernel.jitter"""
    N = 500
    t, y, dy = synth.make_lightcurves(N, 1, seed=51)
    y, dy = y[0], dy[0]
    th = synth.truth(synth.ALT_MODEL)
    kernel = (DampedRandomWalk(th[0], th[1]) + terms.SHOTerm(th[2], th[3], th[4]) + Lorentzian(th[5], th[6], th[7])
              + terms.JitterTerm(np.log(0.05 * np.std(y))))
    g = GPModelling(GappyLightcurve(t, y, dy), kernel)
    ts = golden_util.new_times(t, 9)
    B = 9
    chain = np.hstack([synth.draw_thetas(synth.ALT_MODEL, B, seed=52, percent=0.05),
                       np.log(0.05 * np.std(y)) + 0.1 * np.random.default_rng(53).standard_normal((B, 1))])
    current = g.gp.get_parameter_vector()
    mu, var = g.predict_at(ts, chain)
    mu_n, var_n = g.predict_at(ts, chain, include_noise=True)
    assert mu.shape == (B, len(ts)) and var.shape == (B, len(ts)) and np.array_equal(mu_n, mu)
    assert np.array_equal(g.gp.get_parameter_vector(), current)
    m1, v1 = g.predict_at(ts)                       # no posteriors derived: the GP's current vector
    assert m1.shape == (len(ts),)
    m2, v2 = g.gp.predict(y, t=ts, return_var=True, return_cov=False)
    assert np.array_equal(m1, m2) and np.array_equal(v1, v2)
    for b in range(B):
        g.gp.set_parameter_vector(chain[b])
        m, v = g.gp.predict(y, t=ts, return_var=True, return_cov=False)
        assert np.array_equal(m, mu[b]) and np.array_equal(v, var[b]), "row %d" % b
        assert g.gp.kernel.jitter > 0 and np.array_equal(var_n[b], var[b] + g.gp.kernel.jitter)
    g.gp.set_parameter_vector(current)
