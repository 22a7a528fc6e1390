"""Prediction and solves against the quad-precision truth (tests/golden/predict_golden.npz, made by
tests/golden/make_predict_golden.py from oracle/predict_sweep.h in __float128) at N up to 2e5: Engine.predict
(mtg_predict_kernel: the forward factorisation, then the backward sweep for K^-1 r and diag(K^-1)), Engine.apply_inverse
(mtg_apply_inverse_kernel on the stored generators) and GP.predict at new times (assembled on the host from
apply_inverse).  The test reads the fixture only.

With T the quad truth, c64 the stored float64 baseline (the same recurrences with celerite's phase at the absolute
time), s the stored cancellation scale and u = 2^-53, every stored value of a row satisfies

    e = |out - T| <= max(10 rho, 64 sqrt(N) u) s,   rho = max over the row's stored values of |c64 - T| / s

no worse than honest float64 arithmetic on the problem, and at rounding level where that is.  rho is taken per row
(per column for apply_inverse, which is held in the infinity norm anyway): on an ill-conditioned row the float64 error
of one sample is one draw of the row's rounding, and c64 lands 40 to 200 times below its row's level at single samples
of long_memory and extreme/5sho, where the kernel's own draw is at that level.  Rows of d max(dx) >= 1e4 rad (phase/j3,
phase/j10: up to 1.1e12 rad per step) are also held to factor 1 instead of 10: the kernel reduces its phase modulo 2 pi
exactly and must be no less accurate than celerite's phase at the absolute time -- the claim
tests/test_accuracy_vs_quad_gpu.py makes of the sweeps.  With the plain d (t - t_first) phase the kernel lands at
2.4 to 3.2 times celerite's error there.  The scales:
mu = [mean] + r - d K^-1 r has s_mu = |r| + d |K^-1 r|; var = d - d^2 (K^-1)_nn has s_var = d + d^2 (K^-1)_nn
(d = yerr^2 + jitter); apply_inverse is held column-wise in the infinity norm, ||x - T|| <= max(10 ||c64 - T||,
64 sqrt(N) u ||T||); new times have s_mu = |mean| + sum |k_* K^-1 r| and s_var = k(0) + |k_*^T K^-1 k_*|.  The bounds are
these formulas; they are not fitted to a run.

A known limitation, admitted on purpose by s_var: where the noise dominates (yerr^2 / k(0) >> 1, the noise_dominated
group at 1e4 .. 1e6) var = d - d^2 (K^-1)_nn cancels, and its relative error is about u d / var.  celerite's dense
formula k(0) - diag(K_* K^-1 K_*^T) does not lose those digits; the recurrence is not redesigned here.

Also: status 0 wherever celerite's is; rows are bit for bit the same alone and in a batch of 37 with a mixed lc_index,
rows outside the prior or not positive definite keeping their status and NaN; apply_inverse columns are bit for bit the
same for M in {1, 63, 64, 65, 257}."""
import json
import os

import numpy as np
import pytest

import golden_util
from mind_the_gaps_amd import engine as _engine
from mind_the_gaps_amd import terms
from mind_the_gaps_amd.engine import MEAN_LINEAR
from mind_the_gaps_amd.gp import GP
from mind_the_gaps_amd.models import DampedRandomWalk

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
U = 2.0 ** -53
FIX = np.load(os.path.join(HERE, "golden", "predict_golden.npz"))
GROUPS = {g["name"]: g for g in json.loads(bytes(FIX["manifest"]))["groups"]}
APPLY = [n for n, g in GROUPS.items() if "apply_sha256" in g]
AT = [n for n in GROUPS if n.replace("/", ".") + "/ts" in FIX.files]


def arrays(name):
    key = name.replace("/", ".") + "/"
    return {k[len(key):]: FIX[k] for k in FIX.files if k.startswith(key)}


def lightcurve(name):
    g = GROUPS[name]
    t, y, dy = golden_util.quad_lightcurve(g["lightcurve"])
    assert golden_util.lightcurve_sha256(t, y, dy) == g["sha256"], "%s: the light curve is not the fixture's" % name
    return t, y, dy


def linear(name):
    return GROUPS[name]["mean_kind"] == 1


def free(name, theta):
    """the free parameters: the kernel's, and the fitted line's under mean_kind 1 (a constant mean travels as
    y_offset, frozen at 0 in the model)"""
    return theta if linear(name) else theta[:-1]


def setup(engine, name, theta0, bounds=None):
    g = GROUPS[name]
    t, y, dy = lightcurve(name)
    P = len(theta0) if linear(name) else len(theta0) - 1
    if linear(name):
        engine.set_lightcurves(t, y, dy + 1e-12)
        engine.set_model(g["kinds"], np.asarray(theta0), np.arange(P, dtype=np.int32),
                         np.tile([-np.inf, np.inf], (P, 1)) if bounds is None else bounds, mean_kind=MEAN_LINEAR)
    else:
        engine.set_lightcurves(t, y, dy + 1e-12, y_offset=np.asarray(g["y_offset"]))
        engine.set_model(g["kinds"], np.concatenate([theta0[:P], [0.0]]), np.arange(P, dtype=np.int32),
                         np.tile([-np.inf, np.inf], (P + 1, 1)) if bounds is None else bounds)
    return t, y, dy


def bound(label, N, out, T, c64err, scale, factor=10.0):
    """the module's bound elementwise over [rows][samples]; returns (worst e / tol, where)"""
    c64err, scale = c64err.astype(np.float64), scale.astype(np.float64)
    rho = np.max(np.where(scale > 0, c64err / np.where(scale > 0, scale, 1.0), 0.0), axis=-1, keepdims=True)
    e = np.abs(out - T)
    tol = np.maximum(factor * rho, 64.0 * np.sqrt(N) * U) * scale
    ratio = np.where(tol > 0, e / np.where(tol > 0, tol, 1.0), np.where(e == 0, 0.0, np.inf))
    ratio = np.where(np.isnan(out), np.inf, ratio)
    w = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    assert np.all(ratio <= 1.0), "%s at %s: |out - T| = %.3e > %.3e (c64 %.3e here, row %.3e of the scale; floor %.3e)" % (
        label, w, e[w], tol[w], c64err[w], rho[w[:-1]][0], 64.0 * np.sqrt(N) * U * scale[w])
    return float(ratio[w]), w


def report(label, worst):
    for name, (w, where) in sorted(worst.items(), key=lambda kv: -kv[1][0]):
        print("\nquad-truth %-16s %-28s worst e/tol %.3g at %s" % (label, name, w, where))


@pytest.mark.parametrize("name", list(GROUPS))
def test_predict_at_training_times_against_quad_truth(engine, name):
    """Engine.predict (mtg_predict_kernel) at the stored samples of every row: mu and var within the bound, status 0
    (celerite's status on every fixture row)."""
    a = arrays(name)
    theta = a["theta"]
    t, y, dy = setup(engine, name, theta[0])
    N = len(t)
    mu, var, status = engine.predict(np.array([free(name, r) for r in theta]), lc_index=a["lc"])
    assert np.all(status == 0), "%s: statuses %s (celerite: 0)" % (name, status)
    idx = a["idx"]
    worst = {}
    phase = phase_rows(name, theta, t)
    for v, out in (("mu", mu), ("var", var)):
        worst["%s %s" % (name, v)] = bound("predict %s / %s" % (v, name), N, out[:, idx], a[v], a[v + "_c64err"],
                                           a[v + "_scale"])
        if phase.any():
            bound("predict %s / %s (phase claim)" % (v, name), N, out[phase][:, idx], a[v][phase],
                  a[v + "_c64err"][phase], a[v + "_scale"][phase], factor=1.0)
    report("predict", worst)


def phase_rows(name, theta, t):
    """rows with d max(dx) >= 1e4 rad: there the kernel's phase, reduced modulo 2 pi exactly (mtg_elapsed_sincos), is
    held to celerite's own error (factor 1), the claim tests/test_accuracy_vs_quad_gpu.py makes of the sweeps"""
    from oracle import dense
    kinds = GROUPS[name]["kinds"]
    nk = dense.n_kernel_params(kinds)
    dxmax = float(np.max(np.diff(t))) if len(t) > 1 else 0.0
    return np.array([np.max(dense.build_coeffs(kinds, r[:nk])[5], initial=0.0) * dxmax >= 1.0e4 for r in theta])


@pytest.mark.parametrize("name", APPLY)
def test_apply_inverse_against_quad_truth(engine, name):
    """Engine.apply_inverse (mtg_apply_inverse_kernel) on three columns per row: the residual, a standard-normal
    column and a column of K_*^T; ||x - T||_inf at the stored samples within the bound of each column."""
    g, a = GROUPS[name], arrays(name)
    theta = a["theta"]
    t, y, dy = setup(engine, name, theta[0])
    N, idx, nk = len(t), a["idx"], len(theta[0]) - (2 if linear(name) else 1)
    worst = (0.0, None)
    for b, row in enumerate(theta):
        cols = golden_util.apply_columns(t, y[a["lc"][b]], g["mean_kind"], row, nk, g["kinds"], g["apply_seed"][b])
        assert [golden_util.col_sha(cols[:, 1]), golden_util.col_sha(cols[:, 2])] == g["apply_sha256"][b], \
            "%s row %d: the right-hand sides are not the fixture's" % (name, b)
        x, status = engine.apply_inverse(free(name, row), cols, lc_index=int(a["lc"][b]))
        assert status == 0, "%s row %d: status %d (celerite: 0)" % (name, b, status)
        e = np.max(np.abs(x[idx].T - a["apply_x"][b]), axis=1, keepdims=True)            # [3][1]
        w = bound("apply_inverse / %s row %d" % (name, b), N, e, np.zeros_like(e),
                  a["apply_c64err"][b][:, None], a["apply_tinf"][b][:, None])
        if w[0] >= worst[0]:
            worst = (w[0], (b, w[1][0]))
    report("apply_inverse", {name: worst})


def kernel_of(kinds, th):
    make = {1: lambda p: terms.ComplexTerm(*p), 3: lambda p: terms.SHOTerm(*p), 6: lambda p: DampedRandomWalk(*p)}
    n = {1: 3, 3: 3, 6: 2}
    out, i = None, 0
    for k in kinds:
        term = make[k](th[i:i + n[k]])
        i += n[k]
        out = term if out is None else out + term
    return out


@pytest.mark.parametrize("name", AT)
def test_predict_at_new_times_against_quad_truth(name):
    """GP.predict(y, t=ts, return_var=True) at 48 times between samples, on samples and beyond both ends: the host's
    K_* K^-1 r and k(0) - k_*^T K^-1 k_* over the device's apply_inverse, within the bound."""
    g, a = GROUPS[name], arrays(name)
    t, y, dy = lightcurve(name)
    N, ts = len(t), a["ts"]
    worst = {}
    for b, row in enumerate(a["theta"]):
        nk = len(row) - (2 if linear(name) else 1)
        gp = GP(kernel_of(g["kinds"], row[:nk]), mean=float(row[nk]))
        gp.compute(t, dy[a["lc"][b]] + 1e-12)
        mu, var = gp.predict(y[a["lc"][b]], t=ts, return_var=True, return_cov=False)
        for v, out in (("mu", mu), ("var", var)):
            w = bound("predict_at %s / %s row %d" % (v, name, b), N, out, a["at_" + v][b],
                      a["at_%s_c64err" % v][b], a["at_%s_scale" % v][b])
            key = "%s %s" % (name, v)
            if w[0] >= worst.get(key, (0.0, None))[0]:
                worst[key] = (w[0], (b,) + w[1])
    report("predict_at", worst)


def test_predict_rows_are_batch_invariant(engine):
    """37 rows on two light curves -- the fixture's rows of typical/complex4+real, rows outside the prior box and one
    whose covariance is not positive definite in float64 (a real term of amplitude e^80 and c = e^-40: its rounding
    swamps the noise, celerite's status is 2; the prior itself rejects every covariance that is not positive definite
    in exact arithmetic) -- give bit for bit what each row gives alone.  Rows outside the prior or not positive definite
    get their status and leave mu and var NaN."""
    name = "typical/complex4+real"
    g, a = GROUPS[name], arrays(name)
    rec = dict(g["lightcurve"], L=2)
    t, y, dy = golden_util.quad_lightcurve(rec)
    P = len(a["theta"][0]) - 1
    bounds = np.vstack([np.tile([-100.0, 100.0], (P, 1)), [[-np.inf, np.inf]]])
    engine.set_lightcurves(t, y, dy + 1e-12, y_offset=y.mean(axis=1))
    engine.set_model(g["kinds"], np.concatenate([a["theta"][0][:P], [0.0]]), np.arange(P, dtype=np.int32), bounds)
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
    theta = np.array(rows)
    lc = (np.arange(37) * 7 % 3 % 2).astype(np.int32)
    mu, var, status = engine.predict(theta, lc_index=lc)
    assert list(status) == want, "statuses %s, expected %s" % (list(status), want)
    bad = np.array(want) != _engine.ST_OK
    assert np.all(np.isnan(mu[bad])) and np.all(np.isnan(var[bad]))
    assert np.all(np.isfinite(mu[~bad])) and np.all(np.isfinite(var[~bad]))
    for b in range(37):
        m1, v1, s1 = engine.predict(theta[b:b + 1], lc_index=lc[b:b + 1])
        assert s1[0] == status[b]
        assert np.array_equal(m1[0], mu[b], equal_nan=True) and np.array_equal(v1[0], var[b], equal_nan=True), \
            "row %d differs alone and in the batch of 37" % b


@pytest.mark.parametrize("name", ["offset/seconds", "phase/j3"])
def test_apply_inverse_columns_are_independent_of_m(engine, name):
    """One lane per right-hand side: column j of K^-1 B is bit for bit the same for M in {1, 63, 64, 65, 257}
    (N <= 1e4)."""
    a = arrays(name)
    t, y, dy = setup(engine, name, a["theta"][0])
    assert len(t) <= 10000
    B = np.random.default_rng(3).standard_normal((len(t), 257))
    th = free(name, a["theta"][-1])
    full, st = engine.apply_inverse(th, B, lc_index=int(a["lc"][-1]))
    assert st == 0
    for M in (1, 63, 64, 65):
        x, st = engine.apply_inverse(th, B[:, :M], lc_index=int(a["lc"][-1]))
        assert st == 0 and np.array_equal(x, full[:, :M]), "M = %d: columns differ from M = 257" % M
    x1, st = engine.apply_inverse(th, B[:, 200], lc_index=int(a["lc"][-1]))
    assert st == 0 and np.array_equal(x1, full[:, 200])
