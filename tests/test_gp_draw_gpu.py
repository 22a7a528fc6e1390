"""Engine.gp_draw / GP.sample (mtg_gp_draw_kernel: y = mean + L sqrt(D) q from the factorisation K = L diag(D) L^T) on the
device.  The fixture tests/golden/gp_draw_golden.npz is made by tests/golden/make_gp_draw_golden.py (the recurrence in
mpmath at 40 digits, checked there against the mpmath dense Cholesky); the host replay is tests/gp_draw_replay.py.

1. Truth.  With T the truth, c64 the stored float64 baseline (the same recurrence with celerite's phase at the
   absolute time), s_n = sum_m |L_nm sqrt(D_m) q_m| and u = 2^-53, every stored sample of a row satisfies
       |y - T| <= max(10 rho, 64 sqrt(N) u) s,   rho = max over the row's stored samples of |c64 - T| / s
   with 1 in place of 10 on rows of d max(dx) >= 1e4 rad (the kernel reduces its phase modulo 2 pi exactly and must be
   no less accurate than celerite's phase at the absolute time): the rule of tests/test_predict_vs_quad_gpu.py.
2. A row is bit for bit the same alone, in a batch of 37 with a mixed lc_index, and across a slab boundary; the
   device-drawn normals do not depend on B nor on where set_stream_base puts the row; rows outside the prior or not
   positive definite keep their status and NaN.
3. The device's normals are the replayed Philox / Box-Muller normals.  Through a white model (a jitter term alone:
   y = sqrt(sigma^2 + jitter) q, so q comes back by one division) they are compared value by value.  The device's log
   and sincospi are accurate to 1 ulp and 2 ulp (the OCML figures the math probe of tests/test_device_math_gpu.py
   holds exp and sincos to), numpy's to 1 ulp; rad = sqrt(-2 ln u1) carries at most 1 + 1/2 ulp of either side, the
   product with cos / sin and the two roundings of sqrt(d) q / sqrt(d) three more: |q_dev - q_replay| <= 16 u rad with
   rad >= |q| is that sum with a factor 2 to spare.  Through a correlated model the recovered normals are held to the
   truth test's floor, 64 sqrt(N) u s / sqrt(D_n).
4. Round trip through the shipped likelihood: lnL(y) - lnL(mean) = -1/2 q^T q for a draw y from q, headline model,
   N = 1e4 and 2e5, serial and time-parallel dispatch.  The margin is measured, not guessed: the host replay's draw
   pushed through oracle.quad.loglike misses the identity by its own defect; 10 times that or
   64 sqrt(N) u (1/2 q^T q + |lnL|), whichever is larger.
5. Distribution of 4096 device draws at N = 256 (tests/test_gp_draw_cpu.py asks the same of the replay).
6. The public API: GP.sample and GPModelling.generate_from_posteriors(method=...); the default method's output is the
   one recorded at the parent commit (tests/golden/posterior_sims_golden.npz), bit for bit."""
import json
import os
import sys

import numpy as np
import pytest

import golden_util
import gp_draw_replay as R
import test_gp_draw_cpu as cpu
from mind_the_gaps_amd import engine as _engine
from mind_the_gaps_amd import synthetic as synth
from mind_the_gaps_amd.engine import MEAN_LINEAR
from oracle import dense

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_posterior_sims_golden as PG  # noqa: E402  (the case and the route of posterior_sims_golden.npz)

U = 2.0 ** -53
FIX = np.load(os.path.join(HERE, "golden", "gp_draw_golden.npz"))
GROUPS = {g["name"]: g for g in json.loads(bytes(FIX["manifest"]))["groups"]}
WORST = {}


def arrays(name):
    key = name.replace("/", ".") + "/"
    return {k[len(key):]: FIX[k] for k in FIX.files if k.startswith(key)}


def lightcurves(g):
    parts = [golden_util.quad_lightcurve(r) for r in g["recipes"]]
    for p, want in zip(parts, g["sha256"]):
        assert golden_util.lightcurve_sha256(*p) == want, "%s: the light curve is not the fixture's" % g["name"]
    if len(parts) == 1:
        return parts[0]
    return np.array([p[0] for p in parts]), np.vstack([p[1] for p in parts]), np.vstack([p[2] for p in parts])


def setup(engine, g, theta0, bounds=None):
    t, y, dy = lightcurves(g)
    P = len(theta0)
    if g["mean_kind"] == 1:
        engine.set_lightcurves(t, y, dy + 1e-12)
        engine.set_model(g["kinds"], np.asarray(theta0), np.arange(P, dtype=np.int32),
                         np.tile([-np.inf, np.inf], (P, 1)) if bounds is None else bounds, mean_kind=MEAN_LINEAR)
    else:
        engine.set_lightcurves(t, y, dy + 1e-12, y_offset=np.asarray(g["y_offset"]))
        engine.set_model(g["kinds"], np.concatenate([theta0, [0.0]]), np.arange(P, dtype=np.int32),
                         np.tile([-np.inf, np.inf], (P + 1, 1)) if bounds is None else bounds)
    return t, y, dy


def fixture_normals(g, N):
    q = np.array([golden_util.fp32_column(np.random.default_rng(s).standard_normal(N)) for s in g["normal_seeds"]])
    assert [golden_util.col_sha(r) for r in q] == g["normal_sha256"], "%s: the normals are not the fixture's" % g["name"]
    return q


@pytest.mark.parametrize("name", list(GROUPS))
def test_draw_against_the_truth(engine, name):
    g, a = GROUPS[name], arrays(name)
    theta, lc, idx = a["theta"], a["lc"], a["idx"]
    t, y, dy = setup(engine, g, theta[0])
    N = y.shape[1]
    q = fixture_normals(g, N)
    out, status = engine.gp_draw(theta, lc_index=lc, normals=q)
    assert np.all(status == 0), "%s: statuses %s" % (name, status)
    nk = dense.n_kernel_params(g["kinds"])
    worst = 0.0
    for b in range(len(theta)):
        tt = t[lc[b]] if t.ndim == 2 else t
        d = np.max(dense.build_coeffs(g["kinds"], theta[b][:nk])[5], initial=0.0)
        factor = 1.0 if d * float(np.max(np.diff(tt))) >= 1.0e4 else 10.0
        s, e64 = a["scale"][b].astype(np.float64), a["c64err"][b].astype(np.float64)
        rho = float(np.max(e64 / s))
        tol = np.maximum(factor * rho, 64.0 * np.sqrt(N) * U) * s
        e = np.abs(out[b][idx] - a["T"][b])
        assert not np.any(np.isnan(out[b]))
        w = int(np.argmax(e / tol))
        print("\ngp-draw truth %-28s row %d (factor %2d): worst e/tol %.3g at sample %d (rho %.3g, floor %.3g)"
              % (name, b, factor, e[w] / tol[w], idx[w], rho, 64.0 * np.sqrt(N) * U))
        assert np.all(e <= tol), "%s row %d sample %d: |y - T| = %.3e > %.3e" % (name, b, idx[w], e[w], tol[w])
        worst = max(worst, float(e[w] / tol[w]))
    WORST[name] = worst
    print("\ngp-draw truth %-28s worst ratio of the group %.3g; overall so far %.3g" % (name, worst, max(WORST.values())))


def batch_of_37(engine):
    """37 rows of typical/complex4+real on two light curves, two outside the prior box, one whose covariance is not
    positive definite in float64 (a real term of amplitude e^80, c = e^-40) -- the batch of
    tests/test_predict_vs_quad_gpu.py"""
    g, a = GROUPS["typical/complex4+real"], arrays("typical/complex4+real")
    t, y, dy = golden_util.quad_lightcurve(dict(g["recipes"][0], L=2))
    P = a["theta"].shape[1]
    bounds = np.vstack([np.tile([-100.0, 100.0], (P, 1)), [[-np.inf, np.inf]]])
    engine.set_lightcurves(t, y, dy + 1e-12, y_offset=y.mean(axis=1))
    engine.set_model(g["kinds"], np.concatenate([a["theta"][0], [0.0]]), np.arange(P, dtype=np.int32), bounds)
    rng = np.random.default_rng(7)
    rows, want = [], []
    for i in range(37):
        r = a["theta"][0] + 0.05 * rng.uniform(-1.0, 1.0, P)
        st = _engine.ST_OK
        if i in (5, 22):
            r[i % P] = 101.0 + i
            st = _engine.ST_PRIOR
        elif i == 13:
            r[4], r[5] = 80.0, -40.0
            st = _engine.ST_NOTPD
        rows.append(r)
        want.append(st)
    lc = (np.arange(37) * 7 % 3 % 2).astype(np.int32)
    return np.array(rows), lc, want, len(t)


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def test_rows_are_batch_invariant_with_given_normals(engine):
    theta, lc, want, N = batch_of_37(engine)
    q = np.random.default_rng(11).standard_normal((37, N))
    y, status = engine.gp_draw(theta, lc_index=lc, normals=q)
    assert list(status) == want, "statuses %s, expected %s" % (list(status), want)
    bad = np.array(want) != _engine.ST_OK
    assert np.all(np.isnan(y[bad])) and np.all(np.isfinite(y[~bad]))
    for b in range(37):
        y1, s1 = engine.gp_draw(theta[b:b + 1], lc_index=lc[b:b + 1], normals=q[b:b + 1])
        assert s1[0] == status[b] and same(y1[0], y[b]), "row %d differs alone and in the batch of 37" % b


def test_philox_rows_do_not_depend_on_the_batch(engine):
    """the same (seed, global index, theta, light curve) gives the same row for B = 1, 37, 257 and under
    set_stream_base(k) with the row at position b - k; bad rows keep status and NaN and do not disturb the others"""
    theta, lc, want, N = batch_of_37(engine)
    seed = 0x1234567890ABCDEF
    try:
        engine.set_stream_base(0)
        y, status = engine.gp_draw(theta, lc_index=lc, seed=seed)
        assert list(status) == want
        bad = np.array(want) != _engine.ST_OK
        assert np.all(np.isnan(y[bad])) and np.all(np.isfinite(y[~bad]))
        pick = np.arange(257) % 37
        big, sb = engine.gp_draw(theta[pick], lc_index=lc[pick], seed=seed)
        assert same(big[:37], y) and list(sb[:37]) == want
        assert not same(big[37], big[0])            # another global index: another draw of the same theta
        for b in (0, 5, 13, 14, 36):
            engine.set_stream_base(b)
            y1, s1 = engine.gp_draw(theta[b:b + 1], lc_index=lc[b:b + 1], seed=seed)
            assert s1[0] == status[b] and same(y1[0], y[b]), "row %d differs alone (B = 1) and in the batch" % b
        engine.set_stream_base(20)
        part, sp = engine.gp_draw(theta[20:], lc_index=lc[20:], seed=seed)
        assert same(part, y[20:]) and list(sp) == want[20:]
        other, _ = engine.gp_draw(theta[20:], lc_index=lc[20:], seed=seed + 1)
        assert not same(other[0], y[20])
    finally:
        engine.set_stream_base(0)


def test_rows_across_a_slab_boundary(engine):
    """N = 2e5: 1.6 MB a row, slabs of 128 rows (the multiple of 64 within 256 MiB); rows 127, 128 and 129 of a batch of 130 equal the row alone,
    with the caller's normals and with the device's"""
    g, a = GROUPS["headline/n200000"], arrays("headline/n200000")
    t, y, dy = setup(engine, g, a["theta"][0])
    N = len(t)
    assert (1 << 28) // (N * 8) // 64 * 64 == 128      # rows of a slab: whole workgroups within 256 MiB of draws
    theta = np.tile(a["theta"][0], (130, 1))
    q = fixture_normals(g, N)
    alone, s1 = engine.gp_draw(theta[:1], normals=q)
    assert s1[0] == 0
    out, status = engine.gp_draw(theta, normals=np.tile(q, (130, 1)))
    assert np.all(status == 0)
    for b in (0, 63, 127, 128, 129):
        assert same(out[b], alone[0]), "row %d differs from the row alone" % b
    try:
        engine.set_stream_base(0)
        out, status = engine.gp_draw(theta, seed=5)
        for b in (127, 128, 129):
            engine.set_stream_base(b)
            alone, s1 = engine.gp_draw(theta[:1], seed=5)
            assert same(out[b], alone[0]), "Philox row %d differs from the row alone" % b
    finally:
        engine.set_stream_base(0)


def test_device_normals_are_the_replayed_normals(engine):
    """(3) of the module docstring: a white model gives the normals back by one division; a correlated one (the null
    model at N = 1000) through the replay's inverse, at the floor of the truth test"""
    N = 1001                                       # odd: the last Philox block gives one normal only
    t, y, dy = synth.make_lightcurves(N, 1, seed=41)
    engine.set_lightcurves(t, y, dy + 1e-12)
    engine.set_model([5], np.array([-0.3, 0.0]), np.array([0], dtype=np.int32), np.tile([-np.inf, np.inf], (2, 1)))
    base, seed = (1 << 31) - 2, 0xFEEDFACE12345        # the largest stream bases: the draws' indices pass 2^31
    try:
        engine.set_stream_base(base)
        out, status = engine.gp_draw(np.full((3, 1), -0.3), seed=seed)
        assert np.all(status == 0)
        d = (dy[0] + 1e-12) ** 2 + np.exp(2.0 * -0.3)
        worst = 0.0
        for b in range(3):
            want = R.philox_normals(seed, base + b, N)
            r = R.philox_blocks(seed, base + b, N)
            rad = np.repeat(np.sqrt(-2.0 * np.log(1.0 - R.philox_replay.u01(r[0], r[1]))), 2)[:N]
            e = np.abs(out[b] / np.sqrt(d) - want)
            worst = max(worst, float(np.max(e / (U * rad))))
            assert np.all(e <= 16.0 * U * rad), "draw %d: normals off by %.1f u rad" % (b, np.max(e / (U * rad)))
        print("\ngp-draw normals: device against replayed Box-Muller, worst %.2f u rad (bound 16)" % worst)
        # a correlated model
        kinds = synth.NULL_MODEL
        th = synth.truth(kinds)
        P = len(th)
        engine.set_model(kinds, np.concatenate([th, [0.0]]), np.arange(P, dtype=np.int32), np.tile([-np.inf, np.inf], (P + 1, 1)))
        out, status = engine.gp_draw(np.tile(th, (2, 1)), seed=seed)
        assert np.all(status == 0)
        coeffs = dense.build_coeffs(kinds, th)
        fac = R.factor(t, R.diagonal(dy[0], coeffs), coeffs)
        back = R.whiten(t, dy[0], coeffs, out, factors=fac)
        for b in range(2):
            want = R.philox_normals(seed, base + b, N)
            s = R.scale_at(t, coeffs, fac, want, np.arange(N))
            tol = 64.0 * np.sqrt(N) * U * s / np.sqrt(fac[3]) + 16.0 * U * np.abs(want)
            e = np.abs(back[b] - want)
            print("\ngp-draw normals: correlated model draw %d, worst e/tol %.3g" % (b, np.max(e / tol)))
            assert np.all(e <= tol)
    finally:
        engine.set_stream_base(0)


@pytest.mark.parametrize("N", [10000, 200000])
def test_round_trip_through_the_likelihood(engine, N):
    kinds = synth.ALT_MODEL
    th = synth.truth(kinds)
    P = len(th)
    t, y, dy = synth.make_lightcurves(N, 1, seed=500 + N // 1000)
    q = np.random.default_rng(N).standard_normal(N)
    coeffs = dense.build_coeffs(kinds, th)
    # the host replay's own defect, through the quad-precision likelihood
    from oracle import quad
    yr = R.draw(t, dy[0], coeffs, q)
    full = np.concatenate([th, [0.0]])
    hi, lo, _, st = quad.loglike(t, np.vstack([yr, np.zeros(N)]), np.vstack([dy, dy]), kinds, np.tile(full, (2, 1)),
                                 lc_index=np.array([0, 1], dtype=np.int32))
    assert np.all(st == 0)
    half = 0.5 * float(q @ q)
    defect = abs(((hi[0] - hi[1]) + (lo[0] - lo[1])) + half)
    margin = max(10.0 * defect, 64.0 * np.sqrt(N) * U * (half + abs(hi[0])))
    engine.set_lightcurves(t, y, dy + 1e-12, y_offset=np.zeros(1))
    engine.set_model(kinds, full, np.arange(P, dtype=np.int32), np.tile([-np.inf, np.inf], (P + 1, 1)))
    out, status = engine.gp_draw(th[None, :], normals=q[None, :])
    assert status[0] == 0
    engine.set_lightcurves(t, np.vstack([out[0], np.zeros(N)]), np.vstack([dy, dy]) + 1e-12, y_offset=np.zeros(2))
    try:
        for mode, tag in ((0, "mtg_solve_kernel"), (1, "mtg_tp_")):
            engine.set_time_parallel(mode)
            engine.set_pipeline(0)
            lnl, st = engine.loglike(np.tile(th, (2, 1)), np.array([0, 1], dtype=np.int32), add_prior=False)
            assert np.all(st == 0) and tag in engine.last_solver, engine.last_solver
            miss = abs((lnl[0] - lnl[1]) + half)
            print("\ngp-draw round trip N=%d %-18s |lnL(y) - lnL(0) + q.q/2| = %.3e, margin %.3e (replay's defect %.3e)"
                  % (N, engine.last_solver, miss, margin, defect))
            assert miss <= margin
    finally:
        engine.set_time_parallel(2)
        engine.set_pipeline(2)


def test_distribution_of_the_device_draws(engine):
    kinds, theta, t, dy, coeffs = cpu.distribution_case()
    P = len(theta)
    engine.set_lightcurves(t, np.zeros((1, len(t))), dy[None, :] + 1e-12)
    engine.set_model(kinds, np.concatenate([theta, [0.0]]), np.arange(P, dtype=np.int32), np.tile([-np.inf, np.inf], (P + 1, 1)))
    engine.set_stream_base(0)
    y, status = engine.gp_draw(np.tile(theta, (4096, 1)), seed=cpu.DIST_SEED)
    assert np.all(status == 0)
    cpu.check_distribution(t, dy, coeffs, y)


def test_public_api():
    from mind_the_gaps_amd.gp import GP
    from mind_the_gaps_amd.gpmodelling import GPModelling
    from mind_the_gaps_amd.lightcurves import GappyLightcurve
    from mind_the_gaps_amd.models import DampedRandomWalk, Lorentzian
    rng = np.random.default_rng(3)
    N = 300
    t = np.sort(rng.uniform(0.0, 400.0, N))
    yobs = 50.0 + rng.standard_normal(N)
    dyobs = rng.uniform(0.2, 0.5, N)
    kernel = DampedRandomWalk(1.0, -1.0, bounds=[(-5.0, 5.0), (-5.0, 5.0)]) + \
        Lorentzian(0.5, 1.0, -0.5, bounds=[(-5.0, 5.0), (-2.0, 4.0), (-4.0, 2.0)])
    gp = GP(kernel, mean=50.0)
    gp.compute(t, dyobs + 1e-12)
    np.random.seed(7)
    three = gp.sample(3)
    assert three.shape == (3, N)
    eng, model = gp._bound_engine(np.zeros(N))
    np.random.seed(7)
    want, status = eng.gp_draw(np.tile(model.full[model.free_index], (3, 1)), normals=np.random.randn(3, N))
    assert np.all(status == 0) and np.array_equal(three, want + 50.0)
    assert gp.sample().shape == (N,)
    a, b = gp.sample(2, seed=9), gp.sample(2, seed=9)
    assert a.shape == (2, N) and np.array_equal(a, b) and not np.array_equal(a[0], a[1])
    assert abs(a.mean() - 50.0) < 5.0
    # generate_from_posteriors on a regular pattern with exposures (what the TK95 route needs): the case of
    # tests/golden/make_posterior_sims_golden.py, whose fixture holds the default route's output at the commit before
    # the method keyword existed
    model, lc = PG.case()
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        np.random.seed(5)
        sims = model.generate_from_posteriors(nsims=16, method="gp")
        assert len(sims) == 16
        for s in sims:
            assert isinstance(s, GappyLightcurve) and np.array_equal(s.times, lc.times) and np.array_equal(s.dy, lc.dy)
            assert s.y.shape == (300,) and np.all(np.isfinite(s.y))
        assert not np.array_equal(sims[0].y, sims[1].y)
        np.random.seed(5)
        again = model.generate_from_posteriors(nsims=16, method="gp")
        assert all(np.array_equal(a.y, b.y) for a, b in zip(sims, again))


def test_default_method_is_the_parents_output_bit_for_bit():
    """generate_from_posteriors(nsims=4) under np.random.seed(5) -- the default, Timmer & Koenig route -- returns the
    y and dy recorded on an MI355X at the commit before the method keyword existed
    (tests/golden/posterior_sims_golden.npz), bit for bit; so does an explicit method="tk95"."""
    gold = np.load(os.path.join(HERE, "golden", "posterior_sims_golden.npz"))
    model, lc = PG.case()
    assert np.array_equal(gold["times"], lc.times) and np.array_equal(gold["samples"], model._mcmc_samples), \
        "the light curve or the posterior samples are not the fixture's"
    y, dy = PG.default_route(model)
    assert y.shape == gold["y"].shape == (PG.NSIMS, 300)
    assert np.array_equal(y, gold["y"]), "default route: y differs from the parent's in %d of %d values" % (
        int(np.sum(y != gold["y"])), y.size)
    assert np.array_equal(dy, gold["dy"]), "default route: dy differs from the parent's"
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        np.random.seed(PG.SEED)
        sims = model.generate_from_posteriors(nsims=PG.NSIMS, method="tk95")
    assert np.array_equal(np.array([s.y for s in sims]), gold["y"]) and np.array_equal(np.array([s.dy for s in sims]), gold["dy"])
