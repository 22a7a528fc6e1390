"""Engine.gp_cond_draw / GP.sample_conditional / GPModelling.sample_conditional (mtg_gp_cond_draw: Matheron's rule on the
device, a joint prior draw on the merged series and then mtg_predict_at's conditional mean of y - y~).  The host replay is
tests/gp_cond_draw_replay.py; the cases come from tests/test_gp_cond_draw_cpu.py.

1. The draw is an affine map of its normals.  With all normals zero it is mtg_predict_at's mean, held to that entry's
   quad bound (tests/test_predict_at_vs_quad_gpu.quad_bounds) against the quad truth.  One row per unit vector of the
   N + M' effective normals gives A, and A A^T must be K_** - K_* K^-1 K_*^T of mpmath within max(10 rho, 64 sqrt(N + M) u) s:
   rho is the same ratio for the float64 numpy evaluation of the dense formula, and s_ij the sum of the magnitudes that
   enter the entry on either side -- |K_**| + |K_*| |K^-1 K_*^T| of the formula, and sum_k a_ik a_jk with
   a = |Lj_new| + |C| |Lj_epochs| + |mu| for A, whose entries the test itself forms as differences from the zero-normal row.
2. The device agrees with the replay at N = 65, M = 40 (one checkpoint boundary inside the series) within
   64 sqrt(N + M) u s, s the sum of the magnitudes that enter a value (gp_cond_draw_replay.dense_draw).
3. A row is bit for bit the same alone, in a batch of 37 with a mixed lc_index, across a slab boundary, with ts
   permuted, and -- with the device's normals -- under set_stream_base; the device's normals are the replayed ones:
   fed back as the caller's normals they change a value by at most sum_k |A_k| 16 u rad_k (the bound of
   tests/test_gp_draw_gpu.py on a normal, through the map) plus the floor of (2).
5. 4096 device draws at N = 64, M = 32 have mtg_predict_at's mean and variance within 5 standard errors; with error bars
   of 1e-6 of the amplitude a draw at the epochs gives the data back to 6 of those error bars (the conditional
   variance there is below sigma^2).
6. Edges and 7. the Python layers."""
import numpy as np
import pytest

import gp_cond_draw_replay as CR
import test_gp_cond_draw_cpu as cpu
import test_mean_profile_gpu as mp_tests
import test_predict_at_vs_quad_gpu as pq
from mind_the_gaps_amd import engine as _engine
from mind_the_gaps_amd import synthetic as synth
from oracle import dense

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
same = pq.same


def bind(engine, kinds, theta, t, y, dy, bounds=None):
    """one light curve with its average as y_offset, every kernel parameter free -> that average"""
    P = len(theta)
    off = float(np.mean(y))
    engine.set_lightcurves(t, np.atleast_2d(y), np.atleast_2d(dy) + 1e-12, y_offset=np.array([off]))
    engine.set_model(kinds, np.concatenate([theta, [0.0]]), np.arange(P, dtype=np.int32),
                     np.tile([-np.inf, np.inf], (P + 1, 1)) if bounds is None else bounds)
    return off


@pytest.mark.parametrize("rank", sorted(cpu.RANKS))
def test_mean_and_covariance_of_the_affine_map(engine, rank):
    kinds, theta, t, y, dy, ts, coeffs = cpu.small_case(rank)
    N, M = len(t), len(ts)
    off = bind(engine, kinds, theta, t, y, dy)
    tu, first, inv, order, is_new = CR.merge(t, ts)
    Mu = len(tu)
    eff = np.concatenate([np.arange(N), N + first])               # the normals that are read
    q = np.zeros((1 + N + Mu, N + M))
    q[1 + np.arange(N + Mu), eff] = 1.0
    out, status = engine.gp_cond_draw(np.tile(theta, (len(q), 1)), ts, normals=q)
    assert np.all(status == 0) and "mtg_gp_cond_draw_kernel<%d>" % rank == engine.last_solver
    assert np.array_equal(out[:, 0], out[:, 5]), "the duplicated pair differs"
    # the mean: mtg_predict_at's quad bound, against the quad truth
    _, var, st = engine.predict_at(theta[None, :], tu)
    pq.quad_bounds("gp_cond_draw mean rank %d" % rank, N, t, y, dy, kinds, np.append(theta, off), tu, [(out[0][first] + off, var[0])])
    # the covariance
    A = (out[1:] - out[0])[:, first].T                            # [Mu][N + Mu], columns in the order of eff
    got = A @ A.T
    T = CR.mp_cond_cov(t, dy + 1e-12, coeffs, ts)
    c64, s_formula = CR.cond_cov(t, dy + 1e-12, coeffs, ts)
    a = CR.dense_map(t, dy + 1e-12, coeffs, ts)[1]
    mu0, _ = CR.dense_draw(t, y - off, dy + 1e-12, coeffs, lambda x: np.zeros(len(x)), tu, np.zeros(N + Mu))
    a = a + np.abs(mu0)[:, None]
    s = s_formula + a @ a.T
    rho = float(np.max(np.abs(c64 - T) / s))
    tol = max(10.0 * rho, 64.0 * np.sqrt(N + M) * U) * s
    e = np.abs(got - T)
    print("\ngp-cond-draw covariance rank %d: worst |A A^T - T| / tol = %.3g (rho %.3g, floor %.3g)"
          % (rank, np.max(e / tol), rho, 64.0 * np.sqrt(N + M) * U))
    assert np.all(e <= tol)


@pytest.mark.parametrize("rank", sorted(cpu.RANKS))
def test_device_is_the_replay_across_a_checkpoint(engine, rank):
    kinds = cpu.RANKS[rank]
    theta = synth.truth(kinds)
    N, M = 65, 40
    t, y, dy = synth.make_lightcurves(N, 1, seed=650 + rank)
    rng = np.random.default_rng(rank)
    ts = rng.uniform(t[0] - 10.0, t[-1] + 10.0, M)
    ts[7], ts[11], ts[30] = t[63], t[64], ts[2]                   # on the epochs around the checkpoint, and a pair
    off = bind(engine, kinds, theta, t, y[0], dy[0])
    q = rng.standard_normal((2, N + M))
    out, status = engine.gp_cond_draw(np.tile(theta, (2, 1)), ts, normals=q)
    assert np.all(status == 0)
    coeffs = dense.build_coeffs(kinds, theta)
    zero = lambda x: np.zeros(len(x))
    _, s = CR.dense_draw(t, y[0] - off, dy[0] + 1e-12, coeffs, zero, ts, q)
    for b in range(2):
        want = CR.draw(t, y[0] - off, dy[0] + 1e-12, coeffs, zero, ts, q[b])
        e = np.abs(out[b] - want) / (64.0 * np.sqrt(N + M) * U * s[b])
        print("\ngp-cond-draw device against replay rank %d row %d: worst e/floor %.3g" % (rank, b, e.max()))
        assert np.all(e <= 1.0)


def test_rows_are_invariant_bit_for_bit(engine):
    g, a, t, y, dy, P, bounds, theta, want, lc = pq.batch_of_37()
    engine.set_lightcurves(t, y, dy + 1e-12, y_offset=y.mean(axis=1))
    engine.set_model(g["kinds"], np.concatenate([a["theta"][0][:P], [0.0]]), np.arange(P, dtype=np.int32), bounds)
    N = len(t)
    ts = pq.golden_util.new_times(t, 4242)
    ts = np.concatenate([ts, ts[5:8]])                            # duplicates
    M = len(ts)
    q = np.random.default_rng(3).standard_normal((37, N + M))
    out, status = engine.gp_cond_draw(theta, ts, lc_index=lc, normals=q)
    assert list(status) == want, "statuses %s, expected %s" % (list(status), want)
    bad = np.array(want) != _engine.ST_OK
    assert np.all(np.isnan(out[bad])) and np.all(np.isfinite(out[~bad]))
    assert same(out[:, 5:8], out[:, -3:])
    for b in range(37):
        o1, s1 = engine.gp_cond_draw(theta[b:b + 1], ts, lc_index=lc[b:b + 1], normals=q[b:b + 1])
        assert s1[0] == status[b] and same(o1[0], out[b]), "row %d differs alone and in the batch of 37" % b
    # ts permuted, the new times' normals with it (the first of a pair stays the first)
    perm = np.concatenate([np.random.default_rng(4).permutation(M - 3), M - 3 + np.arange(3)])
    o2, s2 = engine.gp_cond_draw(theta, ts[perm], lc_index=lc, normals=np.hstack([q[:, :N], q[:, N:][:, perm]]))
    assert list(s2) == want and same(o2, out[:, perm])
    # the device's normals: B, the stream base and the order of ts do not matter
    seed = 0x1234567890ABCDEF
    try:
        engine.set_stream_base(0)
        ph, sp = engine.gp_cond_draw(theta, ts, lc_index=lc, seed=seed)
        assert list(sp) == want and np.all(np.isfinite(ph[~bad]))
        o3, _ = engine.gp_cond_draw(theta, ts[::-1].copy(), lc_index=lc, seed=seed)
        assert same(o3[:, ::-1], ph)
        for k in (0, 5, 13, 14, 36):
            engine.set_stream_base(k)
            o1, s1 = engine.gp_cond_draw(theta[k:k + 1], ts, lc_index=lc[k:k + 1], seed=seed)
            assert s1[0] == status[k] and same(o1[0], ph[k]), "row %d differs alone (B = 1) and in the batch" % k
        engine.set_stream_base(0)
        other, _ = engine.gp_cond_draw(theta[:1], ts, lc_index=lc[:1], seed=seed + 1)
        assert not same(other[0], ph[0])
        # ... and they are the replayed normals
        kinds = g["kinds"]
        for b in (0, 36):
            qd, rad = CR.device_normals(seed, b, N, ts)
            given, _ = engine.gp_cond_draw(theta[b:b + 1], ts, lc_index=lc[b:b + 1], normals=qd[None, :])
            coeffs = dense.build_coeffs(kinds, theta[b][:dense.n_kernel_params(kinds)])
            tb, yb, db = (t[lc[b]] if t.ndim == 2 else t), y[lc[b]], dy[lc[b]] + 1e-12
            tu, first, inv, order, is_new = CR.merge(tb, ts)
            absA = CR.dense_map(tb, db, coeffs, ts)[1]
            radm = np.concatenate([rad[:N], rad[N:][first]])[order]
            _, s = CR.dense_draw(tb, yb - yb.mean(), db, coeffs, lambda x: np.zeros(len(x)), ts, qd)
            tol = (absA @ (16.0 * U * radm))[inv] + 64.0 * np.sqrt(N + M) * U * s
            e = np.abs(ph[b] - given[0])
            print("\ngp-cond-draw normals row %d: device against replayed Box-Muller, worst e/tol %.3g" % (b, np.max(e / tol)))
            assert np.all(e <= tol)
    finally:
        engine.set_stream_base(0)


def test_rows_across_a_slab_boundary(engine):
    """phase/j10 (N = 20011, J = 10: 5.3 MB a row of stored generators), 210 rows -> two slabs of the 1 GiB workspace: rows
    on either side of the boundary are the rows alone"""
    name = "phase/j10"
    a = pq.arrays(name)
    t, y, dy = pq.setup(engine, name, a["theta"][0])
    rows = np.array([pq.free(name, r) for r in a["theta"]])
    Bs = (1 << 30) // (len(t) * 33 * 8)
    assert Bs < 209
    pick = np.arange(210) % len(rows)
    try:
        engine.set_stream_base(0)
        out, status = engine.gp_cond_draw(rows[pick], a["ts"], seed=5)
        assert np.all(status == 0) and np.all(np.isfinite(out))
        for b in (Bs - 1, Bs, 209):
            engine.set_stream_base(b)
            alone, s1 = engine.gp_cond_draw(rows[pick[b]:pick[b] + 1], a["ts"], seed=5)
            assert same(alone[0], out[b]), "row %d differs from the row alone" % b
    finally:
        engine.set_stream_base(0)


def test_a_slab_bounded_by_the_new_times(engine):
    """N = 12, M = 30 000: a row keeps 1152 bytes of generators and (N + 2 M' + M) 8 = 720 096 of its own, so the 1 GiB
    budget takes 1488 rows; rows on either side of that boundary in a batch of 1500 are the rows alone"""
    kinds, theta, t, y, dy, ts, coeffs = cpu.small_case(3)
    bind(engine, kinds, theta, t, y, dy)
    M = 30000
    ts = np.linspace(t[0] - 5.0, t[-1] + 5.0, M)
    Bs = (1 << 30) // (12 * 12 * 8 + (12 + 3 * M) * 8)
    assert Bs == 1488
    try:
        engine.set_stream_base(0)
        out, status = engine.gp_cond_draw(np.tile(theta, (1500, 1)), ts, seed=7)
        assert np.all(status == 0) and np.all(np.isfinite(out))
        for b in (Bs - 1, Bs, 1499):
            engine.set_stream_base(b)
            alone, s1 = engine.gp_cond_draw(theta[None, :], ts, seed=7)
            assert same(alone[0], out[b]), "row %d differs from the row alone" % b
    finally:
        engine.set_stream_base(0)


def test_distribution_of_the_device_draws(engine):
    kinds, theta, t, y, dy, ts = cpu.distribution_case()
    bind(engine, kinds, theta, t, y, dy)
    engine.set_stream_base(0)
    draws, status = engine.gp_cond_draw(np.tile(theta, (4096, 1)), ts, seed=cpu.DIST_SEED)
    assert np.all(status == 0)
    mu, var, st = engine.predict_at(theta[None, :], ts)
    cpu.check_distribution(draws, mu[0], var[0])


def test_tiny_errors_give_the_data_back_at_the_epochs():
    """the t=None path of GP.sample_conditional"""
    from mind_the_gaps_amd.gp import GP
    i, kernel, _ = mp_tests.python_problem(65)
    t, y = mp_tests.arr(i, "t"), mp_tests.arr(i, "y")[0]
    sigma = 1e-6 * np.sqrt(float(kernel.get_value(0.0)))            # 1e-6 of the amplitude
    gp = GP(kernel, mean=float(np.mean(y)))
    gp.compute(t, np.full(len(t), sigma))
    out = gp.sample_conditional(y, size=3, seed=1)
    assert out.shape == (3, len(t)) and not np.array_equal(out[0], out[1])
    print("\ngp-cond-draw at the epochs: worst |y* - y| / sigma = %.3g" % (np.max(np.abs(out - y)) / sigma))
    assert np.all(np.abs(out - y) <= 6.0 * sigma)


def test_edges(engine):
    kinds, theta, t, y, dy, ts, coeffs = cpu.small_case(3)
    N = len(t)
    P = len(theta)
    bounds = np.vstack([np.tile([-100.0, 100.0], (P, 1)), [[-np.inf, np.inf]]])
    off = bind(engine, kinds, theta, t, y, dy, bounds)
    out, status = engine.gp_cond_draw(theta[None, :], np.empty(0))
    assert out.shape == (1, 0) and list(status) == [0]
    for side in (t[0] - np.array([5.0, 1.0, 30.0]), t[-1] + np.array([5.0, 1.0, 30.0])):
        out, status = engine.gp_cond_draw(theta[None, :], side, normals=np.zeros((1, N + 3)))
        mu, _, st = engine.predict_at(theta[None, :], side)
        assert status[0] == 0 and np.array_equal(out, mu)
        out, status = engine.gp_cond_draw(theta[None, :], side, seed=3)
        assert status[0] == 0 and np.all(np.isfinite(out)) and not np.array_equal(out, mu)
    with pytest.raises(_engine.EngineError) as err:
        engine.gp_cond_draw(theta[None, :], np.array([1.0, np.nan]))
    assert err.value.code == _engine.E_ARG
    outside = theta.copy()
    outside[0] = 150.0
    out, status = engine.gp_cond_draw(np.array([theta, outside]), ts, seed=3)
    assert list(status) == [_engine.ST_OK, _engine.ST_PRIOR] and np.all(np.isfinite(out[0])) and np.all(np.isnan(out[1]))
    # rank 0: the latent process is zero
    engine.set_model([synth.K_JITTER], np.array([-0.3, 0.0]), np.array([0], dtype=np.int32), np.tile([-np.inf, np.inf], (2, 1)))
    out, status = engine.gp_cond_draw(np.array([[-0.3]]), ts, seed=3)
    assert status[0] == 0 and np.array_equal(out, np.zeros((1, len(ts)))) and engine.last_solver == "mtg_gp_cond_draw_kernel<0>"
    # a profile mean is the host layer's (the cases of tests/test_mean_profile_gpu.py)
    for kind in (2, 3, 4):
        th, _ = mp_tests.setup(engine, mp_tests.index("j1/kind%d/n3" % kind))
        with pytest.raises(_engine.EngineError) as err:
            engine.gp_cond_draw(th, np.array([51.0, 52.5]))
        assert err.value.code == _engine.E_UNSUPPORTED and mp_tests.NAMES[kind] in str(err.value), str(err.value)


def test_python_gp():
    """shapes, seeds, and a SineModel mean against the zero-mean GP on y - mean(t) (test_python_gp of
    tests/test_mean_profile_gpu.py)"""
    from mind_the_gaps_amd.gp import GP
    i, kernel, mean = mp_tests.python_problem(65)
    t, y, dy = mp_tests.arr(i, "t"), mp_tests.arr(i, "y")[0], mp_tests.arr(i, "dy")[0]
    N = len(t)
    ts = np.linspace(t[0] - 1.0, t[-1] + 1.0, 23)
    gp = GP(kernel, mean=mean, fit_mean=True)
    gp.compute(t, dy + 1e-12)
    one, five = gp.sample_conditional(y, ts, seed=4), gp.sample_conditional(y, ts, size=5, seed=4)
    assert one.shape == (23,) and five.shape == (5, 23) and np.array_equal(five[0], one)
    assert gp.sample_conditional(y, seed=4).shape == (N,) and gp.sample_conditional(y, ts, size=0).shape == (0, 23)
    np.random.seed(8)
    a = gp.sample_conditional(y, ts, size=2)
    np.random.seed(8)
    assert np.array_equal(a, gp.sample_conditional(y, ts, size=2)) and not np.array_equal(a[0], a[1])
    zero = GP(kernel, mean=0.0)
    zero.compute(t, dy + 1e-12)
    want = zero.sample_conditional(y - mean.get_value(t), ts, size=5, seed=4) + mean.get_value(ts)
    np.testing.assert_allclose(five, want, rtol=1e-12, atol=0)


def test_python_gpmodelling():
    import warnings
    from mind_the_gaps_amd.gpmodelling import GPModelling
    from mind_the_gaps_amd.lightcurves import GappyLightcurve
    i, kernel, _ = mp_tests.python_problem(129)
    lc = GappyLightcurve(mp_tests.arr(i, "t"), mp_tests.arr(i, "y")[0], mp_tests.arr(i, "dy")[0])
    np.random.seed(4)
    model = GPModelling(lc, kernel)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model.derive_posteriors(walkers=16, max_steps=40, convergence_steps=20, progress=False)
    ts = np.linspace(lc.times[0] - 3.0, lc.times[-1] + 3.0, 50)
    a = model.sample_conditional(ts, nsims=6, seed=11)
    assert a.shape == (6, 50) and np.all(np.isfinite(a)) and not np.array_equal(a[0], a[1])
    assert np.array_equal(a, model.sample_conditional(ts, nsims=6, seed=11))
    assert not np.array_equal(a, model.sample_conditional(ts, nsims=6, seed=12))
    b = model.sample_conditional(ts, nsims=3, parameters=model.max_parameters, seed=11)
    assert b.shape == (3, 50) and np.all(np.isfinite(b)) and not np.array_equal(b[0], b[1])
    assert model.sample_conditional(nsims=2, seed=1).shape == (2, len(lc.times))
