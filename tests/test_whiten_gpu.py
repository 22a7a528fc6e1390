"""Engine.whiten / GP.whiten / GPModelling.whitened_residuals and residual_diagnostics (mtg_whiten_kernel: the one-step-ahead
residuals q = D^-1/2 L^-1 (y - mean), the inverse of the draw; mtg_whiten_ks_kernel, mtg_whiten_acf_kernel) on the
device.  The fixture tests/golden/whiten_golden.npz is made by tests/golden/make_whiten_golden.py (the recurrence in
mpmath at 40 digits, checked there against the mpmath dense Cholesky); the host replay is tests/whiten_replay.py.

1. Truth.  With T the truth, c64 the stored float64 baseline (celerite's phase at the absolute time),
   s_n = (|r_n| + sum_i |U_ni f_ni|) / sqrt(D_n) and u = 2^-53, every stored sample satisfies
       |q - T| <= max(10 rho, 64 sqrt(N) u) s,   rho = max over the row's stored samples of |c64 - T| / s
   with 1 in place of 10 on rows of d max(dx) >= 1e4 rad: the rule of tests/test_predict_vs_quad_gpu.py.  stats[1] and
   stats[2] are held to the same rule with the sum of their terms' magnitudes as the scale.
2. Tiles and batches: N in {1, 2, 31, 32, 33, 64, 97}, B in {1, 37, 65, 130}; a given y and the resident y of the same data
   give the same bits; a row is bit for bit the same alone, in the batch of 37 of tests/test_gp_draw_gpu.py (two rows
   outside the prior, one not positive definite: NaN in q, stats and acf, with their statuses) and across a slab
   boundary (the slab's budget follows set_window_bytes: two rows' worth makes slabs of 64); q == NULL gives the same stats
   and acf.
3. whiten(gp_draw(normals = q0)) recovers q0 within twice the floor tests/test_gp_draw_gpu.py holds recovered normals
   to, 64 sqrt(N) u s_n / sqrt(D_n) (s_n the draw's scale): both kernels contribute.  Ranks 1, 3, 6, 10; N = 257.
4. -1/2 (stats[1] + stats[2] + N ln 2 pi) against engine.loglike of the same rows (headline model, N = 1e4, B = 4 and
   300: the time-parallel and the serial dispatch), within 64 sqrt(N) u (stats[1] / 2 + |stats[2]| / 2 + N ln 2 pi / 2).
5. KS: max(stats[5], stats[6]) against the statistic of the device's own q with mpmath.ncdf at 30 digits, N = 257 and
   1000, within (2 E + 8) u: Phi <= 1 through erfc (E ulp of a value below 2), i / N, one subtraction.  No accuracy
   table of OCML ships with the ROCm installation, so E is measured: scripts/whiten_probe.py compares the device's erfc
   with mpmath at the 3771 values of q the device returns for this test's own rows (whiten_replay.ks_case) and finds
   2.13 ulp of the value (the line "E:" of profiles/whiten_probe.txt; 2.09 over 4096 other q in [-8, 8]).  E = 3: the
   next integer, 40 per cent above the figure, for the q of the tile and public-API tests, which hold their KS
   distances to the same (2 E + 8) u = 14 u.  The p-value agrees with scipy's ks_1samp on that q to 1e-9; a row whose q are all
   equal is included.
6. ACF against np.correlate on the device's q, K in {1, N - 1, N // 4}, N = 97 and 1000: |delta| <= 4 N u (both sides sum
   at most N products whose absolute sum over sum q^2 is <= 1).  K = 0, K = N, K < 0 with acf are MTG_E_ARG.
7. The public API on a tutorial-like light curve with [B][P] rows; the notebook's three lines on whitened_residuals
   give residual_diagnostics' numbers; the sine-mean route; and the calibration: over 512 device draws at the true
   parameters (N = 256) the KS p-values of whiten are uniform (KS test of the p-values, level 1e-4, fixed seed)."""
import ctypes
import json
import os

import numpy as np
import pytest

import golden_util
import gp_draw_replay as R
import test_gp_draw_gpu as G
import whiten_replay as WR
from mind_the_gaps_amd import engine as _engine
from mind_the_gaps_amd import synthetic as synth
from mind_the_gaps_amd.engine import MEAN_LINEAR
from oracle import dense

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
U = 2.0 ** -53
FIX = np.load(os.path.join(HERE, "golden", "whiten_golden.npz"))
GROUPS = {g["name"]: g for g in json.loads(bytes(FIX["manifest"]))["groups"]}
WORST = {}
ERFC_ULP = 3.0         # measured 2.13, profiles/whiten_probe.txt, line "E:": (5) of the module docstring


def arrays(name):
    key = name.replace("/", ".") + "/"
    return {k[len(key):]: FIX[k] for k in FIX.files if k.startswith(key)}


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def setup(engine, g, theta0):
    """the fixture's light curve resident with its y_offset, the model with every parameter free -> (t, y, dy)"""
    t, y, dy = golden_util.quad_lightcurve(g["recipes"][0])
    assert golden_util.lightcurve_sha256(t, y, dy) == g["sha256"][0], "%s: the light curve is not the fixture's" % g["name"]
    P = len(theta0)
    engine.set_window_bytes(golden_util.FULL_WINDOW)
    if g["mean_kind"] == 1:
        engine.set_lightcurves(t, y, dy + 1e-12)
        engine.set_model(g["kinds"], np.asarray(theta0), np.arange(P, dtype=np.int32), np.tile([-np.inf, np.inf], (P, 1)),
                         mean_kind=MEAN_LINEAR)
    else:
        engine.set_lightcurves(t, y, dy + 1e-12, y_offset=np.asarray(g["y_offset"]))
        engine.set_model(g["kinds"], np.concatenate([theta0, [0.0]]), np.arange(P, dtype=np.int32),
                         np.tile([-np.inf, np.inf], (P + 1, 1)))
    return t, y, dy


@pytest.mark.parametrize("name", list(GROUPS))
def test_whiten_against_the_truth(engine, name):
    g, a = GROUPS[name], arrays(name)
    theta, idx = a["theta"], a["idx"]
    t, y, dy = setup(engine, g, theta[0])
    N = len(t)
    q, _, st, status = engine.whiten(theta)
    assert status[0] == 0 and not np.any(np.isnan(q))
    given, _, st_given, _ = engine.whiten(theta, y=y[:1] - g["y_offset"][0])
    assert same(given, q) and same(st_given, st), "%s: a given y and the resident y differ" % name
    nk = dense.n_kernel_params(g["kinds"])
    d = np.max(dense.build_coeffs(g["kinds"], theta[0][:nk])[5], initial=0.0)
    factor = 1.0 if d * float(np.max(np.diff(t))) >= 1.0e4 else 10.0
    s, e64 = a["scale"][0].astype(np.float64), a["c64err"][0].astype(np.float64)
    rho, floor = float(np.max(e64 / s)), 64.0 * np.sqrt(N) * U
    tol = np.maximum(factor * rho, floor) * s
    e = np.abs(q[0][idx] - a["T"][0])
    w = int(np.argmax(e / tol))
    worst = float(e[w] / tol[w])
    # the two sums of the likelihood: scale = the sum of their terms' magnitudes, rho from the baseline's own sums
    sums, s64 = a["sums"][0], a["sums_c64err"][0]
    ratios = []
    for slot, truth, scale, err64 in ((1, sums[1], sums[1], s64[0]), (2, sums[2], sums[5], s64[1])):
        tol_s = max(factor * err64 / scale, floor) * scale
        ratios.append(abs(st[0][slot] - truth) / tol_s)
    print("\nwhiten truth %-22s worst e/tol %.3g at sample %d (rho %.3g, floor %.3g); sum q^2 %.3g, sum ln D %.3g of theirs"
          % (name, worst, idx[w], rho, floor, ratios[0], ratios[1]))
    WORST[name] = max(worst, *ratios)
    print("whiten truth %-22s worst ratio of the group %.3g; overall so far %.3g" % (name, WORST[name], max(WORST.values())))
    assert np.all(e <= tol), "%s sample %d: |q - T| = %.3e > %.3e" % (name, idx[w], e[w], tol[w])
    assert max(ratios) <= 1.0, "%s: sum q^2 and sum ln D at %s of their tolerances" % (name, ratios)


@pytest.mark.parametrize("N", [1, 2, 31, 32, 33, 64, 97])
def test_tiles_and_workgroups(engine, N):
    """partial tiles, a partial workgroup and two workgroups: every row of B = 37, 65, 130 equals the row alone, with the
    resident data and with the same data given; q == NULL changes neither stats nor acf"""
    kinds = synth.NULL_MODEL
    th = synth.truth(kinds)
    P = len(th)
    t, y, dy = synth.make_lightcurves(N, 3, seed=60 + N)
    off = y.mean(axis=1)
    engine.set_window_bytes(golden_util.FULL_WINDOW)
    engine.set_lightcurves(t, y, dy + 1e-12, y_offset=off)
    engine.set_model(kinds, np.concatenate([th, [0.0]]), np.arange(P, dtype=np.int32), np.tile([-np.inf, np.inf], (P + 1, 1)))
    K = N - 1 if N > 1 else 0
    rng = np.random.default_rng(N)
    theta = th[None, :] + 0.05 * rng.uniform(-1.0, 1.0, (130, P))
    lc = (np.arange(130) % 3).astype(np.int32)
    q, acf, st, status = engine.whiten(theta, lc_index=lc, lags=K)
    assert np.all(status == 0) and np.all(np.isfinite(q)) and np.all(np.isfinite(st))
    assert "mtg_whiten_kernel<3>" in engine.last_solver, engine.last_solver
    data = y[lc] - off[lc][:, None]
    gq, gacf, gst, _ = engine.whiten(theta, lc_index=lc, y=data, lags=K)
    assert same(gq, q) and same(gst, st) and (K == 0 or same(gacf, acf)), "given and resident y differ"
    nq, nacf, nst, _ = engine.whiten(theta, lc_index=lc, residuals=False, lags=K) if K else (None, None, None, None)
    if K:
        assert nq is None and same(nst, st) and same(nacf, acf), "q == NULL changes stats or acf"
    # stats alone: the sums are the same, the KS slots NaN (nothing of size N is stored)
    _, _, sums, _ = engine.whiten(theta, lc_index=lc, residuals=False, ks=False)
    with pytest.raises(ValueError):
        engine.whiten(theta, lc_index=lc, residuals=False)      # the KS distances are not dropped silently
    keep = [0, 1, 2, 3, 4, 7]
    assert same(sums[:, keep], st[:, keep]) and np.all(np.isnan(sums[:, 5:7]))
    for B in (1, 37, 65):
        for first in (0, 130 - B):
            rows = slice(first, first + B)
            q1, a1, s1, _ = engine.whiten(theta[rows], lc_index=lc[rows], lags=K)
            assert same(q1, q[rows]) and same(s1, st[rows]) and (K == 0 or same(a1, acf[rows])), "B = %d from row %d" % (B, first)
    if N > 1:      # against the replay's definitions, on the device's own q (exact up to the order of the sums)
        want = WR.acf(q[5], K)
        assert np.all(np.abs(acf[5] - want) <= 4.0 * N * U)
        dp, dm = WR.ks_distances(q[5])
        assert abs(st[5][5] - dp) <= (2 * ERFC_ULP + 8) * U and abs(st[5][6] - dm) <= (2 * ERFC_ULP + 8) * U


def test_batch_of_37_and_a_slab_boundary(engine):
    theta, lc, want, N = G.batch_of_37(engine)
    K = N // 4
    engine.set_window_bytes(golden_util.FULL_WINDOW)
    q, acf, st, status = engine.whiten(theta, lc_index=lc, lags=K)
    assert list(status) == want, "statuses %s, expected %s" % (list(status), want)
    bad = np.array(want) != _engine.ST_OK
    for out in (q, acf, st):
        assert np.all(np.isnan(out[bad])) and np.all(np.isfinite(out[~bad]))
    for b in range(37):
        q1, a1, s1, t1 = engine.whiten(theta[b:b + 1], lc_index=lc[b:b + 1], lags=K)
        assert t1[0] == status[b] and same(q1[0], q[b]) and same(a1[0], acf[b]) and same(s1[0], st[b]), \
            "row %d differs alone and in the batch of 37" % b
    # slabs of 64 rows: the budget of a slab is the window, here two rows' worth; 130 rows = 64 + 64 + 2
    pick = np.arange(130) % 37
    try:
        engine.set_window_bytes(N * 16)
        for kw in (dict(), dict(y=np.tile(np.linspace(-1.0, 1.0, N), (130, 1)))):
            ref = engine.whiten(theta, lc_index=lc, lags=K, **({} if not kw else dict(y=kw["y"][:37])))      # one slab
            big = engine.whiten(theta[pick], lc_index=lc[pick], lags=K, **kw)
            assert list(big[3][:37]) == want
            for b in (0, 13, 36, 63, 64, 65, 127, 128, 129):
                for k in range(3):
                    assert same(big[k][b], ref[k][b % 37]), "row %d, output %d differs across the slab boundary" % (b, k)
            nq = engine.whiten(theta[pick], lc_index=lc[pick], lags=K, residuals=False, **kw)
            assert same(nq[1], big[1]) and same(nq[2], big[2])
    finally:
        engine.set_window_bytes(golden_util.FULL_WINDOW)


@pytest.mark.parametrize("kinds,theta", [
    ([synth.K_DRW], synth.truth([synth.K_DRW])),
    (synth.NULL_MODEL, synth.truth(synth.NULL_MODEL)),
    (synth.ALT_MODEL, synth.truth(synth.ALT_MODEL)),
    ([synth.K_SHO] * 5, np.concatenate([synth.TRUTH[synth.K_SHO] + np.array([0.0, 0.3 * k, 0.5 * k]) for k in range(5)])),
], ids=["J1", "J3", "J6", "J10"])
def test_whiten_inverts_the_draw(engine, kinds, theta, request):
    # the instantiation each case must reach; celerite's rank 6 of the headline model is the device's 5 (the engine drops
    # the Lorentzian's null real term)
    rank = {"J1": 1, "J3": 3, "J6": 5, "J10": 10}[request.node.callspec.id]
    N = 257
    t, y, dy = synth.make_lightcurves(N, 1, seed=77)
    P = len(theta)
    engine.set_window_bytes(golden_util.FULL_WINDOW)
    engine.set_lightcurves(t, y, dy + 1e-12, y_offset=np.zeros(1))
    engine.set_model(kinds, np.concatenate([theta, [0.0]]), np.arange(P, dtype=np.int32), np.tile([-np.inf, np.inf], (P + 1, 1)))
    q0 = np.random.default_rng(P).standard_normal((3, N))
    th = np.tile(theta, (3, 1))
    drawn, status = engine.gp_draw(th, normals=q0)
    assert np.all(status == 0)
    back, _, _, status = engine.whiten(th, y=drawn, stats=False)
    assert np.all(status == 0) and engine.last_solver == "mtg_whiten_kernel<%d>" % rank, engine.last_solver
    coeffs = dense.build_coeffs(kinds, theta)
    fac = R.factor(t, R.diagonal(dy[0], coeffs), coeffs)
    for b in range(3):
        s = R.scale_at(t, coeffs, fac, q0[b], np.arange(N))
        tol = 2.0 * 64.0 * np.sqrt(N) * U * s / np.sqrt(fac[3])
        e = np.abs(back[b] - q0[b])
        print("\nwhiten(gp_draw(q0)) rank %d draw %d: worst e/tol %.3g" % (len(fac[0][0]), b, np.max(e / tol)))
        assert np.all(e <= tol)


@pytest.mark.parametrize("B", [4, 300])
def test_likelihood_identity(engine, B):
    kinds = synth.ALT_MODEL
    N = 10000
    t, y, dy = synth.make_lightcurves(N, 2, seed=91)
    theta = synth.draw_thetas(kinds, B, seed=92, percent=0.02)
    P = theta.shape[1]
    lc = (np.arange(B) % 2).astype(np.int32)
    engine.set_window_bytes(golden_util.FULL_WINDOW)
    engine.set_lightcurves(t, y, dy + 1e-12, y_offset=y.mean(axis=1))
    engine.set_model(kinds, np.concatenate([theta[0], [0.0]]), np.arange(P, dtype=np.int32), np.tile([-np.inf, np.inf], (P + 1, 1)))
    _, _, st, status = engine.whiten(theta, lc_index=lc, residuals=False, ks=False)
    lnl, lstatus = engine.loglike(theta, lc, add_prior=False)
    print("\nwhiten identity B=%d: loglike dispatched to %s" % (B, engine.last_solver))
    assert np.all(status == 0) and np.all(lstatus == 0)
    mine = -0.5 * (st[:, 1] + st[:, 2] + N * np.log(2.0 * np.pi))
    tol = 64.0 * np.sqrt(N) * U * 0.5 * (st[:, 1] + np.abs(st[:, 2]) + N * np.log(2.0 * np.pi))
    print("whiten identity B=%d: worst |lnL - identity| / tol %.3g" % (B, np.max(np.abs(mine - lnl) / tol)))
    assert np.all(np.abs(mine - lnl) <= tol)


def mp_ks(q):
    import mpmath as mp
    with mp.workdps(30):
        x = sorted(mp.mpf(float(v)) for v in q)
        N = len(x)
        cdf = [mp.ncdf(v) for v in x]
        dp = max(mp.mpf(i + 1) / N - c for i, c in enumerate(cdf))
        dm = max(c - mp.mpf(i) / N for i, c in enumerate(cdf))
        return float(dp), float(dm)


@pytest.mark.parametrize("N", [257, 1000])
def test_ks_statistic_and_pvalue(engine, N):
    from scipy.stats import ks_1samp, norm
    from mind_the_gaps_amd.gpmodelling import whiten_diagnostics
    # a white model with sigma^2 + jitter = D known: row 0 standard normals through it, row 1 a constant q, row 2 the
    # data as they are (far from normal)
    t, y, dy, theta, data = WR.ks_case(N)
    engine.set_window_bytes(golden_util.FULL_WINDOW)
    engine.set_lightcurves(t, y, dy + 1e-12, y_offset=np.zeros(1))
    engine.set_model([synth.K_JITTER], np.array([-0.3, 0.0]), np.array([0], dtype=np.int32), np.tile([-np.inf, np.inf], (2, 1)))
    q, _, st, status = engine.whiten(theta, y=data)
    assert np.all(status == 0)
    assert np.ptp(q[1]) <= 4.0 * U
    out = whiten_diagnostics(st, np.zeros((3, 1)), N)
    bound = (2.0 * ERFC_ULP + 8.0) * U
    for b in range(3):
        dp, dm = mp_ks(q[b])
        print("\nwhiten KS N=%d row %d: D+ off by %.2f u, D- by %.2f u (bound %.0f u)"
              % (N, b, abs(st[b][5] - dp) / U, abs(st[b][6] - dm) / U, bound / U))
        assert abs(st[b][5] - dp) <= bound and abs(st[b][6] - dm) <= bound
        ref = ks_1samp(q[b], norm.cdf)
        assert abs(out["ks_statistic"][b] - ref.statistic) <= bound + 4.0 * U
        assert abs(out["ks_pvalue"][b] - ref.pvalue) <= 1e-9 * ref.pvalue, (out["ks_pvalue"][b], ref.pvalue)


@pytest.mark.parametrize("N", [97, 1000])
def test_acf_against_numpy(engine, N):
    kinds = synth.NULL_MODEL
    th = synth.truth(kinds)
    P = len(th)
    t, y, dy = synth.make_lightcurves(N, 1, seed=55)
    engine.set_window_bytes(golden_util.FULL_WINDOW)
    engine.set_lightcurves(t, y, dy + 1e-12, y_offset=y.mean(axis=1))
    engine.set_model(kinds, np.concatenate([th, [0.0]]), np.arange(P, dtype=np.int32), np.tile([-np.inf, np.inf], (P + 1, 1)))
    theta = np.tile(th, (2, 1))
    theta[1] += 0.1
    for K in (1, N - 1, N // 4):
        q, acf, _, status = engine.whiten(theta, lags=K)
        assert np.all(status == 0) and acf.shape == (2, K)
        for b in range(2):
            e = np.abs(acf[b] - WR.acf(q[b], K))
            print("\nwhiten acf N=%d K=%d row %d: worst |delta| %.3g = %.3g of 4 N u" % (N, K, b, e.max(), e.max() / (4.0 * N * U)))
            assert np.all(e <= 4.0 * N * U)
    for K in (N, -1):
        with pytest.raises(_engine.EngineError) as err:
            engine.whiten(theta, lags=K)
        assert err.value.code == _engine.E_ARG
    # K = 0 with a place for the lags, and lags without a place for them
    dp = ctypes.POINTER(ctypes.c_double)
    room, status = np.zeros((2, 4)), np.zeros(2, dtype=np.int32)
    call = lambda K, acf: engine._lib.mtg_whiten(engine._ctx, 2, theta.ctypes.data_as(dp), None, None, None, K, acf, None,
                                                  status.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
    assert call(0, room.ctypes.data_as(dp)) == _engine.E_ARG
    assert call(3, None) == _engine.E_ARG
    assert call(0, None) == _engine.E_ARG            # every output NULL
    assert engine._lib.mtg_whiten(engine._ctx, 0, None, None, None, None, 0, None, room.ctypes.data_as(dp),
                                  status.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))) == 0


def tutorial_model(mean_model=None, N=300):
    from mind_the_gaps_amd.gpmodelling import GPModelling
    from mind_the_gaps_amd.lightcurves import GappyLightcurve
    from mind_the_gaps_amd.models import DampedRandomWalk, Lorentzian
    rng = np.random.default_rng(3)
    t = np.sort(rng.uniform(0.0, 400.0, N))
    y = 50.0 + rng.standard_normal(N)
    dy = rng.uniform(0.2, 0.5, N)
    kernel = DampedRandomWalk(1.0, -1.0, bounds=[(-5.0, 5.0), (-5.0, 5.0)]) + \
        Lorentzian(0.5, 1.0, -0.5, bounds=[(-5.0, 5.0), (-2.0, 4.0), (-4.0, 2.0)])
    lc = GappyLightcurve(t, y, dy)
    return GPModelling(lc, kernel, mean_model=mean_model), t, y, dy


def test_public_api():
    from scipy.stats import ks_1samp, norm
    model, t, y, dy = tutorial_model()
    N = len(t)
    p0 = model.gp.get_parameter_vector()
    q = model.whitened_residuals()
    assert q.shape == (N,) and np.array_equal(q, model.gp.whiten(y))
    # GP.sample's draw from these normals is the light curve again
    eng, dm = model.gp._bound_engine(y)
    back, status = eng.gp_draw(dm.full[dm.free_index][None, :], normals=q[None, :])
    assert status[0] == 0 and np.max(np.abs(back[0] + (dm.y_offset or 0.0) - y)) <= 1e-9
    rows = p0[None, :] + 0.05 * np.random.default_rng(1).uniform(-1.0, 1.0, (5, len(p0)))
    qs = model.whitened_residuals(rows)
    assert qs.shape == (5, N) and np.all(np.isfinite(qs))
    diag = model.residual_diagnostics(rows)
    K = N // 4
    assert diag["acf"].shape == (5, K) and diag["acf_band"] == 1.96 / np.sqrt(N)
    for b in range(5):                       # the notebook's three lines
        ks = ks_1samp(qs[b], norm.cdf)
        assert abs(diag["ks_statistic"][b] - ks.statistic) <= (2.0 * ERFC_ULP + 8.0) * U
        assert abs(diag["ks_pvalue"][b] - ks.pvalue) <= 1e-9 * ks.pvalue
        acorr = np.correlate(qs[b], qs[b], mode="full")
        acorr = acorr[N:N + K] / acorr[N - 1]                                  # plt.acorr(q, maxlags=K), positive lags
        assert np.all(np.abs(diag["acf"][b] - acorr) <= 4.0 * N * U)
        assert abs(diag["chi2"][b] - qs[b] @ qs[b]) <= 4.0 * N * U * (qs[b] @ qs[b])
    one = model.residual_diagnostics(lags=10)
    assert one["acf"].shape == (10,) and np.ndim(one["ks_pvalue"]) == 0
    # under a sine mean the device sees the residual with a zero mean
    from mind_the_gaps_amd.models import SineModel
    sine, t, y, dy = tutorial_model(mean_model=SineModel(50.0, 0.3, 0.02, 0.5, bounds=[(40.0, 60.0), (0.0, 5.0), (0.01, 0.04), (-4.0, 4.0)]))
    qsine = sine.whitened_residuals()
    assert qsine.shape == (N,) and np.all(np.isfinite(qsine))
    dsine = sine.residual_diagnostics(sine.gp.get_parameter_vector()[None, :], lags=7)
    assert dsine["acf"].shape == (1, 7) and abs(dsine["chi2"][0] - qsine @ qsine) <= 4.0 * N * U * (qsine @ qsine)


def test_ks_pvalues_are_uniform_under_the_model(engine):
    from scipy.stats import kstest
    from mind_the_gaps_amd.gpmodelling import whiten_diagnostics
    kinds = synth.NULL_MODEL
    th = synth.truth(kinds)
    P, N, B = len(th), 256, 512
    t, y, dy = synth.make_lightcurves(N, 1, seed=17)
    engine.set_window_bytes(golden_util.FULL_WINDOW)
    engine.set_lightcurves(t, y, dy + 1e-12, y_offset=np.zeros(1))
    engine.set_model(kinds, np.concatenate([th, [0.0]]), np.arange(P, dtype=np.int32), np.tile([-np.inf, np.inf], (P + 1, 1)))
    engine.set_stream_base(0)
    theta = np.tile(th, (B, 1))
    draws, status = engine.gp_draw(theta, seed=20261020)
    assert np.all(status == 0)
    _, acf, st, status = engine.whiten(theta, y=draws, residuals=False, lags=1)
    assert np.all(status == 0)
    p = whiten_diagnostics(st, acf, N)["ks_pvalue"]
    verdict = kstest(p, "uniform")
    print("\nwhiten calibration: KS of %d p-values against the uniform: D = %.4f, p = %.3g; mean chi2 / N = %.4f"
          % (B, verdict.statistic, verdict.pvalue, float(np.mean(st[:, 1])) / N))
    assert verdict.pvalue >= 1e-4
