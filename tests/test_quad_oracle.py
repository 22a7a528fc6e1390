"""The quad-precision oracle (oracle/celerite_quad.c, oracle/quad.py) against independent truths: the mpmath goldens
(dense Cholesky at 50 / 80 digits), the OU Kalman recursion in mpmath at N = 1e4, the reference's own coefficient
builders, and its own time-reversed sweep; and the stored rows of tests/golden/quad_golden.json recomputed.  CPU only.

The mpmath goldens were computed from float64 coefficients (oracle.dense.build_coeffs), so they are checked through
the raw-coefficient entry fed the same coefficients.  The bound is the rounding of the stored value, 2^-52 |truth|,
plus the quad sweep's own resolution where the covariance is extreme (celerite_quad.c, "Resolution"):
N 2^-113 A / min(yerr^2), A the summed amplitudes -- below 2^-53 |truth| on all but the top corners of the box."""
import json
import os

import numpy as np
import pytest

import golden_util
from mind_the_gaps_amd import synthetic as synth
from oracle import celerite as oracle_c
from oracle import dense
from oracle import quad

HERE = os.path.dirname(os.path.abspath(__file__))
ULP = 2.0 ** -52


def raw(t, y, dy, co, mean, reverse=False):
    ar, cr, ac, bc, cc, dc, jit = co
    hi, lo, S, st = quad.loglike_coeffs(t, y, dy, *(np.asarray(a)[None] for a in (ar, cr, ac, bc, cc, dc)),
                                        jitter=jit, mean_params=[mean], reverse=reverse)
    assert st[0] == 0
    return hi[0], lo[0], S[0]


def resolution(N, co, dy):
    amp = co[6] + np.sum(np.abs(co[0])) + np.sum(np.abs(co[2])) + np.sum(np.abs(co[3]))
    return N * 2.0 ** -113 * amp / np.min((np.asarray(dy) + 1e-12) ** 2)


def test_box_golden_every_row():
    """All 200 rows of box_golden.json (mp80, N = 50, theta over the whole prior box).  One row is beyond what a
    quad sweep resolves: null model, S0 = e^46.7, Q = e^9.16 (A / yerr^2 ~ 3e20): its value moves by ~10 ulp with
    the phase origin (t + 0.375, t + 1: +0.3, -9.8 ulp), i.e. the quad rounding of U_n V_m at amplitude 8.5e19."""
    g = json.load(open(os.path.join(HERE, "golden", "box_golden.json")))
    t, y, dy = synth.make_lightcurves(g["N"], 1, seed=g["seed"])
    beyond = []
    for c in g["cases"]:
        co = dense.build_coeffs(c["kinds"], c["theta"])
        hi, lo, _ = raw(t, y[0], dy[0], co, g["mean"])
        T = c["lnL_mp80"]
        e = abs((hi - T) + lo)
        assert e <= ULP * abs(T) + resolution(g["N"], co, dy[0]), (c["model"], c["theta"], e)
        if e > ULP * abs(T):
            beyond.append((c["model"], c["theta"], e / abs(T)))
    assert len(g["cases"]) == 200 and len(beyond) <= 1, beyond


def test_loglike_golden_mpmath_cases():
    n = 0
    for c in golden_util.cases():
        if np.isnan(c["lnL_mpmath50"]):
            continue
        kinds, theta = json.loads(c["kinds"]) if isinstance(c["kinds"], str) else c["kinds"], c["theta"]
        theta = json.loads(theta) if isinstance(theta, str) else theta
        mp = json.loads(c["mean_params"]) if isinstance(c["mean_params"], str) else c["mean_params"]
        co = dense.build_coeffs(kinds, theta)
        ar, cr, ac, bc, cc, dc, jit = co
        hi, lo, S, st = quad.loglike_coeffs(c["t"], c["y"], c["dy"], *(np.asarray(a)[None] for a in co[:6]),
                                            jitter=jit, mean_kind=c["mean_kind"], mean_params=[mp])
        T = c["lnL_mpmath50"]
        assert st[0] == 0 and abs((hi[0] - T) + lo[0]) <= ULP * abs(T) + resolution(len(c["t"]), co, c["dy"]), (
            c["id"], c["name"], hi[0] - T + lo[0])
        n += 1
    assert n == 21                        # every case that carries an mpmath value


def test_quad_builders_against_the_reference_builders():
    """The theta entry's quad builders rounded to double, against the reference's own methods (coeff_golden.npz):
    to a few ulp (exp of theta in quad against numpy's exp and the reference's float64 products)."""
    gold = np.load(os.path.join(HERE, "golden", "coeff_golden.npz"))
    kind = {"Lorentzian": synth.K_LORENTZIAN, "Cosinus": synth.K_COSINUS, "DampedRandomWalk": synth.K_DRW,
            "BendingPowerlaw": synth.K_BPL}
    for name in gold["classes"]:
        name = str(name)
        for b, p in enumerate(gold[name + "/params"]):
            got = quad.build_coeffs([kind[name]], p)
            for k, key in enumerate(("a_real", "c_real", "a_comp", "b_comp", "c_comp", "d_comp")):
                want = gold[name + "/" + key][b]
                assert np.allclose(got[k], want, rtol=8 * ULP, atol=0), (name, key, b, got[k], want)


def test_theta_entry_agrees_with_raw_entry_on_well_conditioned_rows():
    """Every term kind, both SHO regimes and the Matern32 eps: lnL(theta) against the raw entry fed dense.build_coeffs
    (which differ by the builders' float64 rounding only, ~1e-16 relative on a well conditioned row)."""
    t, y, dy = synth.make_lightcurves(300, 1, seed=9)
    models = [synth.NULL_MODEL, synth.ALT_MODEL, [synth.K_BPL, synth.K_MATERN32], [synth.K_COMPLEX4, synth.K_REAL],
              [synth.K_COSINUS, synth.K_JITTER, synth.K_SHO], [synth.K_COMPLEX3, synth.K_DRW]]
    for kinds in models:
        thetas = synth.draw_thetas(kinds, 6, seed=4)
        if synth.K_SHO in kinds:                         # over-damped (two real terms) in half the rows
            log_q = sum(synth.NPARAMS[k] for k in kinds[:kinds.index(synth.K_SHO)]) + 1
            thetas[:3, log_q] = np.log(0.3)
        for th in thetas:
            full = np.concatenate([th, [y.mean()]])
            hi, lo, S, st = quad.loglike(t, y, dy, kinds, full[None])
            rh, rl, rS = raw(t, y[0], dy[0], dense.build_coeffs(kinds, th), y.mean())
            assert st[0] == 0 and abs((hi[0] - rh) + (lo[0] - rl)) <= 1e-13 * S[0], (kinds, th)
            assert S[0] == pytest.approx(rS, rel=1e-12)


def _ou_mp(t, y, dy, a, c, mu, dps=40):
    """make_golden.ou_closed_form's scalar Kalman recursion in mpmath."""
    import mpmath as mp
    with mp.workdps(dps):
        a, c, mu = mp.mpf(a), mp.mpf(c), mp.mpf(mu)
        m, P, ll = mp.mpf(0), a, mp.mpf(0)
        two_pi = 2 * mp.pi
        for n in range(len(t)):
            if n > 0:
                phi = mp.exp(-c * (mp.mpf(t[n]) - mp.mpf(t[n - 1])))
                m, P = phi * m, phi * phi * P + a * (1 - phi * phi)
            S = P + mp.mpf(float(np.float64(dy[n]) + 1e-12)) ** 2
            v = mp.mpf(y[n]) - mu - m
            ll += -(mp.log(two_pi * S) + v * v / S) / 2
            K = P / S
            m, P = m + K * v, (1 - K) * P
        return ll


@pytest.mark.parametrize("log_a,log_c", [(np.log(100.0), np.log(2 * np.pi / 20.0)), (np.log(30.0), np.log(3.0)),
                                         (np.log(500.0), np.log(1e-7))], ids=["tutorial", "short", "long-memory"])
def test_drw_against_ou_kalman_in_mpmath(log_a, log_c):
    t, y, dy = synth.make_lightcurves(10000, 1, seed=77)
    co = dense.build_coeffs([synth.K_DRW], [log_a, log_c])
    hi, lo, _ = raw(t, y[0], dy[0], co, float(y.mean()))
    import mpmath as mp
    with mp.workdps(40):
        T = _ou_mp(t, y[0], dy[0], co[0][0], co[1][0], float(y.mean()))
        err = abs(mp.mpf(hi) + mp.mpf(lo) - T)
        assert float(err) <= ULP * abs(float(T)), float(err)


@pytest.mark.parametrize("kinds,offset", [([synth.K_SHO] * 5, 0.0), (synth.ALT_MODEL, 0.0), (synth.NULL_MODEL, 1.0e9)],
                         ids=["5sho", "alt", "null-linear-mean-at-1e9"])
def test_n120_against_dense_mpmath(kinds, offset):
    """theta in, against the 50-digit dense Cholesky fed dense.build_coeffs -- and the theta entry's fitted linear mean
    (mean_kind 1) at t ~ 1e9 s, where slope * t ~ 2e3 (the quad value at theta against the raw entry, the same
    coefficients, and the dense truth)"""
    t, y, dy = synth.make_lightcurves(120, 1, seed=31, offset=offset)
    if offset:
        th = synth.truth(kinds)
        line = [2e-6, float(y.mean()) - 2e-6 * t[60]]
        co = dense.build_coeffs(kinds, th)
        hi, lo, _, st = quad.loglike_coeffs(t, y[0], dy[0], *(np.asarray(a)[None] for a in co[:6]), jitter=co[6],
                                            mean_kind=1, mean_params=[line])
        T = dense.dense_loglike_mp(t, y[0], dy[0], co, 1, line, dps=50)
        assert st[0] == 0 and abs((hi[0] - T) + lo[0]) <= ULP * abs(T), hi[0] - T + lo[0]
        qh, ql, qS, qs = quad.loglike(t, y, dy, kinds, np.concatenate([th, line])[None], mean_kind=1)
        assert qs[0] == 0 and abs((qh[0] - hi[0]) + (ql[0] - lo[0])) <= 1e-13 * qS[0]
        return
    th = synth.truth(kinds).copy()
    if len(kinds) == 5:
        th = np.array([v for i in range(5) for v in (np.log(20.0 + 10 * i), np.log([3.0, 8.0, 10.0, 1.0, 0.3][i]),
                                                     np.log(2 * np.pi / (5.0 + 6 * i)))])
    co = dense.build_coeffs(kinds, th)
    hi, lo, _ = raw(t, y[0], dy[0], co, float(y.mean()))
    T = dense.dense_loglike_mp(t, y[0], dy[0], co, 0, [float(y.mean())], dps=50)
    assert abs((hi - T) + lo) <= ULP * abs(T), hi - T + lo


def test_forward_and_reverse_sweeps_agree_where_celerite_is_accurate():
    """Rows of box_golden.json where celerite's float64 error is below 1e-12: the two directions to 1e-25 S."""
    g = json.load(open(os.path.join(HERE, "golden", "box_golden.json")))
    t, y, dy = synth.make_lightcurves(g["N"], 1, seed=g["seed"])
    n = 0
    for c in g["cases"]:
        c64, st = oracle_c.logprob_batch(t, y, dy, c["kinds"], np.concatenate([c["theta"], [g["mean"]]]))
        if st[0] != 0 or abs(c64[0] - c["lnL_mp80"]) >= 1e-12 * abs(c["lnL_mp80"]):
            continue
        co = dense.build_coeffs(c["kinds"], c["theta"])
        f, r = raw(t, y[0], dy[0], co, g["mean"]), raw(t, y[0], dy[0], co, g["mean"], reverse=True)
        assert abs((f[0] - r[0]) + (f[1] - r[1])) <= 1e-25 * f[2], (c["model"], c["theta"])
        n += 1
    assert n >= 100


def test_fixture_rows_recomputed():
    """A handful of quad_golden.json rows (N <= 2e4, every regime) recomputed: the light curve's hash, the truth to
    the last bit of its double pair, S, and celerite's stored value."""
    doc = json.load(open(os.path.join(HERE, "golden", "quad_golden.json")))
    regimes = set()
    for g in doc["groups"]:
        if g["lightcurve"]["N"] > 20011:
            continue
        t, y, dy = golden_util.quad_lightcurve(g["lightcurve"])
        assert golden_util.lightcurve_sha256(t, y, dy) == g["sha256"], g["name"]
        rows = g["rows"][::3]
        full = np.array([r["theta"] for r in rows])
        lc = np.array([r["lc"] for r in rows], dtype=np.int32)
        mk = g["mean_kind"]
        nm = 2 if mk == 1 else 1
        hi, lo, S, st = quad.loglike(t, y, dy, g["kinds"], full, lc_index=lc, mean_kind=mk)
        c64, cst = oracle_c.logprob_batch(t, y, dy, g["kinds"], full, lc_index=lc, mean_kind=mk, nthreads=4)
        for b, r in enumerate(rows):
            assert st[b] == 0 and abs((hi[b] - r["lnL"]) + (lo[b] - r["lnL_lo"])) <= 1e-30 * r["S"], (g["name"], b)
            assert S[b] == pytest.approx(r["S"], rel=1e-15)
            assert cst[b] == r["c64_status"] and c64[b] == pytest.approx(r["c64"], rel=1e-13, abs=0)
            co = dense.build_coeffs(g["kinds"], r["theta"][:-nm])
            assert [list(a) for a in co[:6]] + [co[6]] == r["coeffs"], (g["name"], b)
            rh, rl, _, rs = quad.loglike_coeffs(t, y[r["lc"]], dy[r["lc"]], *(np.asarray(a)[None] for a in co[:6]),
                                                jitter=co[6], mean_kind=mk, mean_params=[r["theta"][-nm:]])
            assert rs[0] == 0 and abs((rh[0] - r["lnL_raw"]) + (rl[0] - r["lnL_raw_lo"])) <= 1e-30 * r["S"]
        regimes.add(g["regime"])
    assert regimes == {"typical", "signatures", "long_memory", "short_memory", "phase", "extreme", "time_offset",
                       "linear_mean"}


def test_fixture_covers_the_switches_of_the_device_code():
    doc = json.load(open(os.path.join(HERE, "golden", "quad_golden.json")))
    sizes = {g["lightcurve"]["N"] for g in doc["groups"]}
    assert {64, 65, 1000, 4095, 4096, 10000, 20011, 200000} <= sizes
    phases = sorted(r["d_dxmax"] for g in doc["groups"] if g["regime"] == "phase" for r in g["rows"])
    for lo, hi in ((0.8e5, 1e5), (1e5, 1.2e5), (0.8e12, 1e12), (1e12, 1.2e12)):
        assert any(lo <= p <= hi for p in phases), (lo, hi)
    for g in doc["groups"]:
        assert g["rows"], g["name"]
        for r in g["rows"]:
            assert r["c64_status"] == 0
            tol = max(10 * abs((r["c64"] - r["lnL"]) - r["lnL_lo"]),
                      64 * np.sqrt(g["lightcurve"]["N"]) * doc["u"] * r["S"])
            assert r["fwd_rev"] < 1e-3 * tol, g["name"]


# ---------------------------------------------------------------------------------------------------------------------
# The prediction and solve entries (oracle/predict_sweep.h through oracle/predict.py): the truth of
# tests/golden/predict_golden.npz and tests/test_predict_vs_quad_gpu.py
# ---------------------------------------------------------------------------------------------------------------------

def _mp_coeffs(mp, kinds, p):
    """celerite's coefficients built from theta in mpmath (SHO, DRW, real, complex3, jitter)"""
    ar, cr, ac, bc, cc, dc, jit = [], [], [], [], [], [], mp.mpf(0)
    i = 0
    for k in kinds:
        q = [mp.mpf(float(v)) for v in p[i:i + dense.n_kernel_params([k])]]
        i += len(q)
        if k in (synth.K_REAL, synth.K_DRW):
            ar.append(mp.exp(q[0])); cr.append(mp.exp(q[1]))
        elif k == synth.K_COMPLEX3:
            ac.append(mp.exp(q[0])); bc.append(mp.mpf(0)); cc.append(mp.exp(q[1])); dc.append(mp.exp(q[2]))
        elif k == synth.K_JITTER:
            jit += mp.exp(2 * q[0])
        elif k == synth.K_SHO:
            S0, Q, w0 = mp.exp(q[0]), mp.exp(q[1]), mp.exp(q[2])
            if Q < 0.5:
                f = mp.sqrt(1 - 4 * Q * Q)
                ar += [S0 * w0 * Q * (1 + 1 / f) / 2, S0 * w0 * Q * (1 - 1 / f) / 2]
                cr += [w0 / Q * (1 - f) / 2, w0 / Q * (1 + f) / 2]
            else:
                f = mp.sqrt(4 * Q * Q - 1)
                ac.append(S0 * w0 * Q); bc.append(S0 * w0 * Q / f); cc.append(w0 / Q / 2); dc.append(w0 / Q / 2 * f)
        else:
            raise ValueError(k)
    return ar, cr, ac, bc, cc, dc, jit


def _mp_predict(t, y, dy, kinds, full, mean_kind, b, ts, dps=40):
    """dense algebra in mpmath: mu and var at the training times as celerite forms them (mean + K_s K^-1 r,
    k(0) - diag(K_s K^-1 K_s)), K^-1 b, and the prediction at ts -- every value with its error below 1e-30"""
    import mpmath as mp
    with mp.workdps(dps):
        nk = dense.n_kernel_params(kinds)
        ar, cr, ac, bc, cc, dc, jit = _mp_coeffs(mp, kinds, full[:nk])

        def k(tau):
            tau = abs(tau)
            v = sum((a * mp.exp(-c * tau) for a, c in zip(ar, cr)), mp.mpf(0))
            for a, bb, c, d in zip(ac, bc, cc, dc):
                v += mp.exp(-c * tau) * (a * mp.cos(d * tau) + bb * mp.sin(d * tau))
            return v

        def mean(x):
            x = mp.mpf(float(x))
            return mp.mpf(float(full[nk])) * x + mp.mpf(float(full[nk + 1])) if mean_kind == 1 else mp.mpf(float(full[nk]))

        tt = [mp.mpf(float(v)) for v in t]
        N = len(tt)
        Ks = mp.matrix(N, N)
        for i in range(N):
            for j in range(i + 1):
                Ks[i, j] = Ks[j, i] = k(tt[i] - tt[j])
        K = Ks.copy()
        for i in range(N):
            K[i, i] += mp.mpf(float(np.float64(dy[i]) + np.float64(1e-12))) ** 2 + jit
        Lc = mp.cholesky(K)

        def solve(v):
            return mp.cholesky_solve(K, v) if Lc is None else _chol_solve(mp, Lc, v)

        r = mp.matrix([mp.mpf(float(y[i])) - mean(t[i]) for i in range(N)])
        alpha = solve(r)
        KsKinv = [solve(mp.matrix([Ks[i, j] for i in range(N)])) for j in range(N)]
        mu = [mean(t[n]) + sum(Ks[n, j] * alpha[j] for j in range(N)) for n in range(N)]
        var = [k(0) - sum(Ks[n, j] * KsKinv[n][j] for j in range(N)) for n in range(N)]
        x = [solve(mp.matrix([mp.mpf(float(v)) for v in b[:, c]])) for c in range(b.shape[1])]
        mu_at, var_at = [], []
        for s in ts:
            ks = mp.matrix([k(mp.mpf(float(s)) - tt[j]) for j in range(N)])
            v = solve(ks)
            mu_at.append(mean(s) + sum(ks[j] * alpha[j] for j in range(N)))
            var_at.append(k(0) - sum(ks[j] * v[j] for j in range(N)))
        # constant means travel as y_offset: Engine.predict's mu leaves them out (oracle.predict's convention)
        mu_dev = [m - (mean(0) if mean_kind == 0 else 0) for m in mu]
        return mu_dev, var, [[xc[i] for i in range(N)] for xc in x], mu_at, var_at


def _chol_solve(mp, Lc, v):
    N = Lc.rows
    z = mp.matrix(N, 1)
    for i in range(N):
        z[i] = (v[i] - sum(Lc[i, j] * z[j] for j in range(i))) / Lc[i, i]
    x = mp.matrix(N, 1)
    for i in reversed(range(N)):
        x[i] = (z[i] - sum(Lc[j, i] * x[j] for j in range(i + 1, N))) / Lc[i, i]
    return x


def _close(mp_vals, hi, lo, scale, rel=1e-25):
    """|quad - mp| <= rel * scale elementwise, the quad value as its double pair (a zero scale -- the jitter-only
    model's variance at new times -- asks for an exact zero)"""
    import mpmath as mp
    with mp.workdps(40):
        err = [abs((mp.mpf(float(h)) + mp.mpf(float(l))) - v) for v, h, l in zip(mp_vals, np.ravel(hi), np.ravel(lo))]
    err, scale = np.array([float(e) for e in err]), np.ravel(scale)
    assert np.all(err <= rel * scale), (float(np.max(err / np.where(scale > 0, scale, 1.0))), rel)


PRED_MP_CASES = [
    ("sho_underdamped+drw_constant", [synth.K_DRW, synth.K_SHO], [np.log(40.0), np.log(0.2), np.log(20.0), np.log(3.0),
                                                                  np.log(0.8)], 0, 0.0),
    ("sho_overdamped_linear", [synth.K_SHO, synth.K_JITTER], [np.log(30.0), np.log(0.2), np.log(0.9), np.log(0.6)], 1,
     0.0),
    ("complex3+drw_linear_at_1e9", [synth.K_COMPLEX3, synth.K_DRW], [np.log(2.0), np.log(0.3), np.log(40.0),
                                                                    np.log(1.5), np.log(0.2)], 1, 1.0e9),
    ("jitter_only", [synth.K_JITTER], [np.log(0.7)], 0, 0.0),
]


@pytest.mark.parametrize("label,kinds,kernel,mean_kind,offset", PRED_MP_CASES, ids=[c[0] for c in PRED_MP_CASES])
def test_predict_entries_against_dense_mpmath(label, kinds, kernel, mean_kind, offset):
    """predict_batch (both directions), apply_inverse and predict_at against 40-digit dense algebra at N = 60: to 1e-25
    of each value's scale (s_mu, s_var, ||K^-1 b||, the new-time scales).  Constant and linear means, over- and
    under-damped SHO, a phase at t ~ 1e9 s and a jitter-only model (J = 0).  At t ~ 1e9 s the quad phase d t itself is
    rounded at 2^-113 d max|t| (4e-24 rad at d = 40): the bound adds ten times that."""
    pytest.importorskip("mpmath")
    from oracle import predict as P
    N = 60
    t, y, dy = synth.make_lightcurves(N, 1, seed=41, offset=offset)
    y, dy = y[0], dy[0]
    mean = [2e-3, float(y.mean()) - 2e-3 * t[N // 2]] if mean_kind == 1 else [float(y.mean())]
    full = np.concatenate([kernel, mean])
    b = np.column_stack([np.random.default_rng(5).standard_normal(N), y - y.mean()])
    ts = np.array([t[0] - 3.0, t[7], 0.5 * (t[20] + t[21]), t[-1] + 0.25, t[-1] + 40.0])
    mu, var, x, mu_at, var_at = _mp_predict(t, y, dy, kinds, full, mean_kind, b, ts)
    dmax = np.max(dense.build_coeffs(kinds, kernel)[5], initial=0.0)
    rel = 1e-25 + 10.0 * 2.0 ** -113 * dmax * np.max(np.abs(np.concatenate([t, ts])))
    for rev in (False, True):
        q = P.predict(t, y, dy, kinds, full, mean_kind=mean_kind, reverse=rev)
        assert q.status[0] == 0
        _close(mu, q.mu, q.mu_lo, q.s_mu, rel)
        _close(var, q.var, q.var_lo, q.s_var, rel)
        a = P.apply_inverse(t, dy, kinds, full, b, reverse=rev)
        assert a.status == 0
        for c in range(b.shape[1]):
            _close(x[c], a.x[:, c], a.x_lo[:, c], np.full(N, np.max(np.abs(a.x[:, c]))), rel)
        pa = P.predict_at(t, y, dy, kinds, full, ts, mean_kind=mean_kind, reverse=rev)
        assert pa.status == 0
        _close(mu_at, pa.mu, pa.mu_lo, pa.s_mu, rel)
        _close(var_at, pa.var, pa.var_lo, pa.s_var, rel)


def _pred_group(name, rows=1):
    doc = json.load(open(os.path.join(HERE, "golden", "quad_golden.json")))
    g = [g for g in doc["groups"] if g["name"] == name][0]
    t, y, dy = golden_util.quad_lightcurve(g["lightcurve"])
    assert golden_util.lightcurve_sha256(t, y, dy) == g["sha256"]
    return g, t, y, dy, np.array([r["theta"] for r in g["rows"][-rows:]]), \
        np.array([r["lc"] for r in g["rows"][-rows:]], dtype=np.int32)


@pytest.mark.parametrize("name", ["rank10/config5", "phase/j3", "offset/seconds", "linear_mean/j3_seconds"])
def test_predict_forward_and_reverse_sweeps_agree(name):
    """The forward and time-reversed quad sweeps (independent roundings, the phases included) agree far below float64
    resolution: to 2^-53 * 1e-6 of each value's scale -- at N = 2e5 for rank10/config5, and at 9e11 rad per step and
    t ~ 1e9 s -- plus the rounding of the quad phases themselves, a walk of N steps of 2^-113 d max|t|:
    10 sqrt(N) 2^-113 d max|t| (1e-18 at phase/j3's 1.1e12 rad per step, whose phases reach 1e15 rad).  The same for apply_inverse on two columns."""
    from oracle import predict as P
    g, t, y, dy, full, lc = _pred_group(name)
    mk = g["mean_kind"]
    nk = dense.n_kernel_params(g["kinds"])
    dmax = np.max(dense.build_coeffs(g["kinds"], full[0][:nk])[5], initial=0.0)
    rel = 1e-6 * 2.0 ** -53 + 10.0 * np.sqrt(len(t)) * 2.0 ** -113 * dmax * np.max(np.abs(t))
    f = P.predict(t, y, dy, g["kinds"], full, lc_index=lc, mean_kind=mk)
    r = P.predict(t, y, dy, g["kinds"], full, lc_index=lc, mean_kind=mk, reverse=True)
    assert np.all(f.status == 0) and np.all(r.status == 0)
    for v, s in (("mu", "s_mu"), ("var", "s_var")):
        d = np.abs((getattr(f, v) - getattr(r, v)) + (getattr(f, v + "_lo") - getattr(r, v + "_lo")))
        assert np.max(d / getattr(f, s)) <= rel, (v, float(np.max(d / getattr(f, s))), rel)
    if len(t) <= 20011:
        b = np.column_stack([y[lc[0]] - y[lc[0]].mean(), np.random.default_rng(9).standard_normal(len(t))])
        a = P.apply_inverse(t, dy[lc[0]], g["kinds"], full[0], b)
        ar = P.apply_inverse(t, dy[lc[0]], g["kinds"], full[0], b, reverse=True)
        d = np.abs((a.x - ar.x) + (a.x_lo - ar.x_lo))
        assert np.all(np.max(d, axis=0) <= rel * np.max(np.abs(a.x), axis=0))


@pytest.mark.parametrize("name", ["phase/j3", "offset/seconds", "long_memory", "typical/5sho"])
def test_apply_inverse_quad_residual(name):
    """K x - b of the quad solution, with the O(N J) semiseparable product (celerite's dot) in quad: below 2^-100 of
    ||b|| + max(K_nn) ||x||, i.e. the quad solve is exact far beyond float64."""
    from oracle import predict as P
    g, t, y, dy, full, lc = _pred_group(name)
    b = np.column_stack([y[lc[0]] - y[lc[0]].mean(), np.random.default_rng(11).standard_normal(len(t))])
    a = P.apply_inverse(t, dy[lc[0]], g["kinds"], full[0], b, residual=True)
    assert a.status == 0
    co = dense.build_coeffs(g["kinds"], full[0][:dense.n_kernel_params(g["kinds"])])
    kmax = np.max((dy[lc[0]] + 1e-12) ** 2) + dense.kernel_value(co, 0.0) + co[6]
    scale = np.max(np.abs(b), axis=0) + kmax * np.max(np.abs(a.x), axis=0)
    assert np.all(np.max(np.abs(a.residual), axis=0) <= 2.0 ** -100 * scale), np.max(np.abs(a.residual), axis=0) / scale


def test_c64_baseline_against_numpy_dense():
    """The float64 baseline (oracle/celerite_ref.c, celerite's phase at the absolute time) against numpy's dense float64
    algebra at N = 2000, both measured from the quad truth in units of each value's scale: each within 100 times the
    other's error (or of 64 sqrt(N) u, whichever is larger) -- float64 rounding amplified by the problem's conditioning,
    the same for both (LAPACK's dense solve lands 12 times above the recurrence on mu here) -- and neither anywhere near
    the quad truth's own resolution."""
    from oracle import predict as P
    N = 2000
    t, y, dy = synth.make_lightcurves(N, 1, seed=43)
    y, dy = y[0], dy[0]
    kinds = synth.ALT_MODEL
    th = synth.truth(kinds)
    full = np.concatenate([th, [float(y.mean())]])
    c = P.predict(t, y, dy, kinds, full, c64=True)
    q = P.predict(t, y, dy, kinds, full)
    co = dense.build_coeffs(kinds, th)
    mu_d, var_d = dense.dense_predict(t, y, dy, co, 0, [float(y.mean())])
    floor = 64.0 * np.sqrt(N) * 2.0 ** -53

    def agree(e_c64, e_dense):
        assert e_c64 <= 100.0 * max(e_dense, floor) and e_dense <= 100.0 * max(e_c64, floor), (e_c64, e_dense)
        assert max(e_c64, e_dense) > 1e-20

    for v, s, d in (("mu", "s_mu", mu_d - y.mean()), ("var", "s_var", var_d)):
        T, S = getattr(q, v)[0] + getattr(q, v + "_lo")[0], getattr(q, s)[0]
        agree(np.max(np.abs(getattr(c, v)[0] - T) / S), np.max(np.abs(d - T) / S))
    b = np.random.default_rng(13).standard_normal((N, 2))
    K = dense.kernel_value(co, t[:, None] - t[None, :])
    K[np.diag_indices(N)] += (dy + 1e-12) ** 2 + co[6]
    x_d = np.linalg.solve(K, b)
    a64 = P.apply_inverse(t, dy, kinds, full, b, c64=True)
    aq = P.apply_inverse(t, dy, kinds, full, b)
    for j in range(2):
        xinf = np.max(np.abs(aq.x[:, j]))
        agree(np.max(np.abs(a64.x[:, j] - aq.x[:, j])) / xinf, np.max(np.abs(x_d[:, j] - aq.x[:, j])) / xinf)


def test_predict_fixture_recomputed():
    """predict_golden.npz: every group's light curve hash, and the stored truth of a small group recomputed to the bit;
    the noise-dominated group spans yerr^2 / k(0) in [1e4, 1e6]; the file stays under 1 MB."""
    from oracle import predict as P
    path = os.path.join(HERE, "golden", "predict_golden.npz")
    assert os.path.getsize(path) < 1 << 20
    fx = np.load(path)
    man = json.loads(bytes(fx["manifest"]))
    names = {g["name"] for g in man["groups"]}
    doc = json.load(open(os.path.join(HERE, "golden", "quad_golden.json")))
    assert {g["name"] for g in doc["groups"]} < names and "noise_dominated" in names
    for g in man["groups"]:
        t, y, dy = golden_util.quad_lightcurve(g["lightcurve"])
        assert golden_util.lightcurve_sha256(t, y, dy) == g["sha256"], g["name"]
        if g["name"] == "noise_dominated":
            ratio = np.array(g["yerr2_median"]) / np.array(g["k0"])
            assert np.all((ratio >= 0.99e4) & (ratio <= 1.01e6)), ratio
        if g["name"] in ("typical/alt_n65", "offset/seconds"):
            key = g["name"].replace("/", ".")
            q = P.predict(t, y, dy, g["kinds"], fx[key + "/theta"], lc_index=fx[key + "/lc"], mean_kind=g["mean_kind"])
            idx = fx[key + "/idx"]
            assert np.array_equal(q.mu[:, idx], fx[key + "/mu"]) and np.array_equal(q.var[:, idx], fx[key + "/var"])
