"""The host side of mtg_whiten without a GPU: the replay tests/whiten_replay.py against the dense Cholesky and against the
fixture tests/golden/whiten_golden.npz (the rule of tests/test_whiten_gpu.py, item 1), as the inverse of
tests/gp_draw_replay.py's draw; the header and the export list; the slab planner; and the host arithmetic of
GPModelling.residual_diagnostics against scipy with a fake engine that answers from the replay."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import golden_util
import gp_draw_replay as R
import whiten_replay as WR
from mind_the_gaps_amd import engine as _engine
from mind_the_gaps_amd import synthetic as synth
from oracle import dense

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
U = 2.0 ** -53
FIX = np.load(os.path.join(HERE, "golden", "whiten_golden.npz"))
GROUPS = {g["name"]: g for g in json.loads(bytes(FIX["manifest"]))["groups"]}


def arrays(name):
    key = name.replace("/", ".") + "/"
    return {k[len(key):]: FIX[k] for k in FIX.files if k.startswith(key)}


@pytest.mark.parametrize("kinds", [[synth.K_JITTER], [synth.K_DRW], synth.NULL_MODEL, synth.ALT_MODEL], ids=["J0", "J1", "J3", "J6"])
def test_replay_against_the_dense_cholesky(kinds):
    N = 200
    t, y, dy = synth.make_lightcurves(N, 1, seed=5)
    coeffs = dense.build_coeffs(kinds, synth.truth(kinds))
    data = y[0] - y[0].mean()
    fac = WR.factor(t, R.diagonal(dy[0], coeffs), coeffs)
    q = WR.whiten(t, dy[0], coeffs, data, factors=fac)
    qd, logdet = WR.dense_whiten(t, dy[0], coeffs, data)
    # both solve the same triangular system in float64: a few hundred u of the larger entries
    assert np.max(np.abs(q - qd)) <= 1e-11 * np.max(np.abs(qd))
    assert abs(np.sum(np.log(fac[3])) - logdet) <= 1e-11 * np.sum(np.abs(np.log(fac[3])))
    # the likelihood identity against the dense oracle
    lnl = dense.dense_loglike(t, data, dy[0], coeffs)
    st = WR.row_stats(q, fac[3])
    assert abs(-0.5 * (st[1] + st[2] + N * np.log(2.0 * np.pi)) - lnl) <= 1e-10 * abs(lnl)


@pytest.mark.parametrize("name", list(GROUPS))
def test_replay_against_the_fixture(name):
    g, a = GROUPS[name], arrays(name)
    t, y, dy = golden_util.quad_lightcurve(g["recipes"][0])
    assert golden_util.lightcurve_sha256(t, y, dy) == g["sha256"][0]
    N, theta, idx = len(t), a["theta"][0], a["idx"]
    assert len(idx) <= 64 and idx[0] == 0 and idx[-1] == N - 1
    nk = dense.n_kernel_params(g["kinds"])
    coeffs = dense.build_coeffs(g["kinds"], theta[:nk])
    mean = theta[nk] * t + theta[nk + 1] if g["mean_kind"] == 1 else 0.0
    fac = WR.factor(t, R.diagonal(dy[0], coeffs), coeffs)
    q = WR.whiten(t, dy[0], coeffs, y[0] - g["y_offset"][0], mean=mean, factors=fac)
    d = np.max(coeffs[5], initial=0.0)
    factor = 1.0 if d * float(np.max(np.diff(t))) >= 1.0e4 else 10.0
    s, e64 = a["scale"][0].astype(np.float64), a["c64err"][0].astype(np.float64)
    floor = 64.0 * np.sqrt(N) * U
    tol = np.maximum(factor * float(np.max(e64 / s)), floor) * s
    assert np.all(np.abs(q[idx] - a["T"][0]) <= tol)
    st = WR.row_stats(q, fac[3])
    sums, s64 = a["sums"][0], a["sums_c64err"][0]
    assert abs(st[1] - sums[1]) <= max(factor * s64[0] / sums[1], floor) * sums[1]
    assert abs(st[2] - sums[2]) <= max(factor * s64[1] / sums[5], floor) * sums[5]


def test_whiten_inverts_the_replayed_draw():
    kinds = synth.ALT_MODEL
    N = 300
    t, y, dy = synth.make_lightcurves(N, 1, seed=8)
    coeffs = dense.build_coeffs(kinds, synth.truth(kinds))
    fac = WR.factor(t, R.diagonal(dy[0], coeffs), coeffs)
    q0 = np.random.default_rng(1).standard_normal((2, N))
    back = WR.whiten(t, dy[0], coeffs, R.draw(t, dy[0], coeffs, q0, mean=3.0, factors=fac), mean=3.0, factors=fac)
    for b in range(2):
        s = R.scale_at(t, coeffs, fac, q0[b], np.arange(N))
        assert np.all(np.abs(back[b] - q0[b]) <= 2.0 * 64.0 * np.sqrt(N) * U * s / np.sqrt(fac[3]))


def test_header_and_exports():
    text = open(os.path.join(ROOT, "include", "mtg.h")).read()
    flat = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    flat = re.sub(r"\s+", " ", flat)
    assert "#define MTG_WHITEN_NSTATS 8" in text and _engine.WHITEN_NSTATS == 8
    assert ("MTG_API int mtg_whiten(mtg_ctx *ctx, int64_t B, const double *theta, const int32_t *lc_index, const double *y , "
            "double *q , int K, double *acf , double *stats , int32_t *status);") in flat
    assert "mtg_whiten" in _engine.EXPORTS


def plan(N, B, window, sorted_rows=False):
    """mtg_plan_whiten_slab through a host compile of the planner's header, as tests/test_solve_plan_cpu.py reaches it"""
    return _planner().mtg_test_plan_whiten_slab(N, B, window, int(sorted_rows))


_lib = None


def _planner():
    global _lib
    if _lib is None:
        import tempfile
        d = tempfile.mkdtemp(prefix="mtg_whiten_plan_")
        src = os.path.join(d, "plan.cpp")
        with open(src, "w") as f:
            f.write('#include <cstdint>\n#include <cstddef>\n#include "mtg_solve_plan.h"\n'
                    'extern "C" long long mtg_test_plan_whiten_slab(long long N, long long B, unsigned long long w, int sorted)\n'
                    '{ return mtg_plan_whiten_slab(N, B, w, sorted != 0); }\n')
        out = os.path.join(d, "plan.so")
        subprocess.check_call(["c++", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "mind_the_gaps_amd", "csrc"),
                               "-I", os.path.join(ROOT, "include"), src, "-o", out])
        _lib = ctypes.CDLL(out)
        _lib.mtg_test_plan_whiten_slab.restype = ctypes.c_longlong
        _lib.mtg_test_plan_whiten_slab.argtypes = [ctypes.c_longlong, ctypes.c_longlong, ctypes.c_ulonglong, ctypes.c_int]
    return _lib


def test_slab_planner_boundaries():
    full = 0xFFFFFFFF
    table = [
        # N, B, window -> rows of a slab
        (200000, 130, full, 128),          # 256 MiB / 1.6 MB = 167 rows -> whole workgroups: the draw's slab
        (200000, 100, full, 100),          # all B rows
        (10000, 2000, full, 2000),         # 3355 rows fit
        (10000, 5000, full, 3328),
        (1, 10 ** 6, full, 65472),         # the autocorrelation's grid: at most 65472 rows
        (300, 130, 300 * 16, 64),          # the window: two rows' worth -> the floor of one workgroup
        (300, 37, 300 * 16, 37),
        (1000, 1000, 1000 * 8 * 128, 128), # exactly 128 rows within the window
        (1000, 1000, 1000 * 8 * 128 - 1, 64),
        (4 * 10 ** 7, 200, full, 64),      # a row beyond the budget: still one workgroup
    ]
    for N, B, window, want in table:
        assert plan(N, B, window) == want, (N, B, window, plan(N, B, window), want)
    # where the rows are sorted for the KS distances a slab holds fewer than 2^31 samples, down to one row
    for N, B, want in ((4 * 10 ** 7, 200, 53), (2 ** 31 - 1, 5, 1), (2 ** 25, 200, 63), (2 ** 25 - 1, 200, 64), (10000, 2000, 2000)):
        assert plan(N, B, full, True) == want and want * N <= 2 ** 31 - 1, (N, B, plan(N, B, full, True), want)


class FakeEngine:
    """Engine.whiten answered by the replay for one light curve and one parameter-free white model: q = y / sd"""

    def __init__(self, q):
        self.q = np.atleast_2d(q)
        self.calls = []

    def whiten(self, theta, lc_index=None, y=None, residuals=True, lags=0, stats=True):
        self.calls.append(dict(B=len(theta), residuals=residuals, lags=lags, stats=stats))
        B = len(theta)
        q = self.q[np.arange(B) % len(self.q)]
        st = np.array([WR.row_stats(r, np.ones(len(r))) for r in q]) if stats else None
        acf = np.array([WR.acf(r, lags) for r in q]) if lags else None
        return (q if residuals else None), acf, st, np.zeros(B, dtype=np.int32)


def test_residual_diagnostics_host_arithmetic():
    from scipy import stats as sps
    from mind_the_gaps_amd.gpmodelling import GPModelling, whiten_diagnostics
    N = 400
    rng = np.random.default_rng(4)
    q = np.vstack([rng.standard_normal(N), 1.2 * rng.standard_normal(N) + 0.1, np.convolve(rng.standard_normal(N + 2), [1, 1, 1], "valid")])
    fake = FakeEngine(q)

    class Model:                # what residual_diagnostics reads of a GPModelling
        _mcmc_samples = None
        _whiten_rows = GPModelling._whiten_rows
        residual_diagnostics = GPModelling.residual_diagnostics
        whitened_residuals = GPModelling.whitened_residuals

        class _lightcurve:
            times, y = np.arange(N, dtype=np.float64), np.zeros(N)

        class gp:
            _has_profile_mean = staticmethod(lambda: False)
            _raise_for = staticmethod(lambda status: None)
            get_parameter_vector = staticmethod(lambda: np.zeros(2))

            @staticmethod
            def _bound_engine(y):
                import types
                return fake, types.SimpleNamespace(y_offset=0.0)

    m = Model()
    d = m.residual_diagnostics(np.zeros((3, 2)))
    assert fake.calls[-1] == dict(B=3, residuals=False, lags=N // 4, stats=True)      # no [B][N] array comes back
    K = N // 4
    for b in range(3):
        ks = sps.ks_1samp(q[b], sps.norm.cdf)
        assert abs(d["ks_statistic"][b] - ks.statistic) <= 8 * U and abs(d["ks_pvalue"][b] - ks.pvalue) <= 1e-9 * ks.pvalue
        assert abs(d["chi2"][b] - q[b] @ q[b]) <= 1e-12 * (q[b] @ q[b])
        assert abs(d["skewness"][b] - sps.skew(q[b])) <= 1e-10
        assert abs(d["excess_kurtosis"][b] - sps.kurtosis(q[b])) <= 1e-10
        full = np.correlate(q[b], q[b], mode="full")
        acf = full[N:N + K] / full[N - 1]
        assert np.allclose(d["acf"][b], acf, rtol=0, atol=4 * N * U)
        lb = N * (N + 2.0) * np.sum(acf ** 2 / (N - np.arange(1, K + 1)))
        assert abs(d["ljung_box"][b] - lb) <= 1e-10 * lb
        assert abs(d["ljung_box_pvalue"][b] - sps.chi2.sf(lb, K)) <= 1e-9 * sps.chi2.sf(lb, K) + 1e-300
        assert d["max_abs"][b] == np.max(np.abs(q[b]))
    assert d["acf_band"] == 1.96 / np.sqrt(N)
    assert d["ks_pvalue"][0] > 1e-3 and d["ljung_box_pvalue"][2] < 1e-6      # white noise passes, a moving average does not
    one = m.residual_diagnostics(lags=5)
    assert np.ndim(one["ks_statistic"]) == 0 and one["acf"].shape == (5,)
    with pytest.raises(ValueError):
        m.residual_diagnostics(lags=0)
    assert m.whitened_residuals(np.zeros(2)).shape == (N,)
    assert whiten_diagnostics(np.full((1, 8), np.nan), np.full((1, 3), np.nan), N)["ks_pvalue"].shape == (1,)
