"""CPU side of the prediction at new times (mtg_predict_at; tests/test_predict_at_vs_quad_gpu.py is the GPU side).

* tests/predict_at_replay.py -- the recurrence of mind_the_gaps_amd/csrc/mtg_predict_at.hip in numpy float64 -- against
  the quad truth of tests/golden/predict_at_golden.npz for every group with N <= 4096, within the bound the GPU test
  holds the kernel to (test_predict_vs_quad_gpu.bound: |out - T| <= max(10 rho, 64 sqrt(N) u) s).  This is the check of
  the formulas.
* The fixture is the oracle's: three small groups are recomputed with oracle.predict.predict_at and compared exactly as
  stored; the light curves are checked by SHA-256.
* mtg_predict_at is declared, exported and bound; without a GPU the engine raises (no host fallback).
"""
import json
import os
import re

import numpy as np
import pytest

import golden_util
import predict_at_replay
from mind_the_gaps_amd import engine
from oracle import dense
from oracle import predict as oracle_predict
from test_predict_vs_quad_gpu import bound

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = np.load(os.path.join(HERE, "golden", "predict_at_golden.npz"))
GROUPS = {g["name"]: g for g in json.loads(bytes(FIX["manifest"]))["groups"]}
SMALL = [n for n, g in GROUPS.items() if g["N"] <= 4096]
RECOMPUTED = ["typical/null_n64", "typical/alt_n65", "offset/seconds"]


def arrays(name):
    key = name.replace("/", ".") + "/"
    return {k[len(key):]: FIX[k] for k in FIX.files if k.startswith(key)}


def lightcurve(name):
    g = GROUPS[name]
    t, y, dy = golden_util.quad_lightcurve(g["lightcurve"])
    assert golden_util.lightcurve_sha256(t, y, dy) == g["sha256"], "%s: the light curve is not the fixture's" % name
    return t, y, dy


def test_fixture_covers_every_group():
    quad = [g["name"] for g in json.load(open(os.path.join(HERE, "golden", "quad_golden.json")))["groups"]]
    assert list(GROUPS) == quad + ["noise_dominated"]
    for name in GROUPS:
        a = arrays(name)
        rows = len(a["theta"])
        assert 1 <= rows <= 4 and a["ts"].shape == (48,)
        for v in ("mu", "var"):
            assert a[v].shape == (rows, 48) and a[v].dtype == np.float64
            assert a[v + "_c64err"].shape == (rows, 48) and a[v + "_scale"].shape == (rows, 48)
        assert np.array_equal(a["ts"], golden_util.new_times(lightcurve(name)[0], GROUPS[name]["ts_seed"]))


@pytest.mark.parametrize("name", SMALL)
def test_replay_against_quad_truth(name):
    """the formulas, in float64 on the host, within the kernel's bound of every small group"""
    g, a = GROUPS[name], arrays(name)
    t, y, dy = lightcurve(name)
    N = len(t)
    nk = dense.n_kernel_params(g["kinds"])
    for b, row in enumerate(a["theta"]):
        if g["mean_kind"] == 1:
            mean = lambda x, row=row: row[nk] * np.asarray(x) + row[nk + 1]
        else:
            mean = lambda x, row=row: np.full(len(x), row[nk])
        lc = a["lc"][b]
        mu, var = predict_at_replay.predict_at(t, y[lc], dy[lc] + 1e-12, dense.build_coeffs(g["kinds"], row[:nk]), mean,
                                               a["ts"])
        for v, out in (("mu", mu), ("var", var)):
            w = bound("replay %s / %s row %d" % (v, name, b), N, out[None, :], a[v][b][None, :],
                      a[v + "_c64err"][b][None, :], a[v + "_scale"][b][None, :])
            print("\nreplay %-4s %-28s row %d worst e/tol %.3g" % (v, name, b, w[0]))


@pytest.mark.parametrize("name", RECOMPUTED)
def test_fixture_is_the_oracles(name):
    g, a = GROUPS[name], arrays(name)
    t, y, dy = lightcurve(name)
    for b, row in enumerate(a["theta"]):
        lc = a["lc"][b]
        q = oracle_predict.predict_at(t, y[lc], dy[lc], g["kinds"], row, a["ts"], mean_kind=g["mean_kind"])
        c = oracle_predict.predict_at(t, y[lc], dy[lc], g["kinds"], row, a["ts"], mean_kind=g["mean_kind"], c64=True)
        assert q.status == 0 and c.status == 0
        for v, s in (("mu", "s_mu"), ("var", "s_var")):
            T, lo = getattr(q, v), getattr(q, v + "_lo")
            assert np.array_equal(T, a[v][b])
            assert np.array_equal(np.abs((getattr(c, v) - T) - lo).astype(np.float32), a[v + "_c64err"][b])
            assert np.array_equal(getattr(q, s).astype(np.float32), a[v + "_scale"][b])


def test_entry_is_declared_exported_and_bound():
    text = open(os.path.join(os.path.dirname(HERE), "include", "mtg.h")).read()
    assert re.search(r"MTG_API\s+int\s+mtg_predict_at\s*\(", text)
    assert "mtg_predict_at" in engine.EXPORTS
    lib = engine.load_library()
    assert hasattr(lib, "mtg_predict_at")
    assert lib.mtg_predict_at.argtypes is not None and len(lib.mtg_predict_at.argtypes) == 9
    assert callable(engine.Engine.predict_at)
    # no context: an argument error, nothing touched
    assert lib.mtg_predict_at(None, 1, None, None, 1, None, None, None, None) < 0


@pytest.mark.skipif(engine.device_count() > 0, reason="a GPU is present")
def test_no_host_fallback_without_gpu():
    with pytest.raises(engine.EngineUnavailable):
        engine.Engine(0).predict_at(np.zeros((1, 2)), np.zeros(3))
