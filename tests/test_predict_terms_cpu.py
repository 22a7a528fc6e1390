"""CPU side of the per-term prediction (mtg_predict_terms; tests/test_predict_terms_gpu.py is the GPU side).

* tests/predict_terms_replay.py -- the masked evaluation of mind_the_gaps_amd/csrc/mtg_predict_terms.hip in numpy
  float64 -- against the 50-digit dense truth of tests/golden/predict_terms_golden.npz (made by
  tests/golden/make_predict_terms_golden.py) for every group and every mask, within the bound the GPU test holds the
  kernel to (test_predict_vs_quad_gpu.bound: |out - T| <= max(10 rho, 64 sqrt(N) u) s).  This is the check of the
  formulas and of the fixture.
* every term selected, with the mean: equal to predict_at_replay.predict_at bit for bit.
* mtg_predict_terms is declared, exported and bound with the header's arity; GP.predict(kernel=...) refuses what is not
  a set of top-level terms of its own kernel.
"""
import json
import os
import re

import numpy as np
import pytest

import predict_at_replay
import predict_terms_replay
from mind_the_gaps_amd import engine, terms
from mind_the_gaps_amd.gp import GP
from mind_the_gaps_amd.models import DampedRandomWalk, Lorentzian
from oracle import dense
from test_predict_vs_quad_gpu import bound

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = np.load(os.path.join(HERE, "golden", "predict_terms_golden.npz"))
GROUPS = {g["name"]: g for g in json.loads(bytes(FIX["manifest"]))["groups"]}


def arrays(name):
    return {k[len(name) + 1:]: FIX[k] for k in FIX.files if k.startswith(name + "/")}


def host_model(name):
    """-> (arrays, per-term coefficients' owners, whole coefficients, mean function)"""
    g, a = GROUPS[name], arrays(name)
    offs = np.concatenate([[0], np.cumsum([dense.NPARAMS[k] for k in g["kinds"]])])
    per_term = [dense.build_coeffs([k], a["theta"][offs[i]:offs[i + 1]], [g["extra"][i]]) for i, k in enumerate(g["kinds"])]
    owner, whole = predict_terms_replay.slot_owners(per_term)
    nk = offs[-1]
    if g["mean_kind"] == 1:
        mean = lambda x: a["theta"][nk] * np.asarray(x) + a["theta"][nk + 1]
    else:
        mean = lambda x: np.full(len(x), a["theta"][nk])
    return a, owner, whole, mean


def test_fixture_layout():
    assert [GROUPS[n]["N"] for n in GROUPS] == [150, 150, 150, 150, 150, 150, 1, 65]
    for name, g in GROUPS.items():
        a = arrays(name)
        nt = len(g["kinds"])
        single = [1 << k for k in range(nt)]
        pairs = [(1 << i) | (1 << j) for i in range(nt) for j in range(i + 1, nt)]
        assert set(a["masks"]) == set(single + pairs + [(1 << nt) - 1, 0])
        T = len(a["masks"])
        ts, t = a["ts"], a["t"]
        assert ts.shape == (48,) and len(np.unique(ts)) <= 46              # two duplicates at least
        assert np.sum(ts < t[0]) >= 3 and np.sum(ts > t[-1]) >= 3
        on = [n for n in (0, 64, 128, len(t) - 1) if n < len(t)]
        assert all(t[n] in ts for n in on) and (len(t) == 1 or np.sum(np.isin(ts, t)) >= 6)
        for v in ("mu", "var", "mu_c64err", "var_c64err", "mu_scale", "var_scale"):
            assert a[v].shape == (T, 48) and np.all(np.isfinite(a[v]))


@pytest.mark.parametrize("name", list(GROUPS))
def test_replay_against_dense_truth(name):
    a, owner, whole, mean = host_model(name)
    N = len(a["t"])
    mu, var = predict_terms_replay.predict_terms(a["t"], a["y"], a["yerr"], whole, mean, a["ts"], owner, a["masks"], False)
    for v, out in (("mu", mu), ("var", var)):
        w = bound("replay %s / %s" % (v, name), N, out, a[v], a[v + "_c64err"], a[v + "_scale"])
        print("\nreplay %-4s %-20s worst e/tol %.3g" % (v, name, w[0]))
    if GROUPS[name]["mean_kind"] == 1:
        mu, _ = predict_terms_replay.predict_terms(a["t"], a["y"], a["yerr"], whole, mean, a["ts"], owner, a["masks"], True)
        bound("replay mu + mean / %s" % name, N, mu, a["mu"] + a["mean_ts"], a["mu_c64err"], a["mu_scale"] + np.abs(a["mean_ts"]))
    zero = list(a["masks"]).index(0)
    assert np.all(mu[zero] == (a["mean_ts"] if GROUPS[name]["mean_kind"] == 1 else 0.0)) and np.all(var[zero] == 0.0)


@pytest.mark.parametrize("name", list(GROUPS))
def test_all_terms_with_the_mean_is_predict_at_exactly(name):
    a, owner, whole, mean = host_model(name)
    full = (1 << len(GROUPS[name]["kinds"])) - 1
    mu, var = predict_terms_replay.predict_terms(a["t"], a["y"], a["yerr"], whole, mean, a["ts"], owner, [full], True)
    mu0, var0 = predict_at_replay.predict_at(a["t"], a["y"], a["yerr"], whole, mean, a["ts"])
    assert np.array_equal(mu[0], mu0) and np.array_equal(var[0], var0)


def test_owners_follow_the_damping_side():
    """SHO (Q = 0.3) + SHO (Q = 5) + DRW: real slots (0, 0, 2), pair (1, 1); with the two Q swapped (1, 1, 2), (0, 0)"""
    assert list(host_model("sho_over_first")[1]) == [0, 0, 2, 1, 1]
    assert list(host_model("sho_over_second")[1]) == [1, 1, 2, 0, 0]


def test_entry_is_declared_exported_and_bound():
    text = open(os.path.join(os.path.dirname(HERE), "include", "mtg.h")).read()
    decl = re.search(r"MTG_API\s+int\s+mtg_predict_terms\s*\(([^;]*)\)\s*;", text)
    assert decl and re.search(r"#define\s+MTG_TERMS_MEAN\s+\(1u << 31\)", text)
    params = re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).split(",")
    assert "mtg_predict_terms" in engine.EXPORTS and engine.TERMS_MEAN == 1 << 31
    lib = engine.load_library()
    assert lib.mtg_predict_terms.argtypes is not None and len(lib.mtg_predict_terms.argtypes) == len(params) == 11
    assert callable(engine.Engine.predict_terms)
    # no context: an argument error, nothing touched
    assert lib.mtg_predict_terms(None, 1, None, None, 1, None, 1, None, None, None, None) < 0


def test_gp_predict_refuses_a_kernel_that_is_not_its_own_terms():
    drw, lor = DampedRandomWalk(1.0, -1.0), Lorentzian(1.0, 2.0, 0.5)
    prod = terms.RealTerm(0.0, 0.0) * terms.RealTerm(0.1, 0.2)
    gp = GP(drw + lor + prod, mean=0.0)
    y = np.zeros(5)
    for foreign in (DampedRandomWalk(1.0, -1.0), prod.models["k1"] if hasattr(prod, "models") else object(), object(),
                    drw + DampedRandomWalk(1.0, -1.0), "terms[0]"):
        with pytest.raises(ValueError):
            gp.predict(y, kernel=foreign)
    assert gp._term_mask(drw) == 1 and gp._term_mask(lor) == 2 and gp._term_mask(lor + drw) == 3 and gp._term_mask(prod) == 4
