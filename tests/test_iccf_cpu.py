"""The interpolated cross-correlation function (mtg_iccf) without a GPU:

* the fixture tests/golden/iccf_golden.npz (scripts/make_iccf_golden.py): its layout, companions and lag sets, the exact
  counts against the float64 helper tests/iccf_numpy.py, the ties, what each lag set is there for;
* the helper's values against the exact truth within its recorded rho;
* the planner csrc/mtg_iccf_plan.h through tests/iccf_plan_driver.cpp against a restatement and its budget;
* the compiler's resource report: every instantiation, no scratch, no spills, two waves per SIMD or more;
* the entry declared, exported and bound with the header's arity; a null context;
* the host argument checks of Engine.iccf, timedomain.iccf_lags and InterpolatedCrossCorrelation;
* the definition on hand-made series;
* the bookkeeping of ppp.iccf_significance with the stand-ins of tests/ppp_fakes.py and a numpy engine.
"""
import os
import re
import subprocess
import tempfile
import types

import numpy as np
import pytest

import iccf_numpy as inp
from mind_the_gaps_amd import engine, timedomain

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "iccf_golden.npz"))


@pytest.fixture(scope="module")
def ls_golden():
    return np.load(os.path.join(HERE, "golden", "lomb_scargle_golden.npz"))


@pytest.mark.parametrize("name", inp.CASES)
def test_fixture_layout_counts_and_ties(golden, ls_golden, name):
    assert tuple(str(c) for c in golden["cases"]) == inp.CASES and tuple(str(c) for c in golden["lag_sets"]) == inp.LAG_SETS
    assert os.path.getsize(os.path.join(HERE, "golden", "iccf_golden.npz")) < 1 << 19
    t, y = (ls_golden["%s/%s" % (name, k)] for k in ("t", "y"))
    t2, y2 = golden[name + "/t2"], golden[name + "/y2"]
    made = inp.companion(name, t, y)
    assert len(t2) == inp.COMPANION_M[name] and np.array_equal(made[0], t2) and np.allclose(made[1], y2, rtol=1e-13, atol=0)
    sets = inp.lag_sets(t, t2)
    sizes = dict(sym65=65, one=1, fine257=257, shuffled=67)
    for tag in inp.LAG_SETS:
        key = "%s/%s/" % (name, tag)
        lags = golden[key + "lags"]
        K = len(lags)
        assert np.array_equal(lags, sets[tag]) and K == sizes.get(tag, K) and 1 <= K <= engine.ICCF_MAX_LAGS
        got = inp.iccf(t, y, t2, y2, lags)
        for h in "ab":
            r, lo, n, s, rho = (golden[key + q % h] for q in ("r_%s", "r_%s_lo", "n_%s", "s_%s", "rho_%s"))
            assert r.shape == lo.shape == n.shape == s.shape == rho.shape == (K,) and n.dtype == np.int64
            assert np.array_equal(n, got["n_" + h])                              # brackets and counts are exact
            fin = np.isfinite(r)
            assert np.all(np.isnan(r[n < 2])) and np.array_equal(fin, np.isfinite(s)) and np.array_equal(fin, np.isfinite(lo))
            assert np.all(np.abs(r[fin]) <= 1.0) and np.all(np.abs(lo[fin]) <= 2.0 ** -53 * np.abs(r[fin])) and np.all(rho >= 0)
            # the bound is not vacuous: at least half of the finite entries have a scale of 100 or less
            assert not fin.any() or 2 * np.sum(s[fin] <= 100.0) >= fin.sum()
            assert np.all(rho[fin] <= 64 * 2.0 ** -53 * np.sqrt(n[fin]) * s[fin])     # (numpy itself is within the device's bound)
    # what each lag set is there for
    sym = golden[name + "/sym65/lags"]
    assert np.array_equal(sym, -sym[::-1]) and sym[-1] == 0.5 * min(t[-1] - t[0], t2[-1] - t2[0])
    assert np.all(np.isfinite(golden[name + "/sym65/r_a"])) and np.all(np.isfinite(golden[name + "/fine257/r_b"]))
    n_all = np.concatenate([golden[name + "/beyond/n_a"], golden[name + "/beyond/n_b"]])
    assert np.any(n_all == 0) and np.any(n_all == 1) and np.any(np.isnan(golden[name + "/beyond/r_a"]))
    assert np.any(np.isfinite(golden[name + "/beyond/r_a"])) and golden[name + "/beyond/n_a"][0] == 0 == golden[name + "/beyond/n_a"][22]
    m = inp.shuffle_map()
    assert sorted(set(m.tolist())) == list(range(65)) and len(m) == 67 and not np.array_equal(m[:65], np.arange(65))
    for q in ("r_a", "r_b", "n_a", "n_b"):
        assert np.array_equal(golden["%s/shuffled/%s" % (name, q)], golden["%s/sym65/%s" % (name, q)][m], equal_nan=True)
    # ties: every lag puts at least one shifted resident sample exactly on a companion node, the span's ends among them
    lags, ties = golden[name + "/ties/lags"], golden[name + "/ties/tie_pairs"]
    assert set(ties[:, 0].tolist()) == set(range(len(lags))) and {0, len(t2) - 1} <= set(ties[:, 2].tolist()) and 0.0 in lags
    for k, i, j in ties:
        assert t[i] + lags[k] == t2[j]
        # on the node the interpolant is the node's value: the last of a group of equal times
        s = y2 - np.mean(y2)
        last = np.flatnonzero(t2 == t2[j])[-1]
        assert inp.interpolate(t2, s, np.array([t[i] + lags[k]]))[0][0] == s[last]


@pytest.mark.parametrize("name", inp.CASES)
def test_numpy_helper_matches_the_truth(golden, ls_golden, name):
    t, y = (ls_golden["%s/%s" % (name, k)] for k in ("t", "y"))
    t2, y2 = golden[name + "/t2"], golden[name + "/y2"]
    for tag in inp.LAG_SETS:
        key = "%s/%s/" % (name, tag)
        got = inp.iccf(t, y, t2, y2, golden[key + "lags"])
        for h in "ab":
            r, lo = golden[key + "r_" + h], golden[key + "r_%s_lo" % h]
            assert np.array_equal(np.isnan(got["r_" + h]), np.isnan(r))
            fin = np.isfinite(r)
            err = np.abs((got["r_" + h][fin] - r[fin]) - lo[fin])
            assert np.all(err <= golden[key + "rho_" + h][fin] * (1 + 1e-9) + 1e-300), (tag, h)
            assert np.allclose(got["s_" + h][fin], golden[key + "s_" + h][fin], rtol=1e-6)


def planned(K, L, shared, per, half, arrays, rows, limit=0):
    """csrc/mtg_iccf_plan.h restated"""
    limit = limit or 1 << 28
    tile = 1 if not shared or L == 1 else 4
    slab = min(max(limit // (arrays * K * 8 * tile) * tile, tile), L)
    lag_blocks = -(-K // 256)
    blocks = lag_blocks * -(-rows // tile)
    return tile, int(bool(per)), int(not half), arrays, lag_blocks, slab, arrays * slab * K * 8, 0, blocks if blocks <= 0x7fffffff else 0


def test_planner_matches_its_restatement_and_its_budget():
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "iccf_plan_driver")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "mind_the_gaps_amd", "csrc"),
                               os.path.join(HERE, "iccf_plan_driver.cpp"), "-o", exe])
        ask = lambda cases: [tuple(int(v) for v in line.split()) for line in subprocess.run(
            [exe], input="".join("%d %d %d %d %d %d %d %d\n" % c for c in cases), capture_output=True, text=True, check=True).stdout.splitlines()]
        cases = [(K, L, shared, per, half, arrays, rows, limit) for K in (1, 65, 256, 257, 500, 65536) for L in (1, 2, 4, 5, 11, 173, 2000, 1 << 24)
                 for shared in (0, 1) for per in (0, 1) for half in (0, 1) for arrays in (1, 2, 3) for rows in (1, L) for limit in (0, 1 << 16)]
        got = ask(cases)
        assert len(got) == len(cases)
        seen = set()
        for c, g in zip(cases, got):
            assert g == planned(*c), (c, g)
            K, L, shared, per, half, arrays, rows, limit = c
            tile, per_, full, arrays_, lag_blocks, slab, out_bytes, lds, blocks = g
            seen.add((tile, per_, full))
            assert (shared and L > 1 or tile == 1) and full == 1 - half and per_ == per and lds == 0
            assert 1 <= slab <= L and (slab % tile == 0 or slab == L)
            # the outputs' device copies stay within the limit unless one tile's alone are more
            assert out_bytes <= max(limit or 1 << 28, arrays * tile * K * 8)
            assert lag_blocks * 256 >= K > (lag_blocks - 1) * 256
        assert seen == {(r, p, a) for r in (1, 4) for p in (0, 1) for a in (0, 1)}      # every instantiation is reached
        # the set of the GPU test's two slabs: 65536 lags and all three arrays take 1.5 MiB per light curve, 170 fit 256 MiB,
        # 168 in whole tiles of four on shared sampling: L = 169 .. is cut in two; 173 leaves a second slab with a part tile
        K, L = inp.TWO_SLABS["K"], inp.TWO_SLABS["L"]
        assert [g[5] for g in ask([(K, n, 1, 0, 0, 3, n, 0) for n in (168, 169, L)])] == [168, 168, 168]
        assert ask([(K, L, 0, 0, 0, 3, L, 0)])[0][5] == 170 and ask([(K, L, 1, 0, 0, 1, L, 0)])[0][5] == L
        # the headline set: 2000 light curves at 500 lags is one slab whatever is asked for
        assert ask([(500, 2000, 1, 0, 0, 3, 2000, 0)])[0] == (4, 0, 1, 3, 2, 2000, 3 * 2000 * 500 * 8, 0, 2 * 500)


def test_resource_report_lists_every_instantiation_without_scratch():
    rows = [line.split() for line in open(os.path.join(ROOT, "profiles", "iccf_resources.txt")) if line.startswith("mtg_")]
    names = {" ".join(r[:-8]): r for r in rows}
    word = {True: "true", False: "false"}
    for tile in (1, 4):
        for per in (True, False):
            for full in (True, False):
                r = names["mtg_iccf_kernel<%d, %s, %s>" % (tile, word[per], word[full])]
                assert int(r[-7]) <= 256 and int(r[-4]) >= 2 and int(r[-1]) == 0       # VGPRs, waves per SIMD, LDS
    assert "mtg_iccf_peak_kernel" in names and len(rows) == 9
    for r in rows:
        assert r[-5] == "0" and r[-3] == "0" and r[-2] == "0", r   # scratch, SGPR and VGPR spills


def test_entry_is_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "mtg.h")).read()
    plan = open(os.path.join(ROOT, "mind_the_gaps_amd", "csrc", "mtg_iccf_plan.h")).read()
    assert "MTG_ICCF_MAX_LAGS = 65536" in text and "MTG_ICCF_PLAN_MAX_LAGS = 65536" in plan and engine.ICCF_MAX_LAGS == 65536
    assert "MTG_ICCF_BOTH = 0, MTG_ICCF_COMPANION = 1, MTG_ICCF_RESIDENT = 2" in text
    assert engine.ICCF_MODES == dict(both=0, companion=1, resident=2) and tuple(engine.ICCF_MODES) == inp.MODES
    lib = engine.load_library()
    params = ["ctx", "M", "t2", "L2", "y2", "K", "tau", "mode", "threshold", "ccf", "n_a", "n_b", "peak", "peak_index", "centroid"]
    decl = re.search(r"MTG_API\s+int\s+mtg_iccf\s*\(([^;]*)\)\s*;", text)
    got = [p.split()[-1].lstrip("*") for p in re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).split(",")]
    assert got == params and "mtg_iccf" in engine.EXPORTS and len(lib.mtg_iccf.argtypes) == len(params)
    assert engine.Iccf._fields == tuple(params[9:])
    for unit in ("Makefile", "mtg_device.h"):
        assert "mtg_iccf" in open(os.path.join(ROOT, "mind_the_gaps_amd", "csrc", unit)).read()
    # the kernel keeps to the header's operation order: no contraction, no atomics
    src = open(os.path.join(ROOT, "mind_the_gaps_amd", "csrc", "mtg_iccf.hip")).read()
    assert "fp contract(off)" in src and "atomic" not in src.replace("No atomics", "")
    # no context: an argument error, nothing touched
    assert lib.mtg_iccf(None, 2, None, 1, None, 1, None, 0, 0.8, *([None] * 6)) == engine.E_ARG


def test_host_argument_checks():
    eng = types.SimpleNamespace(L=2, _lib=None, _ctx=None)
    call = lambda *a, **k: engine.Engine.iccf(eng, *a, **k)
    t2, y2 = np.array([0.0, 1.0, 2.0]), np.array([1.0, 2.0, 0.5])
    for args, kwargs in (((t2, y2, [0.0]), dict(mode="neither")), ((t2, y2, [0.0]), dict(values=False)), ((t2, y2, []), {}),
                         ((t2, y2, np.zeros(65537)), {}), ((t2, y2, [0.0]), dict(threshold=0.0)), ((t2, y2, [0.0]), dict(threshold=1.5)),
                         ((t2, y2[:2], [0.0]), {}), ((t2[None, :], y2, [0.0]), {}), ((t2, np.zeros((2, 2, 3)), [0.0]), {})):
        with pytest.raises(ValueError):
            call(*args, **kwargs)

    t1 = np.array([0.0, 1.0, 1.5, 4.0, 9.0])
    g = timedomain.iccf_lags(t1, t2, n=5)
    assert np.array_equal(g, [-1.0, -0.5, 0.0, 0.5, 1.0])                  # half the shorter span
    assert np.array_equal(timedomain.iccf_lags(t1, t2, n=3, max_lag=4.0), [-4.0, 0.0, 4.0]) and len(timedomain.iccf_lags(t1, t2)) == 201
    for kwargs in (dict(n=0), dict(n=65537), dict(n=4, max_lag=0.0), dict(n=4, max_lag=-1.0), dict(n=4, max_lag=np.inf)):
        with pytest.raises(ValueError):
            timedomain.iccf_lags(t1, t2, **kwargs)
    with pytest.raises(ValueError):
        timedomain.iccf_lags(t1, t2[:1], 4)
    y1 = np.sin(t1)
    for args in ((t1, y1[:3], t2, y2), (t1, y1, t2, y2[:2]), (t1[::-1], y1, t2, y2), (t1, y1, t2[::-1], y2), (t1, y1, t2, np.stack([y2, y2])),
                 (t1, np.stack([y1, y1]), t2, np.stack([y2, y2, y2])), (t1[:1], y1[:1], t2, y2), (t1, y1, t2[:1], y2[:1])):
        with pytest.raises(ValueError):
            timedomain.InterpolatedCrossCorrelation(*args)
    assert timedomain.InterpolatedCrossCorrelation(t1, np.stack([y1, y1]), t2, y2).y2.shape == (3,)

    from mind_the_gaps_amd import ppp
    for bad in (dict(mode="neither"), dict(threshold=0.0)):
        with pytest.raises(ValueError):
            ppp.iccf_significance(None, None, None, g, **bad)
    import inspect
    sig, ref = inspect.signature(ppp.iccf_significance).parameters, inspect.signature(ppp.cross_lag_significance).parameters
    assert list(sig)[:4] == ["lightcurve", "companion", "null_kernel", "lags"] and sig["mode"].default == "both" and sig["threshold"].default == 0.8
    for k in ("nsims", "levels", "walkers", "max_steps", "sigma_noise", "extension_factor", "seed", "device", "progress", "pdf", "max_iter"):
        assert sig[k].default == ref[k].default, k


def test_the_definition_on_hand_made_series():
    rng = np.random.default_rng(3)
    t = np.sort(rng.uniform(0.0, 64.0, 40))
    y = np.sin(t / 5.0) + 0.1 * rng.standard_normal(40)
    # identical series at lag 0: every sample sits on its own node, r = 1 in all three modes
    got = inp.iccf(t, y, t, y, [0.0])
    for mode in inp.MODES:
        assert abs(inp.combine(mode, got["r_a"], got["r_b"])[0] - 1.0) <= 4 * 2.0 ** -52
    assert got["n_a"][0] == got["n_b"][0] == 40
    # a companion that IS the resident series shifted by d on a grid: at tau = d the companion is sampled on its nodes
    g = np.arange(32, dtype=np.float64)
    z = np.cos(g / 3.0)
    d = 4.0
    got = inp.iccf(g, z, g + d, z, [d, d - 0.5])
    assert abs(got["r_a"][0] - 1.0) <= 4 * 2.0 ** -52 and got["n_a"][0] == 32 and got["r_a"][1] < 1.0 - 1e-4 and got["n_a"][1] == 31
    # a constant companion has no variance: NaN, never an infinity; so has a half with fewer than two samples
    got = inp.iccf(t, y, t, np.full(40, 2.5), [0.0, 1.0])
    assert np.all(np.isnan(got["r_a"])) and np.all(np.isnan(got["r_b"])) and got["n_a"][0] == 40
    far = inp.iccf(t, y, t, y, [63.9, 1000.0])
    assert np.all(np.isnan(far["r_a"])) and far["n_a"].tolist() == [int(np.sum(t + 63.9 <= t[-1])), 0]
    # nothing is extrapolated, and at equal times the last of the group is the left node
    u, zz = np.array([0.0, 1.0, 1.0, 2.0]), np.array([0.0, 5.0, 7.0, 9.0])
    v, p = inp.interpolate(u, zz, np.array([0.0, 0.5, 1.0, 1.5, 2.0]))
    assert v.tolist() == [0.0, 2.5, 7.0, 8.0, 9.0] and p.tolist() == [0, 0, 2, 2, 3]


class NumpyEngine:
    """Engine.set_lightcurves and Engine.iccf by tests/iccf_numpy.py, with a log of the calls"""

    def __init__(self):
        self.calls = []

    def set_lightcurves(self, t, y, dy):
        self.t, self.Y = np.asarray(t), np.atleast_2d(y)
        self.L = len(self.Y)
        self.calls.append(("set_lightcurves", self.Y.shape))

    def iccf(self, t2, y2, lags, mode="both", threshold=0.8, values=True, counts=False, peak=False):
        assert np.ndim(y2) == 1                       # one companion for the whole set: L2 = 1
        self.calls.append(("iccf", self.Y.shape, mode, threshold, values, counts, peak))
        per = [inp.iccf(self.t, row, t2, y2, lags) for row in self.Y]
        ccf = np.stack([inp.combine(mode, p["r_a"], p["r_b"]) for p in per])
        fin = np.isfinite(ccf)
        index = np.where(fin.any(axis=1), np.argmax(np.where(fin, ccf, -np.inf), axis=1), -1)
        top = np.where(index >= 0, ccf[np.arange(len(ccf)), np.maximum(index, 0)], np.nan)
        centroid = timedomain.lag_peak_and_centroid(np.tile(lags, (len(ccf), 1)), ccf, threshold)[1]
        return engine.Iccf(ccf, np.stack([p["n_a"] for p in per]) if counts else None, np.stack([p["n_b"] for p in per]) if counts else None,
                           top, index, centroid)


def test_iccf_significance_bookkeeping_on_the_host():
    import ppp_fakes
    from mind_the_gaps_amd import gp, ppp, simulator
    nsims = 9
    lc = ppp_fakes.lightcurve()
    rng = np.random.default_rng(8)
    lc.y, lc.dy = 50.0 + rng.standard_normal(ppp_fakes.N_TIMES), np.full(ppp_fakes.N_TIMES, 0.3)
    comp = types.SimpleNamespace(times=np.sort(rng.uniform(2.0, 14.0, 9)), y=rng.standard_normal(9), dy=None)
    lags = np.array([-4.0, -1.0, 0.0, 1.5, 3.0, 40.0])       # the last lag leaves no overlap
    eng = NumpyEngine()
    seen = {}

    class Simulator(ppp_fakes.Simulator):
        def simulate(self, samples, make_resident=False, seed=None):
            seen.update(make_resident=make_resident, seed=seed, samples=np.array(samples))
            g = np.random.default_rng(seed)
            rates = 50.0 + g.standard_normal((len(samples), ppp_fakes.N_TIMES))
            rates[2] = lc.y                                       # one simulation IS the observation: a tie at every lag and in the peak
            out = dict(rates=rates, dy=np.full_like(rates, 0.3))
            eng.set_lightcurves(lc.times, out["rates"], out["dy"])
            return out

    def run(seed, which="iccf"):
        del eng.calls[:]
        real = gp.get_engine
        with ppp_fakes.installed():
            simulator.Simulator, gp.get_engine = Simulator, lambda device: eng
            try:
                if which == "cross":
                    return ppp._simulate_null_set(lc, ppp_fakes.Kernel(ppp_fakes.NULL_SIZE), nsims, 8, 10, None, 2, seed, 0, False, "Gaussian", 400)
                return ppp.iccf_significance(lc, comp, ppp_fakes.Kernel(ppp_fakes.NULL_SIZE), lags, nsims=nsims, levels=(0.9,),
                                             mode="companion", threshold=0.5, walkers=8, max_steps=10, seed=seed)
            finally:
                gp.get_engine = real
    res = run(5)
    assert seen["make_resident"] is True and seen["samples"].shape == (nsims, ppp_fakes.NULL_SIZE) and res["sim_seed"] == seen["seed"]
    # the observation alone, then ONE call on the simulated set
    assert eng.calls == [("set_lightcurves", (1, 12)), ("iccf", (1, 12), "companion", 0.5, True, True, True), ("set_lightcurves", (nsims, 12)),
                         ("iccf", (nsims, 12), "companion", 0.5, True, False, True)]
    # the null chain, the picks and the simulated set are the ones every test of this family takes for the seed
    _, _, samples, sim_seed, out = run(5, "cross")
    assert np.array_equal(samples, res["samples"]) and sim_seed == res["sim_seed"] and np.array_equal(out["rates"], res["lightcurves"]["rates"])
    # the statistic restated
    want = inp.iccf(lc.times, lc.y, comp.times, comp.y, lags)
    assert np.array_equal(res["observed"], want["r_a"], equal_nan=True) and np.array_equal(res["n_a"], want["n_a"]) and np.array_equal(res["n_b"], want["n_b"])
    assert np.isnan(res["observed"][-1]) and np.all(np.isfinite(res["observed"][:5])) and res["sims"].shape == (nsims, 6)
    assert np.array_equal(res["sims"][2], res["observed"], equal_nan=True) and np.array_equal(res["lags"], lags)
    ok = np.isfinite(res["observed"])
    assert res["peak"] == np.max(res["observed"][ok]) and res["peak_lag"] == lags[ok][np.argmax(res["observed"][ok])]
    assert res["centroid"] == timedomain.lag_peak_and_centroid(lags, res["observed"], 0.5)[1]
    assert res["sim_peaks"].shape == res["sim_peak_lags"].shape == res["sim_centroids"].shape == (nsims,)
    assert res["sim_peaks"][2] == res["peak"] and res["sim_peak_lags"][2] == res["peak_lag"]
    assert np.array_equal(res["sim_peaks"], np.nanmax(res["sims"], axis=1))
    above = int(np.sum(res["sim_peaks"] >= res["peak"]))
    assert 1 <= above <= nsims and res["p_global"] == (1.0 + above) / (1.0 + nsims)
    levels = ppp._lag_levels(res["observed"], res["sims"], (0.9,))
    assert all(np.array_equal(res[k], levels[k], equal_nan=True) for k in levels)
    # the same seed: the same bits; another seed: other simulations
    again, other = run(5), run(6)
    for k in ("observed", "sims", "sim_peaks", "sim_peak_lags", "sim_centroids", "median", "upper", "lower", "samples"):
        assert np.array_equal(res[k], again[k], equal_nan=True), k
    assert res["p_global"] == again["p_global"] and res["sim_seed"] == again["sim_seed"] != other["sim_seed"]
    assert not np.array_equal(res["sims"], other["sims"], equal_nan=True) and np.array_equal(res["observed"], other["observed"], equal_nan=True)
