"""The lag-bin sums (mtg_lag_sums) without a GPU:

* the fixture tests/golden/lag_golden.npz (scripts/make_lag_golden.py): its layout and edge sets, the exact counts against
  the float64 helper tests/lag_numpy.py, the pairs that sit on an edge;
* the helper's sums against the exact truth, within the bounds the GPU test uses;
* the planner csrc/mtg_lag_plan.h through tests/lag_plan_driver.cpp against a restatement and its budget;
* the compiler's resource report: every instantiation, no scratch;
* the entry declared, exported and bound with the header's arity;
* model_structure_function against the helper's structure function of a simulated damped random walk;
* the argument checks of timedomain that need no device, and the host arithmetic of ppp.lag_significance.
"""
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import lag_numpy as ln
from mind_the_gaps_amd import engine, timedomain

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
VALUES = ("lag", "sf", "cf", "cf2", "noise")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "lag_golden.npz"))


@pytest.fixture(scope="module")
def ls_golden():
    return np.load(os.path.join(HERE, "golden", "lomb_scargle_golden.npz"))


@pytest.mark.parametrize("name", ln.CASES)
def test_fixture_layout_counts_and_ties(golden, ls_golden, name):
    assert tuple(str(c) for c in golden["cases"]) == ln.CASES and tuple(str(c) for c in golden["edge_sets"]) == ln.EDGE_SETS
    t, y, dy = (ls_golden["%s/%s" % (name, k)] for k in ("t", "y", "dy"))
    n = len(t)
    assert n == int(name[1:]) and n * (n - 1) // 2 <= 320000
    sets = ln.edge_sets(t)
    span = t[-1] - t[0]
    nbins = dict(linear8=8, log32=32, one=1, short5=5, wide128=128)
    i, j, tau = ln.pairs(t)
    for tag in ln.EDGE_SETS:
        key = "%s/%s/" % (name, tag)
        edges = golden[key + "edges"]
        assert np.array_equal(edges, sets[tag]) and edges[0] >= 0 and np.all(np.diff(edges) > 0)
        nb = len(edges) - 1
        assert nb == nbins.get(tag, nb) and 1 <= nb <= engine.LAG_MAX_BINS
        got = ln.lag_sums(t, y, dy, edges)
        assert golden[key + "count"].dtype == np.int64 and np.array_equal(golden[key + "count"], got["count"])
        for q in VALUES + ("cfabs",):
            assert golden[key + q].shape == (nb,) and golden[key + q + "_lo"].shape == (nb,)
            assert np.all(np.abs(golden[key + q + "_lo"]) <= 2.0 ** -53 * np.abs(golden[key + q]))
            assert np.all(golden[key + q][golden[key + "count"] == 0] == 0)
        for q in VALUES:
            assert 0 <= float(golden[key + "rho_" + q]) <= 1e-12
    # what each edge set is there for
    assert golden[name + "/short5/edges"][0] > 0 and np.isclose(golden[name + "/short5/edges"][-1], 0.1 * span)
    assert np.sum(tau >= golden[name + "/short5/edges"][-1]) > 0
    if n > 5:    # (the five samples of n5 have no pair that close: all its short5 bins are empty)
        assert np.sum(tau < golden[name + "/short5/edges"][0]) > 0 and golden[name + "/short5/count"].min() > 0
    wide = golden[name + "/wide128/count"]
    assert wide.sum() == n * (n - 1) // 2 and np.all(wide[:16] == 0) and np.all(wide[-30:] == 0) and golden[name + "/wide128/edges"][-1] > span
    assert golden[name + "/linear8/count"].sum() == n * (n - 1) // 2 - np.sum(tau >= span)   # the longest lag sits on the last edge
    # ties: every edge is a pair's lag; the pair is counted in the bin above the edge (none for the last edge)
    edges, ties = golden[name + "/ties/edges"], golden[name + "/ties/tie_pairs"]
    assert len(ties) >= len(edges)
    for a, b, where in ties:
        k = int(np.flatnonzero(edges == t[b] - t[a])[0])
        assert a < b and where == (k if k < len(edges) - 1 else -1)
    assert set(np.flatnonzero(np.isin(edges, t[ties[:, 1]] - t[ties[:, 0]]))) == set(range(len(edges)))
    # counted from the named pairs alone, the upper bins hold at least them
    for k in range(len(edges) - 1):
        assert golden[name + "/ties/count"][k] >= np.sum(ties[:, 2] == k) >= 1


@pytest.mark.parametrize("name", ln.CASES)
def test_numpy_helper_matches_the_truth(golden, ls_golden, name):
    t, y, dy = (ls_golden["%s/%s" % (name, k)] for k in ("t", "y", "dy"))
    for tag in ln.EDGE_SETS:
        key = "%s/%s/" % (name, tag)
        got = ln.lag_sums(t, y, dy, golden[key + "edges"])
        count = golden[key + "count"]
        for q in VALUES:
            scale = np.abs(golden[key + ("cfabs" if q == "cf" else q)])
            err = np.abs((got[q] - golden[key + q]) - golden[key + q + "_lo"])
            assert np.all(err <= ln.bound(float(golden[key + "rho_" + q]), count, scale)), (tag, q)
            assert np.all(got[q][count == 0] == 0)


def planned(N, nbins, L, shared, what, rows):
    """csrc/mtg_lag_plan.h restated"""
    tile = 1 if not shared or L == 1 else 4 if L <= 4 else 8
    full = 1 if what & ~4 else 0
    per_lc, per_tile = (4, 2) if full else (1, 0)
    bytes_of = lambda r: (per_lc * r + per_tile * -(-r // tile)) * nbins * N * 8
    slab = min(max((1 << 30) // bytes_of(tile) * tile, tile), L)
    lds = 2048 + 8 * 130 + (24 if full else 8) * tile * 256
    row_blocks = -(-N // 256)
    blocks = row_blocks * -(-rows // tile)
    return tile, full, per_lc, per_tile, row_blocks, slab, bytes_of(slab), lds, blocks if blocks <= 0x7fffffff else 0


def test_planner_matches_its_restatement_and_its_budget():
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "lag_plan_driver")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "mind_the_gaps_amd", "csrc"),
                               os.path.join(HERE, "lag_plan_driver.cpp"), "-o", exe])
        cases = [(N, nbins, L, shared, what, rows) for N in (2, 5, 256, 257, 789, 10000, 1 << 20, 1 << 26) for nbins in (1, 8, 50, 128)
                 for L in (1, 2, 4, 5, 11, 90, 2000) for shared in (0, 1) for what in (4, 1, 63, 12) for rows in (1, L)]
        r = subprocess.run([exe], input="".join("%d %d %d %d %d %d\n" % c for c in cases), capture_output=True, text=True, check=True)
        got = [tuple(int(v) for v in line.split()) for line in r.stdout.splitlines()]
        assert len(got) == len(cases)
        seen = set()
        for c, g in zip(cases, got):
            assert g == planned(*c), (c, g)
            N, nbins, L, shared, what, rows = c
            tile, full, per_lc, per_tile, row_blocks, slab, ws, lds, blocks = g
            seen.add((tile, full))
            assert (shared and L > 1 or tile == 1) and full == (what != 4)
            assert 1 <= slab <= L and (slab % tile == 0 or slab == L)
            # the workspace stays within 1 GiB unless one tile's alone is more
            assert ws <= max(1 << 30, (per_lc * tile + per_tile) * nbins * N * 8)
            assert 2 * lds <= 160 * 1024 and lds <= 64 * 1024      # two workgroups on a CU; static LDS
            assert row_blocks * 256 >= N > (row_blocks - 1) * 256
        assert seen == {(r, a) for r in (1, 4, 8) for a in (0, 1)}
        # the headline set at 50 bins: sf alone in slabs of 256 light curves, everything in slabs of 56
        head = subprocess.run([exe], input="10000 50 2000 1 4 2000\n10000 50 2000 1 63 2000\n", capture_output=True, text=True, check=True).stdout.split()
        assert [int(v) for v in head] == [8, 0, 1, 0, 40, 264, 264 * 4000000, 19472, 40 * 250, 8, 1, 4, 2, 40, 56, (4 * 56 + 2 * 7) * 4000000, 52240, 40 * 250]


def test_resource_report_lists_every_instantiation_without_scratch():
    rows = [line.split() for line in open(os.path.join(ROOT, "profiles", "lag_resources.txt")) if line.startswith("mtg_")]
    names = {" ".join(r[:-8]): r for r in rows}
    for tile in (1, 4, 8):
        for full in (True, False):
            r = names["mtg_lag_kernel<%d, %s>" % (tile, "true" if full else "false")]
            assert int(r[-7]) <= 256 and int(r[-4]) >= 2                      # VGPRs, waves per SIMD
            assert int(r[-1]) == planned(300, 1, 1, 1, 63 if full else 4, 1)[7] + (24 if full else 8) * (tile - 1) * 256   # LDS as planned
        assert "mtg_lag_reduce_kernel<%d>" % tile in names
    for r in rows:
        assert r[-5] == "0" and r[-3] == "0" and r[-2] == "0", r   # scratch, SGPR and VGPR spills


def test_entry_is_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "mtg.h")).read()
    assert int(re.search(r"MTG_LAG_MAX_BINS\s*=\s*(\d+)", text).group(1)) == engine.LAG_MAX_BINS == 128
    plan = open(os.path.join(ROOT, "mind_the_gaps_amd", "csrc", "mtg_lag_plan.h")).read()
    assert int(re.search(r"MTG_LAG_PLAN_MAX_BINS\s*=\s*(\d+)", plan).group(1)) == engine.LAG_MAX_BINS
    lib = engine.load_library()
    params = ["ctx", "nbins", "edges", "count", "lag", "sf", "cf", "cf2", "noise"]
    decl = re.search(r"MTG_API\s+int\s+mtg_lag_sums\s*\(([^;]*)\)\s*;", text)
    got = [p.split()[-1].lstrip("*") for p in re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).split(",")]
    assert got == params and "mtg_lag_sums" in engine.EXPORTS and len(lib.mtg_lag_sums.argtypes) == len(params)
    assert tuple(params[3:]) == engine.LAG_SUMS == ln.SUMS
    assert set(engine.LAG_SUMS) <= set(engine.Engine.lag_sums.__code__.co_varnames)
    # no context: an argument error, nothing touched
    assert lib.mtg_lag_sums(None, 1, None, None, None, None, None, None, None) == engine.E_ARG


def test_model_structure_function_against_a_simulated_damped_random_walk():
    from mind_the_gaps_amd import terms
    # an exact AR(1) draw on an irregular grid: k(tau) = a exp(-c tau); 4000 samples over 400 time constants
    a, c, jitter = 2.0, 0.5, 0.3
    rng = np.random.default_rng(7)
    t = np.sort(rng.uniform(0.0, 800.0, 4000))
    y = np.empty(len(t))
    y[0] = np.sqrt(a) * rng.standard_normal()
    for n in range(1, len(t)):
        phi = np.exp(-c * (t[n] - t[n - 1]))
        y[n] = phi * y[n - 1] + np.sqrt(a * (1.0 - phi * phi)) * rng.standard_normal()
    dy = np.full(len(t), jitter)
    y = y + jitter * rng.standard_normal(len(t))
    kernel = terms.RealTerm(log_a=np.log(a), log_c=np.log(c))
    edges = timedomain.lag_bins(t, 12, spacing="log", min_lag=0.05, max_lag=20.0)
    sums = ln.lag_sums(t, y, dy, edges)
    lag, sf2, count = timedomain.sf_from_sums(sums, subtract_noise=True)
    model = timedomain.model_structure_function(kernel, lag)
    assert np.allclose(model, 2.0 * a * (1.0 - np.exp(-c * lag)))
    assert np.allclose(timedomain.model_structure_function(kernel, lag, jitter=jitter), model + 2.0 * jitter ** 2)
    # sampling error: the pairs of a bin are far from independent; with ~ 400 time constants of data the plateau 2 a is
    # known to ~ sqrt(2 / 400) = 7 %, the short lags better.  Stated factor: within 30 % + 4 noise terms' scatter.
    noise_scatter = 2.0 * jitter ** 2 * np.sqrt(8.0 / count)
    assert np.all(count > 50) and np.all(np.abs(sf2 - model) <= 0.30 * model + 4.0 * noise_scatter), (sf2, model)
    # without the noise term the curve sits higher by 2 sigma^2
    raw = timedomain.sf_from_sums(sums, subtract_noise=False)[1]
    assert np.allclose(raw - sf2, 2.0 * jitter ** 2)
    # and the correlation function at short lags is close to exp(-c tau)
    r = y - y.mean()
    _, dcf, err, _ = timedomain.dcf_from_sums(sums, np.mean(r * r), jitter ** 2)
    assert np.all(np.abs(dcf - np.exp(-c * lag)) <= 0.25) and np.all(err > 0)


def test_normalisations_on_hand_made_sums():
    sums = dict(count=np.array([[0, 1, 4]]), lag=np.array([[0.0, 2.0, 12.0]]), sf=np.array([[0.0, 3.0, 8.0]]),
                noise=np.array([[0.0, 1.0, 2.0]]), cf=np.array([[0.0, 0.5, 2.0]]), cf2=np.array([[0.0, 0.25, 1.5]]))
    lag, sf2, count = timedomain.sf_from_sums(sums)
    assert np.isnan(lag[0, 0]) and np.isnan(sf2[0, 0]) and np.array_equal(lag[0, 1:], [2.0, 3.0]) and np.array_equal(sf2[0, 1:], [2.0, 1.5])
    assert np.array_equal(timedomain.sf_from_sums(sums, subtract_noise=False)[1][0, 1:], [3.0, 2.0])
    lag, dcf, err, count = timedomain.dcf_from_sums(sums, np.array([1.25]), np.array([0.25]))
    assert np.isnan(dcf[0, 0]) and np.array_equal(dcf[0, 1:], [0.5, 0.5])
    assert np.isnan(err[0, 0]) and np.isnan(err[0, 1]) and err[0, 2] == np.sqrt(1.5 - 4.0 / 4.0) / 3.0


def test_argument_checks_that_need_no_device():
    t = np.array([0.0, 1.0, 1.5, 4.0, 9.0])
    e = timedomain.lag_bins(t, 4)
    assert len(e) == 5 and e[0] == 0.5 and e[-1] == 4.5 and np.allclose(np.diff(e), 1.0)
    g = timedomain.lag_bins(t, 3, spacing="log", min_lag=0.1, max_lag=100.0)
    assert np.allclose(g, [0.1, 1.0, 10.0, 100.0])
    assert timedomain.lag_bins(t, 2, min_lag=0.0)[0] == 0.0
    for kwargs in (dict(nbins=0), dict(nbins=129), dict(nbins=4, spacing="sqrt"), dict(nbins=4, min_lag=5.0), dict(nbins=4, min_lag=-1.0),
                   dict(nbins=4, max_lag=np.inf), dict(nbins=4, spacing="log", min_lag=0.0)):
        with pytest.raises(ValueError):
            timedomain.lag_bins(t, **kwargs)
    with pytest.raises(ValueError):
        timedomain.lag_bins(t[:1], 4)
    with pytest.raises(ValueError):
        timedomain.lag_bins(np.zeros(4), 4)
    y = np.sin(t)
    for cls in (timedomain.StructureFunction, timedomain.DiscreteCorrelation):
        with pytest.raises(ValueError):
            cls(t, y[:3])
        with pytest.raises(ValueError):
            cls(t[::-1], y)
        with pytest.raises(ValueError):
            cls(t[:1], y[:1])
        one = cls(t, y)
        assert one.dy is None and cls(t, np.stack([y, y]), 0.1).dy.shape == (2, 5)

    from mind_the_gaps_amd import ppp
    with pytest.raises(ValueError, match="statistic"):
        ppp.lag_significance(None, None, e, statistic="acf")
    import inspect
    sig, ref = inspect.signature(ppp.lag_significance).parameters, inspect.signature(ppp.periodogram_significance).parameters
    assert sig["statistic"].default == "sf" and sig["nsims"].default == 100 and sig["levels"].default == (0.95, 0.997)
    for k in ("walkers", "max_steps", "sigma_noise", "extension_factor", "seed", "device", "progress", "pdf", "max_iter"):
        assert sig[k].default == ref[k].default


def test_lag_significance_bookkeeping_on_the_host():
    from mind_the_gaps_amd import ppp
    rng = np.random.default_rng(3)
    sims = rng.standard_normal((40, 5))
    sims[7, 3] = np.nan                      # an empty bin in one simulation
    observed = np.array([0.1, -5.0, 5.0, 0.0, np.nan])
    observed[0] = sims[4, 0]                 # a tie counts on both sides
    got = ppp._lag_levels(observed, sims, (0.9, 0.975))
    ok = [0, 1, 2]
    assert np.array_equal(got["median"][ok], np.quantile(sims[:, ok], 0.5, axis=0))
    assert np.array_equal(got["upper"][:, ok], np.quantile(sims[:, ok], [0.9, 0.975], axis=0))
    assert np.array_equal(got["lower"][:, ok], np.quantile(sims[:, ok], [1 - 0.9, 1 - 0.975], axis=0))
    assert got["share_above"][1] == 1.0 and got["share_below"][1] == 0.0 and got["share_above"][2] == 0.0 and got["share_below"][2] == 1.0
    assert got["share_above"][0] + got["share_below"][0] == 1.0 + 1.0 / 40
    for k in ("median", "share_above", "share_below"):
        assert np.all(np.isnan(got[k][3:])) and got[k].shape == (5,)
    for k in ("lower", "upper"):
        assert np.all(np.isnan(got[k][:, 3:])) and got[k].shape == (2, 5)
    with pytest.raises(ValueError):
        ppp._lag_levels(observed, sims, (0.4,))
