"""The two-series lag-bin sums (mtg_cross_sums) without a GPU:

* the fixture tests/golden/cross_golden.npz (scripts/make_cross_golden.py): its layout, companions and edge sets, the exact
  counts against the float64 helper tests/cross_numpy.py, the pairs that sit on an edge, what each edge set is there for;
* the helper's sums against the exact truth, within the bounds the GPU test uses;
* the planner csrc/mtg_cross_plan.h through tests/cross_plan_driver.cpp against a restatement and its budget;
* the compiler's resource report: every instantiation, no scratch;
* the entry declared, exported and bound with the header's arity;
* ccf_from_sums (both normalisations) and lag_peak_and_centroid on hand-made sums;
* the argument checks of timedomain and ppp that need no device;
* the bookkeeping of ppp.cross_lag_significance with the stand-ins of tests/ppp_fakes.py and a numpy engine.
"""
import os
import re
import subprocess
import tempfile
import types

import numpy as np
import pytest

import cross_numpy as cn
from mind_the_gaps_amd import engine, timedomain

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "cross_golden.npz"))


@pytest.fixture(scope="module")
def ls_golden():
    return np.load(os.path.join(HERE, "golden", "lomb_scargle_golden.npz"))


@pytest.mark.parametrize("name", cn.CASES)
def test_fixture_layout_counts_and_ties(golden, ls_golden, name):
    assert tuple(str(c) for c in golden["cases"]) == cn.CASES and tuple(str(c) for c in golden["edge_sets"]) == cn.EDGE_SETS
    t, y = (ls_golden["%s/%s" % (name, k)] for k in ("t", "y"))
    t2, y2 = golden[name + "/t2"], golden[name + "/y2"]
    n, m = len(t), len(t2)
    assert n == int(name[1:]) and m == cn.COMPANION_M[name] and m != n and m % 256 != 0 and len(y2) == m
    made = cn.companion(name, t, y)
    assert np.array_equal(made[0], t2) and np.allclose(made[1], y2, rtol=1e-13, atol=0)
    assert np.all(np.diff(t2) >= 0) and np.all(np.isfinite(y2))
    # the spans overlap only partly; lags of both signs and tau == 0 occur
    assert t[0] < t2[0] < t[-1] < t2[-1]
    i, j, tau = cn.pairs(t, t2)
    assert len(tau) == n * m and np.sum(tau == 0) >= 1 and np.sum(tau < 0) > 0 and np.sum(tau > 0) > 0
    assert np.array_equal(i, np.repeat(np.arange(n), m)) and np.array_equal(j, np.tile(np.arange(m), n))
    sets = cn.edge_sets(t, t2)
    nbins = dict(sym8=8, one=1, negative6=6, short5=5, wide128=128)
    for tag in cn.EDGE_SETS:
        key = "%s/%s/" % (name, tag)
        edges = golden[key + "edges"]
        assert np.array_equal(edges, sets[tag]) and np.all(np.diff(edges) > 0)
        nb = len(edges) - 1
        assert nb == nbins.get(tag, nb) and 1 <= nb <= engine.LAG_MAX_BINS
        got = cn.cross_sums(t, y, t2, y2, edges)
        assert golden[key + "count"].dtype == np.int64 and np.array_equal(golden[key + "count"], got["count"])
        for q in cn.VALUES + ("lagabs", "cfabs", "saabs", "sbabs"):
            assert golden[key + q].shape == (nb,) and golden[key + q + "_lo"].shape == (nb,)
            assert np.all(np.abs(golden[key + q + "_lo"]) <= 2.0 ** -53 * np.abs(golden[key + q]))
            assert np.all(golden[key + q][golden[key + "count"] == 0] == 0)
        for q in cn.VALUES:
            assert 0 <= float(golden[key + "rho_" + q]) <= 1e-12
            assert np.all(np.abs(golden[key + q]) <= golden[key + cn.SCALE[q]])
    # what each edge set is there for
    sym = golden[name + "/sym8/edges"]
    assert np.array_equal(sym, -sym[::-1]) and sym[-1] == 0.5 * min(t[-1] - t[0], t2[-1] - t2[0])
    assert golden[name + "/negative6/edges"][-1] < 0 and golden[name + "/negative6/count"].sum() > 0
    short = golden[name + "/short5/edges"]
    assert short[0] > 0 and np.sum(tau < short[0]) > 0 and np.sum(tau >= short[-1]) > 0
    wide = golden[name + "/wide128/count"]
    assert wide.sum() == n * m and np.all(wide[:21] == 0) and np.all(wide[-21:] == 0)
    # ties: every edge is a pair's lag, 0 among them; the pair is counted in the bin above the edge (none for the last edge)
    edges, ties = golden[name + "/ties/edges"], golden[name + "/ties/tie_pairs"]
    assert len(ties) >= len(edges) and 0.0 in edges
    for a, b, where in ties:
        k = int(np.flatnonzero(edges == t2[b] - t[a])[0])
        assert where == (k if k < len(edges) - 1 else -1)
    assert set(np.flatnonzero(np.isin(edges, t2[ties[:, 1]] - t[ties[:, 0]]))) == set(range(len(edges)))
    for k in range(len(edges) - 1):
        assert golden[name + "/ties/count"][k] >= np.sum(ties[:, 2] == k) >= 1


def test_some_workgroups_start_late_and_some_exit_early(golden, ls_golden):
    # n789 x 523: four row blocks (the last partly filled) and three chunks
    t, t2 = ls_golden["n789/t"], golden["n789/t2"]
    late, early, total = cn.skipped_chunks(t, t2, golden["n789/short5/edges"])
    assert total == 12 and late >= 1 and early >= 1 and late + early < total
    assert cn.skipped_chunks(t, t2, golden["n789/wide128/edges"]) == (0, 0, 12)
    assert cn.skipped_chunks(t, t2, golden["n789/negative6/edges"])[1] >= 1
    # a skipped chunk holds no pair in a bin for any row of its block: the rule is safe
    for tag in cn.EDGE_SETS:
        edges = golden["n789/%s/edges" % tag]
        for row0 in range(0, 789, 256):
            rows = t[row0:row0 + 256]
            k = 0
            starts = list(range(0, 523, 256))
            while k < 3 and not t2[min(starts[k] + 256, 523) - 1] - rows[0] >= edges[0]:
                tau = t2[None, starts[k]:starts[k] + 256] - rows[:, None]
                assert np.all(tau < edges[0])
                k += 1
            while k < 3 and not t2[starts[k]] - rows[-1] >= edges[-1]:
                k += 1
            if k < 3:
                assert np.all(t2[None, starts[k]:] - rows[:, None] >= edges[-1])


@pytest.mark.parametrize("name", cn.CASES)
def test_numpy_helper_matches_the_truth(golden, ls_golden, name):
    t, y = (ls_golden["%s/%s" % (name, k)] for k in ("t", "y"))
    t2, y2 = golden[name + "/t2"], golden[name + "/y2"]
    for tag in cn.EDGE_SETS:
        key = "%s/%s/" % (name, tag)
        got = cn.cross_sums(t, y, t2, y2, golden[key + "edges"])
        count = golden[key + "count"]
        for q in cn.VALUES:
            scale = np.abs(golden[key + cn.SCALE[q]])
            err = np.abs((got[q] - golden[key + q]) - golden[key + q + "_lo"])
            assert np.all(err <= cn.bound(float(golden[key + "rho_" + q]), count, scale)), (tag, q)
            assert np.all(got[q][count == 0] == 0)


def planned(N, M, nbins, L, shared, per, what, rows, limit=0):
    """csrc/mtg_cross_plan.h restated"""
    limit = limit or 1 << 30
    tile = 1 if not shared or L == 1 else 4 if L <= 4 else 8
    full = 1 if what & ~15 else 0
    per_lc, per_tile = (4 if full else 2), 2
    bytes_of = lambda r: (per_lc * r + per_tile * -(-r // tile)) * nbins * N * 8
    slab = min(max(limit // bytes_of(tile) * tile, tile), L)
    lds = 2048 + 8 * 130 + 8 * (tile if per else 1) * 256
    row_blocks, chunks = -(-N // 256), -(-M // 256)
    blocks = row_blocks * -(-rows // tile)
    return tile, int(bool(per)), full, per_lc, per_tile, row_blocks, chunks, slab, bytes_of(slab), lds, blocks if blocks <= 0x7fffffff else 0


def test_planner_matches_its_restatement_and_its_budget():
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "cross_plan_driver")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "mind_the_gaps_amd", "csrc"),
                               os.path.join(HERE, "cross_plan_driver.cpp"), "-o", exe])
        ask = lambda cases: [tuple(int(v) for v in line.split()) for line in subprocess.run(
            [exe], input="".join("%d %d %d %d %d %d %d %d %d\n" % c for c in cases), capture_output=True, text=True, check=True).stdout.splitlines()]
        cases = [(N, M, nbins, L, shared, per, what, rows, limit) for N in (1, 5, 256, 257, 789, 10000, 1 << 26) for M in (1, 300, (1 << 28) - 1)
                 for nbins in (1, 50, 128) for L in (1, 2, 4, 5, 11, 313, 2000) for shared in (0, 1) for per in (0, 1)
                 for what in (1, 15, 16, 32, 255) for rows in (1, L) for limit in (0, 1 << 24)]
        got = ask(cases)
        assert len(got) == len(cases)
        seen = set()
        for c, g in zip(cases, got):
            assert g == planned(*c), (c, g)
            N, M, nbins, L, shared, per, what, rows, limit = c
            tile, per_, full, per_lc, per_tile, row_blocks, chunks, slab, ws, lds, blocks = g
            seen.add((tile, per_, full))
            assert (shared and L > 1 or tile == 1) and full == (what > 15) and per_ == per
            assert 1 <= slab <= L and (slab % tile == 0 or slab == L)
            # the workspace stays within its limit unless one tile's alone is more
            assert ws <= max(limit or 1 << 30, (per_lc * tile + per_tile) * nbins * N * 8)
            assert 2 * lds <= 160 * 1024 and lds <= 64 * 1024      # two workgroups on a CU; static LDS
            assert row_blocks * 256 >= N > (row_blocks - 1) * 256 and chunks * 256 >= M > (chunks - 1) * 256
        assert seen == {(r, p, a) for r in (1, 4, 8) for p in (0, 1) for a in (0, 1)}
        # the set of tests/test_cross_gpu.py's two slabs: 789 rows, 128 bins, every sum -- 312 light curves on shared sampling
        # and 221 stored per light curve fit 1 GiB, so L = 313 is the smallest set cut in two on shared sampling
        assert [g[7] for g in ask([(789, 523, 128, L, 1, 1, 255, L, 0) for L in (312, 313)])] == [312, 312]
        assert ask([(789, 523, 128, 313, 0, 1, 255, 313, 0)])[0][7] == 221
        assert ask([(789, 523, 128, 313, 1, 1, 15, 313, 0)])[0][7] == 313          # (the light variant: one slab)
        # the headline set at 50 bins: the light variant in slabs of 112 light curves, everything in slabs of 56
        head = ask([(10000, 10000, 50, 2000, 1, 0, 15, 2000, 0), (10000, 10000, 50, 2000, 1, 1, 255, 2000, 0)])
        assert head[0] == (8, 0, 0, 2, 2, 40, 40, 112, (2 * 112 + 2 * 14) * 4000000, 5136, 40 * 250)
        assert head[1] == (8, 1, 1, 4, 2, 40, 40, 56, (4 * 56 + 2 * 7) * 4000000, 19472, 40 * 250)


def test_resource_report_lists_every_instantiation_without_scratch():
    rows = [line.split() for line in open(os.path.join(ROOT, "profiles", "cross_resources.txt")) if line.startswith("mtg_")]
    names = {" ".join(r[:-8]): r for r in rows}
    word = {True: "true", False: "false"}
    for tile in (1, 4, 8):
        for per in (True, False):
            for full in (True, False):
                r = names["mtg_cross_kernel<%d, %s, %s>" % (tile, word[per], word[full])]
                assert int(r[-7]) <= 256 and int(r[-4]) >= 2                      # VGPRs, waves per SIMD
                assert int(r[-1]) == planned(300, 300, 1, 8, 1, per, 255 if full else 15, 1)[9] + (8 * (tile - 8) * 256 if per else 0)   # LDS as planned
        assert "mtg_cross_reduce_kernel<%d>" % tile in names
    assert len(rows) == 15
    for r in rows:
        assert r[-5] == "0" and r[-3] == "0" and r[-2] == "0", r   # scratch, SGPR and VGPR spills


def test_entry_is_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "mtg.h")).read()
    plan = open(os.path.join(ROOT, "mind_the_gaps_amd", "csrc", "mtg_cross_plan.h")).read()
    assert "MTG_CROSS_MAX_M ((int64_t)1 << 28)" in plan and engine.CROSS_MAX_M == 1 << 28
    lib = engine.load_library()
    params = ["ctx", "M", "t2", "L2", "y2", "nbins", "edges", "count", "lag", "cf", "cf2", "sa", "sb", "saa", "sbb"]
    decl = re.search(r"MTG_API\s+int\s+mtg_cross_sums\s*\(([^;]*)\)\s*;", text)
    got = [p.split()[-1].lstrip("*") for p in re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).split(",")]
    assert got == params and "mtg_cross_sums" in engine.EXPORTS and len(lib.mtg_cross_sums.argtypes) == len(params)
    assert tuple(params[7:]) == engine.CROSS_SUMS == cn.SUMS
    assert set(engine.CROSS_SUMS) <= set(engine.Engine.cross_sums.__code__.co_varnames)
    # the planner's bits follow the outputs' order
    bits = dict(re.findall(r"MTG_CROSS_(COUNT|LAG|CF|CF2|SA|SB|SAA|SBB) = (\d+)", plan))
    assert [int(bits[k.upper()]) for k in engine.CROSS_SUMS] == [1 << k for k in range(8)]
    # the reduction is shared with the lag sweep
    for unit in ("mtg_lag.hip", "mtg_cross.hip"):
        src = open(os.path.join(ROOT, "mind_the_gaps_amd", "csrc", unit)).read()
        assert '#include "mtg_row_reduce.h"' in src and "lag_block_sum(V v" not in src
    # no context: an argument error, nothing touched
    assert lib.mtg_cross_sums(None, 1, None, 1, None, 1, None, *([None] * 8)) == engine.E_ARG


def test_normalisations_on_hand_made_sums():
    # bins: empty; one pair; four pairs (r, s) = (1, 2), (1, 4), (3, 2), (3, 4): no local correlation;
    # four pairs (1, 2), (1, 2), (3, 6), (3, 6): local correlation 1; two pairs with equal s: no local variance
    pairs = [[], [(2.0, 3.0)], [(1, 2), (1, 4), (3, 2), (3, 4)], [(1, 2), (1, 2), (3, 6), (3, 6)], [(1.0, 5.0), (2.0, 5.0)]]
    tot = lambda f: np.array([[sum(f(r, s) for r, s in bin_) for bin_ in pairs]], dtype=np.float64)
    sums = dict(count=np.array([[len(b) for b in pairs]]), lag=np.array([[0.0, -2.0, 8.0, -4.0, 1.0]]), cf=tot(lambda r, s: r * s),
                cf2=tot(lambda r, s: (r * s) ** 2), sa=tot(lambda r, s: r), sb=tot(lambda r, s: s), saa=tot(lambda r, s: r * r),
                sbb=tot(lambda r, s: s * s))
    lag, ccf, err, count = timedomain.ccf_from_sums(sums, np.array([4.25]), 1.25, np.array([0.25]), 0.25)      # sqrt(4 x 1) = 2
    assert np.isnan(lag[0, 0]) and np.array_equal(lag[0, 1:], [-2.0, 2.0, -1.0, 0.5]) and np.array_equal(count, sums["count"])
    assert np.isnan(ccf[0, 0]) and np.isnan(ccf[0, 1]) and np.array_equal(ccf[0, 2:], [24 / 4 / 2, 40 / 4 / 2, 15 / 2 / 2])
    assert np.isnan(err[0, 0]) and np.isnan(err[0, 1]) and err[0, 2] == np.sqrt(200.0 - 24.0 ** 2 / 4) / (3 * 2)
    # without the noise terms, scalars for both variances
    assert np.array_equal(timedomain.ccf_from_sums(sums, 4.0, 4.0)[1][0, 2:], [24 / 4 / 4, 40 / 4 / 4, 15 / 2 / 4])
    # a variance that is not positive: NaN
    assert np.all(np.isnan(timedomain.ccf_from_sums(sums, 0.25, 1.25, 0.25, 0.25)[1]))
    assert np.all(np.isnan(timedomain.ccf_from_sums(sums, -1.0, -1.0)[1]))
    l_lag, l_ccf, l_err, l_count = timedomain.ccf_from_sums(sums, None, None, normalization="local")
    assert np.array_equal(l_lag, lag, equal_nan=True) and np.array_equal(l_count, count)
    assert np.isnan(l_ccf[0, 0]) and np.isnan(l_ccf[0, 1]) and l_ccf[0, 2] == 0.0 and l_ccf[0, 3] == 1.0 and np.isnan(l_ccf[0, 4])
    assert l_err[0, 2] == np.sqrt(200.0 - 24.0 ** 2 / 4) / (3 * np.sqrt(1.0 * 1.0)) and np.isnan(l_err[0, 4])
    with pytest.raises(ValueError):
        timedomain.ccf_from_sums(sums, 1.0, 1.0, normalization="welsh")


def test_lag_peak_and_centroid_on_hand_made_curves():
    lag = np.array([-2.0, -1.0, 0.0, 1.0, 2.0])
    ccf = np.array([0.1, 0.5, 1.0, 0.9, np.nan])
    peak, centroid = timedomain.lag_peak_and_centroid(lag, ccf)
    assert peak == 0.0 and centroid == (0.0 * 1.0 + 1.0 * 0.9) / 1.9
    assert timedomain.lag_peak_and_centroid(lag, ccf, threshold=0.5)[1] == (-1.0 * 0.5 + 1.0 * 0.9) / 2.4
    assert timedomain.lag_peak_and_centroid(lag, ccf, threshold=1.0) == (0.0, 0.0)
    rows = np.stack([ccf, np.full(5, np.nan), [0.25, 0.25, -1.0, 0.125, 0.25], [-3.0, -1.0, -2.0, np.nan, -5.0]])
    peak, centroid = timedomain.lag_peak_and_centroid(np.tile(lag, (4, 1)), rows)
    assert peak[0] == 0.0 and np.isnan(peak[1]) and np.isnan(centroid[1])
    assert peak[2] == -2.0 and centroid[2] == (-2.0 - 1.0 + 2.0) * 0.25 / 0.75     # the first of equal maxima; all at the peak
    assert peak[3] == -1.0 and np.isnan(centroid[3])                                   # a peak below zero has no centroid
    for bad in (dict(threshold=0.0), dict(threshold=1.5)):
        with pytest.raises(ValueError):
            timedomain.lag_peak_and_centroid(lag, ccf, **bad)
    with pytest.raises(ValueError):
        timedomain.lag_peak_and_centroid(lag[:4], ccf)


def test_argument_checks_that_need_no_device():
    t1, t2 = np.array([0.0, 1.0, 1.5, 4.0, 9.0]), np.array([2.0, 3.0, 8.0])
    e = timedomain.cross_lag_bins(t1, t2, 6)
    assert len(e) == 7 and e[0] == -3.0 and e[-1] == 3.0 and np.allclose(np.diff(e), 1.0)       # half the shorter span
    assert np.array_equal(timedomain.cross_lag_bins(t1, t2, 2, max_lag=5.0), [-5.0, 0.0, 5.0])
    for kwargs in (dict(nbins=0), dict(nbins=129), dict(nbins=4, max_lag=0.0), dict(nbins=4, max_lag=-1.0), dict(nbins=4, max_lag=np.inf)):
        with pytest.raises(ValueError):
            timedomain.cross_lag_bins(t1, t2, **kwargs)
    with pytest.raises(ValueError):
        timedomain.cross_lag_bins(t1, t2[:1], 4)          # no span, no default
    with pytest.raises(ValueError):
        timedomain.cross_lag_bins(t1, t2[:0], 4, max_lag=1.0)
    y1, y2 = np.sin(t1), np.cos(t2)
    for args in ((t1, y1[:3], t2, y2), (t1, y1, t2, y2[:2]), (t1[::-1], y1, t2, y2), (t1, y1, t2[::-1], y2), (t1, y1, t2, np.stack([y2, y2])),
                 (t1, np.stack([y1, y1]), t2, np.stack([y2, y2, y2])), (t1[:0], y1[:0], t2, y2)):
        with pytest.raises(ValueError):
            timedomain.CrossCorrelation(*args)
    one = timedomain.CrossCorrelation(t1, y1, t2, y2)
    assert one.dy1 is None and one.dy2 is None
    both = timedomain.CrossCorrelation(t1, np.stack([y1, y1]), t2, np.stack([y2, y2]), 0.1, np.full(3, 0.2))
    assert both.dy1.shape == (2, 5) and both.dy2.shape == (2, 3)
    with pytest.raises(ValueError, match="normalization"):
        one.ccf(e, normalization="none")

    from mind_the_gaps_amd import ppp
    with pytest.raises(ValueError, match="normalization"):
        ppp.cross_lag_significance(None, None, None, e, normalization="none")
    import inspect
    sig, ref = inspect.signature(ppp.cross_lag_significance).parameters, inspect.signature(ppp.lag_significance).parameters
    assert sig["normalization"].default == "global" and list(sig)[:4] == ["lightcurve", "companion", "null_kernel", "edges"]
    for k in ("nsims", "levels", "walkers", "max_steps", "sigma_noise", "extension_factor", "subtract_noise", "seed", "device", "progress", "pdf",
              "max_iter"):
        assert sig[k].default == ref[k].default, k
    assert set(ref) - {"statistic"} <= set(sig)


class NumpyEngine:
    """Engine.set_lightcurves and Engine.cross_sums by tests/cross_numpy.py, with a log of the calls"""

    def __init__(self):
        self.calls = []

    def set_lightcurves(self, t, y, dy):
        self.t, self.Y = np.asarray(t), np.atleast_2d(y)
        self.L = len(self.Y)
        self.calls.append(("set_lightcurves", self.Y.shape))

    def cross_sums(self, t2, y2, edges, **want):
        assert np.ndim(y2) == 1                       # one companion for the whole set: L2 = 1
        self.calls.append(("cross_sums", self.Y.shape, tuple(sorted(k for k, v in want.items() if v))))
        per = [cn.cross_sums(self.t, row, t2, y2, edges) for row in self.Y]
        return {k: np.stack([p[k] for p in per]) for k in cn.SUMS if want.get(k)}


@pytest.mark.parametrize("normalization", ["global", "local"])
def test_cross_lag_significance_bookkeeping_on_the_host(normalization):
    import ppp_fakes
    from mind_the_gaps_amd import gp, ppp, simulator
    nsims = 9
    lc = ppp_fakes.lightcurve()
    rng = np.random.default_rng(8)
    lc.y, lc.dy = 50.0 + rng.standard_normal(ppp_fakes.N_TIMES), np.full(ppp_fakes.N_TIMES, 0.3)
    comp = types.SimpleNamespace(times=np.sort(rng.uniform(2.0, 14.0, 9)), y=rng.standard_normal(9), dy=None)
    edges = np.array([-6.0, -2.0, 2.0, 6.0, 40.0, 50.0])       # the last bin holds no pair
    eng = NumpyEngine()
    seen = {}

    class Simulator(ppp_fakes.Simulator):
        def simulate(self, samples, make_resident=False, seed=None):
            seen.update(make_resident=make_resident, seed=seed, samples=np.array(samples))
            g = np.random.default_rng(seed)
            rates = 50.0 + g.standard_normal((len(samples), ppp_fakes.N_TIMES))
            rates[2] = lc.y                                       # one simulation IS the observation: a tie in every bin and in the peak
            out = dict(rates=rates, dy=np.full_like(rates, 0.3))
            eng.set_lightcurves(lc.times, out["rates"], out["dy"])
            return out

    def run(seed):
        del eng.calls[:]
        real = gp.get_engine
        with ppp_fakes.installed():
            simulator.Simulator, gp.get_engine = Simulator, lambda device: eng
            try:
                return ppp.cross_lag_significance(lc, comp, ppp_fakes.Kernel(ppp_fakes.NULL_SIZE), edges, nsims=nsims, levels=(0.9,),
                                                  normalization=normalization, walkers=8, max_steps=10, seed=seed)
            finally:
                gp.get_engine = real
    res = run(5)
    assert seen["make_resident"] is True and seen["samples"].shape == (nsims, ppp_fakes.NULL_SIZE) and res["sim_seed"] == seen["seed"]
    # the observation alone, then ONE call on the simulated set; the local moments only where they are needed
    outputs = tuple(sorted(cn.SUMS if normalization == "local" else ("count", "lag", "cf", "cf2")))
    assert eng.calls == [("set_lightcurves", (1, 12)), ("cross_sums", (1, 12), outputs), ("set_lightcurves", (nsims, 12)),
                         ("cross_sums", (nsims, 12), outputs)]
    assert np.array_equal(res["lightcurves"]["rates"][2], lc.y) and res["samples"].shape == (nsims, ppp_fakes.NULL_SIZE)
    # the statistic restated
    sums = cn.cross_sums(lc.times, lc.y, comp.times, comp.y, edges)
    want = timedomain.ccf_from_sums({k: v[None, :] for k, v in sums.items()}, np.var(lc.y), np.var(comp.y), 0.3 ** 2, 0.0, normalization)
    assert np.allclose(res["observed"], want[1][0], rtol=1e-12, equal_nan=True) and np.array_equal(res["count"], sums["count"])
    assert np.isnan(res["observed"][-1]) and np.all(np.isfinite(res["observed"][:3])) and res["sims"].shape == (nsims, 5)
    assert np.array_equal(res["sims"][2], res["observed"], equal_nan=True)
    # the peak over the finite bins and the global p-value: ties count as at or above
    ok = np.isfinite(res["observed"])
    assert res["peak"] == np.max(np.abs(res["observed"][ok])) and res["peak_lag"] == res["lag"][ok][np.argmax(np.abs(res["observed"][ok]))]
    assert res["sim_peaks"].shape == res["sim_peak_lags"].shape == (nsims,) and res["sim_peaks"][2] == res["peak"]
    assert np.array_equal(res["sim_peaks"], np.nanmax(np.abs(res["sims"]), axis=1))
    above = int(np.sum(res["sim_peaks"] >= res["peak"]))
    assert 1 <= above <= nsims and res["p_global"] == (1.0 + above) / (1.0 + nsims) and 2.0 / (1 + nsims) <= res["p_global"] <= 1.0
    assert ppp._cross_global_p(0.5, [0.1, 0.5, 0.9, np.nan]) == 3.0 / 5.0 and np.isnan(ppp._cross_global_p(np.nan, [0.1]))
    assert ppp._cross_global_p(2.0, np.zeros(99)) == 0.01
    peaks, lags = ppp._cross_peaks(np.array([[1.0, 2.0, 3.0], [1.0, 2.0, 3.0]]), np.array([[0.2, -0.7, np.nan], [np.nan] * 3]))
    assert peaks[0] == 0.7 and lags[0] == 2.0 and np.isnan(peaks[1]) and np.isnan(lags[1])
    # per bin: _lag_levels of the same rows
    levels = ppp._lag_levels(res["observed"], res["sims"], (0.9,))
    assert all(np.array_equal(res[k], levels[k], equal_nan=True) for k in levels)
    assert np.all(res["share_above"][ok] + res["share_below"][ok] >= 1.0 + 1.0 / nsims - 1e-15)
    # the same seed: the same bits; another seed: other simulations
    again, other = run(5), run(6)
    for k in ("observed", "sims", "sim_peaks", "sim_peak_lags", "median", "upper", "lower", "samples"):
        assert np.array_equal(res[k], again[k], equal_nan=True), k
    assert res["p_global"] == again["p_global"] and res["sim_seed"] == again["sim_seed"] != other["sim_seed"]
    assert not np.array_equal(res["sims"], other["sims"], equal_nan=True) and np.array_equal(res["observed"], other["observed"], equal_nan=True)
