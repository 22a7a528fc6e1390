"""Epoch folding without a GPU:

* the fixture tests/golden/epoch_fold_golden.npz (scripts/make_epoch_fold_golden.py): its layout and the conditions the
  GPU test leans on (rho, the named near-edge samples, empty and full bins, the kinds of the `edges` case);
* the float64 helper tests/epoch_fold_numpy.py: its bins equal the rational ones on every fixture sample, its powers
  the 50-digit truth within max(10 rho, 64 sqrt(N) u);
* the four normalisations are one truth; nested bins (2 -> 32) never explain less;
* the planner csrc/mtg_ef_plan.h through tests/ef_plan_driver.cpp against a restatement and its LDS budget;
* the header declares both entries, the library exports them and the engine binds them with the header's arity.
"""
import os
import re
import subprocess
import tempfile
from fractions import Fraction

import numpy as np
import pytest

import epoch_fold_numpy as efn
from mind_the_gaps_amd import engine

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CASES = ("n5", "n52", "n216", "n789", "fast216")
NBINS = (2, 10, 32)
EDGE_NBINS = (2, 8, 10, 32)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "epoch_fold_golden.npz"))


@pytest.fixture(scope="module")
def ls_golden():
    return np.load(os.path.join(HERE, "golden", "lomb_scargle_golden.npz"))


def case_inputs(golden, ls_golden, name):
    """t, y, dy, freqs, time_0, nbins of a fixture case"""
    if name.startswith("edges"):
        t, y, dy, freqs = (golden["edges/" + k] for k in ("t", "y", "dy", "freqs"))
        return t, y, dy, freqs, float(golden[name + "/time_0"]), EDGE_NBINS
    t, y, dy = (ls_golden["%s/%s" % (name, k)] for k in ("t", "y", "dy"))
    return t, y, dy, ls_golden[name + "/freqs"][golden[name + "/freq_index"]], float(golden[name + "/time_0"]), NBINS


ALL_CASES = CASES + ("edges", "edges_neg")


@pytest.mark.parametrize("name", ALL_CASES)
def test_fixture_layout_and_conditions(golden, ls_golden, name):
    t, y, dy, freqs, time_0, nbins = case_inputs(golden, ls_golden, name)
    assert np.all(np.diff(t) > 0) and len(y) == len(dy) == len(t)
    if not name.startswith("edges"):
        assert time_0 == t[0]
    te = t - time_0
    named = {tuple(v) for v in golden[name + "/near_edges"]}
    for nb in nbins:
        count = golden["%s/nb%d/count" % (name, nb)]
        assert count.shape == (len(freqs), nb) and count.dtype == np.int64 and np.all(count.sum(axis=1) == len(t))
        for tag in "wu":
            for k in efn.NORMALIZATIONS:
                assert golden["%s/nb%d/%s_%s" % (name, nb, tag, k)].shape == (len(freqs),)
        for k, f in enumerate(freqs):
            exact = efn.exact_bins(f, te, nb)
            # the helper's bins are the rational ones on every fixture sample, and the counts are theirs
            assert np.array_equal(efn.bins(f, te, nb), exact), (name, nb, k)
            assert np.array_equal(np.bincount(exact, minlength=nb), count[k])
            for n, x in enumerate(te):
                ph = efn.exact_phase(f, x)
                d = abs(ph * nb - round(ph * nb))
                if ph != 0 and d < Fraction(1, 2 ** 40):
                    assert (k, n, nb) in named
                elif not name.startswith("edges"):
                    assert ph == 0 or d >= Fraction(1, 10 ** 9)
    for tag in "wu":
        assert 0 <= float(golden["%s/%s_rho" % (name, tag)]) <= 1e-9


def test_fixture_has_empty_bins_and_full_ones(golden):
    assert np.any(golden["n5/nb32/count"] == 0)
    assert any(np.all(golden["%s/nb%d/count" % (name, nb)] > 0) for name in CASES for nb in NBINS)


def test_edges_case_holds_every_kind(golden):
    t, freqs = golden["edges/t"], golden["edges/freqs"]
    assert float(golden["edges/time_0"]) == 0.0
    kinds = {k: golden["edges/kind_" + k] for k in ("a", "b", "c", "e", "b10", "c10")}
    for k, v in kinds.items():
        assert len(v) >= 24, k
    for k, n in kinds["a"]:
        assert (Fraction(freqs[k]) * Fraction(t[n]) * 32).denominator == 1
    assert any((Fraction(freqs[k]) * Fraction(t[n]) * 2).denominator == 1 for k, n in kinds["a"])
    wrong = 0
    for kind in ("b", "c", "e"):
        for k, n in kinds[kind]:
            rounded, exact = Fraction(freqs[k] * t[n]), Fraction(freqs[k]) * Fraction(t[n])
            assert (rounded * 32).denominator == 1 and exact != rounded
            if kind != "e":
                assert (exact < rounded) == (kind == "b")
            if exact < rounded:
                wrong += int(efn.rounded_bins(freqs[k], t[n:n + 1], 32)[0] != efn.exact_bins(freqs[k], t[n:n + 1], 32)[0])
    assert wrong >= 24   # the rounded product picks the wrong bin there
    assert any(freqs[k] * t[n] > 9e5 for k, n in kinds["e"])
    for kind in ("b10", "c10"):
        for k, n in kinds[kind]:
            rounded, exact = Fraction(freqs[k] * t[n]), Fraction(freqs[k]) * Fraction(t[n])
            edge = Fraction(round(exact * 10), 10)
            assert (exact < edge <= rounded) if kind == "b10" else (rounded < edge <= exact)
    # (d) negative elapsed times: the same light curve from an epoch inside its span
    assert np.any(t - float(golden["edges_neg/time_0"]) < 0) and np.any(t - float(golden["edges_neg/time_0"]) > 0)


@pytest.mark.parametrize("name", ALL_CASES)
def test_numpy_helper_matches_the_truth(golden, ls_golden, name):
    t, y, dy, freqs, time_0, nbins = case_inputs(golden, ls_golden, name)
    for tag, weighted in (("w", True), ("u", False)):
        rho = float(golden["%s/%s_rho" % (name, tag)])
        _, _, _, YY, sw = efn.weights(y, dy, weighted)
        for nb in nbins:
            P = golden["%s/nb%d/%s_standard" % (name, nb, tag)]
            for k in efn.NORMALIZATIONS:
                got = efn.power(t, y, dy, freqs, nb, time_0, weighted, k)
                want = golden["%s/nb%d/%s_%s" % (name, nb, tag, k)]
                tol = efn.bound(rho, len(t)) * efn.dnorm_dstandard(P, YY, sw, k)
                assert np.all(np.abs(got - want) <= tol), (name, tag, nb, k, float(np.max(np.abs(got - want) / tol)))


@pytest.mark.parametrize("name", ALL_CASES)
def test_normalisations_are_one_truth_and_nested_bins_explain_more(golden, ls_golden, name):
    t, y, dy, freqs, time_0, nbins = case_inputs(golden, ls_golden, name)
    for tag, weighted in (("w", True), ("u", False)):
        _, _, _, YY, sw = efn.weights(y, dy, weighted)
        for nb in nbins:
            P = golden["%s/nb%d/%s_standard" % (name, nb, tag)]
            assert np.all((P >= 0) & (P <= 1 + 1e-15))
            ok = P < 1 - 1e-9    # (a profile that explains everything: model and log diverge)
            assert np.allclose(golden["%s/nb%d/%s_model" % (name, nb, tag)][ok], (P / (1 - P))[ok], rtol=1e-12, atol=1e-30)
            assert np.allclose(golden["%s/nb%d/%s_log" % (name, nb, tag)][ok], -np.log1p(-P[ok]), rtol=1e-12, atol=1e-30)
            assert np.allclose(golden["%s/nb%d/%s_psd" % (name, nb, tag)], P * YY * 0.5 * sw, rtol=1e-12, atol=1e-30)
        # 2 | 32: every bin of 2 is a union of bins of 32 (2 | 10 too, but 10 does not divide 32)
        assert np.all(golden["%s/nb32/%s_standard" % (name, tag)] >= golden["%s/nb2/%s_standard" % (name, tag)] - 1e-14)


def test_bins_just_below_zero_go_to_the_last_bin():
    te = np.array([-1e-18, -1e-20, -1e-300, -2.0 ** -60, 0.0, 1e-300, 1e-20])
    for nb in (2, 3, 8, 10, 32):
        for f in (1.0, 0.7, 3.0):
            exact = efn.exact_bins(f, te, nb)
            assert np.array_equal(exact[:4], np.full(4, nb - 1)) and np.array_equal(exact[4:], np.zeros(3, dtype=np.int64))
            assert np.array_equal(efn.bins(f, te, nb), exact), (nb, f)


def planned(nbins, F, L, shared, weighted):
    """csrc/mtg_ef_plan.h restated"""
    budget = 80 * 1024

    def acc(tile, lanes):
        return 16 * tile * nbins * lanes if weighted or tile == 1 else (8 + 8 * tile) * nbins * lanes

    def chunk(tile):
        return 2048 + 4096 * (tile if weighted else (tile + 1) // 2)

    lanes = 64 if F <= 64 else 128 if F <= 128 else 256
    tile = 1
    if shared and L > 1:
        for r in (2, 4):
            if acc(r, lanes) + chunk(r) <= budget:
                tile = r
    while lanes > 64 and acc(1, lanes) + chunk(1) > budget:
        lanes //= 2
    return tile, lanes, acc(tile, lanes), acc(tile, lanes) + chunk(tile)


def test_planner_matches_its_restatement_and_its_budget():
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "ef_plan_driver")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "mind_the_gaps_amd", "csrc"),
                               os.path.join(HERE, "ef_plan_driver.cpp"), "-o", exe])
        cases = [(nb, F, L, shared, weighted) for nb in range(2, 33) for F in (1, 64, 65, 128, 129, 5000) for L in (1, 2, 3, 11, 2000)
                 for shared in (0, 1) for weighted in (0, 1)]
        r = subprocess.run([exe], input="".join("%d %d %d %d %d\n" % c for c in cases), capture_output=True, text=True, check=True)
        got = [tuple(int(v) for v in line.split()) for line in r.stdout.splitlines()]
        assert len(got) == len(cases)
        tiles = set()
        for c, g in zip(cases, got):
            assert g == planned(*c), (c, g)
            nb, F, L, shared, weighted = c
            tile, lanes, acc_bytes, lds_bytes = g
            tiles.add(tile)
            assert tile in (1, 2, 4) and lanes in (64, 128, 256) and (shared and L > 1 or tile == 1)
            # [bin][lane] entries of 16 bytes per light curve, or 8 for the tile's W and 8 per light curve: inside the budget
            # it claims, two workgroups inside a CU's 160 KiB
            per_lane = 16 * tile * nb if weighted or tile == 1 else (8 + 8 * tile) * nb
            assert acc_bytes == per_lane * lanes and acc_bytes % (16 * lanes) in (0, 8 * lanes)
            assert acc_bytes < lds_bytes <= 80 * 1024 and 2 * lds_bytes <= 160 * 1024
        assert tiles == {1, 2, 4}


def test_resource_report_lists_every_instantiation_without_scratch():
    rows = [line.split() for line in open(os.path.join(ROOT, "profiles", "epoch_fold_resources.txt")) if line.startswith("mtg_")]
    names = {" ".join(r[:-8]) for r in rows}
    for tile in (1, 2, 4):
        for weighted in ("true", "false"):
            assert "mtg_epoch_fold_kernel<%d, %s>" % (tile, weighted) in names
    assert "mtg_phase_fold_counts_kernel" in names   # (the peaks are reduced by the Lomb-Scargle unit's kernel)
    for r in rows:
        assert r[-5] == "0" and r[-3] == "0" and r[-2] == "0", r   # scratch, SGPR and VGPR spills


def test_entries_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "mtg.h")).read()
    assert int(re.search(r"MTG_EF_MAX_BINS\s*=\s*(\d+)", text).group(1)) == engine.EF_MAX_BINS == 32
    lib = engine.load_library()
    want = {"mtg_epoch_fold": ["ctx", "F", "freqs", "nbins", "time_0", "normalization", "weighted", "power", "peak_power", "peak_index"],
            "mtg_phase_fold": ["ctx", "F", "freqs", "nbins", "time_0", "weighted", "count", "wsum", "wrsum", "varsum"]}
    for name, params in want.items():
        decl = re.search(r"MTG_API\s+int\s+%s\s*\(([^;]*)\)\s*;" % name, text)
        got = [p.split()[-1].lstrip("*") for p in re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).split(",")]
        assert got == params
        assert name in engine.EXPORTS
        assert len(getattr(lib, name).argtypes) == len(params)
    for method in ("epoch_fold", "phase_fold"):
        assert {"nbins", "time_0", "weighted"} <= set(getattr(engine.Engine, method).__code__.co_varnames)
    # no context: an argument error, nothing touched
    assert lib.mtg_epoch_fold(None, 1, None, 10, 0.0, 0, 1, None, None, None) == engine.E_ARG
    assert lib.mtg_phase_fold(None, 1, None, 10, 0.0, 1, None, None, None, None) == engine.E_ARG
