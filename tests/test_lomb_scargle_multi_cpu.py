"""CPU side of the multi-harmonic Lomb-Scargle periodogram (mtg_lomb_scargle_multi; tests/test_lomb_scargle_multi_gpu.py
is the GPU side).

* astropy's chi2 form in numpy float64 (tests/lomb_scargle_multi_numpy.py) against the 50-digit truths of
  tests/golden/lomb_scargle_multi_golden.npz (scripts/make_lomb_scargle_multi_golden.py), and the fixture holds what the
  GPU test relies on; its K = 1 is the tau-free formula of tests/lomb_scargle_numpy.py;
* the tile planner (csrc/mtg_ls_plan.h through tests/ls_multi_plan_driver.cpp) against a restatement, one term included;
* periodogram.LombScargle takes nterms = 1, 3, 4, 5 and still refuses what the device does not do;
* the header declares both new entries, the library exports them and the engine binds them with the header's arity.
"""
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import lomb_scargle_multi_numpy
import lomb_scargle_numpy
from mind_the_gaps_amd import engine
from mind_the_gaps_amd.periodogram import LombScargle

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = np.load(os.path.join(HERE, "golden", "lomb_scargle_golden.npz"))
FIX = np.load(os.path.join(HERE, "golden", "lomb_scargle_multi_golden.npz"))
CASES = ("n52", "n216", "n789", "fast216")
NTERMS = (2, 3, 5)
U = 2.0 ** -53


def test_fixture_layout_and_conditions():
    assert tuple(str(c) for c in FIX["cases"]) == CASES and tuple(int(k) for k in FIX["nterms"]) == NTERMS
    worst = {}
    for c in CASES:
        n, F = len(SRC[c + "/t"]), len(SRC[c + "/freqs"])
        for tag in "wu":
            inv = SRC[c + "/dy"] ** -2.0 if tag == "w" else np.ones(n)
            assert np.isclose(FIX["%s/%s_psd_factor" % (c, tag)], 0.5 * inv.sum(), rtol=1e-13)
            slope = FIX["%s/%s_psd_factor" % (c, tag)] * FIX["%s/%s_YY" % (c, tag)]      # d psd / d standard
            previous = SRC["%s/%s_standard" % (c, tag)]
            for K in NTERMS:
                std = FIX["%s/%s_k%d_standard" % (c, tag, K)]
                kappa = FIX["%s/%s_k%d_kappa" % (c, tag, K)]
                assert std.shape == kappa.shape == (F,) and np.all((std > 0) & (std < 1))
                assert np.all(kappa >= 1) and kappa.max() <= 1e6 and FIX["%s/%s_k%d_rho" % (c, tag, K)] <= 1e-9
                worst[c] = max(worst.get(c, 0.0), float(kappa.max()))
                # more harmonics never explain less
                assert np.all(std >= previous - 1e-12)
                previous = std
                # the four normalisations are one truth
                assert np.allclose(FIX["%s/%s_k%d_model" % (c, tag, K)], std / (1 - std), rtol=1e-12)
                assert np.allclose(FIX["%s/%s_k%d_log" % (c, tag, K)], -np.log1p(-std), rtol=1e-12)
                assert np.allclose(FIX["%s/%s_k%d_psd" % (c, tag, K)], std * slope, rtol=1e-12)
    print("\nlargest kappa per case: %s" % worst)
    assert max(worst.values()) <= 1e4


@pytest.mark.parametrize("case", CASES)
def test_numpy_chi2_form_against_the_50_digit_truth(case):
    """Entry by entry within max(2 rho, 64 sqrt(N) u kappa): rho is this very evaluation's error where the fixture was
    made (another LAPACK may round differently, hence the 2), the second term the project's bound for a solve of
    condition kappa."""
    t, y, dy, f = (SRC["%s/%s" % (case, k)] for k in ("t", "y", "dy", "freqs"))
    for tag, err in (("w", dy), ("u", None)):
        for K in NTERMS:
            got = lomb_scargle_multi_numpy.power(t, y, err, f, K)
            e = np.abs(got - FIX["%s/%s_k%d_standard" % (case, tag, K)])
            rho = float(FIX["%s/%s_k%d_rho" % (case, tag, K)])
            print("\nnumpy %s %s K = %d: max error %.3g, stored rho %.3g" % (case, tag, K, e.max(), rho))
            assert np.all(e <= np.maximum(2.0 * rho, 64.0 * np.sqrt(len(t)) * U * FIX["%s/%s_k%d_kappa" % (case, tag, K)]))
    for norm in ("model", "log", "psd"):
        ref = FIX["%s/w_k3_%s" % (case, norm)]
        assert np.allclose(lomb_scargle_multi_numpy.power(t, y, dy, f, 3, norm), ref, rtol=0, atol=1e-8 * np.max(np.abs(ref)))


def test_numpy_kappa_is_the_fixtures():
    t, y, dy, f = (SRC["n52/%s" % k] for k in ("t", "y", "dy", "freqs"))
    for tag, err in (("w", dy), ("u", None)):
        _, kappa = lomb_scargle_multi_numpy.power(t, y, err, f, 5, return_kappa=True)
        assert np.allclose(kappa, FIX["n52/%s_k5_kappa" % tag], rtol=1e-9)


@pytest.mark.parametrize("case", ["n216", "fast216"])
def test_one_term_is_the_tau_free_formula(case):
    t, y, dy, f = (SRC["%s/%s" % (case, k)] for k in ("t", "y", "dy", "freqs"))
    for tag, err in (("w", dy), ("u", None)):
        for norm in lomb_scargle_numpy.NORMALIZATIONS:
            one = lomb_scargle_multi_numpy.power(t, y, err, f, 1, norm)
            ref = lomb_scargle_numpy.power(t, y, err, f, norm)
            assert np.allclose(one, ref, rtol=0, atol=20.0 * float(SRC["%s/%s_rho" % (case, tag)]) * max(1.0, np.max(np.abs(ref))))


def planned_tile(nterms, L, shared, weighted):
    """mtg_ls_plan.h restated: the largest tile whose running and chunk sums stay within 96 doubles per lane
    (2 x 6 K R weighted; 2 x (2 K R + 4 K) unweighted, R even: the chunk holds pairs), 1 without shared sampling.  One
    term has the rule of its own kernel: 4 up to four light curves, else 8 weighted and 16 unweighted."""
    if not shared or L <= 1:
        return 1
    if nterms == 1:
        return 4 if L <= 4 else 8 if weighted else 16
    if weighted:
        return max(r for r in range(1, 17) if 2 * 6 * nterms * r <= 96 or r == 1)
    return max(r for r in range(2, 17, 2) if 2 * (2 * nterms * r + 4 * nterms) <= 96)


def test_planner_against_its_restatement():
    with tempfile.TemporaryDirectory(prefix="lsm_plan_") as tmp:
        exe = os.path.join(tmp, "ls_multi_plan_driver")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "mind_the_gaps_amd", "csrc"),
                               os.path.join(HERE, "ls_multi_plan_driver.cpp"), "-o", exe])
        cases = [(K, L, shared, weighted) for K in (1, 2, 3, 4, 5) for L in (1, 2, 3, 4, 5, 8, 9, 11, 37, 2000, 10 ** 6)
                 for shared in (0, 1) for weighted in (0, 1)]
        r = subprocess.run([exe], input="".join("%d %d %d %d\n" % c for c in cases), capture_output=True, text=True, check=True)
        got = [int(v) for v in r.stdout.split()]
        assert len(got) == len(cases)
        for c, g in zip(cases, got):
            assert g == planned_tile(*c), (c, g)
        # the budget of the issue: K = 5 weighted does not carry the one-term kernel's R = 8
        full = {(K, w): planned_tile(K, 100, 1, w) for K in (2, 3, 4, 5) for w in (0, 1)}
        assert full == {(2, 1): 4, (3, 1): 2, (4, 1): 2, (5, 1): 1, (2, 0): 10, (3, 0): 6, (4, 0): 4, (5, 0): 2}
        # one term, pinned for every L above: 1 alone or on a sampling of its own, 4 up to four light curves, then 8 / 16
        for L in (1, 2, 3, 4, 5, 8, 9, 11, 37, 2000, 10 ** 6):
            for weighted in (0, 1):
                assert got[cases.index((1, L, 0, weighted))] == 1
                assert got[cases.index((1, L, 1, weighted))] == (1 if L <= 1 else 4 if L <= 4 else 8 if weighted else 16)
        # outside 1 .. 5 there is no tile to launch
        r = subprocess.run([exe], input="0 10 1 1\n6 10 1 0\n", capture_output=True, text=True, check=True)
        assert r.stdout.split() == ["0", "0"]


def planned_slab(F, tile, L):
    """mtg_ls_slab restated: at most 2^25 powers on the device, in whole tiles, at least one tile, at most L"""
    return min(max((2 ** 25 // F) // tile * tile, tile), L)


def test_slab_rule_against_its_restatement():
    """light curves per slab of mtg_lomb_scargle and mtg_epoch_fold (csrc/mtg_ls_plan.h: mtg_ls_slab)"""
    with tempfile.TemporaryDirectory(prefix="ls_slab_") as tmp:
        exe = os.path.join(tmp, "ls_multi_plan_driver")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "mind_the_gaps_amd", "csrc"),
                               os.path.join(HERE, "ls_multi_plan_driver.cpp"), "-o", exe])
        tiles = sorted({planned_tile(K, 100, 1, w) for K in (1, 2, 3, 4, 5) for w in (0, 1)} | {1, 2, 4})    # mtg_ls_full_tile's, mtg_ef_plan's
        assert tiles == [1, 2, 4, 6, 8, 10, 16]
        cases = []
        for F in (1, 3, 70, 2 ** 21, 2 ** 21 + 1, 2 ** 25 - 1, 2 ** 25, 2 ** 25 + 1):
            for tile in tiles:
                one = planned_slab(F, tile, 10 ** 12)      # a slab of a set too large for one
                cases += [(F, tile, L) for L in sorted({1, 2, tile, tile + 1, max(one - 1, 1), one, one + 1, 3 * one + 1, 10 ** 6})]
        r = subprocess.run([exe], input="".join("slab %d %d %d\n" % c for c in cases), capture_output=True, text=True, check=True)
        got = [int(v) for v in r.stdout.split()]
        assert len(got) == len(cases)
        for (F, tile, L), slab in zip(cases, got):
            assert slab == planned_slab(F, tile, L), (F, tile, L, slab)
            assert slab == L or slab % tile == 0, (F, tile, L, slab)             # whole tiles, unless the whole set
            assert slab == L or slab >= tile, (F, tile, L, slab)                 # at least one tile, or the whole set
            assert 1 <= slab <= L
            assert slab * F <= 2 ** 25 or slab == min(tile, L), (F, tile, L, slab)   # the budget, but where one tile exceeds it
        # pinned: one frequency keeps 2^25 light curves; 2^21 frequencies 16, whatever the tile divides; past the budget a tile
        assert got[cases.index((1, 1, 10 ** 6))] == 10 ** 6
        assert [planned_slab(2 ** 21, tile, 100) for tile in tiles] == [16, 16, 16, 12, 16, 10, 16]
        assert [planned_slab(2 ** 25 + 1, tile, 100) for tile in tiles] == tiles
        assert planned_slab(2 ** 25, 1, 100) == 1 and planned_slab(2 ** 25, 4, 3) == 3


def test_resource_report_lists_every_instantiation_without_scratch():
    text = open(os.path.join(ROOT, "profiles", "lomb_scargle_multi_resources.txt")).read()
    rows = {m.group(1): [int(v) for v in m.group(2).split()]
            for m in re.finditer(r"^mtg_lomb_scargle_multi_kernel<([^>]*)>\s+([\d\s]+)$", text, flags=re.M)}
    want = set()
    for K in (2, 3, 4, 5):
        for w in (0, 1):
            for R in {1, planned_tile(K, 100, 1, w)}:
                want.add("%d, %d, %s" % (K, R, "true" if w else "false"))
    assert set(rows) == want
    for name, (sgpr, vgpr, agpr, scratch, occupancy, sspill, vspill, lds) in rows.items():
        assert scratch == 0 and sspill == 0 and vspill == 0 and vgpr + agpr <= 256 and occupancy >= 2, name
        assert 2 * lds <= 160 * 1024, name


def test_nterms_is_accepted_up_to_five_and_the_rest_still_refused():
    t, y = np.arange(12.0), np.zeros(12)
    for K in (1, 3, 4, 5):
        assert LombScargle(t, y, nterms=K).nterms == K          # (nterms = 3 raised before this feature)
    # (nterms = 2 through this class raises; Engine.lomb_scargle takes it)
    for kw in (dict(nterms=2), dict(nterms=6), dict(nterms=0), dict(fit_mean=False), dict(center_data=False)):
        with pytest.raises(NotImplementedError, match=list(kw)[0]):
            LombScargle(t, y, **kw)


def test_entries_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "mtg.h")).read()
    assert int(re.search(r"MTG_LS_MAX_TERMS\s*=\s*(\d+)", text).group(1)) == engine.LS_MAX_TERMS == 5
    lib = engine.load_library()
    for name, base, arity in (("mtg_lomb_scargle_multi", "mtg_lomb_scargle", 9),
                              ("mtg_lomb_scargle_envelope_multi", "mtg_lomb_scargle_envelope", 15)):
        params = {}
        for entry in (name, base):
            decl = re.search(r"MTG_API\s+int\s+%s\s*\(([^;]*)\)\s*;" % entry, text)
            params[entry] = [p.split()[-1].lstrip("*") for p in re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).split(",")]
        # the existing entry's arguments with nterms before the normalization
        at = params[base].index("normalization")
        assert params[name] == params[base][:at] + ["nterms"] + params[base][at:]
        assert name in engine.EXPORTS
        assert len(getattr(lib, name).argtypes) == len(params[name]) == arity
    assert "nterms" in engine.Engine.lomb_scargle.__code__.co_varnames and "nterms" in engine.Engine.lomb_scargle_envelope.__code__.co_varnames
    # no context: an argument error, nothing touched
    assert lib.mtg_lomb_scargle_multi(None, 1, None, 2, 0, 1, None, None, None) == engine.E_ARG
