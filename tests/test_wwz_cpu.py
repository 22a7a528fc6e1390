"""The weighted wavelet Z-transform without a GPU:

* the fixture tests/golden/wwz_golden.npz (scripts/make_wwz_golden.py): its layout, its grid, and the share of entries
  with N_eff < 4 that the GPU test leaves out of the accuracy comparison (at most 10 % of a case);
* the float64 helper tests/wwz_numpy.py against the 50-digit truth, within the bounds the GPU test uses;
* the planner csrc/mtg_wwz_plan.h through tests/wwz_plan_driver.cpp against a restatement, its LDS budget and its grid;
* the compiler's resource report: every instantiation, no scratch, two waves per SIMD;
* the header's constants against engine.py; the entry declared, exported and bound with the header's arity;
* the argument checks of Engine.wwz, periodogram.WWZ and ppp.periodogram_peak_test that need no device.
"""
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import wwz_numpy as wn
from mind_the_gaps_amd import engine, periodogram

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CASES = ("n52", "n216", "n789", "fast216")
QUANTITIES = ("power", "z", "amplitude", "neff", "vx", "kappa")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "wwz_golden.npz"))


@pytest.fixture(scope="module")
def ls_golden():
    return np.load(os.path.join(HERE, "golden", "lomb_scargle_golden.npz"))


@pytest.mark.parametrize("name", CASES)
def test_fixture_layout_grid_and_left_out_share(golden, ls_golden, name):
    assert tuple(str(c) for c in golden["cases"]) == CASES
    decays = golden["decays"]
    assert decays[0] == wn.DECAY == engine.WWZ_DECAY and decays[1] == 0.001 and decays[2] == 0.0
    t = ls_golden[name + "/t"]
    f, taus = golden[name + "/freqs"], golden[name + "/taus"]
    span, nyquist = t[-1] - t[0], 0.5 * len(t) / (t[-1] - t[0])
    assert len(f) == 15 and np.isclose(f[0], 1.0 / span) and np.isclose(f[11], nyquist) and np.all(f[12:] > nyquist) and np.all(np.diff(f) > 0)
    assert len(taus) == 8 and np.all((taus[:6] > t[0]) & (taus[:6] < t[-1])) and taus[7] > t[-1]
    gap = int(np.argmax(np.diff(t)))
    assert t[gap] < taus[6] < t[gap + 1]
    left_out = 0
    for tag in "wu":
        for q in QUANTITIES:
            assert golden["%s/%s_%s" % (name, tag, q)].shape == (3, 8, 15)
        ne, P = golden["%s/%s_neff" % (name, tag)], golden["%s/%s_power" % (name, tag)]
        keep = ne >= 4.0
        left_out += int(np.sum(~keep))
        assert np.all(ne >= 1.0 - 1e-12) and np.all(ne <= len(t) * (1 + 1e-12))
        assert np.all((P[keep] >= 0) & (P[keep] <= 1)) and np.all(golden["%s/%s_kappa" % (name, tag)][keep] < 1e3)
        assert 0 <= float(golden["%s/%s_rho" % (name, tag)]) <= 1e-9 and 0 <= float(golden["%s/%s_rho_a" % (name, tag)]) <= 1e-9
        # Z and P are one truth
        Z = golden["%s/%s_z" % (name, tag)]
        assert np.allclose(Z[keep], (ne[keep] - 3.0) * P[keep] / (2.0 * (1.0 - P[keep])), rtol=1e-9)
    assert left_out <= 0.10 * 2 * 3 * 8 * 15
    # no window, unweighted: every sample counts once
    assert np.allclose(golden[name + "/u_neff"][2], len(t), rtol=1e-14)


@pytest.mark.parametrize("name", CASES)
def test_numpy_helper_matches_the_truth(golden, ls_golden, name):
    t, y, dy = (ls_golden["%s/%s" % (name, k)] for k in ("t", "y", "dy"))
    f, taus = golden[name + "/freqs"], golden[name + "/taus"]
    n = len(t)
    for tag, weighted in (("w", True), ("u", False)):
        rho, rho_a = float(golden["%s/%s_rho" % (name, tag)]), float(golden["%s/%s_rho_a" % (name, tag)])
        for ci, c in enumerate(golden["decays"]):
            want = {q: golden["%s/%s_%s" % (name, tag, q)][ci] for q in QUANTITIES}
            keep = want["neff"] >= 4.0
            got = wn.wwz(t, y, dy, f, taus, decay=float(c), weighted=weighted)
            k = want["kappa"]
            assert np.all(np.abs(got["power"] - want["power"])[keep] <= wn.bound_power(rho, n, k)[keep])
            assert np.all(np.abs(got["neff"] - want["neff"])[keep] <= (wn.bound_neff_rel(n) * want["neff"])[keep])
            assert np.all(np.abs(got["z"] - want["z"])[keep] <= wn.bound_z(rho, n, k, want["power"], want["neff"])[keep])
            assert np.all(np.abs(got["amplitude"] - want["amplitude"])[keep] <= wn.bound_amplitude(rho_a, n, k, want["vx"])[keep])
            assert np.allclose(got["kappa"][keep], k[keep], rtol=1e-6)


def planned(F, T, L, shared, weighted, rows):
    """csrc/mtg_wwz_plan.h restated"""
    tile = (4 if weighted else 8) if shared and L > 1 else 1
    lanes = 64 if F <= 64 else 128 if F <= 128 else 256
    nfb = -(-F // lanes)
    slab = (1 << 25) // F // T // tile * tile
    slab = min(max(slab, tile), L)
    lds = 32768 + 4096 + 4096 * (tile if weighted else (tile + 1) // 2) + 2048 + 8
    tiles = -(-rows // tile)
    blocks = nfb * T * tiles
    return tile, lanes, nfb, slab, lds, blocks if blocks <= 0x7fffffff and nfb * T <= 0x7fffffff else 0


def test_planner_matches_its_restatement_its_budget_and_its_grid():
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "wwz_plan_driver")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "mind_the_gaps_amd", "csrc"),
                               os.path.join(HERE, "wwz_plan_driver.cpp"), "-o", exe])
        cases = [(F, T, L, shared, weighted, rows) for F in (1, 64, 65, 128, 129, 300, 500, 1 << 18, 1 << 26) for T in (1, 8, 16, 100, 1 << 20)
                 for L in (1, 2, 9, 11, 2000) for shared in (0, 1) for weighted in (0, 1) for rows in (1, L)]
        r = subprocess.run([exe], input="".join("%d %d %d %d %d %d\n" % c for c in cases), capture_output=True, text=True, check=True)
        got = [tuple(int(v) for v in line.split()) for line in r.stdout.splitlines()]
        assert len(got) == len(cases)
        tiles = set()
        for c, g in zip(cases, got):
            assert g == planned(*c), (c, g)
            F, T, L, shared, weighted, rows = c
            tile, lanes, nfb, slab, lds, blocks = g
            tiles.add((tile, weighted))
            assert (shared and L > 1 or tile == 1) and lanes in (64, 128, 256) and nfb * lanes >= F > (nfb - 1) * lanes
            assert 1 <= slab <= L and (slab % tile == 0 or slab == L)
            # the maps of a slab stay within 2^25 entries unless one tile's alone are more
            assert slab * T * F <= max(1 << 25, tile * T * F)
            assert 2 * lds <= 160 * 1024     # two workgroups on a CU
            assert blocks == 0 or blocks == nfb * T * -(-rows // tile) <= 0x7fffffff
        assert tiles == {(1, 0), (1, 1), (4, 1), (8, 0)}
        # the headline set: tiles of 8 (4 weighted), two frequency blocks, slabs of 664 (668) light curves
        head = subprocess.run([exe], input="500 100 2000 1 0 2000\n500 100 2000 1 1 2000\n", capture_output=True, text=True, check=True).stdout.split()
        assert [int(v) for v in head] == [8, 256, 2, 664, 55304, 2 * 100 * 250, 4, 256, 2, 668, 55304, 2 * 100 * 500]


def test_resource_report_lists_every_instantiation_without_scratch_at_two_waves():
    rows = [line.split() for line in open(os.path.join(ROOT, "profiles", "wwz_resources.txt")) if line.startswith("mtg_")]
    names = {" ".join(r[:-8]): r for r in rows}
    for tile, weighted in ((1, "true"), (4, "true"), (1, "false"), (8, "false")):
        r = names["mtg_wwz_kernel<%d, %s>" % (tile, weighted)]
        assert int(r[-7]) <= 256 and int(r[-4]) >= 2      # VGPRs, waves per SIMD
        assert int(r[-1]) == planned(300, 1, 2 if tile > 1 else 1, 1, weighted == "true", 1)[4]   # LDS as planned
    assert "mtg_wwz_nearest_kernel" in names
    for r in rows:
        assert r[-5] == "0" and r[-3] == "0" and r[-2] == "0", r   # scratch, SGPR and VGPR spills


def test_entry_is_declared_exported_and_bound_and_the_constants_agree():
    text = open(os.path.join(ROOT, "include", "mtg.h")).read()
    for name, value in (("POWER", engine.WWZ_POWER), ("Z", engine.WWZ_Z), ("AMPLITUDE", engine.WWZ_AMPLITUDE)):
        assert int(re.search(r"#define\s+MTG_WWZ_%s\s+(\d+)" % name, text).group(1)) == value
    assert engine.WWZ_STATISTICS == {"power": 0, "z": 1, "amplitude": 2}
    assert float(re.search(r"#define\s+MTG_WWZ_DECAY\s+([0-9.eE+-]+)", text).group(1)) == engine.WWZ_DECAY == 1.0 / (8.0 * np.pi ** 2)
    lib = engine.load_library()
    params = ["ctx", "F", "freqs", "T", "taus", "decay", "statistic", "weighted", "out", "neff", "peak", "peak_index"]
    decl = re.search(r"MTG_API\s+int\s+mtg_wwz\s*\(([^;]*)\)\s*;", text)
    got = [p.split()[-1].lstrip("*") for p in re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).split(",")]
    assert got == params and "mtg_wwz" in engine.EXPORTS and len(lib.mtg_wwz.argtypes) == len(params)
    assert {"taus", "decay", "statistic", "weighted", "values", "neff", "peak"} <= set(engine.Engine.wwz.__code__.co_varnames)
    # no context: an argument error, nothing touched
    assert lib.mtg_wwz(None, 1, None, 1, None, engine.WWZ_DECAY, engine.WWZ_Z, 1, None, None, None, None) == engine.E_ARG
    # the chunk of the planner is the sweep's
    plan = open(os.path.join(ROOT, "mind_the_gaps_amd", "csrc", "mtg_wwz_plan.h")).read()
    phase = open(os.path.join(ROOT, "mind_the_gaps_amd", "csrc", "mtg_ls_phase.h")).read()
    assert re.search(r"MTG_WWZ_CHUNK\s*=\s*(\d+)", plan).group(1) == re.search(r"#define\s+MTG_LS_CHUNK\s+(\d+)", phase).group(1) == "256"


def test_argument_checks_that_need_no_device():
    t = np.arange(10.0)
    y = np.sin(t)
    with pytest.raises(ValueError, match="statistic"):
        periodogram.WWZ(t, y, statistic="psd")
    for bad in (-1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match="decay"):
            periodogram.WWZ(t, y, decay=bad)
    with pytest.raises(ValueError):
        periodogram.WWZ(t, y[:5])
    w = periodogram.WWZ(t, y)
    assert w.dy is None and w.decay == engine.WWZ_DECAY and w.statistic == "z"
    tau = w.autotau()
    assert len(tau) == 50 and tau[0] == 0.0 and tau[-1] == 9.0 and np.allclose(np.diff(tau), 9.0 / 49)
    assert len(w.autotau(7)) == 7
    with pytest.raises(ValueError):
        w.autotau(0)
    assert np.array_equal(w.autofrequency(), periodogram.LombScargle(t, y).autofrequency())
    with pytest.raises(ValueError, match="statistic"):
        w.power([0.1], [1.0], statistic="psd")

    from mind_the_gaps_amd import ppp
    with pytest.raises(ValueError, match="statistic"):
        ppp.periodogram_peak_test(None, None, [0.1], statistic="wavelet")
    with pytest.raises(ValueError, match="nterms"):
        ppp.periodogram_peak_test(None, None, [0.1], statistic="wwz", nterms=2)
    import inspect
    sig = inspect.signature(ppp.periodogram_peak_test).parameters
    assert sig["taus"].default is None and sig["decay"].default == engine.WWZ_DECAY and sig["statistic"].default == "lomb_scargle"
