"""What a context computed before does not change what it computes now: the hipFFT plans a context keeps (simulator, chirp-z,
E13 adjustment, convergence check: csrc/mtg_capi.hip's FftPlan, slots by csrc/mtg_sim_plan.h) are remade, kept or evicted by
the calls that came earlier, and every result must be the one a fresh context gives, bit for bit.  Engine.simulate_tk95 with
a tabulated spectrum on N = 8 epochs; every case once on a context of its own, and once on a context that has first run all
of them in a mixed order."""
import numpy as np
import pytest

from mind_the_gaps_amd import synthetic as synth
from mind_the_gaps_amd.engine import Engine

pytestmark = pytest.mark.gpu

N = 8
KINDS = [synth.K_DRW]
THETA = synth.truth(KINDS)

# name -> (nfft, S, transform, pairs, flux pdf, seg_len, make_resident).  At 256 points the library's plan runs 256 series
# per execution: 257 series end on a short group, 1 and 3 take the second plan slot.  254 = 2 x 127 goes through chirp-z
# transforms of 512 points, 128 per execution: with pairs an odd number of series leaves a pair half filled.
CASES = {}
for S in (1, 3, 257):
    CASES["native-256-S%d" % S] = (256, S, "auto", True, "gaussian", 64, False)
for pairs in (True, False):
    for S in (1, 3, 257):
        CASES["chirpz-254-S%d-%s" % (S, "pairs" if pairs else "single")] = (254, S, "auto", pairs, "gaussian", 64, False)
CASES["library-254-S257"] = (254, 257, "library", True, "gaussian", 64, False)     # takes the bulk slot of the library's plans ...
CASES["native-256-S257-again"] = (256, 257, "auto", True, "gaussian", 64, False)   # ... which this call remakes
CASES["lognormal-seg64"] = (256, 3, "auto", True, "lognormal", 64, False)
CASES["lognormal-seg96"] = (256, 3, "auto", True, "lognormal", 96, False)          # the E13 pair is remade
CASES["resident-then-loglike"] = (256, 3, "auto", True, "gaussian", 64, True)
MIXED = [5, 0, 9, 12, 2, 7, 11, 4, 13, 1, 8, 10, 3, 6]                              # the order of the history


def make_engine():
    eng = Engine(0)
    t = np.arange(N) * 8.0 + 3.0
    y = np.sin(t)[None, :] + 10.0
    full, free, bounds = synth.model_spec(KINDS, y, per_lc_mean=True)
    eng.set_lightcurves(t, y, np.full((1, N), 0.5), y_offset=y.mean(axis=1))
    eng.set_model(KINDS, full, free, bounds)
    return eng


def run_case(eng, name):
    nfft, S, transform, pairs, pdf, seg_len, resident = CASES[name]
    step = seg_len // N
    lo = np.arange(N, dtype=np.int32) * step
    table = 1.0 / (1.0 + (np.arange(nfft // 2 + 1) / 8.0) ** 2)
    eng.set_simulate_transform(transform)
    eng.set_simulate_pairs(pairs)
    eng.set_simulate_pdf(pdf)
    out = eng.simulate_tk95(S, 1234, nfft, 1.0, 10.0, seg_len, lo, lo + step - 2, noise_kind=1, sigma_noise=0.5,
                            want_clean=True, want_segments=True, make_resident=resident, psd_table=table)
    if resident:
        out["lnp"], out["status"] = eng.loglike(np.tile(THETA, (S, 1)), np.arange(S, dtype=np.int32), add_prior=False)
        sampling = np.arange(N) * 8.0 + 3.0        # the next case starts from one light curve again
        y = np.sin(sampling)[None, :] + 10.0
        eng.set_lightcurves(sampling, y, np.full((1, N), 0.5), y_offset=y.mean(axis=1))
    return {k: v for k, v in out.items() if v is not None}


@pytest.fixture(scope="module")
def fresh():
    """every case on a context that has done nothing else"""
    got = {}
    for name in CASES:
        eng = make_engine()
        got[name] = run_case(eng, name)
        eng.close()
    return got


@pytest.fixture(scope="module")
def used():
    """every case on ONE context that has first run all of them in a mixed order"""
    names = list(CASES)
    assert sorted(MIXED) == list(range(len(names)))
    eng = make_engine()
    for i in MIXED:
        run_case(eng, names[i])
    got = {name: run_case(eng, name) for name in names}
    yield got, eng
    eng.close()


@pytest.mark.parametrize("name", list(CASES))
def test_history_does_not_change_a_simulation(fresh, used, name):
    a, b = fresh[name], used[0][name]
    assert set(a) == set(b) and {"rates", "dy", "means", "clean", "segments"} <= set(a)
    assert np.all(np.isfinite(a["rates"])) and np.std(a["clean"]) > 0
    for key in a:
        assert np.array_equal(a[key], b[key]), (name, key, np.max(np.abs(a[key] - b[key])))
    if "lnp" in a:
        assert np.all(a["status"] == 0) and np.all(np.isfinite(a["lnp"]))


def test_cases_differ_where_they_should(fresh):
    """the comparison above is not one of equal constants: another grid, another flux PDF, another segment give other series"""
    assert not np.array_equal(fresh["native-256-S3"]["clean"], fresh["chirpz-254-S3-pairs"]["clean"])
    assert not np.array_equal(fresh["native-256-S3"]["clean"], fresh["lognormal-seg64"]["clean"])
    assert not np.array_equal(fresh["lognormal-seg64"]["clean"], fresh["lognormal-seg96"]["clean"])
    assert np.array_equal(fresh["native-256-S257"]["rates"], fresh["native-256-S257-again"]["rates"])
    assert np.array_equal(fresh["native-256-S257"]["rates"][:3], fresh["native-256-S3"]["rates"])     # a series is its global index's


def test_convergence_check_plans_are_evicted_and_remade(used):
    """four plan slots, the least recently used one making room: a fifth shape evicts the first, whose return costs a
    sixth pair -- and gives the values of its first call"""
    eng = used[1]
    rng = np.random.default_rng(5)
    chains = [rng.standard_normal((200, 6, k)).cumsum(axis=0) for k in (2, 3, 4, 5, 6)]
    built = eng.acf_plans_built
    first = [eng.chain_autocorr(c) for c in chains]
    assert eng.acf_plans_built == built + 5
    again = eng.chain_autocorr(chains[0])
    assert eng.acf_plans_built == built + 6
    assert np.array_equal(again, first[0])
    assert np.array_equal(eng.chain_autocorr(chains[4]), first[4]) and eng.acf_plans_built == built + 6     # still held
