"""mtg_lomb_scargle_envelope on the GPU: order statistics, valid and exceed counts down the columns of the power array,
ratio peaks along its rows -- none of which brings the array to the host.

Every expected value is formed on the host from ``Engine.lomb_scargle(power=True)`` (unchanged by the entry under test)
with numpy: ``np.sort(axis=0)`` puts NaN last, ``>=`` and ``/`` are IEEE.  All comparisons are exact.  N is small
throughout: the periodogram itself is not under test.
"""
import numpy as np
import pytest

from lomb_scargle_envelope_plan import Planner
from mind_the_gaps_amd import engine
from mind_the_gaps_amd.engine import Engine, EngineError

pytestmark = pytest.mark.gpu

PLANNER = Planner()
# one L on each side of every boundary of the implementation: where the columns a workgroup carries change, and where the
# LDS sort hands over to the segmented sort (named by the planner, tests/lomb_scargle_envelope_plan.py)
BOUNDARIES = PLANNER.boundaries()
BOUNDARY_LS = [L + d for L, _ in BOUNDARIES for d in (0, 1)]


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def make_set(L, N, seed, per_lc=False):
    rng = np.random.default_rng(seed)
    t = np.sort(rng.uniform(0.0, 40.0, size=(L, N) if per_lc else N), axis=-1) + 100.0
    y = rng.standard_normal((L, N)) + np.sin(0.9 * t)
    dy = rng.uniform(0.1, 0.5, size=(L, N))
    return t, y, dy


def host(power, ranks, reference, scale):
    """The one-shot host computation -> (order_stat, valid, exceed, peak_ratio, peak_ratio_index)"""
    L = len(power)
    with np.errstate(invalid="ignore"):
        order = np.sort(power, axis=0)[np.asarray(ranks, dtype=int)]
        valid = np.sum(~np.isnan(power), axis=0)
        exceed = np.sum(power >= reference, axis=0)
        ratio = power / scale
    masked = np.where(np.isnan(ratio), -np.inf, ratio)
    ix = masked.argmax(axis=1)
    pk = ratio[np.arange(L), ix]
    ix = np.where(np.isnan(ratio).all(axis=1), -1, ix)
    return order, valid, exceed, pk, ix


def check(eng, freqs, ranks, reference, scale, norm, weighted, where):
    power = eng.lomb_scargle(freqs, normalization=norm, weighted=weighted)
    want = host(power, ranks, reference, scale)
    got = eng.lomb_scargle_envelope(freqs, ranks=ranks, reference=reference, scale=scale, normalization=norm, weighted=weighted)
    names = ("order_stat", "valid", "exceed", "peak_ratio", "peak_ratio_index")
    for name, g, w in zip(names, got, want):
        assert g.shape == w.shape and np.array_equal(g, w, equal_nan=name in ("order_stat", "peak_ratio")), (where, name)
    return power, got


def references(power, rng):
    """a reference that splits every column (one of its own entries, so that >= meets equality) and a positive scale"""
    L, F = power.shape
    pick = np.nan_to_num(power[rng.integers(L, size=F), np.arange(F)], nan=0.25)
    return pick, np.nan_to_num(np.abs(power[rng.integers(L, size=F), np.arange(F)]), nan=1.0) + 1e-3


@pytest.mark.parametrize("L", [1, 2, 11] + BOUNDARY_LS)
def test_smallest_shapes_and_both_sides_of_every_boundary(eng, L):
    plan = PLANNER.plan(L)
    rng = np.random.default_rng(L)
    # every rank of the smallest sets; otherwise descending, with duplicates
    ranks = np.arange(L) if L <= 2 else np.array([L - 1, L - 1, (2 * L) // 3, L // 2, 1, 0, L // 2])
    # 37: no multiple of any column count but 1
    widths = (1, 7, 37) if L <= 11 else (37,)
    for per_lc in (False, True):
        t, y, dy = make_set(L, 8, seed=L + per_lc, per_lc=per_lc)
        eng.set_lightcurves(t, y, dy)
        for F in widths:
            freqs = rng.uniform(0.02, 0.5, size=F)
            for weighted, norm in ((True, "standard"), (False, "psd"), (True, "log"), (False, "standard")):
                power = eng.lomb_scargle(freqs, normalization=norm, weighted=weighted)
                reference, scale = references(power, rng)
                check(eng, freqs, ranks, reference, scale, norm, weighted, (L, per_lc, F, weighted, norm))
                if plan["in_lds"]:
                    assert eng.last_solver == "mtg_ls_envelope_column_kernel<%d>" % plan["columns"]
                    assert plan["columns"] == 1 or 37 % plan["columns"] != 0
                else:
                    assert eng.last_solver == "mtg_ls_envelope_select_kernel"
                assert eng.last_kernel_ms > 0


def test_frequency_slabs_and_the_first_maximum_across_them(eng):
    L, Q = 1025, 5
    width = PLANNER.plan(L, 10 ** 9, Q)["width"]
    F = width + 100                                       # a second slab of 100 columns: L F 8 bytes just exceed the budget
    assert L * width * 8 <= PLANNER.budget < L * F * 8 and PLANNER.plan(L, F, Q)["width"] == width
    rng = np.random.default_rng(9)
    t, y, dy = make_set(L, 8, seed=9)
    eng.set_lightcurves(t, y, dy)
    freqs = rng.uniform(0.02, 0.5, size=F)
    freqs[width + 7] = freqs[3]                           # one frequency in both slabs
    power = eng.lomb_scargle(freqs)
    assert np.array_equal(power[:, 3], power[:, width + 7])
    reference, scale = references(power, rng)
    # that column's ratio is the largest of most light curves: its median scaled down far below the other columns'
    scale[3] = scale[width + 7] = 1e-4 * np.median(power[:, 3])
    ranks = np.array([L - 1, 0, L // 2, 974, 974])
    _, got = check(eng, freqs, ranks, reference, scale, "standard", True, "two slabs")
    assert np.sum(got.peak_ratio_index == 3) > L // 2 and not np.any(got.peak_ratio_index == width + 7)


def test_nan_powers_are_last_uncounted_and_passed_over(eng):
    # 16 samples with weights 1 / 16 at whole-number times: at a whole-number frequency every phase is a whole cycle,
    # cos = 1 and sin = 0 exactly, CC SS - CS^2 = 0 and the power is NaN; the other light curves' times are not whole
    L, N = 11, 16
    t, y, dy = make_set(L, N, seed=4, per_lc=True)
    whole = [0, 3, 7]
    for l in whole:
        t[l] = 100.0 + np.sort(np.random.default_rng(l).choice(40, size=N, replace=False))
    eng.set_lightcurves(t, y, dy)
    freqs = np.array([0.37, 1.0, 0.81, 2.0, 3.0, 0.05])
    power = eng.lomb_scargle(freqs, weighted=False)
    nan = np.isnan(power)
    assert np.array_equal(np.flatnonzero(nan[:, 1]), whole) and nan[:, [1, 3, 4]].all(axis=1).sum() == 3
    assert not nan[:, [0, 2, 5]].any()                     # NaN in some entries of some columns, not in all
    rng = np.random.default_rng(4)
    reference, scale = references(power, rng)
    _, got = check(eng, freqs, np.arange(L)[::-1], reference, scale, "standard", False, "NaN")
    assert np.array_equal(got.valid, [11, 8, 11, 8, 8, 11])
    assert np.isnan(got.order_stat[:3, 1]).all() and not np.isnan(got.order_stat[3:, 1]).any()   # (ranks 10, 9, 8 first)
    assert np.all(got.exceed <= got.valid) and np.all(got.peak_ratio_index >= 0)
    # rows of nothing but NaN: NaN and -1
    only = freqs[[1, 3, 4]]
    _, got = check(eng, only, [0, 7, 8, 10], reference[[1, 3, 4]], scale[[1, 3, 4]], "standard", False, "all-NaN rows")
    assert np.array_equal(got.peak_ratio_index[whole], [-1, -1, -1]) and np.isnan(got.peak_ratio[whole]).all()
    assert np.all(got.peak_ratio_index[[1, 2, 4, 5, 6, 8, 9, 10]] >= 0)
    assert np.isnan(got.order_stat[2:]).all() and not np.isnan(got.order_stat[:2]).any()


def test_invariances_bit_for_bit(eng):
    L, N, F = 11, 32, 300
    rng = np.random.default_rng(12)
    t, y, dy = make_set(L, N, seed=12)
    freqs = rng.uniform(0.02, 0.4, size=F)
    ranks = [10, 5, 0, 5]
    for weighted in (True, False):
        eng.set_lightcurves(t, y, dy)
        power = eng.lomb_scargle(freqs, weighted=weighted)
        reference, scale = references(power, rng)
        kw = dict(ranks=ranks, weighted=weighted)
        base = eng.lomb_scargle_envelope(freqs, reference=reference, scale=scale, **kw)
        # column k from F = 1 against F = 300 permuted
        perm = rng.permutation(F)
        shuffled = eng.lomb_scargle_envelope(freqs[perm], reference=reference[perm], scale=scale[perm], **kw)
        assert np.array_equal(shuffled.order_stat, base.order_stat[:, perm])
        assert np.array_equal(shuffled.valid, base.valid[perm]) and np.array_equal(shuffled.exceed, base.exceed[perm])
        assert np.array_equal(shuffled.peak_ratio, base.peak_ratio)
        for k in (0, 63, 64, 255, 256, 299):
            one = eng.lomb_scargle_envelope(freqs[k:k + 1], reference=reference[k:k + 1], scale=scale[k:k + 1], **kw)
            assert np.array_equal(one.order_stat[:, 0], base.order_stat[:, k]) and one.exceed[0] == base.exceed[k]
            assert one.valid[0] == base.valid[k] and np.array_equal(one.peak_ratio, power[:, k] / scale[k])
        # the light curves in another order: a column is a set
        order = rng.permutation(L)
        eng.set_lightcurves(t, y[order], dy[order])
        moved = eng.lomb_scargle_envelope(freqs, reference=reference, scale=scale, **kw)
        for name in ("order_stat", "valid", "exceed"):
            assert np.array_equal(getattr(moved, name), getattr(base, name)), name
        assert np.array_equal(moved.peak_ratio, base.peak_ratio[order])
        assert np.array_equal(moved.peak_ratio_index, base.peak_ratio_index[order])
        # the same sampling stored per light curve
        eng.set_lightcurves(np.tile(t, (L, 1)), y, dy)
        stored = eng.lomb_scargle_envelope(freqs, reference=reference, scale=scale, **kw)
        for name in base._fields:
            assert np.array_equal(getattr(stored, name), getattr(base, name)), name


def test_refusals_and_the_resident_set_afterwards(eng):
    fresh = Engine(0)
    who = "mtg_lomb_scargle_envelope"
    try:
        with pytest.raises(EngineError) as exc:
            fresh.lomb_scargle_envelope([0.1], ranks=[0])
        assert exc.value.code == engine.E_STATE and "mtg_set_lightcurves" in str(exc.value)
        fresh.set_lightcurves(np.array([0.0, 1.0, 2.5]), np.array([1.0, 2.0, 0.5]), np.ones(3))
        with pytest.raises(EngineError) as exc:
            fresh.lomb_scargle_envelope([0.1], ranks=[0])
        assert exc.value.code == engine.E_ARG and who + ": N = 3" in str(exc.value)
        t, y, dy = make_set(5, 12, seed=2)
        fresh.set_lightcurves(t, y, dy)
        f = np.array([0.1, 0.2, 0.3])
        before = fresh.lomb_scargle(f)
        ones = np.ones(3)
        refused = [
            (dict(freqs=[], ranks=[0]), "F >= 1"),
            (dict(freqs=[0.1, np.nan], ranks=[0]), "freqs[1]"),
            (dict(freqs=[-1.0], ranks=[0]), "freqs[0]"),
            (dict(freqs=f, ranks=[0], normalization=4), "normalization 4"),
            (dict(freqs=f, ranks=[0, 5]), "ranks[1] = 5"),
            (dict(freqs=f, ranks=[-1]), "ranks[0] = -1"),
            (dict(freqs=f, reference=[1.0, np.inf, 1.0]), "reference[1]"),
            (dict(freqs=f, reference=[np.nan, 1.0, 1.0]), "reference[0]"),
            (dict(freqs=f, scale=[1.0, 1.0, 0.0]), "scale[2]"),
            (dict(freqs=f, scale=[1.0, -2.0, 1.0]), "scale[1]"),
            (dict(freqs=f, scale=[np.inf, 1.0, 1.0]), "scale[0]"),
            (dict(freqs=f), "all NULL"),
        ]
        for kw, word in refused:
            with pytest.raises(EngineError) as exc:
                fresh.lomb_scargle_envelope(**kw)
            assert exc.value.code == engine.E_ARG and who in str(exc.value) and word in str(exc.value), (kw, str(exc.value))
        # what the method cannot express, through the C entry itself
        lib, ctx = fresh._lib, fresh._ctx
        fp = engine._ptr
        ip = lambda a: a.ctypes.data_as(engine.ctypes.POINTER(engine.ctypes.c_int64))
        r, os_, cnt, pk, ix = np.zeros(1, dtype=np.int64), np.zeros((1, 3)), np.zeros(3, dtype=np.int64), np.zeros(5), np.zeros(5, dtype=np.int64)
        direct = [
            ((-1, None, None, ip(cnt), None, None, None, None, None), "Q = -1"),
            ((1, ip(r), None, None, None, None, None, None, None), "order_stat is NULL"),
            ((0, None, None, None, None, ip(cnt), None, None, None), "exceed needs reference"),
            ((0, None, None, None, None, None, None, fp(pk), None), "need scale"),
            ((0, None, None, None, None, None, None, None, ip(ix)), "need scale"),
            ((0, None, None, None, fp(ones), None, fp(ones), None, None), "all NULL"),
        ]
        for args, word in direct:
            rc = lib.mtg_lomb_scargle_envelope(ctx, 3, fp(f), 0, 1, *args)
            msg = lib.mtg_last_error(ctx).decode()
            assert rc == engine.E_ARG and who in msg and word in msg, (word, msg)
        del os_
        # the resident set is as it was, and the entry works after the refusals
        assert np.array_equal(fresh.lomb_scargle(f), before)
        got = fresh.lomb_scargle_envelope(f, ranks=[4, 0], reference=ones * 0.1)
        assert np.array_equal(got.order_stat, np.sort(before, axis=0)[[4, 0]]) and got.peak_ratio is None
        assert np.array_equal(got.exceed, np.sum(before >= 0.1, axis=0)) and np.array_equal(got.valid, [5, 5, 5])
        assert fresh.last_solver == "mtg_ls_envelope_column_kernel<%d>" % PLANNER.plan(5)["columns"]
        only = fresh.lomb_scargle_envelope(f, scale=ones)
        assert only.order_stat is None and only.valid is None and only.exceed is None
        assert np.array_equal(only.peak_ratio, before.max(axis=1)) and np.array_equal(only.peak_ratio_index, before.argmax(axis=1))
        assert np.array_equal(fresh.lomb_scargle(f), before)
    finally:
        fresh.close()


def test_envelope_levels_are_numpys_quantiles_of_the_power_array(eng):
    from mind_the_gaps_amd.periodogram import envelope_levels, envelope_ranks
    L = 23
    t, y, dy = make_set(L, 24, seed=31)
    eng.set_lightcurves(t, y, dy)
    freqs = np.linspace(0.03, 0.45, 29)
    levels = (0.5, 0.95, 0.997, 0.1, 1.0)
    ranks = envelope_ranks(L, levels)
    for norm in ("standard", "psd"):
        power = eng.lomb_scargle(freqs, normalization=norm)
        got = eng.lomb_scargle_envelope(freqs, ranks=ranks, normalization=norm)
        # numpy's own interpolation form (a + (b - a) t, b - (b - a) (1 - t) from t = 1/2 on) on the same two neighbours: exact
        assert np.array_equal(envelope_levels(got.order_stat, ranks, L, levels), np.quantile(power, levels, axis=0))


def test_periodogram_significance(eng):
    from mind_the_gaps_amd import synthetic as synth
    from mind_the_gaps_amd.lightcurves import GappyLightcurve
    from mind_the_gaps_amd.models import DampedRandomWalk
    from mind_the_gaps_amd.ppp import periodogram_peak_test, periodogram_significance
    th = synth.truth(synth.ALT_MODEL)
    times, rates, err = synth.make_lightcurves(60, 1, seed=43)
    lc = GappyLightcurve(times, rates[0] + 50.0, err[0], exposures=0.5 * np.diff(times).min())
    T = times[-1] - times[0]
    freqs = np.linspace(1.0 / T, 20.0 / T, 12)

    def kernel():
        return DampedRandomWalk(th[0], th[1], bounds=[(-10, 50), (-10, 10)])
    kw = dict(nsims=16, walkers=8, max_steps=60, sigma_noise=0.5, seed=21)
    levels = (0.9, 0.99)
    first = periodogram_significance(lc, kernel(), freqs, levels=levels, **kw)
    again = periodogram_significance(lc, kernel(), freqs, levels=levels, **kw)
    for key in ("observed_power", "median", "levels", "local_p", "sim_ratio_peaks", "samples"):
        assert np.array_equal(first[key], again[key]), key
    for key in ("observed_ratio_peak", "observed_frequency", "global_p", "sim_seed"):
        assert first[key] == again[key], key
    assert np.array_equal(first["lightcurves"]["rates"], again["lightcurves"]["rates"])
    # the chain, the picks and the simulated set of the peak test
    peak = periodogram_peak_test(lc, kernel(), freqs, **kw)
    assert np.array_equal(peak["samples"], first["samples"]) and peak["sim_seed"] == first["sim_seed"]
    assert np.array_equal(peak["lightcurves"]["rates"], first["lightcurves"]["rates"])
    assert np.array_equal(peak["lightcurves"]["dy"], first["lightcurves"]["dy"])
    # the host computation from the power array of the returned light curves
    out = first["lightcurves"]
    eng.set_lightcurves(times, out["rates"], out["dy"] + 1e-12, y_offset=out["means"])
    power = eng.lomb_scargle(freqs)
    sim_peaks, _ = eng.lomb_scargle(freqs, power=False, peak=True)
    assert np.array_equal(sim_peaks, peak["sim_peaks"])        # (the set is the one both functions had resident)
    q = np.quantile(power, (0.5,) + levels, axis=0)
    assert np.array_equal(first["median"], q[0]) and np.array_equal(first["levels"], q[1:])
    eng.set_lightcurves(times, lc.y, lc.dy)
    observed = eng.lomb_scargle(freqs)[0]
    assert np.array_equal(first["observed_power"], observed)
    assert np.array_equal(first["local_p"], (1.0 + np.sum(power >= observed, axis=0)) / 17.0)
    ratio = power / q[0]
    assert np.array_equal(first["sim_ratio_peaks"], ratio.max(axis=1))
    assert first["observed_ratio_peak"] == (observed / q[0]).max() and first["observed_frequency"] == freqs[np.argmax(observed / q[0])]
    assert first["global_p"] == (1.0 + np.sum(ratio.max(axis=1) >= first["observed_ratio_peak"])) / 17.0
    assert 0.0 < first["global_p"] <= 1.0 and first["null"] is not None
