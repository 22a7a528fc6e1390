"""The simulator's random draws and spectra on the device against their exact host replay (simulator_replay.py, itself
held to mpmath and to the Poisson law by test_simulator_replay_cpu.py): Poisson and Kraft counts count for count, the
Gaussian noise and E13's own lognormal and uniform draws block for block, the model spectrum term by term on both sides
of Q = 1 / 2, and calls of more than one chunk against the calls of their parts.

The figures the tolerances are set against (units of 2^-52 relative; printed by the CPU test, the device's by this one):
  R_draw   normal2 1.60 (held to 2);  uniform kind 1.00 (held to 2);  lognormal kind 2 + 1 x at exponent
           x = |s_ln z| for std / mean in [0.2, 1] (measured: 1.32 at x < 0.02, slope at most 0.62)
  R_psd    drw 1.79;  sho 1.47e3;  matern32 311;  complex4 30;  drw+sho+jitter 68.4   (rows within 1e-3 of Q = 1 / 2
           cancel in 1 +- 1 / f; the Matern term in a c - b d); each model is held to 8 x its own figure + 8
  undecided Poisson epochs (a decision of the replay taken by less than 1e-9 relative): 0 of 4800 / 6000 per case on
           the host; the cap here is 1 in 10^4
Measured on an MI355X (the same units):
  Poisson / Kraft   undecided share 0 in all four cases (smallest margin 1.5e-6); every count equal; dy 0.00 ulp off
  Gaussian noise    0.32 (base 0) and 0.35 (base 3) ulp of |clean| + |sigma g1|, bound 4
  E13 lognormal     sorted series within 1.2 .. 2.0 ulp of the replayed draws at S <= 5 (at most 0.10 of the bound),
                    4.9 ulp at S = 300 (0.20 of the bound); uniform 0.67 .. 0.77 ulp, 1.5 at S = 300, bound 4
  spectrum          drw 1.95 (bound 22);  sho 735 (1.2e4);  matern32 157 (2.5e3);  complex4 15.5 (248);
                    drw+sho+jitter 34 (555) -- the device lands within half of the replay's own error in every model
  chirp-z, S = 259  paired against single transforms 1.9e-15 of the scatter, bound 1e-12
Wrong kernels these tests were seen to fail against (scratch builds, one change each): 2.54 for 2.53 in PTRS's b
(ptrs-25 counts), sg for sg + sbase in the Gaussian branch (base 3), var for sd in the uniform half-width
(E13 kind 2), nr0 + sig for nr0 + 2 sig (sho spectrum)."""
import numpy as np
import pytest

import simulator_replay as sr
from mind_the_gaps_amd import synthetic as synth
from mind_the_gaps_amd.models import DampedRandomWalk
from mind_the_gaps_amd.simulator import Simulator

pytestmark = pytest.mark.gpu
EPS = sr.EPS

def test_replay_speaks_the_packages_term_kinds():
    for name in ("K_REAL", "K_COMPLEX3", "K_COMPLEX4", "K_SHO", "K_MATERN32", "K_JITTER", "K_DRW", "K_LORENTZIAN"):
        assert getattr(sr, name) == getattr(synth, name) and sr.NPARAMS[getattr(sr, name)] == synth.NPARAMS[getattr(synth, name)]


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


# ---- (a) Poisson and Kraft, count for count ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def poisson_runs():
    """every case once: the whole set with its clean rates, and series 7 .. 39 as a block of their own"""
    got = {}
    for name in list(sr.POISSON_CASES) + ["kraft"]:
        sim, thetas, seed = sr.kraft_simulator() if name == "kraft" else sr.poisson_simulator(name)
        whole = sim.simulate(thetas, seed=seed, want_clean=True, index_base=0)
        block = sim.simulate(thetas[7:], seed=seed, index_base=7)
        got[name] = (sim, seed, whole, block)
    return got


@pytest.mark.parametrize("name", list(sr.POISSON_CASES) + ["kraft"])
def test_poisson_counts_are_the_replays(poisson_runs, name):
    """tk95_poisson on the counters (epoch, 10, series, trip): from the device's own clean rates the replay gives the
    count of every decided epoch exactly -- Knuth below 10, PTRS above, NaN for a negative mean in that epoch alone --
    and dy = sqrt(counts) / exposure within 2 ulp; for Kraft noise the total picks the table entry or the Poisson
    formulas.  Undecided epochs: at most 1 in 10^4.  A block (index_base = 7) is the whole set's series 7 .. 39."""
    sim, seed, whole, block = poisson_runs[name]
    rates, dy, clean = whole["rates"], whole["dy"], whole["clean"]
    S, N = rates.shape
    assert (S, N) == (sr.POISSON_S, len(sim._times))
    expo, bkg = sim._exposures[None, :], sim._bkg_counts[None, :]
    lam = clean * expo + bkg if name == "kraft" else clean * expo
    counts, margin = sr.poisson(lam, np.arange(N)[None, :], np.arange(S)[:, None], seed)
    decided = margin > sr.DECIDED
    share = 1.0 - decided.mean()
    negative = ~(lam >= 0.0)
    print("%s: lam %.2f .. %.2f, %d of %d epochs with a negative mean, undecided share %.3g, smallest margin %.3g"
          % (name, np.nanmin(lam), np.nanmax(lam), negative.sum(), lam.size, share, margin.min()))
    assert share <= 1e-4
    assert np.array_equal(np.isnan(rates), negative) and np.array_equal(np.isnan(dy), negative)
    ok = decided & ~negative
    if name == "kraft":
        med, half = sim._kraft_tables()
        err = sim._bkg_rate_err[None, :]
        faint = ok & (counts < sim.kraft_counts)
        bright = ok & ~faint
        at = np.where(faint, counts, 0).astype(np.int64)
        n_of = np.broadcast_to(np.arange(N)[None, :], (S, N))
        assert np.array_equal(rates[faint], (med[n_of, at] / expo)[faint]) and np.array_equal(dy[faint], (half[n_of, at] / expo)[faint])
        assert np.array_equal(rates[bright], ((counts - bkg) / expo)[bright])
        want_dy = np.sqrt((np.sqrt(counts) / expo) ** 2 + err ** 2)
        assert np.all(np.abs(dy - want_dy)[bright] <= 2 * EPS * want_dy[bright])
        assert faint.mean() > 0.05 and bright.mean() > 0.05
    else:
        assert _same((rates * expo)[ok], counts[ok]) and _same(rates[ok], (counts / expo)[ok])
        want_dy = np.sqrt(counts) / expo
        worst = np.max((np.abs(dy - want_dy) / np.where(want_dy > 0, want_dy, 1.0))[ok]) / EPS
        print("%s: dy within %.2f ulp of sqrt(counts) / exposure" % (name, worst))
        assert worst <= 2.0
        if name == "knuth-2":
            assert negative.sum() >= 5 and np.all(lam[~negative] < 10)
        elif name == "ptrs-25":
            assert np.all(lam >= 10)
        else:
            assert np.mean(lam < 10) > 0.2 and np.mean(lam >= 10) > 0.2
    assert _same(block["rates"], rates[7:]) and _same(block["dy"], dy[7:])


# ---- (b) Gaussian noise ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base", [0, 3])
def test_gaussian_noise_is_sigma_times_the_replayed_normal(base):
    """rates - clean = sigma g1 of block (epoch, 10, series + base, 0), within 4 ulp of |clean| + |sigma g1| (one rounding
    of the sum or the fma, the device's log and sincospi against R_draw); dy = sigma exactly"""
    S, N, sigma, seed = 5, 50, 2.5, 0xFEED5EED77
    kernel = DampedRandomWalk(np.log(4.0), np.log(0.3), bounds=[(-10, 50), (-10, 10)])
    sim = Simulator(kernel, np.arange(0.5, N, 1.0), 0.5, 50.0, "Gaussian", sigma_noise=sigma, extension_factor=2, random_state=5)
    out = sim.simulate(np.tile(kernel.get_parameter_vector(), (S, 1)), seed=seed, want_clean=True, index_base=base)
    assert out["rates"].shape == (S, N) and np.all(out["dy"] == sigma)
    want = sigma * sr.gaussian_noise(np.arange(N)[None, :], base + np.arange(S)[:, None], seed)
    got = np.asarray(out["rates"].astype(np.longdouble) - out["clean"].astype(np.longdouble), dtype=np.float64)
    scale = np.abs(out["clean"]) + np.abs(want)
    worst = np.max(np.abs(got - want) / scale) / EPS
    print("Gaussian noise, base %d: within %.2f ulp of |clean| + |sigma g1| (R_draw of the normals: %.2f)" % (base, worst, sr.R_NORMAL))
    assert worst <= 4.0
    assert 1.5 < np.std(got) < 3.5


# ---- engine-level set-up for (c) and (d): N = seg_len epochs, one-sample windows ---------------------------------------
def _bind(engine, kinds, n_epochs):
    t = np.arange(n_epochs, dtype=np.float64)
    y = np.zeros((1, n_epochs))
    engine.set_lightcurves(t, y, np.ones((1, n_epochs)), y_offset=[0.0])
    full, free, bounds = synth.model_spec(kinds, y, per_lc_mean=True)
    engine.set_model(kinds, full, free, bounds)


def _reset(engine):
    engine.set_simulate_pdf(0)
    engine.set_stream_base(0)
    engine.set_simulate_draws(None, None)


# ---- (c) E13's own draws ---------------------------------------------------------------------------------------------
E13_DT = 0.5
E13_CASES = [(kind, seg_len, S, base) for kind in (1, 2) for seg_len in (37, 64, 1500) for S, base in ((1, 0), (5, 11))] + \
    [(1, 64, 300, 0), (2, 64, 300, 0)]
E13_RESEED = {(2, 1500, 5, 11): 5}      # the first seed of this case meets a tie on the host (4.7e-10): the sixth does not
E13_RESEED = {(2, 1500, 5, 11): 5}      # the first seed of this case meets a tie on the host (4.7e-10): the sixth does not


@pytest.mark.parametrize("kind,seg_len,S,base", E13_CASES)
def test_e13_draws_and_final_order_are_the_replays(engine, kind, seg_len, S, base):
    """mtg_e13_std_kernel + mtg_e13_draw_kernel + the rank loop, sample by sample (one-sample windows on a power-of-two
    sim_dt): with the same seed, pdf = 0 returns the TK95 segments and pdf = 1 / 2 the adjusted series.  The adjusted
    series is a permutation of the replayed draws e13_draws(kind, mean, np.std(segment), ...) -- sorted, they agree within
    8 x R_draw (lognormal) or 4 ulp (uniform) -- in the order the host loop started from those draws ends on.
    37: odd (a dropped second element) and below one workgroup of the std kernel; 1500: above 1024, not a multiple of it;
    S = 300 at 64: chunks of 256 and 44, s0 > 0 and zero-filled slots (permutation and convergence only)."""
    mean = 25.0 if kind == 1 else 100.0          # (the uniform kind's support stays away from 0, where a relative bound means nothing)
    nfft = 128 if seg_len <= 64 else 4096
    seed = 0xE13000 + 1000 * kind + seg_len + 100000 * E13_RESEED.get((kind, seg_len, S, base), 0)
    thetas = np.array([np.log(100.0), np.log(1.5)])[None, :] + 0.03 * (np.arange(S) % 7)[:, None] * np.array([1.0, -1.0])
    lo = np.arange(seg_len, dtype=np.int32)
    _bind(engine, [synth.K_DRW], seg_len)
    try:
        engine.set_stream_base(base)
        engine.set_simulate_pdf(0)
        plain = engine.simulate_tk95(thetas, seed, nfft, E13_DT, mean, seg_len, lo, lo + 1, want_segments=True)
        engine.set_simulate_pdf(kind, 400)
        shaped = engine.simulate_tk95(thetas, seed, nfft, E13_DT, mean, seg_len, lo, lo + 1, want_segments=True)
        report = engine.simulate_pdf_report()
    finally:
        _reset(engine)
    segments, rates = plain["segments"], shaped["rates"]
    assert np.array_equal(shaped["segments"], segments) and rates.shape == (S, seg_len)
    assert report["not_converged"] == 0 and 1 <= report["iterations"] <= 401
    std = np.std(segments, axis=1)
    assert kind == 2 or (np.all(std / mean > 0.2) and np.all(std / mean < 1.0))          # the range R_draw was measured over
    draws, expo = sr.e13_draws(kind, mean, std, seg_len, base + np.arange(S), seed, with_exponent=True)
    order = np.argsort(draws, axis=1, kind="stable")
    want = np.take_along_axis(draws, order, axis=1)
    bound = 8.0 * sr.r_draw(np.take_along_axis(expo, order, axis=1)) if kind == 1 else np.full(want.shape, 4.0)
    err = np.abs(np.sort(rates, axis=1) - want) / np.abs(want) / EPS
    print("E13 kind %d, n = %d, S = %d, base %d: sorted series within %.2f ulp of the replayed draws (%.2f of the bound), %d iterations"
          % (kind, seg_len, S, base, err.max(), np.max(err / bound), report["iterations"]))
    assert np.all(err <= bound)
    if S > 5:
        return
    for s in range(S):
        host, closest = sr.e13_host_loop(segments[s], draws[s])
        assert closest >= 1e-9, "series %d meets a tie on the host (%.2e): the seed is to be changed" % (s, closest)
        assert np.array_equal(np.argsort(rates[s], kind="stable"), np.argsort(host, kind="stable")), s


# ---- (d) the spectrum, term by term ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(sr.PSD_MODELS))
def test_model_spectrum_line_by_line(engine, name):
    """mtg_psd with nr = nr0 + 2 sig, nc = nc0 - sig: a single real 1 at line k of the caller's normals, every start 0,
    seg_len = nfft = 64; the first sample of the series over the same sample of a call with a table of ones is
    sqrt(psd(w_k)) -- the ratio removes every normalisation -- within 8 R_psd + 8 ulp of the spectrum at 40 digits.
    Six rows of theta times the lines 1 .. 32 (Nyquist included) in one batch: SHO rows on both sides of Q = 1 / 2."""
    kinds, rows = sr.PSD_MODELS[name]
    nfft, dt, nk = sr.PSD_NFFT, sr.PSD_DT, sr.PSD_NFFT // 2 + 1
    lines = np.arange(1, nk)
    theta, ks = np.repeat(rows, len(lines), axis=0), np.tile(lines, len(rows))
    S = len(ks)
    normals = np.zeros((S, 2, nk))
    normals[np.arange(S), 0, ks] = 1.0
    lo = np.arange(nfft, dtype=np.int32)
    _bind(engine, kinds, nfft)
    try:
        engine.set_simulate_draws(normals, np.zeros(S, dtype=np.int64))
        model = engine.simulate_tk95(theta, 1, nfft, dt, 0.0, nfft, lo, lo + 1, want_segments=True)
        engine.set_simulate_draws(normals, np.zeros(S, dtype=np.int64))
        table = engine.simulate_tk95(S, 1, nfft, dt, 0.0, nfft, lo, lo + 1, want_segments=True, psd_table=np.ones((1, nk)))
    finally:
        _reset(engine)
    ratio = model["segments"][:, 0] / table["segments"][:, 0]
    w = sr.grid_omega(lines, nfft, dt)
    with sr.mpmath.workdps(sr.DIGITS):
        truth = [sr.mpmath.sqrt(p) for row in rows for p in sr.psd(kinds, row, w)]
    err = sr.rel_ulps(ratio, truth)
    bound = 8.0 * sr.r_psd(name) + 8.0
    print("spectrum %s: sqrt(psd) within %.3g ulp (R_psd %.3g, bound %.3g); per row %s"
          % (name, err.max(), sr.r_psd(name), bound, " ".join("%.3g" % v for v in err.reshape(len(rows), -1).max(axis=1))))
    assert np.all(err <= bound)
    if sr.K_SHO in kinds:
        assert {sr.signature(kinds, row) for row in rows} == {0, 1}


def test_nyquist_line_is_real(engine):
    """the imaginary part of the Nyquist line is forced to 0: a single 1 in that slot leaves the series at the mean"""
    kinds, rows = sr.PSD_MODELS["drw"]
    nfft, nk = sr.PSD_NFFT, sr.PSD_NFFT // 2 + 1
    normals = np.zeros((len(rows), 2, nk))
    normals[:, 1, nk - 1] = 1.0
    lo = np.arange(nfft, dtype=np.int32)
    _bind(engine, kinds, nfft)
    try:
        engine.set_simulate_draws(normals, np.zeros(len(rows), dtype=np.int64))
        out = engine.simulate_tk95(rows, 1, nfft, sr.PSD_DT, 3.0, nfft, lo, lo + 1, want_segments=True)
        normals[:, 1, nk - 2] = 1.0            # ... and the line below it is not
        engine.set_simulate_draws(normals, np.zeros(len(rows), dtype=np.int64))
        other = engine.simulate_tk95(rows, 1, nfft, sr.PSD_DT, 3.0, nfft, lo, lo + 1, want_segments=True)
    finally:
        _reset(engine)
    assert np.all(out["segments"] == 3.0) and np.all(out["rates"] == 3.0)
    assert np.all(np.std(other["segments"], axis=1) > 0)


# ---- (e) more than one chunk on the plain path -------------------------------------------------------------------------
def _chunk_simulator(transform):
    kernel = DampedRandomWalk(np.log(4.0), np.log(0.3), bounds=[(-10, 50), (-10, 10)])
    sim = Simulator(kernel, np.arange(0.5, 32, 1.0), 0.5, 10.0, "Gaussian", sigma_noise=1.0, extension_factor=1, random_state=1,
                    transform=transform)
    assert sim.fftndatapoints == 126          # 2 x 3^2 x 7: a native length; 256 series per execution of its plan
    return sim, kernel.get_parameter_vector()


def test_second_chunk_and_short_last_chunk_on_the_library_path():
    """S = 300 goes through the plan as 256 + 44 (s0 > 0, zero-filled slots): series 0 .. 255 are a call of 256, series
    256 .. 299 a call of 44 with index_base = 256, bit for bit"""
    sim, th = _chunk_simulator("library")
    thetas = th[None, :] + 0.01 * (np.arange(300) % 11)[:, None]
    whole = sim.simulate(thetas, noise=False, seed=2024, index_base=0)["rates"]
    first = sim.simulate(thetas[:256], noise=False, seed=2024, index_base=0)["rates"]
    last = sim.simulate(thetas[256:], noise=False, seed=2024, index_base=256)["rates"]
    assert whole.shape == (300, 32) and np.all(np.isfinite(whole)) and np.std(whole) > 0.5
    assert np.array_equal(whole[:256], first) and np.array_equal(whole[256:], last)
    assert not np.array_equal(whole[256:], sim.simulate(thetas[256:], noise=False, seed=2024, index_base=0)["rates"])


def test_odd_last_pair_on_the_chirp_z_path():
    """the same on the forced chirp-z path with S = 259 -- a last chunk of three series, a pair and a lone one: equal to
    the calls of its parts with pairing off, and within 1e-12 of the scatter with it on"""
    sim, th = _chunk_simulator("chirp-z")
    thetas = th[None, :] + 0.01 * (np.arange(259) % 11)[:, None]
    run = lambda rows, base, pairs: sim.simulate(rows, noise=False, seed=2025, index_base=base, pair_series=pairs)["rates"]
    single = run(thetas, 0, False)
    assert np.array_equal(single[:256], run(thetas[:256], 0, False)) and np.array_equal(single[256:], run(thetas[256:], 256, False))
    paired = run(thetas, 0, True)
    scale = np.std(single)
    assert scale > 0.5
    worst = np.max(np.abs(paired - single)) / scale
    print("chirp-z, S = 259: paired against single transforms %.3g of the scatter" % worst)
    assert worst <= 1e-12
    parts = np.vstack([run(thetas[:256], 0, True), run(thetas[256:], 256, True)])
    assert np.max(np.abs(parts - single)) <= 1e-12 * scale
    library = _chunk_simulator("library")[0].simulate(thetas, noise=False, seed=2025, index_base=0)["rates"]
    assert np.max(np.abs(library - single)) <= 1e-11 * scale
