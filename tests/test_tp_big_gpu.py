"""GPU parity of the rank-10 time-parallel path (csrc/mtg_tp_big.h, mtg_tp_scan.h): composition by
two waves per 64 chunks, scan with one wave per combination, likelihood with and without the filter
pass, every chunk count the dispatch can pick, the large-phase reduction, the fall-back of badly
cancelling evaluations -- against the oracle (celerite's algorithm on the CPU) and against the serial
sweep of the same library.  BASELINE configs[4] (N = 200 000, five SHO terms, 512 walkers) at its full
batch of 256 evaluations, directly and through the device-resident sampler."""
import numpy as np
import pytest

import philox_replay
from mind_the_gaps_amd import synthetic as synth
from oracle import celerite as oracle_c

pytestmark = pytest.mark.gpu

FIVE = [synth.K_SHO] * 5


def config5_theta():
    th = synth.truth(FIVE)
    for i in range(5):
        th[3 * i:3 * i + 3] = [np.log(20.0 + 10 * i), np.log([3.0, 8.0, 10.0, 1.0, 0.8][i]), np.log(2 * np.pi / (5.0 + 6 * i))]
    return th


def setup(engine, N, L=1, seed=7):
    t, y, dy = synth.make_lightcurves(N, L, seed=seed)
    full, free, bounds = synth.model_spec(FIVE, y, per_lc_mean=True)
    y_mean = y.mean(axis=1)
    engine.set_lightcurves(t, y, dy + 1e-12, y_offset=y_mean)
    engine.set_model(FIVE, full, free, bounds)
    return t, y, dy, y_mean, bounds


def oracle(t, y, dy, y_mean, bounds, theta, lc=None, add_prior=True):
    lc = np.zeros(len(theta), dtype=np.int32) if lc is None else lc
    return oracle_c.logprob_batch(t, y, dy, FIVE, np.hstack([theta, y_mean[lc][:, None]]), bounds=bounds, lc_index=lc,
                                  add_prior=add_prior, nthreads=8)


def rel(a, b):
    return float(np.max(np.abs(a - b) / np.abs(b)))


@pytest.mark.parametrize("N", [1030, 5000, 20011])
def test_direct_and_filter_pass_agree_with_the_oracle(engine, N):
    """All six signatures (0 .. 5 over-damped oscillators) in one batch; lnL from the composition + scan
    alone (default) and from the filter pass; statuses as the oracle's."""
    L, B = 2, 24
    t, y, dy, y_mean, bounds = setup(engine, N, L, seed=300 + N)
    theta = synth.draw_thetas(FIVE, B, seed=31)
    for b in range(B):
        for k in range(b % 6):
            theta[b, 3 * k + 1] = np.log(0.1 + 0.05 * k)
    theta[5, 0] = 60.0                                        # outside the prior box
    lc = (np.arange(B) % L).astype(np.int32)
    ref, rst = oracle(t, y, dy, y_mean, bounds, theta, lc)
    try:
        engine.set_time_parallel(1)
        engine.set_tp_direct(1)
        out_d, st_d = engine.loglike(theta, lc, add_prior=True)
        engine.set_tp_direct(0)
        out_f, st_f = engine.loglike(theta, lc, add_prior=True)
    finally:
        engine.set_tp_direct(1)
        engine.set_time_parallel(2)
    assert np.array_equal(st_d, rst) and np.array_equal(st_f, rst)
    ok = rst == 0
    assert ok.sum() == B - 1
    assert rel(out_d[ok], ref[ok]) <= 1e-8 and rel(out_f[ok], ref[ok]) <= 1e-8
    assert rel(out_d[ok], out_f[ok]) <= 1e-11


def test_result_does_not_depend_on_the_chunk_count(engine):
    """The dispatch cuts the light curve into 64 .. 4096 chunks depending on the batch (and the scan into
    groups of 4 or 16): the same evaluation in batches of every size."""
    N = 120000
    t, y, dy, y_mean, bounds = setup(engine, N, 1, seed=11)
    th = synth.draw_thetas(FIVE, 3, seed=2)
    th[1, 4] = np.log(0.3)                                    # one over-damped oscillator
    ref, rst = oracle(t, y, dy, y_mean, bounds, th)
    assert np.all(rst == 0)
    try:
        engine.set_time_parallel(1)
        for B in (3, 20, 70, 300, 1100):
            theta = np.tile(th, ((B + 2) // 3, 1))[:B]
            out, st = engine.loglike(theta, add_prior=True)
            assert np.all(st == 0)
            assert rel(out, np.tile(ref, (B + 2) // 3)[:B]) <= 1e-8, B
            if B > 3:
                assert np.array_equal(out[:B - 3], out[3:]), B          # copies of one row agree exactly
    finally:
        engine.set_time_parallel(2)


def test_large_phase_increments(engine):
    """d * max(dx) beyond the exact range of the table reduction (1e5): the two-part reduction modulo
    2 pi in front of the table path (tpb_transition, fast = false)."""
    N, B = 6000, 8
    t, y, dy, y_mean, bounds = setup(engine, N, 1, seed=5)
    assert np.max(np.diff(t)) > 90.0
    theta = synth.draw_thetas(FIVE, B, seed=4)
    theta[:, 2] = np.log(3000.0) + 0.1 * np.arange(B)         # omega0 ~ 3000 / day x 100-day gaps
    theta[:, 1] = np.log(5.0)
    ref, rst = oracle(t, y, dy, y_mean, bounds, theta)
    assert np.all(rst == 0)
    try:
        engine.set_time_parallel(1)
        out, st = engine.loglike(theta, add_prior=True)
        engine.set_tp_direct(0)
        out_f, st_f = engine.loglike(theta, add_prior=True)
        engine.set_time_parallel(0)
        thr, st_t = engine.loglike(theta, add_prior=True)
    finally:
        engine.set_tp_direct(1)
        engine.set_time_parallel(2)
    assert np.all(st == 0) and np.all(st_f == 0) and np.all(st_t == 0)
    # celerite evaluates cos/sin at the absolute times: at phases of ~1e9 rad its own rounding is ~1e-7
    assert rel(out, ref) <= 1e-6 and rel(out_f, ref) <= 1e-6
    assert rel(out, thr) <= 1e-8 and rel(out, out_f) <= 1e-10


def test_extreme_parameters(engine):
    """Amplitudes of e^40 against unit noise and oscillators of Q = 8000 (memory far longer than a
    chunk): the likelihood without the filter pass stays as close to the filter pass as the filter pass
    is to the serial sweep (the problem's own conditioning, ~1e-11 here)."""
    N, B = 9001, 12
    t, y, dy, y_mean, bounds = setup(engine, N, 1, seed=8)
    theta = synth.draw_thetas(FIVE, B, seed=6)
    theta[::3, 0] = 40.0
    theta[1::3, 4] = 9.0
    theta[1::3, 3] = 8.0
    try:
        engine.set_time_parallel(1)
        engine.set_tp_direct(1)
        out_d, st_d = engine.loglike(theta, add_prior=False)
        engine.set_tp_direct(0)
        out_f, st_f = engine.loglike(theta, add_prior=False)
        engine.set_time_parallel(0)
        thr, st_t = engine.loglike(theta, add_prior=False)
    finally:
        engine.set_tp_direct(1)
        engine.set_time_parallel(2)
    assert np.array_equal(st_d, st_f) and np.array_equal(st_d, st_t) and np.all(st_d == 0)
    assert rel(out_d, out_f) <= 1e-9 and rel(out_d, thr) <= 1e-9


def test_rows_that_are_not_positive_definite(engine):
    """Five four-parameter ComplexTerms (the (0, 5) structure) with the prior off: rows whose b is far
    too large for a positive definite covariance.  Anything not positive on the way sends the row
    through the filter pass, whose pivots are celerite's: same statuses and values as the oracle."""
    kinds = [synth.K_COMPLEX4] * 5
    N, B = 3000, 16
    t, y, dy = synth.make_lightcurves(N, 1, seed=21)
    full, free, bounds = synth.model_spec(kinds, y, per_lc_mean=True)
    y_mean = y.mean(axis=1)
    engine.set_lightcurves(t, y, dy + 1e-12, y_offset=y_mean)
    engine.set_model(kinds, full, free, bounds)
    theta = synth.draw_thetas(kinds, B, seed=3)
    theta[::2, 1] += 6.0                                      # log_b of the first term: b >> a c / d
    ref, rst = oracle_c.logprob_batch(t, y, dy, kinds, np.hstack([theta, np.full((B, 1), y_mean[0])]), bounds=bounds,
                                      add_prior=False, nthreads=8)
    assert (rst == 2).sum() >= 4 and (rst == 0).sum() >= 4
    try:
        engine.set_time_parallel(1)
        out, st = engine.loglike(theta, add_prior=False)
    finally:
        engine.set_time_parallel(2)
    assert np.array_equal(st, rst)
    ok = rst == 0
    assert np.all(np.isneginf(out[~ok])) and rel(out[ok], ref[ok]) <= 1e-8


def test_config5_full_half_step(engine):
    """BASELINE configs[4] at the size of its ensemble half-step: 256 evaluations of N = 200 000, J = 10,
    time-parallel (default dispatch) and serial sweep against the oracle."""
    N, B = 200000, 256
    t, y, dy = synth.make_lightcurves(N, 1, seed=20250709)
    th = config5_theta()
    rng = np.random.default_rng(5)
    theta = th + 0.05 * np.abs(th) * rng.standard_normal((B, len(th)))
    theta[::17, 4] = np.log(0.3)                                       # a second signature in the batch
    full = np.concatenate([th, [0.0]])
    bounds = np.vstack([synth.bounds_for(FIVE), [(-np.inf, np.inf)]])
    engine.set_lightcurves(t, y, dy + 1e-12, y_offset=y.mean(axis=1))
    engine.set_model(FIVE, full, np.arange(15, dtype=np.int32), bounds)
    ref, rst = oracle_c.logprob_batch(t, y[0], dy[0], FIVE, np.hstack([theta, np.full((B, 1), y.mean())]),
                                      bounds=bounds, add_prior=True, nthreads=8)
    assert np.all(rst == 0)
    out, st = engine.loglike(theta, add_prior=True)                    # automatic dispatch: time-parallel
    assert engine.last_kernel_ms < 20.0                                # (the serial sweep takes ~200 ms)
    try:
        engine.set_time_parallel(0)
        thr, st_t = engine.loglike(theta, add_prior=True)
    finally:
        engine.set_time_parallel(2)
    assert np.array_equal(st, rst) and np.array_equal(st_t, rst)
    assert rel(out, ref) < 1e-8 and rel(thr, ref) < 1e-8


def test_config5_device_sampler_replays_on_the_host(engine):
    """configs[4] through the device-resident sampler: 512 walkers, one light curve of 200 000 samples;
    the chain replayed on the host with the oracle likelihood takes the same decisions."""
    N, W, steps, seed = 200000, 512, 2, 0x5EED5EED
    t, y, dy = synth.make_lightcurves(N, 1, seed=20250709)
    th = config5_theta()
    bounds = np.vstack([synth.bounds_for(FIVE), [(-np.inf, np.inf)]])
    engine.set_lightcurves(t, y, dy + 1e-12, y_offset=y.mean(axis=1))
    engine.set_model(FIVE, np.concatenate([th, [0.0]]), np.arange(15, dtype=np.int32), bounds)
    rng = np.random.default_rng(12)
    p0 = (th * (1 + 0.01 * rng.standard_normal((1, W, 15))))

    def oracle_lnp(q, ens):
        return oracle_c.logprob_batch(t, y[0], dy[0], FIVE, np.hstack([q, np.full((len(q), 1), y.mean())]),
                                      bounds=bounds, add_prior=True, nthreads=8)[0]

    engine.ensemble_init(p0, seed=seed)
    st0 = engine.ensemble_state()
    lnp0 = oracle_lnp(p0.reshape(W, -1), np.zeros(W, dtype=int)).reshape(1, W)
    assert rel(st0["log_prob"], lnp0) < 1e-9
    chain, lnp_chain = engine.ensemble_run(steps, store_chain=True)
    ref_chain, ref_lnp, ref_acc = philox_replay.run(p0, lnp0, oracle_lnp, steps, seed)
    assert np.allclose(chain, ref_chain, rtol=0, atol=1e-10)
    assert np.allclose(lnp_chain, ref_lnp, rtol=1e-9)
    assert np.array_equal(engine.ensemble_state()["naccept"], ref_acc)
