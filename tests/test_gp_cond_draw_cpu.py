"""CPU tests of the conditional draw (mtg_gp_cond_draw): the host replay tests/gp_cond_draw_replay.py against the dense
Matheron formula in numpy, the merge and the normals' layout, the fixed seed of the device's distribution test, and the
public signatures.  tests/test_gp_cond_draw_gpu.py takes its cases from here.

The replay (the factorisation on the merged series, then predict_at_replay) and the dense route (np.linalg.cholesky of the
merged covariance, np.linalg.solve with K) are two float64 evaluations of the same affine map of the normals; each is
allowed the floor 64 sqrt(N + M) u s of tests/test_gp_draw_gpu.py, s the sum of the magnitudes that enter a value
(gp_cond_draw_replay.dense_draw), so their difference is held to twice that."""
import inspect

import numpy as np
import pytest

import gp_cond_draw_replay as CR
from mind_the_gaps_amd import synthetic as synth
from oracle import dense

U = 2.0 ** -53
# 3: one real + one complex term; 6: two real + two complex (the device counts a Lorentzian's (0, 0) real term out: the
# alternative model of the Protassov test is rank 5 there)
RANKS = {1: [synth.K_DRW], 3: synth.NULL_MODEL, 6: [synth.K_REAL, synth.K_DRW, synth.K_SHO, synth.K_COMPLEX4]}


def small_case(rank):
    """N = 12 irregular epochs with unequal error bars, M = 7 new times: before the first epoch, after the last, on an
    epoch, a duplicated pair, and two inside gaps; given out of order"""
    kinds = RANKS[rank]
    theta = synth.truth(kinds)
    t, y, dy = synth.make_lightcurves(12, 1, seed=1200 + rank)
    g = 0.5 * (t[3] + t[4])
    ts = np.array([g, t[-1] + 5.0, t[5], 0.25 * t[7] + 0.75 * t[8], t[0] - 3.0, g, 0.5 * (t[9] + t[10])])
    return kinds, theta, t, y[0], dy[0], ts, dense.build_coeffs(kinds, theta)


def floor(N, M):
    return 64.0 * np.sqrt(N + M) * U


def test_merge_puts_a_new_time_after_its_epoch_and_keeps_the_first_of_a_pair():
    kinds, theta, t, y, dy, ts, coeffs = small_case(1)
    tu, first, inv, order, is_new = CR.merge(t, ts)
    assert len(tu) == 6 and np.array_equal(tu[inv], ts)
    assert list(first) == [4, 0, 2, 3, 6, 1]                      # the pair (entries 0 and 5): entry 0
    tm = np.concatenate([t, tu])[order]
    assert np.all(np.diff(tm) >= 0.0) and is_new[0] and is_new[-1]
    k = int(np.flatnonzero(is_new & (tm == t[5]))[0])
    assert not is_new[k - 1] and tm[k - 1] == t[5]                # the epoch first, then the new time equal to it
    q = np.arange(12 + 7, dtype=np.float64)
    assert np.array_equal(CR.merged_normals(q, 12, first, order)[0][is_new], 12.0 + first)


@pytest.mark.parametrize("rank", sorted(RANKS))
def test_replay_is_the_dense_matheron_formula(rank):
    kinds, theta, t, y, dy, ts, coeffs = small_case(rank)
    N, M = len(t), len(ts)
    mean = lambda x: np.full(len(x), 100.0)
    q = np.random.default_rng(rank).standard_normal((3, N + M))
    q[0] = 0.0                                                    # the conditional mean itself
    want, s = CR.dense_draw(t, y, dy + 1e-12, coeffs, mean, ts, q)
    for b in range(3):
        got = CR.draw(t, y, dy + 1e-12, coeffs, mean, ts, q[b])
        e = np.abs(got - want[b]) / s[b]
        print("\ngp-cond-draw replay rank %d row %d: worst |replay - dense| / s = %.3g (allowed %.3g)" % (rank, b, e.max(), 2.0 * floor(N, M)))
        assert np.all(e <= 2.0 * floor(N, M))
        assert got[0] == got[5]                                   # the duplicated pair
    # the other entry of a pair is not read
    q2 = q[1].copy()
    q2[N + 5] = 1e6
    assert np.array_equal(CR.draw(t, y, dy + 1e-12, coeffs, mean, ts, q2), CR.draw(t, y, dy + 1e-12, coeffs, mean, ts, q[1]))


def test_device_normals_depend_on_the_set_of_new_times_only():
    ts = np.array([3.0, 1.0, 3.0, 2.0, 7.5])
    q, rad = CR.device_normals(9, 4, 10, ts)
    p = np.array([4, 2, 0, 3, 1])
    q2, _ = CR.device_normals(9, 4, 10, ts[p])
    assert np.array_equal(q2[:10], q[:10]) and np.array_equal(q2[10:], q[10:][p]) and q[10] == q[12]
    assert not np.array_equal(CR.device_normals(9, 5, 10, ts)[0], q) and np.all(rad >= np.abs(q))
    # the epochs' normals and the new times' come from different counter words
    assert not np.array_equal(CR.philox_normals(9, 4, 4, CR.PURPOSE_EPOCH)[0], CR.philox_normals(9, 4, 4, CR.PURPOSE_NEW)[0])


DIST_SEED = 20250131


def distribution_case():
    """N = 64, M = 32 new times spread over the light curve and beyond both ends, the rank-3 model"""
    kinds = RANKS[3]
    theta = synth.truth(kinds)
    t, y, dy = synth.make_lightcurves(64, 1, seed=64)
    ts = np.linspace(t[0] - 5.0, t[-1] + 5.0, 32)
    return kinds, theta, t, y[0], dy[0], ts


def check_distribution(draws, mu, var):
    """draws [B][M] against the conditional mean and variance: 5 standard errors of the sample mean and variance"""
    B = len(draws)
    sd = np.sqrt(var)
    em = np.abs(draws.mean(axis=0) - mu) / (5.0 * sd / np.sqrt(B))
    ev = np.abs(draws.var(axis=0, ddof=1) - var) / (5.0 * var * np.sqrt(2.0 / (B - 1)))
    print("\ngp-cond-draw distribution of %d draws: mean at %.3g, variance at %.3g of 5 standard errors" % (B, em.max(), ev.max()))
    assert np.all(em <= 1.0) and np.all(ev <= 1.0)


def test_the_fixed_seed_passes_the_distribution_test_on_the_host():
    """what tests/test_gp_cond_draw_gpu.py asks of 4096 device draws, asked first of the replayed Philox normals pushed
    through the dense Matheron formula"""
    kinds, theta, t, y, dy, ts = distribution_case()
    coeffs = dense.build_coeffs(kinds, theta)
    mean = lambda x: np.full(len(x), float(np.mean(y)))
    q = np.array([CR.device_normals(DIST_SEED, g, len(t), ts)[0] for g in range(4096)])
    draws, _ = CR.dense_draw(t, y, dy + 1e-12, coeffs, mean, ts, q)
    mu, _ = CR.dense_draw(t, y, dy + 1e-12, coeffs, mean, ts, np.zeros(len(t) + len(ts)))
    cov, _ = CR.cond_cov(t, dy + 1e-12, coeffs, ts)
    check_distribution(draws, mu, np.diag(cov))


def test_public_signatures():
    from mind_the_gaps_amd.engine import EXPORTS, Engine
    from mind_the_gaps_amd.gp import GP
    from mind_the_gaps_amd.gpmodelling import GPModelling
    from mind_the_gaps_amd.lightcurves import GappyLightcurve
    from mind_the_gaps_amd.models import DampedRandomWalk
    assert "mtg_gp_cond_draw" in EXPORTS
    p = inspect.signature(Engine.gp_cond_draw).parameters
    assert list(p) == ["self", "theta", "ts", "lc_index", "seed", "normals"]
    assert p["lc_index"].default is None and p["seed"].default == 0 and p["normals"].default is None
    p = inspect.signature(GP.sample_conditional).parameters             # celerite's, and the seed of GP.sample
    assert list(p) == ["self", "y", "t", "size", "seed"] and all(p[k].default is None for k in ("t", "size", "seed"))
    p = inspect.signature(GPModelling.sample_conditional).parameters
    assert list(p) == ["self", "times", "nsims", "parameters", "seed"] and p["nsims"].default == 1
    lc = GappyLightcurve(np.arange(100.0), np.arange(100.0), np.ones(100))
    model = GPModelling(lc, DampedRandomWalk(5.0, 1.0, bounds=[(0.0, 10.0), (-5.0, 5.0)]))
    with pytest.raises(RuntimeError):                                   # no posteriors to draw parameters from
        model.sample_conditional(nsims=4)
