"""The seven host-pointer entries that evaluate rows of theta -- Engine.loglike, loglike_coeffs, predict, predict_at,
gp_draw, loglike_grad, apply_inverse -- stage their inputs through one call object (RowCall in csrc/mtg_capi.hip) and
the context's staging buffers.  What such a shared stager gets wrong is state the previous entry left in the context:
a light-curve index picked up for a call that gave none, a status or a theta of a longer batch, a buffer that was not
grown.  So one engine runs the seven entries in two different interleavings, over batches of 37, 5 and 130 rows (the
staging grows, and is reused while larger than needed) that alternate between a mixed lc_index and none, and every
result must equal bit for bit the same call made FIRST on a fresh engine; for the calls without an index every row
must also equal what an explicit index of zeros gives.

N = 257 samples (past four checkpoints of 64 and eight tiles of 32, each with a tail of one), L = 3 light curves with
times of their own, DRW + SHO with rows on either side of Q = 1/2 and one row outside the prior, whose status a stale
buffer would hide.  A few seconds in all.
"""
import numpy as np
import pytest

from mind_the_gaps_amd import engine as E

pytestmark = pytest.mark.gpu

N, L, M = 257, 3, 9
SIZES = (37, 5, 130)
ENTRIES = ("loglike", "loglike_coeffs", "predict", "predict_at", "gp_draw", "loglike_grad", "apply_inverse")
REJECTED = 3   # the row outside the prior in every batch


def lightcurves():
    rng = np.random.default_rng(20261019)
    t = 50.0 + np.cumsum(rng.uniform(0.3, 1.7, (L, N)), axis=1)
    return t, 10.0 + rng.standard_normal((L, N)), rng.uniform(0.1, 0.3, (L, N))


def fresh_engine():
    t, y, dy = lightcurves()
    eng = E.Engine(0)
    eng.set_lightcurves(t, y, dy + 1e-12, y_offset=y.mean(axis=1))
    # log a, log c | log S0, log Q, log w0; the mean a frozen 0
    base = np.array([-0.5, -1.5, 0.2, np.log(2.0), np.log(0.8)])
    bounds = np.vstack([np.tile([-10.0, 10.0], (5, 1)), [[-np.inf, np.inf]]])
    eng.set_model([E.TERM_DRW, E.TERM_SHO], np.concatenate([base, [0.0]]), np.arange(5, dtype=np.int32), bounds)
    return eng, base


def inputs(base, B):
    """theta [B][5] (every third row over-damped, row REJECTED outside the prior), a mixed lc_index, raw coefficients"""
    rng = np.random.default_rng(B)
    theta = np.tile(base, (B, 1)) + 0.05 * rng.uniform(-1.0, 1.0, (B, len(base)))
    theta[2::3, 3] = np.log(0.3)
    theta[REJECTED, 0] = 11.0
    lc = rng.integers(0, L, B).astype(np.int32)
    lc[:3] = (2, 0, 1)
    coeffs = [np.exp(rng.normal(m, 0.3, (B, 1))) for m in (0.0, -1.0, -0.5, -1.5, -1.0, 0.0)]   # a, c | a, b, c, d
    coeffs[3] *= 0.1
    return theta, lc, coeffs


def call(eng, base, entry, B, indexed, zeros=False):
    """one entry on a batch of B rows -> tuple of arrays; indexed: the mixed lc_index, else none (zeros: all 0 instead)"""
    theta, lc, coeffs = inputs(base, B)
    lc = lc if indexed else (np.zeros(B, dtype=np.int32) if zeros else None)
    if entry == "loglike":
        return eng.loglike(theta, lc)
    if entry == "loglike_coeffs":
        return eng.loglike_coeffs(*coeffs, jitter=np.full(B, 0.01), lc_index=lc)
    if entry == "predict":
        return eng.predict(theta, lc)
    if entry == "predict_at":
        ts = 50.0 + np.random.default_rng(7).uniform(-5.0, 270.0, M)
        return eng.predict_at(theta, ts, lc)
    if entry == "gp_draw":
        return eng.gp_draw(theta, lc, seed=99)
    if entry == "loglike_grad":
        return eng.loglike_grad(theta, lc, add_prior=True)
    rhs = np.random.default_rng(B + 1).standard_normal((N, 3))   # one row: the first of the batch (never the rejected one)
    x, status = eng.apply_inverse(theta[0], rhs, lc_index=int(lc[0]) if indexed else 0)
    return x, np.int32(status)


@pytest.fixture(scope="module")
def first_calls():
    """(entry, B, indexed, zeros) -> the call's results as the first call of a fresh engine, made once"""
    made = {}

    def get(entry, B, indexed, zeros=False):
        key = (entry, B, indexed, zeros)
        if key not in made:
            eng, base = fresh_engine()
            try:
                made[key] = call(eng, base, entry, B, indexed, zeros)
            finally:
                eng.close()
        return made[key]
    return get


def same(got, want):
    return len(got) == len(want) and all(np.array_equal(np.asarray(g), np.asarray(w), equal_nan=True) for g, w in zip(got, want))


# call i of an interleaving takes entry order[i % 7], SIZES[(i + shift) % 3] rows and an index when (i + shift) is even:
# 7 is coprime to 3 and to 2, so over 21 calls every entry meets every size, and runs both with and without an index
@pytest.mark.parametrize("order, shift", [(ENTRIES, 0), (ENTRIES[::-1], 1)], ids=["forward", "backward"])
def test_an_entry_sees_nothing_of_the_entry_before(first_calls, order, shift):
    eng, base = fresh_engine()
    try:
        for i in range(21):
            entry, B, indexed = order[i % 7], SIZES[(i + shift) % 3], (i + shift) % 2 == 0
            got = call(eng, base, entry, B, indexed)
            assert same(got, first_calls(entry, B, indexed)), "call %d: %s, %d rows, lc_index %s" % (i, entry, B, indexed)
            if not indexed:
                assert same(got, first_calls(entry, B, False, zeros=True)), "call %d: %s without lc_index is not light curve 0" % (i, entry)
            status = np.atleast_1d(got[-1])
            if entry == "loglike_coeffs":
                assert np.all(status == 0)
            elif entry != "apply_inverse":
                assert status[REJECTED] == 1 and np.count_nonzero(status) == 1, (i, entry, status)
    finally:
        eng.close()
