"""The time-parallel kernels' per-row fall-back to the filter pass ("pass 3"), taken row by row inside one launch.

Every time-parallel family keeps the likelihood its scan carries only where

    psd (b d <= a c)  &&  min pivot > 0  &&  isfinite(ll)  &&  mag <= 1e3 |ll|

(`good`, mtg_timeparallel.h, for J <= 6; mtg_tpb_top_direct_kernel, mtg_tp_scan.hip, for rank 10, which appends the
others to a redo list).  tests/golden/tp_fallback_golden.json (made by tests/golden/make_tp_fallback_golden.py from the
quad-precision oracle; its own conditions are checked by test_tp_fallback_cpu.py) holds rows on both sides of that line
on one pair of light curves per group:

* healthy     S / |T| <= 10: kept;
* cancelling  |T| <= 1e-6 S, one parameter bisected in quad: mag / |ll| >= ~1e5, redone whatever the last bits are;
* nonfinite   the healthy thetas on light curve 1, whose one sample y = 1e160 overflows the squared residual:
              redone, and pass 3 leaves by its MTG_ST_NONFINITE exit (status 3, -inf, as celerite).

Rows that are not positive definite are deliberately absent for J <= 6: with the prior on, these kernels only see
b d <= a c and positive amplitudes, for which the covariance is positive definite mathematically; the sign of a pivot
is then rounding noise (the comment in test_fuzz_gpu.py) and a test on it would be flaky.  Rank 10's not-positive-
definite exit is covered by test_tp_big_gpu.py.

Layouts, for every family of CASES (each launch pinned by Engine.last_solver), under set_tp_direct(1) and (0):
mixed (healthy, cancelling, nonfinite by i % 3), one suspect (a single cancelling row in the middle / as the last row
among healthy ones), all suspect (every row cancelling; B odd for rank 10, whose redo list then holds B entries with
its counter directly behind them) and none (healthy only).  Groups hold 12 healthy and 24 (rank 10: 33) cancelling
rows, each bisected on its own; larger batches repeat them.

Assertions, with T the quad truth, c64 celerite's float64 value, u = 2^-53, S the row's error scale:

* statuses are the float64 oracle's; nonfinite rows read -inf;
* every status-0 row: |lnL - T| <= max(10 |c64 - T|, 64 sqrt(N) u S) -- test_accuracy_vs_quad_gpu.py's formula,
  absolute in S, so it judges a row whose lnL is ~0;
* the branch is taken row by row: a redone row under set_tp_direct(1) against the same row under set_tp_direct(0)
    - mtg_tp_kernel<..,64>, mtg_tp_fused_kernel<..,64> and <..,128>: bit for bit.  Both settings run the same
      instructions of mtg_tp_body for such a row: compose_chunk by lane, the Hillis-Steele scan, `finish` (which stores
      nothing: `good` is false under either setting), pass 3.
    - mtg_tp_kernel<..,256> and mtg_tp_fused_kernel<..,256> (the same mtg_tp_body with LANES = 256): bit for bit.
      Under (1) the row goes through tp_reduce_tree first, fails `finish`, and then composes its chunks a second time
      by lane (compose_chunk(lane)), scans them and filters -- from there on the arithmetic of setting (0).
    - rank 10: held to 64 sqrt(N) u S, not to bits.  The elements the redone row's start states are made of come from
      two different instantiations of the up-sweep, mtg_tpb_reduce_kernel<10, true> under (1) and <10, false> under (0)
      (launch_up, mtg_tp_scan.hip:290-296; tpw::combine<J, KAPPA>, mtg_tp_scan.h:210): the same formulas for the
      element, compiled separately with the likelihood record's extra terms in between and other launch bounds, so
      nothing in the source promises the same contractions.
  and at least one healthy row of every batch differs in its bits between the two settings: they really took different
  routes (the scan's number under 1, the filter's under 0);
* neighbours are not disturbed: under set_time_parallel(3) every row of every layout is bit for bit the same row of
  every other layout (mtg.h: a row's result does not depend on its batch); in particular the healthy rows of mixed are
  those of none.  Other modes: the healthy rows of mixed against none within 64 sqrt(N) u S;
* all suspect run twice gives identical results (the redo list's order is atomic, rows are written per row);
* the sampler reaches the branch: ensemble_init on 12 cancelling rows of the J = 3 model at N = 4096 (256-lane
  kernel) meets the truth bound.
"""
import json
import os

import numpy as np
import pytest

import golden_util

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
U = 2.0 ** -53
with open(os.path.join(HERE, "golden", "tp_fallback_golden.json")) as _f:
    GOLD = {g["name"]: g for g in json.load(_f)["groups"]}
BITS, FLOOR = "bits", "floor"

CASES = [
    # label, group, time-parallel mode, batch, kernel (both must be in last_solver), redone rows held to
    ("tp64/j3/n70", "j3/n70", 3, 24, ("mtg_tp_kernel<", ",64>"), BITS),
    ("tp64/j3/n1000", "j3/n1000", 3, 24, ("mtg_tp_kernel<", ",64>"), BITS),
    ("tp64/j4/n70", "j4/n70", 3, 24, ("mtg_tp_kernel<", ",64>"), BITS),
    ("tp64/j4/n1000", "j4/n1000", 3, 24, ("mtg_tp_kernel<", ",64>"), BITS),
    ("tp256/j3/n4096", "j3/n4096", 1, 24, ("mtg_tp_kernel<", ",256>"), BITS),
    ("tp256/j3/n4097", "j3/n4097", 1, 24, ("mtg_tp_kernel<", ",256>"), BITS),
    ("tp256/j4/n4096", "j4/n4096", 1, 24, ("mtg_tp_kernel<", ",256>"), BITS),
    ("tp256/j4/n4097", "j4/n4097", 1, 24, ("mtg_tp_kernel<", ",256>"), BITS),
    ("fused64/null/n1000", "null/n1000", 3, 24, ("mtg_tp_fused_kernel<", ",64>"), BITS),
    ("fused128/alt/n4096", "alt/n4096", 1, 384, ("mtg_tp_fused_kernel<", ",128>"), BITS),
    ("fused256/null/n4096", "null/n4096", 1, 24, ("mtg_tp_fused_kernel<", ",256>"), BITS),
    ("rank10_c64/5sho/n1024", "5sho/n1024", 1, 33, ("mtg_tpb_compose4q_kernel", "C = 64)"), FLOOR),
    ("rank10_c256/5sho/n8192", "5sho/n8192", 1, 33, ("mtg_tpb_compose4q_kernel", "C = 256)"), FLOOR),
]
IDS = [c[0] for c in CASES]
LAYOUTS = ("mixed", "one_mid", "one_last", "all", "none")


def rows_of(g, cls):
    return [i for i, r in enumerate(g["rows"]) if r["cls"] == cls]


def layout(g, name, B):
    """fixture row index of every batch row"""
    h, c, n = rows_of(g, "healthy"), rows_of(g, "cancelling"), rows_of(g, "nonfinite")
    pick = lambda rows, k: rows[k % len(rows)]
    if name == "mixed":
        return [pick((h, c, n)[i % 3], i // 3) for i in range(B)]
    if name in ("one_mid", "one_last"):
        at = B // 2 if name == "one_mid" else B - 1
        return [c[0] if i == at else pick(h, i) for i in range(B)]
    return [pick(c if name == "all" else h, i) for i in range(B)]


def setup(engine, g):
    t, y, dy = golden_util.quad_lightcurve(g["lightcurve"])
    assert golden_util.lightcurve_sha256(t, y, dy) == g["sha256"], "%s: the light curve is not the fixture's" % g["name"]
    P = len(g["rows"][0]["theta"]) - 1
    engine.set_lightcurves(t, y, dy + 1e-12, y_offset=np.asarray(g["y_offset"]))
    engine.set_model(g["kinds"], np.concatenate([g["rows"][0]["theta"][:P], [0.0]]), np.arange(P, dtype=np.int32),
                     np.tile([-np.inf, np.inf], (P + 1, 1)))
    return len(t), P


_runs = {}


def runs(engine, case):
    """every layout of a case under set_tp_direct(1) and (0), and all suspect a second time: computed once, shared by
    the tests below -> {(layout, direct): (fixture rows, lnL, status)}, N"""
    label, gname, tp, B, solver, _ = case
    if label in _runs:
        return _runs[label]
    g = GOLD[gname]
    out = {}
    try:
        N, P = setup(engine, g)
        engine.set_time_parallel(tp)
        engine.set_pipeline(0)
        for name in LAYOUTS:
            idx = layout(g, name, B)
            theta = np.array([g["rows"][i]["theta"][:P] for i in idx])
            lc = np.array([g["rows"][i]["lc"] for i in idx], dtype=np.int32)
            for direct in (1, 0) + ((1,) if name == "all" else ()):
                engine.set_tp_direct(direct)
                lnl, st = engine.loglike(theta, lc, add_prior=True)
                assert all(s in engine.last_solver for s in solver), "%s / %s: %s expected, %s dispatched" % (
                    label, name, solver, engine.last_solver)
                out[(name, direct) if (name, direct) not in out else (name, "again")] = (idx, lnl, st)
    finally:
        engine.set_time_parallel(2)
        engine.set_pipeline(2)
        engine.set_tp_direct(1)
    _runs[label] = (out, N)
    return _runs[label]


def floor(N, r):
    return 64.0 * np.sqrt(N) * U * r["S"]


def check_truth(label, g, N, idx, lnl, st):
    """statuses and the truth bound of the module docstring; returns the worst e / tol"""
    worst = 0.0
    for b, i in enumerate(idx):
        r = g["rows"][i]
        assert st[b] == r["c64_status"], "%s row %d (%s): status %d, celerite %d" % (label, b, r["cls"], st[b],
                                                                                    r["c64_status"])
        if r["c64_status"] != 0:
            assert lnl[b] == -np.inf, "%s row %d (%s): %r, not -inf" % (label, b, r["cls"], lnl[b])
            continue
        e = abs((lnl[b] - r["lnL"]) - r["lnL_lo"])
        e64 = abs((r["c64"] - r["lnL"]) - r["lnL_lo"])
        tol = max(10.0 * e64, floor(N, r))
        assert e <= tol, "%s row %d (%s): |lnL - T| = %.3e > %.3e (celerite %.3e, floor %.3e)" % (
            label, b, r["cls"], e, tol, e64, floor(N, r))
        worst = max(worst, e / tol)
    return worst


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_status_and_truth(engine, case):
    out, N = runs(engine, case)
    g = GOLD[case[1]]
    worst = {}
    for (name, direct), (idx, lnl, st) in out.items():
        worst["%s, direct %s" % (name, direct)] = check_truth("%s / %s / direct %s" % (case[0], name, direct), g, N,
                                                              idx, lnl, st)
    name = max(worst, key=worst.get)
    print("\ntp-fallback %-24s worst e/tol %.3g (%s; %s)" % (case[0], worst[name], name, engine.last_solver))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_branch_is_taken_row_by_row(engine, case):
    out, N = runs(engine, case)
    g = GOLD[case[1]]
    for name in LAYOUTS:
        (idx, on, st_on), (_, off, st_off) = out[(name, 1)], out[(name, 0)]
        assert np.array_equal(st_on, st_off), "%s / %s" % (case[0], name)
        cls = np.array([g["rows"][i]["cls"] for i in idx])
        for b in np.flatnonzero(cls != "healthy"):
            r = g["rows"][idx[b]]
            if case[5] == BITS or r["cls"] == "nonfinite":
                assert on[b] == off[b], "%s / %s row %d (%s): %r under set_tp_direct(1), %r under (0)" % (
                    case[0], name, b, r["cls"], on[b], off[b])
            else:
                assert abs(on[b] - off[b]) <= floor(N, r), "%s / %s row %d: %r under set_tp_direct(1), %r under (0)" % (
                    case[0], name, b, on[b], off[b])
        kept = cls == "healthy"
        if kept.any():
            assert np.any(on[kept] != off[kept]), (
                "%s / %s: every healthy row has the filter pass's bits under set_tp_direct(1)" % (case[0], name))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_neighbours_are_not_disturbed(engine, case):
    out, N = runs(engine, case)
    g = GOLD[case[1]]
    for direct in (1, 0):
        if case[2] == 3:      # a row's bits do not depend on its batch: one value per fixture row over all layouts
            seen = {}
            for name in LAYOUTS:
                idx, lnl, _ = out[(name, direct)]
                for b, i in enumerate(idx):
                    where, v = seen.setdefault(i, ("%s row %d" % (name, b), lnl[b]))
                    assert lnl[b] == v, "%s, direct %d: fixture row %d (%s) is %r in %s row %d and %r in %s" % (
                        case[0], direct, i, g["rows"][i]["cls"], lnl[b], name, b, v, where)
        (idx_m, mixed, _), (idx_n, none, _) = out[("mixed", direct)], out[("none", direct)]
        alone = {i: none[b] for b, i in reversed(list(enumerate(idx_n)))}
        for b, i in enumerate(idx_m):
            r = g["rows"][i]
            if r["cls"] != "healthy":
                continue
            if case[2] == 3:
                assert mixed[b] == alone[i], "%s, direct %d: healthy row %d: %r in mixed, %r in none" % (
                    case[0], direct, i, mixed[b], alone[i])
            else:
                assert abs(mixed[b] - alone[i]) <= floor(N, r), "%s, direct %d: healthy row %d: %r in mixed, %r in none" % (
                    case[0], direct, i, mixed[b], alone[i])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_all_suspect_repeats(engine, case):
    out, _ = runs(engine, case)
    (_, first, st1), (_, again, st2) = out[("all", 1)], out[("all", "again")]
    assert np.array_equal(st1, st2) and np.array_equal(first, again), "%s: a second run of all suspect differs" % case[0]
    assert np.all(st1 == 0)


def test_sampler_reaches_the_branch(engine):
    """ensemble_init's log-probabilities (inside the box the prior adds 0) of one ensemble of 12 walkers started on
    cancelling rows, J = 3, N = 4096: the default dispatch takes the 256-lane kernel, whose tree fails `finish` for
    every one of them."""
    g = GOLD["j3/n4096"]
    rows = rows_of(g, "cancelling")[:12]
    try:
        engine.set_time_parallel(2)
        engine.set_pipeline(2)
        N, P = setup(engine, g)
        theta = np.array([g["rows"][i]["theta"][:P] for i in rows])
        engine.ensemble_init(theta[None], seed=1, lc_of_ensemble=[0])
        lnp = engine.ensemble_state()["log_prob"].reshape(-1)
        assert "mtg_tp_kernel<" in engine.last_solver and ",256>" in engine.last_solver, engine.last_solver
    finally:
        engine.set_time_parallel(2)
        engine.set_pipeline(2)
    worst = check_truth("sampler_init / j3/n4096", g, N, rows, lnp, np.zeros(len(rows), dtype=np.int32))
    print("\ntp-fallback %-24s worst e/tol %.3g (%s)" % ("sampler_init", worst, engine.last_solver))
