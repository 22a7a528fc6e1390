"""Every likelihood kernel family against the quad-precision truth (tests/golden/quad_golden.json, made by
tests/golden/make_quad_golden.py from oracle/celerite_quad.c) at N up to 2e5: the serial sweep and its table / libm
phase variants, the structure-sorted and pipelined sweeps, the paired pipeline, the time-parallel kernels (one-wave,
wide, fused 64 / 128 / 256 lanes; scanned likelihood and filter pass), the rank-10 composition (fast and two-part phase
reduction, 64 and 256 chunks), the white kernel, the raw-coefficient entry and the sampler's initial log-probabilities.

Per row, with T the quad truth, c64 celerite's float64 value (stored), u = 2^-53, S the row's error scale
(1/2 (sum |ln D_n| + sum z_n^2 / D_n + N ln 2 pi)) and e = |lnL - T|:

* status 0, as celerite's;
* e <= max(10 |c64 - T|, 64 sqrt(N) u S): no worse than celerite, and at rounding level where celerite is;
* rows of d max(dx) in [1e4, 1e12] (the table phase, N >= 1000) taken by a table-phase kernel:
  e_raw <= max(|c64 - T_raw|, 64 sqrt(N) u S), T_raw the truth of the float64 coefficients both kernels are handed.
  That is the claim of mtg_math.h (above MTG_TRIG_FAST_MAX): the accumulated table phase is no less accurate than
  celerite's phase at the absolute time.  It is held against T_raw, not T: at 1e8 rad per step and beyond, the
  rounding of d to a double alone moves lnL by more than the phase evaluation does, identically for both kernels.
  T_raw is computed from oracle.dense.build_coeffs; should the device's builder round d one ulp differently, lnL moves
  by about |T_raw - T| (at most 1e-4 at 9e11 rad per step), far below celerite's own error on such rows (0.29).

The bounds are these formulas; they are not fitted to a run.  Every kernel is pinned by Engine.last_solver.  Two choices
are made inside a kernel and do not show in its name: the sweep's libm phase variant (per wave; its test asserts that
the batch holds a row beyond MTG_TRIG_FAST_MAX in the same wave and that the shared rows' bits differ from the
table variant's) and the rank-10 path's fast / two-part reduction (per row at d max(dx) = 1e5; covered by fixture rows
on both sides, which test_rank10_fast_and_two_part_reduction_are_both_taken checks).  Groups with mean_kind 1 fit a
linear mean (no y_offset), among them at t ~ 1e9 s."""
import json
import os
import threading

import numpy as np
import pytest

import golden_util
from mind_the_gaps_amd.engine import MEAN_LINEAR

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
U = 2.0 ** -53
with open(os.path.join(HERE, "golden", "quad_golden.json")) as _f:
    GOLD = {g["name"]: g for g in json.load(_f)["groups"]}
SINGLE = ["phase/j3", "long_memory", "typical/bpl+matern32", "typical/complex4+real"]      # one structure, J <= 6
WITH_SHO = ["typical/null", "typical/alt", "typical/null_n64", "typical/alt_n65", "typical/cosinus+jitter+sho",
            "short_memory", "extreme/null", "offset/mjd", "offset/seconds"]
RANK10 = ["typical/5sho", "extreme/5sho", "phase/j10", "rank10/config5"]
LIN_SINGLE = ["linear_mean/drw+real_seconds", "linear_mean/j3_seconds"]       # fitted line, one structure, J <= 6
LIN_SHO = ["linear_mean/null", "linear_mean/null_seconds"]
TABLE_ONLY = lambda r: r["d_dxmax"] <= 1.0e12


def group(name):
    g = GOLD[name]
    t, y, dy = golden_util.quad_lightcurve(g["lightcurve"])
    assert golden_util.lightcurve_sha256(t, y, dy) == g["sha256"], "%s: the light curve is not the fixture's" % name
    return g, t, y, dy


def linear(name):
    return GOLD[name].get("mean_kind", 0) == 1


def free(name, r):
    """a row's free parameters: the kernel's, and the fitted line's under mean_kind 1 (a constant mean is frozen at 0,
    the light curve's average travelling as y_offset)"""
    return r["theta"] if linear(name) else r["theta"][:-1]


def setup(engine, name, rows=None):
    g, t, y, dy = group(name)
    rows = [r for r in g["rows"] if rows is None or rows(r)]
    if linear(name):
        P = len(rows[0]["theta"])
        engine.set_lightcurves(t, y, dy + 1e-12)
        engine.set_model(g["kinds"], np.asarray(rows[0]["theta"]), np.arange(P, dtype=np.int32),
                         np.tile([-np.inf, np.inf], (P, 1)), mean_kind=MEAN_LINEAR)
    else:
        P = len(rows[0]["theta"]) - 1
        engine.set_lightcurves(t, y, dy + 1e-12, y_offset=np.asarray(g["y_offset"]))
        engine.set_model(g["kinds"], np.concatenate([rows[0]["theta"][:P], [0.0]]), np.arange(P, dtype=np.int32),
                         np.tile([-np.inf, np.inf], (P + 1, 1)))
    return g, len(t), rows


def tiled(name, rows, B):
    idx = np.arange(B) % len(rows)
    return (idx, np.array([free(name, rows[i]) for i in idx]),
            np.array([rows[i]["lc"] for i in idx], dtype=np.int32))


def check(label, N, rows, idx, out, status, phase_claim, raw=False):
    """The bounds of the module docstring; returns the worst e / tol."""
    assert np.all(status == 0), "%s: statuses %s (celerite: 0)" % (label, np.unique(status))
    worst = 0.0
    for b, i in enumerate(idx):
        r = rows[i]
        T, lo = (r["lnL_raw"], r["lnL_raw_lo"]) if raw else (r["lnL"], r["lnL_lo"])
        e = abs((out[b] - T) - lo)
        e64 = abs((r["c64"] - T) - lo)
        floor = 64.0 * np.sqrt(N) * U * r["S"]
        tol = max(10.0 * e64, floor)
        assert e <= tol, "%s row %d %s: |lnL - T| = %.3e > %.3e (celerite %.3e, floor %.3e)" % (
            label, i, r["tags"], e, tol, e64, floor)
        worst = max(worst, e / tol)
        if phase_claim and N >= 1000 and 1.0e4 <= r["d_dxmax"] <= 1.0e12:
            er = abs((out[b] - r["lnL_raw"]) - r["lnL_raw_lo"])
            e64r = abs((r["c64"] - r["lnL_raw"]) - r["lnL_raw_lo"])
            assert er <= max(e64r, floor), "%s row %d %s: table phase %.3e worse than celerite's %.3e (floor %.3e)" % (
                label, i, r["tags"], er, e64r, floor)
    return worst


def run(engine, label, names, solver, B=None, tp=0, pipe=0, direct=1, rows=None, phase_claim=True):
    worst = {}
    try:
        engine.set_time_parallel(tp)
        engine.set_pipeline(pipe)
        engine.set_tp_direct(direct)
        for name in names:
            g, N, rs = setup(engine, name, rows)
            idx, theta, lc = tiled(name, rs, B or len(rs))
            out, st = engine.loglike(theta, lc, add_prior=True)
            assert solver in engine.last_solver, "%s / %s: %s expected, %s dispatched" % (label, name, solver,
                                                                                         engine.last_solver)
            worst[name] = check("%s / %s" % (label, name), N, rs, idx, out, st, phase_claim)
    finally:
        engine.set_time_parallel(2)
        engine.set_pipeline(2)
        engine.set_tp_direct(1)
    report(label, worst, engine.last_solver)


def report(label, worst, solver):
    name = max(worst, key=worst.get)
    print("\nquad-truth %-22s worst e/tol %.3g (%s; %s)" % (label, worst[name], name, solver))


ALL_SWEEP = SINGLE + WITH_SHO + ["typical/jitter_only"] + ["signatures"] + RANK10[:3]
CASES = [
    # label, groups, expected kernel, batch, time-parallel mode, pipeline, direct, rows
    ("sweep", [n for n in ALL_SWEEP if n not in ("typical/jitter_only", "phase/j10", "phase/j3")] + LIN_SINGLE + LIN_SHO
     + ["linear_mean/5sho_mjd"], "mtg_solve_kernel<", None, 0, 0, 1, None),
    ("sweep_table_phase", ["phase/j3", "phase/j10"], "mtg_solve_kernel<", None, 0, 0, 1, TABLE_ONLY),
    ("multi", ["signatures", "typical/null", "offset/mjd", "linear_mean/null"], "mtg_solve_kernel_multi<", 128, 0, 0, 1,
     None),
    ("pipe", ["typical/null", "typical/alt", "signatures", "short_memory", "offset/seconds", "extreme/null"] + LIN_SHO,
     "mtg_pipe_kernel<", 128, 0, 1, 1, None),
    ("pipe_linear_single", ["linear_mean/j3_seconds"], "mtg_pipe_kernel<", None, 0, 1, 1, None),   # (needs nc >= 1)
    ("pipe_phase", ["phase/j3"], "mtg_pipe_kernel<", None, 0, 1, 1, TABLE_ONLY),
    ("tp_one_wave", SINGLE + LIN_SINGLE, "mtg_tp_kernel<", None, 3, 0, 1, None),
    ("tp_one_wave_filter", SINGLE + LIN_SINGLE, "mtg_tp_kernel<", None, 3, 0, 0, None),
    ("tp_wide", ["phase/j3", "long_memory"] + LIN_SINGLE, ",256>", None, 1, 0, 1, None),
    ("tp_wide_filter", ["phase/j3", "long_memory"] + LIN_SINGLE, ",256>", None, 1, 0, 0, None),
    ("tp_fused64", WITH_SHO + LIN_SHO, "mtg_tp_fused_kernel<", None, 3, 0, 1, None),
    ("tp_fused256_linear", LIN_SHO, ",256>", 64, 1, 0, 1, None),
    ("tp_fused64_filter", ["signatures", "typical/alt", "short_memory"], ",64>", 640, 1, 0, 0, None),
    ("tp_fused128", ["signatures"], ",128>", 384, 1, 0, 1, None),
    ("tp_fused256", ["signatures", "typical/null"], ",256>", 64, 1, 0, 1, None),
    ("tp_fused256_filter", ["signatures"], ",256>", 64, 1, 0, 0, None),
    ("tpb_c256", ["phase/j10", "rank10/config5"], "C = 256", 128, 1, 0, 1, None),
    ("tpb_c256_filter", ["phase/j10"], "C = 256", 128, 1, 0, 0, None),
    ("tpb_c64", ["phase/j10", "rank10/config5"], "C = 64", 512, 1, 0, 1, None),
    ("tpb_c64_filter", ["phase/j10"], "C = 64", 512, 1, 0, 0, None),
    ("tpb", ["typical/5sho", "extreme/5sho", "linear_mean/5sho_mjd"], "mtg_tpb_compose4q_kernel", None, 1, 0, 1, None),
    ("tpb_filter", ["typical/5sho", "extreme/5sho", "linear_mean/5sho_mjd"], "mtg_tpb_compose4q_kernel", None, 1, 0, 0,
     None),
    ("white", ["typical/jitter_only"], "mtg_white_kernel", None, 0, 0, 1, None),
]


@pytest.mark.parametrize("label,names,solver,B,tp,pipe,direct,rows", CASES, ids=[c[0] for c in CASES])
def test_family_against_quad_truth(engine, label, names, solver, B, tp, pipe, direct, rows):
    run(engine, label, names, solver, B, tp, pipe, direct, rows)


@pytest.mark.parametrize("name", ["phase/j3", "phase/j10"])
def test_sweep_libm_phase_variant_against_quad_truth(engine, name):
    """The serial sweep's libm phase variant: a row with d max(dx) > MTG_TRIG_FAST_MAX (1e12) in the wave sends every
    row of that wave through it.  The whole group fits one wave; its table-range rows, swept alone, take the table
    variant -- and the two runs of those rows must differ in their bits (really another variant), both within the
    bounds (the table-phase claim applies to the table run only)."""
    fast_max = 1.0e12
    try:
        engine.set_time_parallel(0)
        engine.set_pipeline(0)
        g, N, table = setup(engine, name, TABLE_ONLY)
        idx_t, theta_t, lc_t = tiled(name, table, len(table))
        out_t, st_t = engine.loglike(theta_t, lc_t, add_prior=True)
        assert "mtg_solve_kernel<" in engine.last_solver, engine.last_solver
        check("sweep_table / " + name, N, table, idx_t, out_t, st_t, True)
        g, N, rs = setup(engine, name)
        assert len(rs) <= 64 and max(r["d_dxmax"] for r in rs) > fast_max >= max(r["d_dxmax"] for r in table)
        idx, theta, lc = tiled(name, rs, len(rs))
        out, st = engine.loglike(theta, lc, add_prior=True)
        assert "mtg_solve_kernel<" in engine.last_solver, engine.last_solver
        worst = check("sweep_libm / " + name, N, rs, idx, out, st, False)
    finally:
        engine.set_time_parallel(2)
        engine.set_pipeline(2)
    shared = [rs.index(r) for r in table]
    assert np.any(out[shared] != out_t), "%s: the rows came out bit for bit as on the table variant" % name
    report("sweep_libm_phase", {name: worst}, engine.last_solver)


def test_rank10_fast_and_two_part_reduction_are_both_taken():
    """tpb_* above cover both phase reductions of mtg_tp_big.h: rows below and above d max(dx) = 1e5."""
    d = [r["d_dxmax"] for r in GOLD["phase/j10"]["rows"]] + [r["d_dxmax"] for r in GOLD["rank10/config5"]["rows"]]
    assert min(d) <= 1.0e5 < max(d)


def test_paired_pipeline_against_quad_truth(engine):
    """Two contexts' pipelined half-steps in one launch (mtg_pipe_pair_kernel), each driven from its own thread."""
    from mind_the_gaps_amd.engine import Engine
    other = Engine(0)
    engines = {"typical/null": other, "typical/alt": engine}
    batches, got, worst = {}, {}, {}
    try:
        for name, eng in engines.items():
            g, N, rs = setup(eng, name)
            eng.set_time_parallel(0)
            eng.set_pipeline(1)
            batches[name] = (N, rs) + tiled(name, rs, 128)
        other.pair_with(engine)

        def job(name):
            got[name] = engines[name].loglike(batches[name][3], batches[name][4], add_prior=True) + (
                engines[name].last_solver,)
        threads = [threading.Thread(target=job, args=(n,)) for n in engines]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        stats = engine.pair_stats()
        other.unpair()
        assert stats["paired"] >= 1 and not stats["broken"], stats
        for name in engines:
            N, rs, idx = batches[name][:3]
            out, st, solver = got[name]
            assert "mtg_pipe_pair_kernel" in solver, "%s dispatched" % solver
            worst[name] = check("pipe_pair / " + name, N, rs, idx, out, st, True)
    finally:
        for eng in engines.values():
            eng.set_time_parallel(2)
            eng.set_pipeline(2)
        other.close()
    report("pipe_pair", worst, "mtg_pipe_pair_kernel")


@pytest.mark.parametrize("name", ["typical/alt", "phase/j3", "long_memory", "typical/5sho", "linear_mean/null",
                                  "linear_mean/drw+real_seconds", "linear_mean/j3_seconds"])
def test_coefficient_entry_against_quad_truth(engine, name):
    """Engine.loglike_coeffs: the float64 coefficients stored with each row, against their own quad truth (mean
    constant at 0 after y_offset, or the fitted line, MEAN_LINEAR)."""
    g, N, rs = setup(engine, name, TABLE_ONLY)
    co = [np.array([r["coeffs"][k] for r in rs]) for k in range(6)]
    jit = np.array([r["coeffs"][6] for r in rs])
    if linear(name):
        mean = dict(mean_kind=MEAN_LINEAR, mean_params=np.array([r["theta"][-2:] for r in rs]))
    else:
        mean = dict(mean_params=np.zeros((len(rs), 1)))
    out, st = engine.loglike_coeffs(*co, jitter=jit, lc_index=np.array([r["lc"] for r in rs], dtype=np.int32), **mean)
    assert "(coefficients)" in engine.last_solver, engine.last_solver
    report("coeffs", {name: check("coeffs / " + name, N, rs, np.arange(len(rs)), out, st, True, raw=True)},
           engine.last_solver)


@pytest.mark.parametrize("tp,solver", [(2, "mtg_tp_fused_kernel<1,1,2,256>"), (0, "mtg_solve_kernel<")],
                         ids=["default-dispatch", "serial-sweep"])
def test_sampler_initial_log_prob_against_quad_truth(engine, tp, solver):
    """ensemble_init's log-probabilities (inside the box the prior adds 0): one ensemble of 12 walkers, through the
    default dispatch (12 rows of N = 4096: the 256-lane fused time-parallel kernel) and through the serial sweep."""
    name = "typical/null"
    try:
        engine.set_time_parallel(tp)
        engine.set_pipeline(2 if tp else 0)
        g, N, rs = setup(engine, name)
        theta = np.array([free(name, r) for r in rs])
        engine.ensemble_init(theta[None], seed=1)
        lnp = engine.ensemble_state()["log_prob"].reshape(-1)
        assert solver in engine.last_solver, "%s expected, %s dispatched" % (solver, engine.last_solver)
    finally:
        engine.set_time_parallel(2)
        engine.set_pipeline(2)
    report("sampler_init", {name: check("sampler_init / " + name, N, rs, np.arange(len(rs)), lnp,
                                        np.zeros(len(rs), dtype=np.int32), True)}, engine.last_solver)
