"""Loaders for tests/golden/loglike_golden.{json,npz} (made by tests/golden/make_golden.py), the light curves of
tests/golden/quad_golden.json and tests/golden/tp_fallback_golden.json (made by tests/golden/make_quad_golden.py and
tests/golden/make_tp_fallback_golden.py), the right-hand sides and new times of
tests/golden/predict_golden.npz (made by tests/golden/make_predict_golden.py) and the calls of
tests/golden/solve_dispatch.json (made by tests/golden/make_solve_dispatch_golden.py)."""
import hashlib
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
_cache = None


def cases():
    global _cache
    if _cache is None:
        man = json.load(open(os.path.join(HERE, "golden", "loglike_golden.json")))["cases"]
        arr = np.load(os.path.join(HERE, "golden", "loglike_golden.npz"))
        for c in man:
            c["t"], c["y"], c["dy"] = arr[c["id"] + "_t"], arr[c["id"] + "_y"], arr[c["id"] + "_dy"]
            c["full"] = np.array(c["theta"] + c["mean_params"])
        _cache = man
    return _cache


def best_truth(c):
    """Most trustworthy value a case carries: mpmath > OU closed form > dense float64."""
    for k in ("lnL_mpmath50", "lnL_ou_closed_form", "lnL_dense_f64"):
        if not np.isnan(c[k]):
            return c[k]
    raise ValueError(c["id"])


def quad_lightcurve(rec):
    """A quad_golden.json recipe -> (t, y, dy): synthetic.make_lightcurves(N, L, seed, offset), then the edit of the
    sampling if any ("dup_gap": repeated epochs, dx = 0, every N / 7 samples and a gap of 1e6 days after the middle;
    "quiet_spike", tp_fallback_golden.json: the scatter of y about 100 and the errors both scaled by rec["scale"] / 10
    and rec["scale"], then a second light curve equal to the first but for y[1][rec["spike"]] = rec["spike_value"])."""
    from mind_the_gaps_amd import synthetic as synth
    t, y, dy = synth.make_lightcurves(rec["N"], rec["L"], rec["seed"], rec["offset"])
    edit = rec.get("edit")
    if edit == "dup_gap":
        t = t.copy()
        for i in range(10, rec["N"] - 1, rec["N"] // 7):
            t[i + 1] = t[i]
        t[rec["N"] // 2:] += 1.0e6
    elif edit == "quiet_spike":
        quiet = 100.0 + rec["scale"] * (y[0] - 100.0) / 10.0
        y, dy = np.stack([quiet, quiet]), np.stack([rec["scale"] * dy[0]] * 2)
        y[1, rec["spike"]] = rec["spike_value"]
    elif edit is not None:
        raise ValueError(edit)
    return t, y, dy


def lightcurve_sha256(t, y, dy):
    h = hashlib.sha256()
    for a in (t, y, dy):
        h.update(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    return h.hexdigest()


def fp32_column(v):
    """v rounded to float32 (and back): a libm or SIMD path that differs in the last bit of a double gives the same
    column"""
    return np.asarray(v, dtype=np.float64).astype(np.float32).astype(np.float64)


def col_sha(b):
    return hashlib.sha256(np.ascontiguousarray(b, dtype=np.float64).tobytes()).hexdigest()


def apply_columns(t, y, mean_kind, full, nk, kinds, seed):
    """predict_golden.npz's three right-hand sides [N][3] of a row: the residual y - mean, a standard-normal column and
    the column k(t_* - t) of K_*^T at t_* inside the largest gap (the last two float32-rounded)"""
    from oracle import dense
    N = len(t)
    mean = full[nk] * t + full[nk + 1] if mean_kind == 1 else np.full(N, full[nk])
    g = int(np.argmax(np.diff(t)))
    ts = t[g] + 0.375 * (t[g + 1] - t[g])
    kcol = fp32_column(dense.kernel_value(dense.build_coeffs(kinds, full[:nk]), ts - t))
    normal = fp32_column(np.random.default_rng(seed).standard_normal(N))
    return np.column_stack([y - mean, normal, kcol])


FULL_WINDOW = 0xFFFFFFFF   # mtg_set_window_bytes' default


def dispatch_case(eng, case):
    """One call of a solve_dispatch.json case on ``eng``; returns eng.last_solver.  Only the shapes, the modes and the
    order of lc_index decide the kernel, so the values are whatever synthetic.py draws."""
    from mind_the_gaps_amd import synthetic as synth
    N, L, B = case["N"], case["L"], case["B"]
    t, y, dy = synth.make_lightcurves(N, L, seed=N + L)
    rng = np.random.default_rng(B)
    lc = {"random": lambda: rng.integers(0, L, B).astype(np.int32),
          "grouped": lambda: np.sort(rng.integers(0, L, B)).astype(np.int32),
          "none": lambda: None}[case["lc"]]()
    eng.set_window_bytes(FULL_WINDOW)
    eng.set_lightcurves(t, y, dy + 1e-12)
    eng.set_time_parallel(case["tp"])
    eng.set_pipeline(case["pipe"])
    eng.set_sort(case["sort"])
    try:
        if case.get("window"):
            eng.set_window_bytes(case["window"])
        if case["op"] == "coeffs":
            jr, jc = case["jr"], case["jc"]
            eng.loglike_coeffs(np.full((B, jr), 2.0), np.full((B, jr), 0.3), np.full((B, jc), 1.5), np.zeros((B, jc)),
                               np.full((B, jc), 0.2), np.full((B, jc), 0.9), jitter=np.full(B, 0.5),
                               mean_params=np.full((B, 1), 100.0), lc_index=lc)
        else:
            kinds = case["kinds"]
            full, free, bounds = synth.model_spec(kinds, y)
            eng.set_model(kinds, full, free, bounds)
            eng.loglike(synth.draw_thetas(kinds, B, seed=B, percent=0.05), lc, add_prior=case["add_prior"])
        return eng.last_solver
    finally:
        eng.set_window_bytes(FULL_WINDOW)
        eng.set_time_parallel(2)
        eng.set_pipeline(2)
        eng.set_sort(2)


def protassov_problem():
    """The small Protassov test that tests/test_distributed.py's workers and tests/golden/ppp_end_to_end.json run:
    (light curve, null kernel, alternative kernel, the arguments every mode shares).  N = 400 is long enough for the
    time-parallel kernels to be an option."""
    from mind_the_gaps_amd import synthetic as synth
    from mind_the_gaps_amd.lightcurves import GappyLightcurve
    from mind_the_gaps_amd.models import DampedRandomWalk, Lorentzian
    th = synth.truth(synth.ALT_MODEL)
    t, y, dy = synth.make_lightcurves(400, 1, seed=43)
    lc = GappyLightcurve(t, y[0] + 50.0, dy[0], exposures=0.5 * np.diff(t).min())
    null = DampedRandomWalk(th[0], th[1], bounds=[(-10, 50), (-10, 10)])
    alt = DampedRandomWalk(th[0], th[1], bounds=[(-10, 50), (-10, 10)]) + Lorentzian(
        th[5], th[6], th[7], bounds=[(-10, 50), (-10, 10), (-10, 10)])
    return lc, null, alt, dict(nsims=5, walkers=16, max_steps=60, sim_steps=40, seed=11)


def new_times(t, seed):
    """predict_golden.npz's 48 new times: 24 between samples, 12 on samples, 6 before the first and 6 after the last"""
    rng = np.random.default_rng(seed)
    N = len(t)
    span = t[-1] - t[0]
    i = rng.choice(N - 1, 24, replace=False)
    between = t[i] + rng.uniform(0.1, 0.9, 24) * (t[i + 1] - t[i])
    on = t[rng.choice(N, 12, replace=False)]
    before = t[0] - span * np.array([1e-4, 1e-3, 1e-2, 0.05, 0.2, 1.0])
    after = t[-1] + span * np.array([1e-4, 1e-3, 1e-2, 0.05, 0.2, 1.0])
    return np.sort(np.concatenate([between, on, before, after]))
