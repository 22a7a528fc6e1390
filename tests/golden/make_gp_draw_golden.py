#!/usr/bin/env python3
"""Generates tests/golden/gp_draw_golden.npz: the truth of Engine.gp_draw with given normals, for
tests/test_gp_draw_gpu.py.

Truth T: the recurrence y = mean + L sqrt(D) q of csrc/mtg_gp_draw.hip in mpmath at 40 digits with the phases at the
absolute time (tests/gp_draw_replay.mp_draw), rounded to float64.  The generator checks it against the mpmath dense
Cholesky (50 digits) on the first 128 samples of every row and fails if the two differ by more than 1e-3 of the test's
floor 64 sqrt(N) u s.  Next to T: |c64 - T| with c64 the same recurrence in float64 with celerite's phase at the
absolute time (gp_draw_replay.draw on factor(phase="absolute", compensated=False)), and the scale
s_n = sum_m |L_nm sqrt(D_m) q_m| (float32 both: the test needs c64 only through rho = max |c64 - T| / s, and c64 itself
in float64 would take the file past predict_golden.npz's size).

Light curves are golden_util.quad_lightcurve recipes (regenerated, SHA-256 in the manifest); parameter rows are those
of tests/golden/quad_golden.json where a group of that model exists.  The normals of row b are
fp32_column(default_rng(seed_b).standard_normal(N)), SHA-256 in the manifest.  The constant mean travels as y_offset
(the model's mean is 0 and the draw excludes it); a linear mean is part of the draw.  Groups: every kernel family, an
SHO term on either side of Q = 1/2 on two light curves, a time offset of 5e8 s, a fitted linear mean with a jitter
term, per-light-curve sampling, phases up to 1e10 rad per day, J = 10 at N = 1e4, and the headline model
(DRW + SHO + Lorentzian) at N = 2e5, whose truth is kept at the first 64, the last 64 and every 100th sample (every
sample below N = 10 001) so that the file stays below predict_golden.npz's 486 965 bytes.

Run from the repo root:  python tests/golden/make_gp_draw_golden.py   (about 6 minutes on 8 cores; deterministic)
"""
import io
import json
import multiprocessing
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import gp_draw_replay as R  # noqa: E402
from golden_util import col_sha, fp32_column, lightcurve_sha256 as sha  # noqa: E402
from golden_util import quad_lightcurve  # noqa: E402
from mind_the_gaps_amd import synthetic as synth  # noqa: E402
from oracle import dense  # noqa: E402

U = 2.0 ** -53
EVERY = 100
CHECK_N = 128


def quad_rows(name, picks):
    with open(os.path.join(HERE, "quad_golden.json")) as f:
        g = {x["name"]: x for x in json.load(f)["groups"]}[name]
    return g["kinds"], g["lightcurve"], [g["rows"][i] for i in picks]


def groups():
    """(name, kinds, recipes, mean_kind, rows [{theta (kernel, then the line's slope and intercept), lc}])"""
    out = []
    kinds, rec, rows = quad_rows("signatures", [0, 1])      # Q = 0.30 | 0.50 on light curve 0, Q = 0.49 | 3.1 on 1
    out.append(("signatures", kinds, [dict(rec, N=2048)], 0, [dict(theta=r["theta"][:-1], lc=r["lc"]) for r in rows]))
    for name, n in (("typical/bpl+matern32", None), ("typical/cosinus+jitter+sho", 2000), ("typical/complex4+real", None)):
        kinds, rec, rows = quad_rows(name, [0])
        out.append((name, kinds, [rec if n is None else dict(rec, N=n)], 0, [dict(theta=rows[0]["theta"][:-1], lc=0)]))
    kinds, rec, rows = quad_rows("phase/j3", [0, 5])        # complex3 + DRW: d = 0.96 and 1.05e10 rad per day
    out.append(("phase/complex3+drw", kinds, [dict(rec, N=1000)], 0, [dict(theta=r["theta"][:-1], lc=0) for r in rows]))
    null = [float(v) for v in synth.truth(synth.NULL_MODEL)]
    out.append(("offset/5e8s", [int(k) for k in synth.NULL_MODEL], [dict(N=1000, L=1, seed=301, offset=5.0e8, edit=None)], 0,
                [dict(theta=null, lc=0)]))
    # DRW + SHO + jitter (sigma = e^-0.5) under a fitted line, times in seconds past 5e8
    out.append(("linear_mean+jitter", [int(k) for k in synth.NULL_MODEL] + [5],
                [dict(N=1000, L=1, seed=302, offset=5.0e8, edit=None)], 1,
                [dict(theta=null + [-0.5, 2.0e-3, 100.0 - 2.0e-3 * 5.0e8], lc=0)]))
    out.append(("per_lc_sampling", [int(k) for k in synth.NULL_MODEL],
                [dict(N=1000, L=1, seed=303, offset=0.0, edit=None), dict(N=1000, L=1, seed=304, offset=59000.0, edit=None)], 0,
                [dict(theta=null, lc=0), dict(theta=null, lc=1)]))
    kinds, rec, rows = quad_rows("typical/5sho", [0])
    out.append(("typical/5sho", kinds, [rec], 0, [dict(theta=rows[0]["theta"][:-1], lc=0)]))
    out.append(("headline/n200000", [int(k) for k in synth.ALT_MODEL],
                [dict(N=200000, L=1, seed=20250711, offset=0.0, edit=None)], 0,
                [dict(theta=[float(v) for v in synth.truth(synth.ALT_MODEL)], lc=0)]))
    return out


def lightcurves(recipes):
    """one recipe: (t [N], y [L][N], dy [L][N]); several (per-light-curve sampling): t [L][N], one light curve each"""
    parts = [quad_lightcurve(r) for r in recipes]
    if len(parts) == 1:
        return parts[0]
    return np.array([p[0] for p in parts]), np.vstack([p[1] for p in parts]), np.vstack([p[2] for p in parts])


def stored_indices(N):
    if N <= 10000:
        return np.arange(N, dtype=np.int32)
    return np.unique(np.concatenate([np.arange(64), np.arange(0, N, EVERY), np.arange(N - 64, N)])).astype(np.int32)


def normals(seed, N):
    return fp32_column(np.random.default_rng(seed).standard_normal(N))


def row_job(job):
    name, kinds, mean_kind, theta, t, dy, seed = job
    N = len(t)
    nk = dense.n_kernel_params(kinds)
    coeffs = dense.build_coeffs(kinds, theta[:nk])
    mp_mean = tuple(theta[nk:nk + 2]) if mean_kind == 1 else (0.0,)
    mean = theta[nk] * t + theta[nk + 1] if mean_kind == 1 else 0.0
    q = normals(seed, N)
    idx = stored_indices(N)
    T, status = R.mp_draw(t, dy, coeffs, q, mean_kind=mean_kind, mean_params=mp_mean, dps=40)
    assert status == 0, name
    fac = R.factor(t, R.diagonal(dy, coeffs), coeffs, phase="absolute", compensated=False)
    c64 = R.draw(t, dy, coeffs, q, mean=mean, factors=fac)
    s = R.scale_at(t, coeffs, R.factor(t, R.diagonal(dy, coeffs), coeffs, compensated=False), q, idx)
    # the recurrence against the dense Cholesky, both in mpmath, on the first CHECK_N samples (a draw's first samples
    # do not depend on the later ones)
    n = min(N, CHECK_N)
    Td = R.mp_dense_draw(t[:n], dy[:n], coeffs, q[:n], mean_kind=mean_kind, mean_params=mp_mean, dps=50)
    ki = idx[idx < n]
    # both are rounded to float64: up to an ulp of y apart
    slack = np.abs(T[ki] - Td[ki]) - 2.0 * U * np.abs(Td[ki])
    check = float(np.max(slack / (64.0 * np.sqrt(N) * U * s[:len(ki)])))
    return T[idx], np.abs(c64[idx] - T[idx]), s, check, col_sha(q)


def main():
    arr, docs, jobs, where = {}, [], [], []
    for gi, (name, kinds, recipes, mean_kind, rows) in enumerate(groups()):
        t, y, dy = lightcurves(recipes)
        N = y.shape[1]
        key = name.replace("/", ".")
        seeds = [7000 + 10 * gi + b for b in range(len(rows))]
        for b, r in enumerate(rows):
            tt = t[r["lc"]] if t.ndim == 2 else t
            jobs.append((name, kinds, mean_kind, np.array(r["theta"]), tt, dy[r["lc"]], seeds[b]))
            where.append((gi, b))
        arr[key + "/idx"] = stored_indices(N)
        arr[key + "/theta"] = np.array([r["theta"] for r in rows])
        arr[key + "/lc"] = np.array([r["lc"] for r in rows], dtype=np.int32)
        docs.append(dict(name=name, kinds=[int(k) for k in kinds], recipes=recipes, mean_kind=mean_kind, N=N,
                         y_offset=[float(v) for v in y.mean(axis=1)],
                         sha256=[sha(*quad_lightcurve(r)) for r in recipes], normal_seeds=seeds))
    order = sorted(range(len(jobs)), key=lambda i: -len(jobs[i][4]))       # the long rows first
    with multiprocessing.Pool(min(8, len(jobs))) as pool:
        res = dict(zip(order, pool.map(row_job, [jobs[i] for i in order], chunksize=1)))
    for i, (gi, b) in enumerate(where):
        T, e64, s, check, qsha = res[i]
        key = docs[gi]["name"].replace("/", ".")
        if not check <= 1e-3:
            raise SystemExit("%s row %d: mpmath recurrence and dense Cholesky disagree at %.3g of the floor" % (docs[gi]["name"], b, check))
        arr.setdefault(key + "/T", []).append(T)
        arr.setdefault(key + "/c64err", []).append(e64.astype(np.float32))
        arr.setdefault(key + "/scale", []).append(s.astype(np.float32))
        docs[gi].setdefault("normal_sha256", []).append(qsha)
        docs[gi].setdefault("dense_check", []).append(max(check, 0.0))
        print("%-28s row %d  N=%-6d stored %-5d rho %.3g  dense check %.2g of the floor"
              % (docs[gi]["name"], b, docs[gi]["N"], len(T), float(np.max(e64 / s)), check), flush=True)
    arr = {k: np.asarray(v) for k, v in arr.items()}
    arr["manifest"] = np.frombuffer(json.dumps(
        {"generator": "tests/golden/make_gp_draw_golden.py", "u": U, "groups": docs}, sort_keys=True).encode(), dtype=np.uint8)
    path = os.path.join(HERE, "gp_draw_golden.npz")
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as z:     # fixed timestamps: a rerun gives the same bytes
        for k in sorted(arr):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arr[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())
    size = os.path.getsize(path)
    print("wrote %s (%d bytes)" % (path, size))
    assert size <= os.path.getsize(os.path.join(HERE, "predict_golden.npz")), "larger than predict_golden.npz"


if __name__ == "__main__":
    main()
