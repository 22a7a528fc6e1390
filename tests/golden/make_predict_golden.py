#!/usr/bin/env python3
"""Generates tests/golden/predict_golden.npz: the quad-precision truth (oracle/predict_sweep.h in __float128, through
oracle/celerite_quad.c) of Engine.predict, Engine.apply_inverse and GP.predict at new times, for
tests/test_predict_vs_quad_gpu.py.

The light curves and parameter vectors are those of tests/golden/quad_golden.json (its recipes and SHA-256 checks,
up to 4 rows of every group: the largest phases of the phase groups, else spread over the group), plus one noise-dominated group (yerr^2 / k(0) between 1e4 and 1e6).  Per-sample arrays
at N = 2e5 do not fit a committed file, so each group stores K = 128 fixed sample indices (all of them below that):
the first 32, the last 32, both sides of the largest gaps, the rest drawn with a fixed seed.  Per row and index: the
truth T (float64), |c64 - T| and the cancellation scale (float32); c64 is the same recurrence in float64 with
celerite's phase at the absolute time (oracle/celerite_ref.c).  Each row is also swept time-reversed in quad; the
generator fails if the two quad sweeps disagree by more than 1e-3 of the test's tolerance anywhere.

apply_inverse (groups APPLY): three columns per row -- the residual y - mean, a standard-normal column and the column
k(t_* - t) of K_*^T at a time t_* inside the largest gap.  The last two are rounded to float32 so that a libm or SIMD
path that differs in the last bit of a double still gives the same column; their SHA-256 is stored and checked.  Per
column: T at the K indices, ||c64 - T||_inf and ||T||_inf over all N.

New times (groups AT): GP.predict(y, t=ts, return_var=True) at 48 times between samples, on samples and beyond both
ends; T, |c64 - T| and the scales k(0) + |k_*^T K^-1 k_*| (variance), |mean| + sum |k_* K^-1 r| (mean).

Run from the repo root:  python tests/golden/make_predict_golden.py   (a few minutes on 8 cores; deterministic)
"""
import io
import json
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

from mind_the_gaps_amd import synthetic as synth  # noqa: E402
from oracle import dense  # noqa: E402
from oracle import predict as P  # noqa: E402
from golden_util import apply_columns, col_sha, lightcurve_sha256 as sha, new_times  # noqa: E402
from golden_util import quad_lightcurve as lightcurve  # noqa: E402

U = 2.0 ** -53
K_IDX = 128
ROWS = 4
APPLY = ["rank10/config5", "phase/j3", "offset/seconds", "long_memory", "linear_mean/j3_seconds",
         "typical/jitter_only"]
AT = ["phase/j3", "offset/seconds"]
NOISE = "noise_dominated"


def sample_indices(t, seed):
    """the first 32, the last 32, both sides of the 16 largest gaps, then seeded draws: K_IDX sorted indices"""
    N = len(t)
    if N <= K_IDX:
        return np.arange(N, dtype=np.int32)
    keep = set(range(32)) | set(range(N - 32, N))
    for g in np.argsort(-np.diff(t), kind="stable")[:16]:
        keep |= {int(g), int(g) + 1}
    rest = np.setdiff1d(np.arange(N), np.fromiter(keep, dtype=np.int64))
    rng = np.random.default_rng(seed)
    keep |= set(int(i) for i in rng.choice(rest, K_IDX - len(keep), replace=False))
    return np.array(sorted(keep), dtype=np.int32)


def pick_rows(rows):
    if len(rows) <= ROWS:
        return list(range(len(rows)))
    return [int(i) for i in np.unique(np.round(np.linspace(0, len(rows) - 1, ROWS)).astype(int))]


def groups():
    """(name, kinds, recipe, mean_kind, y_offset [L], rows [{theta, lc}]) from quad_golden.json, plus NOISE"""
    with open(os.path.join(HERE, "quad_golden.json")) as f:
        gold = json.load(f)["groups"]
    out = []
    for g in gold:
        t, y, dy = lightcurve(g["lightcurve"])
        assert sha(t, y, dy) == g["sha256"], g["name"]
        # the phase groups keep their largest phases per step (1.1e5 .. 1.1e12 rad, both sides of MTG_TRIG_FAST_MAX)
        rows = g["rows"][-ROWS:] if g["regime"] == "phase" else [g["rows"][i] for i in pick_rows(g["rows"])]
        out.append((g["name"], g["kinds"], g["lightcurve"], g.get("mean_kind", 0), g["y_offset"],
                    [dict(theta=r["theta"], lc=r["lc"]) for r in rows]))
    # noise-dominated: the null model's amplitudes scaled so that yerr^2 / k(0) runs over [1e4, 1e6] along the rows
    rec = dict(N=4096, L=1, seed=130, offset=0.0, edit=None)
    t, y, dy = lightcurve(rec)
    kinds = synth.NULL_MODEL
    th0 = synth.truth(kinds)
    k00 = float(dense.kernel_value(dense.build_coeffs(kinds, th0), 0.0))
    e2 = float(np.median((dy[0] + 1e-12) ** 2))
    rows = []
    for ratio in (1e4, 1e5, 1e6, 3e5):
        th = th0.copy()
        th[0] += np.log(e2 / ratio / k00)       # DRW amplitude (log a)
        th[2] += np.log(e2 / ratio / k00)       # SHO log S0
        rows.append(dict(theta=[float(v) for v in th] + [float(y.mean())], lc=0))
    out.append((NOISE, [int(k) for k in kinds], rec, 0, [float(y.mean())], rows))
    return out


def main():
    arr, groups_doc = {}, []
    nthreads = None
    for gi, (name, kinds, rec, mean_kind, y_offset, rows) in enumerate(groups()):
        t, y, dy = lightcurve(rec)
        L, N = y.shape
        nk = dense.n_kernel_params(kinds)
        idx = sample_indices(t, 1000 + gi)
        key = name.replace("/", ".")
        arr[key + "/idx"] = idx
        full = np.array([r["theta"] for r in rows])
        lc = np.array([r["lc"] for r in rows], dtype=np.int32)
        if mean_kind == 0:      # the constant mean is each light curve's y_offset (quad_golden.json's convention)
            full[:, nk] = np.asarray(y_offset)[lc]
        q = P.predict(t, y, dy, kinds, full, lc_index=lc, mean_kind=mean_kind, nthreads=nthreads)
        qr = P.predict(t, y, dy, kinds, full, lc_index=lc, mean_kind=mean_kind, reverse=True, nthreads=nthreads)
        c = P.predict(t, y, dy, kinds, full, lc_index=lc, mean_kind=mean_kind, c64=True, nthreads=nthreads)
        assert np.all(q.status == 0) and np.all(qr.status == 0) and np.all(c.status == 0), (name, q.status, c.status)
        worst_fr = 0.0
        for v, s in (("mu", "s_mu"), ("var", "s_var")):
            T, lo, S = getattr(q, v), getattr(q, v + "_lo"), getattr(q, s)
            e64 = np.abs((getattr(c, v) - T) - lo)
            tol = np.maximum(10.0 * e64, 64.0 * np.sqrt(N) * U * S)
            fr = np.abs((T - getattr(qr, v)) + (lo - getattr(qr, v + "_lo")))
            worst_fr = max(worst_fr, float(np.max(fr / tol)))
            arr["%s/%s" % (key, v)] = T[:, idx]
            arr["%s/%s_c64err" % (key, v)] = e64[:, idx].astype(np.float32)
            arr["%s/%s_scale" % (key, v)] = S[:, idx].astype(np.float32)
        if not worst_fr <= 1e-3:
            raise SystemExit("%s: forward / reverse quad sweeps disagree at %.3g of the tolerance" % (name, worst_fr))
        arr[key + "/theta"] = full
        arr[key + "/lc"] = lc
        doc = dict(name=name, kinds=[int(k) for k in kinds], lightcurve=rec, mean_kind=mean_kind,
                   y_offset=[float(v) for v in y_offset], sha256=sha(t, y, dy), N=N, fwd_rev=worst_fr,
                   k0=[float(dense.kernel_value(dense.build_coeffs(kinds, full[b, :nk]), 0.0)) for b in range(len(lc))],
                   yerr2_median=[float(np.median((dy[l] + 1e-12) ** 2)) for l in lc])
        if name in APPLY:
            shas, xs, e64s, tinf = [], [], [], []
            for b in range(len(rows)):
                B3 = apply_columns(t, y[lc[b]], mean_kind, full[b], nk, kinds, 2000 + 10 * gi + b)
                a = P.apply_inverse(t, dy[lc[b]], kinds, full[b], B3, nthreads=nthreads)
                ar = P.apply_inverse(t, dy[lc[b]], kinds, full[b], B3, reverse=True, nthreads=nthreads)
                a64 = P.apply_inverse(t, dy[lc[b]], kinds, full[b], B3, c64=True, nthreads=nthreads)
                assert a.status == 0 and ar.status == 0 and a64.status == 0, name
                e64 = np.max(np.abs((a64.x - a.x) - a.x_lo), axis=0)
                ti = np.max(np.abs(a.x), axis=0)
                tol = np.maximum(10.0 * e64, 64.0 * np.sqrt(N) * U * ti)
                fr = np.max(np.abs((a.x - ar.x) + (a.x_lo - ar.x_lo)), axis=0)
                if not np.all(fr <= 1e-3 * tol):
                    raise SystemExit("%s: apply_inverse forward / reverse disagree (%s against %s)" % (name, fr, tol))
                shas.append([col_sha(B3[:, 1]), col_sha(B3[:, 2])])
                xs.append(a.x[idx].T)
                e64s.append(e64)
                tinf.append(ti)
            arr[key + "/apply_x"] = np.array(xs)                            # [B][3][K]
            arr[key + "/apply_c64err"] = np.array(e64s, dtype=np.float32)   # [B][3]
            arr[key + "/apply_tinf"] = np.array(tinf, dtype=np.float32)     # [B][3]
            doc["apply_sha256"] = shas
            doc["apply_seed"] = [2000 + 10 * gi + b for b in range(len(rows))]
        if name in AT:
            ts = new_times(t, 3000 + gi)
            arr[key + "/ts"] = ts
            for b in range(len(rows)):
                yl, dyl = y[lc[b]], dy[lc[b]]
                pa = P.predict_at(t, yl, dyl, kinds, full[b], ts, mean_kind=mean_kind, nthreads=nthreads)
                pr = P.predict_at(t, yl, dyl, kinds, full[b], ts, mean_kind=mean_kind, reverse=True,
                                  nthreads=nthreads)
                p64 = P.predict_at(t, yl, dyl, kinds, full[b], ts, mean_kind=mean_kind, c64=True, nthreads=nthreads)
                assert pa.status == 0 and pr.status == 0 and p64.status == 0, name
                for v, s in (("mu", "s_mu"), ("var", "s_var")):
                    T, lo = getattr(pa, v), getattr(pa, v + "_lo")
                    e64 = np.abs((getattr(p64, v) - T) - lo)
                    tol = np.maximum(10.0 * e64, 64.0 * np.sqrt(N) * U * getattr(pa, s))
                    fr = np.abs((T - getattr(pr, v)) + (lo - getattr(pr, v + "_lo")))
                    if not np.all(fr <= 1e-3 * tol):
                        raise SystemExit("%s: predict_at forward / reverse disagree" % name)
                    arr.setdefault("%s/at_%s" % (key, v), []).append(T)
                    arr.setdefault("%s/at_%s_c64err" % (key, v), []).append(e64.astype(np.float32))
                    arr.setdefault("%s/at_%s_scale" % (key, v), []).append(getattr(pa, s).astype(np.float32))
        groups_doc.append(doc)
        print("%-28s N=%-6d rows %d  fwd/rev %.2g of tol%s%s" % (name, N, len(rows), worst_fr,
                                                                 "  +apply" if name in APPLY else "",
                                                                 "  +at" if name in AT else ""), flush=True)
    arr = {k: np.asarray(v) for k, v in arr.items()}
    arr["manifest"] = np.frombuffer(json.dumps(
        {"generator": "tests/golden/make_predict_golden.py", "u": U, "groups": groups_doc},
        sort_keys=True).encode(), dtype=np.uint8)
    # a zip written entry by entry with a fixed timestamp: a rerun gives the same bytes
    path = os.path.join(HERE, "predict_golden.npz")
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arr):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arr[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
