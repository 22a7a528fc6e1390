#!/usr/bin/env python3
"""Generates tests/golden/predict_at_golden.npz: the quad-precision truth (oracle/predict_sweep.h's predict_at in
__float128, through oracle/predict.py) of the prediction at NEW times, for tests/test_predict_at_cpu.py and
tests/test_predict_at_vs_quad_gpu.py.

Groups, light curves and rows are those of make_predict_golden.groups(): every group of tests/golden/quad_golden.json
(up to 4 rows each, picked as pick_rows does; the largest phases of the phase groups) plus the noise_dominated
recipe -- all of them, N = 2e5 with five SHO terms included, not only the two groups whose dense K_* the host path
could afford.  Per group the 48 times of golden_util.new_times(t, 3000 + gi) (between samples, exactly on samples,
before the first and after the last); per row and time the truth T (float64), |c64 - T| and the scales
s_mu = |mean| + sum |k_* K^-1 r|, s_var = k(0) + |k_*^T K^-1 k_*| (float32).  c64 is celerite's dense expression in
float64 with the phase at the absolute time.  mu includes the whole mean, a constant one too.  Each row is also
computed on the time-reversed series in quad; the generator fails if the two disagree by more than 1e-3 of the test's
tolerance anywhere.

Run from the repo root:  python tests/golden/make_predict_at_golden.py   (minutes on 8 cores; deterministic)
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
sys.path.insert(0, HERE)

from oracle import dense  # noqa: E402
from oracle import predict as P  # noqa: E402
from golden_util import lightcurve_sha256 as sha, new_times  # noqa: E402
from golden_util import quad_lightcurve as lightcurve  # noqa: E402
from make_predict_golden import groups  # noqa: E402

U = 2.0 ** -53


def main():
    arr, groups_doc = {}, []
    for gi, (name, kinds, rec, mean_kind, y_offset, rows) in enumerate(groups()):
        t, y, dy = lightcurve(rec)
        L, N = y.shape
        nk = dense.n_kernel_params(kinds)
        key = name.replace("/", ".")
        full = np.array([r["theta"] for r in rows])
        lc = np.array([r["lc"] for r in rows], dtype=np.int32)
        if mean_kind == 0:      # the constant mean is each light curve's y_offset (quad_golden.json's convention)
            full[:, nk] = np.asarray(y_offset)[lc]
        ts = new_times(t, 3000 + gi)
        arr[key + "/ts"], arr[key + "/theta"], arr[key + "/lc"] = ts, full, lc
        worst_fr = 0.0
        for b in range(len(rows)):
            yl, dyl = y[lc[b]], dy[lc[b]]
            pa = P.predict_at(t, yl, dyl, kinds, full[b], ts, mean_kind=mean_kind)
            pr = P.predict_at(t, yl, dyl, kinds, full[b], ts, mean_kind=mean_kind, reverse=True)
            p64 = P.predict_at(t, yl, dyl, kinds, full[b], ts, mean_kind=mean_kind, c64=True)
            assert pa.status == 0 and pr.status == 0 and p64.status == 0, (name, b, pa.status, pr.status, p64.status)
            for v, s in (("mu", "s_mu"), ("var", "s_var")):
                T, lo = getattr(pa, v), getattr(pa, v + "_lo")
                e64 = np.abs((getattr(p64, v) - T) - lo)
                tol = np.maximum(10.0 * e64, 64.0 * np.sqrt(N) * U * getattr(pa, s))
                fr = np.abs((T - getattr(pr, v)) + (lo - getattr(pr, v + "_lo")))
                # (a model without a celerite term has T = mean, scale 0 and tolerance 0: the sweeps must agree exactly)
                worst_fr = max(worst_fr, float(np.max(np.where(tol > 0, fr / np.where(tol > 0, tol, 1.0),
                                                               np.where(fr == 0, 0.0, np.inf)))))
                arr.setdefault("%s/%s" % (key, v), []).append(T)
                arr.setdefault("%s/%s_c64err" % (key, v), []).append(e64.astype(np.float32))
                arr.setdefault("%s/%s_scale" % (key, v), []).append(getattr(pa, s).astype(np.float32))
        if not worst_fr <= 1e-3:
            raise SystemExit("%s: forward / reverse quad predict_at disagree at %.3g of the tolerance" % (name, worst_fr))
        groups_doc.append(dict(
            name=name, kinds=[int(k) for k in kinds], lightcurve=rec, mean_kind=mean_kind,
            y_offset=[float(v) for v in y_offset], sha256=sha(t, y, dy), N=N, fwd_rev=worst_fr, ts_seed=3000 + gi,
            k0=[float(dense.kernel_value(dense.build_coeffs(kinds, full[b, :nk]), 0.0)) for b in range(len(lc))]))
        print("%-28s N=%-6d rows %d  fwd/rev %.2g of tol" % (name, N, len(rows), worst_fr), flush=True)
    arr = {k: np.asarray(v) for k, v in arr.items()}
    arr["manifest"] = np.frombuffer(json.dumps(
        {"generator": "tests/golden/make_predict_at_golden.py", "u": U, "groups": groups_doc},
        sort_keys=True).encode(), dtype=np.uint8)
    # a zip written entry by entry with a fixed timestamp: a rerun gives the same bytes
    path = os.path.join(HERE, "predict_at_golden.npz")
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
