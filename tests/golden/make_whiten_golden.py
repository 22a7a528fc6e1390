#!/usr/bin/env python3
"""Generates tests/golden/whiten_golden.npz: the truth of Engine.whiten, for tests/test_whiten_cpu.py and
tests/test_whiten_gpu.py.

Truth T: the recurrence q = D^-1/2 L^-1 (y - mean) of csrc/mtg_whiten.hip in mpmath at 40 digits with the phases at the
absolute time (tests/whiten_replay.mp_whiten), rounded to float64.  The generator checks it against the mpmath dense
Cholesky (50 digits; q solves chol(K) q = y - mean by forward substitution) on the first 64 samples of every row -- a
residual's first samples do not depend on the later ones -- and fails if the two differ by more than 1e-3 of the test's
floor 64 sqrt(N) u s.  T is kept at no more than 64 samples of a row, evenly spread, the first and the last among them.
Next to it: the scale s_n = (|r_n| + sum_i |U_ni f_ni|) / sqrt(D_n) from the truth, and |c64 - T| with c64 the same
recurrence in float64 with celerite's phase at the absolute time (gp_draw_replay.whiten on
factor(phase="absolute", compensated=False)), float32 both; per row the truths of sum q .. sum q^4, of sum ln D and of
sum |ln D|, and c64's errors of sum q^2 and sum ln D.

Light curves are golden_util.quad_lightcurve recipes (regenerated, SHA-256 in the manifest); the data whitened are the
recipe's own y minus the light curve's average (the y_offset, which a given y excludes); a linear mean is part of the
model.  Groups: white (J = 0), DRW (1), DRW + SHO at Q = 3 (3), an over-damped SHO at Q = 0.1 (two real slots), the
headline model DRW + SHO + Lorentzian with its null real term (6) at N = 1000, five SHO terms (10), a fitted linear mean
with a jitter term, and a time offset of 5e8.  N = 256 but for the headline model.

Run from the repo root:  python tests/golden/make_whiten_golden.py   (a few seconds; deterministic)
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
import whiten_replay as WR  # noqa: E402
from golden_util import lightcurve_sha256 as sha  # noqa: E402
from golden_util import quad_lightcurve  # noqa: E402
from mind_the_gaps_amd import synthetic as synth  # noqa: E402
from oracle import dense  # noqa: E402

U = 2.0 ** -53
STORED = 64
CHECK_N = 64


def groups():
    """(name, kinds, recipe, mean_kind, theta (kernel, then the line's slope and intercept))"""
    null = [float(v) for v in synth.truth(synth.NULL_MODEL)]
    alt = [float(v) for v in synth.truth(synth.ALT_MODEL)]
    sho = synth.TRUTH[synth.K_SHO]
    with open(os.path.join(HERE, "quad_golden.json")) as f:
        five = {x["name"]: x for x in json.load(f)["groups"]}["typical/5sho"]
    rec = lambda seed, N=256, offset=0.0: dict(N=N, L=1, seed=seed, offset=offset, edit=None)
    return [
        ("white", [synth.K_JITTER], rec(401), 0, [float(v) for v in synth.TRUTH[synth.K_JITTER]]),
        ("drw", [synth.K_DRW], rec(402), 0, [float(v) for v in synth.TRUTH[synth.K_DRW]]),
        ("drw+sho_q3", list(synth.NULL_MODEL), rec(403), 0, null),
        ("sho_overdamped_q0.1", [synth.K_SHO], rec(404), 0, [float(sho[0]), float(np.log(0.1)), float(sho[2])]),
        ("headline/n1000", list(synth.ALT_MODEL), rec(405, N=1000), 0, alt),
        ("5sho", [int(k) for k in five["kinds"]], dict(five["lightcurve"], N=256, L=1), 0,
         [float(v) for v in five["rows"][0]["theta"][:-1]]),
        ("linear_mean+jitter", list(synth.NULL_MODEL) + [synth.K_JITTER], rec(406, offset=5.0e8), 1,
         null + [-0.5, 2.0e-3, 100.0 - 2.0e-3 * 5.0e8]),
        ("offset/5e8", list(synth.NULL_MODEL), rec(407, offset=5.0e8), 0, null),
    ]


def stored_indices(N):
    return np.unique(np.rint(np.linspace(0, N - 1, min(N, STORED)))).astype(np.int32)


def data_of(recipe, mean_kind):
    """(t, the data the device whitens, dy, y_offset): a constant mean travels as y_offset; under a linear mean the data
    are the recipe's y as they are"""
    t, y, dy = quad_lightcurve(recipe)
    off = 0.0 if mean_kind == 1 else float(y[0].mean())
    return t, y[0] - off, dy[0], off


def row_job(job):
    name, kinds, recipe, mean_kind, theta = job
    theta = np.array(theta)
    t, y, dy, _ = data_of(recipe, mean_kind)
    N = len(t)
    nk = dense.n_kernel_params(kinds)
    coeffs = dense.build_coeffs(kinds, theta[:nk])
    mp_mean = tuple(theta[nk:nk + 2]) if mean_kind == 1 else (0.0,)
    mean = theta[nk] * t + theta[nk + 1] if mean_kind == 1 else 0.0
    idx = stored_indices(N)
    tr, status = WR.mp_whiten(t, dy, coeffs, y, mean_kind=mean_kind, mean_params=mp_mean, dps=40)
    assert status == 0, name
    fac = R.factor(t, R.diagonal(dy, coeffs), coeffs, phase="absolute", compensated=False)
    c64 = R.whiten(t, dy, coeffs, y, mean=mean, factors=fac)
    n = min(N, CHECK_N)
    Td = WR.mp_dense_whiten(t[:n], dy[:n], coeffs, y[:n], mean_kind=mean_kind, mean_params=mp_mean, dps=50)
    # both are rounded to float64: up to an ulp of q apart
    slack = np.abs(tr["q"][:n] - Td) - 2.0 * U * np.abs(Td)
    check = float(np.max(slack / (64.0 * np.sqrt(N) * U * tr["scale"][:n])))
    sums = np.array([tr["sum1"], tr["sum2"], tr["logdet"], tr["sum3"], tr["sum4"], tr["logdet_abs"]])
    sums64 = np.array([abs(float(np.sum(c64 * c64)) - tr["sum2"]), abs(float(np.sum(np.log(fac[3]))) - tr["logdet"])])
    return tr["q"][idx], np.abs(c64[idx] - tr["q"][idx]), tr["scale"][idx], sums, sums64, check


def main():
    gs = groups()
    with multiprocessing.Pool(min(8, len(gs))) as pool:
        res = pool.map(row_job, gs, chunksize=1)
    arr, docs = {}, []
    for (name, kinds, recipe, mean_kind, theta), (T, e64, s, sums, sums64, check) in zip(gs, res):
        if not check <= 1e-3:
            raise SystemExit("%s: mpmath recurrence and dense Cholesky disagree at %.3g of the floor" % (name, check))
        t, y, dy, off = data_of(recipe, mean_kind)
        key = name.replace("/", ".")
        arr[key + "/idx"] = stored_indices(len(t))
        arr[key + "/theta"] = np.array([theta])
        arr[key + "/T"] = T[None, :]
        arr[key + "/c64err"] = e64.astype(np.float32)[None, :]
        arr[key + "/scale"] = s.astype(np.float32)[None, :]
        arr[key + "/sums"] = sums[None, :]
        arr[key + "/sums_c64err"] = sums64[None, :]
        docs.append(dict(name=name, kinds=[int(k) for k in kinds], recipes=[recipe], mean_kind=mean_kind, N=len(t),
                         y_offset=[off], sha256=[sha(*quad_lightcurve(recipe))], dense_check=max(check, 0.0)))
        print("%-22s N=%-5d stored %-3d rho %.3g  dense check %.2g of the floor" % (name, len(t), len(T), float(np.max(e64 / s)), check),
              flush=True)
    arr["manifest"] = np.frombuffer(json.dumps(
        {"generator": "tests/golden/make_whiten_golden.py", "u": U, "groups": docs}, sort_keys=True).encode(), dtype=np.uint8)
    path = os.path.join(HERE, "whiten_golden.npz")
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as z:     # fixed timestamps: a rerun gives the same bytes
        for k in sorted(arr):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arr[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())
    size = os.path.getsize(path)
    print("wrote %s (%d bytes)" % (path, size))
    assert size <= os.path.getsize(os.path.join(HERE, "gp_draw_golden.npz")), "larger than gp_draw_golden.npz"


if __name__ == "__main__":
    main()
