"""Loaders for tests/golden/loglike_golden.{json,npz} (made by tests/golden/make_golden.py) and the light curves of
tests/golden/quad_golden.json (made by tests/golden/make_quad_golden.py)."""
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
    sampling if any ("dup_gap": repeated epochs, dx = 0, every N / 7 samples and a gap of 1e6 days after the middle)."""
    from mind_the_gaps_amd import synthetic as synth
    t, y, dy = synth.make_lightcurves(rec["N"], rec["L"], rec["seed"], rec["offset"])
    edit = rec.get("edit")
    if edit == "dup_gap":
        t = t.copy()
        for i in range(10, rec["N"] - 1, rec["N"] // 7):
            t[i + 1] = t[i]
        t[rec["N"] // 2:] += 1.0e6
    elif edit is not None:
        raise ValueError(edit)
    return t, y, dy


def lightcurve_sha256(t, y, dy):
    h = hashlib.sha256()
    for a in (t, y, dy):
        h.update(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    return h.hexdigest()
