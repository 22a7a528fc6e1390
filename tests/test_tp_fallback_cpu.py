"""tests/golden/tp_fallback_golden.json's own conditions (made by tests/golden/make_tp_fallback_golden.py, used by
test_tp_fallback_gpu.py), from the stored numbers and the light-curve recipes alone: no GPU, no oracle."""
import json
import os

import numpy as np
import pytest

import golden_util

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "tp_fallback_golden.json")) as _f:
    GROUPS = json.load(_f)["groups"]
# (model, N) of every family test_tp_fallback_gpu.py launches
WANTED = {"j3/n70", "j3/n1000", "j3/n4096", "j3/n4097", "j4/n70", "j4/n1000", "j4/n4096", "j4/n4097", "null/n1000",
          "null/n4096", "alt/n4096", "5sho/n1024", "5sho/n8192"}


def test_every_family_has_its_group():
    assert {g["name"] for g in GROUPS} == WANTED


@pytest.mark.parametrize("g", GROUPS, ids=[g["name"] for g in GROUPS])
def test_row_classes(g):
    rows = {cls: [r for r in g["rows"] if r["cls"] == cls] for cls in ("healthy", "cancelling", "nonfinite")}
    assert sum(map(len, rows.values())) == len(g["rows"])
    assert len(rows["healthy"]) >= 12 and len(rows["cancelling"]) >= (33 if g["name"].startswith("5sho") else 24)
    for r in rows["cancelling"]:
        T = abs(r["lnL"] + r["lnL_lo"])
        assert r["c64_status"] == 0 and r["lc"] == 0 and T <= 1.0e-6 * r["S"], (g["name"], T, r["S"])
    for r in rows["healthy"]:
        T = abs(r["lnL"] + r["lnL_lo"])
        assert r["c64_status"] == 0 and r["lc"] == 0 and r["S"] <= 10.0 * T, (g["name"], T, r["S"])
    healthy = [r["theta"] for r in rows["healthy"]]
    for r in rows["nonfinite"]:     # MTG_ST_NONFINITE, a healthy theta on the spiked light curve
        assert r["c64_status"] == 3 and r["lc"] == 1 and r["theta"] in healthy
    # every cancelling row was bisected on its own
    assert len({tuple(r["theta"]) for r in rows["cancelling"]}) == len(rows["cancelling"])


@pytest.mark.parametrize("g", GROUPS, ids=[g["name"] for g in GROUPS])
def test_light_curves(g):
    rec = g["lightcurve"]
    t, y, dy = golden_util.quad_lightcurve(rec)
    N = rec["N"]
    assert golden_util.lightcurve_sha256(t, y, dy) == g["sha256"]
    assert y.shape == (2, N) and np.array_equal(dy[0], dy[1])
    differ = np.flatnonzero(y[0] != y[1])
    assert list(differ) == [rec["spike"]] and y[1, rec["spike"]] == 1.0e160
    # neither in the first nor in the last chunk, whatever the lane or chunk count (64, 128, 256 and rank 10's C)
    for chunks in (64, 128, 256):
        per = (N + chunks - 1) // chunks
        last = (N - 1) // per
        assert 0 < rec["spike"] // per < last
    assert g["y_offset"] == [float(y[0].mean())] * 2
