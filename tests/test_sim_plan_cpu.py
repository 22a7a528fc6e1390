"""The simulator's cutting rules (mind_the_gaps_amd/csrc/mtg_sim_plan.h) on the host: tests/sim_plan_driver.cpp, compiled
with g++ against the header alone, prints the layout -- chirp-z or not, transform length, pairs, series per execution,
plan slot, buffer sizes -- for a table of grids and call sizes, and the plan slot the convergence check would take.
Every line is compared with tests/golden/sim_layout.json, recorded from the same driver over the rules as they stood
inside mtg_capi.hip before they moved to the header."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sim_layout.json")

# 254 = 2 x 127: chirp-z with m = 512; 1 087 853: the grid of BASELINE configs[3]
NFFT = [4, 256, 254, 255, 10 ** 4, 1087853, 2 ** 24, 2 ** 30]
SERIES = ["1", "2", "5", "full-1", "full", "full+1", "max"]


def layout_cases():
    cases = ["nfft=%d S=%s transform=%d pairs=%d" % (nfft, s, transform, pairs)
             for nfft in NFFT for s in SERIES for transform in (0, 1, 2) for pairs in (0, 1)]
    # MTG_SIM_BATCH of a measuring build: the forced batch, still within the 2 GiB of one execution
    cases += ["nfft=%d S=%s transform=0 pairs=1 env=%d" % (nfft, s, env)
              for nfft in (256, 2 ** 24) for s in ("1", "full", "full+1", "max") for env in (7, 1000)]
    return cases


def lru_cases():
    def slots(states):
        return " ".join("slot%d=%d,%d,%d,%d,%d" % ((i,) + st) for i, st in enumerate(states))
    full = [(1, 64, 6 + i, 3, age) for i, age in enumerate((7, 3, 9, 5))]   # distinct ages, the oldest in slot 1
    cases = ["lru=1 want=64,6,3 " + slots([(0, 0, 0, 0, 0)] * 4)]                               # all empty
    cases += ["lru=1 want=64,99,3 " + slots(full[:k] + [(0, 0, 0, 0, 0)] * (4 - k)) for k in (1, 2, 3)]
    cases += ["lru=1 want=64,99,3 " + slots([full[0], (0, 0, 0, 0, 0), full[2], full[3]])]      # a hole in the middle
    cases += ["lru=1 want=64,99,3 " + slots(full)]                                              # full: the oldest goes
    cases += ["lru=1 want=64,99,3 " + slots(full[k:] + full[:k]) for k in (1, 2, 3)]
    cases += ["lru=1 want=64,%d,3 " % (6 + k) + slots(full) for k in range(4)]                  # a hit in every position
    cases += ["lru=1 want=128,6,3 " + slots(full), "lru=1 want=64,6,4 " + slots(full)]          # near misses
    cases += ["lru=1 want=0,0,0 " + slots([(0, 0, 0, 0, 0)] * 4)]                               # an empty slot is no hit
    return cases


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("simplan") / "sim_plan_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I",
                           os.path.join(ROOT, "mind_the_gaps_amd", "csrc"), os.path.join(ROOT, "tests", "sim_plan_driver.cpp"),
                           "-o", exe])

    def run(lines):
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True)
        return r.stdout.splitlines()
    return run


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("which, cases", [("layout", layout_cases()), ("lru", lru_cases())])
def test_matches_the_recorded_rules(driver, golden, which, cases):
    assert [row["in"] for row in golden[which]] == cases, "the golden file does not hold this table"
    outs = driver(cases)
    assert len(outs) == len(cases)
    for row, out in zip(golden[which], outs):
        assert out == row["out"], (row["in"], out, row["out"])


def test_table_reaches_the_decisions(golden):
    """the recorded table is not vacuous: both transforms, both slots, short and full groups, every LRU outcome"""
    rows = {row["in"]: dict(tok.split("=") for tok in row["out"].split()) for row in golden["layout"]}
    assert rows["nfft=254 S=max transform=0 pairs=1"]["m"] == "512" and rows["nfft=254 S=max transform=0 pairs=1"]["czt"] == "1"
    assert rows["nfft=256 S=max transform=0 pairs=1"] == dict(rows["nfft=256 S=full transform=0 pairs=1"], S=str(2 ** 63 - 1))
    assert rows["nfft=256 S=full transform=0 pairs=1"]["chunk"] == "256"
    assert rows["nfft=256 S=full-1 transform=0 pairs=1"]["slot"] == "1" and rows["nfft=256 S=full+1 transform=0 pairs=1"]["slot"] == "0"
    assert rows["nfft=256 S=2 transform=2 pairs=1"]["czt"] == "1" and rows["nfft=254 S=2 transform=1 pairs=1"]["czt"] == "0"
    assert rows["nfft=254 S=5 transform=0 pairs=1"]["batch"] == "3" and rows["nfft=254 S=5 transform=0 pairs=0"]["batch"] == "5"
    assert rows["nfft=1087853 S=max transform=0 pairs=1"]["czt"] == "1"
    assert rows["nfft=%d S=max transform=2 pairs=1" % 2 ** 30]["czt"] == "0"    # a work area beyond 2 GiB: the library's plan
    lru = [row["out"] for row in golden["lru"]]
    assert {"slot=%d hit=1" % k for k in range(4)} <= set(lru) and {"slot=%d hit=0" % k for k in range(4)} <= set(lru)
