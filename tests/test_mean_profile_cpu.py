"""The profile means (sine, two sines, Gaussian) without a GPU: the header's constants and mtg_mean_nparams, the
planner with MtgPlanIn::profile_mean set and clear (tests/mean_plan_driver.cpp), and what DeviceModel hands
mtg_set_model for the three classes."""
import os
import re
import subprocess

import numpy as np
import pytest

from mind_the_gaps_amd import engine
from mind_the_gaps_amd.gp import DeviceModel
from mind_the_gaps_amd.models import DampedRandomWalk, GaussianModel, SineModel, TwoSineModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_constants_and_mean_nparams():
    text = open(os.path.join(ROOT, "include", "mtg.h")).read()
    defs = dict(re.findall(r"#define\s+(MTG_\w+)\s+\(?(-?\d+)\)?", text))
    for name, value in (("MTG_MEAN_CONSTANT", engine.MEAN_CONSTANT), ("MTG_MEAN_LINEAR", engine.MEAN_LINEAR),
                        ("MTG_MEAN_SINE", engine.MEAN_SINE), ("MTG_MEAN_TWOSINE", engine.MEAN_TWOSINE),
                        ("MTG_MEAN_GAUSSIAN", engine.MEAN_GAUSSIAN)):
        assert int(defs[name]) == value, name
    lib = engine.load_library()
    assert [lib.mtg_mean_nparams(k) for k in range(5)] == [1, 2, 4, 6, 4]
    assert [lib.mtg_mean_nparams(k) for k in range(5)] == [engine.MEAN_NPARAMS[k] for k in range(5)]
    assert lib.mtg_mean_nparams(5) == -1 and lib.mtg_mean_nparams(-1) == -1


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan") / "mean_plan_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "mind_the_gaps_amd", "csrc"),
                           os.path.join(ROOT, "tests", "mean_plan_driver.cpp"), "-o", exe])
    return subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines()


def test_without_the_field_every_plan_is_the_parents(plans):
    want = open(os.path.join(ROOT, "tests", "golden", "mean_plan_parent.txt")).read().splitlines()
    got = [line for line in plans if line.startswith("plain ")]
    assert len(want) == 576 and got == want


def test_with_the_field_the_plan_is_the_sweep_of_every_structure(plans):
    lines = [line for line in plans if line.startswith("profile ")]
    assert len(lines) == 576
    for line in lines:
        shape, plan = line.split(" : ")
        keys = dict(tok.split("=") for tok in shape.split()[1:])
        out = dict(tok.split("=", 1) for tok in plan.split())
        nsig, nr0, nc0 = int(keys["nsig"]), int(keys["nr0"]), int(keys["nc0"])
        assert out["family"] == "structures" and out["C"] == "0" and out["lanes"] == "0", line
        kernels = out["kernels"].split(",")
        assert len(kernels) == nsig and all(k.startswith("sweep:") for k in kernels), line
        assert out["fan_out"] == ("1" if nsig > 1 else "0"), line
        b0 = int(keys["b0"] == "1" and 0 < nc0 < 4 and nr0 < 5 and nr0 + 2 * nc0 <= 6)
        name = "mtg_white_mean_kernel" if nr0 + nc0 == 0 else "mtg_solve_mean_kernel<%d,%d,%d>" % (nr0, nc0, b0)
        assert out["name"] == name, line
    # the order is sorted exactly where the plain sweep's is (tp_mode = pipe_mode = 0: the plain plan is the sweep too)
    plain = {l.split(" : ")[0][6:]: l for l in plans if l.startswith("plain ") and " tp=0 pipe=0 " in l}
    for line in lines:
        if " tp=0 pipe=0 " in line:
            want = plain[line.split(" : ")[0][8:]]
            if "family=structures" in want:
                assert re.search(r"sort=\d", line).group() == re.search(r"sort=\d", want).group(), line


KERNEL = lambda: DampedRandomWalk(log_S0=0.3, log_omega0=-1.2, bounds=[(-10, 10), (-10, 10)])


def test_device_model_kinds_and_parameter_order():
    sine = SineModel(3.0, 0.8, 0.25, 0.7, bounds=[(0, 6), (0, 5), (0.1, 1.0), (-4, 4)])
    two = TwoSineModel(3.0, 0.8, 0.7, 0.35, -1.1, 0.25)
    gauss = GaussianModel(60.0, 2.5, 10.0, 3.1)
    for mean, kind, names, values in (
            (sine, engine.MEAN_SINE, ("constant", "amplitude", "frequency", "phase"), [3.0, 0.8, 0.25, 0.7]),
            (two, engine.MEAN_TWOSINE, ("constant", "amplitude0", "phase0", "amplitude1", "phase1", "frequency"),
             [3.0, 0.8, 0.7, 0.35, -1.1, 0.25]),
            (gauss, engine.MEAN_GAUSSIAN, ("mean", "sigma", "amplitude", "constant"), [60.0, 2.5, 10.0, 3.1])):
        model = DeviceModel(KERNEL(), mean, mean.unfrozen_mask)
        assert model.mean_kind == kind and mean.parameter_names == names
        assert len(names) == engine.MEAN_NPARAMS[kind]
        assert model.nk == 2 and list(model.full[2:]) == values and model.y_offset is None
        assert list(model.free_index) == list(range(2 + len(names)))
    model = DeviceModel(KERNEL(), sine, sine.unfrozen_mask)
    assert np.array_equal(model.bounds[2:], [[0, 6], [0, 5], [0.1, 1.0], [-4, 4]])


def test_partly_frozen_mean_gives_the_right_free_index():
    gauss = GaussianModel(60.0, 2.5, 10.0, 3.1)
    gauss.freeze_parameter("sigma")
    gauss.freeze_parameter("constant")
    model = DeviceModel(KERNEL(), gauss, gauss.unfrozen_mask)
    assert list(model.free_index) == [0, 1, 2, 4] and model.y_offset is None
    assert list(model.full) == [0.3, -1.2, 60.0, 2.5, 10.0, 3.1]


def test_mean_values_against_the_formulas():
    x = np.array([0.0, 1.5, 50.25, 1.0e4])
    two = TwoSineModel(3.0, 0.8, 0.7, 0.35, -1.1, 0.25)
    assert np.array_equal(two.get_value(x), 3.0 + 0.8 * np.sin(0.25 * x + 0.7) + 0.35 * np.sin(2 * 0.25 * x + -1.1))
    gauss = GaussianModel(60.0, 2.5, 10.0, 3.1)       # the reference's normalisation: 2 pi sigma
    assert np.array_equal(gauss.get_value(x), 10.0 / (2 * np.pi * 2.5) * np.exp(-(x - 60.0) ** 2 / (2 * 2.5 ** 2)) + 3.1)
    sine = SineModel(3.0, 0.8, 0.25, 0.7)
    assert np.array_equal(sine.get_value(x), 3.0 + 0.8 * np.sin(0.25 * x + 0.7))
