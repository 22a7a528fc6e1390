"""The solve planner (mind_the_gaps_amd/csrc/mtg_solve_plan.h) on the host: tests/solve_plan_driver.cpp, compiled with
g++ against the header alone, runs a boundary table -- one step on each side of every crossover, the mode switches,
and shapes taken out of the catalogue -- and every row's family, sort, fan-out, rank-10 chunk count and kernel name
are checked."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DEFAULTS = dict(N=4096, B=1000, L=4, nr0=1, nc0=1, nsig=1, b0=0, tp=2, pipe=2, sort=2, may_sort=1, grouped=0, no_prior=0,
                free_b=0, in_window=1, cus=256)
P = 128 * 256   # MTG_PIPE_ROWS_PER_CU x compute units


def S(name):
    return dict(family="structures", name=name)


# (inputs that differ from DEFAULTS, expected decisions)
CASES = [
    # time-parallel crossovers, J <= 6 (on Bw); wide four-wave form at <= 512 (J <= 3) / 256 rows and N >= 4096
    (dict(B=12288), dict(S("mtg_tp_kernel<1,1,64>"), sort=0)),
    (dict(B=12289), dict(family="pipe", sort=1, name="mtg_pipe_kernel<1,1,1,0>")),
    (dict(nc0=2, B=8192), S("mtg_tp_kernel<1,2,64>")),
    (dict(nc0=2, B=8193), dict(family="pipe", name="mtg_pipe_kernel<1,2,1,0>")),
    (dict(N=4095, B=4096), S("mtg_tp_kernel<1,1,64>")),
    (dict(N=4095, B=4097), dict(family="pipe")),
    (dict(N=256, B=4096), S("mtg_tp_kernel<1,1,64>")),
    (dict(N=255, B=16), dict(S("mtg_solve_kernel<1,1,0>"), sort=0)),
    (dict(B=512), S("mtg_tp_kernel<1,1,256>")),
    (dict(B=513), S("mtg_tp_kernel<1,1,64>")),
    (dict(N=4095, B=512), S("mtg_tp_kernel<1,1,64>")),
    (dict(nr0=2, nc0=1, B=256), S("mtg_tp_kernel<2,1,256>")),
    (dict(nr0=2, nc0=1, B=257), S("mtg_tp_kernel<2,1,64>")),
    (dict(nr0=2, nc0=2, B=256), S("mtg_tp_kernel<2,2,64>")),                      # J = 6: no wide kernel compiled
    (dict(B=20000, Bw=12288), S("mtg_tp_kernel<1,1,64>")),                        # pays and wide look at Bw ...
    (dict(B=20000, Bw=512), S("mtg_tp_kernel<1,1,256>")),
    (dict(tp=0, N=256, B=P), dict(family="pipe")),                               # ... the pipe limit at B
    (dict(tp=0, N=256, B=P + 1), dict(S("mtg_solve_kernel<1,1,0>"), sort=1)),
    (dict(tp=0, N=256, B=P + 1, Bw=100), dict(S("mtg_solve_kernel<1,1,0>"), sort=1)),
    # modes
    (dict(tp=1, N=100, B=100000), S("mtg_tp_kernel<1,1,64>")),
    (dict(tp=0, pipe=0), S("mtg_solve_kernel<1,1,0>")),
    (dict(tp=3, B=256), S("mtg_tp_kernel<1,1,64>")),
    (dict(tp=2, nr0=0, nc0=0), dict(S("mtg_white_kernel"), sort=1)),
    (dict(tp=1, nr0=0, nc0=0), S("mtg_white_kernel")),
    # the time-parallel kernels are forbidden for a free b without the prior
    (dict(B=256, free_b=1, no_prior=1), dict(family="pipe", name="mtg_pipe_kernel<1,1,1,0>")),
    (dict(B=256, free_b=1), S("mtg_tp_kernel<1,1,256>")),
    (dict(B=256, no_prior=1), S("mtg_tp_kernel<1,1,256>")),
    # the pipelined sweep: N, window, modes, catalogue
    (dict(tp=0, pipe=1, N=64, B=100000), dict(family="pipe")),
    (dict(tp=0, pipe=1, N=63, B=100000), S("mtg_solve_kernel<1,1,0>")),
    (dict(tp=0, N=255, B=5000), S("mtg_solve_kernel<1,1,0>")),
    (dict(tp=0, pipe=1, in_window=0), S("mtg_solve_kernel<1,1,0>")),
    (dict(tp=0, no="pipe"), S("mtg_solve_kernel<1,1,0>")),
    (dict(tp=0, b0=1), dict(family="pipe", name="mtg_pipe_kernel<1,1,1,1>")),
    (dict(tp=0, pipe=0, b0=1), S("mtg_solve_kernel<1,1,1>")),
    (dict(tp=0, pipe=0, b0=1, nr0=5, nc0=0), S("mtg_solve_kernel<5,0,0>")),       # no b = 0 form of this shape
    # the order: for the light curves (arbitrary order, L > 1) or for the structures (nsig > 1); never at <= 64 rows
    (dict(tp=0, pipe=0, grouped=1), dict(sort=0)),
    (dict(tp=0, pipe=0, grouped=1, sort=1), dict(sort=1)),
    (dict(tp=0, pipe=0, may_sort=0), dict(sort=0)),
    (dict(tp=0, pipe=0, L=1), dict(sort=0)),
    (dict(tp=0, pipe=0, sort=0), dict(sort=0)),
    (dict(tp=0, pipe=0, B=64), dict(sort=0)),
    (dict(tp=0, pipe=0, B=65), dict(sort=1)),
    # two structures: fused time-parallel (256 / 128 / 64 lanes), pipe and multi only on a sorted order, else fan-out
    (dict(nsig=2, nc0=2, B=256), dict(family="tp_fused", lanes=256, name="mtg_tp_fused_kernel<1,2,2,256>")),
    (dict(nsig=2, nc0=2, B=257), dict(family="tp_fused", lanes=128, name="mtg_tp_fused_kernel<1,2,2,128>")),
    (dict(nsig=2, nc0=2, B=512), dict(family="tp_fused", lanes=128)),
    (dict(nsig=2, nc0=2, B=513), dict(family="tp_fused", lanes=64)),
    (dict(nsig=2, nc0=2, B=512, N=4095), dict(family="tp_fused", lanes=64)),
    (dict(nsig=2, B=300), dict(family="tp_fused", lanes=256)),                    # J = 3: wide up to 512, no mid
    (dict(nsig=2, B=513), dict(family="tp_fused", lanes=64)),
    (dict(nsig=2, nc0=2, B=256, tp=3), dict(family="tp_fused", lanes=64)),
    (dict(nsig=2, nc0=2, B=256, no="fused256"), dict(family="tp_fused", lanes=64)),   # mid is off where wide is on
    (dict(nsig=2, nc0=2, B=300, no="fused128"), dict(family="tp_fused", lanes=64)),
    (dict(nsig=2, B=300, no="fused64,fused128,fused256", fan_out_knob=0),
     dict(family="structures", fan_out=1, kernels="tp_wide:-1,tp_wide:0", name="mtg_tp_kernel<1,1,256>")),
    (dict(nsig=2, tp=0, B=1000), dict(family="pipe", sort=1, name="mtg_pipe_kernel<1,1,2,0>")),
    (dict(nsig=2, tp=0, B=1000, sort=0), dict(family="structures", sort=0, fan_out=1, name="mtg_solve_kernel<1,1,0>")),
    (dict(nsig=2, tp=0, B=64), dict(family="structures", sort=0, fan_out=1)),
    (dict(nsig=2, tp=0, B=65), dict(family="pipe", sort=1)),
    (dict(nsig=2, tp=0, B=65, may_sort=0), dict(family="pipe", sort=1)),
    (dict(nsig=2, tp=0, B=1000, L=0x3FFFFFFF), dict(family="pipe", sort=1)),      # sort key overflow guard
    (dict(nsig=2, tp=0, B=1000, L=0x40000000), dict(family="structures", sort=0)),
    (dict(nsig=2, N=256, B=P + 1), dict(family="multi", sort=1, name="mtg_solve_kernel_multi<1,1,2,0>")),
    (dict(nsig=2, N=256, B=P + 1, in_window=0), dict(family="structures", sort=1, fan_out=1)),
    (dict(nsig=2, N=256, B=P + 1, multi_knob=0), dict(family="structures", sort=1, fan_out=1)),
    (dict(nsig=2, N=256, B=P + 1, fan_out_knob=0, no="multi"),
     dict(family="structures", sort=1, fan_out=0, kernels="sweep:-1,sweep:-1")),
    # fan-out skips a structure without a sweep kernel; the name is structure 0's
    (dict(nsig=3, nc0=2, tp=0, B=1000, sort=0, no="sweep1"),
     dict(family="structures", fan_out=1, kernels="sweep:-1,none:0,sweep:1", name="mtg_solve_kernel<1,2,0>")),
    (dict(nsig=3, nc0=2, tp=0, B=1000, sort=0, b0=1), dict(name="mtg_solve_kernel<1,2,1>")),
    # rank 10 (five SHO terms)
    (dict(nr0=0, nc0=5, nsig=6, N=1024, B=64),
     dict(family="tp_big", C=64, g=4, name="mtg_tpb_compose4q_kernel (+ mtg_tpb_reduce_kernel<10>, C = 64)")),
    (dict(nr0=0, nc0=5, nsig=6, N=1023, B=64), dict(family="structures", sort=0, fan_out=1, C=0,
                                                   name="mtg_solve_kernel<0,5,0>")),
    (dict(nr0=0, nc0=5, nsig=6, N=1023, B=65), dict(family="structures", sort=1, fan_out=1)),
    (dict(nr0=0, nc0=5, nsig=6, N=1024, B=8192), dict(family="tp_big", C=64)),
    (dict(nr0=0, nc0=5, nsig=6, N=1024, B=8193), dict(family="structures", C=0)),
    (dict(nr0=0, nc0=5, nsig=6, N=1024, B=64, tp=3), dict(family="structures")),
    (dict(nr0=0, nc0=5, nsig=6, N=1024, B=64, no="tp"), dict(family="structures")),
    (dict(nr0=0, nc0=5, nsig=6, N=100000, B=16), dict(family="tp_big", C=1024)),
    (dict(nr0=0, nc0=5, nsig=6, N=100000, B=17), dict(family="tp_big", C=2048)),
    (dict(nr0=0, nc0=5, nsig=6, N=100000, B=16, chunk_target=4096), dict(family="tp_big", C=256)),
    (dict(nr0=0, nc0=5, nsig=6, N=100000, B=16, chunk_target=63), dict(family="tp_big", C=1024)),
    (dict(nr0=0, nc0=5, nsig=6, N=100000, B=16, gsize=8), dict(family="tp_big", g=8)),
    (dict(nr0=0, nc0=5, nsig=6, N=100000, B=16, gsize=5), dict(family="tp_big", g=4)),
    (dict(nr0=0, nc0=5, nsig=6, N=1024, B=20000, Bw=8192), dict(family="tp_big")),
    (dict(nr0=0, nc0=5, nsig=6, N=1024, B=50000, tp=1), dict(family="tp_big", C=64)),   # workspace 14.6 GB
    (dict(nr0=0, nc0=5, nsig=6, N=1024, B=65000, tp=1), dict(family="structures")),     # 19.0 GB > 16 GiB
]

SPEC = [  # (tp_mode, nr0, nc0, N, rows3) -> mtg_ensemble_run speculates
    ((2, 1, 2, 4096, 512), 1), ((2, 1, 2, 4096, 513), 0), ((2, 2, 2, 4096, 256), 1), ((2, 2, 2, 4096, 257), 0),
    ((2, 1, 1, 4095, 1024), 1), ((2, 1, 1, 4095, 1025), 0), ((2, 1, 1, 255, 100), 0), ((0, 1, 1, 4096, 100), 0),
    ((3, 1, 1, 4096, 100), 1), ((2, 1, 3, 4096, 100), 0),
]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan") / "solve_plan_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I",
                           os.path.join(ROOT, "mind_the_gaps_amd", "csrc"), os.path.join(ROOT, "tests", "solve_plan_driver.cpp"),
                           "-o", exe])

    def run(lines):
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True)
        return r.stdout.splitlines()
    return run


def line(inputs):
    return " ".join("%s=%s" % kv for kv in dict(DEFAULTS, **inputs).items())


def parse(out):
    head, name = out.split(" name=", 1)
    d = dict(tok.split("=", 1) for tok in head.split())
    d["name"] = name
    return d


def test_boundary_table(driver):
    outs = driver([line(inputs) for inputs, _ in CASES])
    assert len(outs) == len(CASES)
    for (inputs, want), out in zip(CASES, outs):
        got = parse(out)
        for key, value in want.items():
            assert got[key] == str(value), (inputs, key, got)


def test_speculation(driver):
    outs = driver(["tp=%d nr0=%d nc0=%d N=%d B=%d spec=1" % args for args, _ in SPEC])
    assert outs == ["spec=%d" % want for _, want in SPEC]
