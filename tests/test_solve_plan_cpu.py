"""The solve planner (mind_the_gaps_amd/csrc/mtg_solve_plan.h) on the host: tests/solve_plan_driver.cpp, compiled with
g++ against the header alone, runs a boundary table -- one step on each side of every crossover, the mode switches,
and shapes taken out of the catalogue -- and every row's family, sort, fan-out, rank-10 chunk count and kernel name
are checked.  The device sampler's run plan (mtg_plan_ensemble_run) gets a table of the same kind, and its schedule
(mtg_ensemble_step) is compared launch by launch with rows written out by hand from the loops it replaced.  The rows per
slab of mtg_predict_at and mtg_gp_draw (mtg_plan_predict_at_slab, mtg_plan_draw_slab) get a boundary table worked out by
hand from the formulas the two entries carried inline."""
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

# mtg_plan_ensemble_run.  Defaults: one ensemble of 8 walkers (half-steps of 4 rows, 12 in a speculative iteration),
# 3 steps, J = 3, N = 4096, modes auto, unsharded.  3 E W/2 is a multiple of three, so the row limits of
# mtg_plan_speculate (1024, 512, 256; SPEC above has them to the row) are met from the nearest shapes on either side.
RUN_DEFAULTS = dict(E=1, W=8, steps=3, tp=2, spec_mode=1, nr0=1, nc0=1, N=4096, shard=0, lo=0, hi=0)
SEQ = dict(speculative=0, up_front=0, rows=4, solves=6, live=0, perm_bytes=0)
RUN = [
    (dict(spec_mode=0), SEQ),
    (dict(spec_mode=1), dict(speculative=1, up_front=1, rows=12, solves=3, live=0, perm_bytes=3 * 8 * 4)),
    (dict(spec_mode=2), dict(speculative=1, up_front=0, rows=12, solves=3, live=0, perm_bytes=0)),
    (dict(tp=0), SEQ),
    (dict(steps=0), dict(speculative=0, up_front=0, rows=4, solves=0, perm_bytes=0)),
    (dict(steps=1), dict(speculative=1, up_front=1, solves=1, perm_bytes=32)),
    # the splits up front: one row of workgroups per step, 64 MiB at the most
    (dict(steps=65535), dict(speculative=1, up_front=1, solves=65535, perm_bytes=65535 * 32)),
    (dict(steps=65536), dict(speculative=1, up_front=0, solves=65536, perm_bytes=0)),
    (dict(N=256, W=512, steps=32768), dict(speculative=1, up_front=1, rows=768, perm_bytes=64 << 20)),
    # (4 bytes over takes an odd number of walkers, which mtg_ensemble_init refuses and the planner only multiplies)
    (dict(N=256, W=257, steps=65281), dict(speculative=1, up_front=0, rows=384, perm_bytes=0)),
    # where speculation pays (mtg_plan_speculate): rows, rank, length
    (dict(N=256, E=11, W=62), dict(speculative=1, rows=1023, solves=3)),
    (dict(N=256, E=18, W=38), dict(speculative=0, rows=342, solves=6)),              # 3 x 342 = 1026
    (dict(nc0=2, E=10, W=34), dict(speculative=1, rows=510)),
    (dict(nc0=2, E=9, W=38), dict(speculative=0, rows=171)),                          # 3 x 171 = 513
    (dict(nr0=2, nc0=2), dict(speculative=1, rows=12)),                               # J = 6
    (dict(nr0=2, nc0=2, E=5, W=34), dict(speculative=1, rows=255)),
    (dict(nr0=2, nc0=2, E=2, W=86), dict(speculative=0, rows=86)),                    # 3 x 86 = 258
    (dict(nr0=1, nc0=3), SEQ),                                                        # J = 7
    (dict(N=256), dict(speculative=1)),
    (dict(N=255), SEQ),
    # walker sharding: sequential, the solver sees this rank's rows, an empty share as one
    (dict(shard=2, lo=0, hi=2), dict(SEQ, live=2)),
    (dict(shard=1, lo=2, hi=4), dict(SEQ, live=2)),
    (dict(shard=2, lo=4, hi=4), dict(SEQ, live=1)),
]

# mtg_ensemble_step from the priming launch (k = -1) to the last solve, the ensembles at iteration 10 when the run begins:
# (k, bank used, bank filled next, do_accept, half, iteration, do_propose, next_half, next_iteration, chain row, slice of
# the up-front splits for perm, for perm_next), -1 for none.  Written out from the two loops mtg_ensemble_run had: the
# priming launch passes iteration 0; the sequential form flips the bank after every half-step and writes a chain row
# after the second; the last launch of a run proposes nothing and has no perm_next.
PRIME = (-1, -1, 0, 0, 0, 0, 1, 0, 10, -1, -1, -1)
SCHEDULES = [
    (dict(spec_mode=0), [PRIME,
                         (0, 0, 1, 1, 0, 10, 1, 1, 10, -1, -1, -1), (1, 1, 0, 1, 1, 10, 1, 0, 11, 0, -1, -1),
                         (2, 0, 1, 1, 0, 11, 1, 1, 11, -1, -1, -1), (3, 1, 0, 1, 1, 11, 1, 0, 12, 1, -1, -1),
                         (4, 0, 1, 1, 0, 12, 1, 1, 12, -1, -1, -1), (5, 1, 0, 1, 1, 12, 0, 0, 13, 2, -1, -1)]),
    (dict(spec_mode=1), [(-1, -1, 0, 0, 0, 0, 1, 0, 10, -1, -1, 0),
                         (0, 0, 1, 1, 0, 10, 1, 0, 11, 0, 0, 1), (1, 1, 0, 1, 0, 11, 1, 0, 12, 1, 1, 2),
                         (2, 0, 1, 1, 0, 12, 0, 0, 13, 2, 2, -1)]),
    (dict(spec_mode=2), [PRIME,
                         (0, 0, 1, 1, 0, 10, 1, 0, 11, 0, -1, -1), (1, 1, 0, 1, 0, 11, 1, 0, 12, 1, -1, -1),
                         (2, 0, 1, 1, 0, 12, 0, 0, 13, 2, -1, -1)]),
    (dict(spec_mode=0, steps=1), [PRIME, (0, 0, 1, 1, 0, 10, 1, 1, 10, -1, -1, -1), (1, 1, 0, 1, 1, 10, 0, 0, 11, 0, -1, -1)]),
    (dict(spec_mode=1, steps=1), [(-1, -1, 0, 0, 0, 0, 1, 0, 10, -1, -1, 0), (0, 0, 1, 1, 0, 10, 0, 0, 11, 0, 0, -1)]),
    (dict(spec_mode=0, steps=0), []),
]

# mtg_plan_draw_slab(N, B): floor(2^28 / 8 N) rows rounded down to a multiple of 64, at least 64, at most B.
DRAW_SLAB = [  # (N, B) -> rows per slab
    ((200000, 1000), 128),        # 167 rows fit: two tiles of 64 (tests/test_gp_draw_gpu.py crosses this boundary on the device)
    ((200000, 128), 128), ((200000, 127), 127), ((200000, 100), 100),   # B below the slab: B
    ((262144, 1000), 128),        # 2^28 / 2^21 = 128 exactly
    ((262145, 1000), 64),         # 127 fit: one tile
    ((524288, 1000), 64),         # a row of 2^28 / 64 bytes: 64 fit exactly
    ((524289, 1000), 64),         # 8 bytes more: 63 fit, none after the rounding, the floor of one tile
    ((1000000, 1000), 64),        # 33 fit: the floor
    ((524289, 63), 63), ((1000000, 10), 10), ((100, 5), 5),             # B below 64: B
]

# mtg_plan_predict_at_slab(N, J, M, B): floor(2^30 / (8 N (3 J + 3))) rows, at most floor(2^30 / ceil(M / 64)) (the
# second stage's grid), at least 1, at most B; 0 when ceil(M / 64) > 2^30.  N = 10^4, J = 5: rows of 1 440 000 bytes,
# floor(1 073 741 824 / 1 440 000) = 745; the grid allows 745 rows up to 1 441 264 blocks (2^30 / 1 441 264 = 745.0001)
# and 744 from 1 441 265 on (744.9996).
PAT_SLAB = [  # (N, nr0, nc0, M, B) -> rows per slab
    ((10000, 1, 2, 65, 1000), 745), ((10000, 1, 2, 65, 745), 745), ((10000, 1, 2, 65, 744), 744), ((10000, 1, 2, 65, 1), 1),
    ((10000, 1, 2, 64 * 1441264, 1000), 745),          # 1 441 264 blocks: the memory still binds
    ((10000, 1, 2, 64 * 1441264 + 1, 1000), 744),      # 1 441 265 blocks: the grid binds
    ((10000, 1, 2, 64 * 1441264 + 1, 700), 700),
    ((1000, 0, 0, 1, 100000), 44739),                  # J = 0: rows of 24 000 bytes
    ((10000000, 1, 2, 65, 1000), 1),                   # a row of 1.44 GB, larger than the slab: one at a time
    ((10000, 1, 2, 64 << 30, 1000), 1),                # 2^30 blocks: the last M the grid takes, a row at a time
    ((10000, 1, 2, (64 << 30) + 1, 1000), 0),          # one more: refused (the entry's "M ... is too large")
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


def run_line(inputs, what):
    return " ".join("%s=%s" % kv for kv in dict(RUN_DEFAULTS, **inputs).items()) + " %s=1" % what


def test_ensemble_run_plan(driver):
    outs = driver([run_line(inputs, "run") for inputs, _ in RUN])
    assert len(outs) == len(RUN)
    for (inputs, want), out in zip(RUN, outs):
        got = dict(tok.split("=") for tok in out.split())
        for key, value in want.items():
            assert got[key] == str(value), (inputs, key, got)


def test_ensemble_schedule(driver):
    outs = driver([run_line(dict(inputs, iter0=10), "sched") for inputs, _ in SCHEDULES])
    assert len(outs) == len(SCHEDULES)
    for (inputs, want), out in zip(SCHEDULES, outs):
        got = [tuple(int(x) for x in row.split()) for row in out.split("|") if row.strip()]
        assert got == want, (inputs, got)


def test_slab_sizes(driver):
    outs = driver(["N=%d B=%d slab=1" % args for args, _ in DRAW_SLAB])
    assert [o.split()[1] for o in outs] == ["draw=%d" % want for _, want in DRAW_SLAB]
    outs = driver(["N=%d nr0=%d nc0=%d M=%d B=%d slab=1" % args for args, _ in PAT_SLAB])
    assert [o.split()[0] for o in outs] == ["predict_at=%d" % want for _, want in PAT_SLAB]
