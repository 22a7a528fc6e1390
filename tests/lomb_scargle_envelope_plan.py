"""The planner of mtg_lomb_scargle_envelope (mind_the_gaps_amd/csrc/mtg_ls_envelope_plan.h) for the tests: the header
compiled with g++ into tests/ls_envelope_plan_driver.cpp's program, asked line by line.  No GPU, no HIP."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Planner:
    def __init__(self):
        self._dir = tempfile.TemporaryDirectory(prefix="lse_plan_")
        self.exe = os.path.join(self._dir.name, "ls_envelope_plan_driver")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "mind_the_gaps_amd", "csrc"),
                               os.path.join(ROOT, "tests", "ls_envelope_plan_driver.cpp"), "-o", self.exe])
        self.budget, self.lds_keys, self.max_cols, self.threads = (int(v) for v in self._ask(["constants"])[0].split())

    def _ask(self, lines):
        r = subprocess.run([self.exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True)
        return r.stdout.splitlines()

    def plans(self, cases, budget=None):
        """[(L, F, Q)] -> [dict(in_lds, columns, pow2, width, workspace)]"""
        budget = self.budget if budget is None else budget
        outs = self._ask(["%d %d %d %d" % (L, F, Q, budget) for L, F, Q in cases])
        assert len(outs) == len(cases)
        return [dict(zip(("in_lds", "columns", "pow2", "width", "workspace"), map(int, o.split()))) for o in outs]

    def plan(self, L, F=1, Q=0, budget=None):
        return self.plans([(L, F, Q)], budget)[0]

    def boundaries(self):
        """Every L at which the implementation changes: the last L of each columns-per-workgroup value below the LDS
        limit, and the LDS limit itself -> [(L, what changes at L + 1)]"""
        out, L = [], 1
        while L < self.lds_keys:
            if self.plan(L)["columns"] != self.plan(L + 1)["columns"]:
                out.append((L, "columns per workgroup"))
            L *= 2
        out.append((self.lds_keys, "LDS path to segmented sort"))
        return out
