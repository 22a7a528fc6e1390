#!/usr/bin/env python3
"""Generates tests/golden/ppp_trace.json: what ppp.protassov_test does on the host -- every call it makes with its
arguments, seeds and row ranges, and what it returns -- under the recording stand-ins of tests/ppp_fakes.py, for every
case listed there: unsharded, and on 2 and 3 torch.distributed ranks (gloo, CPU tensors).  No GPU is needed.

Record it from a checkout of the commit BEFORE ppp.py got its planner: tests/test_ppp_trace_cpu.py and the sharded trace
test of tests/test_distributed.py hold the planned, staged function to that commit's log value for value.  The recorder
refuses to write when this tree's ppp.py already has ``_plan_protassov``.

Run from the repo root:  python tests/golden/make_ppp_trace_golden.py   (a few seconds; deterministic)
"""
import json
import os
import socket
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import ppp_fakes  # noqa: E402
from mind_the_gaps_amd import ppp  # noqa: E402


def main():
    if hasattr(ppp, "_plan_protassov"):
        raise SystemExit("this tree's ppp.py already has the planner: record the fixture from the commit before it")
    import torch.multiprocessing as mp
    golden = {"world1": [{name: ppp_fakes.run_case(case) for name, case in ppp_fakes.UNSHARDED_CASES.items()}]}
    for world in (2, 3):
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        with tempfile.TemporaryDirectory() as out_dir:
            mp.spawn(ppp_fakes.sharded_worker, args=(world, port, out_dir), nprocs=world, join=True)
            golden["world%d" % world] = [json.load(open(os.path.join(out_dir, "trace%d_%d.json" % (world, r))))
                                         for r in range(world)]
    # (through JSON once: the records as a later reader gets them, tuples as lists)
    with open(os.path.join(HERE, "ppp_trace.json"), "w") as fh:
        fh.write(ppp_fakes.pack_golden(json.loads(json.dumps(golden))))


if __name__ == "__main__":
    main()
