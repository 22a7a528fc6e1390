"""Recording stand-ins for everything ppp.protassov_test drives (the observed chains, the simulator, the lock-step refits,
the side contexts), so that its HOST logic -- who does what, in which order, with which seeds, rows and arguments -- runs
on a CPU and leaves a log of plain numbers and strings.  tests/golden/make_ppp_trace_golden.py records those logs from
the commit before the function was cut into a plan and stages (tests/golden/ppp_trace.json); tests/test_ppp_trace_cpu.py
and the sharded cases of tests/test_distributed.py hold later versions to them value for value.

Every fake's output is a deterministic function of what it was given: a wrong seed, row range or argument anywhere shows
up in ``T_obs`` / ``T_sim`` or in the log.  The collectives are not faked: the sharded cases run real torch.distributed
(gloo) ranks.
"""
import contextlib
import itertools
import os
import threading
import types

import numpy as np

N_TIMES = 12          # epochs of the fake light curve
CHAIN_LENGTH = 37     # rows of a fake chain's mcmc_samples

_lock = threading.Lock()
_log = []             # [lane, in the main thread?, what, payload]
_faults = {}


def _say(lane, what, payload=None):
    with _lock:
        _log.append([lane, threading.current_thread() is threading.main_thread(), what, payload])


def _plain(v):
    """kwargs as JSON holds them: tuples as lists, numpy scalars as Python's, callables as whether they are there."""
    if isinstance(v, (tuple, list)):
        return [_plain(x) for x in v]
    if isinstance(v, (bool, np.bool_)):
        return bool(v)
    if isinstance(v, (int, np.integer)):
        return int(v)
    if isinstance(v, (float, np.floating)):
        return float(v)
    if callable(v):
        return True
    return v


class Kernel:
    """All protassov_test itself reads of a kernel."""

    def __init__(self, vector_size):
        self.vector_size = vector_size


NULL_SIZE, ALT_SIZE = 2, 5


def _model(kernel):
    return {NULL_SIZE: 0, ALT_SIZE: 1}[kernel.vector_size]


def lightcurve():
    return types.SimpleNamespace(times=np.arange(N_TIMES, dtype=np.float64), exposures=0.5, mean=50.0, bkg_rate=None,
                                 bkg_rate_err=None)


class GPModelling:
    def __init__(self, lightcurve, kernel, device=0, own_engine=False, random_state=None):
        self.kernel, self.random_state = kernel, random_state
        self.lane = "chain%d" % _model(kernel)
        self.gp = types.SimpleNamespace(release_engine=lambda: _say(self.lane, "release_engine"))
        _say(self.lane, "GPModelling", dict(device=device, own_engine=_plain(own_engine), random_state=random_state is not None))

    def derive_posteriors(self, **kwargs):
        # the seed it was given: through its own generator, or (odd walkers) through numpy's global one
        draw = (self.random_state or np.random).randint(0, 2 ** 31 - 1)
        _say(self.lane, "derive_posteriors", dict(kwargs={k: _plain(v) for k, v in sorted(kwargs.items())}, draw=int(draw)))
        if _faults.get("observed") == _model(self.kernel):
            raise ArithmeticError("observed chain of model %d" % _model(self.kernel))
        g = np.random.RandomState(draw)
        self.best_loglikelihood = -2.0 * self.kernel.vector_size + g.standard_normal()
        self.mcmc_samples = g.standard_normal((CHAIN_LENGTH, self.kernel.vector_size))


class Simulator:
    def __init__(self, *args, **kwargs):
        self.random_state = kwargs.get("random_state")
        shown = [a.vector_size if isinstance(a, Kernel) else ["array", len(a), float(a.sum())] if isinstance(a, np.ndarray) else _plain(a) for a in args]
        _say("sim", "Simulator", dict(args=shown, kwargs={k: _plain(v) for k, v in kwargs.items()}))

    def warm_up(self):
        _say("sim", "warm_up")

    def simulate(self, samples, index_base=None, pair_series=None):
        samples = np.asarray(samples)
        _say("sim", "simulate", dict(shape=list(samples.shape), checksum=float(np.sum(samples * (1 + np.arange(samples.shape[1])))),
                                     index_base=_plain(index_base), pair_series=pair_series,
                                     draw=int(self.random_state.randint(0, 2 ** 31 - 1))))
        if _faults.get("simulate"):
            raise FloatingPointError("the simulator")
        index = (index_base or 0) + np.arange(len(samples), dtype=np.float64)
        rates = index[:, None] + np.arange(N_TIMES) / 64.0
        return dict(rates=rates, dy=0.5 + rates / 1024.0, clean=None)


def derive_posteriors_batch(times, Y, DY, kernel, **kwargs):
    k = _model(kernel)
    before = kwargs.get("before_sampling")
    _say("refit%d" % k, "derive_posteriors_batch",
         dict(kwargs={n: _plain(v) for n, v in sorted(kwargs.items())}, shape=list(np.shape(Y)),
              checksum=float(np.sum(Y)) + float(np.sum(DY)), times=len(times)))
    if _faults.get("refit") == k:
        raise ZeroDivisionError("refit of model %d" % k)
    if before is not None:
        before()
        _say("refit%d" % k, "past before_sampling")
    index = np.asarray(Y)[:, 0]          # (the fake simulator writes the global index there)
    seed = kwargs["seed"] % 1000003
    return types.SimpleNamespace(max_loglikelihood=-(index + 1.0) * (3 + k) - ((index * 7 + seed) % 11) * (k + 1) / 8.0)


class _SideEngine:
    def __init__(self, device, k):
        self.name = [_plain(device), k]

    def pair_with(self, other):
        _say("side", "pair_with", [self.name, other.name])

    def unpair(self):
        _say("side", "unpair", self.name)

    def pair_stats(self):
        _say("side", "pair_stats", self.name)
        return {"paired": 7, "broken": 0}


def get_side_engine(device, k):
    return _SideEngine(device, k)


@contextlib.contextmanager
def installed(**faults):
    """The fakes in place of what protassov_test looks up when it is called (``faults``: observed / refit = the model
    whose chain / refit raises, simulate = True); an empty log."""
    from mind_the_gaps_amd import gp, gpmodelling, ppp, simulator
    spots = [(gpmodelling, "GPModelling", GPModelling), (simulator, "Simulator", Simulator),
             (ppp, "derive_posteriors_batch", derive_posteriors_batch), (gp, "get_side_engine", get_side_engine)]
    saved = [(m, n, getattr(m, n)) for m, n, _ in spots]
    for m, n, fake in spots:
        setattr(m, n, fake)
    _faults.clear()
    _faults.update(faults)
    del _log[:]
    try:
        yield
    finally:
        for m, n, real in saved:
            setattr(m, n, real)
        _faults.clear()


def _canonical_log():
    """The log with what threads may reorder taken out: every lane's own sequence, and the main thread's across lanes."""
    lanes = {}
    for lane, _, what, payload in _log:
        lanes.setdefault(lane, []).append([what, payload])
    return dict(lanes=lanes, main_thread=[[lane, what] for lane, main, what, _ in _log if main])


def run_case(case, rank=None):
    """One protassov_test call under the fakes -> the record the golden file holds.  ``case``: dict(kwargs, faults, on_rank:
    the only rank the faults are injected on, None = every rank)."""
    from mind_the_gaps_amd import ppp
    faults = case.get("faults", {}) if case.get("on_rank") in (None, rank) else {}
    kwargs = dict(nsims=5, walkers=16, max_steps=60, sim_steps=40, seed=11)
    kwargs.update(case["kwargs"])
    record = {}
    state = np.random.get_state()
    with installed(**faults):
        try:
            res = ppp.protassov_test(lightcurve(), Kernel(NULL_SIZE), Kernel(ALT_SIZE), **kwargs)
            record = dict(T_obs=float(res["T_obs"]), T_sim=[float(v) for v in res["T_sim"]], p_value=float(res["p_value"]),
                          split=res["split"], reproducible=res["reproducible"], paired_launches=res["paired_launches"],
                          seconds=sorted(res["seconds"]),
                          is_none=[k for k in ("null", "alt", "sim_null", "sim_alt", "lightcurves") if res[k] is None])
        except Exception as exc:
            record = dict(raised=[type(exc).__name__, str(exc)])
        if not case["raised_only"]:
            record["log"] = _canonical_log()
    after = np.random.get_state()
    record["numpy_global_state_kept"] = bool(state[0] == after[0] and np.array_equal(state[1], after[1]) and state[2:] == after[2:])
    return record


# The golden file holds 209 records (14 cases in one process, 39 on each of 2 and of 3 ranks) that repeat one another's parts (the same simulator call, the same chain, the same
# T_sim), so it stores every distinct part once: ``pool`` = the distinct values, ``records`` = the distinct records as one
# pool index per field of FIELDS (-1: the record has no such field; a lane = a list of pool indices, one per call),
# ``cases`` = the record of every case and rank.  One pool value or record per line, so that a change of one shows as one.
FIELDS = ("T_obs", "T_sim", "p_value", "split", "reproducible", "paired_launches", "seconds", "is_none", "raised",
          "numpy_global_state_kept", "main_thread", "chain0", "chain1", "sim", "refit0", "refit1", "side")


def pack_golden(cases):
    """{"world1": [{name: record}], "world2": [per rank {name: record}], ...} -> the text of the golden file."""
    import json
    pool, records, seen = [], [], {}

    def put(value, into=pool):
        key = (id(into), json.dumps(value, sort_keys=True))
        if key not in seen:
            seen[key] = len(into)
            into.append(value)
        return seen[key]

    def pack(record):
        flat = {k: v for k, v in record.items() if k != "log"}
        if "log" in record:
            flat["main_thread"] = record["log"]["main_thread"]
            flat.update({lane: [put(call) for call in calls] for lane, calls in sorted(record["log"]["lanes"].items())})
        assert set(flat) <= set(FIELDS), sorted(set(flat) - set(FIELDS))
        return put([put(flat[f]) if f in flat else -1 for f in FIELDS], records)

    index = {group: [{n: pack(r) for n, r in sorted(per.items())} for per in ranks] for group, ranks in sorted(cases.items())}
    dumps = lambda v: json.dumps(v, sort_keys=True, separators=(",", ":"))
    return ('{"fields":%s,\n"pool":[\n%s\n],\n"records":[\n%s\n],\n"cases":{\n%s\n}}\n'
            % (dumps(list(FIELDS)), ",\n".join(dumps(v) for v in pool), ",\n".join(dumps(r) for r in records),
               ",\n".join('"%s":%s' % (group, dumps(per)) for group, per in index.items())))


def load_golden(path):
    """The golden file -> {"world1": [{name: record}], "world2": [per rank {name: record}], "world3": ...}."""
    import json
    packed = json.load(open(path))
    pool = packed["pool"]

    def unpack(row):
        flat = {f: pool[i] for f, i in zip(packed["fields"], row) if i >= 0}
        record = {k: v for k, v in flat.items() if k in FIELDS[:10]}
        if "main_thread" in flat:
            record["log"] = dict(main_thread=flat["main_thread"],
                                 lanes={lane: [pool[i] for i in flat[lane]] for lane in FIELDS[11:] if lane in flat})
        return record

    return {group: [{n: unpack(packed["records"][i]) for n, i in per.items()} for per in ranks]
            for group, ranks in packed["cases"].items()}


def assert_same_records(got, want, where):
    """Value for value: the records hold plain numbers, strings and lists, so there is no tolerance."""
    import json
    got = json.loads(json.dumps(got))            # (tuples as lists, as the golden file holds them)
    assert sorted(got) == sorted(want), where
    for key in want:
        assert got[key] == want[key], "%s: %s\n got %r\nwant %r" % (where, key, got[key], want[key])


def _case(faults=None, on_rank=None, raised_only=False, **kwargs):
    return dict(kwargs=kwargs, faults=faults or {}, on_rank=on_rank, raised_only=raised_only)


# 40 000 rows per half-step is where "auto" stops running the two refits side by side: 8000 walkers = 4000 rows per light
# curve.  ``raised_only``: a case whose arguments are refused -- the planner may refuse them before step 1 where the
# one-block function refused them after it, so only the exception is compared, not the log up to it.
UNSHARDED_CASES = {
    "defaults": _case(),
    "refits_False": _case(concurrent_refits=False),
    "refits_True": _case(concurrent_refits=True),
    "refits_unpaired": _case(concurrent_refits="unpaired"),
    "refits_slices": _case(concurrent_refits="slices"),
    "refits_auto_at_40000_rows": _case(concurrent_refits="auto", nsims=10, sim_walkers=8000),
    "refits_auto_past_40000_rows": _case(concurrent_refits="auto", nsims=11, sim_walkers=8000),
    "refits_auto_one_lightcurve": _case(concurrent_refits="auto", nsims=1),
    "odd_walkers": _case(walkers=15, sim_walkers=16),
    "observed_one_after_the_other": _case(observed_side_by_side=False),
    "reproducible_odd_nsims": _case(reproducible=True, nsims=7),
    "side_by_side_refit_fails": _case(concurrent_refits=True, faults=dict(refit=1)),
    "simulator_fails": _case(faults=dict(simulate=True)),
    "bad_concurrent_refits": _case(concurrent_refits="both", raised_only=True),
}


def sharded_cases(world):
    """name -> case for ``world`` ranks: the whole grid of the issue (split x nsims x reproducible x observed_split), "auto"
    at a walker count where two ranks split five light curves by model and three do not, and the two failures."""
    cases = {}
    for split, nsims, rep, obs in itertools.product(("lightcurves", "models", "auto"), (5, 1), (True, False, None), (True, False)):
        extra = dict(sim_walkers=24000) if split == "auto" else {}
        cases["%s_n%d_rep%s_obs%s" % (split, nsims, rep, obs)] = _case(
            sharded=True, split=split, nsims=nsims, reproducible=rep, observed_split=obs, **extra)
    cases["refit_fails_on_rank_1"] = _case(sharded=True, faults=dict(refit=0), on_rank=1)
    cases["observed_chain_fails_on_rank_1"] = _case(sharded=True, faults=dict(observed=1), on_rank=1)
    cases["bad_split"] = _case(sharded=True, split="columns", raised_only=True)
    return cases


def sharded_worker(rank, world, port, out_dir):
    """One gloo rank (CPU tensors) running every case of ``sharded_cases(world)`` -> out_dir/trace<world>_<rank>.json."""
    import json
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    records = {name: run_case(case, rank) for name, case in sharded_cases(world).items()}
    with open(os.path.join(out_dir, "trace%d_%d.json" % (world, rank)), "w") as fh:
        json.dump(records, fh)
    dist.barrier()
    dist.destroy_process_group()
