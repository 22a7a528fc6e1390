"""What ppp.protassov_test decides before any work starts, as one value: who runs which observed chain, which block of
the simulated light curves a rank holds, how it refits them and how the maxima come together (``_plan_protassov``) -- pure
arithmetic on the sizes, the rank and the mode arguments, so that it can be printed and tested without a GPU or a second
process.  Nothing here touches a device or a process group.
"""
from typing import NamedTuple, Optional

import numpy as np

from .distributed import block_bounds

# rows per half-step of a WHOLE set of light curves up to which derive_posteriors_batch(index_base=...) keeps the chains on
# the batch-independent time-parallel kernel (mtg_set_time_parallel 3); see its docstring
REPRODUCIBLE_TP_ROWS = 16384

# Where results need not be the same for every number of ranks, block b draws from streams of its own: every seed of
# the block is the common one plus this stride times b (protassov_test when not reproducible; derive_posteriors_sharded)
BLOCK_SEED_STRIDE = 7919

# rows per half-step up to which concurrent_refits="auto" runs the two models' refits side by side (protassov_test)
SIDE_BY_SIDE_ROWS = 40000


def _reproducible_is_free(split, nsims, walkers, world):
    """protassov_test(sharded=True, reproducible=None): world-size-independent results by default exactly where they do not
    cost a rank the time-parallel kernels (docstring there): the whole set is within ``REPRODUCIBLE_TP_ROWS`` rows per
    half-step -- every block then runs the batch-independent time-parallel kernel --, or every rank's own share is beyond
    the time-parallel range (8192 rows), where the sweep is what it would run anyway."""
    by_model = _split_by_model(split, nsims, walkers, world)
    rows_per_rank = -(-nsims // (world // 2 if by_model else world)) * (walkers // 2)
    return bool(nsims * (walkers // 2) <= REPRODUCIBLE_TP_ROWS or rows_per_rank > 8192)


def _split_by_model(split, nsims, walkers, world):
    """How protassov_test(sharded=True) divides the refits: by light curve (every rank refits both models on its block)
    or by model (half of the ranks each).  By light curve whenever a rank's half-step fits the pipelined sweep (at most
    32 768 rows: one workgroup of 128 rows per compute unit): the two models' chains then run side by side on the rank
    and its share of BASELINE configs[3] at 8 GPUs takes 3.8 s.  Beyond that a half-step of the
    one-lane sweep costs one wave's latency over the N samples until a rank has about one wave per SIMD (65 536 rows),
    so two half-steps of both models one after the other take twice as long as one half-step of one model on twice
    the rows: by model, when asked for, or -- "auto" -- when the rows of a half-step per rank stay under that mark
    either way (at 8 GPUs that share is ~4.2 s: the alternative's 64 000-row half-steps at 3.7 ms)."""
    if split == "models":
        if world < 2:
            raise ValueError("split='models' needs at least two ranks")
        return True
    if split == "lightcurves" or world < 2:
        return False
    if split != "auto":
        raise ValueError("split must be 'auto', 'lightcurves' or 'models'")
    rows_by_lightcurve = -(-nsims // world) * (walkers // 2)
    if rows_by_lightcurve <= 32768:
        return False
    rows_by_model = -(-nsims // (world // 2)) * (walkers // 2)
    return rows_by_model <= 70000


class ProtassovPlan(NamedTuple):
    """One rank's part of a Protassov test (``_plan_protassov``).  Model 0 is the null kernel, model 1 the alternative."""
    nsims: int
    sim_walkers: int                     # walkers of the refits
    rank: int
    world: int
    sharded: bool
    # step 1, the observed light curve's two chains
    observed: str                        # "by_model" (rank k runs model k's), "side_by_side" (two threads) or "sequential"
    observed_models: tuple               # the chains this rank runs
    observed_device_sampler: bool        # even walker counts; odd ones go through the host sampler and numpy's global generator
    # steps 2 and 3: this rank refits ``models`` on light curves [lo, hi), block ``block`` of ``bounds``
    models: tuple
    block: int
    bounds: tuple
    lo: int
    hi: int
    reproducible: bool                   # resolved: results that do not depend on the number of ranks or on the split
    # the series to simulate: [sim_lo, sim_hi) holds [lo, hi) and, reproducible, the partner of a series that the block's
    # edge cuts off its pair; ``keep`` picks [lo, hi) out of them
    sim_lo: int
    sim_hi: int
    keep: slice
    sim_index_base: Optional[int]        # Simulator.simulate(index_base=, pair_series=)
    pair_series: Optional[bool]
    refits: str                          # "sequential", "side_by_side" (paired contexts), "unpaired" or "slices"
    own_engine: tuple                    # derive_posteriors_batch(own_engine=) of model k's refit
    fit_index_base: Optional[int]        # derive_posteriors_batch(index_base=, total_lightcurves=)
    total_lightcurves: Optional[int]
    # how the maxima of lnL come together: counts[k][r] = values of model k that rank r sends to the all-gather
    counts: tuple
    # None (one process), "lightcurves" (every rank refits both models on its block) or "models" (half of the ranks each)
    split: Optional[str]

    @property
    def refits_meet(self):
        """The two refits run in two threads that meet between their starting fits and their chains."""
        return self.refits != "sequential"

    @property
    def paired(self):
        """... and from there on send both contexts' pipelined half-steps out in one launch (mtg_pair_contexts)."""
        return self.refits == "side_by_side"


def _plan_protassov(nsims, walkers, sim_walkers=None, rank=0, world=1, sharded=False, split="auto", reproducible=None,
                    observed_split=True, observed_side_by_side=True, concurrent_refits="auto"):
    """-> ProtassovPlan for ``rank`` of ``world`` (every rank is called with the same other arguments, so every rank's
    plan tells the same story).  Raises the ValueErrors of ``split`` (sharded only) and ``concurrent_refits``."""
    nsims, rank, world, sharded = int(nsims), int(rank), int(world), bool(sharded)
    sw = sim_walkers or walkers
    by_model_split = sharded and _split_by_model(split, nsims, sw, world)
    if sharded and reproducible is None:
        reproducible = _reproducible_is_free(split, nsims, sw, world)
    reproducible = bool(reproducible)
    if concurrent_refits not in (True, False, "auto", "unpaired", "slices"):
        raise ValueError("concurrent_refits must be True, False, 'auto', 'unpaired' or 'slices'")

    if sharded and world >= 2 and bool(observed_split):
        # one model's chain per rank (0: null, 1: alternative), on the process's own context
        observed, observed_models = "by_model", ((0,), (1,))[rank] if rank < 2 else ()
    else:
        # two single-light-curve chains leave the GPU nearly empty: the two models side by side, each on a context
        # and a generator of its own -- the same chains as one after the other
        observed = "side_by_side" if walkers % 2 == 0 and observed_side_by_side else "sequential"
        observed_models = (0, 1)

    if by_model_split:
        # half of the ranks refit the null model, the other half the alternative, each half over ALL the light
        # curves: twice the rows per rank and one model's half-steps instead of both one after the other
        half = world // 2
        models, block, bounds = ((0,) if rank < half else (1,)), rank % half, block_bounds(nsims, half)
        lo, hi = int(bounds[block]), int(bounds[block + 1])
        if rank >= 2 * half:                                    # an odd rank out takes no part in the refits
            models, lo, hi = (), 0, 0
        sizes = np.diff(bounds)
        counts = [np.concatenate([sizes, 0 * sizes]), np.concatenate([0 * sizes, sizes])]
        if world % 2:
            counts = [np.append(c, 0) for c in counts]
    else:
        models, block, bounds = (0, 1), (rank if sharded else 0), block_bounds(nsims, world if sharded else 1)
        lo, hi = int(bounds[block]), int(bounds[block + 1])
        counts = [np.diff(bounds)] * 2

    if reproducible:
        # Every series with the partner it has in the whole set (the simulator's transform packs series 2p and
        # 2p + 1 together): a block that starts or ends inside a pair simulates the partner too -- its parameters
        # are at hand, every rank holds all the posterior samples -- and drops it.  At most two extra series.
        sim_lo, sim_hi = lo - (lo & 1), min(nsims, hi + (hi & 1))
    else:
        sim_lo, sim_hi = lo, hi

    # each model on a context of its own ("slices": and on its own half of the compute units, mtg_create_on_slice --
    # measured no faster: 7.24 against 7.14 ms per iteration)
    together = len(models) == 2 and (concurrent_refits in (True, "unpaired", "slices") or
                                     (concurrent_refits == "auto" and (hi - lo) * (sw // 2) <= SIDE_BY_SIDE_ROWS and hi - lo > 1))
    refits = "sequential" if not together else concurrent_refits if concurrent_refits in ("unpaired", "slices") else "side_by_side"
    # side by side: model k on the process's k-th extra context (gp.get_side_engine)
    own_engine = tuple((k, 2) if refits == "slices" else ("side", k) if together else False for k in (0, 1))

    return ProtassovPlan(
        nsims=nsims, sim_walkers=sw, rank=rank, world=world, sharded=sharded,
        observed=observed, observed_models=observed_models, observed_device_sampler=walkers % 2 == 0,
        models=models, block=block, bounds=tuple(int(b) for b in bounds), lo=lo, hi=hi, reproducible=reproducible,
        sim_lo=sim_lo, sim_hi=sim_hi, keep=slice(lo - sim_lo, hi - sim_lo),
        sim_index_base=sim_lo if reproducible else None, pair_series=True if reproducible else None,
        refits=refits, own_engine=own_engine,
        fit_index_base=lo if reproducible else None, total_lightcurves=nsims if reproducible else None,
        counts=tuple(tuple(int(c) for c in cs) for cs in counts),
        split=None if not sharded else "models" if by_model_split else "lightcurves")

