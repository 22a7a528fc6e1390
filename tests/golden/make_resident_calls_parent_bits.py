#!/usr/bin/env python3
"""The entries that work on the resident light curves alone -- mtg_lomb_scargle / _multi, mtg_lomb_scargle_envelope / _multi,
mtg_epoch_fold, mtg_phase_fold, mtg_wwz, mtg_lag_sums, mtg_cross_sums -- as the commit before their host code was put through
one call shape (mtg_capi.hip) ran them -> tests/golden/resident_calls_parent_bits.npz, which
tests/test_resident_calls_parent_bits_gpu.py holds every later build to.  Two records:

`run_bits`      the outputs of epoch_fold, phase_fold and wwz, which had no parent fixture yet, as 64-bit patterns
    epoch_fold  N 259 (a full chunk and a ragged one), 256, 2;  L 1, 3, 5 on shared sampling (tiles 1, 2, 4, partly filled
                and ragged) and 3 on a sampling of their own;  F 70, 260 (128 and 256 lanes with idle ones) and 3 (64);
                nbins 2, 10, 19, 32 (both sides of "not even one light curve fits");  weighted and not;  the four
                normalisations and chi2 at one shape;  the peaks with every call.  Every combination at L = 3 shared and
                at F = 3; on the other sets the combinations whose plan differs from those (the widest outputs are the
                fixture's size)
    phase_fold  F = 3 on the same sets and bins, thinned in the same way;  each output alone and all four through the C
                entry (Engine.phase_fold always asks for all)
    wwz         N 259 and 4;  L 1 and 3 shared, 3 own;  F 70;  T 1 and 5, a centre inside a gap of the sampling and one
                outside its span;  the three statistics, decay 0 and Foster's, weighted and not;  values alone, neff alone,
                the peak alone, all
`run_refusals`  for each of the nine entries every refusal it can make (but a HIP error), and calls that are wrong in two
                ways at once, which pin the refusal that wins: the code and the whole message.  Each is followed by one
                small good call of the same entry on the same context, whose bits are stored too.

Public Engine calls, and the library's C entries (Engine._lib, Engine._ctx, Engine._check) where an Engine method cannot
make the call, so that this file runs unchanged on the commit the fixture was made on (`commit` in the fixture) and on
every commit after it.  All calls one after the other in `bits` (`names`, `sizes`: whose and how many; `solvers`:
mtg_last_solver after every call); `refusal_names`, `refusal_codes`, `refusal_messages`.  Both records also keep
mtg_last_kernel_ms after every good call (Recorder.ms), which is not stored.  Run on a GPU:
    python3 tests/golden/make_resident_calls_parent_bits.py --commit $(git rev-parse HEAD)
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "resident_calls_parent_bits.npz")
SEED = 20261022
N_BIG, L_BIG, F_BIG = 259, 5, 260
INPUTS = ("t", "t_own", "y", "dy", "freqs", "taus", "t2", "y2")
NORMALIZATIONS = ("standard", "model", "log", "psd", "chi2")
ENTRIES = ("lomb_scargle", "lomb_scargle_multi", "lomb_scargle_envelope", "lomb_scargle_envelope_multi", "epoch_fold", "phase_fold",
           "wwz", "lag_sums", "cross_sums")
NAN, INF = float("nan"), float("inf")


def draw_inputs():
    """every call's inputs from SEED: the sets are leading slices of one draw"""
    rng = np.random.default_rng(SEED)

    def times(n):      # two seasons with a gap between them (116, 124)
        return np.sort(np.concatenate([rng.uniform(100.0, 116.0, size=n // 2), rng.uniform(124.0, 140.0, size=n - n // 2)]))

    t = times(N_BIG)
    t_own = np.stack([times(N_BIG) for _ in range(3)])
    y = rng.standard_normal((L_BIG, N_BIG)) + 2.0 * np.sin(2 * np.pi * 0.31 * t) + np.cos(2 * np.pi * 1.07 * t)
    dy = rng.uniform(0.1, 0.5, size=(L_BIG, N_BIG))
    freqs = np.linspace(0.02, 2.6, F_BIG)
    taus = np.array([108.0, 120.0, 131.5, 150.0, 101.0])    # 120: inside the gap; 150: beyond the last sample
    t2 = np.sort(rng.uniform(95.0, 135.0, size=40))
    y2 = rng.standard_normal((3, 40))
    return dict(t=t, t_own=t_own, y=y, dy=dy, freqs=freqs, taus=taus, t2=t2, y2=y2)


def bits(arrays):
    return np.concatenate([np.ascontiguousarray(a).ravel().view(np.uint64) for a in arrays])


def i64p(a):
    import ctypes
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))


def f64p(a):
    import ctypes
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


class Recorder:
    def __init__(self, inp):
        self.inp = inp
        self.calls = []       # (name, mtg_last_solver, uint64 bits)
        self.ms = []          # mtg_last_kernel_ms after every good call
        self.where = None

    def resident(self, eng, L, N, own=False):
        inp = self.inp
        eng.set_lightcurves(inp["t_own"][:, :N] if own else inp["t"][:N], inp["y"][:L, :N], inp["dy"][:L, :N])
        self.where = "%s%d_n%d" % ("own" if own else "shared", L, N)

    def keep(self, eng, name, arrays):
        self.calls.append(("%s/%s" % (name, self.where), eng.last_solver, bits(arrays)))
        self.ms.append(eng.last_kernel_ms)


def phase_fold_c(eng, freqs, nbins, weighted, wanted):
    """mtg_phase_fold with only the outputs named in `wanted` -> those arrays, in the entry's order"""
    shape = (int(eng.L), len(freqs), nbins)
    out = dict(count=np.zeros(shape, dtype=np.int64), wsum=np.full(shape, np.nan), wrsum=np.full(shape, np.nan), varsum=np.full(shape, np.nan))
    ptrs = [None if k not in wanted else i64p(out[k]) if k == "count" else f64p(out[k]) for k in ("count", "wsum", "wrsum", "varsum")]
    eng._check(eng._lib.mtg_phase_fold(eng._ctx, len(freqs), f64p(freqs), nbins, eng._first_time, int(weighted), *ptrs))
    return [out[k] for k in ("count", "wsum", "wrsum", "varsum") if k in wanted]


def run_bits(eng, inp):
    """epoch_fold, phase_fold and wwz -> Recorder (calls, ms), in a fixed order"""
    rec = Recorder(inp)
    f260, f70, f3 = inp["freqs"], inp["freqs"][3:73], inp["freqs"][[7, 101, 222]]
    sets = ((1, False), (3, False), (5, False), (3, True))

    def fold(F, freqs, nbins, weighted, normalization="standard"):
        got = eng.epoch_fold(freqs, nbins=nbins, normalization=normalization, weighted=weighted, power=True, peak=True)
        rec.keep(eng, "epoch_fold/f%d_b%d_w%d_%s" % (F, nbins, weighted, normalization), got)

    for L, own in sets:
        rec.resident(eng, L, N_BIG, own)
        whole = L == 3 and not own      # every plan on one set; on the others the plans that differ from it
        for nbins in (2, 10, 19, 32):
            for weighted in (1, 0):
                fold(3, f3, nbins, weighted)
                if L == 3 or nbins in (2, 19):
                    fold(70, f70, nbins, weighted)
                if whole or (own and weighted and nbins in (10, 32)) or (L == 1 and weighted and nbins == 19) or (L == 5 and not weighted and nbins == 2):
                    fold(260, f260, nbins, weighted)
                if (whole and (weighted or nbins in (10, 32))) or (own and weighted and nbins in (10, 32)) or \
                        (L in (1, 5) and (nbins, weighted) in ((2, 0), (19, 1))):
                    rec.keep(eng, "phase_fold/f3_b%d_w%d" % (nbins, weighted), eng.phase_fold(f3, nbins=nbins, weighted=weighted))
        if whole:
            for normalization in NORMALIZATIONS[1:]:
                fold(70, f70, 10, 1, normalization)
            for wanted in (("count",), ("wsum",), ("wrsum",), ("varsum",), ("count", "wsum", "wrsum", "varsum")):
                rec.keep(eng, "phase_fold_c/f3_b10_w1_" + "+".join(wanted), phase_fold_c(eng, f3, 10, 1, wanted))
    for N, F, freqs in ((256, 70, f70), (2, 3, f3)):
        rec.resident(eng, 3, N)
        for weighted in (1, 0):
            fold(F, freqs, 10, weighted)
            rec.keep(eng, "phase_fold/f3_b10_w%d" % weighted, eng.phase_fold(f3, nbins=10, weighted=weighted))

    def wwz(T, statistic="z", decay=None, weighted=1, values=True, neff=False, peak=False):
        kw = {} if decay is None else dict(decay=decay)
        got = eng.wwz(f70, inp["taus"][:T], statistic=statistic, weighted=weighted, values=values, neff=neff, peak=peak, **kw)
        rec.keep(eng, "wwz/t%d_%s_d%s_w%d_%d%d%d" % (T, statistic, "default" if decay is None else "%g" % decay, weighted, values, neff, peak),
                 got if isinstance(got, tuple) else [got])

    rec.resident(eng, 3, N_BIG)
    for statistic in ("power", "z", "amplitude"):
        wwz(5, statistic, None, 1, peak=True)
        wwz(1, statistic, None, 0, peak=True)
    wwz(5, "z", 0.0, 0, peak=True)
    wwz(1, "z", 0.0, 1, peak=True)
    wwz(1, values=True)
    wwz(5, values=False, neff=True)
    wwz(5, values=False, peak=True)
    wwz(5, neff=True, peak=True)
    for L, own, N in ((1, False, N_BIG), (3, True, N_BIG), (3, False, 4)):
        rec.resident(eng, L, N, own)
        wwz(1, "amplitude" if own else "z", 0.0 if N == 4 else None, 0 if L == 1 else 1, neff=True, peak=True)
        wwz(5, "amplitude" if own else "z", 0.0 if N == 4 else None, 1, neff=L == 1, peak=True)
    return rec


def run_refusals(eng, inp):
    """-> ([(name, code, message)], Recorder of the good call after every refusal)"""
    from mind_the_gaps_amd.engine import EngineError
    rec = Recorder(inp)
    refusals = []
    f3 = inp["freqs"][[7, 101, 222]].copy()
    f2 = f3[:2].copy()      # the good calls' frequencies
    bad_f = {"nan": np.array([0.5, NAN, 0.7]), "zero": np.array([0.0, 0.5]), "negative": np.array([0.5, 0.6, -0.25]), "inf": np.array([INF])}
    none_f = np.zeros(0)
    edges = np.array([0.0, 1.0, 2.5, 6.0])
    t2, y2 = inp["t2"], inp["y2"]
    lib = eng._lib

    def good(e, entry):
        """one small call of `entry` on the standard set, its bits kept"""
        if rec.where != "shared3_n259" or e is not eng:
            rec.resident(e, 3, N_BIG)
        if entry == "lomb_scargle":
            got = e.lomb_scargle(f2, peak=True)
        elif entry == "lomb_scargle_multi":
            got = e.lomb_scargle(f2, peak=True, nterms=2)
        elif entry.startswith("lomb_scargle_envelope"):
            got = list(e.lomb_scargle_envelope(f2, ranks=(1,), reference=np.full(2, 0.1), scale=np.ones(2), nterms=2 if entry.endswith("multi") else 1))
        elif entry == "epoch_fold":
            got = e.epoch_fold(f2, peak=True)
        elif entry == "phase_fold":
            got = e.phase_fold(f2, nbins=2)
        elif entry == "wwz":
            got = e.wwz(f2, inp["taus"][:1], peak=True)
        elif entry == "lag_sums":
            got = list(e.lag_sums(edges[:3]).values())
        else:
            got = list(e.cross_sums(t2, y2, edges[:3] - 2.0).values())
        rec.keep(e, "after %s" % refusals[-1][0], got)

    def refused(entry, tag, call, e=None):
        e = e or eng
        try:
            call()
        except EngineError as err:
            refusals.append(("%s: %s" % (entry, tag), int(err.code), str(err)))
        else:
            raise AssertionError("%s: %s was not refused" % (entry, tag))
        good(e, entry)

    def small(N, L=3):
        rec.resident(eng, L, N)

    # -- before mtg_set_lightcurves: a context of its own per entry
    first = {"lomb_scargle": lambda e: e.lomb_scargle(f3), "lomb_scargle_multi": lambda e: e.lomb_scargle(f3, nterms=3),
             "lomb_scargle_envelope": lambda e: e.lomb_scargle_envelope(f3, scale=np.ones(3)),
             "lomb_scargle_envelope_multi": lambda e: e.lomb_scargle_envelope(f3, scale=np.ones(3), nterms=3),
             "epoch_fold": lambda e: e.epoch_fold(f3, time_0=0.0), "phase_fold": lambda e: e.phase_fold(f3, time_0=0.0),
             "wwz": lambda e: e.wwz(f3, inp["taus"]), "lag_sums": lambda e: e.lag_sums(edges), "cross_sums": lambda e: e.cross_sums(t2, y2[0], edges)}
    for entry in ENTRIES:
        fresh = type(eng)(eng.device)
        try:
            refused(entry, "no light curves", lambda: first[entry](fresh), fresh)
        finally:
            fresh.close()
    rec.resident(eng, 3, N_BIG)

    # -- mtg_lomb_scargle and mtg_lomb_scargle_multi
    for entry, K in (("lomb_scargle", 1), ("lomb_scargle_multi", 3)):
        ls = lambda freqs, **kw: eng.lomb_scargle(freqs, nterms=kw.pop("nterms", K), **kw)
        refused(entry, "F = 0", lambda: ls(none_f))
        if K == 1:
            refused(entry, "freqs NULL", lambda: eng._check(lib.mtg_lomb_scargle(eng._ctx, 3, None, 0, 1, f64p(np.zeros((3, 3))), None, None)))
        refused(entry, "nothing asked", lambda: ls(f3, power=False, peak=False))
        refused(entry, "normalization 4", lambda: ls(f3, normalization=4))
        refused(entry, "normalization -1", lambda: ls(f3, normalization=-1))
        if K > 1:
            refused(entry, "nterms 0", lambda: ls(f3, nterms=0))
            refused(entry, "nterms 6", lambda: ls(f3, nterms=6))
        small(2 * K + 1)
        refused(entry, "N too small", lambda: ls(f3))
        for tag, freqs in bad_f.items():
            refused(entry, "freqs " + tag, lambda: ls(freqs))
        refused(entry, "F = 0 + nothing asked", lambda: ls(none_f, power=False, peak=False))
        refused(entry, "nothing asked + normalization", lambda: ls(f3, normalization=9, power=False, peak=False))
        refused(entry, "normalization + freqs nan", lambda: ls(bad_f["nan"], normalization=9))
        small(3)
        refused(entry, "normalization + N too small", lambda: ls(f3, normalization=9))
        small(3)
        refused(entry, "N too small + freqs nan", lambda: ls(bad_f["nan"]))
        if K > 1:
            refused(entry, "nterms 9 + freqs nan", lambda: ls(bad_f["nan"], nterms=9))
            refused(entry, "normalization + nterms 0", lambda: ls(f3, normalization=9, nterms=0))

    # -- mtg_lomb_scargle_envelope and mtg_lomb_scargle_envelope_multi
    for entry, K in (("lomb_scargle_envelope", 1), ("lomb_scargle_envelope_multi", 2)):
        def env(freqs=f3, normalization=0, Q=2, ranks=(0, 2), order_stat=True, valid=True, reference=(0.1, 0.1, 0.1), exceed=True,
                scale=(1.0, 1.0, 1.0), peak=True, index=True, K=K):
            F, L = len(freqs), int(eng.L)
            ranks = None if ranks is None else np.array(ranks, dtype=np.int64)
            reference = None if reference is None else np.array(reference, dtype=np.float64)
            scale = None if scale is None else np.array(scale, dtype=np.float64)
            os_, va, ex = np.zeros((max(Q, 1), F)), np.zeros(F, dtype=np.int64), np.zeros(F, dtype=np.int64)
            pk, ix = np.zeros(L), np.zeros(L, dtype=np.int64)
            rest = (Q, None if ranks is None else i64p(ranks), f64p(os_) if order_stat else None, i64p(va) if valid else None,
                    None if reference is None else f64p(reference), i64p(ex) if exceed else None, None if scale is None else f64p(scale),
                    f64p(pk) if peak else None, i64p(ix) if index else None)
            if K == 1:
                eng._check(lib.mtg_lomb_scargle_envelope(eng._ctx, F, f64p(freqs), normalization, 1, *rest))
            else:
                eng._check(lib.mtg_lomb_scargle_envelope_multi(eng._ctx, F, f64p(freqs), K, normalization, 1, *rest))

        refused(entry, "F = 0", lambda: env(none_f))
        refused(entry, "normalization 4", lambda: env(normalization=4))
        if K > 1:
            refused(entry, "nterms 6", lambda: env(K=6))
        small(2 * K + 1)
        refused(entry, "N too small", lambda: env())
        refused(entry, "freqs nan", lambda: env(bad_f["nan"]))
        refused(entry, "freqs zero", lambda: env(bad_f["zero"], reference=(0.1, 0.1), scale=(1.0, 1.0)))
        refused(entry, "Q < 0", lambda: env(Q=-1))
        refused(entry, "ranks NULL", lambda: env(ranks=None))
        refused(entry, "order_stat NULL", lambda: env(order_stat=False))
        refused(entry, "rank = L", lambda: env(ranks=(0, 3)))
        refused(entry, "rank negative", lambda: env(ranks=(-1, 0)))
        refused(entry, "exceed without reference", lambda: env(reference=None))
        refused(entry, "peak_ratio without scale", lambda: env(scale=None))
        refused(entry, "peak_ratio_index without scale", lambda: env(scale=None, peak=False))
        refused(entry, "nothing asked", lambda: eng.lomb_scargle_envelope(f3, nterms=K))
        refused(entry, "reference inf", lambda: env(reference=(0.1, INF, 0.1)))
        refused(entry, "scale zero", lambda: env(scale=(1.0, 1.0, 0.0)))
        refused(entry, "scale nan", lambda: env(scale=(NAN, 1.0, 1.0)))
        refused(entry, "F = 0 + normalization", lambda: env(none_f, normalization=9))
        refused(entry, "normalization + freqs nan", lambda: env(bad_f["nan"], normalization=9))
        refused(entry, "freqs nan + rank = L", lambda: env(bad_f["nan"], ranks=(0, 3)))
        refused(entry, "rank = L + reference inf", lambda: env(ranks=(0, 3), reference=(0.1, INF, 0.1)))
        refused(entry, "nothing asked + normalization", lambda: eng.lomb_scargle_envelope(f3, normalization=9, nterms=K))
        refused(entry, "reference inf + scale zero", lambda: env(reference=(0.1, INF, 0.1), scale=(1.0, 1.0, 0.0)))

    # -- mtg_epoch_fold
    entry = "epoch_fold"
    ef = eng.epoch_fold
    refused(entry, "F = 0", lambda: ef(none_f))
    refused(entry, "nothing asked", lambda: ef(f3, power=False, peak=False))
    refused(entry, "nbins 1", lambda: ef(f3, nbins=1))
    refused(entry, "nbins 33", lambda: ef(f3, nbins=33))
    refused(entry, "time_0 nan", lambda: ef(f3, time_0=NAN))
    refused(entry, "time_0 inf", lambda: ef(f3, time_0=-INF))
    refused(entry, "normalization 4", lambda: ef(f3, normalization=4))
    small(1)
    refused(entry, "N = 1", lambda: ef(f3))
    for tag, freqs in bad_f.items():
        refused(entry, "freqs " + tag, lambda: ef(freqs))
    refused(entry, "F = 0 + nbins", lambda: ef(none_f, nbins=1))
    refused(entry, "nothing asked + nbins", lambda: ef(f3, nbins=1, power=False, peak=False))
    refused(entry, "nbins + time_0", lambda: ef(f3, nbins=40, time_0=NAN))
    refused(entry, "time_0 + normalization", lambda: ef(f3, time_0=INF, normalization=7))
    refused(entry, "normalization + freqs nan", lambda: ef(bad_f["nan"], normalization=7))
    small(1)
    refused(entry, "N = 1 + freqs nan", lambda: ef(bad_f["nan"]))

    # -- mtg_phase_fold
    entry = "phase_fold"
    pf = eng.phase_fold

    def pf_c(freqs, nbins, F=None, time_0=100.0, want=True):
        F = len(freqs) if F is None else F
        count = np.zeros((int(eng.L), F, max(nbins, 1)), dtype=np.int64)      # (untouched pages: the call is refused)
        eng._check(lib.mtg_phase_fold(eng._ctx, F, f64p(freqs), nbins, time_0, 1, i64p(count) if want else None, None, None, None))

    many = np.full((1 << 23) // 32 + 1, 0.5)
    refused(entry, "F = 0", lambda: pf(none_f))
    refused(entry, "nothing asked", lambda: pf_c(f3, 10, want=False))
    refused(entry, "nbins 1", lambda: pf(f3, nbins=1))
    refused(entry, "nbins 33", lambda: pf(f3, nbins=33))
    refused(entry, "time_0 nan", lambda: pf(f3, time_0=NAN))
    small(1)
    refused(entry, "N = 1", lambda: pf(f3))
    for tag, freqs in bad_f.items():
        refused(entry, "freqs " + tag, lambda: pf(freqs))
    refused(entry, "F nbins too many", lambda: pf_c(many, 32))
    refused(entry, "L F nbins too many", lambda: pf_c(many[:-1], 32))
    refused(entry, "nothing asked + nbins", lambda: pf_c(f3, 99, want=False))
    refused(entry, "nbins + time_0", lambda: pf(f3, nbins=0, time_0=NAN))
    refused(entry, "time_0 + freqs nan", lambda: pf(bad_f["nan"], time_0=INF))
    many[-1] = NAN
    refused(entry, "freqs nan + too many", lambda: pf_c(many, 32))

    # -- mtg_wwz
    entry = "wwz"
    taus = inp["taus"]

    def wwz_c(freqs=f3, T=2, decay=0.0127, statistic=1, want=True):
        out = np.zeros((int(eng.L), min(T, 8), len(freqs)))
        eng._check(lib.mtg_wwz(eng._ctx, len(freqs), f64p(freqs), T, f64p(taus), decay, statistic, 1, f64p(out) if want else None, None, None, None))

    refused(entry, "F = 0", lambda: eng.wwz(none_f, taus))
    refused(entry, "T = 0", lambda: eng.wwz(f3, none_f))
    refused(entry, "taus NULL", lambda: eng._check(lib.mtg_wwz(eng._ctx, 3, f64p(f3), 2, None, 0.0127, 1, 1, f64p(np.zeros((3, 2, 3))), None, None, None)))
    refused(entry, "nothing asked", lambda: wwz_c(want=False))
    refused(entry, "decay nan", lambda: eng.wwz(f3, taus, decay=NAN))
    refused(entry, "decay negative", lambda: eng.wwz(f3, taus, decay=-0.5))
    refused(entry, "statistic 3", lambda: eng.wwz(f3, taus, statistic=3))
    small(3)
    refused(entry, "N = 3", lambda: eng.wwz(f3, taus))
    refused(entry, "T F beyond int64", lambda: wwz_c(T=(1 << 63) // 8 // 3 + 1))       # (refused before a tau is read)
    for tag, freqs in bad_f.items():
        refused(entry, "freqs " + tag, lambda: eng.wwz(freqs, taus))
    refused(entry, "taus inf", lambda: eng.wwz(f3, np.array([110.0, INF])))
    refused(entry, "F = 0 + T = 0", lambda: eng.wwz(none_f, none_f))
    refused(entry, "T = 0 + nothing asked", lambda: wwz_c(T=0, want=False))
    refused(entry, "nothing asked + decay", lambda: wwz_c(decay=NAN, want=False))
    refused(entry, "decay + statistic", lambda: eng.wwz(f3, taus, decay=-1.0, statistic=-1))
    small(3)
    refused(entry, "statistic + N = 3", lambda: eng.wwz(f3, taus, statistic=5))
    small(3)
    refused(entry, "N = 3 + freqs nan", lambda: eng.wwz(bad_f["nan"], taus))
    refused(entry, "freqs nan + taus nan", lambda: eng.wwz(bad_f["nan"], np.array([NAN])))

    # -- mtg_lag_sums
    entry = "lag_sums"

    def lag_c(nbins, e=edges, want=True):
        sf = np.zeros((int(eng.L), max(nbins, 1)))
        eng._check(lib.mtg_lag_sums(eng._ctx, nbins, None if e is None else f64p(e), None, None, f64p(sf) if want else None, None, None, None))

    wide = np.linspace(0.0, 30.0, 130)
    refused(entry, "nbins 0", lambda: lag_c(0))
    refused(entry, "nbins 129", lambda: eng.lag_sums(wide))
    refused(entry, "edges NULL", lambda: lag_c(3, None))
    refused(entry, "nothing asked", lambda: lag_c(3, want=False))
    refused(entry, "edges nan", lambda: eng.lag_sums(np.array([0.0, NAN, 2.0])))
    refused(entry, "edges negative", lambda: eng.lag_sums(np.array([-1.0, 1.0, 2.0])))
    refused(entry, "edges equal", lambda: eng.lag_sums(np.array([0.0, 1.0, 1.0])))
    refused(entry, "edges descending", lambda: eng.lag_sums(np.array([0.0, 2.0, 1.0, 3.0])))
    small(1)
    refused(entry, "N = 1", lambda: eng.lag_sums(edges))
    refused(entry, "nbins 0 + edges NULL", lambda: lag_c(0, None))
    refused(entry, "edges NULL + nothing asked", lambda: lag_c(3, None, want=False))
    refused(entry, "nothing asked + edges nan", lambda: lag_c(2, np.array([0.0, NAN, 2.0]), want=False))
    refused(entry, "edges inf + negative", lambda: eng.lag_sums(np.array([-1.0, 1.0, INF])))
    refused(entry, "edges negative + descending", lambda: eng.lag_sums(np.array([-1.0, 2.0, 1.0])))
    small(1)
    refused(entry, "edges descending + N = 1", lambda: eng.lag_sums(np.array([0.0, 2.0, 1.0])))

    # -- mtg_cross_sums
    entry = "cross_sums"
    cs = eng.cross_sums

    def cross_c(M=40, L2=1, t=t2, y=y2, nbins=3, e=edges, want=True):
        cf = np.zeros((int(eng.L), max(nbins, 1)))
        eng._check(lib.mtg_cross_sums(eng._ctx, M, None if t is None else f64p(t), L2, None if y is None else f64p(y), nbins,
                                      None if e is None else f64p(e), None, None, f64p(cf) if want else None, None, None, None, None, None))

    refused(entry, "M = 0", lambda: cs(none_f, none_f, edges))
    refused(entry, "M = 2^28", lambda: cross_c(M=1 << 28))       # (refused before the companion is read)
    refused(entry, "L2 = 2", lambda: cs(t2, y2[:2], edges))
    refused(entry, "t2 NULL", lambda: cross_c(t=None))
    refused(entry, "y2 NULL", lambda: cross_c(y=None))
    refused(entry, "nbins 0", lambda: cross_c(nbins=0))
    refused(entry, "nbins 129", lambda: cs(t2, y2, wide))
    refused(entry, "edges NULL", lambda: cross_c(e=None))
    refused(entry, "nothing asked", lambda: cross_c(want=False))
    refused(entry, "edges nan", lambda: cs(t2, y2, np.array([-1.0, NAN, 2.0])))
    refused(entry, "edges descending", lambda: cs(t2, y2, np.array([-1.0, -2.0, 3.0])))
    t_nan, t_down, y_inf = t2.copy(), t2.copy(), y2.copy()
    t_nan[5], t_down[7], y_inf[1, 4] = NAN, t2[5], INF
    refused(entry, "t2 nan", lambda: cs(t_nan, y2, edges))
    refused(entry, "t2 descending", lambda: cs(t_down, y2, edges))
    refused(entry, "y2 inf", lambda: cs(t2, y_inf, edges))
    refused(entry, "M = 0 + L2 = 2", lambda: cs(none_f, np.zeros((2, 0)), edges))
    refused(entry, "L2 = 2 + nbins 129", lambda: cs(t2, y2[:2], wide))
    refused(entry, "y2 NULL + edges NULL", lambda: cross_c(y=None, e=None))
    refused(entry, "edges descending + t2 nan", lambda: cs(t_nan, y2, np.array([-1.0, -2.0, 3.0])))
    refused(entry, "t2 nan + y2 inf", lambda: cs(t_nan, y_inf, edges))
    refused(entry, "t2 descending + y2 inf", lambda: cs(t_down, y_inf, edges))
    return refusals, rec


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--commit", required=True, help="the commit the library was built from")
    ap.add_argument("--out", default=FIXTURE)
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from mind_the_gaps_amd.engine import Engine
    inp = draw_inputs()
    eng = Engine(0)
    rec = run_bits(eng, inp)
    refusals, after = run_refusals(eng, inp)
    eng.close()
    calls = rec.calls + after.calls
    assert all(np.isfinite(ms) and ms > 0.0 for ms in rec.ms + after.ms)
    np.savez_compressed(args.out, commit=np.array(args.commit), names=np.array([n for n, _, _ in calls]),
                        solvers=np.array([s for _, s, _ in calls]), sizes=np.array([len(b) for _, _, b in calls], dtype=np.int64),
                        bits=np.concatenate([b for _, _, b in calls]), refusal_names=np.array([n for n, _, _ in refusals]),
                        refusal_codes=np.array([c for _, c, _ in refusals], dtype=np.int64),
                        refusal_messages=np.array([m for _, _, m in refusals]), **inp)
    print("%d calls, %d words, %d kernels, %d refusals -> %s (%d bytes)" % (len(calls), sum(len(b) for _, _, b in calls),
                                                                             len({s for _, s, _ in calls}), len(refusals), args.out,
                                                                             os.path.getsize(args.out)))
    for name, code, message in refusals:
        print("%-60s %d %s" % (name, code, message))


if __name__ == "__main__":
    main()
