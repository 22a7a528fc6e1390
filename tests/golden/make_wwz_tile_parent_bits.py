#!/usr/bin/env python3
"""mtg_wwz, bit for bit, at the smallest shapes that reach what the wavelet sweep (csrc/mtg_wwz.hip) shares with the tile
sweep of csrc/mtg_ls_tile.h and tests/golden/resident_calls_parent_bits.npz does not reach (there every tiled case is one
partly filled tile in one workgroup of 128 lanes over at most two chunks) -> tests/golden/wwz_tile_parent_bits.npz, which
tests/test_wwz_tile_parent_bits_gpu.py holds every later build to.  Made on the commit before the sweep was written on
mtg_ls_tile.h's pieces (`commit` in the fixture).

    sampling   shared, L = 9: weighted two full tiles of 4 and a tile of 1, unweighted a full tile of 8 and a tile of 1;
               one sampling per light curve, L = 2: a light curve per lane with t_stride = N
    samples    N = 700 in two seasons with a gap, ascending and irregular: chunks of 256, 256 and 188, the gap in the second
    freqs      F = 260 ascending: two blocks of 256 lanes, the second with 252 idle ones
    centres    T = 3: just after the first sample, inside the gap, beyond the last sample
    decay      the default
    calls      shared: Z weighted and unweighted with values and peaks; amplitude weighted and power unweighted with
               values.  Own: Z weighted with values and peaks at the gap's centre (block ranges [0, 3) and [1, 2)).
               No N_eff map, for the fixture's size: every Z holds its N_eff, (N_eff - 3) being a factor of it

The frequency blocks' lowest frequencies are far enough apart that, by the range rule of mtg_wwz.hip's header restated in
`chunk_ranges`, the first block keeps all three chunks at every centre and the second keeps one: the first at the first
centre (c_hi < 3), the second at the gap's (c_lo > 0 and c_hi < 3), the third at the last (c_lo > 0).  `check_grid` refuses
a grid that misses one of these and, with tests/wwz_numpy.py, one that leaves a map without finite values; it needs no GPU.

The inputs lie on binary grids (t 2^-16, y 2^-6, dy 2^-8), as recorded photometry does, which keeps them a fifth of
their size in the fixture; the residuals, the weights, the window and every sum are full-width all the same.  The
frequencies and the centres are this file's constants.  Public Engine calls only.
Every output is stored as its 64-bit pattern, all calls one after the other in `bits` (`names`, `sizes`: whose and how
many; `solvers`: mtg_last_solver after every call).  Run on a GPU:
    python3 tests/golden/make_wwz_tile_parent_bits.py --commit $(git rev-parse HEAD)
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "wwz_tile_parent_bits.npz")
SEED = 20261023
N, L, L_OWN, F, T = 700, 9, 2, 260, 3
CHUNK, LANES = 256, 256
DECAY = 1.0 / (8.0 * np.pi ** 2)
CUT = 80.0 * np.log(2.0)
INPUTS = ("t", "t_own", "y", "dy")
FREQS = np.linspace(0.05, 2.64, F)
TAUS = np.array([100.5, 120.0, 141.0])      # just after the first sample, inside the gap, beyond the last sample
WANTED_RANGES = {"c_lo > 0": lambda lo, hi, nch: lo > 0, "c_hi < chunks": lambda lo, hi, nch: hi < nch,
                 "every chunk": lambda lo, hi, nch: (lo, hi) == (0, nch)}


def draw_inputs():
    rng = np.random.default_rng(SEED)

    def times():      # two seasons with a gap between them (116, 124)
        u = np.concatenate([rng.uniform(100.0, 116.0, size=N // 2), rng.uniform(124.0, 140.0, size=N - N // 2)])
        return np.sort(np.round(u * 65536.0) / 65536.0)

    t = times()
    t_own = np.stack([times() for _ in range(L_OWN)])
    y = rng.standard_normal((L, N)) + 2.0 * np.sin(2 * np.pi * 0.31 * t) + np.cos(2 * np.pi * 1.07 * t)
    y = np.round(y * 64.0) / 64.0
    dy = np.round(rng.uniform(0.1, 0.5, size=(L, N)) * 256.0) / 256.0
    return dict(t=t, t_own=t_own, y=y, dy=dy)


def chunk_ranges(t, freqs, taus):
    """the range rule of mtg_wwz.hip's header restated -> {(frequency block, centre): (c_lo, c_hi)}: a chunk is kept
    unless its least |t - tau| -- an end's, or 0 where it lies across tau -- is cut at the block's lowest frequency"""
    kc = 39.478417604357434 * DECAY
    nch = (len(t) + CHUNK - 1) // CHUNK
    out = {}
    for fb in range((len(freqs) + LANES - 1) // LANES):
        flow = freqs[fb * LANES:(fb + 1) * LANES].min()
        alow = (kc * flow) * flow
        for jt, tau in enumerate(taus):
            te = t - tau
            ts2 = np.min(te * te)
            kept = []
            for c in range(nch):
                a, b = te[c * CHUNK], te[min((c + 1) * CHUNK, len(t)) - 1]
                m = a if a >= 0.0 else -b if b <= 0.0 else 0.0
                if not alow * (m * m - ts2) > CUT:
                    kept.append(c)
            out[fb, jt] = (kept[0], kept[-1] + 1)
    return out


def check_grid(inp):
    """the grid reaches the three kinds of chunk range, on every sampling, and leaves finite values in every map"""
    sys.path.insert(0, os.path.dirname(HERE))
    import wwz_numpy
    nch = (N + CHUNK - 1) // CHUNK
    assert nch == 3 and N % CHUNK and (F + LANES - 1) // LANES == 2 and F % LANES
    assert np.all(np.diff(inp["t"]) >= 0) and np.all(np.diff(inp["t_own"], axis=-1) >= 0)
    for t in [inp["t"]] + list(inp["t_own"]):
        ranges = chunk_ranges(t, FREQS, TAUS)
        for what, holds in WANTED_RANGES.items():
            assert any(holds(lo, hi, nch) for lo, hi in ranges.values()), (what, ranges)
    least = 1.0
    for t, ys, dys in [(inp["t"], inp["y"], inp["dy"])] + [(inp["t_own"][l], inp["y"][l:l + 1], inp["dy"][l:l + 1]) for l in range(L_OWN)]:
        for l in range(len(ys)):
            for weighted in (True, False):
                got = wwz_numpy.wwz(t, ys[l], dys[l], FREQS, TAUS, weighted=weighted)
                for key in ("z", "power", "amplitude", "neff"):
                    share = np.isfinite(got[key]).mean(axis=1)
                    assert np.all(share > 0.0), (key, l, weighted, share)
                    least = min(least, float(share.min()))
    return ranges, least


def bits(arrays):
    return np.concatenate([np.ascontiguousarray(a).ravel().view(np.uint64) for a in arrays])


def run(eng, inp):
    """-> [(name, mtg_last_solver, uint64 bits)] of every call, in a fixed order"""
    out = []

    def wwz(where, taus, statistic, weighted, peak=False):
        got = eng.wwz(FREQS, taus, statistic=statistic, weighted=weighted, values=True, peak=peak)
        out.append(("wwz/%s_t%d/%s_w%d_10%d" % (where, len(taus), statistic, weighted, peak), eng.last_solver, bits(got if peak else [got])))

    eng.set_lightcurves(inp["t"], inp["y"], inp["dy"])
    wwz("shared9", TAUS, "z", 1, peak=True)
    wwz("shared9", TAUS, "z", 0, peak=True)
    wwz("shared9", TAUS, "amplitude", 1)
    wwz("shared9", TAUS, "power", 0)
    eng.set_lightcurves(inp["t_own"], inp["y"][:L_OWN], inp["dy"][:L_OWN])
    wwz("own2", TAUS[1:2], "z", 1, peak=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--commit", required=True, help="the commit the library was built from")
    ap.add_argument("--out", default=FIXTURE)
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from mind_the_gaps_amd.engine import Engine
    inp = draw_inputs()
    ranges, least = check_grid(inp)
    print("chunk ranges (frequency block, centre): %s; least share of finite entries in a map %.2f" % (ranges, least))
    eng = Engine(0)
    calls = run(eng, inp)
    eng.close()
    np.savez_compressed(args.out, commit=np.array(args.commit), names=np.array([n for n, _, _ in calls]),
                        solvers=np.array([s for _, s, _ in calls]), sizes=np.array([len(b) for _, _, b in calls], dtype=np.int64),
                        bits=np.concatenate([b for _, _, b in calls]), **inp)
    print("%d calls, %d words, %d kernels -> %s (%d bytes)" % (len(calls), sum(len(b) for _, _, b in calls), len({s for _, s, _ in calls}),
                                                                args.out, os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
