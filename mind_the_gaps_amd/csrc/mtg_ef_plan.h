// mtg_ef_plan.h -- light curves per lane and lanes per workgroup of the epoch-folding sweep (mtg_epoch_fold.hip); pure
// functions of the sizes: no HIP, testable on the host alone, tests/ef_plan_driver.cpp.
//
// A lane owns a frequency and keeps, per light curve of its tile, the sums (W_b, S_b) of every phase bin.  The bin of a
// sample is known only at run time, so the sums live in LDS, laid out [bin][lane]:
//   weighted, or a tile of one   (W, S) pairs, 16 bytes per (light curve, bin, lane): one ds_read_b128 and one
//                                ds_write_b128 per (sample, light curve);
//   unweighted tile of R = 2, 4  W is the tile's (the weights are 1 / N): 8 bytes per (bin, lane), and the S of light
//                                curves (2 j, 2 j + 1) as a pair, 16 bytes per (pair, bin, lane).
// The byte address of a lane's entry is (bin * lanes + lane) * 16 (or * 8) with lanes a multiple of 64: the bank is
// decided by the lane alone, whatever bin each lane holds.  A 16-byte read is served in four groups of 16 lanes, each of
// which holds every residue of lane mod 16 once -- 16 slots of 4 banks, the 64 banks; a 16-byte write in eight groups of 8
// consecutive lanes -- 8 slots of 4 banks, the 32 banks a write sees: no conflicts either way.
//
// Budget.  The LDS limits the waves on a CU, nothing else does (the kernel needs few registers): 16 nbins R bytes per
// lane, at most 160 KiB / (1 KiB nbins R) waves.  The plan keeps two workgroups on a CU, MTG_EF_LDS_BUDGET = 80 KiB each
// with the staged chunk (mtg_ls_tile.h: 2 KiB of elapsed times and 4 KiB per weighted light curve or unweighted pair),
// so that one workgroup's barrier and staging overlap the other's sweep: the largest tile of 1, 2, 4 that fits with
// 256 lanes, and where not even one light curve does (nbins > 18) 128 lanes and a tile of one.  Narrow frequency lists
// run 64 or 128 lanes as the Lomb-Scargle sweep does.  A power does not depend on any of this.
#ifndef MTG_EF_PLAN_H
#define MTG_EF_PLAN_H

#include <stdint.h>

enum { MTG_EF_LDS_BUDGET = 80 * 1024, MTG_EF_CHUNK = 256 };
// light curves per launch of mtg_phase_fold, whose outputs (at most MTG_PF_MAX_ENTRIES entries each, include/mtg.h) stay
// whole on the device: a multiple of every tile; the counts' grid has a row per light curve
enum { MTG_PF_SLAB = 32768 };

struct MtgEfPlan {
    int tile;        // light curves per lane: 1, 2 or 4
    int lanes;       // 64, 128 or 256
    int acc_bytes;   // the bins' sums (dynamic LDS)
    int lds_bytes;   // with the staged chunk
};

// bytes of the bins' sums of one workgroup
static constexpr int mtg_ef_acc_bytes(int nbins, int tile, int lanes, int weighted)
{
    return (weighted || tile == 1) ? 16 * tile * nbins * lanes : (8 + 8 * tile) * nbins * lanes;
}

// bytes of the staged chunk: elapsed times, then the columns of mtg_ls_tile.h
static constexpr int mtg_ef_chunk_bytes(int tile, int weighted)
{
    return 8 * MTG_EF_CHUNK + 16 * MTG_EF_CHUNK * (weighted ? tile : (tile + 1) / 2);
}

// nbins in 2 .. 32 (the caller's check); F frequencies, L light curves
static inline MtgEfPlan mtg_ef_plan(int nbins, int64_t F, int64_t L, int shared_sampling, int weighted)
{
    MtgEfPlan p;
    p.lanes = F <= 64 ? 64 : F <= 128 ? 128 : 256;
    p.tile = 1;
    if (shared_sampling && L > 1)
        for (int r = 2; r <= 4; r *= 2)
            if (mtg_ef_acc_bytes(nbins, r, p.lanes, weighted) + mtg_ef_chunk_bytes(r, weighted) <= MTG_EF_LDS_BUDGET) p.tile = r;
    while (p.lanes > 64 && mtg_ef_acc_bytes(nbins, 1, p.lanes, weighted) + mtg_ef_chunk_bytes(1, weighted) > MTG_EF_LDS_BUDGET) p.lanes /= 2;
    p.acc_bytes = mtg_ef_acc_bytes(nbins, p.tile, p.lanes, weighted);
    p.lds_bytes = p.acc_bytes + mtg_ef_chunk_bytes(p.tile, weighted);
    return p;
}

#endif
