// bft_cgraph.h -- the compacted coloured graph of a canonical index (bft_cgraph.hip): the unitigs' segments completed by the branching k-mers, the
// links between oriented segments, the members of every segment and a colour row per segment.  include/bft_gpu.h defines them.  The call runs the
// mirrored family of the path engine (bft_paths.h, bft_unitigs.h) up to its ends, turns every eligible row that is no node into a kept path of one
// vertex, and lets the engine number, place and spell the lot; members and links are its own.  Beside BftSpScratch's arrays it uses what the ends
// left free, for nv = 2n vertices:
//   succ[]                    [nv] u32    the last vertex of every oriented segment (its end)
//   st[fin]                   [nv] uint4  the at most four link targets of every oriented segment, ascending, BFT_SP_NONE behind them
//   st[fin ^ 1], upper half   [nv] u64    where the link list of an oriented segment begins ({head, distance} per vertex is the lower half)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bft_paths.h"

struct BftCgScratch {
    uint2* hd;       // [nv] {head, distance} of every vertex of a path (the ends'), and of the singles
    uint32_t* endv;  // [nv]
    uint4* tgt;      // [nv]
    uint64_t* loff;  // [nv]
};
static inline BftCgScratch bft_cg_scratch(const BftSpScratch& p, int fin, uint64_t nv) {
    uint8_t* const upper = reinterpret_cast<uint8_t*>(p.st[fin ^ 1]) + nv * 8;
    return BftCgScratch{reinterpret_cast<uint2*>(p.st[fin ^ 1]), p.succ, p.st[fin], reinterpret_cast<uint64_t*>(upper)};
}

// link lists per oriented segment (input of the scan that places them): the targets that are set, for the oriented segments that exist
struct BftCgLinkCount {
    const uint4* tgt;
    const unsigned long long* counts;  // counts[0] = n_segments
    uint64_t nv;
    __device__ __forceinline__ uint64_t operator()(uint64_t a) const {
        if (a >= nv || a >= 2ull * counts[0]) return 0ull;
        const uint4 t = tgt[a];
        return (uint64_t)((t.x != BFT_SP_NONE) + (t.y != BFT_SP_NONE) + (t.z != BFT_SP_NONE) + (t.w != BFT_SP_NONE));
    }
};
