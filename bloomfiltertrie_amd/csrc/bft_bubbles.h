// bft_bubbles.h -- simple bubbles (variants) on the compacted coloured graph, and the k-mer -> segment table (bft_bubbles.hip: bft_gpu_unitig_bubbles /
// _dev, bft_gpu_unitig_segment_of / _dev; include/bft_gpu.h defines them).  Both read the arrays bft_gpu_unitig_graph returned, not the index.  The
// scratch is the handle's own block for them (h->bb with h->bb_buf / h->bb_tmp, bft_handle.h), for 2S oriented segments:
//   flag[]   [2S] u8   1: the oriented segment is the source of a reported bubble
//   slot[]   [2S] u32  the exclusive scan of the flags: where its record goes
// The k-mer -> segment table needs no scratch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr uint32_t BFT_BB_NONE = 0xFFFFFFFFu;

struct BftBbScratch {
    uint8_t* flag;   // [2S]
    uint32_t* slot;  // [2S]
};

// bubbles per oriented segment (input of the scan that places the records): the flag, over exactly the 2S lanes of the call
struct BftBbFlag {
    const uint8_t* flag;
    __device__ __forceinline__ uint32_t operator()(uint64_t a) const { return (uint32_t)flag[a]; }
};
