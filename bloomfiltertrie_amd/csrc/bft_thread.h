// bft_thread.h -- sequence threading through the compacted coloured graph (bft_thread.hip: bft_gpu_thread_sequences / _dev; include/bft_gpu.h defines
// the walks).  The call reads the sorted table of the index, the arrays bft_gpu_unitig_graph and bft_gpu_unitig_segment_of returned, and a batch of
// sequences.  The scratch is the handle's own block for it (h->th with h->th_buf / h->th_tmp, bft_handle.h), for a batch of C characters -- a
// sequence has no more k-mer positions than characters, so every per-position array holds C entries:
//   codes[]  [C / 32 + slack] u64  two bits per character           (k_seq_encode)
//   bad[]    [C / 32 + slack] u32  one "not ACGTU" bit per character
//   npos[], poff[]  [n_seqs + 1] u64  positions per sequence and their exclusive scan (k_seq_plan)
//   tile[]   [C / 64 + 2] u32      the sequence of the first position of every 64 positions (k_seq_tiles)
//   start[]  [2^sb + 1] u32        first row of every bucket of the table (k_sp_buckets), the call's own copy
//   loc[]    [C] 2 x u32           {oriented segment X, index q} of a located position, or {BFT_TH_NONE, reason}
//   flag[]   [C] u8                BFT_TH_LOCATED | BFT_TH_WALK | BFT_TH_STEP (0 behind the last position)
//   widx[]   [C] u32               the exclusive scan of the walk starts: the walk a start opens
//   sidx[]   [C] u32               the exclusive scan of the step starts: where a step goes
// 17 bytes per position, 0.375 per character and 4 per bucket.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr uint32_t BFT_TH_NONE = 0xFFFFFFFFu;
// why a position is not located (loc[p].y where loc[p].x == BFT_TH_NONE)
constexpr uint32_t BFT_TH_INVALID = 0u, BFT_TH_ABSENT = 1u, BFT_TH_NOSEG = 2u;
// flag[p]
constexpr uint32_t BFT_TH_LOCATED = 1u;  // the position is located
constexpr uint32_t BFT_TH_WALK = 2u;     // ... and opens a walk (and its first step)
constexpr uint32_t BFT_TH_STEP = 4u;     // ... and opens a step

struct BftThScratch {
    uint64_t* codes;
    uint32_t* bad;
    uint64_t *npos, *poff;
    uint32_t* tile;
    uint32_t* start;
    uint2* loc;
    uint8_t* flag;
    uint32_t *widx, *sidx;
};

// walks and steps opened per position (inputs of the two scans that number them: two functors over the one flag byte, two passes of 5 bytes per
// position -- a packed 64-bit sum would halve the passes but holds 2^31 of each at most, and a batch has up to 2^32 - 1 positions)
template <uint32_t BIT>
struct BftThFlag {
    const uint8_t* flag;
    __device__ __forceinline__ uint32_t operator()(uint64_t p) const { return (flag[p] & BIT) ? 1u : 0u; }
};
