// bft_prefix.h -- batched prefix matching (bft_prefix.hip): the launchers the entry points there chain with the library's scans.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bft_walk.h"  // BFT_HD

// workgroups of k_pm_count / k_pm_emit: each takes one contiguous chunk of the batch's candidates
#define BFT_PM_CHUNKS 2048
// threads of a workgroup of the k_pm_* kernels = candidates of a tile
constexpr int PM_THREADS = 256;

// Chunk g (of G) of the candidates [0, C): whole tiles, one chunk per workgroup.  The one definition of the rule: k_pm_count and k_pm_emit call
// it, and bft_gpu_debug_prefix_plan hands it to the tests (tests/test_prefix_cases_host.py) without a device.
BFT_HD void pm_chunk(uint64_t C, uint32_t g, uint32_t G, uint64_t* begin, uint64_t* end, uint64_t* size = nullptr) {
    uint64_t cs = (C + G - 1) / G;
    cs = (cs + PM_THREADS - 1) / PM_THREADS * PM_THREADS;
    const uint64_t b = (uint64_t)g * cs;
    *begin = b < C ? b : C;
    *end = *begin + cs < C ? *begin + cs : C;
    if (size) *size = cs;
}

// Per-batch arrays, carved out of one block of the handle's (n = prefixes of the batch):
struct BftPmScratch {
    uint32_t* a;          // [n] first row of prefix i's interval
    uint32_t* filt;       // [n] its filter (k_pm_bounds), 0xFFFFFFFF = none
    uint64_t* cand;       // [n] rows in the interval
    uint64_t* coff;       // [n + 1] exclusive scan of cand (coff[n] = candidates of the batch)
    uint64_t* kept;       // [n] matches of prefix i (the caller scans them into the call's offsets)
    uint64_t* chunk;      // [BFT_PM_CHUNKS] matches per chunk of candidates
    uint64_t* chunk_off;  // [BFT_PM_CHUNKS + 1] exclusive scan of chunk
};

// intervals, filters, candidate counts; kept[i] = candidates of the prefixes without a filter, 0 for the others
int bft_pm_bounds(int W, const uint8_t* d_prefixes, const uint8_t* d_lengths, uint64_t n, int k, int B, const uint64_t* d_tk, uint64_t n_rows,
                  const BftPmScratch& p, hipStream_t s);
// (after coff) adds the matches of the filtered prefixes to kept, writes chunk
int bft_pm_count(int W, uint64_t n, const uint64_t* d_tk, const BftPmScratch& p, hipStream_t s);
// (after chunk_off) the first cap matches: packed k-mers (B bytes each), rows, colour sets; any output may be NULL
int bft_pm_emit(int W, uint64_t n, int k, int B, const uint64_t* d_tk, const uint32_t* d_tcol, const BftPmScratch& p, uint64_t cap, uint8_t* d_kmers_out,
                uint32_t* d_rows_out, uint32_t* d_cs_out, hipStream_t s);
