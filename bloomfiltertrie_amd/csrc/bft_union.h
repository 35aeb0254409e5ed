// bft_union.h -- merging two indexes (bft_union.hip): the co-ranked placement of two sorted k-mer tables and the shift of a dictionary's genome ids.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bft_dev.h"
#include "bft_merge.h"  // BftRun

// Keys of the merged diagonal one workgroup places (k_un_count / k_un_emit).  A tile stages at most BFT_UNION_TILE + 1 rows in LDS (the + 1: the second
// half of a pair of equal keys that would straddle the tile's end is taken in): 32.8 KB at W = 4, so four workgroups of 256 threads per CU.
#define BFT_UNION_TILE 1024
#define BFT_UNION_THREADS 256

// The placement of merge_w (bft_merge.hip) for two tables of similar size, both streamed instead of one searched: the merged table's keys tk (n_o rows
// of W words), per merged row the colour set of a's row (pa) and of b's row (pb), 0xFFFFFFFF where that side does not hold the key, and per row of b
// its merged row (orow).  Both sides non-empty, sorted, distinct.  The launches are timed on `timed` ("timing") when it is not NULL.  Synchronises.
int bft_union_place(int W, const BftRun& a, const BftRun& b, hipStream_t s, bft_gpu* timed, DevBuf& tk, DevBuf& pa, DevBuf& pb, DevBuf& orow, uint64_t* n_o);

// out[i] = in[i] + base for the n genome ids of a dictionary kept w bytes per id (1 / 2 / 4)
int bft_union_shift_ids(const void* d_in, uint32_t w, uint64_t n, uint32_t base, uint32_t* d_out, hipStream_t s);
