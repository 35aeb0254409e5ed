// bft_setops.h -- colour-set algebra over groups of k-mers (bft_setops.hip): what the kernels of bft_gpu_combine_colors / bft_gpu_combine_colorsets share.
// The class bounds below and the kernels' grids reach the tests through bft_gpu_debug_setops_plan: no test repeats a literal of this file.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define BFT_SO_ABSENT 0xFFFFFFFFu   // the colour set of an absent k-mer (BFT_ABSENT_ROW: what the query kernels and bft_gpu_query_rows write)
#define BFT_SO_NONE 0xFFFFFFFEu     // no colour set yet (the start of a run; never an id: an index holds fewer than 2^31 sets)
#define BFT_SO_SMALL 16u            // groups up to this size: a lane per (group, word of the row) -- k_so_small
#define BFT_SO_WAVE_MAX 65536u      // groups up to this size: a wavefront per group -- k_so_wave; larger ones are split -- k_so_split
#define BFT_SO_CHUNK 4096u          // members per wavefront and step of a split group

// The dictionary in the form the call found: bm != NULL, rows of stride32 dwords (bft_ensure_cs_bitmaps), else the sorted id lists.
struct BftSoDict {
    const uint32_t* bm;
    uint32_t stride32;
    const uint32_t* cs_off;
    const void* cs_ids;
    uint32_t cs_w, n_sets;
    uint32_t G, nw;  // genomes; 32-bit words of a row = CEIL(G / 32)
};

// Arrays of one call (carved out of the handle's block): n k-mers, ng groups, nw words per row.
struct BftSoScratch {
    uint32_t* cs;                // [n] colour set per k-mer (the k-mer form only: the colour-set form reads the caller's array)
    uint64_t* bits;              // [CEIL(n / 64)] presence bits of the lookup (the k-mer form only)
    uint32_t* R;                 // [ng x nw] the result rows, dword stride; while a split group is reduced: its OR (AND for op AND) accumulator
    uint32_t* X;                 // [ng x nw] SYMDIFF only: the AND accumulator of the split groups
    uint32_t* nfound;            // [ng] found members per group (when the caller does not ask for them)
    unsigned long long* nsplit;  // [1] number of split groups
    uint32_t* split;             // [ng] their numbers, in no particular order
};

struct BftSoBatch {
    const uint32_t* cs;   // colour set per member, BFT_SO_ABSENT for an absent one
    uint64_t n;           // members of the batch
    const uint64_t* off;  // [ng + 1]
    uint64_t ng;
    int op, skip;
    uint32_t *R, *X, *nf;
};

int bft_so_reduce(const BftSoDict& d, const BftSoBatch& b, const BftSoScratch& p, hipStream_t s, int step);  // step 0..4: plan, small, wave, split, finish
int bft_so_emit(const BftSoDict& d, const uint32_t* R, uint64_t ng, uint8_t* d_rows, hipStream_t s);
int bft_so_count(const BftSoDict& d, const uint32_t* R, uint64_t ng, uint32_t* d_counts, hipStream_t s);
