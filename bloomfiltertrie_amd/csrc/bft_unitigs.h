// bft_unitigs.h -- canonical (bidirected) unitigs and degrees of the index (bft_unitigs.hip): the launchers bft_gpu_unitigs chains with the jumps of
// the simple paths (bft_sp_jump, bft_paths.h) and the library's scans.  An oriented vertex is 2 * row + o: o = 0 reads the stored k-mer, o = 1 its
// reverse complement; v ^ 1 is its flip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bft_paths.h"

// degree byte of a row: out(s,0) << 4 | out(s,1), each 0..4 (the layout of bft_gpu_query_branching's counts); inside bft_gpu_unitigs also
#define BFT_UG_PAL 0x08u  // s == rc(s): the row is always a path of its own

// Arrays of one call over m rows (2m oriented vertices).  `sp` is carved with room for 2m entries per array and read as follows:
//   succ[v]   the only successor vertex of v, or BFT_SP_NONE / BFT_SP_MANY
//   indeg[v]  the length in characters of the KEPT path that head v starts (0: v starts no kept path)
//   pred[v]   the number of the path a head starts
//   flags[v]  BFT_SP_NODE | BFT_SP_OUT | BFT_SP_IN
//   st, choff as for the simple paths
struct BftUgScratch {
    BftSpScratch sp;
    uint8_t* deg;  // [m] degree byte per row (| BFT_UG_PAL)
};

// rows whose stored k-mer is greater than its reverse complement, added to *d_noncanonical (zeroed by the caller)
int bft_ug_canonicity(int W, const uint64_t* d_tk, uint64_t n, int k, unsigned long long* d_noncanonical, hipStream_t s);
// the degree byte of the rows below deg_cap (pal: with BFT_UG_PAL) and, where d_succ is not null, succ[] of all 2n vertices; p.start from bft_sp_buckets
int bft_ug_degrees(int W, const uint64_t* d_tk, uint64_t n, int k, const BftSpScratch& p, uint8_t* d_deg, uint64_t deg_cap, bool pal, uint32_t* d_succ,
                   hipStream_t s);
// nodes, edges and the first state of the jumps (st[0]) of the 2n vertices
int bft_ug_links(uint64_t n, uint32_t t, const uint32_t* d_tcol, const uint32_t* d_cs_off, const void* d_cs_ids, uint32_t cs_w, const BftUgScratch& p, hipStream_t s);
// the final state st[fin] -> {head, steps from the head} per node vertex (over st[fin ^ 1] as uint2); the tail of a kept path writes its length at its
// head's indeg[] (zeroed by the caller); the longest kept path into *d_longest
int bft_ug_ends(uint64_t n, int k, const BftUgScratch& p, int fin, unsigned long long* d_longest, hipStream_t s);
// heads of kept paths (input of the scan that numbers them in ascending vertex id) and their characters (input of the scan that places them)
struct BftUgHead {
    const uint2* hd;
    const uint32_t* len;
    uint64_t n2;
    __host__ __device__ uint32_t operator()(uint64_t i) const { return i < n2 && hd[i].x == (uint32_t)i && len[i] != 0u ? 1u : 0u; }
};
struct BftUgHeadLen {
    const uint2* hd;
    const uint32_t* len;
    uint64_t n2;
    __host__ __device__ uint64_t operator()(uint64_t i) const { return i < n2 && hd[i].x == (uint32_t)i ? (uint64_t)len[i] : 0ull; }
};
// offsets[path] for the kept heads and offsets[n_paths] = n_chars (d_counts = {n_paths, n_chars}), each only where it is below paths_cap + 1
int bft_ug_offsets(uint64_t n, const BftUgScratch& p, int fin, uint64_t* d_offsets, uint64_t paths_cap, const unsigned long long* d_counts, hipStream_t s);
// the nucleotides of every vertex of a kept path, as ASCII, below chars_cap
int bft_ug_spell(int W, const uint64_t* d_tk, uint64_t n, int k, const BftUgScratch& p, int fin, char* d_seqs, uint64_t chars_cap, hipStream_t s);
