// bft_paths.h -- simple paths (unitigs) of the index (bft_paths.hip): the launchers bft_gpu_simple_paths chains with the library's scans.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// succ[u]: the row of u's only stored successor, or one of these
#define BFT_SP_NONE 0xFFFFFFFFu  // no stored successor
#define BFT_SP_MANY 0xFFFFFFFEu  // two or more
// flags[u]
#define BFT_SP_NODE 1u      // in <= 1, out <= 1, colour set of t genomes or more
#define BFT_SP_OUT 2u       // an edge leaves u
#define BFT_SP_IN 4u        // an edge enters u

// Per-row arrays of one call, m rows of room (carved out of the handle's block by the caller).
struct BftSpScratch {
    uint32_t* start;  // [2^sb + 1] first row of every bucket of the top sb bits of the T-form
    uint32_t* succ;   // [m]
    uint32_t* indeg;  // [m] stored predecessors (atomic counts); then the length of the path a head starts
    uint32_t* pred;   // [m] a stored predecessor (the only one when indeg == 1); then the number of the path a head starts
    uint8_t* flags;   // [m]
    uint4* st[2];     // [m] pointer jumping, ping-pong: {back pointer, steps, smallest row of the window, steps to it}
    uint64_t* choff;  // [m] where the path a head starts begins, in characters
    int sb;           // bucket bits
};
// bucket bits for a table of k-mers: the top 20 bits of the T-form (all 18 of it at k = 9)
static inline int bft_sp_bucket_bits(int k) { return 2 * k < 20 ? 2 * k : 20; }

// start[] over the n sorted rows of tk
int bft_sp_buckets(int W, const uint64_t* d_tk, uint64_t n, int k, const BftSpScratch& p, hipStream_t s);
// out-degree and the successor's row of every row; in-degree and a predecessor by scattering over the successors (indeg zeroed by the caller)
int bft_sp_degrees(int W, const uint64_t* d_tk, uint64_t n, int k, const BftSpScratch& p, hipStream_t s);
// nodes, edges (t = min_shared: colour sets from tcol and the dictionary cs_off / cs_ids of cs_w bytes per id) and the first state of the jumps (st[0])
int bft_sp_links(uint64_t n, uint32_t t, const uint32_t* d_tcol, const uint32_t* d_cs_off, const void* d_cs_ids, uint32_t cs_w, const BftSpScratch& p, hipStream_t s);
// one round of pointer jumping st[from] -> st[from ^ 1]
int bft_sp_jump(uint64_t n, const BftSpScratch& p, int from, hipStream_t s);
// the final state st[fin] -> {head row, steps from the head} per node (written over st[fin ^ 1] as uint2), the length of each path at its head's
// indeg[], the longest path into *d_longest (zeroed by the caller)
int bft_sp_ends(uint64_t n, int k, const BftSpScratch& p, int fin, unsigned long long* d_longest, hipStream_t s);
// the head/distance pairs bft_sp_ends wrote
static inline const uint2* bft_sp_hd(const BftSpScratch& p, int fin) { return reinterpret_cast<const uint2*>(p.st[fin ^ 1]); }

// heads (input of the scan that numbers the paths in row order)
struct BftSpHead {
    const uint2* hd;
    uint64_t n;
    __host__ __device__ uint32_t operator()(uint64_t i) const { return i < n && hd[i].x == (uint32_t)i ? 1u : 0u; }
};
// characters of the path a head starts (input of the scan that places the paths)
struct BftSpHeadLen {
    const uint2* hd;
    const uint32_t* len;
    uint64_t n;
    __host__ __device__ uint64_t operator()(uint64_t i) const { return i < n && hd[i].x == (uint32_t)i ? (uint64_t)len[i] : 0ull; }
};
// offsets[pid] for the heads and offsets[n_paths] = n_chars (d_counts = {n_paths, n_chars}), each only where it is below paths_cap + 1
int bft_sp_offsets(uint64_t n, const BftSpScratch& p, int fin, uint64_t* d_offsets, uint64_t paths_cap, const unsigned long long* d_counts, hipStream_t s);
// the nucleotides of every node, as ASCII, below chars_cap
int bft_sp_spell(int W, const uint64_t* d_tk, uint64_t n, int k, const BftSpScratch& p, int fin, char* d_seqs, uint64_t chars_cap, hipStream_t s);
