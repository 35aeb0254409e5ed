// bft_paths.h -- the path engine (bft_paths.hip): maximal non-branching paths over one of two vertex models of the sorted T-form table.
//   rows      a vertex is a stored k-mer: the simple paths (bft_gpu_simple_paths, bft_paths.hip)
//   mirrored  a vertex is an oriented k-mer 2 * row + o (o = 0 reads the stored k-mer, o = 1 its reverse complement; v ^ 1 is its flip), every path
//             occurs as itself and as its mirror, and one of the two is kept: the canonical unitigs (bft_gpu_unitigs, bft_unitigs.hip)
// A family brings its own degrees and links (different predicates) and shares everything behind them: jumps, ends, scans, offsets, spelling, the
// handle's scratch and both forms of the entry point.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bft_handle.h"

// succ[u]: the vertex of u's only stored successor, or one of these
#define BFT_SP_NONE 0xFFFFFFFFu  // no stored successor
#define BFT_SP_MANY 0xFFFFFFFEu  // two or more
// flags[u]
#define BFT_SP_NODE 1u      // in <= 1, out <= 1, colour set of t genomes or more
#define BFT_SP_OUT 2u       // an edge leaves u
#define BFT_SP_IN 4u        // an edge enters u

// Per-vertex arrays of one call, m vertices of room (carved out of the handle's block, bft_sp_scratch).
struct BftSpScratch {
    uint32_t* start;  // [2^sb + 1] first row of every bucket of the top sb bits of the T-form
    uint8_t* deg;     // [rows] mirrored only: the degree byte of a row (bft_unitigs.h)
    uint32_t* succ;   // [m]
    uint32_t* indeg;  // [m] rows: stored predecessors (atomic counts).  Then the length in characters of the path a head starts (mirrored: of the
                      //     KEPT path, 0 where the head's path is the mirror that is not reported)
    uint32_t* pred;   // [m] rows: a stored predecessor (the only one when indeg == 1).  Then the number of the path a head starts
    uint8_t* flags;   // [m]
    uint4* st[2];     // [m] pointer jumping, ping-pong: {back pointer, steps, smallest vertex of the window, steps to it}
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
// one round of pointer jumping st[from] -> st[from ^ 1] over nv vertices
int bft_sp_jump(uint64_t nv, const BftSpScratch& p, int from, hipStream_t s);
// the head/distance pairs the ends write over st[fin ^ 1]
static inline const uint2* bft_sp_hd(const BftSpScratch& p, int fin) { return reinterpret_cast<const uint2*>(p.st[fin ^ 1]); }

// heads (input of the scan that numbers the paths in ascending id of their first vertex); MIRRORED: heads of kept paths
template <bool MIRRORED>
struct BftSpHeadOf {
    const uint2* hd;
    uint64_t n;
    const uint32_t* len = nullptr;  // (read where MIRRORED alone)
    __host__ __device__ uint32_t operator()(uint64_t i) const { return i < n && hd[i].x == (uint32_t)i && (!MIRRORED || len[i] != 0u) ? 1u : 0u; }
};
using BftSpHead = BftSpHeadOf<false>;
// characters of the path a head starts (input of the scan that places the paths)
struct BftSpHeadLen {
    const uint2* hd;
    const uint32_t* len;
    uint64_t n;
    __host__ __device__ uint64_t operator()(uint64_t i) const { return i < n && hd[i].x == (uint32_t)i ? (uint64_t)len[i] : 0ull; }
};

// What tells the two families apart on the host.
struct BftPathFamily {
    bool mirrored;             // vertices: false = the n rows, true = the 2n oriented rows
    uint32_t counts_bytes;     // of d_counts = {n_paths, n_chars, longest[, the family's own]}: 24, 32 or 48
    const char* name;          // first word of every stage name and of the limit's message
    const char* ends_stage;    // the stage of the ends (named by what the family's ends decide)
    const char* capture_msg;   // a capturing stream is refused with this
    const char* nospace_msg;   // the host-buffer form's caps do not hold the paths
    // the family's own steps on stream s, each a stage: whatever it counts into d_counts + 3, the buckets, succ[] (and what its links read), then
    // flags[] and st[0].  d_counts and indeg[] are zeroed
    int (*front)(bft_gpu* h, uint32_t min_shared, hipStream_t s, unsigned long long* d_counts, const BftSpScratch& p);
    // the host-buffer form, after the read-back of the counts and before anything is reported: may refuse the index (null: nothing to check)
    int (*check)(const unsigned long long* counts);
};
// The built index with its table resident, for a call named `what`: no more than 2^31 - 1 k-mers (vertex ids stay below BFT_SP_MANY)
int bft_sp_prepare(bft_gpu* h, const char* what);
// The handle's scratch (h->sp with h->sp_buf / h->sp_tmp, bft_handle.h) on stream s, acquired through `lease` (of h->sp): arrays with room for m
// vertices (0: none -- the bucket starts alone), the scans' temporary for nv <= m of them, a degree byte for each of deg_rows rows (0: none).
// The block is sized exactly for m
int bft_sp_scratch(bft_gpu* h, HandleScratch::Lease& lease, uint64_t m, uint64_t nv, uint64_t deg_rows, hipStream_t s, BftSpScratch* p);
// The steps of a call of family f on stream s, for a caller that puts work of its own between them (bft_cgraph.hip).  d_counts: f.counts_bytes.
//   bft_paths_scratch  the family's scratch through `lease`
//   bft_paths_trace    d_counts zeroed; the family's front, the jumps, the ends: {head, distance} per vertex (bft_sp_hd(p, *fin)), the length of each
//                      (kept) path at its head's indeg[], the longest into d_counts[2].  st[*fin] is free afterwards
//   bft_paths_number   both scans: pred[] = the number of the path a (kept) head starts, choff[] = where it begins; d_counts[0 .. 1]
//   bft_paths_emit     offsets (paths_cap + 1 entries at most) and characters (below chars_cap); either may be null
int bft_paths_scratch(bft_gpu* h, const BftPathFamily& f, HandleScratch::Lease& lease, hipStream_t s, BftSpScratch* p);
int bft_paths_trace(bft_gpu* h, const BftPathFamily& f, uint32_t min_shared, hipStream_t s, unsigned long long* d_counts, const BftSpScratch& p, int* fin);
int bft_paths_number(bft_gpu* h, const BftPathFamily& f, hipStream_t s, unsigned long long* d_counts, const BftSpScratch& p, int fin);
int bft_paths_emit(bft_gpu* h, const BftPathFamily& f, const BftSpScratch& p, int fin, uint64_t* d_offsets, uint64_t paths_cap, char* d_seqs, uint64_t chars_cap,
                   const unsigned long long* d_counts, hipStream_t s);
// bft_gpu_simple_paths_dev / bft_gpu_unitigs_dev and bft_gpu_simple_paths / bft_gpu_unitigs for the family f (include/bft_gpu.h)
int bft_paths_dev(bft_gpu* h, const BftPathFamily& f, uint32_t min_shared, void* d_offsets, void* d_seqs, uint64_t paths_cap, uint64_t chars_cap, void* d_counts,
                  void* hip_stream);
int bft_paths_host(bft_gpu* h, const BftPathFamily& f, uint32_t min_shared, uint64_t* offsets, char* seqs, uint64_t paths_cap, uint64_t chars_cap,
                   uint64_t* n_paths, uint64_t* n_chars);
