// bft_components.h -- connected components of the index (bft_components.hip): the launchers bft_gpu_components chains with the library's scans.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bft_paths.h"

#define BFT_CC_NONE 0xFFFFFFFFu  // parent[] of a row that is not a member; the label of a non-member
#define BFT_CC_IDS 64            // requested genome ids per k_cc_sets launch (they travel as kernel arguments)

// Per-row arrays of one call, m rows of room (carved out of the handle's block by the caller).
struct BftCcScratch {
    BftSpScratch sp;   // only sp.start (2^sb + 1 bucket starts) and sp.sb: bft_sp_buckets
    uint32_t* parent;  // [m] union-find forest (a root is the smallest row of its tree; BFT_CC_NONE: not a member); then the sizes per component
    uint32_t* num;     // [m] exclusive scans (members, then roots); then the label of every row
    uint8_t* member;   // [sets] the colour set holds every requested id
};

// member[cs] for the n_sets colour sets of the dictionary cs_off / cs_ids (cs_w bytes per id): the sorted id list holds ids[0 .. nb) (nb <= BFT_CC_IDS,
// strictly increasing); first = 0 ANDs into what an earlier launch wrote (more than BFT_CC_IDS ids)
int bft_cc_sets(uint64_t n_sets, const uint32_t* d_cs_off, const void* d_cs_ids, uint32_t cs_w, const uint32_t* ids, uint32_t nb, bool first, const BftCcScratch& p,
                hipStream_t s);
// parent[u] = u for a member, BFT_CC_NONE otherwise (d_tcol NULL: every row is a member).  d_marks (bft_marking.h's flag words; NULL: no such
// condition): a member must also hold the vertex flag `through`
int bft_cc_init(uint64_t n, const uint32_t* d_tcol, const BftCcScratch& p, hipStream_t s, const uint32_t* d_marks = nullptr, uint32_t through = 0);
// every member row joined with its member successors (lock-free union-find; start[] from bft_sp_buckets)
int bft_cc_hook(int W, const uint64_t* d_tk, uint64_t n, int k, const BftCcScratch& p, hipStream_t s);
// parent[u] = the root of u
int bft_cc_flatten(uint64_t n, const BftCcScratch& p, hipStream_t s);
// num[u] = label of u (num[root] is the component number after the roots' scan), also into d_labels when not NULL; parent[] zeroed for the sizes
int bft_cc_label(uint64_t n, const BftCcScratch& p, uint32_t* d_labels, hipStream_t s);
// parent[c] = members in component c
int bft_cc_count(uint64_t n, const BftCcScratch& p, hipStream_t s);
// d_sizes[c] for c < min(n_components, sizes_cap) when d_sizes is not NULL; the largest component into d_counts[2] (zeroed by the caller).
// d_counts[0] = n_components, from the roots' scan
int bft_cc_sizes(uint64_t n, const BftCcScratch& p, uint64_t* d_sizes, uint64_t sizes_cap, unsigned long long* d_counts, hipStream_t s);

// members (input of the scan that counts them)
struct BftCcMember {
    const uint32_t* parent;
    __host__ __device__ uint32_t operator()(uint64_t i) const { return parent[i] != BFT_CC_NONE ? 1u : 0u; }
};
// roots, after bft_cc_flatten (input of the scan that numbers the components in row order of their roots, which are their smallest rows)
struct BftCcRoot {
    const uint32_t* parent;
    __host__ __device__ uint32_t operator()(uint64_t i) const { return parent[i] == (uint32_t)i ? 1u : 0u; }
};
