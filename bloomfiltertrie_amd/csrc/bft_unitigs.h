// bft_unitigs.h -- canonical (bidirected) unitigs and degrees of the index (bft_unitigs.hip): the mirrored family of the path engine (bft_paths.h).
// An oriented vertex is 2 * row + o: o = 0 reads the stored k-mer, o = 1 its reverse complement; v ^ 1 is its flip.  The family's own launchers
// are its degrees and links; BftSpScratch holds 2m entries per array for m rows and is read as follows:
//   deg[row]  the degree byte of a row (| BFT_UG_PAL)
//   succ[v]   the only successor vertex of v, or BFT_SP_NONE / BFT_SP_MANY
//   indeg[v]  the length in characters of the KEPT path that head v starts (0: v starts no kept path)
//   pred[v]   the number of the path a head starts
//   flags[v]  BFT_SP_NODE | BFT_SP_OUT | BFT_SP_IN
//   st, choff as for the simple paths
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bft_paths.h"

// degree byte of a row: out(s,0) << 4 | out(s,1), each 0..4 (the layout of bft_gpu_query_branching's counts); inside bft_gpu_unitigs also
#define BFT_UG_PAL 0x08u  // s == rc(s): the row is always a path of its own

// rows whose stored k-mer is greater than its reverse complement, added to *d_noncanonical (zeroed by the caller)
int bft_ug_canonicity(int W, const uint64_t* d_tk, uint64_t n, int k, unsigned long long* d_noncanonical, hipStream_t s);
// the degree byte of the rows below deg_cap (pal: with BFT_UG_PAL) and, where d_succ is not null, succ[] of all 2n vertices; p.start from bft_sp_buckets
int bft_ug_degrees(int W, const uint64_t* d_tk, uint64_t n, int k, const BftSpScratch& p, uint8_t* d_deg, uint64_t deg_cap, bool pal, uint32_t* d_succ,
                   hipStream_t s);
// nodes, edges and the first state of the jumps (st[0]) of the 2n vertices
int bft_ug_links(uint64_t n, uint32_t t, const uint32_t* d_tcol, const uint32_t* d_cs_off, const void* d_cs_ids, uint32_t cs_w, const BftSpScratch& p, hipStream_t s);
// The unitigs' front (the BftPathFamily::front of the mirrored family) with its stages named "<family>: ...": canonicity (into d_counts[3]), buckets,
// degrees of both orientations, links.  bft_ug_check: the family's check (BFT_GPU_E_STATE where counts[3] != 0)
int bft_ug_front(bft_gpu* h, const char* family, uint32_t min_shared, hipStream_t s, unsigned long long* d_counts, const BftSpScratch& p);
int bft_ug_check(const unsigned long long* counts);
