// bft_subgraph.h -- sub-graph builds (bft_subgraph.hip): the launchers bft_gpu_subgraph chains with the library's sort and scans.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// The found k-mers of a batch (presence bits + colour-set id per k-mer, what the query kernels write with emit_cs) as records:
// T-form key words (SoA, word w of record r at keys[w * stride + r]) and the colour-set id.  *d_count (zeroed by the caller) receives the
// number of records; their order is not defined (the caller sorts them).
int bft_sg_compact(int W, const uint8_t* d_kmers, uint64_t n, int k, int B, const uint64_t* d_bits64, const uint32_t* d_cs, uint64_t* d_keys, uint64_t stride,
                   uint32_t* d_vals, unsigned long long* d_count, hipStream_t s);

// Row i of sorted records starts a run of equal keys (the input of the de-duplication scan): 1 or 0
struct BftSgHeads {
    const uint64_t* keys;  // SoA, stride
    uint64_t stride, n;
    int W;
    __host__ __device__ uint32_t operator()(uint64_t i) const {
        if (i >= n) return 0u;
        if (i == 0) return 1u;
        for (int w = 0; w < W; w++)
            if (keys[(uint64_t)w * stride + i] != keys[(uint64_t)w * stride + i - 1]) return 1u;
        return 0u;
    }
};
// the first record of every run (pos: exclusive scan of BftSgHeads) -> row pos[i] of the table (tk: W words per row) and its colour set
int bft_sg_scatter(int W, const uint64_t* d_keys, uint64_t stride, const uint32_t* d_vals, uint64_t n, const uint32_t* d_pos, uint64_t* d_tk, uint32_t* d_tcol,
                   hipStream_t s);

// used[tcol[r]] = 1 for every row (used: n_sets zeroed words)
int bft_sg_mark(const uint32_t* d_tcol, uint64_t nk, uint32_t* d_used, hipStream_t s);
// Ids of the used lists in the new dictionary (the input of the scan that places them): the list's length, 0 for an unused set
struct BftSgUsedLen {
    const uint32_t* used;
    const uint32_t* cs_off;
    uint64_t n_sets;
    __host__ __device__ uint32_t operator()(uint64_t j) const { return j < n_sets && used[j] ? cs_off[j + 1] - cs_off[j] : 0u; }
};
// tcol[r] = new_id[tcol[r]]
int bft_sg_remap(uint32_t* d_tcol, uint64_t nk, const uint32_t* d_new_id, hipStream_t s);
// The used sets in their old order: offsets (new_off[new_id[j]] = id_pos[j], new_off[n_sets'] = id_pos[n_sets]) and their lists, one
// wavefront per set, the ids widened from cs_w bytes to 32 bits
int bft_sg_dict(const uint32_t* d_used, const uint32_t* d_new_id, const uint32_t* d_id_pos, const uint32_t* d_cs_off, const void* d_cs_ids, uint32_t cs_w, uint64_t n_sets,
                uint32_t* d_new_off, uint32_t* d_new_ids, hipStream_t s);
