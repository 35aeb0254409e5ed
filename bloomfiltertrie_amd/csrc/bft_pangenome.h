// bft_pangenome.h -- pan-genome k-mer classes of the index (bft_pangenome.hip): the launchers bft_gpu_kmers_by_count / bft_gpu_pangenome_stats chain
// with the library's scan.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define BFT_PG_NONE 0xFFFFFFFFu  // no colour set (a wavefront without a hot set; a row past the table)
#define BFT_PG_LDS_GENOMES 4095u // k_pg_dict keeps its 3 G + 1 counters in LDS up to this many genomes (48 KB of 32-bit counters); global atomics beyond

// Arrays of one call, room for m rows and `sets` colour sets (carved out of the handle's block by the caller).
struct BftPgScratch {
    uint32_t* slot;   // [m + 1] exclusive scan of the selection: the output slot of a selected row; slot[n] = the number of selected rows
    uint32_t* usage;  // [sets] rows that carry the colour set
};

// a row is selected when its colour set holds lo .. hi genomes (input of the scan that places the selected rows)
struct BftPgSel {
    const uint32_t* tcol;
    const uint32_t* cs_off;
    uint32_t lo, hi;
    __host__ __device__ uint32_t operator()(uint64_t i) const {
        const uint32_t c = tcol[i];
        const uint32_t cnt = cs_off[c + 1] - cs_off[c];
        return cnt >= lo && cnt <= hi ? 1u : 0u;
    }
};

// the selected rows (slot[] from the scan, slot[n] included) below cap, in row order: packed k-mers (B bytes each), ASCII k-mers (k + 1 bytes each, NUL
// included) and rows; any output may be NULL
int bft_pg_emit(int W, const uint64_t* d_tk, uint64_t n, int k, int B, const BftPgScratch& p, uint8_t* d_kmers, char* d_ascii, uint32_t* d_rows, uint64_t cap,
                hipStream_t s);
// usage[cs] += rows of the n-row table that carry cs (usage zeroed by the caller)
int bft_pg_usage(uint64_t n, const uint32_t* d_tcol, const BftPgScratch& p, hipStream_t s);
// one pass over the dictionary: spectrum[|cs|] += usage[cs]; genome_total[g] += usage[cs] for every g of cs; genome_private[g] += usage[cs] when cs = {g}.
// G = number of genomes; the outputs (64-bit, zeroed by the caller) may be NULL
int bft_pg_dict(uint64_t n_sets, uint64_t n_ids, const uint32_t* d_cs_off, const void* d_cs_ids, uint32_t cs_w, uint32_t G, const BftPgScratch& p,
                unsigned long long* d_spectrum, unsigned long long* d_total, unsigned long long* d_private, hipStream_t s);
