// bft_genome_matrix.h -- the genome-by-genome shared k-mer matrix (bft_genome_matrix.hip): M = B^T diag(w) B over the colour-set dictionary, by
// two roads that agree bit for bit (sparse: pair updates per set; dense: 7-bit digits of w on the i8 matrix cores).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define BFT_GM_MAX_GENOMES 16384u  // BFT_GPU_GENOME_MATRIX_MAX_GENOMES (include/bft_gpu.h): 2 GiB of matrix
#define BFT_GM_LDS_GENOMES 127u    // the sparse road keeps the upper triangle (G (G + 1) / 2 64-bit counters, 8128 at most: 63.5 KB) in LDS up to here
#define BFT_GM_DIGITS 5            // 7-bit digits of a 32-bit weight (each fits a signed i8)
#define BFT_GM_STEP 64u            // colour sets per step of the dense road (the K of one mfma_i32_16x16x64_i8)
#define BFT_GM_TILE 16u            // genomes per tile edge of the dense road
#define BFT_GM_FLUSH_SETS (1u << 24)  // sets between two flushes of the i32 accumulators: 127 * 2^24 < 2^31
// The cost model: one pair update of the sparse road is priced as this many multiply-adds of the dense one (digit steps x 64 sets x Gpad^2 / 2,
// the bit-matrix pass included in their time).  Measured with tools/bench_genome_matrix.py (profiles/genome_matrix/bench_genome_matrix.jsonl,
// DESIGN 18): with the LDS triangle (config 3, 100 genomes) the roads take equal time at 23 multiply-adds per pair update, with 64-bit atomics to
// memory (config 5, 2000 genomes) at 4313.  Before the measurement the one constant was 4096, from reasoning.
#define BFT_GM_PAIR_COST_LDS 24ull
#define BFT_GM_PAIR_COST 4096ull
#define BFT_GM_DENSE_MAX_BYTES (1ull << 30)  // a bit matrix beyond this is never built by the cost model (the sparse road then)

enum { BFT_GM_AUTO = 0, BFT_GM_SPARSE = 1, BFT_GM_DENSE = 2 };

// Arrays of one call, room for `sets` colour sets (carved out of the handle's gm_buf by the caller).  sets_pad = sets rounded up to BFT_GM_STEP.
struct BftGmScratch {
    uint32_t* usage;              // [sets] rows (batch entries) that carry the colour set
    uint32_t* w;                  // [sets_pad] the weights
    uint8_t* digit;               // [BFT_GM_DIGITS][sets_pad] digit d of every weight
    uint8_t* stepmask;            // [sets_pad / 64] bit d: some set of the step has a non-zero digit d
    unsigned long long* plan;     // [4] pair updates of the sparse road, digit steps of the dense one, the road taken (1 / 2), unused
    uint16_t* bits;               // [Gpad][sets_pad / 16] the transposed membership matrix, genome-major, sets along the bits (gm_bits)
};

// usage[c] += occurrences of c among the n ids; ids at or past n_sets (0xFFFFFFFF = absent included) are skipped (usage zeroed by the caller)
int bft_gm_usage_ids(const uint32_t* d_ids, uint64_t n, uint32_t n_sets, uint32_t* d_usage, hipStream_t s);
// w[c] = src[c] where lo <= |c| <= hi, else 0; the digits, the step masks and the two costs of the plan (plan zeroed here)
int bft_gm_weights(uint32_t n_sets, const uint32_t* d_cs_off, const uint32_t* d_src, uint32_t lo, uint32_t hi, const BftGmScratch& p, hipStream_t s);
// the road: forced (1 / 2) or by the cost model from the plan's two costs; dense_ok = false: the bit matrix was not allocated
int bft_gm_plan(int forced, bool dense_ok, uint32_t G, const BftGmScratch& p, hipStream_t s);
// every launch below tests the plan's road first and leaves when it is the other one's
int bft_gm_sparse(uint32_t n_sets, const uint32_t* d_cs_off, const void* d_cs_ids, uint32_t cs_w, uint32_t G, const BftGmScratch& p,
                  unsigned long long* d_shared, hipStream_t s);
int bft_gm_bits(uint32_t n_sets, uint64_t n_ids, const uint32_t* d_cs_off, const void* d_cs_ids, uint32_t cs_w, uint32_t G, const BftGmScratch& p, hipStream_t s);
int bft_gm_dense(uint32_t n_sets, uint32_t G, uint32_t flush_sets, const BftGmScratch& p, unsigned long long* d_shared, hipStream_t s);
