// bft_front.h -- the build's front end behind the root-prefix split (bft_front.hip): bucket-wise sort of the composites c = T << gb | genome on the
// bits [gb, split_bit) and the de-duplicated outputs: sorted distinct k-mers, offsets of their genome-id lists, the genome ids.
#pragma once
#include "bft_dev.h"

// what steps 1-3 of a build make of the insertion log (bft_run.hip): sorted distinct T-form k-mers, the offsets of their genome-id lists, the ids
struct BftPairRun { DevBuf tk, seg_off, ids; uint64_t nk = 0, np = 0; };
uint32_t bft_front_bucket_capacity(void);
void bft_test_front_rank_mode(int mode);   // test hook: k_bucket_sort's mode (0 atomics + check, 1 ballots only, 2 the check always fails)
void bft_test_front_wave_cap(uint32_t cap);  // test hook: the largest bucket of the wavefront kernel (0 by rule -- bft_front_plan.h --, 512, 1024)
// d_vals (vw bytes per id): d_c holds whole T-form k-mers grouped by the bits from split_bit - gb up, the ids beside them
int bft_front_buckets(uint64_t* d_c, uint64_t n, const uint32_t* d_boff, uint32_t nb, uint32_t gb, uint32_t split_bit, hipStream_t s, BftPairRun& run,
                      const uint32_t* d_max_bucket, uint32_t* max_bucket, bool* done, uint32_t* n_redone, const void* d_vals = nullptr, uint32_t vw = 0);
// (d_max_bucket: the size of the largest bucket, on the device -- it reaches the host, *max_bucket, while the first sort kernel runs;
// *done = false: that bucket is beyond bft_front_bucket_capacity() and nothing was produced (d_c may have been reordered inside its
// buckets); *n_redone: buckets whose order check failed and that were sorted again)
// two-word keys (33 <= k <= 64): d_hk = the top 64 bits of the T-form, left-aligned, grouped by their top 18 bits (d_boff); d_items = {lo: the 2k - 64
// bits below, id: the genome} (12 bytes each) beside them.  *done = false: a bucket is beyond bft_front2_bucket_capacity(): nothing was produced
// (the arrays may have been reordered inside their buckets); *n_redone as bft_front_buckets'.
uint32_t bft_front2_bucket_capacity(void);
int bft_front2_buckets(uint64_t* d_hk, void* d_items, uint64_t n, const uint32_t* d_boff, uint32_t nb, int k, hipStream_t s, BftPairRun& run,
                       const uint32_t* d_max_bucket, uint32_t* max_bucket, bool* done, uint32_t* n_redone, uint32_t max_gid);
