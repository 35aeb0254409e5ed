// bft_merge.h -- merging a sorted run of newly inserted k-mers into the built index (bft_merge.hip).  A "run" = sorted distinct T-form k-mers, a
// colour-set id per k-mer and the dictionary those ids refer to -- what the index itself is made of.
#pragma once
#include "bft_dev.h"

struct BftRun {
    const uint64_t* tk;
    const uint32_t* tcol;
    uint64_t n;
    const uint32_t* cs_off;
    const uint32_t* cs_ids;
    uint64_t n_sets;
};
struct BftRunOut {  // ... built aside: the output of a merge, and the image-to-be that bft_commit_image takes (bft_handle.h)
    DevBuf tk, tcol, cs_off, cs_ids;
    uint64_t n = 0, n_sets = 0, n_ids = 0;
    void swap(BftRunOut& o) {
        tk.swap(o.tk); tcol.swap(o.tcol); cs_off.swap(o.cs_off); cs_ids.swap(o.cs_ids);
        std::swap(n, o.n); std::swap(n_sets, o.n_sets); std::swap(n_ids, o.n_ids);
    }
};
// How the k-mers are placed.  An insertion build searches every run row in the index (the default: a run is small beside its index); a merge of two
// indexes (bft_union.hip) may stream both tables instead (coranked), has its launches timed on a handle and records its stages ("build_stages").
struct BftMergeOpt {
    bool coranked = false;
    bool stages = false;
    bft_gpu* timed = nullptr;
};
int bft_merge_runs(int W, const BftRun& a, const BftRun& b, hipStream_t s, BftRunOut& out, const BftMergeOpt& opt = BftMergeOpt());
int bft_count_pairs(const uint32_t* d_tcol, uint64_t n, const uint32_t* d_cs_off, hipStream_t s, uint64_t* total);
