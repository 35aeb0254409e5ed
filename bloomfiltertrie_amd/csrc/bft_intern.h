// bft_intern.h -- interning of the colour sets: the genome-id list of every k-mer becomes an id into a dictionary of the distinct lists
// (bft_intern.hip).
#pragma once
#include "bft_dev.h"

void bft_test_weak_signature(int how);            // test hook: 1 every list's signature = its length (collisions galore); 2 the exact pass's second key as well
unsigned long long bft_test_exact_passes(void);   // how many times the interning had to fall back to comparing the lists
// The interning's tail -- the dictionary entries copied out of their representatives' lists, then EVERY k-mer's list compared with the entry it was
// given -- is a third of its time (1.2 of 3.4 ms on config 3) and nothing of the build needs its result before the commit: with `side` set it is
// enqueued on that stream (behind the interning's kernels) and bft_intern_colors_gpu returns at once; the caller keeps d_seg_off / d_pg alive, makes
// whatever reads the dictionary wait for `done`, and calls wait() before it commits -- *collisions != 0: two different lists shared a signature and
// the interning must be run again with exact = true (lists compared; on the caller's stream, nothing deferred).
struct BftInternTail {
    hipStream_t side = nullptr;
    hipEvent_t done = nullptr, ready = nullptr;
    bool pending = false;
    DevBuf rep, bad;  // (what the deferred kernels read and write besides the outputs)
    PinBlock pin;
    uint32_t narrow_w = 4;  // in: bytes per genome id of the resident dictionary (1 / 2: the deferred tail also writes `narrow`, the dictionary's ids in that width)
    DevBuf narrow;
    ~BftInternTail() {
        if (pending && side) (void)hipStreamSynchronize(side);
        if (done) (void)hipEventDestroy(done);
        if (ready) (void)hipEventDestroy(ready);
    }
    int wait(uint32_t* collisions) {
        *collisions = 0;
        if (!pending) return 0;
        HIPCK(hipEventSynchronize(done));
        pending = false;
        *collisions = (uint32_t)pin.p[0];
        return 0;
    }
};
int bft_intern_colors_gpu(const uint32_t* d_seg_off, const uint32_t* d_pg, uint64_t nk, uint64_t np, hipStream_t s, DevBuf& d_tcol,
                          DevBuf& d_cs_off, DevBuf& d_cs_ids, uint64_t& n_sets, uint64_t& n_ids, uint64_t distinct_hint = 0, BftInternTail* tail = nullptr,
                          bool exact = false);
