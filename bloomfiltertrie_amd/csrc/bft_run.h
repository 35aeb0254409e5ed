// bft_run.h -- steps 1-3 of the bulk build (bft_run.hip): the insertion log becomes a run -- sorted distinct T-form k-mers, the offsets of their
// genome-id lists, the ids (BftPairRun, bft_dev.h) --, and what the log looks like to the library's sort and scan on the way: the input functors
// of bft_rs::sort / bft_scan::exclusive_sum that read it.  (Here and not beside the kernels of bft_kernels_build.h: the sort and scan test hooks
// of bft_gpu.hip run the same instantiations.)
#pragma once
#include "bft_dev.h"
#include "bft_sort.h"

int bft_make_run(bft_gpu* h, BftPairRun& run);  // from h's insertion log, on h->stream; sets h->front_redone and h->msd_max_bucket

// ---- composite path: one-word keys whose genome ids arrive in ascending order and fit the key's spare low bits ----------------
// c = (T << gb) | genome: ONE 8-byte array is sorted (on the T bits only: the sort is stable, so the ids keep their ascending
// order inside a k-mer) instead of 8-byte keys + 4-byte values -- a third less traffic in each of the seven radix passes -- and the
// de-duplication flags come out of neighbouring composites on the fly instead of through two flag arrays and two scans.
struct BftCompose {  // input "iterator" of the sort: composite i from the insertion log
    const uint64_t* k;
    const uint32_t* g;
    uint32_t gb;
    __host__ __device__ uint64_t operator()(uint32_t i) const { return g ? (k[i] << gb) | (uint64_t)g[i] : k[i]; }  // (g == NULL: the log already holds composites)
    __device__ uint64_t key(uint32_t i) const { return (*this)(i); }  // (as the input of bft_rs::sort)
    __device__ bft_rs::NoVal val(uint32_t) const { return bft_rs::NoVal{}; }
};
// two-word keys: what the root-prefix split moves -- the top 64 bits of the T-form (left-aligned: their top 18 bits are the root prefix) as the
// key, the bits below them and the genome id as the value (bft_front.hip: BftItem2)
struct __attribute__((packed, aligned(4))) BftSplit2Val {
    uint64_t lo;
    uint32_t id;
};
struct BftSplit2In {
    const uint64_t* k0;  // word 0 (most significant), word 1 of the log
    const uint64_t* k1;
    const uint32_t* g;
    uint32_t sh;  // 2k - 64: the bits of word 1 that belong to the T-form's low part once the top 64 are taken (2 .. 64)
    __device__ uint64_t key(uint32_t i) const { return sh == 64 ? k0[i] : (k0[i] << (64 - sh)) | (k1[i] >> sh); }
    __device__ BftSplit2Val val(uint32_t i) const {
        BftSplit2Val v;
        v.lo = sh == 64 ? k1[i] : (k1[i] & ((1ull << sh) - 1ull));
        v.id = g[i];
        return v;
    }
};
template <class GT>
struct BftPairIn {  // input of the sorts that move (k-mer, id) pairs: the log's k-mers, its ids narrowed to GT
    const uint64_t* k;
    const uint32_t* g;
    __device__ uint64_t key(uint32_t i) const { return k[i]; }
    __device__ GT val(uint32_t i) const { return (GT)g[i]; }
};
struct BftPairFlags {  // input of the scan: (first pair of its k-mer) << 32 | (first pair of its (k-mer, genome))
    const uint64_t* c;
    uint32_t gb;
    __host__ __device__ uint64_t operator()(uint32_t i) const {
        const uint64_t a = c[i], b = i ? c[i - 1] : ~a;
        const uint64_t head = (a >> gb) != (b >> gb), keep = a != b;
        return (head << 32) | keep;
    }
};
