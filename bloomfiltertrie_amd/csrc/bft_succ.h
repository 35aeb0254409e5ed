// bft_succ.h -- the successor search over the sorted T-form table tk shared by the whole-graph kernels (simple paths, bft_paths.hip; bidirected
// unitigs, bft_unitigs.hip; connected components, bft_components.hip; reachability marks, bft_marking.hip): the bucket of a T-form's top bits
// (sp_top); every stored successor x[1..k-1]+N with ONE lower bound, of a word (bft_for_each_successor_of) and of a row (bft_for_each_successor,
// which loads the row and calls the word form); the bucketed exact lookup of a word (bft_find_row); a word's reverse complement (bft_x_revcomp); and the
// colour-set tests of the nodes and edges (sp_set_size, sp_shared).
// Device code only, header only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bft_dev.h"
#include "bft_kernels_seqwin.h"  // rev2_64
#include "bft_walk.h"

// the top sb bits of a T-form (2k bits in W words, word 0 most significant)
template <int W>
__device__ __forceinline__ uint32_t sp_top(const uint64_t* t, int k, int sb) {
    const int tb = 2 * k - 64 * (W - 1);  // bits in word 0
    if (tb >= sb) return (uint32_t)(t[0] >> (tb - sb));
    uint64_t w1 = 0;
#pragma unroll
    for (int w = 1; w < W; w++)
        if (w == 1) w1 = t[1];
    return (uint32_t)((t[0] << (sb - tb)) | (w1 >> (64 - (sb - tb))));
}

// f(r, c) for every stored row r whose k-mer is x[1..k-1]+N, in ascending row; c is N's code.  The four words differ in the last nucleotide only,
// which sits in the two lowest bits of the T-form (k % 9 != 0) or in bits 2-3 of the last block (k % 9 == 0, the block is rotated): they lie in one
// interval of at most 16 rows, found by ONE lower bound inside the bucket (start[], 2^sb + 1 entries) of the word with nucleotide 0 last.
// x: a k-mer as bft_x_from_tform gives it (nucleotide j at bits 2j, the bits above 2k zero) -- a stored row's, or any other word's (the reverse
// complements of bft_unitigs.hip).
template <int W, class F>
__device__ __forceinline__ void bft_for_each_successor_of(const uint64_t* __restrict__ tk, uint32_t n, int k, int sb, const uint32_t* __restrict__ start,
                                                          const uint64_t* x, F&& f) {
    const int vo = (k % 9) ? 0 : 2;  // where the last nucleotide sits in the T-form's last word
    const uint64_t wild = 3ull << vo;
    uint64_t t[W], y[W];
    // the successor with nucleotide 0 last: drop the first nucleotide (the bits above 2k are zero, so the new last one is A)
#pragma unroll
    for (int w = 0; w < W; w++) y[w] = (x[w] >> 2) | (w + 1 < W ? x[w + 1] << 62 : 0ull);
    bft_tform_from_x<W>(y, k, t);
    const uint32_t b = sp_top<W>(t, k, sb), lo = start[b], hi = start[b + 1];
    uint32_t r = lo + bft_rows_lower_bound<W>(tk + (uint64_t)lo * W, hi - lo, t);
    for (; r < n; r++) {
        uint64_t c[W];
        bft_load_row<W>(tk + (uint64_t)r * W, c);
        bool same = true;
#pragma unroll
        for (int w = 0; w < W - 1; w++) same = same && c[w] == t[w];
        if (!same || c[W - 1] > (t[W - 1] | wild)) break;  // (rows at or after t: past the interval)
        if ((c[W - 1] & ~wild) != t[W - 1]) continue;
        f(r, (uint32_t)((c[W - 1] >> vo) & 3ull));
    }
}
// f(r) for every stored successor r of row u, in ascending row
template <int W, class F>
__device__ __forceinline__ void bft_for_each_successor(const uint64_t* __restrict__ tk, uint32_t n, int k, int sb, const uint32_t* __restrict__ start,
                                                       uint64_t u, F&& f) {
    uint64_t t[W], x[W];
    bft_load_row<W>(tk + u * W, t);
    bft_x_from_tform<W>(t, k, x);
    bft_for_each_successor_of<W>(tk, n, k, sb, start, x, [&](uint32_t r, uint32_t) { f(r); });
}

// the row that holds the k-mer x, or 0xFFFFFFFF: a lower bound inside the bucket of its T-form
template <int W>
__device__ __forceinline__ uint32_t bft_find_row(const uint64_t* __restrict__ tk, int k, int sb, const uint32_t* __restrict__ start, const uint64_t* x) {
    uint64_t t[W], c[W];
    bft_tform_from_x<W>(x, k, t);
    const uint32_t b = sp_top<W>(t, k, sb), lo = start[b], hi = start[b + 1];
    const uint32_t r = lo + bft_rows_lower_bound<W>(tk + (uint64_t)lo * W, hi - lo, t);
    if (r >= hi) return 0xFFFFFFFFu;
    bft_load_row<W>(tk + (uint64_t)r * W, c);
    return bft_cmp<W>(c, t) == 0 ? r : 0xFFFFFFFFu;
}

// reverse complement of the k nucleotides of x (nucleotide j at bits 2j; the bits above 2k are zero on both sides)
template <int W>
__device__ __forceinline__ void bft_x_revcomp(const uint64_t* x, int k, uint64_t* xr) {
    uint64_t rv[W + 1];
#pragma unroll
    for (int q = 0; q < W; q++) rv[q] = rev2_64(~x[W - 1 - q]);
    rv[W] = 0;
    const uint32_t dn = (uint32_t)(64 * W - 2 * k);  // < 64
#pragma unroll
    for (int q = 0; q < W; q++) xr[q] = dn ? (rv[q] >> dn) | (rv[q + 1] << (64u - dn)) : rv[q];
    const int top = 2 * k - 64 * (W - 1);
    if (top < 64) xr[W - 1] &= (1ull << top) - 1ull;
}

// the number of genomes of colour set cs
__device__ __forceinline__ uint32_t sp_set_size(const uint32_t* cs_off, uint32_t cs) { return cs_off[cs + 1] - cs_off[cs]; }

// |C(a) & C(b)| >= t for two sorted id lists
__device__ inline bool sp_shared(uint32_t ca, uint32_t cb, uint32_t t, const uint32_t* cs_off, const void* cs_ids, uint32_t cs_w) {
    if (t == 0u || ca == cb) return true;  // (a node's own set has t ids or more)
    uint32_t i = cs_off[ca], ie = cs_off[ca + 1], j = cs_off[cb], je = cs_off[cb + 1], got = 0;
    while (i < ie && j < je) {
        if (got + min(ie - i, je - j) < t) return false;
        const uint32_t a = bft_cs_id_at(cs_ids, cs_w, i), b = bft_cs_id_at(cs_ids, cs_w, j);
        if (a == b) {
            if (++got >= t) return true;
            i++;
            j++;
        } else if (a < b) i++;
        else j++;
    }
    return got >= t;
}
