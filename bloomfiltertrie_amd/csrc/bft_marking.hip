// bft_marking.hip -- vertex marks of the index (set_marking / unset_marking / set_flag_kmer / get_flag_kmer, reference bft.h, src/bft.c:686-765) and
// reachability restricted by mark (what BFS / DFS / BFS_subgraph / DFS_subgraph leave behind, src/snippets.c:605-812): a four-state flag per stored
// k-mer, two bits per row of the sorted T-form table (rows in the bft_gpu_extract order), 16 rows per 32-bit word (bft_marking.h), resident in HBM.
// The batch calls take packed k-mers; their rows come from the lookup bft_gpu_query_rows uses (bft_launch_query), then
//   k_mk_set      one lane per k-mer: one flag for the batch (an atomic and of the bits to clear, then an atomic or of the bits to set: every writer
//                 writes the same value, so any interleaving ends there) or a flag per k-mer (a CAS loop on the word: two writers of one row end as
//                 one of their two values, writers of other rows of the word all land)
//   k_mk_get      one lane per k-mer: its flag, 0xFF for an absent k-mer
//   k_mk_tas      test-and-set: the row moves from `expect` to `flag` by a CAS on its word; the lane whose CAS made the move is the one winner
//   k_mk_fill     every word = the flag sixteen times (rows past the table stay 0)
//   k_mk_counts   rows per state: a lane counts whole words with popcounts, a workgroup reduces through LDS and adds once per state
//   (select: BftMkSel -- flag in a 4-bit mask -- is the input of the library's scan; the emission is the pan-genome one, bft_pg_emit)
// reach (bft_gpu_marks_reach): eligible rows hold the flag `through` and every requested genome id; the forest of their components is the lock-free
// union-find of bft_components.hip (bft_cc_sets / bft_cc_init with the flag test / bft_cc_hook / bft_cc_flatten), kept on the handle, then
//   k_mk_unhit    best[u] = none for every row (with a new forest)
//   k_mk_seed     one lane per seed: an eligible seed writes its index into best[root] with an atomic min
//   k_mk_paint    one lane per flag WORD: the rows whose root was hit get `to` (one plain store per word: the kernel's only writer of it); then one
//                 lane per seed: seed_new = the seed is the one its root kept
//   k_mk_boundary (boundary != 0) one pass over successor edges, seen from both ends: a row outside the forest that still holds `through` and
//                 touches a painted member gets `to` (test-and-set: counted once); so does such a row that is a seed
//   k_mk_unseed   best[root of a seed] = none again: the forest is ready for the next reach
// The number of launches depends on the arguments alone, never on the data.  No kernel needs scratch memory; k_mk_counts and the counters' reduction
// use 64 bytes of LDS.

#include "bft_components.h"
#include "bft_dev.h"
#include "bft_handle.h"
#include "bft_marking.h"
#include "bft_pangenome.h"
#include "bft_scan.h"
#include "bft_succ.h"

namespace {

__device__ __forceinline__ uint32_t mk_load(uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// v summed over the workgroup and added to *dst by ONE lane (every thread of the workgroup calls this, outside any divergent loop)
__device__ __forceinline__ void mk_block_add(uint32_t v, unsigned long long* dst, uint32_t* lds) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d);
    if ((threadIdx.x & 63u) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
#pragma unroll
        for (int w = 0; w < BFT_LAUNCH_THREADS / 64; w++) t += lds[w];
        if (t && dst) atomicAdd(dst, (unsigned long long)t);
    }
    __syncthreads();
}

// row r: expect -> flag; true for the one caller whose CAS made the move
__device__ __forceinline__ bool mk_move(uint32_t* words, uint32_t r, uint32_t expect, uint32_t flag) {
    uint32_t* w = words + (r >> 4);
    const uint32_t sh = 2u * (r & 15u), m = 3u << sh, v = flag << sh;
    uint32_t old = mk_load(w);
    while (((old >> sh) & 3u) == expect) {
        const uint32_t prev = atomicCAS(w, old, (old & ~m) | v);
        if (prev == old) return true;
        old = prev;
    }
    return false;
}

__global__ __launch_bounds__(BFT_LAUNCH_THREADS) void k_mk_set(const uint32_t* __restrict__ rows, uint64_t n, uint32_t n_rows, const uint8_t* __restrict__ fl, uint32_t flag,
                                                       uint32_t* words, unsigned long long* absent) {
    __shared__ uint32_t lds[BFT_LAUNCH_THREADS / 64];
    uint32_t miss = 0;
    for (uint64_t i = blockIdx.x * (uint64_t)BFT_LAUNCH_THREADS + threadIdx.x; i < n; i += (uint64_t)gridDim.x * BFT_LAUNCH_THREADS) {
        const uint32_t r = rows[i];
        if (r >= n_rows) {
            miss++;
            continue;
        }
        uint32_t* w = words + (r >> 4);
        const uint32_t sh = 2u * (r & 15u), m = 3u << sh;
        if (fl) {
            const uint32_t v = ((uint32_t)fl[i] & 3u) << sh;
            uint32_t old = mk_load(w);
            for (;;) {
                const uint32_t nw = (old & ~m) | v;
                if (nw == old) break;
                const uint32_t prev = atomicCAS(w, old, nw);
                if (prev == old) break;
                old = prev;
            }
        } else {
            const uint32_t v = flag << sh;
            if (m & ~v) atomicAnd(w, ~(m & ~v));
            if (v) atomicOr(w, v);
        }
    }
    mk_block_add(miss, absent, lds);
}

__global__ __launch_bounds__(BFT_LAUNCH_THREADS) void k_mk_get(const uint32_t* __restrict__ rows, uint64_t n, uint32_t n_rows, const uint32_t* __restrict__ words,
                                                       uint8_t* __restrict__ out, unsigned long long* absent) {
    __shared__ uint32_t lds[BFT_LAUNCH_THREADS / 64];
    uint32_t miss = 0;
    for (uint64_t i = blockIdx.x * (uint64_t)BFT_LAUNCH_THREADS + threadIdx.x; i < n; i += (uint64_t)gridDim.x * BFT_LAUNCH_THREADS) {
        const uint32_t r = rows[i];
        if (r >= n_rows) {
            miss++;
            out[i] = 0xFFu;
        } else
            out[i] = (uint8_t)bft_mk_field(words[r >> 4], r);
    }
    mk_block_add(miss, absent, lds);
}

__global__ __launch_bounds__(BFT_LAUNCH_THREADS) void k_mk_tas(const uint32_t* __restrict__ rows, uint64_t n, uint32_t n_rows, uint32_t expect, uint32_t flag, uint32_t* words,
                                                       uint8_t* __restrict__ won, unsigned long long* absent) {
    __shared__ uint32_t lds[BFT_LAUNCH_THREADS / 64];
    uint32_t miss = 0;
    for (uint64_t i = blockIdx.x * (uint64_t)BFT_LAUNCH_THREADS + threadIdx.x; i < n; i += (uint64_t)gridDim.x * BFT_LAUNCH_THREADS) {
        const uint32_t r = rows[i];
        bool w = false;
        if (r >= n_rows) miss++;
        else w = mk_move(words, r, expect, flag);
        won[i] = w ? 1u : 0u;
    }
    mk_block_add(miss, absent, lds);
}

__global__ __launch_bounds__(BFT_LAUNCH_THREADS) void k_mk_fill(uint32_t* __restrict__ words, uint64_t n_words, uint32_t n_rows, uint32_t flag) {
    const uint32_t full = flag * 0x55555555u;
    for (uint64_t i = blockIdx.x * (uint64_t)BFT_LAUNCH_THREADS + threadIdx.x; i < n_words; i += (uint64_t)gridDim.x * BFT_LAUNCH_THREADS) {
        const uint32_t live = n_rows - (uint32_t)i * 16u;  // rows of this word that exist (>= 1)
        words[i] = live >= 16u ? full : full & ((1u << (2u * live)) - 1u);
    }
}

__global__ __launch_bounds__(BFT_LAUNCH_THREADS) void k_mk_counts(const uint32_t* __restrict__ words, uint64_t n_words, uint32_t n_rows, unsigned long long* counts) {
    __shared__ uint32_t lds[BFT_LAUNCH_THREADS / 64];
    uint32_t c0 = 0, c1 = 0, c2 = 0, c3 = 0;
    for (uint64_t i = blockIdx.x * (uint64_t)BFT_LAUNCH_THREADS + threadIdx.x; i < n_words; i += (uint64_t)gridDim.x * BFT_LAUNCH_THREADS) {
        const uint32_t w = words[i], lo = w & 0x55555555u, hi = (w >> 1) & 0x55555555u;
        const uint32_t live = n_rows - (uint32_t)i * 16u;
        const uint32_t a = (uint32_t)__popc(lo & ~hi), b = (uint32_t)__popc(hi & ~lo), c = (uint32_t)__popc(lo & hi);
        c1 += a;
        c2 += b;
        c3 += c;
        c0 += (live >= 16u ? 16u : live) - a - b - c;  // (the bits of rows past the table are 0: they are in none of a, b, c)
    }
    mk_block_add(c0, counts + 0, lds);
    mk_block_add(c1, counts + 1, lds);
    mk_block_add(c2, counts + 2, lds);
    mk_block_add(c3, counts + 3, lds);
}

__global__ __launch_bounds__(BFT_LAUNCH_THREADS) void k_mk_unhit(uint32_t n, uint32_t* __restrict__ best) {
    for (uint64_t u = blockIdx.x * (uint64_t)BFT_LAUNCH_THREADS + threadIdx.x; u < n; u += (uint64_t)gridDim.x * BFT_LAUNCH_THREADS) best[u] = BFT_MK_NONE;
}

// (parent[] is flattened: parent[r] is r's root.  A row of the forest whose flag is no longer `through` was painted by an earlier reach: not eligible)
__global__ __launch_bounds__(BFT_LAUNCH_THREADS) void k_mk_seed(const uint32_t* __restrict__ rows, uint64_t n_seeds, uint32_t n_rows, const uint32_t* __restrict__ parent,
                                                        const uint32_t* __restrict__ words, uint32_t through, uint32_t* best, unsigned long long* absent) {
    __shared__ uint32_t lds[BFT_LAUNCH_THREADS / 64];
    uint32_t miss = 0;
    for (uint64_t i = blockIdx.x * (uint64_t)BFT_LAUNCH_THREADS + threadIdx.x; i < n_seeds; i += (uint64_t)gridDim.x * BFT_LAUNCH_THREADS) {
        const uint32_t r = rows[i];
        if (r >= n_rows) {
            miss++;
            continue;
        }
        const uint32_t p = parent[r];
        if (p != BFT_CC_NONE && bft_mk_field(words[r >> 4], r) == through) atomicMin(&best[p], (uint32_t)i);
    }
    mk_block_add(miss, absent, lds);
}

__global__ __launch_bounds__(BFT_LAUNCH_THREADS) void k_mk_paint(uint32_t n_rows, uint64_t n_words, const uint32_t* __restrict__ parent, const uint32_t* __restrict__ best,
                                                         uint32_t* __restrict__ words, uint32_t through, uint32_t to, const uint32_t* __restrict__ rows,
                                                         uint64_t n_seeds, uint8_t* __restrict__ seed_new, unsigned long long* painted) {
    __shared__ uint32_t lds[BFT_LAUNCH_THREADS / 64];
    uint32_t cnt = 0;
    for (uint64_t i = blockIdx.x * (uint64_t)BFT_LAUNCH_THREADS + threadIdx.x; i < n_words; i += (uint64_t)gridDim.x * BFT_LAUNCH_THREADS) {
        const uint32_t w = words[i];
        uint32_t nw = w;
#pragma unroll
        for (uint32_t j = 0; j < 16u; j++) {
            const uint64_t u = i * 16u + j;
            if (u >= n_rows || ((w >> (2u * j)) & 3u) != through) continue;
            const uint32_t p = parent[u];
            if (p == BFT_CC_NONE || best[p] == BFT_MK_NONE) continue;
            nw = (nw & ~(3u << (2u * j))) | (to << (2u * j));
            cnt++;
        }
        if (nw != w) words[i] = nw;
    }
    if (seed_new)
        for (uint64_t i = blockIdx.x * (uint64_t)BFT_LAUNCH_THREADS + threadIdx.x; i < n_seeds; i += (uint64_t)gridDim.x * BFT_LAUNCH_THREADS) {
            const uint32_t r = rows[i];
            const uint32_t p = r < n_rows ? parent[r] : BFT_CC_NONE;
            seed_new[i] = (p != BFT_CC_NONE && best[p] == (uint32_t)i) ? 1u : 0u;
        }
    mk_block_add(cnt, painted, lds);
}

// (after k_mk_paint: parent[] and best[] are only read here, and tell the painted members whatever their flag says now; the flags of the rows
// outside the forest move through -> to by CAS alone)
template <int W>
__global__ __launch_bounds__(BFT_LAUNCH_THREADS) void k_mk_boundary(const uint64_t* __restrict__ tk, uint32_t n, int k, int sb, const uint32_t* __restrict__ start,
                                                            const uint32_t* __restrict__ parent, const uint32_t* __restrict__ best, uint32_t* words,
                                                            uint32_t through, uint32_t to, const uint32_t* __restrict__ rows, uint64_t n_seeds,
                                                            unsigned long long* painted) {
    __shared__ uint32_t lds[BFT_LAUNCH_THREADS / 64];
    uint32_t cnt = 0;
    for (uint64_t u = blockIdx.x * (uint64_t)BFT_LAUNCH_THREADS + threadIdx.x; u < n; u += (uint64_t)gridDim.x * BFT_LAUNCH_THREADS) {
        const uint32_t pu = parent[u];
        const bool hit_u = pu != BFT_CC_NONE && best[pu] != BFT_MK_NONE;
        // an outside row that does not hold `through` now never will again in this kernel; a member that was not hit has no painted neighbour
        const bool out_u = pu == BFT_CC_NONE && bft_mk_field(mk_load(words + (u >> 4)), (uint32_t)u) == through;
        if (!hit_u && !out_u) continue;
        bft_for_each_successor<W>(tk, n, k, sb, start, u, [&](uint32_t v) {
            const uint32_t pv = parent[v];
            if (hit_u) {
                if (pv == BFT_CC_NONE && mk_move(words, v, through, to)) cnt++;
            } else if (pv != BFT_CC_NONE && best[pv] != BFT_MK_NONE && mk_move(words, (uint32_t)u, through, to))
                cnt++;
        });
    }
    for (uint64_t i = blockIdx.x * (uint64_t)BFT_LAUNCH_THREADS + threadIdx.x; i < n_seeds; i += (uint64_t)gridDim.x * BFT_LAUNCH_THREADS) {
        const uint32_t r = rows[i];
        if (r < n && parent[r] == BFT_CC_NONE && mk_move(words, r, through, to)) cnt++;
    }
    mk_block_add(cnt, painted, lds);
}

__global__ __launch_bounds__(BFT_LAUNCH_THREADS) void k_mk_unseed(const uint32_t* __restrict__ rows, uint64_t n_seeds, uint32_t n_rows, const uint32_t* __restrict__ parent,
                                                          uint32_t* __restrict__ best) {
    for (uint64_t i = blockIdx.x * (uint64_t)BFT_LAUNCH_THREADS + threadIdx.x; i < n_seeds; i += (uint64_t)gridDim.x * BFT_LAUNCH_THREADS) {
        const uint32_t r = rows[i];
        const uint32_t p = r < n_rows ? parent[r] : BFT_CC_NONE;
        if (p != BFT_CC_NONE) best[p] = BFT_MK_NONE;  // (seeds of one component all write the same value)
    }
}

struct MkForest {
    BftCcScratch cc;
    uint32_t* best;  // [n] the lowest index of an eligible seed per root, BFT_MK_NONE elsewhere
};
// the arrays of the forest block for n rows and `sets` colour sets (cc.sp.sb set), from `base` on; returns the block's size
size_t mk_carve(uint64_t n, uint64_t sets, uint8_t* base, MkForest* f) {
    Carver c{base};
    c.take(f->cc.sp.start, ((1ull << f->cc.sp.sb) + 1) * 4);
    c.take(f->cc.parent, n * 4);
    c.take(f->cc.member, sets);
    c.take(f->best, n * 4);
    f->cc.num = nullptr;
    return c.off;
}

uint32_t* mk_words(bft_gpu* h) { return h->mk_flags.as<uint32_t>(); }

// What every marks call starts with: the handle is marking, the table is resident, the marks' blocks are this stream's until `lease` leaves scope.
int mk_enter(bft_gpu* h, HandleScratch::Lease& lease, hipStream_t s, const char* what) {
    if (!h->marking) return bft_fail(BFT_GPU_E_STATE, std::string(what) + ": the graph is not initialized for marking (bft_gpu_marks_begin)");
    if (bft_stream_capturing(s)) return bft_fail(BFT_GPU_E_ARG, std::string(what) + " recorded into a graph: not supported (the table may have to come back, scratch may grow)");
    CK(bft_ensure_built(h));  // ("compact_table": the sorted table comes back if an option sent it away; nothing is pending while marking)
    return lease.acquire(s, false);
}

// rows of n resident packed k-mers into h->mk_rows, by the lookup bft_gpu_query_rows uses
int mk_lookup(bft_gpu* h, const uint8_t* d_kmers, uint64_t n, hipStream_t s) {
    CK(h->mk.grow(h->mk_rows, n * 4, n));
    CK(h->mk.grow(h->mk_bits, ((n + 63) / 64) * 8, n / 64));
    return bft_launch_query(h, d_kmers, n, h->mk_bits.as<uint64_t>(), h->mk_rows.as<uint32_t>(), s);
}

enum MkOp { MK_SET, MK_GET, MK_TAS };
// one batch operation on a resident batch; d_io: the flags in (MK_SET, may be NULL), the flags out (MK_GET), the winners out (MK_TAS)
int mk_batch(bft_gpu* h, MkOp op, const uint8_t* d_kmers, uint64_t n, uint8_t* d_io, uint32_t a, uint32_t b, unsigned long long* d_absent, hipStream_t s) {
    if (d_absent) CK(bft_zero_async(d_absent, 8, s));
    if (op != MK_GET) h->mk_forest_ok = false;
    if (n == 0 || h->n_kmers == 0) {
        if (n && op == MK_GET) HIPCK(hipMemsetAsync(d_io, 0xFF, n, s));
        if (n && op == MK_TAS) HIPCK(hipMemsetAsync(d_io, 0, n, s));
        if (n && d_absent) HIPCK(hipMemcpyAsync(d_absent, &n, 8, hipMemcpyHostToDevice, s));
        return 0;
    }
    CK(mk_lookup(h, d_kmers, n, s));
    const uint32_t* rows = h->mk_rows.as<uint32_t>();
    const uint32_t nr = (uint32_t)h->n_kmers;
    return bft_timed_launch(h, s, [&] {
        if (op == MK_SET) return bft_launch256(k_mk_set, n, s, rows, n, nr, (const uint8_t*)d_io, a, mk_words(h), d_absent);
        else if (op == MK_GET) return bft_launch256(k_mk_get, n, s, rows, n, nr, (const uint32_t*)mk_words(h), d_io, d_absent);
        else return bft_launch256(k_mk_tas, n, s, rows, n, nr, a, b, mk_words(h), d_io, d_absent);
    });
}

// The host form of a batch operation: chunks of 2^24 k-mers through device blocks of the call's own.
int mk_batch_host(bft_gpu* h, MkOp op, const uint8_t* kmers, uint64_t n, const uint8_t* in, uint8_t* out, uint32_t a, uint32_t b, uint64_t* n_absent) {
    const hipStream_t s = h->stream;
    if (n_absent) *n_absent = 0;
    if (n == 0) return 0;
    const uint64_t chunk = 1ull << 24, mc = std::min(n, chunk);
    DevBuf dk, dio, dabs;
    CK(dk.alloc(mc * h->B));
    CK(dio.alloc(mc));
    CK(dabs.alloc(8));
    for (uint64_t at = 0; at < n; at += chunk) {
        const uint64_t m = std::min(chunk, n - at);
        HIPCK(hipMemcpyAsync(dk.p, kmers + at * h->B, m * h->B, hipMemcpyHostToDevice, s));
        if (in) HIPCK(hipMemcpyAsync(dio.p, in + at, m, hipMemcpyHostToDevice, s));
        CK(mk_batch(h, op, dk.as<uint8_t>(), m, (op == MK_SET && !in) ? nullptr : dio.as<uint8_t>(), a, b, dabs.as<unsigned long long>(), s));
        unsigned long long ab = 0;
        if (out) HIPCK(hipMemcpyAsync(out + at, dio.p, m, hipMemcpyDeviceToHost, s));
        HIPCK(hipMemcpyAsync(&ab, dabs.p, 8, hipMemcpyDeviceToHost, s));
        HIPCK(hipStreamSynchronize(s));
        if (n_absent) *n_absent += ab;
    }
    return 0;
}

int mk_fill(bft_gpu* h, uint32_t flag, hipStream_t s) {
    h->mk_forest_ok = false;
    const uint64_t nw = bft_mk_words(h->n_kmers);
    if (nw == 0) return 0;
    return bft_timed_launch(h, s, [&] { return bft_launch256(k_mk_fill, nw, s, mk_words(h), nw, (uint32_t)h->n_kmers, flag); });
}

int mk_counts(bft_gpu* h, unsigned long long* d_counts, hipStream_t s) {
    CK(bft_zero_async(d_counts, 32, s));
    const uint64_t nw = bft_mk_words(h->n_kmers);
    if (nw == 0) return 0;
    return bft_timed_launch(h, s, [&] { return bft_launch256(k_mk_counts, nw, s, (const uint32_t*)mk_words(h), nw, (uint32_t)h->n_kmers, d_counts); });
}

// the selection's scan on stream s: slot[] filled (slot[n] included), the number of selected rows at d_count
int mk_select_scan(bft_gpu* h, uint32_t mask, unsigned long long* d_count, hipStream_t s) {
    const uint64_t n = h->n_kmers;
    CK(h->mk.grow(h->mk_slot, (n + 1) * 4, 0));
    CK(h->mk.grow(h->mk_tmp, bft_scan::scratch_bytes(n + 1), 0));
    const BftMkSel sel{mk_words(h), mask};
    return bft_timed_launch(h, s, [&] { return bft_scan::exclusive_sum<uint32_t>(sel, h->mk_slot.as<uint32_t>(), n, s, h->mk_tmp, d_count, true); });
}
int mk_select_emit(bft_gpu* h, uint8_t* d_kmers, char* d_ascii, uint32_t* d_rows, uint64_t cap, hipStream_t s) {
    const BftPgScratch p{h->mk_slot.as<uint32_t>(), nullptr};
    return bft_timed_launch(h, s, [&] { return bft_pg_emit(h->W, h->d_tk.as<uint64_t>(), h->n_kmers, h->k, h->B, p, d_kmers, d_ascii, d_rows, cap, s); });
}

int mk_check_ids(const uint32_t* ids, uint32_t nb) {
    if (nb && !ids) return bft_fail(BFT_GPU_E_ARG, "NULL argument");
    for (uint32_t j = 1; j < nb; j++)
        if (ids[j] <= ids[j - 1]) return bft_fail(BFT_GPU_E_ARG, "marks_reach: genome ids must be strictly increasing");
    return 0;
}
int mk_check_reach(const bft_gpu* h, uint32_t through, uint32_t to) {
    if (through > 3 || to > 3) return bft_fail(BFT_GPU_E_ARG, "marks_reach: a flag can only have as value 0, 1, 2 or 3");
    if (through == to) return bft_fail(BFT_GPU_E_ARG, "marks_reach: `to` must differ from `through`");
    if (h->n_kmers >= (1ull << 31)) return bft_fail(BFT_GPU_E_LIMIT, "marks_reach: at most 2^31 - 1 k-mers");
    return 0;
}

// The reach on stream s; d_counts: {members painted, boundary rows painted, seeds absent} (24 bytes, device); d_seed_new may be NULL.
int mk_reach(bft_gpu* h, const uint8_t* d_seeds, uint64_t n_seeds, const uint32_t* ids, uint32_t nb, uint32_t through, uint32_t to, bool boundary,
             uint8_t* d_seed_new, unsigned long long* d_counts, hipStream_t s) {
    const uint64_t n = h->n_kmers, ns = h->n_sets;
    const int W = h->W, k = h->k;
    CK(bft_zero_async(d_counts, 24, s));
    if (n == 0) {
        if (n_seeds && d_seed_new) HIPCK(hipMemsetAsync(d_seed_new, 0, n_seeds, s));
        if (n_seeds) HIPCK(hipMemcpyAsync(d_counts + 2, &n_seeds, 8, hipMemcpyHostToDevice, s));
        return 0;
    }
    const uint64_t* tk = h->d_tk.as<uint64_t>();
    MkForest f{};
    f.cc.sp.sb = bft_sp_bucket_bits(k);
    const bool cached = h->mk_forest_ok && h->mk_forest_through == through && h->mk_forest_ids.size() == nb && std::equal(ids, ids + nb, h->mk_forest_ids.begin());
    if (!cached) {
        h->mk_forest_ok = false;
        CK(h->mk.grow(h->mk_forest, mk_carve(n, ns, nullptr, &f), 0));
    }
    mk_carve(n, ns, h->mk_forest.as<uint8_t>(), &f);
    if (n_seeds) CK(mk_lookup(h, d_seeds, n_seeds, s));
    const uint32_t* rows = h->mk_rows.as<uint32_t>();
    if (!cached) {
        for (uint32_t j = 0; j < nb; j += BFT_CC_IDS)
            CK(bft_timed_launch(h, s, [&] { return bft_cc_sets(ns, h->d_cs_off.as<uint32_t>(), h->d_cs_ids.p, h->cs_w, ids + j, nb - j, j == 0, f.cc, s); }));
        CK(bft_timed_launch(h, s, [&] { return bft_cc_init(n, nb ? h->d_tcol.as<uint32_t>() : nullptr, f.cc, s, mk_words(h), through); }));
        CK(bft_timed_launch(h, s, [&] { return bft_sp_buckets(W, tk, n, k, f.cc.sp, s); }));
        CK(bft_timed_launch(h, s, [&] { return bft_cc_hook(W, tk, n, k, f.cc, s); }));
        CK(bft_timed_launch(h, s, [&] { return bft_cc_flatten(n, f.cc, s); }));
        CK(bft_timed_launch(h, s, [&] { return bft_launch256(k_mk_unhit, n, s, (uint32_t)n, f.best); }));
        h->mk_forest_through = through;
        h->mk_forest_ids.assign(ids, ids + nb);
        h->mk_forest_ok = true;
    }
    if (n_seeds == 0) return 0;
    const uint64_t nw = bft_mk_words(n);
    CK(bft_timed_launch(h, s, [&] {
        return bft_launch256(k_mk_seed, n_seeds, s, rows, n_seeds, (uint32_t)n, (const uint32_t*)f.cc.parent, (const uint32_t*)mk_words(h), through,
                             f.best, d_counts + 2);
    }));
    CK(bft_timed_launch(h, s, [&] {
        return bft_launch256(k_mk_paint, nw, s, (uint32_t)n, nw, (const uint32_t*)f.cc.parent, (const uint32_t*)f.best, mk_words(h), through, to,
                             rows, n_seeds, d_seed_new, d_counts);
    }));
    if (boundary)
        CK(bft_timed_launch(h, s, [&] {
            return bft_for_w(W, [&](auto KW) {
                return bft_launch256(k_mk_boundary<KW>, n, s, tk, (uint32_t)n, k, f.cc.sp.sb, (const uint32_t*)f.cc.sp.start, (const uint32_t*)f.cc.parent,
                                     (const uint32_t*)f.best, mk_words(h), through, to, rows, n_seeds, d_counts + 1);
            });
        }));
    return bft_timed_launch(h, s, [&] { return bft_launch256(k_mk_unseed, n_seeds, s, rows, n_seeds, (uint32_t)n, (const uint32_t*)f.cc.parent, f.best); });
}

hipStream_t mk_stream(bft_gpu* h, void* hip_stream) { return hip_stream ? (hipStream_t)hip_stream : h->stream; }

}  // namespace

// ------------------------------------------------------------------------------------------------
// the C-ABI entry points
// ------------------------------------------------------------------------------------------------
extern "C" int bft_gpu_marks_begin(bft_gpu* h) {
    if (!h) return bft_fail(BFT_GPU_E_ARG, "NULL handle");
    ENTER(h);
    if (h->marking) return BFT_GPU_OK;  // (src/bft.c:694: a graph that is already marking keeps its flags)
    CK(bft_ensure_built(h));
    if (h->n_kmers >= (1ull << 32) - 1) return bft_fail(BFT_GPU_E_LIMIT, "marks: at most 2^32 - 2 k-mers");
    {
        HandleScratch::Lease lease(h->mk);
        CK(lease.acquire(h->stream, false));
        const size_t bytes = (size_t)bft_mk_words(h->n_kmers) * 4;
        CK(h->mk_flags.alloc(bytes));
        if (bytes) CK(bft_zero_async(h->mk_flags.p, bytes, h->stream));
    }
    h->mk_forest_ok = false;
    h->marking = true;
    return BFT_GPU_OK;
}

extern "C" int bft_gpu_marks_end(bft_gpu* h) {
    if (!h) return bft_fail(BFT_GPU_E_ARG, "NULL handle");
    ENTER(h);
    if (!h->marking) return BFT_GPU_OK;
    HandleScratch::Lease lease(h->mk);
    CK(lease.acquire(h->stream, false));  // (a use on a caller's stream ends first)
    HIPCK(hipStreamSynchronize(h->stream));
    h->mk_flags.release();
    h->mk_rows.release();
    h->mk_bits.release();
    h->mk_slot.release();
    h->mk_tmp.release();
    h->mk_forest.release();
    h->mk_forest_ok = false;
    h->marking = false;
    return BFT_GPU_OK;
}

#define MK_FLAG(f, what)                                                                                      \
    do {                                                                                                      \
        if ((f) > 3) return bft_fail(BFT_GPU_E_ARG, what ": a flag can only have as value 0, 1, 2 or 3"); \
    } while (0)

extern "C" int bft_gpu_marks_set_dev(bft_gpu* h, const void* d_kmers, uint64_t nb_kmers, const void* d_flags, uint8_t flag, void* d_n_absent, void* hip_stream) {
    if (!h || (!d_kmers && nb_kmers)) return bft_fail(BFT_GPU_E_ARG, "NULL argument");
    if (!d_flags) MK_FLAG(flag, "marks_set");
    ENTER(h);
    const hipStream_t s = mk_stream(h, hip_stream);
    {
        HandleScratch::Lease lease(h->mk);
        CK(mk_enter(h, lease, s, "marks_set"));
        CK(mk_batch(h, MK_SET, (const uint8_t*)d_kmers, nb_kmers, (uint8_t*)d_flags, flag, 0, (unsigned long long*)d_n_absent, s));
    }
    return bft_note_foreign_stream(h, s);
}
extern "C" int bft_gpu_marks_set(bft_gpu* h, const uint8_t* kmers, uint64_t nb_kmers, const uint8_t* flags, uint8_t flag, uint64_t* n_absent) {
    if (!h || (!kmers && nb_kmers)) return bft_fail(BFT_GPU_E_ARG, "NULL argument");
    if (!flags) MK_FLAG(flag, "marks_set");
    for (uint64_t i = 0; flags && i < nb_kmers; i++) MK_FLAG(flags[i], "marks_set");
    ENTER(h);
    HandleScratch::Lease lease(h->mk);
    CK(mk_enter(h, lease, h->stream, "marks_set"));
    CK(mk_batch_host(h, MK_SET, kmers, nb_kmers, flags, nullptr, flag, 0, n_absent));
    return BFT_GPU_OK;
}

extern "C" int bft_gpu_marks_get_dev(bft_gpu* h, const void* d_kmers, uint64_t nb_kmers, void* d_flags_out, void* d_n_absent, void* hip_stream) {
    if (!h || ((!d_kmers || !d_flags_out) && nb_kmers)) return bft_fail(BFT_GPU_E_ARG, "NULL argument");
    ENTER(h);
    const hipStream_t s = mk_stream(h, hip_stream);
    {
        HandleScratch::Lease lease(h->mk);
        CK(mk_enter(h, lease, s, "marks_get"));
        CK(mk_batch(h, MK_GET, (const uint8_t*)d_kmers, nb_kmers, (uint8_t*)d_flags_out, 0, 0, (unsigned long long*)d_n_absent, s));
    }
    return bft_note_foreign_stream(h, s);
}
extern "C" int bft_gpu_marks_get(bft_gpu* h, const uint8_t* kmers, uint64_t nb_kmers, uint8_t* flags_out, uint64_t* n_absent) {
    if (!h || ((!kmers || !flags_out) && nb_kmers)) return bft_fail(BFT_GPU_E_ARG, "NULL argument");
    ENTER(h);
    HandleScratch::Lease lease(h->mk);
    CK(mk_enter(h, lease, h->stream, "marks_get"));
    CK(mk_batch_host(h, MK_GET, kmers, nb_kmers, nullptr, flags_out, 0, 0, n_absent));
    return BFT_GPU_OK;
}

extern "C" int bft_gpu_marks_test_and_set_dev(bft_gpu* h, const void* d_kmers, uint64_t nb_kmers, uint8_t expect, uint8_t flag, void* d_won_out, void* d_n_absent,
                                              void* hip_stream) {
    if (!h || ((!d_kmers || !d_won_out) && nb_kmers)) return bft_fail(BFT_GPU_E_ARG, "NULL argument");
    MK_FLAG(expect, "marks_test_and_set");
    MK_FLAG(flag, "marks_test_and_set");
    if (expect == flag) return bft_fail(BFT_GPU_E_ARG, "marks_test_and_set: `flag` must differ from `expect`");
    ENTER(h);
    const hipStream_t s = mk_stream(h, hip_stream);
    {
        HandleScratch::Lease lease(h->mk);
        CK(mk_enter(h, lease, s, "marks_test_and_set"));
        CK(mk_batch(h, MK_TAS, (const uint8_t*)d_kmers, nb_kmers, (uint8_t*)d_won_out, expect, flag, (unsigned long long*)d_n_absent, s));
    }
    return bft_note_foreign_stream(h, s);
}
extern "C" int bft_gpu_marks_test_and_set(bft_gpu* h, const uint8_t* kmers, uint64_t nb_kmers, uint8_t expect, uint8_t flag, uint8_t* won_out, uint64_t* n_absent) {
    if (!h || ((!kmers || !won_out) && nb_kmers)) return bft_fail(BFT_GPU_E_ARG, "NULL argument");
    MK_FLAG(expect, "marks_test_and_set");
    MK_FLAG(flag, "marks_test_and_set");
    if (expect == flag) return bft_fail(BFT_GPU_E_ARG, "marks_test_and_set: `flag` must differ from `expect`");
    ENTER(h);
    HandleScratch::Lease lease(h->mk);
    CK(mk_enter(h, lease, h->stream, "marks_test_and_set"));
    CK(mk_batch_host(h, MK_TAS, kmers, nb_kmers, nullptr, won_out, expect, flag, n_absent));
    return BFT_GPU_OK;
}

extern "C" int bft_gpu_marks_fill_dev(bft_gpu* h, uint8_t flag, void* hip_stream) {
    if (!h) return bft_fail(BFT_GPU_E_ARG, "NULL handle");
    MK_FLAG(flag, "marks_fill");
    ENTER(h);
    const hipStream_t s = mk_stream(h, hip_stream);
    {
        HandleScratch::Lease lease(h->mk);
        CK(mk_enter(h, lease, s, "marks_fill"));
        CK(mk_fill(h, flag, s));
    }
    return bft_note_foreign_stream(h, s);
}
extern "C" int bft_gpu_marks_fill(bft_gpu* h, uint8_t flag) {
    if (!h) return bft_fail(BFT_GPU_E_ARG, "NULL handle");
    MK_FLAG(flag, "marks_fill");
    ENTER(h);
    HandleScratch::Lease lease(h->mk);
    CK(mk_enter(h, lease, h->stream, "marks_fill"));
    CK(mk_fill(h, flag, h->stream));
    HIPCK(hipStreamSynchronize(h->stream));
    return BFT_GPU_OK;
}

extern "C" int bft_gpu_marks_counts_dev(bft_gpu* h, void* d_counts, void* hip_stream) {
    if (!h || !d_counts) return bft_fail(BFT_GPU_E_ARG, "NULL argument");
    ENTER(h);
    const hipStream_t s = mk_stream(h, hip_stream);
    {
        HandleScratch::Lease lease(h->mk);
        CK(mk_enter(h, lease, s, "marks_counts"));
        CK(mk_counts(h, (unsigned long long*)d_counts, s));
    }
    return bft_note_foreign_stream(h, s);
}
extern "C" int bft_gpu_marks_counts(bft_gpu* h, uint64_t* counts) {
    if (!h || !counts) return bft_fail(BFT_GPU_E_ARG, "NULL argument");
    ENTER(h);
    HandleScratch::Lease lease(h->mk);
    CK(mk_enter(h, lease, h->stream, "marks_counts"));
    DevBuf d;
    CK(d.alloc(32));
    CK(mk_counts(h, d.as<unsigned long long>(), h->stream));
    HIPCK(hipMemcpyAsync(counts, d.p, 32, hipMemcpyDeviceToHost, h->stream));
    HIPCK(hipStreamSynchronize(h->stream));
    return BFT_GPU_OK;
}

extern "C" int bft_gpu_marks_select_dev(bft_gpu* h, uint32_t mask, void* d_kmers_out, void* d_ascii_out, void* d_rows_out, uint64_t cap, void* d_count, void* hip_stream) {
    if (!h || !d_count) return bft_fail(BFT_GPU_E_ARG, "NULL argument");
    if (mask > 15) return bft_fail(BFT_GPU_E_ARG, "marks_select: the mask has one bit per flag value, 0 .. 15");
    ENTER(h);
    const hipStream_t s = mk_stream(h, hip_stream);
    {
        HandleScratch::Lease lease(h->mk);
        CK(mk_enter(h, lease, s, "marks_select"));
        if (h->n_kmers >= (1ull << 31)) return bft_fail(BFT_GPU_E_LIMIT, "marks_select: at most 2^31 - 1 k-mers");
        if (h->n_kmers == 0) CK(bft_zero_async(d_count, 8, s));
        else {
            CK(mk_select_scan(h, mask, (unsigned long long*)d_count, s));
            CK(mk_select_emit(h, (uint8_t*)d_kmers_out, (char*)d_ascii_out, (uint32_t*)d_rows_out, cap, s));
        }
    }
    return bft_note_foreign_stream(h, s);
}
// The host form: the selection is counted on the device, and the outputs filled only when cap holds it all (as bft_gpu_kmers_by_count).
extern "C" int bft_gpu_marks_select(bft_gpu* h, uint32_t mask, uint8_t* kmers_out, char* ascii_out, uint32_t* rows_out, uint64_t cap, uint64_t* n_out) {
    if (!h || !n_out) return bft_fail(BFT_GPU_E_ARG, "NULL argument");
    if (mask > 15) return bft_fail(BFT_GPU_E_ARG, "marks_select: the mask has one bit per flag value, 0 .. 15");
    ENTER(h);
    const hipStream_t s = h->stream;
    HandleScratch::Lease lease(h->mk);
    CK(mk_enter(h, lease, s, "marks_select"));
    *n_out = 0;
    if (h->n_kmers >= (1ull << 31)) return bft_fail(BFT_GPU_E_LIMIT, "marks_select: at most 2^31 - 1 k-mers");
    if (h->n_kmers == 0) return BFT_GPU_OK;
    DevBuf dcnt;
    CK(dcnt.alloc(8));
    CK(mk_select_scan(h, mask, dcnt.as<unsigned long long>(), s));
    unsigned long long cnt = 0;
    HIPCK(hipMemcpyAsync(&cnt, dcnt.p, 8, hipMemcpyDeviceToHost, s));
    HIPCK(hipStreamSynchronize(s));
    *n_out = cnt;
    const bool any = kmers_out || ascii_out || rows_out;
    if (any && cap < cnt) return bft_fail(BFT_GPU_E_NOSPACE, "marks_select: buffers too small");
    if (any && cnt) {
        const size_t kb = (size_t)cnt * h->B, ab = (size_t)cnt * (h->k + 1);
        DevBuf dk, da, dr;
        if (kmers_out) CK(dk.alloc(kb));
        if (ascii_out) CK(da.alloc(ab));
        if (rows_out) CK(dr.alloc(cnt * 4));
        CK(mk_select_emit(h, kmers_out ? dk.as<uint8_t>() : nullptr, ascii_out ? da.as<char>() : nullptr, rows_out ? dr.as<uint32_t>() : nullptr, cnt, s));
        if (kmers_out) HIPCK(hipMemcpyAsync(kmers_out, dk.p, kb, hipMemcpyDeviceToHost, s));
        if (ascii_out) HIPCK(hipMemcpyAsync(ascii_out, da.p, ab, hipMemcpyDeviceToHost, s));
        if (rows_out) HIPCK(hipMemcpyAsync(rows_out, dr.p, cnt * 4, hipMemcpyDeviceToHost, s));
        HIPCK(hipStreamSynchronize(s));
    }
    return BFT_GPU_OK;
}

extern "C" int bft_gpu_marks_reach_dev(bft_gpu* h, const void* d_seeds, uint64_t n_seeds, const uint32_t* genome_ids, uint32_t nb_ids, uint8_t through, uint8_t to,
                                       int boundary, void* d_seed_new, void* d_counts, void* hip_stream) {
    if (!h || !d_counts || (!d_seeds && n_seeds)) return bft_fail(BFT_GPU_E_ARG, "NULL argument");
    CK(mk_check_ids(genome_ids, nb_ids));
    ENTER(h);
    const hipStream_t s = mk_stream(h, hip_stream);
    {
        HandleScratch::Lease lease(h->mk);
        CK(mk_enter(h, lease, s, "marks_reach"));
        CK(mk_check_reach(h, through, to));
        CK(mk_reach(h, (const uint8_t*)d_seeds, n_seeds, genome_ids, nb_ids, through, to, boundary != 0, (uint8_t*)d_seed_new, (unsigned long long*)d_counts, s));
    }
    return bft_note_foreign_stream(h, s);
}
extern "C" int bft_gpu_marks_reach(bft_gpu* h, const uint8_t* seeds, uint64_t n_seeds, const uint32_t* genome_ids, uint32_t nb_ids, uint8_t through, uint8_t to,
                                   int boundary, uint8_t* seed_new, uint64_t* counts) {
    if (!h || (!seeds && n_seeds)) return bft_fail(BFT_GPU_E_ARG, "NULL argument");
    CK(mk_check_ids(genome_ids, nb_ids));
    ENTER(h);
    const hipStream_t s = h->stream;
    HandleScratch::Lease lease(h->mk);
    CK(mk_enter(h, lease, s, "marks_reach"));
    CK(mk_check_reach(h, through, to));
    DevBuf dk, dn, dc;
    CK(dk.alloc(n_seeds * h->B));
    CK(dn.alloc(n_seeds));
    CK(dc.alloc(24));
    if (n_seeds) HIPCK(hipMemcpyAsync(dk.p, seeds, n_seeds * h->B, hipMemcpyHostToDevice, s));
    CK(mk_reach(h, dk.as<uint8_t>(), n_seeds, genome_ids, nb_ids, through, to, boundary != 0, dn.as<uint8_t>(), dc.as<unsigned long long>(), s));
    unsigned long long cnt[3] = {0, 0, 0};
    if (seed_new && n_seeds) HIPCK(hipMemcpyAsync(seed_new, dn.p, n_seeds, hipMemcpyDeviceToHost, s));
    HIPCK(hipMemcpyAsync(cnt, dc.p, 24, hipMemcpyDeviceToHost, s));
    HIPCK(hipStreamSynchronize(s));
    if (counts)
        for (int i = 0; i < 3; i++) counts[i] = cnt[i];
    return BFT_GPU_OK;
}

extern "C" int bft_gpu_marks_read(bft_gpu* h, uint8_t* bytes_out, uint64_t cap, uint64_t* n_bytes) {
    if (!h) return bft_fail(BFT_GPU_E_ARG, "NULL handle");
    ENTER(h);
    HandleScratch::Lease lease(h->mk);
    CK(mk_enter(h, lease, h->stream, "marks_read"));
    const uint64_t nb = bft_mk_bytes(h->n_kmers);
    if (n_bytes) *n_bytes = nb;
    if (bytes_out) {
        if (cap < nb) return bft_fail(BFT_GPU_E_NOSPACE, "marks_read: buffer too small");
        if (nb) HIPCK(hipMemcpyAsync(bytes_out, h->mk_flags.p, nb, hipMemcpyDeviceToHost, h->stream));
        HIPCK(hipStreamSynchronize(h->stream));
    }
    return BFT_GPU_OK;
}

extern "C" int bft_gpu_marks_write(bft_gpu* h, const uint8_t* bytes_in, uint64_t n_bytes) {
    if (!h || (!bytes_in && n_bytes)) return bft_fail(BFT_GPU_E_ARG, "NULL argument");
    ENTER(h);
    HandleScratch::Lease lease(h->mk);
    CK(mk_enter(h, lease, h->stream, "marks_write"));
    const uint64_t n = h->n_kmers, nb = bft_mk_bytes(n);
    if (n_bytes != nb) return bft_fail(BFT_GPU_E_ARG, "marks_write: the array holds CEIL(k-mers / 4) bytes");
    if ((n & 3u) && (bytes_in[nb - 1] >> (2u * (n & 3u)))) return bft_fail(BFT_GPU_E_ARG, "marks_write: the bits behind the last k-mer must be 0");
    h->mk_forest_ok = false;
    if (nb) {
        // (the last word's bytes past the array stay 0, as bft_gpu_marks_begin and the fill leave them)
        CK(bft_zero_async(h->mk_flags.as<uint32_t>() + (bft_mk_words(n) - 1), 4, h->stream));
        HIPCK(hipMemcpyAsync(h->mk_flags.p, bytes_in, nb, hipMemcpyHostToDevice, h->stream));
        HIPCK(hipStreamSynchronize(h->stream));
    }
    return BFT_GPU_OK;
}
