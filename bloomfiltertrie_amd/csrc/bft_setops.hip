// bft_setops.hip -- colour-set algebra over groups of k-mers: intersection_annotations / union_annotations / sym_difference_annotations (reference
// include/bft.h:112-114, src/bft.c:421-613) for a batch of groups, without a row per k-mer leaving the GPU.  Group g is the members
// group_off[g] .. group_off[g + 1] of the batch; a member is a colour-set id (what the k-mer hash hands out with im.emit_cs, or the caller's array), and
// its set a row of the dictionary: a bitmap row of d_cs_bm, or -- where that form does not exist -- the sorted id list cs_off / cs_ids.  A segmented
// reduction of dictionary rows into one row per group, held in dwords (R: ng x nw) until the last kernel:
//   k_so_plan    a lane per group: the groups of more than BFT_SO_WAVE_MAX members go on the split list, their accumulators are set up
//   k_so_small   groups of up to BFT_SO_SMALL members: a lane per (group, word of the row); a wavefront holds 64 pairs at up to 32 genomes, and the
//                lanes of one wide row read consecutive words of each dictionary row
//   k_so_wave    groups up to BFT_SO_WAVE_MAX: a wavefront per group.  Rows of one or two words (<= 64 genomes): a lane per member, 64 at a time, and a
//                shuffle reduction at the end.  Wider rows: lanes across the words of the row, 64 words at a time; the members' ids are loaded 64 at a
//                time and only the heads of runs of equal ids (one ballot) are visited
//   k_so_split   the groups of the list in steps of BFT_SO_CHUNK members, a wavefront per step, the same two reductions; a step ends with 32-bit
//                atomicAnd / atomicOr into the group's accumulators (R; X holds the AND of a SYMDIFF) and an atomicAdd of its found members
//   k_so_finish  the split groups' accumulators become their result
//   k_so_emit    R into the caller's rows of CEIL(G / 8) bytes: a lane per ALIGNED dword of the output array (its four bytes may belong to two rows);
//                only the array's first and last dword, where they are partial, are written as bytes -- nothing outside the array is touched
//   k_so_count   counts[g] = the bits of row g: 1 .. 64 lanes per group
// A dictionary row is fetched once per run of equal ids, never per member; an AND that has reached zero stops fetching (its members are still
// counted).  A group whose end lies before its start or past the batch is empty (so_range): no kernel reads outside the batch, whatever the offsets
// hold.  Integer AND / OR / ADD only: results do not depend on scheduling.  No kernel needs scratch memory.
#include "bft_dev.h"
#include "bft_handle.h"
#include "bft_setops.h"
#include "bft_walk.h"

namespace {

constexpr int SO_THREADS = 256;
constexpr int SO_SPLIT_BLOCKS = 512;
constexpr int SO_FINISH_BLOCKS = 64;

__device__ __forceinline__ void so_range(const uint64_t* __restrict__ off, uint64_t g, uint64_t n, uint64_t& a, uint64_t& e) {
    a = off[g];
    e = off[g + 1];
    if (e < a || e > n) a = e = 0;
}
// (an id that is no set of the dictionary is the empty set: it takes the absent k-mer's role)
__device__ __forceinline__ uint32_t so_id(const uint32_t* __restrict__ cs, uint64_t i, uint32_t n_sets) {
    const uint32_t c = cs[i];
    return c < n_sets ? c : BFT_SO_ABSENT;
}
// word w of the row of set c
__device__ __forceinline__ uint32_t so_word(const BftSoDict& d, uint32_t c, uint32_t w) {
    if (d.bm) return d.bm[(uint64_t)c * d.stride32 + w];
    const uint32_t e = d.cs_off[c + 1], first = w * 32u;
    uint32_t lo = d.cs_off[c], hi = e;  // the first id >= first (the list ascends)
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (bft_cs_id_at(d.cs_ids, d.cs_w, mid) < first) lo = mid + 1;
        else hi = mid;
    }
    uint32_t v = 0;
    for (; lo < e; lo++) {
        const uint32_t id = bft_cs_id_at(d.cs_ids, d.cs_w, lo) - first;
        if (id >= 32u) break;
        v |= 1u << id;
    }
    return v;
}
__device__ __forceinline__ uint32_t so_mask(const BftSoDict& d, uint32_t w) { return (w + 1u == d.nw && (d.G & 31u)) ? (1u << (d.G & 31u)) - 1u : 0xFFFFFFFFu; }
// the result word from the AND and OR of the members that count (neff of them; A is already zero where an absent member counts as the empty set)
__device__ __forceinline__ uint32_t so_final(int op, uint32_t A, uint32_t O, uint64_t neff, uint32_t mask) {
    const uint32_t v = op == BFT_GPU_SETOP_AND ? (neff ? A : 0u) : op == BFT_GPU_SETOP_OR ? O : neff == 1 ? O : (O & ~A);
    return v & mask;
}
__device__ __forceinline__ uint32_t so_wave_and(uint32_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v &= (uint32_t)__shfl_xor((int)v, d);
    return v;
}
__device__ __forceinline__ uint32_t so_wave_or(uint32_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v |= (uint32_t)__shfl_xor((int)v, d);
    return v;
}
__device__ __forceinline__ uint32_t so_wave_sum(uint32_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d);
    return v;
}

__global__ __launch_bounds__(SO_THREADS) void k_so_plan(BftSoDict d, BftSoBatch b, unsigned long long* __restrict__ nsplit, uint32_t* __restrict__ split) {
    for (uint64_t g = blockIdx.x * (uint64_t)SO_THREADS + threadIdx.x; g < b.ng; g += (uint64_t)gridDim.x * SO_THREADS) {
        uint64_t a, e;
        so_range(b.off, g, b.n, a, e);
        if (e - a <= BFT_SO_WAVE_MAX) continue;
        split[atomicAdd(nsplit, 1ull)] = (uint32_t)g;  // (at most one entry per group: the list has ng entries)
        b.nf[g] = 0;
        for (uint32_t w = 0; w < d.nw; w++) {
            b.R[g * d.nw + w] = b.op == BFT_GPU_SETOP_AND ? 0xFFFFFFFFu : 0u;
            if (b.op == BFT_GPU_SETOP_SYMDIFF) b.X[g * d.nw + w] = 0xFFFFFFFFu;
        }
    }
}

__global__ __launch_bounds__(SO_THREADS) void k_so_small(BftSoDict d, BftSoBatch b) {
    const uint64_t items = b.ng * d.nw;
    for (uint64_t t = blockIdx.x * (uint64_t)SO_THREADS + threadIdx.x; t < items; t += (uint64_t)gridDim.x * SO_THREADS) {
        const uint64_t g = t / d.nw;
        const uint32_t w = (uint32_t)(t - g * d.nw);
        uint64_t a, e;
        so_range(b.off, g, b.n, a, e);
        if (e - a > BFT_SO_SMALL) continue;
        uint32_t A = 0xFFFFFFFFu, O = 0, fnd = 0, prev = BFT_SO_NONE;
        bool hole = false;
        for (uint64_t i = a; i < e; i++) {
            const uint32_t c = so_id(b.cs, i, d.n_sets);
            if (c == BFT_SO_ABSENT) {
                hole = true;
                continue;
            }
            fnd++;
            if (c == prev) continue;
            prev = c;
            if (b.op == BFT_GPU_SETOP_AND && (A == 0 || (hole && !b.skip))) continue;  // (already empty: nothing more to fetch)
            const uint32_t v = so_word(d, c, w);
            A &= v;
            O |= v;
        }
        if (hole && !b.skip) A = 0;
        b.R[t] = so_final(b.op, A, O, b.skip ? (uint64_t)fnd : e - a, so_mask(d, w));
        if (w == 0) b.nf[g] = fnd;
    }
}

// The members a .. e of one group (or of one step of a split group) reduced by one wavefront: sink(w, A, O) is called by the lane that holds word w,
// with the AND (zero already where an absent member counts) and the OR of the members' rows; *fnd = found members (the same in every lane).
template <bool NARROW, class Sink>
__device__ __forceinline__ void so_wave_reduce(const BftSoDict& d, const uint32_t* __restrict__ cs, uint64_t a, uint64_t e, int op, int skip, uint32_t lane,
                                               uint32_t* fnd, Sink&& sink) {
    if constexpr (NARROW) {  // one or two words: a lane per member
        uint32_t A0 = 0xFFFFFFFFu, A1 = 0xFFFFFFFFu, O0 = 0, O1 = 0, f = 0;
        bool hole = false;
        for (uint64_t i = a + lane; i < e; i += 64) {
            const uint32_t c = so_id(cs, i, d.n_sets);
            if (c == BFT_SO_ABSENT) {
                hole = true;
                continue;
            }
            f++;
            if (i > a && so_id(cs, i - 1, d.n_sets) == c) continue;  // (the head of the run fetches the row)
            const uint32_t v0 = so_word(d, c, 0), v1 = d.nw > 1 ? so_word(d, c, 1) : 0u;
            A0 &= v0;
            A1 &= v1;
            O0 |= v0;
            O1 |= v1;
        }
        A0 = so_wave_and(A0);
        A1 = so_wave_and(A1);
        O0 = so_wave_or(O0);
        O1 = so_wave_or(O1);
        *fnd = so_wave_sum(f);
        if (__ballot(hole) != 0ull && !skip) A0 = A1 = 0;
        if (lane == 0) {
            sink(0u, A0, O0);
            if (d.nw > 1) sink(1u, A1, O1);
        }
        return;
    }
    uint32_t f = 0;
    for (uint32_t w0 = 0; w0 < d.nw; w0 += 64) {  // lanes across 64 words of the row at a time
        const uint32_t w = w0 + lane;
        const bool act = w < d.nw;
        uint32_t A = 0xFFFFFFFFu, O = 0, prev = BFT_SO_NONE;
        bool hole = false;
        for (uint64_t i0 = a; i0 < e; i0 += 64) {
            const bool valid = i0 + lane < e;
            const uint32_t c = valid ? so_id(cs, i0 + lane, d.n_sets) : BFT_SO_ABSENT;
            uint32_t up = (uint32_t)__shfl_up((int)c, 1);
            if (lane == 0) up = prev;
            const bool present = valid && c != BFT_SO_ABSENT;
            if (w0 == 0) f += (uint32_t)__popcll(__ballot(present));
            if (__ballot(valid && !present) != 0ull) hole = true;
            unsigned long long heads = __ballot(present && c != up);  // the first member of every run of one set
            prev = (uint32_t)__shfl((int)c, 63);
            if (prev == BFT_SO_ABSENT) prev = BFT_SO_NONE;
            while (heads) {
                const int j = __ffsll((long long)heads) - 1;
                heads &= heads - 1;
                const uint32_t cj = (uint32_t)__shfl((int)c, j);
                if (act && !(op == BFT_GPU_SETOP_AND && A == 0)) {
                    const uint32_t v = so_word(d, cj, w);
                    A &= v;
                    O |= v;
                }
            }
        }
        if (hole && !skip) A = 0;
        if (w0 == 0) *fnd = f;
        if (act) sink(w, A, O);
    }
}

template <bool NARROW>
__global__ __launch_bounds__(SO_THREADS) void k_so_wave(BftSoDict d, BftSoBatch b) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t waves = (uint64_t)gridDim.x * (SO_THREADS / 64);
    for (uint64_t g = blockIdx.x * (uint64_t)(SO_THREADS / 64) + (threadIdx.x >> 6); g < b.ng; g += waves) {
        uint64_t a, e;
        so_range(b.off, g, b.n, a, e);
        if (e - a <= BFT_SO_SMALL || e - a > BFT_SO_WAVE_MAX) continue;
        uint32_t fnd = 0;
        so_wave_reduce<NARROW>(d, b.cs, a, e, b.op, b.skip, lane, &fnd, [&](uint32_t w, uint32_t A, uint32_t O) {
            b.R[g * d.nw + w] = so_final(b.op, A, O, b.skip ? (uint64_t)fnd : e - a, so_mask(d, w));
        });
        if (lane == 0) b.nf[g] = fnd;
    }
}

template <bool NARROW>
__global__ __launch_bounds__(SO_THREADS) void k_so_split(BftSoDict d, BftSoBatch b, const unsigned long long* __restrict__ nsplit, const uint32_t* __restrict__ split) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t waves = (uint64_t)gridDim.x * (SO_THREADS / 64), wave = blockIdx.x * (uint64_t)(SO_THREADS / 64) + (threadIdx.x >> 6);
    const uint64_t ns = min((uint64_t)*nsplit, b.ng);
    for (uint64_t li = 0; li < ns; li++) {
        const uint64_t g = split[li];
        uint64_t a, e;
        so_range(b.off, g, b.n, a, e);
        const uint64_t steps = (e - a + BFT_SO_CHUNK - 1) / BFT_SO_CHUNK;
        for (uint64_t st = wave; st < steps; st += waves) {
            const uint64_t sa = a + st * BFT_SO_CHUNK, se = min(e, sa + BFT_SO_CHUNK);
            uint32_t fnd = 0;
            so_wave_reduce<NARROW>(d, b.cs, sa, se, b.op, b.skip, lane, &fnd, [&](uint32_t w, uint32_t A, uint32_t O) {
                uint32_t* const r = b.R + g * d.nw + w;
                if (b.op == BFT_GPU_SETOP_AND) {
                    if (A != 0xFFFFFFFFu) atomicAnd(r, A);
                } else {
                    if (O) atomicOr(r, O);
                    if (b.op == BFT_GPU_SETOP_SYMDIFF && A != 0xFFFFFFFFu) atomicAnd(b.X + g * d.nw + w, A);
                }
            });
            if (lane == 0 && fnd) atomicAdd(&b.nf[g], fnd);
        }
    }
}

__global__ __launch_bounds__(SO_THREADS) void k_so_finish(BftSoDict d, BftSoBatch b, const unsigned long long* __restrict__ nsplit, const uint32_t* __restrict__ split) {
    const uint64_t items = min((uint64_t)*nsplit, b.ng) * d.nw;
    for (uint64_t t = blockIdx.x * (uint64_t)SO_THREADS + threadIdx.x; t < items; t += (uint64_t)gridDim.x * SO_THREADS) {
        const uint64_t g = split[t / d.nw];
        const uint32_t w = (uint32_t)(t % d.nw);
        uint64_t a, e;
        so_range(b.off, g, b.n, a, e);
        const uint32_t r = b.R[g * d.nw + w];
        const uint32_t A = b.op == BFT_GPU_SETOP_AND ? r : b.op == BFT_GPU_SETOP_SYMDIFF ? b.X[g * d.nw + w] : 0u;
        b.R[g * d.nw + w] = so_final(b.op, A, r, b.skip ? (uint64_t)b.nf[g] : e - a, so_mask(d, w));
    }
}

// rows: ng x rb bytes at any alignment; lane t holds the aligned dword t of the array (dword 0 starts `mis` bytes in front of it)
__global__ __launch_bounds__(SO_THREADS) void k_so_emit(const uint32_t* __restrict__ R, uint32_t nw, uint32_t rb, uint64_t total, uint8_t* __restrict__ rows, uint32_t mis) {
    const uint64_t ndw = (total + mis + 3) / 4;
    for (uint64_t t = blockIdx.x * (uint64_t)SO_THREADS + threadIdx.x; t < ndw; t += (uint64_t)gridDim.x * SO_THREADS) {
        const uint64_t lo = t * 4 < mis ? 0 : t * 4 - mis;              // first byte of the array in this dword
        const uint64_t hi = min(total, t * 4 + 4 - mis);                // one past its last
        uint64_t g = lo / rb;
        uint32_t r = (uint32_t)(lo - g * rb), v = 0;
        for (uint64_t q = lo; q < hi; q++) {
            const uint32_t byte = (R[g * nw + (r >> 2)] >> (8u * (r & 3u))) & 0xFFu;
            v |= byte << (8u * (uint32_t)(q + mis - t * 4));
            if (++r == rb) {
                r = 0;
                g++;
            }
        }
        if (hi - lo == 4) *reinterpret_cast<uint32_t*>(rows + lo) = v;  // (lo + mis = 4 t: aligned)
        else
            for (uint64_t q = lo; q < hi; q++) rows[q] = (uint8_t)(v >> (8u * (uint32_t)(q + mis - t * 4)));
    }
}

__global__ __launch_bounds__(SO_THREADS) void k_so_count(const uint32_t* __restrict__ R, uint32_t nw, uint64_t ng, uint32_t L, uint32_t* __restrict__ counts) {
    const uint64_t tid = blockIdx.x * (uint64_t)SO_THREADS + threadIdx.x, nthreads = (uint64_t)gridDim.x * SO_THREADS;
    const uint32_t sub = (uint32_t)(tid & (L - 1u));
    for (uint64_t g = tid / L; g < ng; g += nthreads / L) {  // (the L lanes of a group sit in one wavefront and leave the loop together)
        uint32_t c = 0;
        for (uint32_t w = sub; w < nw; w += L) c += (uint32_t)__popc(R[g * nw + w]);
        for (uint32_t dd = L >> 1; dd >= 1; dd >>= 1) c += (uint32_t)__shfl_xor((int)c, (int)dd);
        if (sub == 0) counts[g] = c;
    }
}

dim3 so_grid(uint64_t items) { return dim3(bft_grid_for((items + SO_THREADS - 1) / SO_THREADS)); }

}  // namespace

int bft_so_reduce(const BftSoDict& d, const BftSoBatch& b, const BftSoScratch& p, hipStream_t s, int step) {
    const bool narrow = d.nw <= 2;
    const dim3 blk(SO_THREADS);
    switch (step) {
    case 0: hipLaunchKernelGGL(k_so_plan, so_grid(b.ng), blk, 0, s, d, b, p.nsplit, p.split); break;
    case 1: hipLaunchKernelGGL(k_so_small, so_grid(b.ng * d.nw), blk, 0, s, d, b); break;
    case 2:
        if (narrow) hipLaunchKernelGGL(k_so_wave<true>, so_grid(b.ng * 64), blk, 0, s, d, b);
        else hipLaunchKernelGGL(k_so_wave<false>, so_grid(b.ng * 64), blk, 0, s, d, b);
        break;
    case 3:
        if (narrow) hipLaunchKernelGGL(k_so_split<true>, dim3(SO_SPLIT_BLOCKS), blk, 0, s, d, b, (const unsigned long long*)p.nsplit, (const uint32_t*)p.split);
        else hipLaunchKernelGGL(k_so_split<false>, dim3(SO_SPLIT_BLOCKS), blk, 0, s, d, b, (const unsigned long long*)p.nsplit, (const uint32_t*)p.split);
        break;
    default: hipLaunchKernelGGL(k_so_finish, dim3(SO_FINISH_BLOCKS), blk, 0, s, d, b, (const unsigned long long*)p.nsplit, (const uint32_t*)p.split); break;
    }
    HIPCK(hipGetLastError());
    return 0;
}

int bft_so_emit(const BftSoDict& d, const uint32_t* R, uint64_t ng, uint8_t* d_rows, hipStream_t s) {
    const uint32_t rb = (d.G + 7) / 8, mis = (uint32_t)((uintptr_t)d_rows & 3u);
    const uint64_t total = ng * rb;
    if (total == 0) return 0;
    hipLaunchKernelGGL(k_so_emit, so_grid((total + mis + 3) / 4), dim3(SO_THREADS), 0, s, R, d.nw, rb, total, d_rows, mis);
    HIPCK(hipGetLastError());
    return 0;
}

int bft_so_count(const BftSoDict& d, const uint32_t* R, uint64_t ng, uint32_t* d_counts, hipStream_t s) {
    uint32_t L = 1;
    while (L < 64u && L < d.nw) L <<= 1;
    hipLaunchKernelGGL(k_so_count, so_grid(ng * L), dim3(SO_THREADS), 0, s, R, d.nw, ng, L, d_counts);
    HIPCK(hipGetLastError());
    return 0;
}

// Test hook: the constants that decide a group's class and every kernel's grid (tests/test_setops_cases_host.py derives its cases from them).
extern "C" int bft_gpu_debug_setops_plan(uint64_t out[6]) {
    if (!out) return bft_fail(BFT_GPU_E_ARG, "NULL argument");
    out[0] = BFT_SO_SMALL;
    out[1] = BFT_SO_WAVE_MAX;
    out[2] = BFT_SO_CHUNK;
    out[3] = (uint64_t)SO_SPLIT_BLOCKS * (SO_THREADS / 64);
    out[4] = (uint64_t)SO_FINISH_BLOCKS * SO_THREADS;
    out[5] = (uint64_t)bft_grid_for(~0ull) * SO_THREADS;  // (so_grid of a batch beyond the cap)
    return BFT_GPU_OK;
}

// ------------------------------------------------------------------------------------------------
// the C-ABI entry points: the handle's scratch, the chain of launches, the host-buffer forms
// ------------------------------------------------------------------------------------------------
// the arrays of a call over n looked-up k-mers (0 in the colour-set form), ng groups and rows of nw words, from `base` on; returns the block's size
static size_t so_carve(uint64_t n, uint64_t ng, uint32_t nw, bool symdiff, uint8_t* base, BftSoScratch* p) {
    Carver c{base};
    c.take(p->nsplit, 8);
    c.take(p->cs, n * 4);
    c.take(p->bits, ((n + 63) / 64) * 8);
    c.take(p->R, ng * nw * 4);
    c.take(p->X, symdiff ? ng * nw * 4 : 0);
    c.take(p->nfound, ng * 4);
    c.take(p->split, ng * 4);
    return c.off;
}

static int so_zero_u32(uint32_t* d, uint64_t n, hipStream_t s) { return d && n ? bft_zero_async(d, n * 4, s) : 0; }

// One call on stream s.  d_kmers != NULL: the k-mer form (the members are looked up first); else d_cs holds the members' colour sets.
static int so_core(bft_gpu* h, const uint8_t* d_kmers, const uint32_t* d_cs, uint64_t n, const uint64_t* d_off, uint64_t ng, int op, int skip, uint8_t* d_rows,
                   uint32_t* d_counts, uint32_t* d_found, hipStream_t s) {
    if (ng == 0 || (!d_rows && !d_counts && !d_found)) return 0;
    const uint32_t G = h->im.nb_genomes, rb = (G + 7) / 8, nw = (G + 31) / 32;
    if (G == 0 || h->n_kmers == 0 || h->n_sets == 0) {  // an index without a k-mer: every group is empty
        if (d_rows && rb) HIPCK(hipMemsetAsync(d_rows, 0, ng * rb, s));
        CK(so_zero_u32(d_counts, ng, s));
        return so_zero_u32(d_found, ng, s);
    }
    CK(bft_ensure_cs_bitmaps(h));
    HandleScratch::Lease lease(h->so);  // (the scratch's use ends with this function)
    BftSoScratch p;
    CK(lease.acquire(s, false));  // (the entry points refuse a capturing stream)
    const bool look = d_kmers != nullptr;
    CK(h->so.grow(h->so_buf, so_carve(look ? n : 0, ng, nw, op == BFT_GPU_SETOP_SYMDIFF, nullptr, &p), 0));
    so_carve(look ? n : 0, ng, nw, op == BFT_GPU_SETOP_SYMDIFF, h->so_buf.as<uint8_t>(), &p);
    BftSoDict d;
    d.bm = h->has_cs_bm ? reinterpret_cast<const uint32_t*>(h->d_cs_bm.as<uint8_t>() + CS_BM_SLACK) : nullptr;
    d.stride32 = (rb + 3) / 4;
    d.cs_off = h->d_cs_off.as<uint32_t>();
    d.cs_ids = h->d_cs_ids.p;
    d.cs_w = h->cs_w;
    d.n_sets = (uint32_t)h->n_sets;
    d.G = G;
    d.nw = nw;
    {
        StageScope stage_scope(h, s);
        if (look && n) {  // the colour set of every k-mer out of the line that answers presence ("compact_table" stays in force)
            h->im.emit_cs = 1;
            const int rc = bft_launch_query(h, d_kmers, n, p.bits, p.cs, s);
            h->im.emit_cs = 0;
            CK(rc);
            bft_stage("set operations: colour set per k-mer", (double)n * (h->B + 64 + 4), s);
        }
        const BftSoBatch b{look ? p.cs : d_cs, n, d_off, ng, op, skip, p.R, p.X, d_found ? d_found : p.nfound};
        CK(bft_zero_async(p.nsplit, 8, s));
        for (int step = 0; step < 5; step++) CK(bft_timed_launch(h, s, [&] { return bft_so_reduce(d, b, p, s, step); }));
        // (bytes: the members' ids, a dictionary row per member at most -- one per run of equal sets --, the result rows)
        bft_stage("set operations: segmented reduction", (double)n * 4 + (double)ng * 16 + (double)ng * nw * 4, s);
        if (d_rows) CK(bft_timed_launch(h, s, [&] { return bft_so_emit(d, p.R, ng, d_rows, s); }));
        if (d_counts) CK(bft_timed_launch(h, s, [&] { return bft_so_count(d, p.R, ng, d_counts, s); }));
        bft_stage("set operations: rows and counts", (double)ng * nw * 4 * ((d_rows ? 1 : 0) + (d_counts ? 1 : 0)) + (double)ng * ((d_rows ? rb : 0) + (d_counts ? 4 : 0)), s);
    }
    return 0;
}

static int so_check_op(int op) { return op >= BFT_GPU_SETOP_AND && op <= BFT_GPU_SETOP_SYMDIFF ? 0 : bft_fail(BFT_GPU_E_ARG, "set operations: op must be BFT_GPU_SETOP_AND, _OR or _SYMDIFF"); }
static int so_check_offsets(const uint64_t* off, uint64_t ng, uint64_t n) {
    for (uint64_t g = 0; g < ng; g++)
        if (off[g + 1] < off[g]) return bft_fail(BFT_GPU_E_ARG, "set operations: group offsets must not decrease");
    if (ng && off[ng] > n) return bft_fail(BFT_GPU_E_ARG, "set operations: the last group ends behind the batch");
    return 0;
}

static int so_dev(bft_gpu* h, const void* d_kmers, const void* d_cs, uint64_t n, const void* d_off, uint64_t ng, int op, int skip, void* d_rows, void* d_counts,
                  void* d_found, void* hip_stream, bool kmers) {
    if (!h || (ng && !d_off) || (n && ng && !(kmers ? d_kmers : d_cs))) return bft_fail(BFT_GPU_E_ARG, "NULL argument");
    CK(so_check_op(op));
    ENTER(h);
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : h->stream;
    if (bft_stream_capturing(s)) return bft_fail(BFT_GPU_E_ARG, "set operations recorded into a graph: not supported (scratch may grow, the dictionary's bitmaps may have to be derived)");
    CK(bft_ensure_built(h, false));
    // (a batch without k-mers: every group is empty; the lookup is skipped, the kernels see n = 0 and read no member)
    CK(so_core(h, kmers ? (n ? (const uint8_t*)d_kmers : nullptr) : nullptr, kmers ? nullptr : (const uint32_t*)d_cs, n, (const uint64_t*)d_off, ng, op, skip,
               (uint8_t*)d_rows, (uint32_t*)d_counts, (uint32_t*)d_found, s));
    return bft_note_foreign_stream(h, s);
}

extern "C" int bft_gpu_combine_colors_dev(bft_gpu* h, const void* d_kmers, uint64_t nb_kmers, const void* d_group_off, uint64_t nb_groups, int op, int skip_absent,
                                          void* d_rows, void* d_counts, void* d_found, void* hip_stream) {
    return so_dev(h, d_kmers, nullptr, nb_kmers, d_group_off, nb_groups, op, skip_absent != 0, d_rows, d_counts, d_found, hip_stream, true);
}
extern "C" int bft_gpu_combine_colorsets_dev(bft_gpu* h, const void* d_colorsets, uint64_t nb, const void* d_group_off, uint64_t nb_groups, int op, void* d_rows,
                                             void* d_counts, void* hip_stream) {
    return so_dev(h, nullptr, d_colorsets, nb, d_group_off, nb_groups, op, 0, d_rows, d_counts, nullptr, hip_stream, false);
}

// The host-buffer forms: the batch and its offsets staged whole through device blocks of the call's own, one synchronisation at the end.
static int so_host(bft_gpu* h, const uint8_t* kmers, const uint32_t* cs, uint64_t n, const uint64_t* off, uint64_t ng, int op, int skip, uint8_t* rows, uint32_t* counts,
                   uint32_t* found, bool is_kmers) {
    if (!h || (ng && !off) || (n && ng && !(is_kmers ? (const void*)kmers : (const void*)cs))) return bft_fail(BFT_GPU_E_ARG, "NULL argument");
    CK(so_check_op(op));
    CK(so_check_offsets(off, ng, n));
    ENTER(h);
    CK(bft_ensure_built(h, false));
    if (!is_kmers)
        for (uint64_t i = 0; i < n; i++)
            if (cs[i] != BFT_SO_ABSENT && cs[i] >= h->n_sets) return bft_fail(BFT_GPU_E_ARG, "set operations: a colour-set id is outside the dictionary");
    if (ng == 0 || (!rows && !counts && !found)) return BFT_GPU_OK;
    const hipStream_t s = h->stream;
    const uint32_t rb = (h->im.nb_genomes + 7) / 8;
    const size_t in_bytes = is_kmers ? (size_t)n * h->B : (size_t)n * 4;
    DevBuf din, doff, drows, dcnt, dfnd;
    CK(din.alloc(in_bytes));
    CK(doff.alloc((ng + 1) * 8));
    if (rows && rb) CK(drows.alloc(ng * rb));
    if (counts) CK(dcnt.alloc(ng * 4));
    if (found) CK(dfnd.alloc(ng * 4));
    if (in_bytes) HIPCK(hipMemcpyAsync(din.p, is_kmers ? (const void*)kmers : (const void*)cs, in_bytes, hipMemcpyHostToDevice, s));
    HIPCK(hipMemcpyAsync(doff.p, off, (ng + 1) * 8, hipMemcpyHostToDevice, s));
    CK(so_core(h, is_kmers && n ? din.as<uint8_t>() : nullptr, is_kmers ? nullptr : din.as<uint32_t>(), n, doff.as<uint64_t>(), ng, op, skip, rows && rb ? drows.as<uint8_t>() : nullptr,
               counts ? dcnt.as<uint32_t>() : nullptr, found ? dfnd.as<uint32_t>() : nullptr, s));
    if (rows && rb) HIPCK(hipMemcpyAsync(rows, drows.p, ng * rb, hipMemcpyDeviceToHost, s));
    if (counts) HIPCK(hipMemcpyAsync(counts, dcnt.p, ng * 4, hipMemcpyDeviceToHost, s));
    if (found) HIPCK(hipMemcpyAsync(found, dfnd.p, ng * 4, hipMemcpyDeviceToHost, s));
    HIPCK(hipStreamSynchronize(s));
    return BFT_GPU_OK;
}

extern "C" int bft_gpu_combine_colors(bft_gpu* h, const uint8_t* kmers, uint64_t nb_kmers, const uint64_t* group_off, uint64_t nb_groups, int op, int skip_absent,
                                      uint8_t* rows, uint32_t* counts, uint32_t* found) {
    return so_host(h, kmers, nullptr, nb_kmers, group_off, nb_groups, op, skip_absent != 0, rows, counts, found, true);
}
extern "C" int bft_gpu_combine_colorsets(bft_gpu* h, const uint32_t* colorsets, uint64_t nb, const uint64_t* group_off, uint64_t nb_groups, int op, uint8_t* rows,
                                         uint32_t* counts) {
    return so_host(h, nullptr, colorsets, nb, group_off, nb_groups, op, 0, rows, counts, nullptr, false);
}
