// bft_paths.hip -- simple paths (unitigs) of the index (extract_simple_paths / extract_simple_core_paths, reference snippets.h, src/snippets.c:115-603)
// over the sorted T-form table tk (one row per stored k-mer, rows in the bft_gpu_extract order):
//   k_sp_buckets  first row of every bucket of the top bits of the T-form: a lower bound in tk starts inside one bucket (about 40 rows on the
//                 config-3 index) instead of the whole table
//   k_sp_degrees  one lane per row u.  The four successors x[1..k-1]+N of u lie in one interval of at most 16 rows, found by ONE lower bound
//                 (bft_for_each_successor, bft_succ.h).  Out-degree and the successor's row come from that interval; in-degrees and predecessors
//                 are the same relation read backwards, so each successor found gets an atomic increment and u's row -- no second lookup
//   k_sp_links    nodes (in <= 1, out <= 1, colour set of t genomes or more) and edges (u -> v: v is u's only successor, u is v's only
//                 predecessor, both nodes, |C(u) & C(v)| >= t; the sorted id lists are merged, equal colour-set ids skip it), each decided
//                 at both of its ends by the same predicate; the first state of the jumps
//   k_sp_jump     ceil(log2(n + 1)) rounds of pointer jumping backwards along the edges.  A lane's state covers a window of 2^r nodes ending at
//                 it: the node before the window, the window's length (steps to the head once the head is in it), the smallest row in the
//                 window and the steps back to it.  A chain ends with {head, distance}; a cycle, which has no head, with {smallest row of
//                 the cycle, distance from it}: the cycle is cut before its smallest row without a second pass
//   k_sp_ends     {head, distance} per node; the tail (no edge out, or the edge back to the cycle's smallest row) writes its path's length at
//                 the head; the longest path (an atomic from a wavefront only when it beats the counter's current value)
//   (two scans: paths numbered by their heads in row order, BftSpHead; characters placed, BftSpHeadLen)
//   k_sp_offsets  offsets[path] from the heads
//   k_sp_spell    a head writes its k nucleotides, every other node its last one at offset + k - 1 + distance
// No kernel needs LDS or scratch memory.
#include <type_traits>

#include "bft_dev.h"
#include "bft_handle.h"
#include "bft_paths.h"
#include "bft_scan.h"
#include "bft_succ.h"

namespace {

constexpr int SP_THREADS = 256;

template <int W>
__global__ __launch_bounds__(SP_THREADS) void k_sp_buckets(const uint64_t* __restrict__ tk, uint32_t n, int k, int sb, uint32_t* __restrict__ start) {
    const uint32_t nb = 1u << sb;
    for (uint64_t b = blockIdx.x * (uint64_t)SP_THREADS + threadIdx.x; b <= nb; b += (uint64_t)gridDim.x * SP_THREADS) {
        uint32_t lo = 0, hi = n;
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            uint64_t r[W];
            bft_load_row<W>(tk + (uint64_t)mid * W, r);
            if (sp_top<W>(r, k, sb) < (uint32_t)b) lo = mid + 1;
            else hi = mid;
        }
        start[b] = lo;
    }
}

template <int W>
__global__ __launch_bounds__(SP_THREADS) void k_sp_degrees(const uint64_t* __restrict__ tk, uint32_t n, int k, int sb, const uint32_t* __restrict__ start,
                                                           uint32_t* __restrict__ succ, uint32_t* __restrict__ indeg, uint32_t* __restrict__ pred) {
    for (uint64_t u = blockIdx.x * (uint64_t)SP_THREADS + threadIdx.x; u < n; u += (uint64_t)gridDim.x * SP_THREADS) {
        uint32_t cnt = 0, v = BFT_SP_NONE;
        bft_for_each_successor<W>(tk, n, k, sb, start, u, [&](uint32_t r) {
            cnt++;
            v = r;
            atomicAdd(&indeg[r], 1u);
            pred[r] = (uint32_t)u;
        });
        succ[u] = cnt == 0 ? BFT_SP_NONE : cnt == 1 ? v : BFT_SP_MANY;
    }
}

__device__ __forceinline__ bool sp_node(uint32_t i, uint32_t t, const uint32_t* succ, const uint32_t* indeg, const uint32_t* tcol, const uint32_t* cs_off) {
    return indeg[i] <= 1u && succ[i] != BFT_SP_MANY && (t == 0u || sp_set_size(cs_off, tcol[i]) >= t);
}

__global__ __launch_bounds__(SP_THREADS) void k_sp_links(uint32_t n, uint32_t t, const uint32_t* __restrict__ tcol, const uint32_t* __restrict__ cs_off,
                                                         const void* __restrict__ cs_ids, uint32_t cs_w, const uint32_t* __restrict__ succ,
                                                         const uint32_t* __restrict__ indeg, const uint32_t* __restrict__ pred, uint8_t* __restrict__ flags,
                                                         uint4* __restrict__ st) {
    for (uint64_t i0 = blockIdx.x * (uint64_t)SP_THREADS + threadIdx.x; i0 < n; i0 += (uint64_t)gridDim.x * SP_THREADS) {
        const uint32_t i = (uint32_t)i0;
        uint32_t f = 0, back = i;
        if (sp_node(i, t, succ, indeg, tcol, cs_off)) {
            f = BFT_SP_NODE;
            const uint32_t v = succ[i];
            if (v < n && v != i && sp_node(v, t, succ, indeg, tcol, cs_off) && sp_shared(tcol[i], tcol[v], t, cs_off, cs_ids, cs_w)) f |= BFT_SP_OUT;
            // (pred[] is written only where a successor was found; with indeg 1 it is the one predecessor, and succ[u] == i says i is u's only successor)
            const uint32_t u = indeg[i] == 1u ? pred[i] : i;
            if (u != i && succ[u] == i && sp_node(u, t, succ, indeg, tcol, cs_off) && sp_shared(tcol[u], tcol[i], t, cs_off, cs_ids, cs_w)) {
                f |= BFT_SP_IN;
                back = u;
            }
        }
        flags[i] = (uint8_t)f;
        st[i] = make_uint4(back, back != i ? 1u : 0u, i, 0u);
    }
}

__global__ __launch_bounds__(SP_THREADS) void k_sp_jump(uint32_t n, const uint4* __restrict__ src, uint4* __restrict__ dst) {
    for (uint64_t i = blockIdx.x * (uint64_t)SP_THREADS + threadIdx.x; i < n; i += (uint64_t)gridDim.x * SP_THREADS) {
        const uint4 a = src[i];
        if (a.y == 0u) {  // a head, a lone node or a row outside every path: nothing behind it
            dst[i] = a;
            continue;
        }
        const uint4 b = src[a.x];
        const bool mine = a.z <= b.z;  // (ties: the nearer occurrence)
        dst[i] = make_uint4(b.x, a.y + b.y, mine ? a.z : b.z, mine ? a.w : a.y + b.w);
    }
}

__global__ __launch_bounds__(SP_THREADS) void k_sp_ends(uint32_t n, int k, const uint4* __restrict__ st, const uint8_t* __restrict__ flags,
                                                        const uint32_t* __restrict__ succ, uint2* __restrict__ hd, uint32_t* __restrict__ len,
                                                        unsigned long long* __restrict__ longest) {
    // (every lane of a wavefront runs the same iterations: the wavefront's maximum is combined with shuffles)
    for (uint64_t i0 = blockIdx.x * (uint64_t)SP_THREADS + (threadIdx.x & ~63u); i0 < n; i0 += (uint64_t)gridDim.x * SP_THREADS) {
        const uint64_t i = i0 + (threadIdx.x & 63u);
        uint32_t mx = 0;
        if (i < n) {
            const uint32_t f = flags[i];
            uint2 o = make_uint2(BFT_SP_NONE, 0u);
            if (f & BFT_SP_NODE) {
                const uint4 s = st[i];
                const bool cyc = (flags[s.x] & BFT_SP_IN) != 0;  // (the end of a chain's jumps is its head, which no edge enters)
                o = cyc ? make_uint2(s.z, s.w) : make_uint2(s.x, s.y);
                const bool tail = cyc ? succ[i] == s.z : !(f & BFT_SP_OUT);
                if (tail) {
                    len[o.x] = (uint32_t)k + o.y;
                    mx = (uint32_t)k + o.y;
                }
            }
            hd[i] = o;
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, d));
        // (only a wavefront that beats what the counter already holds takes the atomic: one per wavefront serialises on the one address,
        // 7.4 ms for the 7x10^5 wavefronts of the config-3 index)
        if ((threadIdx.x & 63u) == 0 && mx && mx > __hip_atomic_load(longest, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(longest, (unsigned long long)mx);
    }
}

__global__ __launch_bounds__(SP_THREADS) void k_sp_offsets(uint32_t n, const uint2* __restrict__ hd, const uint32_t* __restrict__ pid,
                                                           const uint64_t* __restrict__ choff, uint64_t* __restrict__ offsets, uint64_t paths_cap,
                                                           const unsigned long long* __restrict__ counts) {
    for (uint64_t i = blockIdx.x * (uint64_t)SP_THREADS + threadIdx.x; i < n; i += (uint64_t)gridDim.x * SP_THREADS) {
        if (i == 0) {
            const uint64_t np = counts[0];
            if (np <= paths_cap) offsets[np] = counts[1];
        }
        if (hd[i].x != (uint32_t)i) continue;
        const uint64_t p = pid[i];
        if (p <= paths_cap) offsets[p] = choff[i];
    }
}

template <int W>
__global__ __launch_bounds__(SP_THREADS) void k_sp_spell(const uint64_t* __restrict__ tk, uint32_t n, int k, const uint2* __restrict__ hd,
                                                         const uint64_t* __restrict__ choff, char* __restrict__ seqs, uint64_t cap) {
    for (uint64_t i = blockIdx.x * (uint64_t)SP_THREADS + threadIdx.x; i < n; i += (uint64_t)gridDim.x * SP_THREADS) {
        const uint2 o = hd[i];
        if (o.x == BFT_SP_NONE) continue;
        const uint64_t base = choff[o.x];
        uint64_t t[W], x[W];
        bft_load_row<W>(tk + i * W, t);
        bft_x_from_tform<W>(t, k, x);
        int j0 = o.y ? k - 1 : 0;
        uint64_t pos = base + (o.y ? (uint64_t)(k - 1) + o.y : 0ull);
        for (int j = j0; j < k && pos < cap; j++, pos++) {
            uint64_t wv = 0;
#pragma unroll
            for (int w = 0; w < W; w++)
                if (w == (j >> 5)) wv = x[w];
            seqs[pos] = "ACGT"[(wv >> (2 * (j & 31))) & 3ull];
        }
    }
}

template <class F>
int sp_dispatch(int W, F&& f) {
    switch (W) {
    case 1: f(std::integral_constant<int, 1>()); break;
    case 2: f(std::integral_constant<int, 2>()); break;
    case 3: f(std::integral_constant<int, 3>()); break;
    default: f(std::integral_constant<int, 4>()); break;
    }
    HIPCK(hipGetLastError());
    return 0;
}
dim3 sp_grid(uint64_t n) { return dim3(bft_grid_for((n + SP_THREADS - 1) / SP_THREADS)); }

}  // namespace

int bft_sp_buckets(int W, const uint64_t* d_tk, uint64_t n, int k, const BftSpScratch& p, hipStream_t s) {
    const uint64_t nb = (1ull << p.sb) + 1;
    return sp_dispatch(W, [&](auto KW) { hipLaunchKernelGGL((k_sp_buckets<KW>), sp_grid(nb), dim3(SP_THREADS), 0, s, d_tk, (uint32_t)n, k, p.sb, p.start); });
}

int bft_sp_degrees(int W, const uint64_t* d_tk, uint64_t n, int k, const BftSpScratch& p, hipStream_t s) {
    if (n == 0) return 0;
    return sp_dispatch(W, [&](auto KW) {
        hipLaunchKernelGGL((k_sp_degrees<KW>), sp_grid(n), dim3(SP_THREADS), 0, s, d_tk, (uint32_t)n, k, p.sb, p.start, p.succ, p.indeg, p.pred);
    });
}

int bft_sp_links(uint64_t n, uint32_t t, const uint32_t* d_tcol, const uint32_t* d_cs_off, const void* d_cs_ids, uint32_t cs_w, const BftSpScratch& p, hipStream_t s) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_sp_links, sp_grid(n), dim3(SP_THREADS), 0, s, (uint32_t)n, t, d_tcol, d_cs_off, d_cs_ids, cs_w, p.succ, p.indeg, p.pred, p.flags, p.st[0]);
    HIPCK(hipGetLastError());
    return 0;
}

int bft_sp_jump(uint64_t n, const BftSpScratch& p, int from, hipStream_t s) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_sp_jump, sp_grid(n), dim3(SP_THREADS), 0, s, (uint32_t)n, p.st[from], p.st[from ^ 1]);
    HIPCK(hipGetLastError());
    return 0;
}

int bft_sp_ends(uint64_t n, int k, const BftSpScratch& p, int fin, unsigned long long* d_longest, hipStream_t s) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_sp_ends, sp_grid(n), dim3(SP_THREADS), 0, s, (uint32_t)n, k, p.st[fin], p.flags, p.succ, reinterpret_cast<uint2*>(p.st[fin ^ 1]), p.indeg,
                       d_longest);
    HIPCK(hipGetLastError());
    return 0;
}

int bft_sp_offsets(uint64_t n, const BftSpScratch& p, int fin, uint64_t* d_offsets, uint64_t paths_cap, const unsigned long long* d_counts, hipStream_t s) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_sp_offsets, sp_grid(n), dim3(SP_THREADS), 0, s, (uint32_t)n, bft_sp_hd(p, fin), p.pred, p.choff, d_offsets, paths_cap, d_counts);
    HIPCK(hipGetLastError());
    return 0;
}

int bft_sp_spell(int W, const uint64_t* d_tk, uint64_t n, int k, const BftSpScratch& p, int fin, char* d_seqs, uint64_t chars_cap, hipStream_t s) {
    if (n == 0 || chars_cap == 0) return 0;
    return sp_dispatch(W, [&](auto KW) {
        hipLaunchKernelGGL((k_sp_spell<KW>), sp_grid(n), dim3(SP_THREADS), 0, s, d_tk, (uint32_t)n, k, bft_sp_hd(p, fin), p.choff, d_seqs, chars_cap);
    });
}

// ------------------------------------------------------------------------------------------------
// the C-ABI entry points: the handle's scratch, the chain of launches, the host-buffer form
// ------------------------------------------------------------------------------------------------
// the arrays of a block with room for m rows (p->sb set), from `base` on; returns the block's size
static size_t sp_carve(uint64_t m, uint8_t* base, BftSpScratch* p) {
    Carver c{base};
    c.take(p->start, ((1ull << p->sb) + 1) * 4);
    c.take(p->succ, m * 4);
    c.take(p->indeg, m * 4);
    c.take(p->pred, m * 4);
    c.take(p->flags, m);
    c.take(p->st[0], m * 16);
    c.take(p->st[1], m * 16);
    c.take(p->choff, m * 8);
    return c.off;
}
// The handle's scratch (h->sp: HandleScratch, bft_handle.h) for an index of n rows on stream s: its own block, shared with no other query, sized exactly.
static int sp_scratch(bft_gpu* h, uint64_t n, hipStream_t s, BftSpScratch* p) {
    CK(h->sp.acquire(s, false));  // (the entry points refuse a capturing stream)
    p->sb = bft_sp_bucket_bits(h->k);
    h->sp_m = std::max(n, h->sp_m);
    CK(h->sp.grow(h->sp_buf, sp_carve(h->sp_m, nullptr, p), 0));
    CK(h->sp.grow(h->sp_tmp, bft_scan::scratch_bytes(n + 1), 0));
    sp_carve(h->sp_m, h->sp_buf.as<uint8_t>(), p);
    return 0;
}
// Degrees, links, ranks, lengths and both scans on stream s: d_counts = {n_paths, n_chars, longest} (24 bytes, device); *fin: the jumps' last buffer.
// With "build_stages" on, every step is a stage (bft_gpu_build_stages), its bytes those its algorithm reads and writes.
static int sp_count(bft_gpu* h, uint32_t t, hipStream_t s, unsigned long long* d_counts, const BftSpScratch& p, int* fin) {
    const uint64_t n = h->n_kmers;
    const int W = h->W, k = h->k;
    const uint64_t* tk = h->d_tk.as<uint64_t>();
    const double nd = (double)n, rowb = 8.0 * W;
    CK(bft_zero_async(d_counts, 24, s));
    CK(bft_zero_async(p.indeg, n * 4, s));
    CK(bft_timed_launch(h, s, [&] { return bft_sp_buckets(W, tk, n, k, p, s); }));
    bft_stage("simple paths: buckets of the table", (double)((1ull << p.sb) + 1) * 4, s);
    CK(bft_timed_launch(h, s, [&] { return bft_sp_degrees(W, tk, n, k, p, s); }));
    bft_stage("simple paths: degrees and successors", nd * (2 * rowb + 4 + 4 + 12), s);
    CK(bft_timed_launch(h, s, [&] { return bft_sp_links(n, t, h->d_tcol.as<uint32_t>(), h->d_cs_off.as<uint32_t>(), h->d_cs_ids.p, h->cs_w, p, s); }));
    bft_stage("simple paths: nodes and edges", nd * (12 + 8 + (t ? 8 : 0) + 1 + 16), s);
    int cur = 0, rounds = 0;  // (ceil(log2(n + 1)) of them: no chain is longer than n, nothing is read back)
    for (uint64_t span = 1; span < n + 1; span <<= 1, cur ^= 1, rounds++) CK(bft_timed_launch(h, s, [&] { return bft_sp_jump(n, p, cur, s); }));
    *fin = cur;
    bft_stage("simple paths: pointer jumping", nd * 48 * rounds, s);
    CK(bft_timed_launch(h, s, [&] { return bft_sp_ends(n, k, p, cur, d_counts + 2, s); }));
    bft_stage("simple paths: heads, tails, lengths", nd * (16 + 1 + 4 + 8 + 4), s);
    const uint2* hd = bft_sp_hd(p, cur);
    CK(bft_timed_launch(h, s, [&] { return bft_scan::exclusive_sum<uint32_t>(BftSpHead{hd, n}, p.pred, n, s, h->sp_tmp, d_counts, false); }));
    CK(bft_timed_launch(h, s, [&] { return bft_scan::exclusive_sum<uint64_t>(BftSpHeadLen{hd, p.indeg, n}, p.choff, n, s, h->sp_tmp, d_counts + 1, false); }));
    bft_stage("simple paths: two scans (paths, characters)", nd * (8 + 4 + 8 + 4 + 8), s);
    return 0;
}
// offsets (paths_cap + 1 entries at most) and characters (chars_cap at most) of the paths sp_count counted
static int sp_emit(bft_gpu* h, const BftSpScratch& p, int fin, uint64_t* d_offsets, uint64_t paths_cap, char* d_seqs, uint64_t chars_cap,
                   const unsigned long long* d_counts, hipStream_t s) {
    const uint64_t n = h->n_kmers;
    if (d_offsets) CK(bft_timed_launch(h, s, [&] { return bft_sp_offsets(n, p, fin, d_offsets, paths_cap, d_counts, s); }));
    bft_stage("simple paths: offsets", (double)n * 8, s);
    if (d_seqs) CK(bft_timed_launch(h, s, [&] { return bft_sp_spell(h->W, h->d_tk.as<uint64_t>(), n, h->k, p, fin, d_seqs, chars_cap, s); }));
    bft_stage("simple paths: spelling", (double)n * (8.0 * h->W + 8 + 8 + 1), s);
    return 0;
}
static int sp_prepare(bft_gpu* h) {
    CK(bft_ensure_built(h));  // ("compact_table": the sorted table comes back, as for rows and prefixes)
    if (h->n_kmers >= (1ull << 31)) return bft_fail(BFT_GPU_E_LIMIT, "simple paths: at most 2^31 - 1 k-mers");
    return 0;
}

extern "C" int bft_gpu_simple_paths_dev(bft_gpu* h, uint32_t min_shared, void* d_offsets, void* d_seqs, uint64_t paths_cap, uint64_t chars_cap, void* d_counts,
                                        void* hip_stream) {
    if (!h || !d_counts) return bft_fail(BFT_GPU_E_ARG, "NULL argument");
    ENTER(h);
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : h->stream;
    if (bft_stream_capturing(s)) return bft_fail(BFT_GPU_E_ARG, "simple paths recorded into a graph: not supported (the table may have to come back, scratch may grow)");
    CK(sp_prepare(h));
    if (h->n_kmers == 0) {
        CK(bft_zero_async(d_counts, 24, s));
        if (d_offsets) CK(bft_zero_async(d_offsets, 8, s));
        return bft_note_foreign_stream(h, s);
    }
    BftSpScratch p;
    CK(sp_scratch(h, h->n_kmers, s, &p));
    {
        StageScope stage_scope(h, s);
        int fin = 0;
        CK(sp_count(h, min_shared, s, (unsigned long long*)d_counts, p, &fin));
        CK(sp_emit(h, p, fin, (uint64_t*)d_offsets, paths_cap, (char*)d_seqs, chars_cap, (const unsigned long long*)d_counts, s));
    }
    h->sp.release();
    return bft_note_foreign_stream(h, s);
}

// The host-buffer form: the paths are counted on the device, and the outputs filled only when the caps hold them all.
extern "C" int bft_gpu_simple_paths(bft_gpu* h, uint32_t min_shared, uint64_t* offsets, char* seqs, uint64_t paths_cap, uint64_t chars_cap, uint64_t* n_paths,
                                    uint64_t* n_chars) {
    if (!h || !n_paths || !n_chars) return bft_fail(BFT_GPU_E_ARG, "NULL argument");
    ENTER(h);
    CK(sp_prepare(h));
    *n_paths = *n_chars = 0;
    if (h->n_kmers == 0) {
        if (offsets) offsets[0] = 0;
        return BFT_GPU_OK;
    }
    const hipStream_t s = h->stream;
    DevBuf dcnt;
    CK(dcnt.alloc(24));
    BftSpScratch p;
    CK(sp_scratch(h, h->n_kmers, s, &p));
    StageScope stage_scope(h);
    int fin = 0;
    CK(sp_count(h, min_shared, s, dcnt.as<unsigned long long>(), p, &fin));
    unsigned long long cnt[3] = {0, 0, 0};
    HIPCK(hipMemcpyAsync(cnt, dcnt.p, 24, hipMemcpyDeviceToHost, s));
    HIPCK(hipStreamSynchronize(s));
    *n_paths = cnt[0];
    *n_chars = cnt[1];
    if ((offsets && cnt[0] > paths_cap) || (seqs && cnt[1] > chars_cap)) {
        h->sp.release();
        return bft_fail(BFT_GPU_E_NOSPACE, "simple path buffers too small");
    }
    if (offsets || seqs) {
        DevBuf doff, dseq;
        if (offsets) CK(doff.alloc((cnt[0] + 1) * 8));
        if (seqs && cnt[1]) CK(dseq.alloc(cnt[1]));
        CK(sp_emit(h, p, fin, offsets ? doff.as<uint64_t>() : nullptr, cnt[0], seqs ? dseq.as<char>() : nullptr, cnt[1], dcnt.as<unsigned long long>(), s));
        if (offsets) HIPCK(hipMemcpyAsync(offsets, doff.p, (cnt[0] + 1) * 8, hipMemcpyDeviceToHost, s));
        if (seqs && cnt[1]) HIPCK(hipMemcpyAsync(seqs, dseq.p, cnt[1], hipMemcpyDeviceToHost, s));
        HIPCK(hipStreamSynchronize(s));
    }
    h->sp.release();
    return BFT_GPU_OK;
}
