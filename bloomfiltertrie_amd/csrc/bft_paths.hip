// bft_paths.hip -- the path engine, and its first family: the simple paths (unitigs) of the index (extract_simple_paths / extract_simple_core_paths,
// reference snippets.h, src/snippets.c:115-603) over the sorted T-form table tk (one row per stored k-mer, rows in the bft_gpu_extract order).
// The engine serves two vertex models (bft_paths.h): the rows themselves (here), and the oriented rows 2 * row + o of a canonical index, where every
// path has a mirror and one of the two is kept (bft_unitigs.hip).  A kernel that both models run is a template over MIRRORED, a compile-time
// parameter: the row instantiation holds nothing of the mirrored one.
// The simple paths' own:
//   k_sp_degrees  one lane per row u.  The four successors x[1..k-1]+N of u lie in one interval of at most 16 rows, found by ONE lower bound
//                 (bft_for_each_successor, bft_succ.h).  Out-degree and the successor's row come from that interval; in-degrees and predecessors
//                 are the same relation read backwards, so each successor found gets an atomic increment and u's row -- no second lookup
//   k_sp_links    nodes (in <= 1, out <= 1, colour set of t genomes or more) and edges (u -> v: v is u's only successor, u is v's only
//                 predecessor, both nodes, |C(u) & C(v)| >= t; the sorted id lists are merged, equal colour-set ids skip it), each decided
//                 at both of its ends by the same predicate; the first state of the jumps
// Shared by both families (and k_sp_buckets by every unit that searches successors: components, reachability marks):
//   k_sp_buckets  first row of every bucket of the top bits of the T-form: a lower bound in tk starts inside one bucket (about 40 rows on the
//                 config-3 index) instead of the whole table
//   k_sp_jump     ceil(log2(n + 1)) rounds of pointer jumping backwards along the edges.  A lane's state covers a window of 2^r nodes ending at
//                 it: the node before the window, the window's length (steps to the head once the head is in it), the smallest vertex in the
//                 window and the steps back to it.  A chain ends with {head, distance}; a cycle, which has no head, with {smallest vertex of
//                 the cycle, distance from it}: the cycle is cut before its smallest vertex without a second pass
//   k_sp_ends     {head, distance} per node; the tail (no edge out, or the edge back to the cycle's smallest vertex) writes its path's length at
//                 the head; the longest path (an atomic from a wavefront only when it beats the counter's current value).  MIRRORED: every path
//                 occurs twice, as P and as its mirror (reversed, every vertex flipped); the tail q of a chain with head h keeps it iff
//                 h < q ^ 1, a cycle is kept where its smallest vertex is even (the (s, 0) of its smallest row), and only the tail of a kept
//                 path writes: a head with length 0 starts no reported path
//   (two scans: paths numbered by their (kept) heads in ascending vertex, BftSpHeadOf; characters placed, BftSpHeadLen)
//   k_sp_offsets  offsets[path] from the (kept) heads
//   k_sp_spell    a head writes its k nucleotides, every other node its last one at offset + k - 1 + distance.  MIRRORED: the vertices of kept
//                 paths alone, an odd vertex from the reverse complement of its row (its last nucleotide: the complement of s[0])
// and on the host the scratch (bft_sp_scratch), the chain of launches with its stages (bft_paths_trace, bft_paths_number, bft_paths_emit: also run by bft_cgraph.hip) and both forms of the entry point
// (bft_paths_dev, bft_paths_host), driven by a family's BftPathFamily.
// No kernel needs LDS or scratch memory.
#include "bft_dev.h"
#include "bft_handle.h"
#include "bft_paths.h"
#include "bft_scan.h"
#include "bft_succ.h"

namespace {

template <int W>
__global__ __launch_bounds__(BFT_LAUNCH_THREADS) void k_sp_buckets(const uint64_t* __restrict__ tk, uint32_t n, int k, int sb, uint32_t* __restrict__ start) {
    const uint32_t nb = 1u << sb;
    for (uint64_t b = blockIdx.x * (uint64_t)BFT_LAUNCH_THREADS + threadIdx.x; b <= nb; b += (uint64_t)gridDim.x * BFT_LAUNCH_THREADS) {
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
__global__ __launch_bounds__(BFT_LAUNCH_THREADS) void k_sp_degrees(const uint64_t* __restrict__ tk, uint32_t n, int k, int sb, const uint32_t* __restrict__ start,
                                                           uint32_t* __restrict__ succ, uint32_t* __restrict__ indeg, uint32_t* __restrict__ pred) {
    for (uint64_t u = blockIdx.x * (uint64_t)BFT_LAUNCH_THREADS + threadIdx.x; u < n; u += (uint64_t)gridDim.x * BFT_LAUNCH_THREADS) {
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

__global__ __launch_bounds__(BFT_LAUNCH_THREADS) void k_sp_links(uint32_t n, uint32_t t, const uint32_t* __restrict__ tcol, const uint32_t* __restrict__ cs_off,
                                                         const void* __restrict__ cs_ids, uint32_t cs_w, const uint32_t* __restrict__ succ,
                                                         const uint32_t* __restrict__ indeg, const uint32_t* __restrict__ pred, uint8_t* __restrict__ flags,
                                                         uint4* __restrict__ st) {
    for (uint64_t i0 = blockIdx.x * (uint64_t)BFT_LAUNCH_THREADS + threadIdx.x; i0 < n; i0 += (uint64_t)gridDim.x * BFT_LAUNCH_THREADS) {
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

__global__ __launch_bounds__(BFT_LAUNCH_THREADS) void k_sp_jump(uint32_t n, const uint4* __restrict__ src, uint4* __restrict__ dst) {
    for (uint64_t i = blockIdx.x * (uint64_t)BFT_LAUNCH_THREADS + threadIdx.x; i < n; i += (uint64_t)gridDim.x * BFT_LAUNCH_THREADS) {
        const uint4 a = src[i];
        if (a.y == 0u) {  // a head, a lone node or a vertex outside every path: nothing behind it
            dst[i] = a;
            continue;
        }
        const uint4 b = src[a.x];
        const bool mine = a.z <= b.z;  // (ties: the nearer occurrence)
        dst[i] = make_uint4(b.x, a.y + b.y, mine ? a.z : b.z, mine ? a.w : a.y + b.w);
    }
}

template <bool MIRRORED>
__global__ __launch_bounds__(BFT_LAUNCH_THREADS) void k_sp_ends(uint32_t n, int k, const uint4* __restrict__ st, const uint8_t* __restrict__ flags,
                                                        const uint32_t* __restrict__ succ, uint2* __restrict__ hd, uint32_t* __restrict__ len,
                                                        unsigned long long* __restrict__ longest) {
    // (every lane of a wavefront runs the same iterations: the wavefront's maximum is combined with shuffles)
    for (uint64_t i0 = blockIdx.x * (uint64_t)BFT_LAUNCH_THREADS + (threadIdx.x & ~63u); i0 < n; i0 += (uint64_t)gridDim.x * BFT_LAUNCH_THREADS) {
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
                // the mirror of a chain h .. q is q ^ 1 .. h ^ 1; a cycle and its mirror hold the two orientations of their smallest row
                const bool keep = !MIRRORED || (cyc ? (s.z & 1u) == 0u : o.x < ((uint32_t)i ^ 1u));
                if (tail && keep) {
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

// (len: read where MIRRORED alone -- a head whose path is the mirror that is not reported has length 0)
template <bool MIRRORED>
__global__ __launch_bounds__(BFT_LAUNCH_THREADS) void k_sp_offsets(uint32_t n, const uint2* __restrict__ hd, const uint32_t* __restrict__ len,
                                                           const uint32_t* __restrict__ pid, const uint64_t* __restrict__ choff, uint64_t* __restrict__ offsets,
                                                           uint64_t paths_cap, const unsigned long long* __restrict__ counts) {
    for (uint64_t i = blockIdx.x * (uint64_t)BFT_LAUNCH_THREADS + threadIdx.x; i < n; i += (uint64_t)gridDim.x * BFT_LAUNCH_THREADS) {
        if (i == 0) {
            const uint64_t np = counts[0];
            if (np <= paths_cap) offsets[np] = counts[1];
        }
        if (hd[i].x != (uint32_t)i || (MIRRORED && len[i] == 0u)) continue;
        const uint64_t p = pid[i];
        if (p <= paths_cap) offsets[p] = choff[i];
    }
}

template <int W, bool MIRRORED>
__global__ __launch_bounds__(BFT_LAUNCH_THREADS) void k_sp_spell(const uint64_t* __restrict__ tk, uint32_t n, int k, const uint2* __restrict__ hd,
                                                         const uint32_t* __restrict__ len, const uint64_t* __restrict__ choff, char* __restrict__ seqs,
                                                         uint64_t cap) {
    for (uint64_t i = blockIdx.x * (uint64_t)BFT_LAUNCH_THREADS + threadIdx.x; i < n; i += (uint64_t)gridDim.x * BFT_LAUNCH_THREADS) {
        const uint2 o = hd[i];
        if (o.x == BFT_SP_NONE || (MIRRORED && len[o.x] == 0u)) continue;  // (in no path, or in the mirror that is not reported)
        const uint64_t base = choff[o.x];
        const uint64_t row = MIRRORED ? i >> 1 : i;
        uint64_t t[W], x[W], xr[W];
        bft_load_row<W>(tk + row * W, t);
        bft_x_from_tform<W>(t, k, x);
        if (MIRRORED) bft_x_revcomp<W>(x, k, xr);
        const bool rev = MIRRORED && (i & 1u) != 0;
        int j0 = o.y ? k - 1 : 0;
        uint64_t pos = base + (o.y ? (uint64_t)(k - 1) + o.y : 0ull);
        for (int j = j0; j < k && pos < cap; j++, pos++) {
            uint64_t wv = 0;
#pragma unroll
            for (int w = 0; w < W; w++)
                if (w == (j >> 5)) wv = rev ? xr[w] : x[w];
            seqs[pos] = "ACGT"[(wv >> (2 * (j & 31))) & 3ull];
        }
    }
}

}  // namespace

int bft_sp_buckets(int W, const uint64_t* d_tk, uint64_t n, int k, const BftSpScratch& p, hipStream_t s) {
    return bft_for_w(W, [&](auto KW) { return bft_launch256(k_sp_buckets<KW>, (1ull << p.sb) + 1, s, d_tk, (uint32_t)n, k, p.sb, p.start); });
}

int bft_sp_degrees(int W, const uint64_t* d_tk, uint64_t n, int k, const BftSpScratch& p, hipStream_t s) {
    return bft_for_w(W, [&](auto KW) { return bft_launch256(k_sp_degrees<KW>, n, s, d_tk, (uint32_t)n, k, p.sb, p.start, p.succ, p.indeg, p.pred); });
}

int bft_sp_links(uint64_t n, uint32_t t, const uint32_t* d_tcol, const uint32_t* d_cs_off, const void* d_cs_ids, uint32_t cs_w, const BftSpScratch& p, hipStream_t s) {
    return bft_launch256(k_sp_links, n, s, (uint32_t)n, t, d_tcol, d_cs_off, d_cs_ids, cs_w, p.succ, p.indeg, p.pred, p.flags, p.st[0]);
}

int bft_sp_jump(uint64_t nv, const BftSpScratch& p, int from, hipStream_t s) { return bft_launch256(k_sp_jump, nv, s, (uint32_t)nv, p.st[from], p.st[from ^ 1]); }

// the final state st[fin] -> {head, steps from the head} per node (written over st[fin ^ 1] as uint2), the length of each (kept) path at its head's
// indeg[] (mirrored: zeroed by the caller), the longest (kept) path into *d_longest (zeroed by the caller)
static int sp_ends(bool mirrored, uint64_t nv, int k, const BftSpScratch& p, int fin, unsigned long long* d_longest, hipStream_t s) {
    return bft_launch256(mirrored ? k_sp_ends<true> : k_sp_ends<false>, nv, s, (uint32_t)nv, k, p.st[fin], p.flags, p.succ, reinterpret_cast<uint2*>(p.st[fin ^ 1]),
                         p.indeg, d_longest);
}
// offsets[pid] for the (kept) heads and offsets[n_paths] = n_chars (d_counts = {n_paths, n_chars}), each only where it is below paths_cap + 1
static int sp_offsets(bool mirrored, uint64_t nv, const BftSpScratch& p, int fin, uint64_t* d_offsets, uint64_t paths_cap, const unsigned long long* d_counts,
                      hipStream_t s) {
    return bft_launch256(mirrored ? k_sp_offsets<true> : k_sp_offsets<false>, nv, s, (uint32_t)nv, bft_sp_hd(p, fin), p.indeg, p.pred, p.choff, d_offsets, paths_cap,
                         d_counts);
}
// the nucleotides of every node (of a kept path), as ASCII, below chars_cap
static int sp_spell(bool mirrored, int W, const uint64_t* d_tk, uint64_t nv, int k, const BftSpScratch& p, int fin, char* d_seqs, uint64_t chars_cap, hipStream_t s) {
    if (chars_cap == 0) return 0;
    return bft_for_w(W, [&](auto KW) {
        return bft_launch256(mirrored ? k_sp_spell<KW, true> : k_sp_spell<KW, false>, nv, s, d_tk, (uint32_t)nv, k, bft_sp_hd(p, fin), p.indeg, p.choff, d_seqs,
                             chars_cap);
    });
}

// ------------------------------------------------------------------------------------------------
// the handle's scratch, the chain of launches, the two forms of the entry point: one of each for both families
// ------------------------------------------------------------------------------------------------
// the arrays of a block with room for m vertices and deg_rows degree bytes (p->sb set), from `base` on; returns the block's size (107 bytes per row
// and the bucket starts for the mirrored model).  m = 0: the bucket starts and the degree bytes alone
static size_t sp_carve(uint64_t m, uint64_t deg_rows, uint8_t* base, BftSpScratch* p) {
    Carver c{base};
    c.take(p->start, ((1ull << p->sb) + 1) * 4);
    if (deg_rows) c.take(p->deg, deg_rows);
    if (m == 0) return c.off;
    c.take(p->succ, m * 4);
    c.take(p->indeg, m * 4);
    c.take(p->pred, m * 4);
    c.take(p->flags, m);
    c.take(p->st[0], m * 16);
    c.take(p->st[1], m * 16);
    c.take(p->choff, m * 8);
    return c.off;
}
// (its own block, shared with no other query: the calls of both families are serialised on a handle, the block holds the larger)
int bft_sp_scratch(bft_gpu* h, HandleScratch::Lease& lease, uint64_t m, uint64_t nv, uint64_t deg_rows, hipStream_t s, BftSpScratch* p) {
    CK(lease.acquire(s, false));  // (the entry points refuse a capturing stream)
    *p = BftSpScratch{};
    p->sb = bft_sp_bucket_bits(h->k);
    CK(h->sp.grow(h->sp_buf, sp_carve(m, deg_rows, nullptr, p), 0));
    if (nv) CK(h->sp.grow(h->sp_tmp, bft_scan::scratch_bytes(nv + 1), 0));
    sp_carve(m, deg_rows, h->sp_buf.as<uint8_t>(), p);
    return 0;
}

int bft_sp_prepare(bft_gpu* h, const char* what) {
    CK(bft_ensure_built(h));  // ("compact_table": the sorted table comes back, as for rows and prefixes)
    if (h->n_kmers >= (1ull << 31)) return bft_fail(BFT_GPU_E_LIMIT, std::string(what) + ": at most 2^31 - 1 k-mers");  // (vertex ids stay below BFT_SP_MANY)
    return 0;
}

static uint64_t sp_vertices(const bft_gpu* h, const BftPathFamily& f) { return f.mirrored ? 2 * h->n_kmers : h->n_kmers; }
// The scratch of a call of family f.  (The arrays' places in the block are part of what a call costs -- the jumps read them at random --, so each
// family keeps its rule: the rows carve for the most rows the handle has seen, h->sp_m; the mirrored model for its 2n vertices, and a degree byte per row.)
int bft_paths_scratch(bft_gpu* h, const BftPathFamily& f, HandleScratch::Lease& lease, hipStream_t s, BftSpScratch* p) {
    const uint64_t n = h->n_kmers;
    if (f.mirrored) return bft_sp_scratch(h, lease, 2 * n, 2 * n, n, s, p);
    h->sp_m = std::max(n, h->sp_m);
    return bft_sp_scratch(h, lease, h->sp_m, n, 0, s, p);
}
// a stage named "<family>: <what>" (the name is put together only where "build_stages" is on)
static void sp_stage(const bft_gpu* h, const BftPathFamily& f, const char* what, double bytes, hipStream_t s) {
    if (h->opt_build_stages) bft_stage((std::string(f.name) + ": " + what).c_str(), bytes, s);
}

// The family's front, jumps and ends on stream s: d_counts = {., ., longest[, ...]} (f.counts_bytes, device, zeroed here); *fin: the jumps' last
// buffer.  With "build_stages" on, every step is a stage (bft_gpu_build_stages), its bytes those its algorithm reads and writes.
int bft_paths_trace(bft_gpu* h, const BftPathFamily& f, uint32_t t, hipStream_t s, unsigned long long* d_counts, const BftSpScratch& p, int* fin) {
    const uint64_t n = h->n_kmers, nv = sp_vertices(h, f);
    const double nd = (double)n, vd = (double)nv;
    CK(bft_zero_async(d_counts, f.counts_bytes, s));
    CK(bft_zero_async(p.indeg, nv * 4, s));
    CK(f.front(h, t, s, d_counts, p));
    // ceil(log2(n + 1)) rounds in both models: a path of a canonical index never holds both orientations of a row (its mirror does), so no chain or
    // cycle is longer than n vertices; nothing is read back.  (On an index that is not canonical the mirrored paths are unspecified; every index
    // stays inside the arrays.)
    int cur = 0, rounds = 0;
    for (uint64_t span = 1; span < n + 1; span <<= 1, cur ^= 1, rounds++) CK(bft_timed_launch(h, s, [&] { return bft_sp_jump(nv, p, cur, s); }));
    *fin = cur;
    sp_stage(h, f, "pointer jumping", vd * 48 * rounds, s);
    CK(bft_timed_launch(h, s, [&] { return sp_ends(f.mirrored, nv, h->k, p, cur, d_counts + 2, s); }));
    bft_stage(f.ends_stage, f.mirrored ? vd * (16 + 1 + 4 + 8) + nd * 4 : nd * (16 + 1 + 4 + 8 + 4), s);
    return 0;
}
// Both scans over what the ends left: the (kept) heads numbered in ascending vertex (pred[]), their paths placed (choff[]); d_counts[0 .. 1] =
// {n_paths, n_chars}
int bft_paths_number(bft_gpu* h, const BftPathFamily& f, hipStream_t s, unsigned long long* d_counts, const BftSpScratch& p, int fin) {
    const uint64_t n = h->n_kmers, nv = sp_vertices(h, f);
    const double nd = (double)n, vd = (double)nv;
    const uint2* hd = bft_sp_hd(p, fin);
    if (f.mirrored) CK(bft_timed_launch(h, s, [&] { return bft_scan::exclusive_sum<uint32_t>(BftSpHeadOf<true>{hd, nv, p.indeg}, p.pred, nv, s, h->sp_tmp, d_counts, false); }));
    else CK(bft_timed_launch(h, s, [&] { return bft_scan::exclusive_sum<uint32_t>(BftSpHead{hd, nv}, p.pred, nv, s, h->sp_tmp, d_counts, false); }));
    CK(bft_timed_launch(h, s, [&] { return bft_scan::exclusive_sum<uint64_t>(BftSpHeadLen{hd, p.indeg, nv}, p.choff, nv, s, h->sp_tmp, d_counts + 1, false); }));
    sp_stage(h, f, "two scans (paths, characters)", f.mirrored ? vd * (8 + 4 + 4 + 8 + 4 + 8) : nd * (8 + 4 + 8 + 4 + 8), s);
    return 0;
}
static int sp_count(bft_gpu* h, const BftPathFamily& f, uint32_t t, hipStream_t s, unsigned long long* d_counts, const BftSpScratch& p, int* fin) {
    CK(bft_paths_trace(h, f, t, s, d_counts, p, fin));
    return bft_paths_number(h, f, s, d_counts, p, *fin);
}
// offsets (paths_cap + 1 entries at most) and characters (chars_cap at most) of the paths the scans numbered and placed
int bft_paths_emit(bft_gpu* h, const BftPathFamily& f, const BftSpScratch& p, int fin, uint64_t* d_offsets, uint64_t paths_cap, char* d_seqs, uint64_t chars_cap,
            const unsigned long long* d_counts, hipStream_t s) {
    const uint64_t n = h->n_kmers, nv = sp_vertices(h, f);
    if (d_offsets) CK(bft_timed_launch(h, s, [&] { return sp_offsets(f.mirrored, nv, p, fin, d_offsets, paths_cap, d_counts, s); }));
    sp_stage(h, f, "offsets", f.mirrored ? (double)n * 2 * 12 : (double)n * 8, s);
    if (d_seqs) CK(bft_timed_launch(h, s, [&] { return sp_spell(f.mirrored, h->W, h->d_tk.as<uint64_t>(), nv, h->k, p, fin, d_seqs, chars_cap, s); }));
    sp_stage(h, f, "spelling", f.mirrored ? (double)n * 2 * (8.0 * h->W + 8 + 4 + 8 + 1) : (double)n * (8.0 * h->W + 8 + 8 + 1), s);
    return 0;
}

int bft_paths_dev(bft_gpu* h, const BftPathFamily& f, uint32_t min_shared, void* d_offsets, void* d_seqs, uint64_t paths_cap, uint64_t chars_cap, void* d_counts,
                  void* hip_stream) {
    if (!h || !d_counts) return bft_fail(BFT_GPU_E_ARG, "NULL argument");
    ENTER(h);
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : h->stream;
    if (bft_stream_capturing(s)) return bft_fail(BFT_GPU_E_ARG, f.capture_msg);
    CK(bft_sp_prepare(h, f.name));
    if (h->n_kmers == 0) {
        CK(bft_zero_async(d_counts, f.counts_bytes, s));
        if (d_offsets) CK(bft_zero_async(d_offsets, 8, s));
        return bft_note_foreign_stream(h, s);
    }
    {
        HandleScratch::Lease lease(h->sp);
        BftSpScratch p;
        CK(bft_paths_scratch(h, f, lease, s, &p));
        StageScope stage_scope(h, s);
        int fin = 0;
        CK(sp_count(h, f, min_shared, s, (unsigned long long*)d_counts, p, &fin));
        CK(bft_paths_emit(h, f, p, fin, (uint64_t*)d_offsets, paths_cap, (char*)d_seqs, chars_cap, (const unsigned long long*)d_counts, s));
    }
    return bft_note_foreign_stream(h, s);
}

// The host-buffer form: the paths are counted on the device, and the outputs filled only when the family's check passes and the caps hold them all.
int bft_paths_host(bft_gpu* h, const BftPathFamily& f, uint32_t min_shared, uint64_t* offsets, char* seqs, uint64_t paths_cap, uint64_t chars_cap,
                   uint64_t* n_paths, uint64_t* n_chars) {
    if (!h || !n_paths || !n_chars) return bft_fail(BFT_GPU_E_ARG, "NULL argument");
    ENTER(h);
    CK(bft_sp_prepare(h, f.name));
    *n_paths = *n_chars = 0;
    if (h->n_kmers == 0) {
        if (offsets) offsets[0] = 0;
        return BFT_GPU_OK;
    }
    const hipStream_t s = h->stream;
    DevBuf dcnt;
    CK(dcnt.alloc(f.counts_bytes));
    HandleScratch::Lease lease(h->sp);
    BftSpScratch p;
    CK(bft_paths_scratch(h, f, lease, s, &p));
    StageScope stage_scope(h);
    int fin = 0;
    CK(sp_count(h, f, min_shared, s, dcnt.as<unsigned long long>(), p, &fin));
    unsigned long long cnt[4] = {0, 0, 0, 0};
    HIPCK(hipMemcpyAsync(cnt, dcnt.p, f.counts_bytes, hipMemcpyDeviceToHost, s));
    HIPCK(hipStreamSynchronize(s));
    if (f.check) CK(f.check(cnt));
    *n_paths = cnt[0];
    *n_chars = cnt[1];
    if ((offsets && cnt[0] > paths_cap) || (seqs && cnt[1] > chars_cap)) return bft_fail(BFT_GPU_E_NOSPACE, f.nospace_msg);
    if (offsets || seqs) {
        DevBuf doff, dseq;
        if (offsets) CK(doff.alloc((cnt[0] + 1) * 8));
        if (seqs && cnt[1]) CK(dseq.alloc(cnt[1]));
        CK(bft_paths_emit(h, f, p, fin, offsets ? doff.as<uint64_t>() : nullptr, cnt[0], seqs ? dseq.as<char>() : nullptr, cnt[1], dcnt.as<unsigned long long>(), s));
        if (offsets) HIPCK(hipMemcpyAsync(offsets, doff.p, (cnt[0] + 1) * 8, hipMemcpyDeviceToHost, s));
        if (seqs && cnt[1]) HIPCK(hipMemcpyAsync(seqs, dseq.p, cnt[1], hipMemcpyDeviceToHost, s));
        HIPCK(hipStreamSynchronize(s));
    }
    return BFT_GPU_OK;
}

// ------------------------------------------------------------------------------------------------
// the simple paths: the row family
// ------------------------------------------------------------------------------------------------
// buckets, degrees (with the predecessors), links
static int sp_front(bft_gpu* h, uint32_t t, hipStream_t s, unsigned long long*, const BftSpScratch& p) {
    const uint64_t n = h->n_kmers;
    const int W = h->W, k = h->k;
    const uint64_t* tk = h->d_tk.as<uint64_t>();
    const double nd = (double)n, rowb = 8.0 * W;
    CK(bft_timed_launch(h, s, [&] { return bft_sp_buckets(W, tk, n, k, p, s); }));
    bft_stage("simple paths: buckets of the table", (double)((1ull << p.sb) + 1) * 4, s);
    CK(bft_timed_launch(h, s, [&] { return bft_sp_degrees(W, tk, n, k, p, s); }));
    bft_stage("simple paths: degrees and successors", nd * (2 * rowb + 4 + 4 + 12), s);
    CK(bft_timed_launch(h, s, [&] { return bft_sp_links(n, t, h->d_tcol.as<uint32_t>(), h->d_cs_off.as<uint32_t>(), h->d_cs_ids.p, h->cs_w, p, s); }));
    bft_stage("simple paths: nodes and edges", nd * (12 + 8 + (t ? 8 : 0) + 1 + 16), s);
    return 0;
}
static const BftPathFamily SP_FAMILY = {
    false,
    24,
    "simple paths",
    "simple paths: heads, tails, lengths",
    "simple paths recorded into a graph: not supported (the table may have to come back, scratch may grow)",
    "simple path buffers too small",
    sp_front,
    nullptr,
};

extern "C" int bft_gpu_simple_paths_dev(bft_gpu* h, uint32_t min_shared, void* d_offsets, void* d_seqs, uint64_t paths_cap, uint64_t chars_cap, void* d_counts,
                                        void* hip_stream) {
    return bft_paths_dev(h, SP_FAMILY, min_shared, d_offsets, d_seqs, paths_cap, chars_cap, d_counts, hip_stream);
}

extern "C" int bft_gpu_simple_paths(bft_gpu* h, uint32_t min_shared, uint64_t* offsets, char* seqs, uint64_t paths_cap, uint64_t chars_cap, uint64_t* n_paths,
                                    uint64_t* n_chars) {
    return bft_paths_host(h, SP_FAMILY, min_shared, offsets, seqs, paths_cap, chars_cap, n_paths, n_chars);
}
