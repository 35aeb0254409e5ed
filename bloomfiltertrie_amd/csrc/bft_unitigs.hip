// bft_unitigs.hip -- canonical (bidirected) unitigs and degrees: the compacted de Bruijn graph of an index that stores the smaller of each k-mer and
// its reverse complement (bft_gpu_insert_sequences(..., canonical = 1)), over the sorted T-form table tk.  include/bft_gpu.h defines the paths; an
// oriented vertex is v = 2 * row + o with word s (o = 0) or rc(s) (o = 1), its flip v ^ 1.
//   k_ug_canon    rows with s > rc(s): the call is defined where there is none
//   k_ug_degrees  one lane per row, both orientations.  The successor words w[1..k-1]+N of an orientation are represented by a stored y or a stored
//                 rc(y).  The four y lie in one interval of the table (ONE lower bound inside a bucket, as bft_for_each_successor); the four rc(y) =
//                 comp(N) + rc(w)[0..k-2] differ in the FIRST nucleotide and lie in four buckets: one bucketed lower bound each, and only for the N
//                 that the interval did not hold -- so a word counts once, a palindromic y too.  (A scatter from the interval, as k_sp_degrees finds
//                 its predecessors, learns only half of them here -- a hit (u,o) -> (r,0) says (r,1) -> (u,1-o), never what follows (r,0) as a
//                 reverse complement -- and needs an atomic mask per vertex to count words once: searched instead, no atomics, same answer every run.)
//                 A palindrome has one orientation: searched once.
//   k_ug_links    one lane per vertex: nodes (out(v) <= 1, out(v ^ 1) <= 1, colour set of t genomes or more) and edges (u -> v: v is u's only
//                 successor, u ^ 1 is (v ^ 1)'s, both nodes, two rows, no palindrome, |C(u) & C(v)| >= t), each decided at both of its ends and in
//                 both mirrors by the same predicate; the vertex before v is the flip of (v ^ 1)'s successor: no predecessor array.  The first
//                 state of the jumps
//   (bft_sp_jump, bft_paths.h, over the 2n vertices)
//   k_ug_ends     {head, distance} per node vertex.  Every path occurs twice, as P and as its mirror (reversed, every vertex flipped); the tail q of
//                 a chain with head h keeps it iff h < q ^ 1, a cycle is kept where its smallest vertex is even (the (s, 0) of its smallest row).
//                 The tail of a kept path writes the length at its head: a head with length 0 starts no reported path
//   (two scans over kept heads: paths numbered in ascending id of their first vertex, characters placed)
//   k_ug_offsets  offsets[path] from the kept heads
//   k_ug_spell    a kept head writes the k nucleotides of its word, every other vertex of a kept path its word's last one ((s,1): the complement
//                 of s[0]) at offset + k - 1 + distance
// No kernel needs LDS or scratch memory.
#include <type_traits>

#include "bft_dev.h"
#include "bft_handle.h"
#include "bft_kernels_seqwin.h"
#include "bft_scan.h"
#include "bft_succ.h"
#include "bft_unitigs.h"

namespace {

constexpr int UG_THREADS = 256;

// reverse complement of the k nucleotides of x (nucleotide j at bits 2j; the bits above 2k are zero on both sides)
template <int W>
__device__ __forceinline__ void ug_rc(const uint64_t* x, int k, uint64_t* xr) {
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
// a <=> b by nucleotide, A < C < G < T, first nucleotide first (the rule of seq_window): the lowest differing field decides
template <int W>
__device__ __forceinline__ int ug_cmp(const uint64_t* a, const uint64_t* b) {
    int r = 0;
#pragma unroll
    for (int q = W - 1; q >= 0; q--) {
        const uint64_t df = a[q] ^ b[q];
        if (df) {
            const int fs = __builtin_ctzll(df) & ~1;
            r = ((a[q] >> fs) & 3ull) < ((b[q] >> fs) & 3ull) ? -1 : 1;
        }
    }
    return r;
}
// the stored k-mer of row u and its reverse complement; returns s <=> rc(s)
template <int W>
__device__ __forceinline__ int ug_row(const uint64_t* __restrict__ tk, uint64_t u, int k, uint64_t* x, uint64_t* xr) {
    uint64_t t[W];
    bft_load_row<W>(tk + u * W, t);
    bft_x_from_tform<W>(t, k, x);
    ug_rc<W>(x, k, xr);
    return ug_cmp<W>(x, xr);
}

// the row that holds x, or BFT_SP_NONE: a lower bound inside the bucket of its T-form
template <int W>
__device__ __forceinline__ uint32_t ug_find(const uint64_t* __restrict__ tk, int k, int sb, const uint32_t* __restrict__ start, const uint64_t* x) {
    uint64_t t[W], c[W];
    bft_tform_from_x<W>(x, k, t);
    const uint32_t b = sp_top<W>(t, k, sb), lo = start[b], hi = start[b + 1];
    const uint32_t r = lo + bft_rows_lower_bound<W>(tk + (uint64_t)lo * W, hi - lo, t);
    if (r >= hi) return BFT_SP_NONE;
    bft_load_row<W>(tk + (uint64_t)r * W, c);
    return bft_cmp<W>(c, t) == 0 ? r : BFT_SP_NONE;
}

// succ[] of the vertex with word w: its represented successor words counted once each; the vertex of the only one
template <int W>
__device__ __forceinline__ uint32_t ug_successors(const uint64_t* __restrict__ tk, uint32_t n, int k, int sb, const uint32_t* __restrict__ start,
                                                  const uint64_t* w, uint32_t* out) {
    const int vo = (k % 9) ? 0 : 2;  // where the last nucleotide sits in the T-form's last word (bft_succ.h)
    const uint64_t wild = 3ull << vo;
    uint64_t y[W], t[W], z[W];
    // the successor word with nucleotide A last (the bits above 2k are zero)
#pragma unroll
    for (int q = 0; q < W; q++) y[q] = (w[q] >> 2) | (q + 1 < W ? w[q + 1] << 62 : 0ull);
    bft_tform_from_x<W>(y, k, t);
    const uint32_t b = sp_top<W>(t, k, sb), lo = start[b], hi = start[b + 1];
    uint32_t cnt = 0, v = BFT_SP_NONE, have = 0;
    for (uint32_t r = lo + bft_rows_lower_bound<W>(tk + (uint64_t)lo * W, hi - lo, t); r < n; r++) {
        uint64_t c[W];
        bft_load_row<W>(tk + (uint64_t)r * W, c);
        bool same = true;
#pragma unroll
        for (int q = 0; q < W - 1; q++) same = same && c[q] == t[q];
        if (!same || c[W - 1] > (t[W - 1] | wild)) break;
        if ((c[W - 1] & ~wild) != t[W - 1]) continue;
        have |= 1u << (uint32_t)((c[W - 1] >> vo) & 3ull);  // (the last nucleotide's code, whichever the layout)
        cnt++;
        v = 2u * r;
    }
    // rc of that word: T + rc(w)[0..k-2]; with N last, comp(N) comes first
    ug_rc<W>(y, k, z);
    for (uint32_t c = 0; c < 4; c++) {
        if ((have >> c) & 1u) continue;
        z[0] = (z[0] & ~3ull) | (uint64_t)(3u - c);
        const uint32_t r = ug_find<W>(tk, k, sb, start, z);
        if (r == BFT_SP_NONE) continue;
        cnt++;
        v = 2u * r + 1u;
    }
    *out = cnt;
    return cnt == 0 ? BFT_SP_NONE : cnt == 1 ? v : BFT_SP_MANY;
}

template <int W>
__global__ __launch_bounds__(UG_THREADS) void k_ug_canon(const uint64_t* __restrict__ tk, uint32_t n, int k, unsigned long long* __restrict__ bad) {
    // (every lane of a wavefront runs the same iterations: the wavefront's count is one ballot)
    for (uint64_t i0 = blockIdx.x * (uint64_t)UG_THREADS + (threadIdx.x & ~63u); i0 < n; i0 += (uint64_t)gridDim.x * UG_THREADS) {
        const uint64_t i = i0 + (threadIdx.x & 63u);
        bool gt = false;
        if (i < n) {
            uint64_t x[W], xr[W];
            gt = ug_row<W>(tk, i, k, x, xr) > 0;
        }
        const unsigned long long m = __ballot(gt);
        if ((threadIdx.x & 63u) == 0 && m) atomicAdd(bad, (unsigned long long)__popcll(m));  // (none on a canonical index)
    }
}

template <int W>
__global__ __launch_bounds__(UG_THREADS) void k_ug_degrees(const uint64_t* __restrict__ tk, uint32_t n, int k, int sb, const uint32_t* __restrict__ start,
                                                           uint8_t* __restrict__ deg, uint64_t deg_cap, uint32_t pal_bit, uint32_t* __restrict__ succ) {
    for (uint64_t u = blockIdx.x * (uint64_t)UG_THREADS + threadIdx.x; u < n; u += (uint64_t)gridDim.x * UG_THREADS) {
        uint64_t x[W], xr[W];
        const bool pal = ug_row<W>(tk, u, k, x, xr) == 0;
        uint32_t o0 = 0, o1 = 0;
        const uint32_t s0 = ug_successors<W>(tk, n, k, sb, start, x, &o0);
        uint32_t s1 = s0;
        if (pal) o1 = o0;
        else s1 = ug_successors<W>(tk, n, k, sb, start, xr, &o1);
        if (u < deg_cap) deg[u] = (uint8_t)(o0 << 4 | o1 | (pal ? pal_bit : 0u));
        if (succ) *reinterpret_cast<uint2*>(succ + 2 * u) = make_uint2(s0, s1);
    }
}

__device__ __forceinline__ bool ug_node(uint32_t row, uint32_t t, const uint8_t* deg, const uint32_t* tcol, const uint32_t* cs_off) {
    const uint32_t d = deg[row];
    return ((d >> 4) & 7u) <= 1u && (d & 7u) <= 1u && (t == 0u || sp_set_size(cs_off, tcol[row]) >= t);
}
// the edge u -> v, for u whose only successor is v
__device__ __forceinline__ bool ug_edge(uint32_t u, uint32_t v, uint32_t t, const uint32_t* succ, const uint8_t* deg, const uint32_t* tcol, const uint32_t* cs_off,
                                        const void* cs_ids, uint32_t cs_w) {
    const uint32_t ru = u >> 1, rv = v >> 1;
    if (ru == rv || succ[v ^ 1u] != (u ^ 1u)) return false;  // (a self-loop or a hairpin; the mirror must agree)
    if ((deg[ru] | deg[rv]) & BFT_UG_PAL) return false;
    return ug_node(ru, t, deg, tcol, cs_off) && ug_node(rv, t, deg, tcol, cs_off) && sp_shared(tcol[ru], tcol[rv], t, cs_off, cs_ids, cs_w);
}

__global__ __launch_bounds__(UG_THREADS) void k_ug_links(uint32_t n2, uint32_t t, const uint32_t* __restrict__ tcol, const uint32_t* __restrict__ cs_off,
                                                         const void* __restrict__ cs_ids, uint32_t cs_w, const uint32_t* __restrict__ succ,
                                                         const uint8_t* __restrict__ deg, uint8_t* __restrict__ flags, uint4* __restrict__ st) {
    for (uint64_t i0 = blockIdx.x * (uint64_t)UG_THREADS + threadIdx.x; i0 < n2; i0 += (uint64_t)gridDim.x * UG_THREADS) {
        const uint32_t i = (uint32_t)i0;
        uint32_t f = 0, back = i;
        if (ug_node(i >> 1, t, deg, tcol, cs_off)) {
            f = BFT_SP_NODE;
            const uint32_t v = succ[i];
            if (v < n2 && ug_edge(i, v, t, succ, deg, tcol, cs_off, cs_ids, cs_w)) f |= BFT_SP_OUT;
            // (the vertex before i: the flip of the only successor of i's flip -- and i must be its only successor)
            const uint32_t fv = succ[i ^ 1u];
            if (fv < n2 && succ[fv ^ 1u] == i && ug_edge(fv ^ 1u, i, t, succ, deg, tcol, cs_off, cs_ids, cs_w)) {
                f |= BFT_SP_IN;
                back = fv ^ 1u;
            }
        }
        flags[i] = (uint8_t)f;
        st[i] = make_uint4(back, back != i ? 1u : 0u, i, 0u);
    }
}

__global__ __launch_bounds__(UG_THREADS) void k_ug_ends(uint32_t n2, int k, const uint4* __restrict__ st, const uint8_t* __restrict__ flags,
                                                        const uint32_t* __restrict__ succ, uint2* __restrict__ hd, uint32_t* __restrict__ len,
                                                        unsigned long long* __restrict__ longest) {
    // (every lane of a wavefront runs the same iterations: the wavefront's maximum is combined with shuffles)
    for (uint64_t i0 = blockIdx.x * (uint64_t)UG_THREADS + (threadIdx.x & ~63u); i0 < n2; i0 += (uint64_t)gridDim.x * UG_THREADS) {
        const uint64_t i = i0 + (threadIdx.x & 63u);
        uint32_t mx = 0;
        if (i < n2) {
            const uint32_t f = flags[i];
            uint2 o = make_uint2(BFT_SP_NONE, 0u);
            if (f & BFT_SP_NODE) {
                const uint4 s = st[i];
                const bool cyc = (flags[s.x] & BFT_SP_IN) != 0;  // (the end of a chain's jumps is its head, which no edge enters)
                o = cyc ? make_uint2(s.z, s.w) : make_uint2(s.x, s.y);
                const bool tail = cyc ? succ[i] == s.z : !(f & BFT_SP_OUT);
                // the mirror of a chain h .. q is q ^ 1 .. h ^ 1; a cycle and its mirror hold the two orientations of their smallest row
                const bool keep = cyc ? (s.z & 1u) == 0u : o.x < ((uint32_t)i ^ 1u);
                if (tail && keep) {
                    len[o.x] = (uint32_t)k + o.y;
                    mx = (uint32_t)k + o.y;
                }
            }
            hd[i] = o;
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, d));
        // (only a wavefront that beats what the counter already holds takes the atomic, as k_sp_ends)
        if ((threadIdx.x & 63u) == 0 && mx && mx > __hip_atomic_load(longest, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(longest, (unsigned long long)mx);
    }
}

__global__ __launch_bounds__(UG_THREADS) void k_ug_offsets(uint32_t n2, const uint2* __restrict__ hd, const uint32_t* __restrict__ len,
                                                           const uint32_t* __restrict__ pid, const uint64_t* __restrict__ choff, uint64_t* __restrict__ offsets,
                                                           uint64_t paths_cap, const unsigned long long* __restrict__ counts) {
    for (uint64_t i = blockIdx.x * (uint64_t)UG_THREADS + threadIdx.x; i < n2; i += (uint64_t)gridDim.x * UG_THREADS) {
        if (i == 0) {
            const uint64_t np = counts[0];
            if (np <= paths_cap) offsets[np] = counts[1];
        }
        if (hd[i].x != (uint32_t)i || len[i] == 0u) continue;
        const uint64_t p = pid[i];
        if (p <= paths_cap) offsets[p] = choff[i];
    }
}

template <int W>
__global__ __launch_bounds__(UG_THREADS) void k_ug_spell(const uint64_t* __restrict__ tk, uint32_t n2, int k, const uint2* __restrict__ hd,
                                                         const uint32_t* __restrict__ len, const uint64_t* __restrict__ choff, char* __restrict__ seqs,
                                                         uint64_t cap) {
    for (uint64_t i = blockIdx.x * (uint64_t)UG_THREADS + threadIdx.x; i < n2; i += (uint64_t)gridDim.x * UG_THREADS) {
        const uint2 o = hd[i];
        if (o.x == BFT_SP_NONE || len[o.x] == 0u) continue;  // (in no path, or in the mirror that is not reported)
        const uint64_t base = choff[o.x];
        uint64_t x[W], xr[W];
        ug_row<W>(tk, i >> 1, k, x, xr);
        const bool rev = (i & 1u) != 0;
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

template <class F>
int ug_dispatch(int W, F&& f) {
    switch (W) {
    case 1: f(std::integral_constant<int, 1>()); break;
    case 2: f(std::integral_constant<int, 2>()); break;
    case 3: f(std::integral_constant<int, 3>()); break;
    default: f(std::integral_constant<int, 4>()); break;
    }
    HIPCK(hipGetLastError());
    return 0;
}
dim3 ug_grid(uint64_t n) { return dim3(bft_grid_for((n + UG_THREADS - 1) / UG_THREADS)); }

}  // namespace

int bft_ug_canonicity(int W, const uint64_t* d_tk, uint64_t n, int k, unsigned long long* d_noncanonical, hipStream_t s) {
    if (n == 0) return 0;
    return ug_dispatch(W, [&](auto KW) { hipLaunchKernelGGL((k_ug_canon<KW>), ug_grid(n), dim3(UG_THREADS), 0, s, d_tk, (uint32_t)n, k, d_noncanonical); });
}

int bft_ug_degrees(int W, const uint64_t* d_tk, uint64_t n, int k, const BftSpScratch& p, uint8_t* d_deg, uint64_t deg_cap, bool pal, uint32_t* d_succ,
                   hipStream_t s) {
    if (n == 0) return 0;
    return ug_dispatch(W, [&](auto KW) {
        hipLaunchKernelGGL((k_ug_degrees<KW>), ug_grid(n), dim3(UG_THREADS), 0, s, d_tk, (uint32_t)n, k, p.sb, p.start, d_deg, deg_cap, pal ? BFT_UG_PAL : 0u, d_succ);
    });
}

int bft_ug_links(uint64_t n, uint32_t t, const uint32_t* d_tcol, const uint32_t* d_cs_off, const void* d_cs_ids, uint32_t cs_w, const BftUgScratch& p, hipStream_t s) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_ug_links, ug_grid(2 * n), dim3(UG_THREADS), 0, s, (uint32_t)(2 * n), t, d_tcol, d_cs_off, d_cs_ids, cs_w, p.sp.succ, p.deg, p.sp.flags, p.sp.st[0]);
    HIPCK(hipGetLastError());
    return 0;
}

int bft_ug_ends(uint64_t n, int k, const BftUgScratch& p, int fin, unsigned long long* d_longest, hipStream_t s) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_ug_ends, ug_grid(2 * n), dim3(UG_THREADS), 0, s, (uint32_t)(2 * n), k, p.sp.st[fin], p.sp.flags, p.sp.succ,
                       reinterpret_cast<uint2*>(p.sp.st[fin ^ 1]), p.sp.indeg, d_longest);
    HIPCK(hipGetLastError());
    return 0;
}

int bft_ug_offsets(uint64_t n, const BftUgScratch& p, int fin, uint64_t* d_offsets, uint64_t paths_cap, const unsigned long long* d_counts, hipStream_t s) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_ug_offsets, ug_grid(2 * n), dim3(UG_THREADS), 0, s, (uint32_t)(2 * n), bft_sp_hd(p.sp, fin), p.sp.indeg, p.sp.pred, p.sp.choff, d_offsets,
                       paths_cap, d_counts);
    HIPCK(hipGetLastError());
    return 0;
}

int bft_ug_spell(int W, const uint64_t* d_tk, uint64_t n, int k, const BftUgScratch& p, int fin, char* d_seqs, uint64_t chars_cap, hipStream_t s) {
    if (n == 0 || chars_cap == 0) return 0;
    return ug_dispatch(W, [&](auto KW) {
        hipLaunchKernelGGL((k_ug_spell<KW>), ug_grid(2 * n), dim3(UG_THREADS), 0, s, d_tk, (uint32_t)(2 * n), k, bft_sp_hd(p.sp, fin), p.sp.indeg, p.sp.choff, d_seqs,
                           chars_cap);
    });
}

// ------------------------------------------------------------------------------------------------
// the C-ABI entry points: the handle's scratch, the chain of launches, the host-buffer forms
// ------------------------------------------------------------------------------------------------
// the arrays of a block for m rows (p->sp.sb set), from `base` on; returns the block's size: 107 bytes per row and the bucket starts.
// full = false: what the degrees alone need (the bucket starts and a byte per row)
static size_t ug_carve(uint64_t m, bool full, uint8_t* base, BftUgScratch* p) {
    Carver c{base};
    c.take(p->sp.start, ((1ull << p->sp.sb) + 1) * 4);
    c.take(p->deg, m);
    if (!full) return c.off;
    c.take(p->sp.succ, 2 * m * 4);
    c.take(p->sp.indeg, 2 * m * 4);
    c.take(p->sp.pred, 2 * m * 4);
    c.take(p->sp.flags, 2 * m);
    c.take(p->sp.st[0], 2 * m * 16);
    c.take(p->sp.st[1], 2 * m * 16);
    c.take(p->sp.choff, 2 * m * 8);
    return c.off;
}
// The scratch is the simple paths' (h->sp with h->sp_buf / h->sp_tmp, bft_handle.h): the two calls are serialised on a handle, the block holds the larger.
static int ug_scratch(bft_gpu* h, uint64_t n, bool full, hipStream_t s, BftUgScratch* p) {
    CK(h->sp.acquire(s, false));  // (the entry points refuse a capturing stream)
    *p = BftUgScratch{};
    p->sp.sb = bft_sp_bucket_bits(h->k);
    CK(h->sp.grow(h->sp_buf, ug_carve(n, full, nullptr, p), 0));
    if (full) CK(h->sp.grow(h->sp_tmp, bft_scan::scratch_bytes(2 * n + 1), 0));
    ug_carve(n, full, h->sp_buf.as<uint8_t>(), p);
    return 0;
}
static int ug_prepare(bft_gpu* h, const char* what) {
    CK(bft_ensure_built(h));  // ("compact_table": the sorted table comes back, as for the simple paths)
    if (h->n_kmers >= (1ull << 31)) return bft_fail(BFT_GPU_E_LIMIT, std::string(what) + ": at most 2^31 - 1 k-mers");  // (vertex ids stay below BFT_SP_MANY)
    return 0;
}

// Canonicity, degrees, links, jumps, ends and both scans on stream s: d_counts = {n_paths, n_chars, longest, non-canonical rows} (32 bytes, device).
static int ug_count(bft_gpu* h, uint32_t t, hipStream_t s, unsigned long long* d_counts, const BftUgScratch& p, int* fin) {
    const uint64_t n = h->n_kmers, n2 = 2 * n;
    const int W = h->W, k = h->k;
    const uint64_t* tk = h->d_tk.as<uint64_t>();
    const double nd = (double)n, rowb = 8.0 * W;
    CK(bft_zero_async(d_counts, 32, s));
    CK(bft_zero_async(p.sp.indeg, n2 * 4, s));
    CK(bft_timed_launch(h, s, [&] { return bft_ug_canonicity(W, tk, n, k, d_counts + 3, s); }));
    bft_stage("unitigs: canonicity", nd * rowb, s);
    CK(bft_timed_launch(h, s, [&] { return bft_sp_buckets(W, tk, n, k, p.sp, s); }));
    bft_stage("unitigs: buckets of the table", (double)((1ull << p.sp.sb) + 1) * 4, s);
    CK(bft_timed_launch(h, s, [&] { return bft_ug_degrees(W, tk, n, k, p.sp, p.deg, n, true, p.sp.succ, s); }));
    bft_stage("unitigs: bidirected degrees and successors", nd * (rowb + 1 + 8), s);
    CK(bft_timed_launch(h, s, [&] { return bft_ug_links(n, t, h->d_tcol.as<uint32_t>(), h->d_cs_off.as<uint32_t>(), h->d_cs_ids.p, h->cs_w, p, s); }));
    bft_stage("unitigs: nodes and edges", 2 * nd * (12 + 2 + (t ? 8 : 0) + 1 + 16), s);
    // ceil(log2(n + 1)) rounds, not ceil(log2(2n + 1)): a path of a canonical index never holds both orientations of a row (its mirror does), so no
    // chain or cycle is longer than n vertices.  (On an index that is not canonical the paths are unspecified; every index stays inside the arrays.)
    int cur = 0, rounds = 0;
    for (uint64_t span = 1; span < n + 1; span <<= 1, cur ^= 1, rounds++) CK(bft_timed_launch(h, s, [&] { return bft_sp_jump(n2, p.sp, cur, s); }));
    *fin = cur;
    bft_stage("unitigs: pointer jumping", 2 * nd * 48 * rounds, s);
    CK(bft_timed_launch(h, s, [&] { return bft_ug_ends(n, k, p, cur, d_counts + 2, s); }));
    bft_stage("unitigs: heads, tails, lengths, the kept mirror", 2 * nd * (16 + 1 + 4 + 8) + nd * 4, s);
    const uint2* hd = bft_sp_hd(p.sp, cur);
    CK(bft_timed_launch(h, s, [&] { return bft_scan::exclusive_sum<uint32_t>(BftUgHead{hd, p.sp.indeg, n2}, p.sp.pred, n2, s, h->sp_tmp, d_counts, false); }));
    CK(bft_timed_launch(h, s, [&] { return bft_scan::exclusive_sum<uint64_t>(BftUgHeadLen{hd, p.sp.indeg, n2}, p.sp.choff, n2, s, h->sp_tmp, d_counts + 1, false); }));
    bft_stage("unitigs: two scans (paths, characters)", 2 * nd * (8 + 4 + 4 + 8 + 4 + 8), s);
    return 0;
}
// offsets (paths_cap + 1 entries at most) and characters (chars_cap at most) of the paths ug_count counted
static int ug_emit(bft_gpu* h, const BftUgScratch& p, int fin, uint64_t* d_offsets, uint64_t paths_cap, char* d_seqs, uint64_t chars_cap,
                   const unsigned long long* d_counts, hipStream_t s) {
    const uint64_t n = h->n_kmers;
    if (d_offsets) CK(bft_timed_launch(h, s, [&] { return bft_ug_offsets(n, p, fin, d_offsets, paths_cap, d_counts, s); }));
    bft_stage("unitigs: offsets", (double)n * 2 * 12, s);
    if (d_seqs) CK(bft_timed_launch(h, s, [&] { return bft_ug_spell(h->W, h->d_tk.as<uint64_t>(), n, h->k, p, fin, d_seqs, chars_cap, s); }));
    bft_stage("unitigs: spelling", (double)n * 2 * (8.0 * h->W + 8 + 4 + 8 + 1), s);
    return 0;
}

extern "C" int bft_gpu_unitigs_dev(bft_gpu* h, uint32_t min_shared, void* d_offsets, void* d_seqs, uint64_t paths_cap, uint64_t chars_cap, void* d_counts,
                                   void* hip_stream) {
    if (!h || !d_counts) return bft_fail(BFT_GPU_E_ARG, "NULL argument");
    ENTER(h);
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : h->stream;
    if (bft_stream_capturing(s)) return bft_fail(BFT_GPU_E_ARG, "unitigs recorded into a graph: not supported (the table may have to come back, scratch may grow)");
    CK(ug_prepare(h, "unitigs"));
    if (h->n_kmers == 0) {
        CK(bft_zero_async(d_counts, 32, s));
        if (d_offsets) CK(bft_zero_async(d_offsets, 8, s));
        return bft_note_foreign_stream(h, s);
    }
    BftUgScratch p;
    CK(ug_scratch(h, h->n_kmers, true, s, &p));
    {
        StageScope stage_scope(h, s);
        int fin = 0;
        CK(ug_count(h, min_shared, s, (unsigned long long*)d_counts, p, &fin));
        CK(ug_emit(h, p, fin, (uint64_t*)d_offsets, paths_cap, (char*)d_seqs, chars_cap, (const unsigned long long*)d_counts, s));
    }
    h->sp.release();
    return bft_note_foreign_stream(h, s);
}

// The host-buffer form: the paths are counted on the device, and the outputs filled only when the index is canonical and the caps hold them all.
extern "C" int bft_gpu_unitigs(bft_gpu* h, uint32_t min_shared, uint64_t* offsets, char* seqs, uint64_t paths_cap, uint64_t chars_cap, uint64_t* n_paths,
                               uint64_t* n_chars) {
    if (!h || !n_paths || !n_chars) return bft_fail(BFT_GPU_E_ARG, "NULL argument");
    ENTER(h);
    CK(ug_prepare(h, "unitigs"));
    *n_paths = *n_chars = 0;
    if (h->n_kmers == 0) {
        if (offsets) offsets[0] = 0;
        return BFT_GPU_OK;
    }
    const hipStream_t s = h->stream;
    DevBuf dcnt;
    CK(dcnt.alloc(32));
    BftUgScratch p;
    CK(ug_scratch(h, h->n_kmers, true, s, &p));
    StageScope stage_scope(h);
    int fin = 0;
    CK(ug_count(h, min_shared, s, dcnt.as<unsigned long long>(), p, &fin));
    unsigned long long cnt[4] = {0, 0, 0, 0};
    HIPCK(hipMemcpyAsync(cnt, dcnt.p, 32, hipMemcpyDeviceToHost, s));
    HIPCK(hipStreamSynchronize(s));
    if (cnt[3]) {
        h->sp.release();
        return bft_fail(BFT_GPU_E_STATE, "unitigs: the index is not canonical (" + std::to_string(cnt[3]) + " k-mers above their reverse complement)");
    }
    *n_paths = cnt[0];
    *n_chars = cnt[1];
    if ((offsets && cnt[0] > paths_cap) || (seqs && cnt[1] > chars_cap)) {
        h->sp.release();
        return bft_fail(BFT_GPU_E_NOSPACE, "unitig buffers too small");
    }
    if (offsets || seqs) {
        DevBuf doff, dseq;
        if (offsets) CK(doff.alloc((cnt[0] + 1) * 8));
        if (seqs && cnt[1]) CK(dseq.alloc(cnt[1]));
        CK(ug_emit(h, p, fin, offsets ? doff.as<uint64_t>() : nullptr, cnt[0], seqs ? dseq.as<char>() : nullptr, cnt[1], dcnt.as<unsigned long long>(), s));
        if (offsets) HIPCK(hipMemcpyAsync(offsets, doff.p, (cnt[0] + 1) * 8, hipMemcpyDeviceToHost, s));
        if (seqs && cnt[1]) HIPCK(hipMemcpyAsync(seqs, dseq.p, cnt[1], hipMemcpyDeviceToHost, s));
        HIPCK(hipStreamSynchronize(s));
    }
    h->sp.release();
    return BFT_GPU_OK;
}

// canonicity and the degree bytes of the rows below cap on stream s (d_degrees may be null: the count alone)
static int ug_degrees(bft_gpu* h, uint8_t* d_degrees, uint64_t cap, unsigned long long* d_noncanonical, hipStream_t s) {
    const uint64_t n = h->n_kmers;
    const uint64_t* tk = h->d_tk.as<uint64_t>();
    CK(bft_zero_async(d_noncanonical, 8, s));
    CK(bft_timed_launch(h, s, [&] { return bft_ug_canonicity(h->W, tk, n, h->k, d_noncanonical, s); }));
    bft_stage("bidirected degrees: canonicity", (double)n * 8.0 * h->W, s);
    if (!d_degrees || cap == 0) return 0;
    BftUgScratch p;
    CK(ug_scratch(h, n, false, s, &p));
    CK(bft_timed_launch(h, s, [&] { return bft_sp_buckets(h->W, tk, n, h->k, p.sp, s); }));
    bft_stage("bidirected degrees: buckets of the table", (double)((1ull << p.sp.sb) + 1) * 4, s);
    CK(bft_timed_launch(h, s, [&] { return bft_ug_degrees(h->W, tk, n, h->k, p.sp, d_degrees, cap, false, nullptr, s); }));
    bft_stage("bidirected degrees: degrees", (double)n * (8.0 * h->W + 1), s);
    h->sp.release();
    return 0;
}

extern "C" int bft_gpu_bidirected_degrees_dev(bft_gpu* h, void* d_degrees, uint64_t cap, void* d_noncanonical, void* hip_stream) {
    if (!h || !d_noncanonical) return bft_fail(BFT_GPU_E_ARG, "NULL argument");
    ENTER(h);
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : h->stream;
    if (bft_stream_capturing(s)) return bft_fail(BFT_GPU_E_ARG, "bidirected degrees recorded into a graph: not supported (the table may have to come back, scratch may grow)");
    CK(ug_prepare(h, "bidirected degrees"));
    if (h->n_kmers == 0) {
        CK(bft_zero_async(d_noncanonical, 8, s));
        return bft_note_foreign_stream(h, s);
    }
    {
        StageScope stage_scope(h, s);
        CK(ug_degrees(h, (uint8_t*)d_degrees, cap, (unsigned long long*)d_noncanonical, s));
    }
    return bft_note_foreign_stream(h, s);
}

extern "C" int bft_gpu_bidirected_degrees(bft_gpu* h, uint8_t* degrees, uint64_t cap, uint64_t* n_noncanonical) {
    if (!h || !n_noncanonical) return bft_fail(BFT_GPU_E_ARG, "NULL argument");
    ENTER(h);
    CK(ug_prepare(h, "bidirected degrees"));
    *n_noncanonical = 0;
    const uint64_t n = h->n_kmers;
    if (n == 0) return BFT_GPU_OK;
    if (degrees && cap < n) return bft_fail(BFT_GPU_E_NOSPACE, "degree buffer too small");
    const hipStream_t s = h->stream;
    DevBuf dcnt, ddeg;
    CK(dcnt.alloc(8));
    if (degrees) CK(ddeg.alloc(n));
    StageScope stage_scope(h);
    CK(ug_degrees(h, degrees ? ddeg.as<uint8_t>() : nullptr, n, dcnt.as<unsigned long long>(), s));
    unsigned long long bad = 0;
    HIPCK(hipMemcpyAsync(&bad, dcnt.p, 8, hipMemcpyDeviceToHost, s));
    if (degrees) HIPCK(hipMemcpyAsync(degrees, ddeg.p, n, hipMemcpyDeviceToHost, s));
    HIPCK(hipStreamSynchronize(s));
    *n_noncanonical = bad;
    return BFT_GPU_OK;
}
