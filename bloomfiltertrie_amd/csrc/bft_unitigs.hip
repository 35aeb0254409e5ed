// bft_unitigs.hip -- canonical (bidirected) unitigs and degrees: the compacted de Bruijn graph of an index that stores the smaller of each k-mer and
// its reverse complement (bft_gpu_insert_sequences(..., canonical = 1)), over the sorted T-form table tk.  include/bft_gpu.h defines the paths; an
// oriented vertex is v = 2 * row + o with word s (o = 0) or rc(s) (o = 1), its flip v ^ 1.  The unitigs are the mirrored family of the path engine
// (bft_paths.h, bft_paths.hip): this unit holds what is the family's own -- canonicity, degrees, links -- and its descriptor.
//   k_ug_canon    rows with s > rc(s): the call is defined where there is none
//   k_ug_degrees  one lane per row, both orientations.  The successor words w[1..k-1]+N of an orientation are represented by a stored y or a stored
//                 rc(y).  The four y lie in one interval of the table (ONE lower bound inside a bucket: bft_for_each_successor_of, bft_succ.h, the
//                 word form of the search the simple paths and the components run on rows); the four rc(y) = comp(N) + rc(w)[0..k-2] differ in the
//                 FIRST nucleotide and lie in four buckets: one bucketed exact lookup each (bft_find_row), and only for the N that the interval did
//                 not hold -- so a word counts once, a palindromic y too.  (A scatter from the interval, as k_sp_degrees finds
//                 its predecessors, learns only half of them here -- a hit (u,o) -> (r,0) says (r,1) -> (u,1-o), never what follows (r,0) as a
//                 reverse complement -- and needs an atomic mask per vertex to count words once: searched instead, no atomics, same answer every run.)
//                 A palindrome has one orientation: searched once.
//   k_ug_links    one lane per vertex: nodes (out(v) <= 1, out(v ^ 1) <= 1, colour set of t genomes or more) and edges (u -> v: v is u's only
//                 successor, u ^ 1 is (v ^ 1)'s, both nodes, two rows, no palindrome, |C(u) & C(v)| >= t), each decided at both of its ends and in
//                 both mirrors by the same predicate; the vertex before v is the flip of (v ^ 1)'s successor: no predecessor array.  The first
//                 state of the jumps
//   (the engine's, over the 2n vertices: k_sp_buckets, k_sp_jump, and the MIRRORED instantiations of k_sp_ends -- the kept mirror --, of the two
//   scans over kept heads, of k_sp_offsets and of k_sp_spell)
// No kernel needs LDS or scratch memory.
#include "bft_dev.h"
#include "bft_handle.h"
#include "bft_succ.h"
#include "bft_unitigs.h"

namespace {

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
    bft_x_revcomp<W>(x, k, xr);
    return ug_cmp<W>(x, xr);
}

// succ[] of the vertex with word w: its represented successor words counted once each; the vertex of the only one
template <int W>
__device__ __forceinline__ uint32_t ug_successors(const uint64_t* __restrict__ tk, uint32_t n, int k, int sb, const uint32_t* __restrict__ start,
                                                  const uint64_t* w, uint32_t* out) {
    uint32_t cnt = 0, v = BFT_SP_NONE, have = 0;
    // the stored successor words: row r holds the one with nucleotide c last
    bft_for_each_successor_of<W>(tk, n, k, sb, start, w, [&](uint32_t r, uint32_t c) {
        have |= 1u << c;
        cnt++;
        v = 2u * r;
    });
    // the others, as stored reverse complements.  rc of the successor word with A last: T + rc(w)[0..k-2]; with N last, comp(N) comes first
    uint64_t y[W], z[W];
#pragma unroll
    for (int q = 0; q < W; q++) y[q] = (w[q] >> 2) | (q + 1 < W ? w[q + 1] << 62 : 0ull);
    bft_x_revcomp<W>(y, k, z);
    for (uint32_t c = 0; c < 4; c++) {
        if ((have >> c) & 1u) continue;
        z[0] = (z[0] & ~3ull) | (uint64_t)(3u - c);
        const uint32_t r = bft_find_row<W>(tk, k, sb, start, z);
        if (r == BFT_SP_NONE) continue;
        cnt++;
        v = 2u * r + 1u;
    }
    *out = cnt;
    return cnt == 0 ? BFT_SP_NONE : cnt == 1 ? v : BFT_SP_MANY;
}

template <int W>
__global__ __launch_bounds__(BFT_LAUNCH_THREADS) void k_ug_canon(const uint64_t* __restrict__ tk, uint32_t n, int k, unsigned long long* __restrict__ bad) {
    // (every lane of a wavefront runs the same iterations: the wavefront's count is one ballot)
    for (uint64_t i0 = blockIdx.x * (uint64_t)BFT_LAUNCH_THREADS + (threadIdx.x & ~63u); i0 < n; i0 += (uint64_t)gridDim.x * BFT_LAUNCH_THREADS) {
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
__global__ __launch_bounds__(BFT_LAUNCH_THREADS) void k_ug_degrees(const uint64_t* __restrict__ tk, uint32_t n, int k, int sb, const uint32_t* __restrict__ start,
                                                                   uint8_t* __restrict__ deg, uint64_t deg_cap, uint32_t pal_bit, uint32_t* __restrict__ succ) {
    for (uint64_t u = blockIdx.x * (uint64_t)BFT_LAUNCH_THREADS + threadIdx.x; u < n; u += (uint64_t)gridDim.x * BFT_LAUNCH_THREADS) {
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

__global__ __launch_bounds__(BFT_LAUNCH_THREADS) void k_ug_links(uint32_t n2, uint32_t t, const uint32_t* __restrict__ tcol, const uint32_t* __restrict__ cs_off,
                                                                 const void* __restrict__ cs_ids, uint32_t cs_w, const uint32_t* __restrict__ succ,
                                                                 const uint8_t* __restrict__ deg, uint8_t* __restrict__ flags, uint4* __restrict__ st) {
    for (uint64_t i0 = blockIdx.x * (uint64_t)BFT_LAUNCH_THREADS + threadIdx.x; i0 < n2; i0 += (uint64_t)gridDim.x * BFT_LAUNCH_THREADS) {
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

}  // namespace

int bft_ug_canonicity(int W, const uint64_t* d_tk, uint64_t n, int k, unsigned long long* d_noncanonical, hipStream_t s) {
    return bft_for_w(W, [&](auto KW) { return bft_launch256(k_ug_canon<KW>, n, s, d_tk, (uint32_t)n, k, d_noncanonical); });
}

int bft_ug_degrees(int W, const uint64_t* d_tk, uint64_t n, int k, const BftSpScratch& p, uint8_t* d_deg, uint64_t deg_cap, bool pal, uint32_t* d_succ,
                   hipStream_t s) {
    return bft_for_w(W, [&](auto KW) { return bft_launch256(k_ug_degrees<KW>, n, s, d_tk, (uint32_t)n, k, p.sb, p.start, d_deg, deg_cap, pal ? BFT_UG_PAL : 0u, d_succ); });
}

int bft_ug_links(uint64_t n, uint32_t t, const uint32_t* d_tcol, const uint32_t* d_cs_off, const void* d_cs_ids, uint32_t cs_w, const BftSpScratch& p, hipStream_t s) {
    return bft_launch256(k_ug_links, 2 * n, s, (uint32_t)(2 * n), t, d_tcol, d_cs_off, d_cs_ids, cs_w, p.succ, p.deg, p.flags, p.st[0]);
}

// ------------------------------------------------------------------------------------------------
// the C-ABI entry points: the unitigs through the path engine, the degrees on their own
// ------------------------------------------------------------------------------------------------
// a stage named "<family>: <what>" (the name is put together only where "build_stages" is on)
static void ug_stage(const bft_gpu* h, const char* family, const char* what, double bytes, hipStream_t s) {
    if (h->opt_build_stages) bft_stage((std::string(family) + ": " + what).c_str(), bytes, s);
}
// canonicity (into d_counts[3]), buckets, degrees of both orientations, links
int bft_ug_front(bft_gpu* h, const char* family, uint32_t t, hipStream_t s, unsigned long long* d_counts, const BftSpScratch& p) {
    const uint64_t n = h->n_kmers;
    const int W = h->W, k = h->k;
    const uint64_t* tk = h->d_tk.as<uint64_t>();
    const double nd = (double)n, rowb = 8.0 * W;
    CK(bft_timed_launch(h, s, [&] { return bft_ug_canonicity(W, tk, n, k, d_counts + 3, s); }));
    ug_stage(h, family, "canonicity", nd * rowb, s);
    CK(bft_timed_launch(h, s, [&] { return bft_sp_buckets(W, tk, n, k, p, s); }));
    ug_stage(h, family, "buckets of the table", (double)((1ull << p.sb) + 1) * 4, s);
    CK(bft_timed_launch(h, s, [&] { return bft_ug_degrees(W, tk, n, k, p, p.deg, n, true, p.succ, s); }));
    ug_stage(h, family, "bidirected degrees and successors", nd * (rowb + 1 + 8), s);
    CK(bft_timed_launch(h, s, [&] { return bft_ug_links(n, t, h->d_tcol.as<uint32_t>(), h->d_cs_off.as<uint32_t>(), h->d_cs_ids.p, h->cs_w, p, s); }));
    ug_stage(h, family, "nodes and edges", 2 * nd * (12 + 2 + (t ? 8 : 0) + 1 + 16), s);
    return 0;
}
static int ug_front(bft_gpu* h, uint32_t t, hipStream_t s, unsigned long long* d_counts, const BftSpScratch& p) { return bft_ug_front(h, "unitigs", t, s, d_counts, p); }
// the host-buffer form fills nothing where the index is not canonical
int bft_ug_check(const unsigned long long* cnt) {
    if (cnt[3]) return bft_fail(BFT_GPU_E_STATE, "unitigs: the index is not canonical (" + std::to_string(cnt[3]) + " k-mers above their reverse complement)");
    return 0;
}
// d_counts = {n_paths, n_chars, longest, non-canonical rows}
static const BftPathFamily UG_FAMILY = {
    true,
    32,
    "unitigs",
    "unitigs: heads, tails, lengths, the kept mirror",
    "unitigs recorded into a graph: not supported (the table may have to come back, scratch may grow)",
    "unitig buffers too small",
    ug_front,
    bft_ug_check,
};

extern "C" int bft_gpu_unitigs_dev(bft_gpu* h, uint32_t min_shared, void* d_offsets, void* d_seqs, uint64_t paths_cap, uint64_t chars_cap, void* d_counts,
                                   void* hip_stream) {
    return bft_paths_dev(h, UG_FAMILY, min_shared, d_offsets, d_seqs, paths_cap, chars_cap, d_counts, hip_stream);
}

extern "C" int bft_gpu_unitigs(bft_gpu* h, uint32_t min_shared, uint64_t* offsets, char* seqs, uint64_t paths_cap, uint64_t chars_cap, uint64_t* n_paths,
                               uint64_t* n_chars) {
    return bft_paths_host(h, UG_FAMILY, min_shared, offsets, seqs, paths_cap, chars_cap, n_paths, n_chars);
}

// canonicity and the degree bytes of the rows below cap on stream s (d_degrees may be null: the count alone)
static int ug_degrees(bft_gpu* h, uint8_t* d_degrees, uint64_t cap, unsigned long long* d_noncanonical, hipStream_t s) {
    const uint64_t n = h->n_kmers;
    const uint64_t* tk = h->d_tk.as<uint64_t>();
    CK(bft_zero_async(d_noncanonical, 8, s));
    CK(bft_timed_launch(h, s, [&] { return bft_ug_canonicity(h->W, tk, n, h->k, d_noncanonical, s); }));
    bft_stage("bidirected degrees: canonicity", (double)n * 8.0 * h->W, s);
    if (!d_degrees || cap == 0) return 0;
    // (of the handle's scratch the bucket starts alone: its use ends here, before whatever the caller does behind the degrees)
    HandleScratch::Lease lease(h->sp);
    BftSpScratch p;
    CK(bft_sp_scratch(h, lease, 0, 0, 0, s, &p));
    CK(bft_timed_launch(h, s, [&] { return bft_sp_buckets(h->W, tk, n, h->k, p, s); }));
    bft_stage("bidirected degrees: buckets of the table", (double)((1ull << p.sb) + 1) * 4, s);
    CK(bft_timed_launch(h, s, [&] { return bft_ug_degrees(h->W, tk, n, h->k, p, d_degrees, cap, false, nullptr, s); }));
    bft_stage("bidirected degrees: degrees", (double)n * (8.0 * h->W + 1), s);
    return 0;
}

extern "C" int bft_gpu_bidirected_degrees_dev(bft_gpu* h, void* d_degrees, uint64_t cap, void* d_noncanonical, void* hip_stream) {
    if (!h || !d_noncanonical) return bft_fail(BFT_GPU_E_ARG, "NULL argument");
    ENTER(h);
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : h->stream;
    if (bft_stream_capturing(s)) return bft_fail(BFT_GPU_E_ARG, "bidirected degrees recorded into a graph: not supported (the table may have to come back, scratch may grow)");
    CK(bft_sp_prepare(h, "bidirected degrees"));
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
    CK(bft_sp_prepare(h, "bidirected degrees"));
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
