// bft_thread.hip -- sequence threading: the maximal walks over oriented segments of the compacted coloured graph that a batch of sequences spells
// exactly (bft_gpu_thread_sequences / _dev; include/bft_gpu.h defines them).  The call reads the sorted T-form table of a canonical index, the arrays
// bft_gpu_unitig_graph and bft_gpu_unitig_segment_of returned, and the sequences.
//   (the front of a sequence batch, unchanged: k_seq_encode, k_seq_plan, a scan, k_seq_tiles -- bft_kernels_seqenc.h)
//   (the unitigs' front kernels into this call's own scratch: k_ug_canon -- the rows above their reverse complement --, k_sp_buckets)
//   k_th_locate  one lane per position: the window and its strand (seq_window_strand), the bucketed exact lookup of the canonical word
//                (bft_find_row), seg_of / pos of the row -> {X, q}, or a code that says why the position is not located.  The three reasons are
//                summed per wavefront over its whole grid-stride loop: one atomic per wavefront and statistic
//   k_th_flags   one lane per position: the transition from position p - 1 of the same sequence (whatever workgroup or tile holds it: loc[] is
//                complete), the at most four links of an across transition; a flag byte -- located, opens a walk, opens a step; breaks counted
//                per wavefront like the reasons
//   (two scans over the flag bytes, BftThFlag: the walk a start opens, the slot of every step; their totals are n_walks and n_steps)
//   k_th_emit    a walk start writes {s, p0, -, q0} and its entry of walk_off, a step start its step; walk_off[n_walks] once; all below the caps
//   k_th_close   the last position of a walk -- the next one opens a walk or is not located -- writes n_w
// A walk's end is read off the NEXT position's flag instead of being decided by a second classification in k_th_flags, and its length needs the
// start's position, which only the start lane knows: k_th_emit leaves it in the n_w slot, k_th_close turns it into the length.
// No kernel needs LDS or scratch memory.
#include "bft_thread.h"

#include "bft_dev.h"
#include "bft_handle.h"
#include "bft_paths.h"
#include "bft_scan.h"
#include "bft_succ.h"
#include "bft_unitigs.h"

namespace {

#include "bft_kernels_seqenc.h"

// the graph and the segment table as the caller gave them.  n2 = 2S <= 2^32 - 2
struct ThGraph {
    const uint32_t* __restrict__ seg_of;
    const uint32_t* __restrict__ pos;
    const uint64_t* __restrict__ seg_off;
    const uint64_t* __restrict__ link_off;
    const uint32_t* __restrict__ links;
    uint64_t n2, n_links;
    int k;
};
// the batch: codes and plan in the scratch, the caller's offsets
struct ThBatch {
    const uint64_t* __restrict__ codes;
    const uint32_t* __restrict__ bad;
    const uint64_t* __restrict__ seq_off;
    const uint64_t* __restrict__ pos_off;
    const uint32_t* __restrict__ tile_seq;
    uint32_t n_seqs;
    uint64_t n_chars;  // characters of the blob = entries of every per-position array
};

// positions of the batch (never more than the per-position arrays hold, whatever the offsets say)
__device__ __forceinline__ uint64_t th_positions(const ThBatch& b) { return min(b.pos_off[b.n_seqs], b.n_chars); }
// the sequence of position p (p < positions): from the tile table, stepping over sequences without a position
__device__ __forceinline__ uint32_t th_seq_of(const ThBatch& b, uint64_t p) {
    uint32_t lo = b.tile_seq[p >> 6];
    while (lo + 1 < b.n_seqs && b.pos_off[lo + 1] <= p) lo++;
    return lo;
}
// members of segment i (i < S); 0 where the offsets give none
__device__ __forceinline__ uint64_t th_members(const ThGraph& g, uint32_t i) {
    const uint64_t o0 = g.seg_off[i], o1 = g.seg_off[(uint64_t)i + 1], km1 = (uint64_t)(g.k - 1);
    return o1 >= o0 && o1 - o0 > km1 ? o1 - o0 - km1 : 0ull;
}
// y is in out(x): a list of more than 4 entries or past n_links is the empty list
__device__ __forceinline__ bool th_linked(const ThGraph& g, uint32_t x, uint32_t y) {
    const uint64_t lo = g.link_off[x], hi = g.link_off[(uint64_t)x + 1];
    if (lo > hi || hi > g.n_links || hi - lo > 4) return false;
    bool is = false;
    for (uint64_t j = lo; j < hi; j++) is = is || g.links[j] == y;
    return is;
}

// counts[2] = positions, counts[3 .. 5] += invalid / absent / in no segment
template <int W>
__global__ __launch_bounds__(BFT_LAUNCH_THREADS) void k_th_locate(const uint64_t* __restrict__ tk, int sb, const uint32_t* __restrict__ start, ThBatch b, ThGraph g,
                                                                  uint2* __restrict__ loc, unsigned long long* __restrict__ counts) {
    const uint64_t P = th_positions(b);
    if (blockIdx.x == 0 && threadIdx.x == 0) counts[2] = P;
    // (every lane of a wavefront runs the same iterations: what the wavefront found is summed over its whole grid-stride loop)
    uint32_t invalid = 0, absent = 0, noseg = 0;
    for (uint64_t p0 = blockIdx.x * (uint64_t)BFT_LAUNCH_THREADS + (threadIdx.x & ~63u); p0 < P; p0 += (uint64_t)gridDim.x * BFT_LAUNCH_THREADS) {
        const uint64_t p = p0 + (threadIdx.x & 63u);
        if (p >= P) continue;
        const uint32_t s = th_seq_of(b, p);
        const uint64_t c0 = b.seq_off[s] + (p - b.pos_off[s]);
        uint2 out = make_uint2(BFT_TH_NONE, BFT_TH_INVALID);
        uint64_t x[W];
        uint32_t strand = 0;
        int kk = g.k;  // (this turn's own value: what the window and the T-form derive from it is computed where it is used, as in k_ing_write)
        asm volatile("" : "+s"(kk));
        if (c0 <= b.n_chars && b.n_chars - c0 >= (uint64_t)kk && seq_window_strand<W>(b.codes, b.bad, c0, kk, x, &strand)) {
            const uint32_t r = bft_find_row<W>(tk, kk, sb, start, x);
            if (r == BFT_TH_NONE) out.y = BFT_TH_ABSENT;
            else {
                out.y = BFT_TH_NOSEG;
                const uint32_t so = g.seg_of[r];
                if ((uint64_t)so < g.n2) {  // (0xFFFFFFFF is none)
                    const uint64_t m = th_members(g, so >> 1), q = g.pos[r];
                    const uint32_t X = so ^ strand;
                    if (q < m) out = make_uint2(X, (uint32_t)((X & 1u) ? m - 1 - q : q));
                }
            }
        }
        loc[p] = out;
        if (out.x == BFT_TH_NONE) {
            invalid += out.y == BFT_TH_INVALID;
            absent += out.y == BFT_TH_ABSENT;
            noseg += out.y == BFT_TH_NOSEG;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        invalid += __shfl_xor(invalid, o);
        absent += __shfl_xor(absent, o);
        noseg += __shfl_xor(noseg, o);
    }
    if ((threadIdx.x & 63u) == 0) {
        if (invalid) atomicAdd(counts + 3, (unsigned long long)invalid);
        if (absent) atomicAdd(counts + 4, (unsigned long long)absent);
        if (noseg) atomicAdd(counts + 5, (unsigned long long)noseg);
    }
}

// flag[p] of every entry of the per-position arrays (0 from the last position on); counts[6] += breaks
__global__ __launch_bounds__(BFT_LAUNCH_THREADS) void k_th_flags(ThBatch b, ThGraph g, const uint2* __restrict__ loc, uint8_t* __restrict__ flag,
                                                                 unsigned long long* __restrict__ counts) {
    const uint64_t P = th_positions(b);
    uint32_t breaks = 0;
    for (uint64_t p0 = blockIdx.x * (uint64_t)BFT_LAUNCH_THREADS + (threadIdx.x & ~63u); p0 < b.n_chars; p0 += (uint64_t)gridDim.x * BFT_LAUNCH_THREADS) {
        const uint64_t p = p0 + (threadIdx.x & 63u);
        if (p >= b.n_chars) continue;
        uint32_t f = 0;
        if (p < P) {
            const uint2 cur = loc[p];
            if (cur.x != BFT_TH_NONE) {
                f = BFT_TH_LOCATED | BFT_TH_WALK | BFT_TH_STEP;
                const uint32_t s = th_seq_of(b, p);
                if (p != b.pos_off[s]) {  // (p - 1 is a position of the same sequence)
                    const uint2 prv = loc[p - 1];
                    if (prv.x != BFT_TH_NONE) {
                        if (cur.x == prv.x && cur.y == prv.y + 1u) f = BFT_TH_LOCATED;  // inside
                        else if (cur.y == 0u && (uint64_t)prv.y + 1ull == th_members(g, prv.x >> 1) && th_linked(g, prv.x, cur.x)) f = BFT_TH_LOCATED | BFT_TH_STEP;  // across
                        else breaks++;
                    }
                }
            }
        }
        flag[p] = (uint8_t)f;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) breaks += __shfl_xor(breaks, o);
    if ((threadIdx.x & 63u) == 0 && breaks) atomicAdd(counts + 6, (unsigned long long)breaks);
}

// the records below the caps: {s, p0, (the walk's first position in the batch: k_th_close makes it n_w), q0}, walk_off, steps
__global__ __launch_bounds__(BFT_LAUNCH_THREADS) void k_th_emit(ThBatch b, const uint2* __restrict__ loc, const uint8_t* __restrict__ flag, const uint32_t* __restrict__ widx,
                                                                const uint32_t* __restrict__ sidx, const unsigned long long* __restrict__ counts,
                                                                uint64_t* __restrict__ walks, uint64_t* __restrict__ walk_off, uint64_t walks_cap,
                                                                uint32_t* __restrict__ steps, uint64_t steps_cap) {
    if (blockIdx.x == 0 && threadIdx.x == 0 && walk_off && counts[0] <= walks_cap) walk_off[counts[0]] = counts[1];
    for (uint64_t p = blockIdx.x * (uint64_t)BFT_LAUNCH_THREADS + threadIdx.x; p < b.n_chars; p += (uint64_t)gridDim.x * BFT_LAUNCH_THREADS) {
        const uint32_t f = flag[p];
        if (!(f & BFT_TH_STEP)) continue;
        const uint64_t si = sidx[p];
        const uint2 at = loc[p];
        if (steps && si < steps_cap) steps[si] = at.x;
        if (!(f & BFT_TH_WALK)) continue;
        const uint64_t w = widx[p];
        if (walk_off && w <= walks_cap) walk_off[w] = si;  // (walks_cap + 1 entries: the walks below the cap have their whole range of steps)
        if (walks && w < walks_cap) {
            const uint32_t s = th_seq_of(b, p);
            uint64_t* const r = walks + 4 * w;
            r[0] = s;
            r[1] = p - b.pos_off[s];
            r[2] = p;
            r[3] = at.y;
        }
    }
}

__global__ __launch_bounds__(BFT_LAUNCH_THREADS) void k_th_close(uint64_t n, const uint8_t* __restrict__ flag, const uint32_t* __restrict__ widx, uint64_t* __restrict__ walks,
                                                                 uint64_t walks_cap) {
    for (uint64_t p = blockIdx.x * (uint64_t)BFT_LAUNCH_THREADS + threadIdx.x; p < n; p += (uint64_t)gridDim.x * BFT_LAUNCH_THREADS) {
        const uint32_t f = flag[p];
        if (!(f & BFT_TH_LOCATED)) continue;
        const uint32_t nx = p + 1 < n ? flag[p + 1] : 0u;
        if ((nx & BFT_TH_LOCATED) && !(nx & BFT_TH_WALK)) continue;  // (the walk goes on)
        const uint64_t w = (uint64_t)widx[p] + ((f & BFT_TH_WALK) ? 1u : 0u) - 1ull;  // (an inclusive count of walk starts: one at least)
        if (w < walks_cap) walks[4 * w + 2] = p + 1 - walks[4 * w + 2];
    }
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// the chain of launches, the two forms of the entry point
// ------------------------------------------------------------------------------------------------
static const char* const TH_CAPTURE_MSG = "threading recorded into a graph: not supported (the table may have to come back, scratch may grow)";

// the per-position arrays hold one entry per character of the batch
static void th_carve(Carver& c, BftThScratch* p, uint64_t n_seqs, uint64_t n_chars, int sb) {
    const uint64_t n_cw = (n_chars + 31) / 32;
    c.take(p->codes, (n_cw + BFT_MAX_W + 2) * 8);
    c.take(p->bad, (n_cw + BFT_MAX_W + 2) * 4);
    c.take(p->npos, (n_seqs + 1) * 8);
    c.take(p->poff, (n_seqs + 1) * 8);
    c.take(p->tile, (n_chars / 64 + 2) * 4);
    c.take(p->start, ((1ull << sb) + 1) * 4);
    c.take(p->loc, n_chars * 8);
    c.take(p->flag, n_chars);
    c.take(p->widx, n_chars * 4);
    c.take(p->sidx, n_chars * 4);
}
// The handle's scratch (h->th: HandleScratch, bft_handle.h) for a batch on stream s: its own block, shared with no other family
static int th_scratch(bft_gpu* h, HandleScratch::Lease& lease, uint64_t n_seqs, uint64_t n_chars, hipStream_t s, BftThScratch* p) {
    CK(lease.acquire(s, false));  // (the entry points refuse a capturing stream)
    const int sb = bft_sp_bucket_bits(h->k);
    Carver c{nullptr};
    th_carve(c, p, n_seqs, n_chars, sb);
    CK(h->th.grow(h->th_buf, c.off, c.off / 8));
    CK(h->th.grow(h->th_tmp, bft_scan::scratch_bytes(std::max(n_seqs + 1, n_chars) + 1), 0));
    c = Carver{h->th_buf.as<uint8_t>()};
    th_carve(c, p, n_seqs, n_chars, sb);
    return 0;
}
static int th_check_sizes(uint64_t n_seqs, uint64_t n_chars, uint64_t n_segments) {
    if (n_chars >= (1ull << 32)) return bft_fail(BFT_GPU_E_LIMIT, "threading: fewer than 2^32 characters per call");
    if (n_seqs >= (1ull << 32)) return bft_fail(BFT_GPU_E_LIMIT, "threading: at most 2^32 - 1 sequences per call");
    return n_segments < (1ull << 31) ? 0 : bft_fail(BFT_GPU_E_LIMIT, "threading: at most 2^31 - 1 segments");  // (oriented segments and 0xFFFFFFFF stay apart)
}
// the built index with its table resident, and the segment table of exactly its rows
static int th_prepare(bft_gpu* h, uint64_t n_rows) {
    CK(bft_sp_prepare(h, "threading"));
    return n_rows == h->n_kmers ? 0 : bft_fail(BFT_GPU_E_ARG, "threading: n_rows is not the index's k-mer count (" + std::to_string(h->n_kmers) + ")");
}
template <class K, class... A>
static int th_launch_plain(K kernel, uint64_t blocks, hipStream_t s, const A&... args) {  // (the front's kernels stride by blockDim)
    hipLaunchKernelGGL(kernel, dim3(bft_grid_for(blocks)), dim3(256), 0, s, args...);
    HIPCK(hipGetLastError());
    return 0;
}

// Everything that counts: d_counts (64 bytes) complete; loc, flags and both scans in the scratch
static int th_count(bft_gpu* h, const char* d_seqs, const uint64_t* d_seq_off, uint64_t n_seqs, uint64_t n_chars, const ThGraph& g, hipStream_t s,
                    unsigned long long* d_counts, const BftThScratch& p, ThBatch* batch) {
    const int W = h->W, k = h->k, sb = bft_sp_bucket_bits(k);
    const uint64_t n = h->n_kmers, n_cw = (n_chars + 31) / 32;
    const uint64_t* tk = h->d_tk.as<uint64_t>();
    const double cd = (double)n_chars;
    CK(bft_zero_async(d_counts, 64, s));
    // (the slack words behind the codes are read by windows at the very end of the blob: keep them defined)
    CK(bft_zero_async(p.codes + n_cw, (BFT_MAX_W + 2) * 8, s));
    CK(bft_zero_async(p.bad + n_cw, (BFT_MAX_W + 2) * 4, s));
    if (n_cw) CK(bft_timed_launch(h, s, [&] { return th_launch_plain(k_seq_encode, (n_cw + 255) / 256, s, d_seqs, n_chars, n_cw, p.codes, p.bad); }));
    bft_stage("threading: encode", cd * (1 + 0.375), s);
    CK(bft_timed_launch(h, s, [&] {  // the plan: positions per sequence, their offsets, the tile table
        CK(th_launch_plain(k_seq_plan, (n_seqs + 256) / 256, s, d_seq_off, n_seqs, k, p.npos));
        CK(bft_scan::exclusive_sum_ptr<uint64_t>(p.npos, p.poff, n_seqs + 1, s, h->th_tmp));
        return th_launch_plain(k_seq_tiles, 256 * 4, s, (const uint64_t*)p.poff, (uint32_t)n_seqs, p.tile);
    }));
    bft_stage("threading: plan", (double)n_seqs * 32, s);
    // the unitigs' front kernels, into this call's own scratch (the paths' block is not touched)
    CK(bft_timed_launch(h, s, [&] { return bft_ug_canonicity(W, tk, n, k, d_counts + 7, s); }));
    bft_stage("threading: canonicity", (double)n * 8.0 * W, s);
    BftSpScratch buckets{};
    buckets.start = p.start;
    buckets.sb = sb;
    CK(bft_timed_launch(h, s, [&] { return bft_sp_buckets(W, tk, n, k, buckets, s); }));
    bft_stage("threading: buckets of the table", (double)((1ull << sb) + 1) * 4, s);
    const ThBatch b{p.codes, p.bad, d_seq_off, p.poff, p.tile, (uint32_t)n_seqs, n_chars};
    *batch = b;
    CK(bft_timed_launch(h, s, [&] {
        return bft_for_w(W, [&](auto KW) { return bft_launch256(k_th_locate<KW>, std::max<uint64_t>(n_chars, 1), s, tk, sb, (const uint32_t*)p.start, b, g, p.loc, d_counts); });
    }));
    bft_stage("threading: locate", 0, s);  // (one bucketed lower bound per position: no streaming stage)
    CK(bft_timed_launch(h, s, [&] { return bft_launch256(k_th_flags, n_chars, s, b, g, (const uint2*)p.loc, p.flag, d_counts); }));
    bft_stage("threading: transitions", cd * (8 + 1), s);
    CK(bft_timed_launch(h, s, [&] { return bft_scan::exclusive_sum<uint32_t>(BftThFlag<BFT_TH_WALK>{p.flag}, p.widx, n_chars, s, h->th_tmp, d_counts + 0, false); }));
    CK(bft_timed_launch(h, s, [&] { return bft_scan::exclusive_sum<uint32_t>(BftThFlag<BFT_TH_STEP>{p.flag}, p.sidx, n_chars, s, h->th_tmp, d_counts + 1, false); }));
    bft_stage("threading: scans of the walk and step starts", 2 * cd * (1 + 4), s);
    return 0;
}
static int th_emit(bft_gpu* h, const ThBatch& b, const BftThScratch& p, const unsigned long long* d_counts, uint64_t* d_walks, uint64_t* d_walk_off, uint64_t walks_cap,
                   uint32_t* d_steps, uint64_t steps_cap, hipStream_t s) {
    const bool any = d_walks || d_walk_off || d_steps;
    if (any)
        CK(bft_timed_launch(h, s, [&] {
            return bft_launch256(k_th_emit, std::max<uint64_t>(b.n_chars, 1), s, b, (const uint2*)p.loc, (const uint8_t*)p.flag, (const uint32_t*)p.widx, (const uint32_t*)p.sidx,
                                 d_counts, d_walks, d_walk_off, walks_cap, d_steps, steps_cap);
        }));
    if (d_walks && walks_cap)
        CK(bft_timed_launch(h, s, [&] { return bft_launch256(k_th_close, b.n_chars, s, b.n_chars, (const uint8_t*)p.flag, (const uint32_t*)p.widx, d_walks, walks_cap); }));
    bft_stage("threading: walks and steps", any ? (double)b.n_chars * (1 + 1) : 0, s);  // (the flags, twice; indexes, loc and records of the lanes that are set)
    return 0;
}

extern "C" int bft_gpu_thread_sequences_dev(bft_gpu* h, const void* d_seqs, const void* d_seq_off, uint64_t nb_seqs, uint64_t total_chars, const void* d_seg_of,
                                            const void* d_pos, uint64_t n_rows, const void* d_seg_off, uint64_t n_segments, const void* d_link_off, const void* d_links,
                                            uint64_t n_links, void* d_walks, void* d_walk_off, uint64_t walks_cap, void* d_steps, uint64_t steps_cap, void* d_counts,
                                            void* hip_stream) {
    if (!h || !d_counts || (nb_seqs && !d_seq_off) || (total_chars && !d_seqs) || (n_rows && (!d_seg_of || !d_pos)) || (n_segments && (!d_seg_off || !d_link_off)) ||
        (n_segments && n_links && !d_links))
        return bft_fail(BFT_GPU_E_ARG, "NULL argument");
    CK(th_check_sizes(nb_seqs, total_chars, n_segments));
    ENTER(h);
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : h->stream;
    if (bft_stream_capturing(s)) return bft_fail(BFT_GPU_E_ARG, TH_CAPTURE_MSG);
    CK(th_prepare(h, n_rows));
    {
        const ThGraph g{(const uint32_t*)d_seg_of, (const uint32_t*)d_pos, (const uint64_t*)d_seg_off, (const uint64_t*)d_link_off, (const uint32_t*)d_links, 2 * n_segments,
                        n_links, h->k};
        HandleScratch::Lease lease(h->th);
        BftThScratch p;
        ThBatch b;
        CK(th_scratch(h, lease, nb_seqs, total_chars, s, &p));
        StageScope stage_scope(h, s);
        CK(th_count(h, (const char*)d_seqs, (const uint64_t*)d_seq_off, nb_seqs, total_chars, g, s, (unsigned long long*)d_counts, p, &b));
        CK(th_emit(h, b, p, (const unsigned long long*)d_counts, (uint64_t*)d_walks, (uint64_t*)d_walk_off, walks_cap, (uint32_t*)d_steps, steps_cap, s));
    }
    return bft_note_foreign_stream(h, s);
}

// The host-buffer form: the arrays are checked and uploaded, the walks counted on the device, and the outputs filled only when the caps hold them all.
extern "C" int bft_gpu_thread_sequences(bft_gpu* h, const char* seqs, const uint64_t* seq_off, uint64_t nb_seqs, const uint32_t* seg_of, const uint32_t* pos,
                                        uint64_t n_rows, const uint64_t* seg_off, uint64_t n_segments, const uint64_t* link_off, const uint32_t* links, uint64_t n_links,
                                        uint64_t* walks, uint64_t* walk_off, uint64_t walks_cap, uint32_t* steps, uint64_t steps_cap, uint64_t counts[8]) {
    if (!h || !counts || (nb_seqs && (!seq_off || !seqs)) || (n_rows && (!seg_of || !pos)) || (n_segments && (!seg_off || !link_off)) || (n_segments && n_links && !links))
        return bft_fail(BFT_GPU_E_ARG, "NULL argument");
    for (uint64_t i = 0; i < nb_seqs; i++)
        if (seq_off[i + 1] < seq_off[i]) return bft_fail(BFT_GPU_E_ARG, "threading: sequence offsets must not decrease");
    const uint64_t c0 = nb_seqs ? seq_off[0] : 0, nc = nb_seqs ? seq_off[nb_seqs] - c0 : 0;  // (the blob is read from the first sequence on)
    CK(th_check_sizes(nb_seqs, nc, n_segments));
    ENTER(h);
    CK(th_prepare(h, n_rows));
    const uint64_t n2 = 2 * n_segments;
    if (n_segments) {
        for (uint64_t a = 0; a < n2; a++)
            if (link_off[a + 1] < link_off[a]) return bft_fail(BFT_GPU_E_ARG, "threading: link offsets must not decrease");
        if (link_off[n2] != n_links) return bft_fail(BFT_GPU_E_ARG, "threading: the last link offset must be n_links");
        for (uint64_t j = link_off[0]; j < n_links; j++)
            if (links[j] >= n2) return bft_fail(BFT_GPU_E_ARG, "threading: a link target is no oriented segment");
        for (uint64_t i = 0; i < n_segments; i++)
            if (seg_off[i + 1] < seg_off[i] + (uint64_t)h->k) return bft_fail(BFT_GPU_E_ARG, "threading: segment offsets must grow by k characters or more");
    }
    for (int i = 0; i < 8; i++) counts[i] = 0;
    const hipStream_t s = h->stream;
    DevBuf dseq, dqo, dsg, dps, dso, dlo, dln, dcnt, dwalks, dwoff, dsteps;
    std::vector<uint64_t> rel;  // the offsets from the first sequence's first character
    if (c0) {
        rel.assign(seq_off, seq_off + nb_seqs + 1);
        for (uint64_t& v : rel) v -= c0;
    }
    CK(dseq.alloc(nc));
    CK(dqo.alloc((nb_seqs + 1) * 8));
    CK(dsg.alloc(n_rows * 4));
    CK(dps.alloc(n_rows * 4));
    CK(dso.alloc((n_segments + 1) * 8));
    CK(dlo.alloc((n2 + 1) * 8));
    CK(dln.alloc(n_links * 4));
    CK(dcnt.alloc(64));
    if (nc) HIPCK(hipMemcpyAsync(dseq.p, seqs + c0, nc, hipMemcpyHostToDevice, s));
    if (nb_seqs) HIPCK(hipMemcpyAsync(dqo.p, c0 ? rel.data() : seq_off, (nb_seqs + 1) * 8, hipMemcpyHostToDevice, s));
    if (n_rows) {
        HIPCK(hipMemcpyAsync(dsg.p, seg_of, n_rows * 4, hipMemcpyHostToDevice, s));
        HIPCK(hipMemcpyAsync(dps.p, pos, n_rows * 4, hipMemcpyHostToDevice, s));
    }
    if (n_segments) {
        HIPCK(hipMemcpyAsync(dso.p, seg_off, (n_segments + 1) * 8, hipMemcpyHostToDevice, s));
        HIPCK(hipMemcpyAsync(dlo.p, link_off, (n2 + 1) * 8, hipMemcpyHostToDevice, s));
        if (n_links) HIPCK(hipMemcpyAsync(dln.p, links, n_links * 4, hipMemcpyHostToDevice, s));
    }
    const ThGraph g{dsg.as<uint32_t>(), dps.as<uint32_t>(), dso.as<uint64_t>(), dlo.as<uint64_t>(), dln.as<uint32_t>(), n2, n_links, h->k};
    HandleScratch::Lease lease(h->th);
    BftThScratch p;
    ThBatch b;
    CK(th_scratch(h, lease, nb_seqs, nc, s, &p));
    StageScope stage_scope(h);
    CK(th_count(h, dseq.as<char>(), dqo.as<uint64_t>(), nb_seqs, nc, g, s, dcnt.as<unsigned long long>(), p, &b));
    unsigned long long cnt[8];
    HIPCK(hipMemcpyAsync(cnt, dcnt.p, sizeof cnt, hipMemcpyDeviceToHost, s));
    HIPCK(hipStreamSynchronize(s));
    for (int i = 0; i < 8; i++) counts[i] = cnt[i];
    if (cnt[7]) return bft_fail(BFT_GPU_E_STATE, "threading: the index is not canonical (" + std::to_string(cnt[7]) + " k-mers above their reverse complement)");
    if (((walks || walk_off) && cnt[0] > walks_cap) || (steps && cnt[1] > steps_cap)) return bft_fail(BFT_GPU_E_NOSPACE, "threading buffers too small");
    if (!walks && !walk_off && !steps) return BFT_GPU_OK;
    if (walks) CK(dwalks.alloc(cnt[0] * 32));
    if (walk_off) CK(dwoff.alloc((cnt[0] + 1) * 8));
    if (steps) CK(dsteps.alloc(cnt[1] * 4));
    CK(th_emit(h, b, p, dcnt.as<unsigned long long>(), walks ? dwalks.as<uint64_t>() : nullptr, walk_off ? dwoff.as<uint64_t>() : nullptr, cnt[0],
               steps ? dsteps.as<uint32_t>() : nullptr, cnt[1], s));
    if (walks && cnt[0]) HIPCK(hipMemcpyAsync(walks, dwalks.p, cnt[0] * 32, hipMemcpyDeviceToHost, s));
    if (walk_off) HIPCK(hipMemcpyAsync(walk_off, dwoff.p, (cnt[0] + 1) * 8, hipMemcpyDeviceToHost, s));
    if (steps && cnt[1]) HIPCK(hipMemcpyAsync(steps, dsteps.p, cnt[1] * 4, hipMemcpyDeviceToHost, s));
    HIPCK(hipStreamSynchronize(s));
    return BFT_GPU_OK;
}
