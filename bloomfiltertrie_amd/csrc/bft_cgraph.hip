// bft_cgraph.hip -- the compacted coloured graph of a canonical index: segments (the unitigs and the branching k-mers), links between oriented
// segments, members, a colour row per segment (bft_gpu_unitig_graph / _dev, bft_gpu_unitig_colors / _dev; include/bft_gpu.h defines them).
// The front, the jumps and the ends are the unitigs' (bft_unitigs.hip through the path engine, bft_paths.hip).  Then
//   k_cg_singles  one lane per row: an eligible row that is no node becomes a kept path of its one vertex (s, 0) -- {head, distance} = {(s, 0), 0},
//                 length k -- so the engine's two scans, k_sp_offsets<true> and k_sp_spell<true> number, place and spell unitigs and singles together, in
//                 ascending id of the first vertex, with no kernel of their own
//   k_cg_members  one lane per vertex of a kept path: its id at member offset + distance; the head and the tail of a path write the ends of the two
//                 oriented segments (the last vertex of (i, 0) is the tail, of (i, 1) the flip of the head)
//   k_cg_links    one lane per oriented segment end, dense (2 x segments lanes, not 2n): the successor words of the end as k_ug_degrees searches them
//                 (one interval of the table, an exact lookup for each word the interval did not hold), every hit kept: the oriented segment that
//                 starts with it, where the two colour sets share min_shared genomes (sp_shared); the at most four targets sorted in registers
//   (a scan over the targets that are set: where every link list begins, the number of links)
//   k_cg_emit     link_off and links below their caps
//   k_cg_groups   the colours' front: character offsets -> member offsets, members -> colour-set ids; the reduction is bft_setops.hip's
// No kernel needs LDS or scratch memory.
#include "bft_cgraph.h"
#include "bft_dev.h"
#include "bft_handle.h"
#include "bft_scan.h"
#include "bft_setops.h"
#include "bft_succ.h"
#include "bft_unitigs.h"

namespace {

__global__ __launch_bounds__(BFT_LAUNCH_THREADS) void k_cg_singles(uint32_t n, int k, uint32_t t, const uint32_t* __restrict__ tcol, const uint32_t* __restrict__ cs_off,
                                                                   const uint8_t* __restrict__ flags, uint2* __restrict__ hd, uint32_t* __restrict__ len,
                                                                   unsigned long long* __restrict__ counts) {
    // (every lane of a wavefront runs the same iterations: the wavefront's count is a ballot per iteration, summed over its whole grid-stride loop --
    // ONE atomic per wavefront of the grid, 8192 at the most: one per wavefront and iteration serialises on the one address, 15.7 ms for the 7x10^5
    // wavefronts of the config-3 index where most hold a branching k-mer)
    uint32_t singles = 0;
    for (uint64_t i0 = blockIdx.x * (uint64_t)BFT_LAUNCH_THREADS + (threadIdx.x & ~63u); i0 < n; i0 += (uint64_t)gridDim.x * BFT_LAUNCH_THREADS) {
        const uint64_t i = i0 + (threadIdx.x & 63u);
        bool single = false;
        if (i < n) {
            single = !(flags[2 * i] & BFT_SP_NODE) && (t == 0u || sp_set_size(cs_off, tcol[i]) >= t);
            if (single) {
                hd[2 * i] = make_uint2((uint32_t)(2 * i), 0u);
                len[2 * i] = (uint32_t)k;
            }
        }
        singles += (uint32_t)__popcll(__ballot(single));
    }
    if ((threadIdx.x & 63u) == 0 && singles) {
        atomicAdd(counts + 5, (unsigned long long)singles);
        if ((unsigned long long)k > __hip_atomic_load(counts + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(counts + 2, (unsigned long long)k);
    }
}

__global__ __launch_bounds__(BFT_LAUNCH_THREADS) void k_cg_members(uint32_t nv, int k, const uint2* __restrict__ hd, const uint32_t* __restrict__ len,
                                                                   const uint32_t* __restrict__ pid, const uint64_t* __restrict__ choff,
                                                                   uint32_t* __restrict__ members, uint64_t members_cap, uint32_t* __restrict__ endv) {
    for (uint64_t i = blockIdx.x * (uint64_t)BFT_LAUNCH_THREADS + threadIdx.x; i < nv; i += (uint64_t)gridDim.x * BFT_LAUNCH_THREADS) {
        const uint2 o = hd[i];
        if (o.x == BFT_SP_NONE) continue;
        const uint32_t L = len[o.x];
        if (L == 0u) continue;  // (the mirror that is not reported)
        const uint64_t seg = pid[o.x];
        if (members) {
            const uint64_t pos = choff[o.x] - seg * (uint64_t)(k - 1) + o.y;
            if (pos < members_cap) members[pos] = (uint32_t)i;
        }
        // (2 * seg + 1 < nv on a canonical index: every row lies in one segment)
        if (o.y == 0u && 2 * seg + 1 < nv) endv[2 * seg + 1] = (uint32_t)i ^ 1u;
        if (o.y == L - (uint32_t)k && 2 * seg < nv) endv[2 * seg] = (uint32_t)i;
    }
}

// the oriented segment whose first vertex is w: w heads a kept path, or its flip is the tail of one
__device__ __forceinline__ uint32_t cg_first(uint32_t w, int k, const uint2* hd, const uint32_t* len, const uint32_t* pid) {
    uint2 o = hd[w];
    if (o.x != BFT_SP_NONE && len[o.x] != 0u) return o.y == 0u ? 2u * pid[w] : BFT_SP_NONE;
    o = hd[w ^ 1u];
    if (o.x == BFT_SP_NONE) return BFT_SP_NONE;
    const uint32_t L = len[o.x];
    return L != 0u && o.y == L - (uint32_t)k ? 2u * pid[o.x] + 1u : BFT_SP_NONE;
}

__device__ __forceinline__ void cg_cswap(uint32_t& a, uint32_t& b) {
    const uint32_t lo = min(a, b), hi = max(a, b);
    a = lo;
    b = hi;
}

template <int W>
__global__ __launch_bounds__(BFT_LAUNCH_THREADS) void k_cg_links(const uint64_t* __restrict__ tk, uint32_t n, int k, int sb, const uint32_t* __restrict__ start, uint32_t t,
                                                                 const uint32_t* __restrict__ tcol, const uint32_t* __restrict__ cs_off, const void* __restrict__ cs_ids,
                                                                 uint32_t cs_w, const uint2* __restrict__ hd, const uint32_t* __restrict__ len,
                                                                 const uint32_t* __restrict__ pid, const uint32_t* __restrict__ endv,
                                                                 const unsigned long long* __restrict__ counts, uint32_t nv, uint4* __restrict__ tgt) {
    const uint64_t na = min(2ull * counts[0], (unsigned long long)nv);
    for (uint64_t a = blockIdx.x * (uint64_t)BFT_LAUNCH_THREADS + threadIdx.x; a < na; a += (uint64_t)gridDim.x * BFT_LAUNCH_THREADS) {
        const uint32_t e = endv[a], row = e >> 1;
        uint32_t b0 = BFT_SP_NONE, b1 = BFT_SP_NONE, b2 = BFT_SP_NONE, b3 = BFT_SP_NONE;
        if (row < n) {
            uint64_t tf[W], x[W], w[W];
            bft_load_row<W>(tk + (uint64_t)row * W, tf);
            bft_x_from_tform<W>(tf, k, x);
            if (e & 1u) bft_x_revcomp<W>(x, k, w);
            else {
#pragma unroll
                for (int q = 0; q < W; q++) w[q] = x[q];
            }
            const uint32_t ce = tcol[row];
            // the target behind successor vertex v, found as the word with nucleotide c last
            auto keep = [&](uint32_t v, uint32_t c) {
                uint32_t b = cg_first(v, k, hd, len, pid);
                if (b != BFT_SP_NONE && !sp_shared(ce, tcol[v >> 1], t, cs_off, cs_ids, cs_w)) b = BFT_SP_NONE;
                b0 = c == 0u ? b : b0;
                b1 = c == 1u ? b : b1;
                b2 = c == 2u ? b : b2;
                b3 = c == 3u ? b : b3;
            };
            uint32_t have = 0;
            // the stored successor words: row r holds the one with nucleotide c last (a palindromic one is found here: the vertex (y, 0))
            bft_for_each_successor_of<W>(tk, n, k, sb, start, w, [&](uint32_t r, uint32_t c) {
                have |= 1u << c;
                keep(2u * r, c);
            });
            // the others, as stored reverse complements: comp(N) + rc(w)[0..k-2]
            uint64_t y[W], z[W];
#pragma unroll
            for (int q = 0; q < W; q++) y[q] = (w[q] >> 2) | (q + 1 < W ? w[q + 1] << 62 : 0ull);
            bft_x_revcomp<W>(y, k, z);
            for (uint32_t c = 0; c < 4; c++) {
                if ((have >> c) & 1u) continue;
                z[0] = (z[0] & ~3ull) | (uint64_t)(3u - c);
                const uint32_t r = bft_find_row<W>(tk, k, sb, start, z);
                if (r != BFT_SP_NONE) keep(2u * r + 1u, c);
            }
            cg_cswap(b0, b1);
            cg_cswap(b2, b3);
            cg_cswap(b0, b2);
            cg_cswap(b1, b3);
            cg_cswap(b1, b2);
        }
        tgt[a] = make_uint4(b0, b1, b2, b3);
    }
}

__global__ __launch_bounds__(BFT_LAUNCH_THREADS) void k_cg_emit(uint32_t nv, const unsigned long long* __restrict__ counts, const uint4* __restrict__ tgt,
                                                                const uint64_t* __restrict__ loff, uint64_t* __restrict__ link_off, uint64_t seg_cap,
                                                                uint32_t* __restrict__ links, uint64_t links_cap) {
    const uint64_t ns = counts[0], na = min(2ull * ns, (unsigned long long)nv);
    if (blockIdx.x == 0 && threadIdx.x == 0 && link_off && ns <= seg_cap) link_off[2 * ns] = counts[4];
    for (uint64_t a = blockIdx.x * (uint64_t)BFT_LAUNCH_THREADS + threadIdx.x; a < na; a += (uint64_t)gridDim.x * BFT_LAUNCH_THREADS) {
        const uint64_t at = loff[a];
        if (link_off && a <= 2 * seg_cap) link_off[a] = at;
        if (!links) continue;
        const uint4 b = tgt[a];
        if (b.x != BFT_SP_NONE && at < links_cap) links[at] = b.x;
        if (b.y != BFT_SP_NONE && at + 1 < links_cap) links[at + 1] = b.y;
        if (b.z != BFT_SP_NONE && at + 2 < links_cap) links[at + 2] = b.z;
        if (b.w != BFT_SP_NONE && at + 3 < links_cap) links[at + 3] = b.w;
    }
}

// cs[j] = the colour set of member j's row (a member outside the table: the absent k-mer); goff[g] = seg_off[g] - g (k - 1)
__global__ __launch_bounds__(BFT_LAUNCH_THREADS) void k_cg_groups(uint64_t n_members, uint64_t n_segments, int k, uint32_t nv, const uint32_t* __restrict__ members,
                                                                  const uint64_t* __restrict__ seg_off, const uint32_t* __restrict__ tcol, uint32_t* __restrict__ cs,
                                                                  uint64_t* __restrict__ goff) {
    const uint64_t items = max(n_members, n_segments + 1);
    for (uint64_t i = blockIdx.x * (uint64_t)BFT_LAUNCH_THREADS + threadIdx.x; i < items; i += (uint64_t)gridDim.x * BFT_LAUNCH_THREADS) {
        if (i < n_members) {
            const uint32_t m = members[i];
            cs[i] = m < nv ? tcol[m >> 1] : BFT_SO_ABSENT;
        }
        if (i <= n_segments) {
            // (offsets that are no segment offsets: whatever comes out, the reduction treats a group that ends before it starts or past the batch as empty)
            const uint64_t o = seg_off[i], sub = i * (uint64_t)(k - 1);
            goff[i] = o >= sub ? o - sub : 0ull;
        }
    }
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// the graph: the chain of launches, the two forms of the entry point
// ------------------------------------------------------------------------------------------------
static int cg_front(bft_gpu* h, uint32_t t, hipStream_t s, unsigned long long* d_counts, const BftSpScratch& p) { return bft_ug_front(h, "unitig graph", t, s, d_counts, p); }
// d_counts = {n_segments, n_chars, longest, non-canonical rows, n_links, singles}
static const BftPathFamily CG_FAMILY = {
    true,
    48,
    "unitig graph",
    "unitig graph: heads, tails, lengths, the kept mirror",
    "unitig graph recorded into a graph: not supported (the table may have to come back, scratch may grow)",
    "unitig graph buffers too small",
    cg_front,
    bft_ug_check,
};

static int cg_members(bft_gpu* h, const BftSpScratch& p, const BftCgScratch& c, uint32_t* d_members, uint64_t members_cap, hipStream_t s) {
    const uint64_t nv = 2 * h->n_kmers;
    return bft_timed_launch(h, s, [&] { return bft_launch256(k_cg_members, nv, s, (uint32_t)nv, h->k, (const uint2*)c.hd, (const uint32_t*)p.indeg, (const uint32_t*)p.pred, (const uint64_t*)p.choff, d_members, members_cap, c.endv); });
}

// Everything that counts: segments numbered and placed, ends (and members below members_cap, where d_members is not null), link targets, where the
// link lists begin.  d_counts (48 bytes) complete; *fin: the jumps' last buffer
static int cg_count(bft_gpu* h, uint32_t t, hipStream_t s, unsigned long long* d_counts, const BftSpScratch& p, int* fin, uint32_t* d_members, uint64_t members_cap) {
    const uint64_t n = h->n_kmers, nv = 2 * n;
    const double nd = (double)n, vd = (double)nv;
    const uint32_t* tcol = h->d_tcol.as<uint32_t>();
    const uint32_t* cs_off = h->d_cs_off.as<uint32_t>();
    CK(bft_paths_trace(h, CG_FAMILY, t, s, d_counts, p, fin));
    const BftCgScratch c = bft_cg_scratch(p, *fin, nv);
    CK(bft_timed_launch(h, s, [&] { return bft_launch256(k_cg_singles, n, s, (uint32_t)n, h->k, t, tcol, cs_off, (const uint8_t*)p.flags, c.hd, p.indeg, d_counts); }));
    bft_stage("unitig graph: single-k-mer segments", nd * (1 + (t ? 8 : 0)), s);
    CK(bft_paths_number(h, CG_FAMILY, s, d_counts, p, *fin));
    CK(cg_members(h, p, c, d_members, members_cap, s));
    bft_stage("unitig graph: members and segment ends", vd * (8 + 4) + nd * (4 + 8 + (d_members ? 4 : 0)), s);
    CK(bft_timed_launch(h, s, [&] {
        return bft_for_w(h->W, [&](auto KW) {
            return bft_launch256(k_cg_links<KW>, nv, s, h->d_tk.as<uint64_t>(), (uint32_t)n, h->k, p.sb, (const uint32_t*)p.start, t, tcol, cs_off, (const void*)h->d_cs_ids.p,
                                 h->cs_w, (const uint2*)c.hd, (const uint32_t*)p.indeg, (const uint32_t*)p.pred, (const uint32_t*)c.endv,
                                 (const unsigned long long*)d_counts, (uint32_t)nv, c.tgt);
        });
    }));
    bft_stage("unitig graph: link targets", 0, s);  // (per segment end, not per vertex: no streaming stage)
    CK(bft_timed_launch(h, s, [&] { return bft_scan::exclusive_sum<uint64_t>(BftCgLinkCount{c.tgt, d_counts, nv}, c.loff, nv, s, h->sp_tmp, d_counts + 4, false); }));
    bft_stage("unitig graph: scan of the link lists", vd * 8, s);
    return 0;
}
// the outputs that are not null, below their caps (d_members: written by cg_count where it was given there)
static int cg_emit(bft_gpu* h, const BftSpScratch& p, int fin, uint64_t* d_seg_off, char* d_seqs, uint64_t* d_link_off, uint32_t* d_links, uint64_t seg_cap,
                   uint64_t chars_cap, uint64_t links_cap, const unsigned long long* d_counts, hipStream_t s) {
    const uint64_t nv = 2 * h->n_kmers;
    const BftCgScratch c = bft_cg_scratch(p, fin, nv);
    CK(bft_paths_emit(h, CG_FAMILY, p, fin, d_seg_off, seg_cap, d_seqs, chars_cap, d_counts, s));
    if (d_link_off || d_links)
        CK(bft_timed_launch(h, s, [&] { return bft_launch256(k_cg_emit, nv, s, (uint32_t)nv, d_counts, (const uint4*)c.tgt, (const uint64_t*)c.loff, d_link_off, seg_cap, d_links, links_cap); }));
    bft_stage("unitig graph: links", 0, s);
    return 0;
}

extern "C" int bft_gpu_unitig_graph_dev(bft_gpu* h, uint32_t min_shared, void* d_seg_off, void* d_seqs, void* d_link_off, void* d_links, void* d_members, uint64_t seg_cap,
                                        uint64_t chars_cap, uint64_t links_cap, uint64_t members_cap, void* d_counts, void* hip_stream) {
    if (!h || !d_counts) return bft_fail(BFT_GPU_E_ARG, "NULL argument");
    ENTER(h);
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : h->stream;
    if (bft_stream_capturing(s)) return bft_fail(BFT_GPU_E_ARG, CG_FAMILY.capture_msg);
    CK(bft_sp_prepare(h, CG_FAMILY.name));
    if (h->n_kmers == 0) {
        CK(bft_zero_async(d_counts, CG_FAMILY.counts_bytes, s));
        if (d_seg_off) CK(bft_zero_async(d_seg_off, 8, s));
        if (d_link_off) CK(bft_zero_async(d_link_off, 8, s));
        return bft_note_foreign_stream(h, s);
    }
    {
        HandleScratch::Lease lease(h->sp);
        BftSpScratch p;
        CK(bft_paths_scratch(h, CG_FAMILY, lease, s, &p));
        StageScope stage_scope(h, s);
        int fin = 0;
        CK(cg_count(h, min_shared, s, (unsigned long long*)d_counts, p, &fin, (uint32_t*)d_members, members_cap));
        CK(cg_emit(h, p, fin, (uint64_t*)d_seg_off, (char*)d_seqs, (uint64_t*)d_link_off, (uint32_t*)d_links, seg_cap, chars_cap, links_cap, (const unsigned long long*)d_counts, s));
    }
    return bft_note_foreign_stream(h, s);
}

// The host-buffer form: everything is counted on the device, and the outputs filled only when the index is canonical and the caps hold them all.
extern "C" int bft_gpu_unitig_graph(bft_gpu* h, uint32_t min_shared, uint64_t* seg_off, char* seqs, uint64_t* link_off, uint32_t* links, uint32_t* members, uint64_t seg_cap,
                                    uint64_t chars_cap, uint64_t links_cap, uint64_t members_cap, uint64_t counts[6]) {
    if (!h || !counts) return bft_fail(BFT_GPU_E_ARG, "NULL argument");
    ENTER(h);
    CK(bft_sp_prepare(h, CG_FAMILY.name));
    for (int i = 0; i < 6; i++) counts[i] = 0;
    if (h->n_kmers == 0) {
        if (seg_off) seg_off[0] = 0;
        if (link_off) link_off[0] = 0;
        return BFT_GPU_OK;
    }
    const hipStream_t s = h->stream;
    DevBuf dcnt;
    CK(dcnt.alloc(CG_FAMILY.counts_bytes));
    HandleScratch::Lease lease(h->sp);
    BftSpScratch p;
    CK(bft_paths_scratch(h, CG_FAMILY, lease, s, &p));
    StageScope stage_scope(h);
    int fin = 0;
    CK(cg_count(h, min_shared, s, dcnt.as<unsigned long long>(), p, &fin, nullptr, 0));
    unsigned long long cnt[6] = {0, 0, 0, 0, 0, 0};
    HIPCK(hipMemcpyAsync(cnt, dcnt.p, sizeof cnt, hipMemcpyDeviceToHost, s));
    HIPCK(hipStreamSynchronize(s));
    for (int i = 0; i < 6; i++) counts[i] = cnt[i];
    CK(bft_ug_check(cnt));
    const uint64_t ns = cnt[0], nc = cnt[1], nl = cnt[4], nm = nc - ns * (uint64_t)(h->k - 1);
    if (((seg_off || link_off) && ns > seg_cap) || (seqs && nc > chars_cap) || (links && nl > links_cap) || (members && nm > members_cap))
        return bft_fail(BFT_GPU_E_NOSPACE, CG_FAMILY.nospace_msg);
    if (!seg_off && !seqs && !link_off && !links && !members) return BFT_GPU_OK;
    DevBuf dso, dseq, dlo, dln, dmem;
    if (seg_off) CK(dso.alloc((ns + 1) * 8));
    if (seqs && nc) CK(dseq.alloc(nc));
    if (link_off) CK(dlo.alloc((2 * ns + 1) * 8));
    if (links && nl) CK(dln.alloc(nl * 4));
    if (members && nm) CK(dmem.alloc(nm * 4));
    if (dmem.p) CK(cg_members(h, p, bft_cg_scratch(p, fin, 2 * h->n_kmers), dmem.as<uint32_t>(), nm, s));
    CK(cg_emit(h, p, fin, seg_off ? dso.as<uint64_t>() : nullptr, dseq.as<char>(), link_off ? dlo.as<uint64_t>() : nullptr, dln.as<uint32_t>(), ns, nc, nl,
               dcnt.as<unsigned long long>(), s));
    if (seg_off) HIPCK(hipMemcpyAsync(seg_off, dso.p, (ns + 1) * 8, hipMemcpyDeviceToHost, s));
    if (dseq.p) HIPCK(hipMemcpyAsync(seqs, dseq.p, nc, hipMemcpyDeviceToHost, s));
    if (link_off) HIPCK(hipMemcpyAsync(link_off, dlo.p, (2 * ns + 1) * 8, hipMemcpyDeviceToHost, s));
    if (dln.p) HIPCK(hipMemcpyAsync(links, dln.p, nl * 4, hipMemcpyDeviceToHost, s));
    if (dmem.p) HIPCK(hipMemcpyAsync(members, dmem.p, nm * 4, hipMemcpyDeviceToHost, s));
    HIPCK(hipStreamSynchronize(s));
    return BFT_GPU_OK;
}

// ------------------------------------------------------------------------------------------------
// a colour row per segment: the members' colour sets and the groups' offsets, then the colour-set road of bft_setops.hip
// ------------------------------------------------------------------------------------------------
static int cg_check_op(int op) { return op >= BFT_GPU_SETOP_AND && op <= BFT_GPU_SETOP_SYMDIFF ? 0 : bft_fail(BFT_GPU_E_ARG, "unitig colours: op must be BFT_GPU_SETOP_AND, _OR or _SYMDIFF"); }

extern "C" int bft_gpu_unitig_colors_dev(bft_gpu* h, const void* d_members, uint64_t n_members, const void* d_seg_off, uint64_t n_segments, int op, void* d_rows,
                                         void* d_counts, void* hip_stream) {
    if (!h || (n_segments && !d_seg_off) || (n_members && n_segments && !d_members)) return bft_fail(BFT_GPU_E_ARG, "NULL argument");
    CK(cg_check_op(op));
    ENTER(h);
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : h->stream;
    if (bft_stream_capturing(s)) return bft_fail(BFT_GPU_E_ARG, "unitig colours recorded into a graph: not supported (the table may have to come back, scratch may grow)");
    CK(bft_sp_prepare(h, "unitig colours"));
    if (n_segments == 0 || (!d_rows && !d_counts)) return BFT_GPU_OK;
    // (of the handle's path scratch: the members' colour sets and the groups' offsets, in use until the reduction behind them on s is through)
    HandleScratch::Lease lease(h->sp);
    CK(lease.acquire(s, false));
    uint32_t* cs = nullptr;
    uint64_t* goff = nullptr;
    Carver c{nullptr};
    c.take(goff, (n_segments + 1) * 8);
    c.take(cs, n_members * 4);
    CK(h->sp.grow(h->sp_buf, c.off, 0));
    c = Carver{h->sp_buf.as<uint8_t>()};
    c.take(goff, (n_segments + 1) * 8);
    c.take(cs, n_members * 4);
    // ("build_stages": the stages of the call are the reduction's, bft_gpu_combine_colorsets_dev's)
    CK(bft_timed_launch(h, s, [&] {
        return bft_launch256(k_cg_groups, std::max(n_members, n_segments + 1), s, n_members, n_segments, h->k, (uint32_t)(2 * h->n_kmers), (const uint32_t*)d_members,
                             (const uint64_t*)d_seg_off, (const uint32_t*)h->d_tcol.as<uint32_t>(), cs, goff);
    }));
    CK(bft_gpu_combine_colorsets_dev(h, cs, n_members, goff, n_segments, op, d_rows, d_counts, s));
    return bft_note_foreign_stream(h, s);
}

extern "C" int bft_gpu_unitig_colors(bft_gpu* h, const uint32_t* members, uint64_t n_members, const uint64_t* seg_off, uint64_t n_segments, int op, uint8_t* rows,
                                     uint32_t* counts) {
    if (!h || (n_segments && !seg_off) || (n_members && n_segments && !members)) return bft_fail(BFT_GPU_E_ARG, "NULL argument");
    CK(cg_check_op(op));
    ENTER(h);
    CK(bft_sp_prepare(h, "unitig colours"));
    const uint64_t km1 = (uint64_t)(h->k - 1);
    for (uint64_t g = 0; g < n_segments; g++)
        if (seg_off[g + 1] < seg_off[g] + km1 || seg_off[g] < g * km1) return bft_fail(BFT_GPU_E_ARG, "unitig colours: segment offsets must grow by k - 1 characters or more");
    if (n_segments && seg_off[n_segments] - n_segments * km1 > n_members) return bft_fail(BFT_GPU_E_ARG, "unitig colours: the last segment ends behind the members");
    for (uint64_t i = 0; i < n_members; i++)
        if (members[i] >= 2 * h->n_kmers) return bft_fail(BFT_GPU_E_ARG, "unitig colours: a member is no vertex of the index");
    if (n_segments == 0 || (!rows && !counts)) return BFT_GPU_OK;
    const hipStream_t s = h->stream;
    const uint32_t rb = (h->im.nb_genomes + 7) / 8;
    DevBuf dmem, doff, drows, dcnt;
    if (n_members) CK(dmem.alloc(n_members * 4));
    CK(doff.alloc((n_segments + 1) * 8));
    if (rows && rb) CK(drows.alloc(n_segments * rb));
    if (counts) CK(dcnt.alloc(n_segments * 4));
    if (n_members) HIPCK(hipMemcpyAsync(dmem.p, members, n_members * 4, hipMemcpyHostToDevice, s));
    HIPCK(hipMemcpyAsync(doff.p, seg_off, (n_segments + 1) * 8, hipMemcpyHostToDevice, s));
    CK(bft_gpu_unitig_colors_dev(h, dmem.p, n_members, doff.p, n_segments, op, drows.p, dcnt.p, s));
    if (drows.p) HIPCK(hipMemcpyAsync(rows, drows.p, n_segments * rb, hipMemcpyDeviceToHost, s));
    if (counts) HIPCK(hipMemcpyAsync(counts, dcnt.p, n_segments * 4, hipMemcpyDeviceToHost, s));
    HIPCK(hipStreamSynchronize(s));
    return BFT_GPU_OK;
}
