// bft_bubbles.hip -- simple bubbles (variants) on the compacted coloured graph and the k-mer -> segment table (bft_gpu_unitig_bubbles / _dev,
// bft_gpu_unitig_segment_of / _dev; include/bft_gpu.h defines them).  Both read what bft_gpu_unitig_graph returned: no kernel touches the index.
//   k_bb_find   one lane per oriented segment A: the definition's predicate, left at the first rule that fails (most lanes at m < 2: an end with fewer
//               than two links).  The at most four branches stay in four registers, the sink's in-links are tested against them with the 16
//               compares written out.  A flag per lane; branches, substitution shapes and the longest branch are summed per wavefront over its whole
//               grid-stride loop: one atomic per wavefront and statistic
//   (a scan over the flags of exactly 2S lanes: where every record goes, the number of bubbles)
//   k_bb_emit   the records below the cap: a flagged lane reads its links and its first branch's one link again
//   k_bb_fill   the k-mer -> segment table's rows to 0xFFFFFFFF
//   k_bb_segof  one lane per member: its segment by a lower bound over the member offsets seg_off[i] - i (k - 1), then the row's two entries
// No kernel needs LDS or scratch memory.
#include "bft_bubbles.h"
#include "bft_dev.h"
#include "bft_handle.h"
#include "bft_scan.h"

namespace {

// the graph as the caller gave it.  n2 = 2S <= 2^32 - 2; seqs holds seg_off[S] characters
struct BbGraph {
    const uint64_t* __restrict__ seg_off;
    const char* __restrict__ seqs;
    const uint64_t* __restrict__ link_off;
    const uint32_t* __restrict__ links;
    uint64_t n2, n_links, max_chars;
    int k;
};

// out(x) as {first entry, length}; false: no list inside links[0 .. n_links)
__device__ __forceinline__ bool bb_list(const BbGraph& g, uint32_t x, uint64_t& lo, uint64_t& m) {
    lo = g.link_off[x];
    const uint64_t hi = g.link_off[(uint64_t)x + 1];
    m = hi - lo;
    return lo <= hi && hi <= g.n_links;
}
// out(x) == [t]
__device__ __forceinline__ bool bb_only(const BbGraph& g, uint32_t x, uint32_t& t) {
    uint64_t lo, m;
    if (!bb_list(g, x, lo, m) || m != 1) return false;
    t = g.links[lo];
    return true;
}
// characters of segment i; false: its offsets are no stretch of seqs
__device__ __forceinline__ bool bb_chars(const BbGraph& g, uint32_t i, uint64_t n_chars, uint64_t& lo, uint64_t& len) {
    lo = g.seg_off[i];
    const uint64_t hi = g.seg_off[(uint64_t)i + 1];
    len = hi - lo;
    return lo <= hi && hi <= n_chars;
}
__device__ __forceinline__ char bb_comp(char c) { return c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : '\0'; }
// segment i is one k-mer that is its own reverse complement (even k only)
__device__ __forceinline__ bool bb_palindromic(const BbGraph& g, uint32_t i, uint64_t n_chars) {
    if (g.k & 1) return false;
    uint64_t lo, len;
    if (!bb_chars(g, i, n_chars, lo, len) || len != (uint64_t)g.k) return false;
    for (int j = 0; j < g.k / 2; j++)
        if (g.seqs[lo + j] != bb_comp(g.seqs[lo + g.k - 1 - j])) return false;
    return true;
}

// A is the source of a reported bubble: its branches (nb), the longest of them in characters, whether all have 2k - 1
__device__ __forceinline__ bool bb_source(const BbGraph& g, uint32_t A, uint32_t& nb, uint64_t& longest, bool& subst) {
    uint64_t lo, m;
    if (!bb_list(g, A, lo, m) || m < 2 || m > 4) return false;
    const uint32_t n2 = (uint32_t)g.n2;
    const uint32_t b0 = g.links[lo], b1 = g.links[lo + 1], b2 = m > 2 ? g.links[lo + 2] : BFT_BB_NONE, b3 = m > 3 ? g.links[lo + 3] : BFT_BB_NONE;
    if (b0 >= n2 || b1 >= n2 || (m > 2 && b2 >= n2) || (m > 3 && b3 >= n2)) return false;
    // every branch: one way out, the same Z for all
    uint32_t Z, z;
    if (!bb_only(g, b0, Z) || Z >= n2) return false;
    if (!(A < (Z ^ 1u))) return false;  // (the mirror reports it)
    if (!bb_only(g, b1, z) || z != Z) return false;
    if (m > 2 && (!bb_only(g, b2, z) || z != Z)) return false;
    if (m > 3 && (!bb_only(g, b3, z) || z != Z)) return false;
    // ... and one way in, from A
    if (!bb_only(g, b0 ^ 1u, z) || z != (A ^ 1u)) return false;
    if (!bb_only(g, b1 ^ 1u, z) || z != (A ^ 1u)) return false;
    if (m > 2 && (!bb_only(g, b2 ^ 1u, z) || z != (A ^ 1u))) return false;
    if (m > 3 && (!bb_only(g, b3 ^ 1u, z) || z != (A ^ 1u))) return false;
    // the sink: exactly m ways in, each the flip of a branch (an entry that is no oriented segment is none; a slot behind m: a branch)
    uint64_t zlo, zm;
    if (!bb_list(g, Z ^ 1u, zlo, zm) || zm != m) return false;
    const uint32_t l0 = g.links[zlo], l1 = g.links[zlo + 1], l2 = m > 2 ? g.links[zlo + 2] : b0 ^ 1u, l3 = m > 3 ? g.links[zlo + 3] : b0 ^ 1u;
    if (l0 >= n2 || l1 >= n2 || l2 >= n2 || l3 >= n2) return false;
    const uint32_t t0 = l0 ^ 1u, t1 = l1 ^ 1u, t2 = l2 ^ 1u, t3 = l3 ^ 1u;
    if (!((t0 == b0 || t0 == b1 || t0 == b2 || t0 == b3) && (t1 == b0 || t1 == b1 || t1 == b2 || t1 == b3) && (t2 == b0 || t2 == b1 || t2 == b2 || t2 == b3) &&
          (t3 == b0 || t3 == b1 || t3 == b2 || t3 == b3)))
        return false;
    // source, sink and branches: pairwise different segments
    const uint32_t sA = A >> 1, sZ = Z >> 1, s0 = b0 >> 1, s1 = b1 >> 1, s2 = b2 >> 1, s3 = b3 >> 1;
    bool same = sA == sZ || sA == s0 || sA == s1 || sZ == s0 || sZ == s1 || s0 == s1;
    if (m > 2) same |= sA == s2 || sZ == s2 || s0 == s2 || s1 == s2;
    if (m > 3) same |= sA == s3 || sZ == s3 || s0 == s3 || s1 == s3 || s2 == s3;
    if (same) return false;
    const uint64_t n_chars = g.seg_off[g.n2 >> 1];
    if (bb_palindromic(g, sA, n_chars) || bb_palindromic(g, sZ, n_chars)) return false;
    // the branches' characters
    uint64_t at, c0, c1, c2 = 0, c3 = 0;
    if (!bb_chars(g, s0, n_chars, at, c0) || !bb_chars(g, s1, n_chars, at, c1)) return false;
    if (m > 2 && !bb_chars(g, s2, n_chars, at, c2)) return false;
    if (m > 3 && !bb_chars(g, s3, n_chars, at, c3)) return false;
    longest = max(max(c0, c1), max(c2, c3));
    if (g.max_chars && longest > g.max_chars) return false;
    const uint64_t sub = 2ull * (uint64_t)g.k - 1ull;
    subst = c0 == sub && c1 == sub && (m < 3 || c2 == sub) && (m < 4 || c3 == sub);
    nb = (uint32_t)m;
    return true;
}

__device__ __forceinline__ uint64_t bb_shfl_xor64(uint64_t v, int o) {
    const uint32_t lo = __shfl_xor((uint32_t)v, o), hi = __shfl_xor((uint32_t)(v >> 32), o);
    return ((uint64_t)hi << 32) | lo;
}

// counts[1] += branches, counts[2] += bubbles of substitution shape, counts[3] = max(longest branch)
__global__ __launch_bounds__(BFT_LAUNCH_THREADS) void k_bb_find(BbGraph g, uint8_t* __restrict__ flag, unsigned long long* __restrict__ counts) {
    // (every lane of a wavefront runs the same iterations: what the wavefront found is summed over its whole grid-stride loop -- one atomic per
    // wavefront of the grid and statistic, not one per iteration on the one address, as k_cg_singles)
    uint32_t branches = 0, shaped = 0;
    uint64_t longest = 0;
    for (uint64_t i0 = blockIdx.x * (uint64_t)BFT_LAUNCH_THREADS + (threadIdx.x & ~63u); i0 < g.n2; i0 += (uint64_t)gridDim.x * BFT_LAUNCH_THREADS) {
        const uint64_t i = i0 + (threadIdx.x & 63u);
        bool is = false, subst = false;
        uint32_t nb = 0;
        uint64_t lg = 0;
        if (i < g.n2) {
            is = bb_source(g, (uint32_t)i, nb, lg, subst);
            flag[i] = is ? 1 : 0;
        }
        if (is) {
            branches += nb;
            longest = max(longest, lg);
        }
        shaped += (uint32_t)__popcll(__ballot(is && subst));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        branches += __shfl_xor(branches, o);
        longest = max(longest, bb_shfl_xor64(longest, o));
    }
    if ((threadIdx.x & 63u) == 0 && branches) {
        atomicAdd(counts + 1, (unsigned long long)branches);
        if (shaped) atomicAdd(counts + 2, (unsigned long long)shaped);
        if (longest > __hip_atomic_load(counts + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(counts + 3, (unsigned long long)longest);
    }
}

// {A, Z, B_1 .. B_4} of every flagged lane whose slot is below cap (k_bb_find proved the lists it reads again)
__global__ __launch_bounds__(BFT_LAUNCH_THREADS) void k_bb_emit(BbGraph g, const uint8_t* __restrict__ flag, const uint32_t* __restrict__ slot, uint32_t* __restrict__ bubbles,
                                                                uint64_t cap) {
    for (uint64_t a = blockIdx.x * (uint64_t)BFT_LAUNCH_THREADS + threadIdx.x; a < g.n2; a += (uint64_t)gridDim.x * BFT_LAUNCH_THREADS) {
        if (!flag[a]) continue;
        const uint64_t at = slot[a];
        if (at >= cap) continue;
        const uint64_t lo = g.link_off[a], m = g.link_off[a + 1] - lo;
        const uint32_t b0 = g.links[lo];
        uint32_t* const r = bubbles + 6 * at;
        r[0] = (uint32_t)a;
        r[1] = g.links[g.link_off[b0]];
        r[2] = b0;
        r[3] = g.links[lo + 1];
        r[4] = m > 2 ? g.links[lo + 2] : BFT_BB_NONE;
        r[5] = m > 3 ? g.links[lo + 3] : BFT_BB_NONE;
    }
}

__global__ __launch_bounds__(BFT_LAUNCH_THREADS) void k_bb_fill(uint64_t n, uint32_t* __restrict__ a, uint32_t* __restrict__ b) {
    for (uint64_t i = blockIdx.x * (uint64_t)BFT_LAUNCH_THREADS + threadIdx.x; i < n; i += (uint64_t)gridDim.x * BFT_LAUNCH_THREADS) {
        if (a) a[i] = BFT_BB_NONE;
        if (b) b[i] = BFT_BB_NONE;
    }
}

// member offset of segment i (k_cg_groups' rule: offsets that are none give 0)
__device__ __forceinline__ uint64_t bb_moff(const uint64_t* seg_off, uint64_t i, uint64_t km1) {
    const uint64_t o = seg_off[i], sub = i * km1;
    return o >= sub ? o - sub : 0ull;
}

// seg_of[row] = 2 i + o, pos[row] = the index in segment i, for member j = vertex 2 row + o of segment i; rows below min(n_rows, cap) only.  A member
// that is no vertex and a member whose segment the offsets do not give are skipped
__global__ __launch_bounds__(BFT_LAUNCH_THREADS) void k_bb_segof(uint64_t n_members, uint64_t n_segments, int k, uint64_t n_rows, const uint32_t* __restrict__ members,
                                                                 const uint64_t* __restrict__ seg_off, uint32_t* __restrict__ seg_of, uint32_t* __restrict__ pos,
                                                                 uint64_t cap) {
    const uint64_t km1 = (uint64_t)(k - 1);
    for (uint64_t j = blockIdx.x * (uint64_t)BFT_LAUNCH_THREADS + threadIdx.x; j < n_members; j += (uint64_t)gridDim.x * BFT_LAUNCH_THREADS) {
        uint64_t lo = 0, hi = n_segments;  // the last segment that starts at or before j lies in [lo, hi)
        while (hi - lo > 1) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (bb_moff(seg_off, mid, km1) <= j) lo = mid;
            else hi = mid;
        }
        const uint64_t o0 = seg_off[lo], o1 = seg_off[lo + 1], s0 = lo * km1, s1 = s0 + km1;
        if (o0 < s0 || o1 < s1 || o0 - s0 > j || j >= o1 - s1) continue;
        const uint32_t v = members[j];
        const uint64_t row = v >> 1;
        if (row >= n_rows || row >= cap) continue;
        if (seg_of) seg_of[row] = (uint32_t)(2 * lo) + (v & 1u);
        if (pos) pos[row] = (uint32_t)(j - (o0 - s0));
    }
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// bubbles: the chain of launches, the two forms of the entry point
// ------------------------------------------------------------------------------------------------
static const char* const BB_CAPTURE_MSG = "bubbles recorded into a graph: not supported (scratch may grow)";

// The handle's scratch (h->bb: HandleScratch, bft_handle.h) for n2 oriented segments on stream s: its own block, shared with no other family
static int bb_scratch(bft_gpu* h, HandleScratch::Lease& lease, uint64_t n2, hipStream_t s, BftBbScratch* p) {
    CK(lease.acquire(s, false));  // (the entry points refuse a capturing stream)
    Carver c{nullptr};
    c.take(p->flag, n2);
    c.take(p->slot, n2 * 4);
    CK(h->bb.grow(h->bb_buf, c.off, 0));
    CK(h->bb.grow(h->bb_tmp, bft_scan::scratch_bytes(n2), 0));
    c = Carver{h->bb_buf.as<uint8_t>()};
    c.take(p->flag, n2);
    c.take(p->slot, n2 * 4);
    return 0;
}
static int bb_check_sizes(uint64_t n_segments) {
    return n_segments < (1ull << 31) ? 0 : bft_fail(BFT_GPU_E_LIMIT, "bubbles: at most 2^31 - 1 segments");  // (oriented segments and 0xFFFFFFFF stay apart)
}
// Everything that counts: d_counts (32 bytes) complete, flags and slots in the scratch
static int bb_count(bft_gpu* h, const BbGraph& g, hipStream_t s, unsigned long long* d_counts, const BftBbScratch& p) {
    const double vd = (double)g.n2;
    CK(bft_zero_async(d_counts, 32, s));
    CK(bft_timed_launch(h, s, [&] { return bft_launch256(k_bb_find, g.n2, s, g, p.flag, d_counts); }));
    bft_stage("bubbles: sources", 0, s);  // (most lanes leave after two offsets, the others chase links: no streaming stage)
    CK(bft_timed_launch(h, s, [&] { return bft_scan::exclusive_sum<uint32_t>(BftBbFlag{p.flag}, p.slot, g.n2, s, h->bb_tmp, d_counts, false); }));
    bft_stage("bubbles: scan of the flags", vd * (1 + 4), s);
    return 0;
}
static int bb_emit(bft_gpu* h, const BbGraph& g, const BftBbScratch& p, uint32_t* d_bubbles, uint64_t cap, hipStream_t s) {
    if (d_bubbles && cap) CK(bft_timed_launch(h, s, [&] { return bft_launch256(k_bb_emit, g.n2, s, g, (const uint8_t*)p.flag, (const uint32_t*)p.slot, d_bubbles, cap); }));
    bft_stage("bubbles: records", d_bubbles && cap ? (double)g.n2 : 0, s);  // (the flags; slots, links and records of the few lanes that are set)
    return 0;
}

extern "C" int bft_gpu_unitig_bubbles_dev(bft_gpu* h, const void* d_seg_off, const void* d_seqs, const void* d_link_off, const void* d_links, uint64_t n_segments,
                                          uint64_t n_links, uint64_t max_branch_chars, void* d_bubbles, uint64_t cap, void* d_counts, void* hip_stream) {
    if (!h || !d_counts || (n_segments && (!d_seg_off || !d_seqs || !d_link_off)) || (n_segments && n_links && !d_links)) return bft_fail(BFT_GPU_E_ARG, "NULL argument");
    CK(bb_check_sizes(n_segments));
    ENTER(h);
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : h->stream;
    if (bft_stream_capturing(s)) return bft_fail(BFT_GPU_E_ARG, BB_CAPTURE_MSG);
    if (n_segments == 0) {
        CK(bft_zero_async(d_counts, 32, s));
        return bft_note_foreign_stream(h, s);
    }
    {
        const BbGraph g{(const uint64_t*)d_seg_off, (const char*)d_seqs, (const uint64_t*)d_link_off, (const uint32_t*)d_links, 2 * n_segments, n_links, max_branch_chars, h->k};
        HandleScratch::Lease lease(h->bb);
        BftBbScratch p;
        CK(bb_scratch(h, lease, g.n2, s, &p));
        StageScope stage_scope(h, s);
        CK(bb_count(h, g, s, (unsigned long long*)d_counts, p));
        CK(bb_emit(h, g, p, (uint32_t*)d_bubbles, cap, s));
    }
    return bft_note_foreign_stream(h, s);
}

// The host-buffer form: the arrays are checked and uploaded, the bubbles counted on the device, and the records filled only when cap holds them all.
extern "C" int bft_gpu_unitig_bubbles(bft_gpu* h, const uint64_t* seg_off, const char* seqs, const uint64_t* link_off, const uint32_t* links, uint64_t n_segments,
                                      uint64_t n_links, uint64_t max_branch_chars, uint32_t* bubbles, uint64_t cap, uint64_t counts[4]) {
    if (!h || !counts || (n_segments && (!seg_off || !seqs || !link_off)) || (n_segments && n_links && !links)) return bft_fail(BFT_GPU_E_ARG, "NULL argument");
    CK(bb_check_sizes(n_segments));
    ENTER(h);
    const uint64_t n2 = 2 * n_segments;
    if (n_segments) {
        for (uint64_t a = 0; a < n2; a++)
            if (link_off[a + 1] < link_off[a]) return bft_fail(BFT_GPU_E_ARG, "bubbles: link offsets must not decrease");
        if (link_off[n2] != n_links) return bft_fail(BFT_GPU_E_ARG, "bubbles: the last link offset must be n_links");
        for (uint64_t j = link_off[0]; j < n_links; j++)
            if (links[j] >= n2) return bft_fail(BFT_GPU_E_ARG, "bubbles: a link target is no oriented segment");
        for (uint64_t i = 0; i < n_segments; i++)
            if (seg_off[i + 1] < seg_off[i] + (uint64_t)h->k) return bft_fail(BFT_GPU_E_ARG, "bubbles: segment offsets must grow by k characters or more");
    }
    for (int i = 0; i < 4; i++) counts[i] = 0;
    if (n_segments == 0) return BFT_GPU_OK;
    const hipStream_t s = h->stream;
    const uint64_t nc = seg_off[n_segments];
    DevBuf dso, dseq, dlo, dln, dcnt, drec;
    CK(dso.alloc((n_segments + 1) * 8));
    CK(dseq.alloc(nc));
    CK(dlo.alloc((n2 + 1) * 8));
    CK(dln.alloc(n_links * 4));
    CK(dcnt.alloc(32));
    HIPCK(hipMemcpyAsync(dso.p, seg_off, (n_segments + 1) * 8, hipMemcpyHostToDevice, s));
    HIPCK(hipMemcpyAsync(dseq.p, seqs, nc, hipMemcpyHostToDevice, s));
    HIPCK(hipMemcpyAsync(dlo.p, link_off, (n2 + 1) * 8, hipMemcpyHostToDevice, s));
    if (n_links) HIPCK(hipMemcpyAsync(dln.p, links, n_links * 4, hipMemcpyHostToDevice, s));
    const BbGraph g{dso.as<uint64_t>(), dseq.as<char>(), dlo.as<uint64_t>(), dln.as<uint32_t>(), n2, n_links, max_branch_chars, h->k};
    HandleScratch::Lease lease(h->bb);
    BftBbScratch p;
    CK(bb_scratch(h, lease, n2, s, &p));
    StageScope stage_scope(h);
    CK(bb_count(h, g, s, dcnt.as<unsigned long long>(), p));
    unsigned long long cnt[4] = {0, 0, 0, 0};
    HIPCK(hipMemcpyAsync(cnt, dcnt.p, sizeof cnt, hipMemcpyDeviceToHost, s));
    HIPCK(hipStreamSynchronize(s));
    for (int i = 0; i < 4; i++) counts[i] = cnt[i];
    if (bubbles && cnt[0] > cap) return bft_fail(BFT_GPU_E_NOSPACE, "bubble buffer too small");
    if (!bubbles || cnt[0] == 0) return BFT_GPU_OK;
    CK(drec.alloc(cnt[0] * 24));
    CK(bb_emit(h, g, p, drec.as<uint32_t>(), cnt[0], s));
    HIPCK(hipMemcpyAsync(bubbles, drec.p, cnt[0] * 24, hipMemcpyDeviceToHost, s));
    HIPCK(hipStreamSynchronize(s));
    return BFT_GPU_OK;
}

// ------------------------------------------------------------------------------------------------
// the k-mer -> segment table
// ------------------------------------------------------------------------------------------------
extern "C" int bft_gpu_unitig_segment_of_dev(bft_gpu* h, const void* d_members, uint64_t n_members, const void* d_seg_off, uint64_t n_segments, void* d_seg_of, void* d_pos,
                                             uint64_t cap, void* hip_stream) {
    if (!h || (n_segments && !d_seg_off) || (n_members && n_segments && !d_members)) return bft_fail(BFT_GPU_E_ARG, "NULL argument");
    ENTER(h);
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : h->stream;
    if (bft_stream_capturing(s)) return bft_fail(BFT_GPU_E_ARG, "segment table recorded into a graph: not supported (pending insertions may have to be built)");
    CK(bft_ensure_built(h, false));  // (the number of rows; the table itself is not read)
    uint32_t* const so = (uint32_t*)d_seg_of;
    uint32_t* const po = (uint32_t*)d_pos;
    const uint64_t rows = std::min<uint64_t>(cap, h->n_kmers);
    if ((!so && !po) || rows == 0) return BFT_GPU_OK;
    StageScope stage_scope(h, s);
    CK(bft_timed_launch(h, s, [&] { return bft_launch256(k_bb_fill, rows, s, rows, so, po); }));
    bft_stage("bubbles: segment table, fill", (double)rows * 4 * ((so ? 1 : 0) + (po ? 1 : 0)), s);
    if (n_segments && n_members) {
        CK(bft_timed_launch(h, s, [&] {
            return bft_launch256(k_bb_segof, n_members, s, n_members, n_segments, h->k, (uint64_t)h->n_kmers, (const uint32_t*)d_members, (const uint64_t*)d_seg_off, so, po, cap);
        }));
    }
    bft_stage("bubbles: segment table, members", (double)n_members * (4 + 4 * ((so ? 1 : 0) + (po ? 1 : 0))), s);
    return bft_note_foreign_stream(h, s);
}

extern "C" int bft_gpu_unitig_segment_of(bft_gpu* h, const uint32_t* members, uint64_t n_members, const uint64_t* seg_off, uint64_t n_segments, uint32_t* seg_of,
                                         uint32_t* pos, uint64_t cap) {
    if (!h || (n_segments && !seg_off) || (n_members && n_segments && !members)) return bft_fail(BFT_GPU_E_ARG, "NULL argument");
    ENTER(h);
    CK(bft_ensure_built(h, false));
    const uint64_t km1 = (uint64_t)(h->k - 1), n = h->n_kmers;
    for (uint64_t g = 0; g < n_segments; g++)
        if (seg_off[g + 1] < seg_off[g] + km1 || seg_off[g] < g * km1) return bft_fail(BFT_GPU_E_ARG, "segment table: segment offsets must grow by k - 1 characters or more");
    if (n_segments && seg_off[n_segments] - n_segments * km1 > n_members) return bft_fail(BFT_GPU_E_ARG, "segment table: the last segment ends behind the members");
    if (n_segments)
        for (uint64_t i = 0; i < n_members; i++)
            if (members[i] >= 2 * n) return bft_fail(BFT_GPU_E_ARG, "segment table: a member is no vertex of the index");
    if (!seg_of && !pos) return BFT_GPU_OK;
    if (cap < n) return bft_fail(BFT_GPU_E_NOSPACE, "segment table buffers too small");
    if (n == 0) return BFT_GPU_OK;
    const hipStream_t s = h->stream;
    DevBuf dmem, doff, dso, dpo;
    if (n_segments && n_members) CK(dmem.alloc(n_members * 4));
    if (n_segments) CK(doff.alloc((n_segments + 1) * 8));
    if (seg_of) CK(dso.alloc(n * 4));
    if (pos) CK(dpo.alloc(n * 4));
    if (dmem.p) HIPCK(hipMemcpyAsync(dmem.p, members, n_members * 4, hipMemcpyHostToDevice, s));
    if (doff.p) HIPCK(hipMemcpyAsync(doff.p, seg_off, (n_segments + 1) * 8, hipMemcpyHostToDevice, s));
    CK(bft_gpu_unitig_segment_of_dev(h, dmem.p, dmem.p ? n_members : 0, doff.p, n_segments, dso.p, dpo.p, n, s));
    if (seg_of) HIPCK(hipMemcpyAsync(seg_of, dso.p, n * 4, hipMemcpyDeviceToHost, s));
    if (pos) HIPCK(hipMemcpyAsync(pos, dpo.p, n * 4, hipMemcpyDeviceToHost, s));
    HIPCK(hipStreamSynchronize(s));
    return BFT_GPU_OK;
}
