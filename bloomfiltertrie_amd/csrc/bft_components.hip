// bft_components.hip -- connected components of the index (get_nb_connected_component with BFS / DFS / BFS_subgraph / DFS_subgraph, reference
// snippets.h, src/snippets.c:605-960) over the sorted T-form table tk (one row per stored k-mer, rows in the bft_gpu_extract order):
//   (bft_sp_buckets  first row of every bucket of the top bits of the T-form, as for the simple paths)
//   k_cc_sets     one lane per colour set: does its sorted id list hold every requested id (a merge of the two sorted lists)
//   k_cc_init     parent[u] = u for a member, BFT_CC_NONE for any other row (bft_marking.hip adds a condition on the row's vertex flag)
//   k_cc_hook     one lane per member row u: its stored successors come from ONE lower bound (bft_for_each_successor, bft_succ.h), and u is joined
//                 with every member successor v != u.  Predecessor edges are the same edges seen from the other end.  The union-find is lock-free:
//                 the larger root is linked under the smaller (atomicCAS(&parent[hi], hi, lo), retried from the returned value), so a tree's root
//                 is its smallest row; finds halve the path with CAS.  Every read of parent[] is an agent-scope atomic load: the eight XCD L2s are
//                 not coherent within a kernel, a plain load may return a stale line, and the CAS alone decides
//   k_cc_flatten  after the kernel boundary: parent[u] = root of u
//   (two scans: members counted, BftCcMember; roots numbered in row order, BftCcRoot)
//   k_cc_label    num[u] = num[root of u], the label; parent[] becomes the size counters
//   k_cc_count    parent[label] += 1 per member: a lane sums its members of one label over 64 rows (non-members skipped), a wavefront whose
//                 lanes all hold one label adds once
//   k_cc_sizes    sizes[c] out; the largest component (an atomic from a wavefront only when it beats the counter's current value)
// No kernel needs LDS or scratch memory.
#include "bft_components.h"
#include "bft_dev.h"
#include "bft_handle.h"
#include "bft_scan.h"
#include "bft_succ.h"

namespace {

constexpr int CC_COUNT_ROUNDS = 64;  // rows per lane in k_cc_count (64-row rounds of a wavefront's stretch)

struct CcIds {
    uint32_t n;
    uint32_t id[BFT_CC_IDS];
};

__global__ __launch_bounds__(BFT_LAUNCH_THREADS) void k_cc_sets(uint32_t n_sets, const uint32_t* __restrict__ cs_off, const void* __restrict__ cs_ids, uint32_t cs_w,
                                                        CcIds q, int first, uint8_t* __restrict__ member) {
    for (uint64_t c = blockIdx.x * (uint64_t)BFT_LAUNCH_THREADS + threadIdx.x; c < n_sets; c += (uint64_t)gridDim.x * BFT_LAUNCH_THREADS) {
        uint32_t i = cs_off[c];
        const uint32_t e = cs_off[c + 1];
        bool ok = first || member[c] != 0;
        for (uint32_t j = 0; j < q.n && ok; j++) {
            const uint32_t id = q.id[j];
            while (i < e && bft_cs_id_at(cs_ids, cs_w, i) < id) i++;
            ok = i < e && bft_cs_id_at(cs_ids, cs_w, i) == id;
            i++;
        }
        member[c] = ok ? 1 : 0;
    }
}

// (marks: the two-bit vertex flags of bft_marking.h, 16 rows per word -- a member must also hold the flag `through`; NULL: no such condition)
__global__ __launch_bounds__(BFT_LAUNCH_THREADS) void k_cc_init(uint32_t n, const uint32_t* __restrict__ tcol, const uint8_t* __restrict__ member,
                                                        const uint32_t* __restrict__ marks, uint32_t through, uint32_t* __restrict__ parent) {
    for (uint64_t u = blockIdx.x * (uint64_t)BFT_LAUNCH_THREADS + threadIdx.x; u < n; u += (uint64_t)gridDim.x * BFT_LAUNCH_THREADS) {
        bool in = tcol == nullptr || member[tcol[u]];
        if (in && marks != nullptr) in = ((marks[u >> 4] >> (2u * ((uint32_t)u & 15u))) & 3u) == through;
        parent[u] = in ? (uint32_t)u : BFT_CC_NONE;
    }
}

__device__ __forceinline__ uint32_t cc_load(uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// A node of x's tree, found by halving: x moves to its grandparent, and a CAS points x there first.  Values only ever decrease (a parent is
// smaller than its child), so whatever a load returns -- stale or not -- is a node of x's tree, and the walk ends.  The result is a root unless a
// stale load made a former root look like one; the caller's CAS finds that out.
__device__ __forceinline__ uint32_t cc_find(uint32_t* parent, uint32_t x) {
    uint32_t p = cc_load(&parent[x]);
    while (p != x) {
        const uint32_t g = cc_load(&parent[p]);
        if (g == p) return p;
        atomicCAS(&parent[x], p, g);  // (a failed CAS: someone already moved x lower)
        x = g;
        p = cc_load(&parent[x]);
    }
    return x;
}

// Joins the trees of a and b: the larger root under the smaller, retried from the value the CAS returns.  Each retry starts below the last hi
// (old < hi, lo < hi), so the loop ends.  The root of a tree stays its smallest row, so lo is never in hi's own tree and no cycle can form.
__device__ __forceinline__ void cc_unite(uint32_t* parent, uint32_t a, uint32_t b) {
    for (;;) {
        a = cc_find(parent, a);
        b = cc_find(parent, b);
        if (a == b) return;
        const uint32_t hi = max(a, b), lo = min(a, b);
        const uint32_t old = atomicCAS(&parent[hi], hi, lo);
        if (old == hi) return;
        a = old;
        b = lo;
    }
}

template <int W>
__global__ __launch_bounds__(BFT_LAUNCH_THREADS) void k_cc_hook(const uint64_t* __restrict__ tk, uint32_t n, int k, int sb, const uint32_t* __restrict__ start,
                                                        uint32_t* parent) {
    for (uint64_t u = blockIdx.x * (uint64_t)BFT_LAUNCH_THREADS + threadIdx.x; u < n; u += (uint64_t)gridDim.x * BFT_LAUNCH_THREADS) {
        if (cc_load(&parent[u]) == BFT_CC_NONE) continue;  // (membership never changes: a member's parent is never BFT_CC_NONE)
        bft_for_each_successor<W>(tk, n, k, sb, start, u, [&](uint32_t r) {
            if (r != (uint32_t)u && cc_load(&parent[r]) != BFT_CC_NONE) cc_unite(parent, (uint32_t)u, r);
        });
    }
}

// (plain loads: the hook's writes are visible after the kernel boundary; a lane here reads either a row's parent from the hook or the root another
// lane wrote, and both lead to the same root)
__global__ __launch_bounds__(BFT_LAUNCH_THREADS) void k_cc_flatten(uint32_t n, uint32_t* parent) {
    for (uint64_t u = blockIdx.x * (uint64_t)BFT_LAUNCH_THREADS + threadIdx.x; u < n; u += (uint64_t)gridDim.x * BFT_LAUNCH_THREADS) {
        const uint32_t p = parent[u];
        if (p == BFT_CC_NONE || p == (uint32_t)u) continue;
        uint32_t r = p, q = parent[r];
        while (q != r) {
            r = q;
            q = parent[r];
        }
        if (r != p) parent[u] = r;
    }
}

__global__ __launch_bounds__(BFT_LAUNCH_THREADS) void k_cc_label(uint32_t n, uint32_t* __restrict__ parent, uint32_t* __restrict__ num, uint32_t* __restrict__ labels) {
    for (uint64_t u = blockIdx.x * (uint64_t)BFT_LAUNCH_THREADS + threadIdx.x; u < n; u += (uint64_t)gridDim.x * BFT_LAUNCH_THREADS) {
        const uint32_t p = parent[u];
        const uint32_t lab = p == BFT_CC_NONE ? BFT_CC_NONE : num[p];
        if (labels) labels[u] = lab;
        if (p != (uint32_t)u) num[u] = lab;  // (a root keeps its number: the other rows of its component read it)
        parent[u] = 0;                        // (only this lane reads parent[u])
    }
}

__global__ __launch_bounds__(BFT_LAUNCH_THREADS) void k_cc_count(uint32_t n, const uint32_t* __restrict__ lab, uint32_t* __restrict__ sz) {
    constexpr uint64_t STRETCH = 64ull * CC_COUNT_ROUNDS;  // rows per wavefront and pass
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t waves = (uint64_t)gridDim.x * (BFT_LAUNCH_THREADS / 64);
    for (uint64_t base = (blockIdx.x * (uint64_t)(BFT_LAUNCH_THREADS / 64) + (threadIdx.x >> 6)) * STRETCH; base < n; base += waves * STRETCH) {
        uint32_t cur = BFT_CC_NONE, cnt = 0;
        for (int r = 0; r < CC_COUNT_ROUNDS; r++) {
            const uint64_t i = base + (uint64_t)r * 64u + lane;
            const uint32_t c = i < n ? lab[i] : BFT_CC_NONE;
            if (c == BFT_CC_NONE) continue;  // (a non-member does not end the run: a sparse sub-graph of one genome is one run per lane)
            if (c != cur) {
                if (cnt) atomicAdd(&sz[cur], cnt);
                cur = c;
                cnt = 0;
            }
            cnt++;
        }
        // one component for the whole stretch (a long genome): one add for the wavefront instead of 64
        const uint64_t act = __ballot(cnt != 0);
        if (act == 0) continue;
        const int lead = __ffsll((unsigned long long)act) - 1;
        const uint32_t c0 = (uint32_t)__shfl((int)cur, lead);
        if (__ballot(cnt != 0 && cur != c0) == 0) {
            uint32_t tot = cnt;
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) tot += (uint32_t)__shfl_xor((int)tot, d);
            if ((int)lane == lead) atomicAdd(&sz[c0], tot);
        } else if (cnt)
            atomicAdd(&sz[cur], cnt);
    }
}

__global__ __launch_bounds__(BFT_LAUNCH_THREADS) void k_cc_sizes(const uint32_t* __restrict__ sz, uint64_t* __restrict__ sizes, uint64_t cap,
                                                         unsigned long long* __restrict__ counts) {
    const uint64_t nc = counts[0];
    // (every lane of a wavefront runs the same iterations: the wavefront's maximum is combined with shuffles)
    for (uint64_t c0 = blockIdx.x * (uint64_t)BFT_LAUNCH_THREADS + (threadIdx.x & ~63u); c0 < nc; c0 += (uint64_t)gridDim.x * BFT_LAUNCH_THREADS) {
        const uint64_t c = c0 + (threadIdx.x & 63u);
        uint32_t v = 0;
        if (c < nc) {
            v = sz[c];
            if (sizes && c < cap) sizes[c] = v;
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, d));
        // (only a wavefront that beats what the counter already holds takes the atomic, as k_sp_ends)
        if ((threadIdx.x & 63u) == 0 && v && v > __hip_atomic_load(&counts[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&counts[2], (unsigned long long)v);
    }
}

}  // namespace

int bft_cc_sets(uint64_t n_sets, const uint32_t* d_cs_off, const void* d_cs_ids, uint32_t cs_w, const uint32_t* ids, uint32_t nb, bool first, const BftCcScratch& p,
                hipStream_t s) {
    CcIds q{};
    q.n = nb < BFT_CC_IDS ? nb : BFT_CC_IDS;
    for (uint32_t j = 0; j < q.n; j++) q.id[j] = ids[j];
    return bft_launch256(k_cc_sets, n_sets, s, (uint32_t)n_sets, d_cs_off, d_cs_ids, cs_w, q, first ? 1 : 0, p.member);
}

int bft_cc_init(uint64_t n, const uint32_t* d_tcol, const BftCcScratch& p, hipStream_t s, const uint32_t* d_marks, uint32_t through) {
    return bft_launch256(k_cc_init, n, s, (uint32_t)n, d_tcol, (const uint8_t*)p.member, d_marks, through, p.parent);
}

int bft_cc_hook(int W, const uint64_t* d_tk, uint64_t n, int k, const BftCcScratch& p, hipStream_t s) {
    return bft_for_w(W, [&](auto KW) { return bft_launch256(k_cc_hook<KW>, n, s, d_tk, (uint32_t)n, k, p.sp.sb, (const uint32_t*)p.sp.start, p.parent); });
}

int bft_cc_flatten(uint64_t n, const BftCcScratch& p, hipStream_t s) {
    return bft_launch256(k_cc_flatten, n, s, (uint32_t)n, p.parent);
}

int bft_cc_label(uint64_t n, const BftCcScratch& p, uint32_t* d_labels, hipStream_t s) {
    return bft_launch256(k_cc_label, n, s, (uint32_t)n, p.parent, p.num, d_labels);
}

int bft_cc_count(uint64_t n, const BftCcScratch& p, hipStream_t s) {
    if (n == 0) return 0;
    // (the items are lanes: each takes CC_COUNT_ROUNDS rows)
    return bft_launch256(k_cc_count, (n + CC_COUNT_ROUNDS - 1) / CC_COUNT_ROUNDS, s, (uint32_t)n, (const uint32_t*)p.num, p.parent);
}

int bft_cc_sizes(uint64_t n, const BftCcScratch& p, uint64_t* d_sizes, uint64_t sizes_cap, unsigned long long* d_counts, hipStream_t s) {
    return bft_launch256(k_cc_sizes, n, s, (const uint32_t*)p.parent, d_sizes, sizes_cap, d_counts);
}

// ------------------------------------------------------------------------------------------------
// the C-ABI entry points: the handle's scratch, the chain of launches, the host-buffer form
// ------------------------------------------------------------------------------------------------
// the arrays of a block with room for m rows and `sets` colour sets (p->sp.sb set), from `base` on; returns the block's size
static size_t cc_carve(uint64_t m, uint64_t sets, uint8_t* base, BftCcScratch* p) {
    Carver c{base};
    c.take(p->sp.start, ((1ull << p->sp.sb) + 1) * 4);
    c.take(p->parent, m * 4);
    c.take(p->num, m * 4);
    c.take(p->member, sets);
    return c.off;
}
// The handle's scratch (h->cc: HandleScratch, bft_handle.h) for an index of n rows and n_sets colour sets on stream s: its own block, shared with no
// other query, sized exactly.
static int cc_scratch(bft_gpu* h, HandleScratch::Lease& lease, uint64_t n, uint64_t n_sets, hipStream_t s, BftCcScratch* p) {
    CK(lease.acquire(s, false));  // (the entry points refuse a capturing stream)
    p->sp = BftSpScratch{};
    p->sp.sb = bft_sp_bucket_bits(h->k);
    h->cc_m = std::max(n, h->cc_m);
    h->cc_sets = std::max(n_sets, h->cc_sets);
    CK(h->cc.grow(h->cc_buf, cc_carve(h->cc_m, h->cc_sets, nullptr, p), 0));
    CK(h->cc.grow(h->cc_tmp, bft_scan::scratch_bytes(n + 1), 0));
    cc_carve(h->cc_m, h->cc_sets, h->cc_buf.as<uint8_t>(), p);
    return 0;
}
// Membership, forest, numbering, labels and sizes on stream s: d_counts = {n_components, n_members, largest} (24 bytes, device); the labels stay in
// p.num, the sizes in p.parent.  d_labels / d_sizes (may be NULL): the labels, the sizes below sizes_cap.  The number of launches depends on nb alone.
// With "build_stages" on, every step is a stage (bft_gpu_build_stages), its bytes those its algorithm reads and writes.
static int cc_run(bft_gpu* h, const uint32_t* ids, uint32_t nb, hipStream_t s, unsigned long long* d_counts, const BftCcScratch& p, uint32_t* d_labels,
                  uint64_t* d_sizes, uint64_t sizes_cap) {
    const uint64_t n = h->n_kmers, ns = h->n_sets;
    const int W = h->W, k = h->k;
    const uint64_t* tk = h->d_tk.as<uint64_t>();
    const double nd = (double)n, rowb = 8.0 * W;
    CK(bft_zero_async(d_counts, 24, s));
    for (uint32_t j = 0; j < nb; j += BFT_CC_IDS)
        CK(bft_timed_launch(h, s, [&] { return bft_cc_sets(ns, h->d_cs_off.as<uint32_t>(), h->d_cs_ids.p, h->cs_w, ids + j, nb - j, j == 0, p, s); }));
    if (nb) bft_stage("components: members among the colour sets", (double)ns * 9 + (double)h->n_ids * h->cs_w, s);
    CK(bft_timed_launch(h, s, [&] { return bft_cc_init(n, nb ? h->d_tcol.as<uint32_t>() : nullptr, p, s); }));
    bft_stage("components: members", nd * (4 + (nb ? 5 : 0)), s);
    CK(bft_timed_launch(h, s, [&] { return bft_sp_buckets(W, tk, n, k, p.sp, s); }));
    bft_stage("components: buckets of the table", (double)((1ull << p.sp.sb) + 1) * 4, s);
    CK(bft_timed_launch(h, s, [&] { return bft_cc_hook(W, tk, n, k, p, s); }));
    bft_stage("components: successors and hooking", nd * (2 * rowb + 4 + 4 + 8), s);
    CK(bft_timed_launch(h, s, [&] { return bft_cc_flatten(n, p, s); }));
    bft_stage("components: roots", nd * 12, s);
    CK(bft_timed_launch(h, s, [&] { return bft_scan::exclusive_sum<uint32_t>(BftCcMember{p.parent}, p.num, n, s, h->cc_tmp, d_counts + 1, false); }));
    CK(bft_timed_launch(h, s, [&] { return bft_scan::exclusive_sum<uint32_t>(BftCcRoot{p.parent}, p.num, n, s, h->cc_tmp, d_counts, false); }));
    bft_stage("components: two scans (members, components)", nd * 16, s);
    CK(bft_timed_launch(h, s, [&] { return bft_cc_label(n, p, d_labels, s); }));
    bft_stage("components: labels", nd * (4 + 4 + 4 + 4 + (d_labels ? 4 : 0)), s);
    CK(bft_timed_launch(h, s, [&] { return bft_cc_count(n, p, s); }));
    bft_stage("components: sizes", nd * 4, s);
    CK(bft_timed_launch(h, s, [&] { return bft_cc_sizes(n, p, d_sizes, sizes_cap, d_counts, s); }));
    bft_stage("components: sizes out, largest", 0.0, s);  // (n_components entries: not known on the host without a read-back)
    return 0;
}
static int cc_prepare(bft_gpu* h) {
    CK(bft_ensure_built(h));  // ("compact_table": the sorted table comes back, as for rows, prefixes and simple paths)
    if (h->n_kmers >= (1ull << 31)) return bft_fail(BFT_GPU_E_LIMIT, "components: at most 2^31 - 1 k-mers");
    return 0;
}

extern "C" int bft_gpu_components_dev(bft_gpu* h, const uint32_t* genome_ids, uint32_t nb_ids, void* d_labels, void* d_sizes, uint64_t sizes_cap, void* d_counts,
                                      void* hip_stream) {
    if (!h || !d_counts || (nb_ids && !genome_ids)) return bft_fail(BFT_GPU_E_ARG, "NULL argument");
    for (uint32_t j = 1; j < nb_ids; j++)
        if (genome_ids[j] <= genome_ids[j - 1]) return bft_fail(BFT_GPU_E_ARG, "components: genome ids must be strictly increasing");
    ENTER(h);
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : h->stream;
    if (bft_stream_capturing(s)) return bft_fail(BFT_GPU_E_ARG, "components recorded into a graph: not supported (the table may have to come back, scratch may grow)");
    CK(cc_prepare(h));
    if (h->n_kmers == 0) {
        CK(bft_zero_async(d_counts, 24, s));
        return bft_note_foreign_stream(h, s);
    }
    {
        HandleScratch::Lease lease(h->cc);
        BftCcScratch p;
        CK(cc_scratch(h, lease, h->n_kmers, h->n_sets, s, &p));
        StageScope stage_scope(h, s);
        CK(cc_run(h, genome_ids, nb_ids, s, (unsigned long long*)d_counts, p, (uint32_t*)d_labels, (uint64_t*)d_sizes, sizes_cap));
    }
    return bft_note_foreign_stream(h, s);
}

// The host-buffer form: the components are counted on the device, and the outputs filled only when the caps hold them all.
extern "C" int bft_gpu_components(bft_gpu* h, const uint32_t* genome_ids, uint32_t nb_ids, uint32_t* labels, uint64_t labels_cap, uint64_t* sizes,
                                  uint64_t sizes_cap, uint64_t* counts) {
    if (!h || !counts || (nb_ids && !genome_ids)) return bft_fail(BFT_GPU_E_ARG, "NULL argument");
    for (uint32_t j = 1; j < nb_ids; j++)
        if (genome_ids[j] <= genome_ids[j - 1]) return bft_fail(BFT_GPU_E_ARG, "components: genome ids must be strictly increasing");
    ENTER(h);
    CK(cc_prepare(h));
    counts[0] = counts[1] = counts[2] = 0;
    const uint64_t n = h->n_kmers;
    if (n == 0) return BFT_GPU_OK;
    const hipStream_t s = h->stream;
    DevBuf dcnt;
    CK(dcnt.alloc(24));
    HandleScratch::Lease lease(h->cc);
    BftCcScratch p;
    CK(cc_scratch(h, lease, n, h->n_sets, s, &p));
    StageScope stage_scope(h);
    CK(cc_run(h, genome_ids, nb_ids, s, dcnt.as<unsigned long long>(), p, nullptr, nullptr, 0));
    unsigned long long cnt[3] = {0, 0, 0};
    HIPCK(hipMemcpyAsync(cnt, dcnt.p, 24, hipMemcpyDeviceToHost, s));
    HIPCK(hipStreamSynchronize(s));
    for (int i = 0; i < 3; i++) counts[i] = cnt[i];
    if ((labels && labels_cap < n) || (sizes && sizes_cap < cnt[0])) return bft_fail(BFT_GPU_E_NOSPACE, "component buffers too small");
    DevBuf dsz;
    if (sizes && cnt[0]) {  // (the counters are 32-bit in the scratch: widened by a second pass of the last kernel)
        CK(dsz.alloc(cnt[0] * 8));
        CK(bft_timed_launch(h, s, [&] { return bft_cc_sizes(n, p, dsz.as<uint64_t>(), cnt[0], dcnt.as<unsigned long long>(), s); }));
        HIPCK(hipMemcpyAsync(sizes, dsz.p, cnt[0] * 8, hipMemcpyDeviceToHost, s));
    }
    if (labels) HIPCK(hipMemcpyAsync(labels, p.num, n * 4, hipMemcpyDeviceToHost, s));
    if (labels || sizes) HIPCK(hipStreamSynchronize(s));
    return BFT_GPU_OK;
}
