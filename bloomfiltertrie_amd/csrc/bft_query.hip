// bft_query.hip -- the k-mer and sequence queries of the C-ABI (include/bft_gpu.h): which kernel a batch takes (bft_launch_query), the launchers of
// the container walk, of the k-mer hash and of the branching query, the claim slots (ClaimSlots, bft_handle.h), residency / probe tuning
// (bft_tune_residency), the pinned block of small host batches, colour lists and colour rows, sequence queries, and the entry points
// bft_gpu_query_presence / _branching / _colors / _color_rows / _sequences (each with its _dev form) and bft_gpu_query_rows.  With its device code:
//   bft_kernels_query.h  k_query / k_query8 / k_query6 (batched isKmerPresent as a container walk, src/presenceNode.c:1823-1921: one lane per
//                        k-mer, coalesced dword loads of the batch, hash table + root Bloom block + root CC headers staged in LDS, 64 presence
//                        bits per wavefront via __ballot), k_branching / k_branching8 / k_branching6 (src/branchingNode.c)
//   bft_kernels_seq.h    query_sequence (src/bft.c:1241-1351) around the walk
//   bft_kernels_color.h  batched get_annotation + get_list_id_genomes (src/bft.c:363-387, 622-641)
//   bft_walk.h           the per-k-mer walk itself (shared with the host-side test helper)
// A launch is given what it uses as arguments -- the image (a copy where the launch differs from the handle's), the launch shape (WalkShape), the claim
// (ClaimSlots::Claim) -- and never reads it from a handle field that an earlier statement set for it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstring>
#include <initializer_list>
#include <type_traits>
#include <vector>

#include "bft_handle.h"
#include "bft_scan.h"
#include "bft_walk.h"

#define BFT_BLOCK 256
#define BFT_ABSENT_ROW 0xFFFFFFFFu

// device code, by topic
#include "bft_kernels_query.h"
#include "bft_kernels_seq.h"
#include "bft_kernels_color.h"

// ------------------------------------------------------------------------------------------------
// claim slots (ClaimSlots: bft_handle.h)
// ------------------------------------------------------------------------------------------------
void ClaimSlots::ensure() {
    if (ctr || failed) return;
    if (hipMalloc((void**)&ctr, KH_CTR_SLOTS * 8) != hipSuccess || hipMemset(ctr, 0, KH_CTR_SLOTS * 8) != hipSuccess ||
        hipDeviceSynchronize() != hipSuccess) {  // (blocking: no launch of any stream can meet a counter that is not zero yet)
        (void)hipGetLastError();
        if (ctr) (void)hipFree(ctr);
        ctr = nullptr;
        failed = true;
    }
}

ClaimSlots::Claim ClaimSlots::take(hipStream_t s, bool wanted, uint64_t units) {
    const Claim none{BftClaimCtr{nullptr, 0}, -1};
    if (!wanted || !ctr) return none;
    // a launch being recorded into a graph gets static rounds: `base` is a kernel argument, frozen at capture time, and from the second replay on the
    // counter stands above it -- every workgroup would answer its first round only (the counter cannot be reset on the device without giving up
    // the property that nothing an unfinished launch leaves behind can hurt the next one)
    if (bft_stream_capturing(s)) return none;
    int slot = -1;
    for (int i = 0; i < used; i++)
        if (stream[i] == s) slot = i;
    if (slot < 0 && used < KH_CTR_SLOTS) {
        slot = used++;
        stream[slot] = s;
    }
    if (slot < 0) {  // every slot taken: the least recently used one, if its stream has nothing of ours in flight any more
        int lru = 0;
        for (int i = 1; i < KH_CTR_SLOTS; i++)
            if (tick[i] < tick[lru]) lru = i;
        // (a slot last used before the handle started recording events -- its stream may be gone by now, so there is nothing to ask but the device:
        // once per such slot at most)
        const bool over = ev[lru] ? hipEventQuery(ev[lru]) == hipSuccess : hipDeviceSynchronize() == hipSuccess;
        if (over) {
            slot = lru;
            stream[slot] = s;
        } else {
            (void)hipGetLastError();
            static_launches++;
            return none;
        }
    }
    tick[slot] = ++clock;
    const Claim c{BftClaimCtr{ctr + slot, base[slot]}, slot};
    base[slot] += units + ((unsigned long long)1 << 24);  // (2^24: more than the resident workgroups x the largest claim)
    return c;
}

void ClaimSlots::launched(int slot, hipStream_t s) {
    if (slot < 0 || used < KH_CTR_SLOTS / 2) return;  // (no event traffic on a handle that is queried on a few streams)
    if (!ev[slot] && hipEventCreateWithFlags(&ev[slot], hipEventDisableTiming) != hipSuccess) { ev[slot] = nullptr; (void)hipGetLastError(); return; }
    if (hipEventRecord(ev[slot], s) != hipSuccess) (void)hipGetLastError();
}

int ClaimSlots::stale(int mode) {
    if (!ctr) return 0;
    HIPCK(hipDeviceSynchronize());
    unsigned long long v[KH_CTR_SLOTS];
    for (int i = 0; i < KH_CTR_SLOTS; i++) v[i] = mode == 3 ? 0ull : base[i] - (mode == 1 && base[i] ? 1ull : 0ull);
    HIPCK(hipMemcpy(ctr, v, sizeof(v), hipMemcpyHostToDevice));
    return 0;
}

// Whether a launch that deals out n k-mers (lines of work for the branching kernel) asks for a claim counter: "query_dynamic", BFT_GPU_QUERY_DYNAMIC=0
// and the smallest batch that is worth one ("query_dynamic_min").
static bool claims_wanted(const bft_gpu* h, uint64_t n) {
    static const bool env_off = getenv("BFT_GPU_QUERY_DYNAMIC") && atoi(getenv("BFT_GPU_QUERY_DYNAMIC")) == 0;
    return h->opt_query_dynamic && !env_off && n >= h->opt_query_dynamic_min;
}

// ------------------------------------------------------------------------------------------------
// the container walk: launch shape, kernel selection, launchers
// ------------------------------------------------------------------------------------------------
// Resident k_query workgroups per CU.  Measured on MI355X (tools/perf_probe.py): a one-level index whose suffix-group
// table exceeds the L2 runs at the beyond-L2 gather rate with 4 waves per SIMD and loses 10 % with 8; deep walks and
// L2-resident indexes gain 10-40 % from 8; which side an index falls on is measured, not guessed (bft_tune_residency).
int bft_query_residency(const bft_gpu* h) {
    if (h->opt_wgs_per_cu) return h->opt_wgs_per_cu;
    return h->tuned_wgs ? h->tuned_wgs : 2;
}

// How the walk kernels sit on a CU at residency res -- 1: one 1024-thread workgroup per CU, 2: two (8 wavefronts per SIMD), 3: two of 768 threads
// (6 per SIMD).  LDS: hash table + the root area (the root's Bloom block (<= 64 CCs) and CC headers, or -- with the derived root tables -- k_query's
// queue of deferred lanes): at most two workgroups fit a CU (160 KB).  With one workgroup per CU the request is padded past half the LDS so that the
// dispatcher cannot pair two on a CU.
// block: threads per workgroup; lds: dynamic LDS per workgroup; resident: workgroups the device holds at a time (256 CUs x resident workgroups per CU)
struct WalkShape { int res; uint32_t block; size_t lds; uint64_t resident; };
static WalkShape walk_shape(int res) {
    const int wgs = res == 1 ? 1 : 2;
    size_t lds = BFT_LDS_HM_BYTES + ((size_t)BFT_MODULO_HASH * 8 + 15) / 16 * 16 + BFT_LDS_ROOT_MAX_CC * sizeof(BftCCX);
    if (wgs == 1) lds = std::max<size_t>(lds, 84u << 10);
    return WalkShape{res, res == 3 ? (uint32_t)BFT_BLOCK6 : 1024u, lds, 256ull * (uint64_t)wgs};
}
// The walk kernels ask for more dynamic LDS than a kernel gets unasked.  The attribute is per kernel and per device: `done` -- a static of the
// instantiation that launches `kernels` -- holds one bit per device it was set on.
static int allow_walk_lds(std::atomic<uint64_t>& done, int device, std::initializer_list<const void*> kernels) {
    const uint64_t dev_bit = 1ull << (device & 63);
    if (done.load(std::memory_order_acquire) & dev_bit) return 0;
    for (const void* k : kernels) HIPCK(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, 84 << 10));
    done.fetch_or(dev_bit, std::memory_order_release);
    return 0;
}

// The walk kernels are templates over the key width W, the root staging (STAGED: the root's 1 .. BFT_LDS_ROOT_MAX_CC CCs are copied into LDS) and the
// probe mode (PROBE 1: 8-row probes of suffix groups, rows of BFT_PROBE_MAX_W words at most): f(W, STAGED, PROBE) is called with the three as
// std::integral_constant.  PROBES false (branching, sequences): PROBE is always 0, and f is never instantiated with 1.
template <bool PROBES, int W, bool STAGED, class F>
static int walk_dispatch_probe(bool probe8, F& f) {
    if constexpr (PROBES && W <= BFT_PROBE_MAX_W)
        if (probe8) return f(std::integral_constant<int, W>{}, std::bool_constant<STAGED>{}, std::integral_constant<int, 1>{});
    return f(std::integral_constant<int, W>{}, std::bool_constant<STAGED>{}, std::integral_constant<int, 0>{});
}
template <bool PROBES, class F>
static int walk_dispatch(const bft_gpu* h, bool probe8, F&& f) {
    const bool staged = h->root_ncc >= 1 && h->root_ncc <= BFT_LDS_ROOT_MAX_CC;
    switch (h->W) {
    case 1: return staged ? walk_dispatch_probe<PROBES, 1, true>(probe8, f) : walk_dispatch_probe<PROBES, 1, false>(probe8, f);
    case 2: return staged ? walk_dispatch_probe<PROBES, 2, true>(probe8, f) : walk_dispatch_probe<PROBES, 2, false>(probe8, f);
    case 3: return staged ? walk_dispatch_probe<PROBES, 3, true>(probe8, f) : walk_dispatch_probe<PROBES, 3, false>(probe8, f);
    default: return staged ? walk_dispatch_probe<PROBES, 4, true>(probe8, f) : walk_dispatch_probe<PROBES, 4, false>(probe8, f);
    }
}

// Presence bits (and rows, or colour sets with im.emit_cs) of n k-mers through the walk over image im at shape sh; no timing bookkeeping.  With
// im.walk_kh the walk looks plain root groups up in the k-mer hash (bft_walkh.hip; 4-row probes only).  h: the device, the root's CC count, the
// grid multiplier and the claim slots.  rec: bytes per input record (B, or 8W for the zero-padded word records of the sequence path).
static int launch_walk(bft_gpu* h, const BftImage& im, const WalkShape& sh, const uint8_t* d_kmers, uint64_t n, uint64_t* d_bits64, uint32_t* d_rows, hipStream_t s, int rec) {
    // chunks of 1024 k-mers per wavefront (query_body): the first by wavefront number, the others claimed from the stream's counter
    const uint64_t n_chunks = (n + 1023) / 1024, wg_chunks = (n_chunks + sh.block / 64 - 1) / (sh.block / 64);
    const ClaimSlots::Claim claim = h->claims.take(s, claims_wanted(h, n), n_chunks);
    const uint64_t grid_cap = h->opt_test_walk_grid ? h->opt_test_walk_grid : ~0ull;  // ("test_walk_grid": the claim above is still sized by n_chunks)
    const dim3 grid((unsigned)std::max<uint64_t>(1, std::min<uint64_t>(std::min<uint64_t>(wg_chunks, sh.resident * h->opt_grid_mult), grid_cap)));
    CK(walk_dispatch<true>(h, im.probe_big && !im.walk_kh, [&](auto w, auto staged, auto probe) {
        constexpr int W = decltype(w)::value, PROBE = decltype(probe)::value;
        constexpr bool STAGED = decltype(staged)::value;
        static std::atomic<uint64_t> lds_allowed{0};
        CK(allow_walk_lds(lds_allowed, h->device, {(const void*)k_query<W, 1024, STAGED, PROBE>, (const void*)k_query8<W, 1024, STAGED, PROBE>, (const void*)k_query6<W, STAGED, PROBE>}));
        if (im.walk_kh && PROBE == 0) return bft_walkh_query(im, d_kmers, n, rec, d_bits64, d_rows, claim.ctr, (uint32_t)h->opt_grid_mult, h->opt_test_walk_grid, s);
        if (sh.res == 1) hipLaunchKernelGGL((k_query<W, 1024, STAGED, PROBE>), grid, dim3(sh.block), sh.lds, s, im, d_kmers, n, rec, d_bits64, d_rows, claim.ctr);
        else if (sh.res == 3) hipLaunchKernelGGL((k_query6<W, STAGED, PROBE>), grid, dim3(sh.block), sh.lds, s, im, d_kmers, n, rec, d_bits64, d_rows, claim.ctr);
        else hipLaunchKernelGGL((k_query8<W, 1024, STAGED, PROBE>), grid, dim3(sh.block), sh.lds, s, im, d_kmers, n, rec, d_bits64, d_rows, claim.ctr);
        HIPCK(hipGetLastError());
        return 0;
    }));
    h->claims.launched(claim.slot, s);
    return 0;
}

// through_kh: plain root groups are looked up in the k-mer hash (k_query6h) -- the caller wants presence or colour sets, not rows
static int launch_query_walk(bft_gpu* h, const uint8_t* d_kmers, uint64_t n, uint64_t* d_bits64, uint32_t* d_rows, hipStream_t s, int rec, bool through_kh) {
    BftImage im = h->im;
    if (!through_kh) im.walk_kh = 0;
    hipEvent_t e0, e1;
    CK(bft_timing_begin(h, s, &e0, &e1));
    CK(launch_walk(h, im, walk_shape(bft_query_residency(h)), d_kmers, n, d_bits64, d_rows, s, rec));
    return bft_timing_end(h, s, e0, e1);
}

// Presence (and, with im.emit_cs, the colour set of every found k-mer into d_out32) through the k-mer hash.
static int launch_query_kh(bft_gpu* h, const uint8_t* d_kmers, uint64_t n, uint64_t* d_bits64, uint32_t* d_out32, hipStream_t s, int rec) {
    hipEvent_t e0, e1;
    CK(bft_timing_begin(h, s, &e0, &e1));
    const ClaimSlots::Claim claim = h->claims.take(s, claims_wanted(h, n), (n + 255) / 256);
    CK(bft_kh_query(h->im, h->opt_grid_mult, d_kmers, n, rec, d_bits64, d_out32, claim.ctr, h->opt_query_chunk, s));
    HIPCK(hipGetLastError());
    h->claims.launched(claim.slot, s);
    return bft_timing_end(h, s, e0, e1);
}

// Which kernel a batch takes: the k-mer hash answers presence and colour sets (one cache line per k-mer); rows -- positions in the
// sorted table, what the reference keeps in resultPresence -- come from the container walk, as does everything on an image
// without the k-mer hash ("kmer_hash" 0, a table that could not be allocated or whose overflow list ran full: kh_wanted, kh_finish).  Same answers either way (tests/test_gpu_parity.py).
int bft_launch_query(bft_gpu* h, const uint8_t* d_kmers, uint64_t n, uint64_t* d_bits64, uint32_t* d_rows, hipStream_t s, int rec_bytes) {
    if (n == 0) return 0;
    const int rec = rec_bytes ? rec_bytes : h->B;
    const bool no_rows = d_rows == nullptr || h->im.emit_cs;  // presence or colour sets: what the k-mer hash holds
    if (h->im.kh_lines != nullptr && no_rows && !h->opt_walk_hash) return launch_query_kh(h, d_kmers, n, d_bits64, d_rows, s, rec);
    CK(bft_ensure_table(h));
    // the walk looks plain root groups up in the k-mer hash when no row is asked for ("walk_hash")
    return launch_query_walk(h, d_kmers, n, d_bits64, d_rows, s, rec, no_rows && h->opt_walk_hash);
}

// ------------------------------------------------------------------------------------------------
// residency / probe tuning
// ------------------------------------------------------------------------------------------------
// Synthetic batch for tune_residency: k-mers of the index itself (pseudo-random rows of tk), every other one with a
// single-nucleotide change -- the mix of present k-mers and near misses that exercises the whole walk.
template <int W>
__global__ void k_tune_queries(const uint64_t* __restrict__ tk, uint64_t n_kmers, int k, int B, uint64_t m, uint8_t* __restrict__ out) {
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < m; i += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t z = (i + 0x9E3779B97F4A7C15ull) * 0xBF58476D1CE4E5B9ull;
        z ^= z >> 31; z *= 0x94D049BB133111EBull; z ^= z >> 29;
        const uint64_t row = z % n_kmers;
        uint64_t t[W], x[W];
#pragma unroll
        for (int w = 0; w < W; w++) t[w] = tk[row * W + w];
        bft_x_from_tform<W>(t, k, x);
        if (i & 1) {
            const int pos = (int)((z >> 33) % (uint64_t)k);
            const uint64_t flip = 1 + ((z >> 20) % 3);
#pragma unroll
            for (int w = 0; w < W; w++)
                if (w == (2 * pos) >> 6) x[w] ^= flip << ((2 * pos) & 63);
        }
        for (int b = 0; b < B; b++) {
            uint64_t v = 0;
#pragma unroll
            for (int w = 0; w < W; w++)
                if (w == (b >> 3)) v = x[w];
            out[i * B + b] = (uint8_t)(v >> (8 * (b & 7)));
        }
    }
}

namespace {
struct TuneEvents {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ~TuneEvents() {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    }
};
// what bft_tune_residency measured, before any of it is written to the handle
struct Tuned {
    float best[6] = {1e30f, 1e30f, 1e30f, 1e30f, 1e30f, 1e30f};  // (residency 1 / 2 / 3) x (probe block 4 / 8 rows)
    int wgs = 2, probe = 4;
    float rs[2] = {1e30f, 1e30f};  // the root-table comparison: direct table alone / with the range table
    int rstart = -1;               // its winner; -1: not run
};
}  // namespace

// The measurement: every candidate is an image copy and a shape of its own, launched without timing bookkeeping; h is not written.
static int tune_measure(bft_gpu* h, Tuned& t) {
    const uint64_t m = 1ull << 22;
    DevBuf q, bits;
    CK(q.alloc(m * h->B));
    CK(bits.alloc(((m + 63) / 64) * 8));
    const dim3 grid(bft_grid_for((m + 255) / 256)), block(256);
    switch (h->W) {
    case 1: hipLaunchKernelGGL(k_tune_queries<1>, grid, block, 0, h->stream, h->im.tk, h->n_kmers, h->k, h->B, m, q.as<uint8_t>()); break;
    case 2: hipLaunchKernelGGL(k_tune_queries<2>, grid, block, 0, h->stream, h->im.tk, h->n_kmers, h->k, h->B, m, q.as<uint8_t>()); break;
    case 3: hipLaunchKernelGGL(k_tune_queries<3>, grid, block, 0, h->stream, h->im.tk, h->n_kmers, h->k, h->B, m, q.as<uint8_t>()); break;
    default: hipLaunchKernelGGL(k_tune_queries<4>, grid, block, 0, h->stream, h->im.tk, h->n_kmers, h->k, h->B, m, q.as<uint8_t>()); break;
    }
    HIPCK(hipGetLastError());
    TuneEvents ev;
    if (hipEventCreate(&ev.e0) != hipSuccess || hipEventCreate(&ev.e1) != hipSuccess) return bft_fail(BFT_GPU_E_HIP, "hipEventCreate failed");
    // the batch `reps` times over image im at residency res: the first repetition warms the caches, the best of the others counts
    auto measure = [&](const BftImage& im, int res, int reps, float& best) {
        const WalkShape sh = walk_shape(res);
        for (int rep = 0; rep < reps; rep++) {
            if (hipEventRecord(ev.e0, h->stream) != hipSuccess) return bft_fail(BFT_GPU_E_HIP, "hipEventRecord failed");
            CK(launch_walk(h, im, sh, q.as<uint8_t>(), m, bits.as<uint64_t>(), nullptr, h->stream, h->B));
            if (hipEventRecord(ev.e1, h->stream) != hipSuccess || hipEventSynchronize(ev.e1) != hipSuccess) return bft_fail(BFT_GPU_E_HIP, "k_query failed while tuning");
            float ms = 0;
            if (hipEventElapsedTime(&ms, ev.e0, ev.e1) != hipSuccess) return bft_fail(BFT_GPU_E_HIP, "hipEventElapsedTime failed");
            if (rep > 0 && ms < best) best = ms;
        }
        return 0;
    };
    BftImage im = h->im;  // the candidates: rows are not asked for, so plain root groups are never looked up in the k-mer hash
    im.walk_kh = 0;
    im.debug_stop = 0;  // (only read by -DBFT_PERF_PROBE builds)
    // (residency 1 / 2 / 3) x (probe block 4 / 8 rows); options fixed by the caller are not varied
    for (int cfg = 0; cfg < 6; cfg++) {
        const int wgs = 1 + cfg % 3, probe = cfg >= 3 ? 8 : 4;
        if ((h->opt_wgs_per_cu && h->opt_wgs_per_cu != wgs) || (h->opt_probe && h->opt_probe != probe) || (h->W > BFT_PROBE_MAX_W && probe == 8))
            continue;
        im.probe_big = bft_probe_mode(probe);
        CK(measure(im, wgs, 2, t.best[cfg]));
    }
    // Residency 3 is the incumbent: on full batches and on the eight walks per k-mer of k_branching it is as fast as the better of
    // the other two or 5-15 % faster (k = 36..63, config 5), and the 2^22-query tuning batch resolves differences of a few per
    // cent poorly -- another arrangement has to win by more than 4 %.
    int win = -1;
    float win_score = 1e30f;
    for (int cfg = 0; cfg < 6; cfg++) {
        if (t.best[cfg] >= 1e29f) continue;
        const float score = t.best[cfg] * (cfg % 3 == 2 ? 0.96f : 1.0f);
        if (score < win_score) { win_score = score; win = cfg; }
    }
    if (win < 0) win = 1;
    t.wgs = 1 + win % 3;
    t.probe = win >= 3 ? 8 : 4;
    // root level: range table + direct table, or the direct table alone ("root_direct" 3).  The range table halves the L2
    // footprint of the root level; its special prefixes (child Nodes) pay one more dependent load -- which side wins depends
    // on how many there are, so both are timed with the residency / probe mode just chosen.
    if (h->opt_root_direct == 3 && h->rstart_ok) {
        im.probe_big = bft_probe_mode(h->opt_probe ? h->opt_probe : t.probe);
        for (int mode = 0; mode < 2; mode++) {
            im.rstart = mode ? h->d_rstart.as<uint32_t>() : nullptr;
            im.rq = mode && h->rq_ok ? h->d_rq.as<uint32_t>() : nullptr;
            CK(measure(im, h->opt_wgs_per_cu ? h->opt_wgs_per_cu : t.wgs, 3, t.rs[mode]));
        }
        t.rstart = t.rs[1] < t.rs[0] ? 1 : 0;
    }
    return 0;
}

// bft_gpu_set_option("tune", 1): the launch shape of the container walk measured on THIS image, on a batch drawn from the index
// (synchronises; never called implicitly -- a build or a query only ever applies default_launch_shape).  The handle is written here and
// nowhere else: once, with what was measured.
int bft_tune_residency(bft_gpu* h) {
    if (h->n_kmers < (1u << 16)) {  // small (L2-resident) indexes: always two workgroups, 4-row probes
        h->tuned_wgs = 2;
        h->tuned_probe = 4;
        h->im.probe_big = bft_probe_mode(h->opt_probe);
        return 0;
    }
    Tuned t;
    const int rc = tune_measure(h, t);
    if (rc) {  // nothing measured stands: two workgroups per CU (bft_query_residency) and the option's probe mode, as a failed tune always left them
        h->tuned_wgs = 0;
        h->im.probe_big = bft_probe_mode(h->opt_probe);
        return rc;
    }
    for (int r = 0; r < 3; r++) h->tune_ms[r] = std::min(t.best[r], t.best[r + 3]) < 1e29f ? std::min(t.best[r], t.best[r + 3]) : 0;
    h->tuned_wgs = t.wgs;
    h->tuned_probe = t.probe;
    h->im.probe_big = bft_probe_mode(h->opt_probe ? h->opt_probe : t.probe);
    if (t.rstart >= 0) {
        h->rstart_tune_ms[0] = t.rs[0];
        h->rstart_tune_ms[1] = t.rs[1];
        h->tuned_rstart = t.rstart;
        h->im.rstart = t.rstart ? h->d_rstart.as<uint32_t>() : nullptr;
        h->im.rq = t.rstart && h->rq_ok ? h->d_rq.as<uint32_t>() : nullptr;
    }
    return 0;
}

// ------------------------------------------------------------------------------------------------
// branching
// ------------------------------------------------------------------------------------------------
// eight walks per k-mer over image im at shape sh (the residency measured for k_query applies); h: the device, the root's CC count, B
static int launch_branching_walk(const bft_gpu* h, const BftImage& im, const WalkShape& sh, const uint8_t* d_kmers, uint64_t n, uint64_t* d_bits64, uint8_t* d_counts, hipStream_t s) {
    const uint64_t nblk = (n + sh.block - 1) / sh.block;
    const uint64_t grid_cap = h->opt_test_walk_grid ? h->opt_test_walk_grid : ~0ull;  // ("test_walk_grid")
    const dim3 grid((unsigned)std::max<uint64_t>(1, std::min<uint64_t>(std::min<uint64_t>(nblk, sh.resident), grid_cap)));
    return walk_dispatch<false>(h, false, [&](auto w, auto staged, auto probe) {
        constexpr int W = decltype(w)::value, PROBE = decltype(probe)::value;
        constexpr bool STAGED = decltype(staged)::value;
        static std::atomic<uint64_t> lds_allowed{0};
        CK(allow_walk_lds(lds_allowed, h->device,
                          {(const void*)k_branching<W, 1024, STAGED, PROBE>, (const void*)k_branching8<W, 1024, STAGED, PROBE>, (const void*)k_branching6<W, STAGED, PROBE>}));
        if (sh.res == 1) hipLaunchKernelGGL((k_branching<W, 1024, STAGED, PROBE>), grid, dim3(sh.block), sh.lds, s, im, d_kmers, n, h->B, d_bits64, d_counts);
        else if (sh.res == 3) hipLaunchKernelGGL((k_branching6<W, STAGED, PROBE>), grid, dim3(sh.block), sh.lds, s, im, d_kmers, n, h->B, d_bits64, d_counts);
        else hipLaunchKernelGGL((k_branching8<W, 1024, STAGED, PROBE>), grid, dim3(sh.block), sh.lds, s, im, d_kmers, n, h->B, d_bits64, d_counts);
        HIPCK(hipGetLastError());
        return 0;
    });
}

static int launch_branching(bft_gpu* h, const uint8_t* d_kmers, uint64_t n, uint64_t* d_bits64, uint8_t* d_counts, hipStream_t s) {
    if (n == 0) return 0;
    hipEvent_t e0, e1;
    CK(bft_timing_begin(h, s, &e0, &e1));
    if (h->im.kh_lines != nullptr) {  // eight candidates per k-mer, each one cache line of the k-mer hash, four in flight at a time
        const ClaimSlots::Claim claim = h->claims.take(s, claims_wanted(h, n * 8), (n + 255) / 256);
        CK(bft_kh_branching(h->im, d_kmers, n, h->B, d_bits64, d_counts, claim.ctr, h->opt_query_chunk, s));
        h->claims.launched(claim.slot, s);
    } else
        CK(launch_branching_walk(h, h->im, walk_shape(bft_query_residency(h)), d_kmers, n, d_bits64, d_counts, s));
    return bft_timing_end(h, s, e0, e1);
}

extern "C" int bft_gpu_query_branching_dev(bft_gpu* h, const void* d_kmers, uint64_t n, void* d_branching_bits, void* d_counts, void* hip_stream) {
    if (!h || ((!d_kmers || !d_branching_bits) && n)) return bft_fail(BFT_GPU_E_ARG, "NULL argument");
    ENTER(h);
    CK(bft_ensure_built(h, false));  // (the k-mer hash answers; the walk fetches the table itself)
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : h->stream;
    CK(launch_branching(h, (const uint8_t*)d_kmers, n, (uint64_t*)d_branching_bits, (uint8_t*)d_counts, s));
    return bft_note_foreign_stream(h, s);
}

extern "C" int bft_gpu_query_branching(bft_gpu* h, const uint8_t* kmers, uint64_t n, uint8_t* branching_bits, uint8_t* counts) {
    if (!h || ((!kmers || !branching_bits) && n)) return bft_fail(BFT_GPU_E_ARG, "NULL argument");
    ENTER(h);
    CK(bft_ensure_built(h, false));  // (the k-mer hash answers; the walk fetches the table itself)
    const uint64_t chunk = 1ull << 26;
    const uint64_t mc = std::min(n, chunk);
    DevBuf dk, db, dc;
    CK(dk.alloc(mc * h->B));
    CK(db.alloc(((mc + 63) / 64) * 8));
    if (counts) CK(dc.alloc(mc));
    for (uint64_t a = 0; a < n; a += chunk) {
        const uint64_t m = std::min(chunk, n - a);
        HIPCK(hipMemcpyAsync(dk.p, kmers + a * h->B, m * h->B, hipMemcpyHostToDevice, h->stream));
        CK(launch_branching(h, dk.as<uint8_t>(), m, db.as<uint64_t>(), counts ? dc.as<uint8_t>() : nullptr, h->stream));
        HIPCK(hipMemcpyAsync(branching_bits + a / 8, db.p, (m + 7) / 8, hipMemcpyDeviceToHost, h->stream));
        if (counts) HIPCK(hipMemcpyAsync(counts + a, dc.p, m, hipMemcpyDeviceToHost, h->stream));
        HIPCK(hipStreamSynchronize(h->stream));
    }
    return BFT_GPU_OK;
}

// ------------------------------------------------------------------------------------------------
// presence, colour lists, colour rows
// ------------------------------------------------------------------------------------------------
extern "C" int bft_gpu_query_presence_dev(bft_gpu* h, const void* d_kmers, uint64_t n, void* d_present_bits, void* hip_stream) {
    if (!h || ((!d_kmers || !d_present_bits) && n)) return bft_fail(BFT_GPU_E_ARG, "NULL argument");
    ENTER(h);
    CK(bft_ensure_built(h, false));  // (the k-mer hash answers; the walk fetches the table itself)
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : h->stream;
    CK(bft_launch_query(h, (const uint8_t*)d_kmers, n, (uint64_t*)d_present_bits, nullptr, s));
    return bft_note_foreign_stream(h, s);
}

// ---- small host batches through the pinned block -------------------------------------------------------------------------
#define BFT_PIN_MAX_N 4096u                       // k-mers per call served this way
#define BFT_PIN_IN (BFT_PIN_MAX_N * 32u)          // B <= 32 bytes per k-mer
#define BFT_PIN_BITS_OFF BFT_PIN_IN
#define BFT_PIN_ROWS_OFF (BFT_PIN_BITS_OFF + BFT_PIN_MAX_N / 8u)
#define BFT_PIN_SETS_OFF (BFT_PIN_ROWS_OFF + BFT_PIN_MAX_N * 4u)
#define BFT_PIN_BYTES (BFT_PIN_SETS_OFF + BFT_PIN_MAX_N * 4u)

static int pin_block(bft_gpu* h) {
    if (h->pin) return 0;
    void* p = nullptr;
    HIPCK(hipHostMalloc(&p, BFT_PIN_BYTES, hipHostMallocMapped));
    h->pin = (uint8_t*)p;
    return 0;
}

// presence (+ rows, + colour-set ids) of n <= BFT_PIN_MAX_N host k-mers; any output pointer may be NULL
static int query_small(bft_gpu* h, const uint8_t* kmers, uint64_t n, uint8_t* present_bits, uint32_t* rows, uint32_t* colorsets) {
    CK(pin_block(h));
    uint8_t* pin = h->pin;
    memcpy(pin, kmers, n * h->B);
    uint32_t* prow = (uint32_t*)(pin + BFT_PIN_ROWS_OFF);
    uint32_t* pset = (uint32_t*)(pin + BFT_PIN_SETS_OFF);
    const bool want_rows = rows || colorsets;
    CK(bft_launch_query(h, pin, n, (uint64_t*)(pin + BFT_PIN_BITS_OFF), want_rows ? prow : nullptr, h->stream));
    if (colorsets) {
        hipLaunchKernelGGL(k_row_colorsets, dim3(bft_grid_for((n + 255) / 256)), dim3(256), 0, h->stream, prow, h->im.tcol, n, pset);
        HIPCK(hipGetLastError());
    }
    HIPCK(hipStreamSynchronize(h->stream));
    if (present_bits) memcpy(present_bits, pin + BFT_PIN_BITS_OFF, (n + 7) / 8);
    if (rows) memcpy(rows, prow, n * 4);
    if (colorsets) memcpy(colorsets, pset, n * 4);
    return BFT_GPU_OK;
}

extern "C" int bft_gpu_query_presence(bft_gpu* h, const uint8_t* kmers, uint64_t n, uint8_t* present_bits) {
    if (!h || ((!kmers || !present_bits) && n)) return bft_fail(BFT_GPU_E_ARG, "NULL argument");
    ENTER(h);
    CK(bft_ensure_built(h, false));  // (the k-mer hash answers; the walk fetches the table itself)
    if (n && n <= BFT_PIN_MAX_N) return query_small(h, kmers, n, present_bits, nullptr, nullptr);
    const uint64_t chunk = 1ull << 26;  // multiple of 64: chunks are byte aligned in the bitmap
    DevBuf dk, db;
    CK(dk.alloc(std::min(n, chunk) * h->B));
    CK(db.alloc(((std::min(n, chunk) + 63) / 64) * 8));
    for (uint64_t a = 0; a < n; a += chunk) {
        const uint64_t m = std::min(chunk, n - a);
        HIPCK(hipMemcpyAsync(dk.p, kmers + a * h->B, m * h->B, hipMemcpyHostToDevice, h->stream));
        CK(bft_launch_query(h, dk.as<uint8_t>(), m, db.as<uint64_t>(), nullptr, h->stream));
        HIPCK(hipMemcpyAsync(present_bits + a / 8, db.p, (m + 7) / 8, hipMemcpyDeviceToHost, h->stream));
        HIPCK(hipStreamSynchronize(h->stream));
    }
    return BFT_GPU_OK;
}

// shared front half of the colour queries: rows + presence bits for one chunk
static int query_rows(bft_gpu* h, const uint8_t* kmers, uint64_t m, DevBuf& dk, DevBuf& db, DevBuf& dr, uint8_t* present_bits) {
    HIPCK(hipMemcpyAsync(dk.p, kmers, m * h->B, hipMemcpyHostToDevice, h->stream));
    CK(bft_launch_query(h, dk.as<uint8_t>(), m, db.as<uint64_t>(), dr.as<uint32_t>(), h->stream));
    if (present_bits) HIPCK(hipMemcpyAsync(present_bits, db.p, (m + 7) / 8, hipMemcpyDeviceToHost, h->stream));
    return 0;
}

// get_annotation + get_list_id_genomes for a resident batch (src/bft.c:363-387, 622-641; src/annotation.c:2086-2250): the k-mer hash hands out
// the colour-set id of every found k-mer (emit_cs: the same line that answers presence), the lists' lengths are scanned into offsets straight
// from the dictionary, and the wavefronts stream the ids out.  No row, no sorted table ("compact_table" stays), no host round trip.
static int colors_core(bft_gpu* h, const uint8_t* d_kmers, uint64_t n, uint64_t* d_bits64, uint64_t* d_offsets, uint32_t* d_ids, uint64_t ids_cap, uint64_t* d_needed,
                       hipStream_t s, bool fill) {
    HandleScratch::Lease lease(h->qc);  // (the scratch's use ends with this function)
    CK(lease.acquire(s, bft_stream_capturing(s)));
    if (fill && h->im.kh_lines != nullptr && !h->opt_walk_hash && bft_kh_has_kernels(h->W, h->im.kh.S) && h->im.nb_genomes < 65536u) {  // (k_colors_kh keeps list lengths in 16 bits)
        // through the k-mer hash: lookup, offsets and ids in ONE launch (k_colors_kh; the host entry point counts first and fills per chunk: the three steps below)
        // (a block of its own: the kernel writes its counter and states raw, which a block of bft_scan's -- qc_tmp -- must never see)
        const size_t sb = bft_kh_colors_scratch_bytes(n);
        CK(h->qc.grow(h->qc_kh, sb, sb / 2));
        CK(bft_timed_launch(h, s, [&] { return bft_kh_colors(h->im, d_kmers, n, h->B, d_bits64, d_offsets, d_ids, d_ids ? ids_cap : 0, d_needed, h->qc_kh.p, s); }));
        return 0;
    }
    const size_t tb = bft_scan::scratch_bytes(n + 1);  // (the scan's tile states)
    CK(h->qc.grow(h->qc_cs, n * 4, n / 2));
    CK(h->qc.grow(h->qc_tmp, tb, tb / 2));
    uint32_t* d_cs = h->qc_cs.as<uint32_t>();
    {   // (the k-mer hash has the colour set in the line that answers presence; the walk, on an image without the table, takes it from tcol[row])
        h->im.emit_cs = 1;
        const int rc = bft_launch_query(h, d_kmers, n, d_bits64, d_cs, s);
        h->im.emit_cs = 0;
        CK(rc);
    }
    const BftCsLen len{d_cs, h->im.cs_off, n};
    CK((bft_scan::exclusive_sum<uint64_t>(len, d_offsets, n + 1, s, h->qc_tmp)));
    if (fill) {
        CK(bft_timed_launch(h, s, [&] {
            hipLaunchKernelGGL(k_color_fill_cs, dim3(bft_grid_for((n + 255) / 256)), dim3(256), 0, s, d_cs, h->im.cs_off, h->im.cs_ids, h->im.cs_w, d_offsets, n, ids_cap, d_ids, d_needed);
            HIPCK(hipGetLastError());
            return 0;
        }));
    }
    return 0;
}

extern "C" int bft_gpu_query_colors_dev(bft_gpu* h, const void* d_kmers, uint64_t n, void* d_present_bits, void* d_offsets, void* d_ids, uint64_t ids_cap,
                                        void* d_ids_needed, void* hip_stream) {
    if (!h || !d_offsets || ((!d_kmers || !d_present_bits) && n)) return bft_fail(BFT_GPU_E_ARG, "NULL argument");
    ENTER(h);
    CK(bft_ensure_built(h, false));
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : h->stream;
    if (n == 0) {
        CK(bft_zero_async(d_offsets, 8, s));  // (kernels, not memsets, wherever a caller may be capturing: bft_dev.h)
        if (d_ids_needed) CK(bft_zero_async(d_ids_needed, 8, s));
        return bft_note_foreign_stream(h, s);
    }
    CK(colors_core(h, (const uint8_t*)d_kmers, n, (uint64_t*)d_present_bits, (uint64_t*)d_offsets, (uint32_t*)d_ids, ids_cap, (uint64_t*)d_ids_needed, s, true));
    return bft_note_foreign_stream(h, s);
}

// The host-buffer form: the resident one on staged chunks.
extern "C" int bft_gpu_query_colors(bft_gpu* h, const uint8_t* kmers, uint64_t n, uint8_t* present_bits, uint64_t* offsets,
                                    uint32_t* ids, uint64_t ids_cap, uint64_t* ids_needed) {
    if (!h || !offsets || ((!kmers) && n)) return bft_fail(BFT_GPU_E_ARG, "NULL argument");
    ENTER(h);
    CK(bft_ensure_built(h, false));
    const uint64_t chunk = 1ull << 24;
    const uint64_t mc = std::min(n, chunk);
    DevBuf dk, db, doff, dids;
    CK(dk.alloc(mc * h->B));
    CK(db.alloc(((mc + 63) / 64) * 8));
    CK(doff.alloc((mc + 1) * 8));
    uint64_t total = 0;
    bool overflow = false;
    for (uint64_t a = 0; a < n; a += chunk) {
        const uint64_t m = std::min(chunk, n - a);
        HIPCK(hipMemcpyAsync(dk.p, kmers + a * h->B, m * h->B, hipMemcpyHostToDevice, h->stream));
        CK(colors_core(h, dk.as<uint8_t>(), m, db.as<uint64_t>(), doff.as<uint64_t>(), nullptr, 0, nullptr, h->stream, false));
        if (present_bits) HIPCK(hipMemcpyAsync(present_bits + a / 8, db.p, (m + 7) / 8, hipMemcpyDeviceToHost, h->stream));
        HIPCK(hipMemcpyAsync(offsets + a, doff.p, (m + 1) * 8, hipMemcpyDeviceToHost, h->stream));
        HIPCK(hipStreamSynchronize(h->stream));
        const uint64_t cnt = offsets[a + m];
        if (total)
            for (uint64_t i = 0; i <= m; i++) offsets[a + i] += total;  // chunk-local -> global
        if (!overflow && ids && total + cnt <= ids_cap) {
            if (cnt) {
                CK(dids.alloc(cnt * 4));
                CK(bft_timed_launch(h, h->stream, [&] {
                    hipLaunchKernelGGL(k_color_fill_cs, dim3(bft_grid_for((m + 255) / 256)), dim3(256), 0, h->stream, h->qc_cs.as<uint32_t>(), h->im.cs_off, h->im.cs_ids, h->im.cs_w,
                                       doff.as<uint64_t>(), m, cnt, dids.as<uint32_t>(), (uint64_t*)nullptr);
                    HIPCK(hipGetLastError());
                    return 0;
                }));
                HIPCK(hipMemcpyAsync(ids + total, dids.p, cnt * 4, hipMemcpyDeviceToHost, h->stream));
                HIPCK(hipStreamSynchronize(h->stream));
            }
        } else
            overflow = true;
        total += cnt;
    }
    if (n == 0) offsets[0] = 0;
    if (ids_needed) *ids_needed = total;
    if (overflow) return bft_fail(BFT_GPU_E_NOSPACE, "ids buffer too small");
    return BFT_GPU_OK;
}

// Bitmap form of the colour-set dictionary (one dword-aligned row per set), used by the colour-row queries when it stays
// below 4 GiB; derived on the first such query of an image, on the handle's stream.
int bft_ensure_cs_bitmaps(bft_gpu* h) {
    if (h->cs_bm_tried) return 0;
    h->cs_bm_tried = true;
    if (h->opt_no_cs_bitmaps) return 0;  // ("test_no_cs_bitmaps": as if the bitmaps passed 4 GiB)
    const uint64_t rowbytes = (h->im.nb_genomes + 7) / 8, nsets = h->n_sets;
    if (rowbytes && nsets && nsets * rowbytes <= (4ull << 30)) {
        const uint64_t stride = (rowbytes + 3) & ~3ull;  // dword-aligned dictionary rows (k_color_rows_bm)
        // (CS_BM_SLACK zero bytes in front of the first row and behind the last: k_color_rows_bm16 loads 16 bytes from up to 15 bytes before a row
        // and up to its last byte)
        CK(h->d_cs_bm.alloc_zero(nsets * stride + 2 * CS_BM_SLACK, h->stream));
        hipLaunchKernelGGL(k_cs_bitmaps, dim3(bft_grid_for((nsets + 255) / 256)), dim3(256), 0, h->stream, h->im.cs_off, h->im.cs_ids, h->im.cs_w, nsets, (uint32_t)stride,
                           h->d_cs_bm.as<uint8_t>() + CS_BM_SLACK);
        HIPCK(hipGetLastError());
        HIPCK(hipStreamSynchronize(h->stream));  // the row kernel may run on a caller's stream
        h->has_cs_bm = true;
    }
    return 0;
}

// d_rowidx: the row of every k-mer (scratch: overwritten with the colour-set ids when the bitmap dictionary is used)
static int launch_color_rows(bft_gpu* h, uint32_t* d_rowidx, uint64_t n, uint32_t rowbytes, uint8_t* d_out, hipStream_t s, bool are_colorsets = false) {
    CK(bft_ensure_cs_bitmaps(h));
    hipEvent_t e0, e1;
    CK(bft_timing_begin(h, s, &e0, &e1));
    if (h->has_cs_bm) {
        if (!are_colorsets)
            hipLaunchKernelGGL(k_row_colorsets, dim3(bft_grid_for((n + 255) / 256)), dim3(256), 0, s, d_rowidx, h->im.tcol, n, d_rowidx);  // row -> colour set, in place
        // (16-byte rows and up, 16-byte aligned output: the 16-bytes-per-lane kernel, whose tiles are a multiple of 16 k-mers)
        const bool wide16 = rowbytes >= 16 && ((uintptr_t)d_out & 15u) == 0;
        // the tile (a multiple of 4 / 16 k-mers) and the magic number of the division by rowbytes: bft_color_plan.h
        const BftColorRowsPlan plan = bft_color_rows_plan(rowbytes, wide16 ? BFT_ROWS_FORM_16 : BFT_ROWS_FORM_DWORD);
        const uint32_t tile_rows = plan.tile_rows, div_m = plan.div_m, div_l = plan.div_l;
        const uint64_t tiles = (n + tile_rows - 1) / tile_rows;
        dim3 cgrid((unsigned)std::min<uint64_t>(tiles, 256ull * 8));
        if (wide16) {
            // the tiles are dealt out by workgroup number: a grid larger than what is resident would run its last workgroups -- with all
            // their tiles -- behind the others (82 registers: five workgroups per CU, not eight)
            static std::atomic<int> resident16_dev[64];  // per device: CU count and partition mode may differ between the GPUs of a process
            std::atomic<int>& resident16 = resident16_dev[h->device & 63];
            int r = resident16.load(std::memory_order_relaxed);
            if (!r) {
                int per_cu = 0, cus = 0;
                if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_color_rows_bm16, 256, 0) != hipSuccess || per_cu < 1) { per_cu = 4; (void)hipGetLastError(); }
                if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device) != hipSuccess || cus < 1) { cus = 256; (void)hipGetLastError(); }
                r = per_cu * cus;
                resident16.store(r, std::memory_order_relaxed);
            }
            cgrid = dim3((unsigned)std::min<uint64_t>((tiles + 3) / 4, (uint64_t)r));
        }
        if (wide16)
            hipLaunchKernelGGL(k_color_rows_bm16, cgrid, dim3(256), 0, s, d_rowidx, h->d_cs_bm.as<uint8_t>() + CS_BM_SLACK, (rowbytes + 3) & ~3u, n, rowbytes, tile_rows, div_m,
                               div_l, d_out);
        else if (rowbytes >= 4)
            hipLaunchKernelGGL(k_color_rows_bm<true>, cgrid, dim3(256), 0, s, d_rowidx, h->d_cs_bm.as<uint8_t>() + CS_BM_SLACK, (rowbytes + 3) & ~3u, n, rowbytes, tile_rows, div_m,
                               div_l, d_out);
        else
            hipLaunchKernelGGL(k_color_rows_bm<false>, cgrid, dim3(256), 0, s, d_rowidx, h->d_cs_bm.as<uint8_t>() + CS_BM_SLACK, (rowbytes + 3) & ~3u, n, rowbytes, tile_rows, div_m,
                               div_l, d_out);
    }
    else
        hipLaunchKernelGGL(k_color_rows, dim3(bft_grid_for((n + 255) / 256)), dim3(256), 0, s, d_rowidx, h->im.tcol, h->im.cs_off, h->im.cs_ids, h->im.cs_w, n, rowbytes, d_out);
    HIPCK(hipGetLastError());
    return bft_timing_end(h, s, e0, e1);
}

// device-resident colour rows: presence bits + CEIL(nb_genomes/8)-byte bitmap row per k-mer, no synchronisation
extern "C" int bft_gpu_query_color_rows_dev(bft_gpu* h, const void* d_kmers, uint64_t n, void* d_present_bits, void* d_rows, void* d_scratch_rows_u32,
                                            void* hip_stream) {
    if (!h || ((!d_kmers || !d_present_bits || !d_rows || !d_scratch_rows_u32) && n)) return bft_fail(BFT_GPU_E_ARG, "NULL argument");
    ENTER(h);
    CK(bft_ensure_built(h, false));
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : h->stream;
    const uint32_t rowbytes = (h->im.nb_genomes + 7) / 8;
    if (n == 0 || rowbytes == 0) return BFT_GPU_OK;
    // with the bitmap dictionary the query kernel writes colour sets straight away (the k-mer hash holds them; bft_hit_out in the
    // walk): no row -> colour set pass
    CK(bft_ensure_cs_bitmaps(h));
    const bool direct = h->has_cs_bm;
    // rows of 16 bytes and up through the k-mer hash: lookup and rows in one launch (the scratch array stays unused)
    if (direct && rowbytes >= 16 && ((uintptr_t)d_rows & 15u) == 0 && h->im.kh_lines != nullptr && !h->opt_walk_hash && bft_kh_has_kernels(h->W, h->im.kh.S)) {
        CK(bft_timed_launch(h, s, [&] {
            return bft_kh_color_rows(h->im, (const uint8_t*)d_kmers, n, h->B, (uint64_t*)d_present_bits, h->d_cs_bm.as<uint8_t>() + CS_BM_SLACK, (rowbytes + 3) & ~3u, rowbytes,
                                     (uint8_t*)d_rows, h->device, s);
        }));
        return bft_note_foreign_stream(h, s);
    }
    if (!direct) CK(bft_ensure_table(h));
    if (direct) h->im.emit_cs = 1;
    const int rc = bft_launch_query(h, (const uint8_t*)d_kmers, n, (uint64_t*)d_present_bits, (uint32_t*)d_scratch_rows_u32, s);
    h->im.emit_cs = 0;
    CK(rc);
    CK(launch_color_rows(h, (uint32_t*)d_scratch_rows_u32, n, rowbytes, (uint8_t*)d_rows, s, direct));
    return bft_note_foreign_stream(h, s);
}

extern "C" int bft_gpu_query_color_rows(bft_gpu* h, const uint8_t* kmers, uint64_t n, uint8_t* present_bits, uint8_t* rows) {
    if (!h || !rows || (!kmers && n)) return bft_fail(BFT_GPU_E_ARG, "NULL argument");
    ENTER(h);
    CK(bft_ensure_built(h));
    const uint32_t rowbytes = (h->im.nb_genomes + 7) / 8;
    if (rowbytes == 0) return BFT_GPU_OK;
    const uint64_t chunk = 1ull << 22;
    const uint64_t mc = std::min(n, chunk);
    DevBuf dk, db, dr, dout;
    CK(dk.alloc(mc * h->B));
    CK(db.alloc(((mc + 63) / 64) * 8));
    CK(dr.alloc(mc * 4));
    CK(dout.alloc(mc * rowbytes));
    for (uint64_t a = 0; a < n; a += chunk) {
        const uint64_t m = std::min(chunk, n - a);
        CK(query_rows(h, kmers + a * h->B, m, dk, db, dr, present_bits ? present_bits + a / 8 : nullptr));
        CK(launch_color_rows(h, dr.as<uint32_t>(), m, rowbytes, dout.as<uint8_t>(), h->stream));
        HIPCK(hipMemcpyAsync(rows + a * rowbytes, dout.p, m * rowbytes, hipMemcpyDeviceToHost, h->stream));
        HIPCK(hipStreamSynchronize(h->stream));
    }
    return BFT_GPU_OK;
}

// ------------------------------------------------------------------------------------------------
// sequence queries
// ------------------------------------------------------------------------------------------------
// query_sequence (src/bft.c:1241-1351) for a batch of ASCII sequences
// Sequence queries on device-resident input.  Scratch (codes, plan, colour set per position) belongs to the handle and only grows; calls on
// different streams take turns on it.  Nothing here waits for the GPU: the positions of a chunk are counted on the device
// (k_seq_plan + scan) and the kernels read the total from there.
// The colour set of every k-mer position of a chunk (h->sq_cs) from the arrays of query_sequences_core, through the k-mer hash where the image has one
// (units: a bound on the blocks of k-mer positions that kernel deals out, for its claim), else through the walk: a fixed grid of 512 workgroups, of
// 1024 threads (two per CU) or, for two-word keys, of 768.
static int launch_seq_lookups(bft_gpu* h, const BftImage& image, uint32_t ns, int canonical, const uint64_t* d_soff, uint64_t units, hipStream_t s) {
    if (image.kh_lines != nullptr) {
        const ClaimSlots::Claim claim = h->claims.take(s, claims_wanted(h, h->opt_query_dynamic_min), units);
        CK(bft_kh_seq(image, h->sq_codes.as<uint64_t>(), h->sq_bad.as<uint32_t>(), d_soff, h->sq_poff.as<uint64_t>(), h->sq_tile.as<uint32_t>(), ns, canonical,
                      h->sq_cs.as<uint32_t>(), claim.ctr, h->opt_query_chunk, s));
        h->claims.launched(claim.slot, s);
        return 0;
    }
    BftImage im = image;
    im.emit_cs = 1;
    return walk_dispatch<false>(h, false, [&](auto w, auto staged, auto probe) {
        constexpr int W = decltype(w)::value, PROBE = decltype(probe)::value;
        constexpr bool STAGED = decltype(staged)::value;
        static std::atomic<uint64_t> lds_allowed{0};
        auto launch = [&](auto kernel, const WalkShape& sh) {
            CK(allow_walk_lds(lds_allowed, h->device, {(const void*)kernel}));
            hipLaunchKernelGGL(kernel, dim3(512), dim3(sh.block), sh.lds, s, im, h->sq_codes.as<uint64_t>(), h->sq_bad.as<uint32_t>(), d_soff, h->sq_poff.as<uint64_t>(),
                               h->sq_tile.as<uint32_t>(), ns, canonical, h->sq_cs.as<uint32_t>());
            HIPCK(hipGetLastError());
            return 0;
        };
        if constexpr (W != 2) return launch(k_seq_walk8<W, STAGED, PROBE>, walk_shape(2));
        else return launch(k_seq_walk6<W, STAGED, PROBE>, walk_shape(3));
    });
}

static int query_sequences_core(bft_gpu* h, const char* d_seqs, const uint64_t* d_seq_off, uint64_t n_seqs, uint64_t total_chars, double threshold,
                                int canonical, uint8_t* d_rows, hipStream_t s) {
    const uint32_t G = h->im.nb_genomes, rowbytes = (G + 7) / 8;
    if (rowbytes == 0 || n_seqs == 0) return 0;
    HandleScratch::Lease lease(h->sq);  // (the scratch's use ends with this function)
    CK(lease.acquire(s, bft_stream_capturing(s)));
    auto need = [&](DevBuf& b, size_t bytes) { return h->sq.grow(b, bytes, bytes / 8); };
    // sequences per chunk: 32-bit sequence numbers
    const uint64_t chunk = 1ull << 30;
    const uint64_t cmax = std::min(chunk, n_seqs);
    const uint64_t n_cw = (total_chars + 31) / 32;  // code words of the blob (32 characters each)
    const size_t scan_bytes = bft_scan::scratch_bytes(cmax + 1);  // (the scan's tile states)
    CK(need(h->sq_codes, (n_cw + BFT_MAX_W + 2) * 8));
    CK(need(h->sq_bad, (n_cw + BFT_MAX_W + 2) * 4));
    CK(need(h->sq_npos, (cmax + 1) * 8));
    CK(need(h->sq_poff, (cmax + 1) * 8));
    CK(need(h->sq_tmp, scan_bytes));
    CK(need(h->sq_tile, (total_chars / 64 + 2) * 4));
    CK(need(h->sq_cs, (total_chars + 64) * 4));  // colour set of every k-mer position of a chunk (positions <= characters)
    // (the slack words behind the codes are read by windows at the very end of the blob: keep them defined)
    CK(bft_zero_async(h->sq_codes.as<uint64_t>() + n_cw, (BFT_MAX_W + 2) * 8, s));
    CK(bft_zero_async(h->sq_bad.as<uint32_t>() + n_cw, (BFT_MAX_W + 2) * 4, s));
    if (n_cw)
        CK(bft_timed_launch(h, s, [&] {
            hipLaunchKernelGGL(k_seq_encode, dim3(bft_grid_for((n_cw + 255) / 256)), dim3(256), 0, s, d_seqs, total_chars, n_cw, h->sq_codes.as<uint64_t>(),
                               h->sq_bad.as<uint32_t>());
            HIPCK(hipGetLastError());
            return 0;
        }));
    for (uint64_t a = 0; a < n_seqs; a += chunk) {
        const uint64_t ns = std::min(chunk, n_seqs - a);
        const uint64_t* soff = d_seq_off + a;
        CK(bft_timed_launch(h, s, [&] {  // (the plan: positions per read, their offsets, the tile table)
            hipLaunchKernelGGL(k_seq_plan, dim3(bft_grid_for((ns + 256) / 256)), dim3(256), 0, s, soff, ns, h->k, h->sq_npos.as<uint64_t>());
            CK(bft_scan::exclusive_sum_ptr<uint64_t>(h->sq_npos.as<uint64_t>(), h->sq_poff.as<uint64_t>(), ns + 1, s, h->sq_tmp));
            hipLaunchKernelGGL(k_seq_tiles, dim3(256 * 4), dim3(256), 0, s, h->sq_poff.as<uint64_t>(), (uint32_t)ns, h->sq_tile.as<uint32_t>());
            HIPCK(hipGetLastError());
            return 0;
        }));
        // (k-mer positions <= characters: total_chars / 256 + 2 bounds the blocks the kernel can deal out)
        CK(bft_timed_launch(h, s, [&] { return launch_seq_lookups(h, h->im, (uint32_t)ns, canonical, soff, total_chars / 256 + 2, s); }));
        const uint32_t win = std::min<uint32_t>(SEQ_TALLY_G, (G + 63u) & ~63u);  // counters per wavefront: all genomes up to 2048
        CK(bft_timed_launch(h, s, [&] {
            hipLaunchKernelGGL(k_seq_tally, dim3((unsigned)std::min<uint64_t>((ns + SEQ_TALLY_WAVES - 1) / SEQ_TALLY_WAVES, 256ull * 16)), dim3(64 * SEQ_TALLY_WAVES),
                               (size_t)SEQ_TALLY_WAVES * win * 4, s, h->sq_cs.as<uint32_t>(), h->sq_poff.as<uint64_t>(), (uint32_t)ns, h->im.cs_off, h->im.cs_ids, h->im.cs_w, G,
                               rowbytes, threshold, win, d_rows + a * rowbytes);
            HIPCK(hipGetLastError());
            return 0;
        }));
    }
    return 0;
}

extern "C" int bft_gpu_query_sequences_dev(bft_gpu* h, const void* d_seqs, const void* d_seq_off, uint64_t n_seqs, uint64_t total_chars, double threshold,
                                           int canonical, void* d_rows, void* hip_stream) {
    if (!h || ((!d_seqs || !d_seq_off || !d_rows) && n_seqs)) return bft_fail(BFT_GPU_E_ARG, "NULL argument");
    if (!(threshold > 0) || threshold > 1) return bft_fail(BFT_GPU_E_ARG, "the threshold must be in (0, 1] (reference src/bft.c:1246-1247)");
    ENTER(h);
    CK(bft_ensure_built(h, false));  // (the k-mer hash answers; the walk fetches the table itself)
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : h->stream;
    CK(query_sequences_core(h, (const char*)d_seqs, (const uint64_t*)d_seq_off, n_seqs, total_chars, threshold, canonical, (uint8_t*)d_rows, s));
    return bft_note_foreign_stream(h, s);
}

extern "C" int bft_gpu_query_sequences(bft_gpu* h, const char* seqs, const uint64_t* seq_off, uint64_t n_seqs, double threshold, int canonical,
                                       uint8_t* rows) {
    if (!h || ((!seqs || !seq_off || !rows) && n_seqs)) return bft_fail(BFT_GPU_E_ARG, "NULL argument");
    if (!(threshold > 0) || threshold > 1) return bft_fail(BFT_GPU_E_ARG, "the threshold must be in (0, 1] (reference src/bft.c:1246-1247)");
    ENTER(h);
    CK(bft_ensure_built(h, false));  // (the k-mer hash answers; the walk fetches the table itself)
    const uint32_t G = h->im.nb_genomes, rowbytes = (G + 7) / 8;
    if (rowbytes == 0 || n_seqs == 0) return BFT_GPU_OK;
    // host buffers: the blob and its offsets (rebased to the first sequence) go up in pieces of at most 2^30 characters
    uint64_t a = 0;
    while (a < n_seqs) {
        uint64_t b = a + 1;
        while (b < n_seqs && seq_off[b + 1] - seq_off[a] <= (1ull << 30)) b++;
        const uint64_t ns = b - a, nchars = seq_off[b] - seq_off[a];
        std::vector<uint64_t> soff(ns + 1);
        for (uint64_t i = 0; i <= ns; i++) soff[i] = seq_off[a + i] - seq_off[a];
        DevBuf d_seq, d_soff, d_out;
        CK(d_seq.alloc(nchars + 16));
        CK(d_soff.alloc((ns + 1) * 8));
        CK(d_out.alloc(ns * rowbytes));
        HIPCK(hipMemcpyAsync(d_seq.p, seqs + seq_off[a], nchars, hipMemcpyHostToDevice, h->stream));
        HIPCK(hipMemcpyAsync(d_soff.p, soff.data(), (ns + 1) * 8, hipMemcpyHostToDevice, h->stream));
        CK(query_sequences_core(h, d_seq.as<char>(), d_soff.as<uint64_t>(), ns, nchars, threshold, canonical, d_out.as<uint8_t>(), h->stream));
        HIPCK(hipMemcpyAsync(rows + a * rowbytes, d_out.p, ns * rowbytes, hipMemcpyDeviceToHost, h->stream));
        HIPCK(hipStreamSynchronize(h->stream));
        a = b;
    }
    return BFT_GPU_OK;
}

// ------------------------------------------------------------------------------------------------
// rows
// ------------------------------------------------------------------------------------------------
// What the reference keeps in resultPresence (include/Node.h:60-92) for a found k-mer, as indexes instead of host pointers:
// the row of the k-mer in the sorted table (the order of bft_gpu_extract) and the id of its colour set.
extern "C" int bft_gpu_query_rows(bft_gpu* h, const uint8_t* kmers, uint64_t n, uint8_t* present_bits, uint32_t* rows, uint32_t* colorsets) {
    if (!h || (!kmers && n)) return bft_fail(BFT_GPU_E_ARG, "NULL argument");
    ENTER(h);
    CK(bft_ensure_built(h));
    if (n && n <= BFT_PIN_MAX_N) return query_small(h, kmers, n, present_bits, rows, colorsets);
    const uint64_t chunk = 1ull << 24;
    const uint64_t mc = std::min(n, chunk);
    DevBuf dk, db, dr, dc;
    CK(dk.alloc(mc * h->B));
    CK(db.alloc(((mc + 63) / 64) * 8));
    CK(dr.alloc(mc * 4));
    if (colorsets) CK(dc.alloc(mc * 4));
    for (uint64_t a = 0; a < n; a += chunk) {
        const uint64_t m = std::min(chunk, n - a);
        CK(query_rows(h, kmers + a * h->B, m, dk, db, dr, present_bits ? present_bits + a / 8 : nullptr));
        if (rows) HIPCK(hipMemcpyAsync(rows + a, dr.p, m * 4, hipMemcpyDeviceToHost, h->stream));
        if (colorsets) {
            hipLaunchKernelGGL(k_row_colorsets, dim3(bft_grid_for((m + 255) / 256)), dim3(256), 0, h->stream, dr.as<uint32_t>(), h->im.tcol, m, dc.as<uint32_t>());
            HIPCK(hipGetLastError());
            HIPCK(hipMemcpyAsync(colorsets + a, dc.p, m * 4, hipMemcpyDeviceToHost, h->stream));
        }
        HIPCK(hipStreamSynchronize(h->stream));
    }
    return BFT_GPU_OK;
}
