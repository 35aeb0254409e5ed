// bft_gpu.hip -- the C-ABI of include/bft_gpu.h: handle (bft_handle.h), device-memory cache, insertion log, bulk build (its run stage: bft_run.hip) and
// commit, options and info.  The image read out and in -- files, the replication blob, the read-outs, the width of the dictionary's ids -- is
// bft_image_io.hip; what the handle derives from a committed image -- root tables, k-mer hash, node prefix hash,
// launch shape, compact table -- is bft_derive.hip; the k-mer and sequence queries, their tuner and the claim slots are bft_query.hip; prefixes,
// sub-graphs, paths, components and the other analysis families sit beside their kernels.  Device code from
//   bft_kernels_query.h  k_pack_to_tform (packed 2-bit k-mers -> T-form words: the per-level rev[]/rotation work of
//                        src/presenceNode.c:1327-1371 done once per k-mer; over the declarations of bft_walk.h)
// The bulk build turns the log into a sorted, de-duplicated run in bft_run.hip (the library's own sort and scan: bft_sort.h, bft_scan.h);
// colour-set interning is bft_intern.hip, container assembly bft_assemble.hip, the flat form of the big CCs bft_flat.hip -- see DESIGN.md "Insertion".
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/bft_gpu.h"
#include "bft_assemble.h"
#include "bft_color_plan.h"
#include "bft_front.h"
#include "bft_handle.h"
#include "bft_hash.h"
#include "bft_index.h"
#include "bft_intern.h"
#include "bft_merge.h"
#include "bft_run_plan.h"
#include "bft_sort.h"
#include "bft_walk.h"

#define BFT_BLOCK 256
#define BFT_ABSENT_ROW 0xFFFFFFFFu
// Genome ids index colour rows of CEIL(nb_genomes/8) bytes and bit positions of annotations: ids from 2^24 on are refused
// (the reference's own annotation codec holds 6 bits per byte, include/log2.h:45-50: 2^24 ids already take 4-byte entries).
#define BFT_MAX_GENOME_ID (1u << 24)

static thread_local std::string g_err;
int bft_fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}
static int fail(int code, const std::string& msg) { return bft_fail(code, msg); }

double bft_now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
// BFT_GPU_TRACE_BUILD=1: host-side timeline of bft_gpu_build on stderr (where the host waits, allocates, reads counts back)
static bool g_trace = getenv("BFT_GPU_TRACE_BUILD") != nullptr;
static double g_trace_t0 = 0, g_trace_last = 0;
bool bft_trace_on(void) { return g_trace; }
void bft_trace_mark(const char* what) {
    if (!g_trace) return;
    const double t = bft_now_ms();
    if (!what) { g_trace_t0 = g_trace_last = t; return; }
    fprintf(stderr, "[bft_gpu build] %8.3f ms (+%.3f) %s\n", t - g_trace_t0, t - g_trace_last, what);
    g_trace_last = t;
}

// Stage record of a build ("build_stages" 1): bft_stage() drops an event on the build's stream where a stage ends and notes the
// bytes the stage's algorithm reads + writes (from its own array sizes); bft_gpu_build resolves the events into GPU time per stage
// when it is done (bft_gpu_build_stages).  The host's waits between stages are inside the figures: a stage is what the stream spent
// between two marks.  One build at a time per thread.
namespace {
struct StageMark { std::string name; double bytes; hipEvent_t ev; };
thread_local bool t_stages_on = false;
thread_local std::vector<StageMark> t_stage_marks;
thread_local std::vector<hipEvent_t> t_stage_pool;
}  // namespace
void bft_stage(const char* name, double bytes, hipStream_t s) {
    if (!t_stages_on) return;
    hipEvent_t ev = nullptr;
    if (!t_stage_pool.empty()) { ev = t_stage_pool.back(); t_stage_pool.pop_back(); }
    else if (hipEventCreate(&ev) != hipSuccess) { (void)hipGetLastError(); return; }
    if (hipEventRecord(ev, s) != hipSuccess) { (void)hipGetLastError(); t_stage_pool.push_back(ev); return; }
    t_stage_marks.push_back({name, bytes, ev});
}

#include "bft_kernels_query.h"  // k_pack_to_tform
// ------------------------------------------------------------------------------------------------
// device-memory cache (see bft_dev.h)
// ------------------------------------------------------------------------------------------------
namespace {
struct PoolBlock {
    void* p;
    size_t cap;
    int device;
    hipStream_t stream;
};
std::mutex g_pool_mu;
std::vector<PoolBlock> g_pool;
size_t g_pool_bytes = 0;
// cached, unused memory kept at most (per process): an eighth of the device's memory (36 GB of an MI355X's 288: the transients of a
// 2 x 10^8-pair build are ~12 GB, and a hipFree of a gigabyte block costs a device synchronisation and ~0.2 ms), 8 GiB at least,
// unless BFT_GPU_POOL_MAX_MB says otherwise (0 = no cache); torch's allocator cannot see these blocks, so the cap bounds what the
// library withholds from it
size_t pool_max_bytes() {
    static const size_t v = [] {
        const char* e = getenv("BFT_GPU_POOL_MAX_MB");
        if (e) return (size_t)strtoull(e, nullptr, 10) << 20;
        size_t fr = 0, tot = 0;
        if (hipMemGetInfo(&fr, &tot) != hipSuccess) { (void)hipGetLastError(); tot = 0; }
        return std::max<size_t>((size_t)8 << 30, tot / 8);
    }();
    return v;
}
constexpr size_t POOL_MAX_BLOCKS = 256;
// tag of a block whose stream was synchronised and destroyed since (a closed handle's): nothing to wait for, whoever takes it
const hipStream_t POOL_DRAINED = (hipStream_t)(uintptr_t)1;
double g_malloc_ms = 0;          // time spent in hipMalloc by this process (diagnostic: bft_gpu_build_time)
uint64_t g_malloc_calls = 0;
double g_free_ms = 0;            // ... and in hipFree
uint64_t g_free_calls = 0;
thread_local int t_pool_device = -1;
thread_local hipStream_t t_pool_stream = nullptr;

void pool_free_block(const PoolBlock& b) {
    int cur = -1;
    (void)hipGetDevice(&cur);
    if (cur != b.device) (void)hipSetDevice(b.device);
    (void)hipFree(b.p);
    if (cur != b.device && cur >= 0) (void)hipSetDevice(cur);
}
}  // namespace

void bft_pool_set_stream(int device, hipStream_t s) {
    t_pool_device = device;
    t_pool_stream = s;
}

int bft_pool_alloc(void** p, size_t n, size_t* cap) {
    *p = nullptr;
    n += 256;  // slack behind every device array: aligned multi-row probes may read past the last row (bft_load_pair)
    PoolBlock take{nullptr, 0, 0, nullptr};
    {
        std::lock_guard<std::mutex> lk(g_pool_mu);
        size_t best = (size_t)-1;
        for (size_t i = 0; i < g_pool.size(); i++) {
            const PoolBlock& b = g_pool[i];
            if (b.device != t_pool_device || b.cap < n || b.cap > n + n / 2 + 4096) continue;  // similar size only
            if (best == (size_t)-1 || b.cap < g_pool[best].cap) best = i;
        }
        if (best != (size_t)-1) {
            take = g_pool[best];
            g_pool[best] = g_pool.back();
            g_pool.pop_back();
            g_pool_bytes -= take.cap;
        }
    }
    if (take.p) {
        // released under another stream: its work must have drained before the block is written again
        if (take.stream != t_pool_stream && take.stream != POOL_DRAINED && hipStreamSynchronize(take.stream) != hipSuccess) {
            pool_free_block(take);
            take.p = nullptr;
        }
    }
    if (take.p) {
        *p = take.p;
        *cap = take.cap;
        return 0;
    }
    const double t_m0 = bft_now_ms();
    hipError_t e = hipMalloc(p, n);
    {
        std::lock_guard<std::mutex> lk(g_pool_mu);
        g_malloc_ms += bft_now_ms() - t_m0;
        g_malloc_calls++;
    }
    if (e != hipSuccess) {
        // out of memory with blocks parked in the cache: give them back and retry once
        std::vector<PoolBlock> all;
        {
            std::lock_guard<std::mutex> lk(g_pool_mu);
            all.swap(g_pool);
            g_pool_bytes = 0;
        }
        for (const PoolBlock& b : all) pool_free_block(b);
        (void)hipGetLastError();
        e = hipMalloc(p, n);
    }
    if (e != hipSuccess) return bft_fail(BFT_GPU_E_HIP, std::string("hipMalloc: ") + hipGetErrorString(e));
    *cap = n;
    return 0;
}

void bft_pool_release(void* p, size_t cap) {
    if (!p) return;
    PoolBlock b{p, cap, t_pool_device, t_pool_stream};
    bool keep = t_pool_device >= 0;
    if (keep) {
        std::lock_guard<std::mutex> lk(g_pool_mu);
        if (g_pool.size() < POOL_MAX_BLOCKS && g_pool_bytes + cap <= pool_max_bytes()) {
            g_pool.push_back(b);
            g_pool_bytes += cap;
        } else
            keep = false;
    }
    if (!keep) {
        const double t0 = bft_now_ms();
        (void)hipFree(p);
        std::lock_guard<std::mutex> lk(g_pool_mu);
        g_free_ms += bft_now_ms() - t0;
        g_free_calls++;
    }
}

void bft_pool_drop_stream(hipStream_t s) {
    // (the caller has synchronised s and destroys it next: its blocks stay in the cache -- the next handle's build of the same size finds them,
    // where a hipMalloc of a gigabyte block costs from a millisecond to 0.4 s depending on the box -- but must never be waited for on s again)
    std::lock_guard<std::mutex> lk(g_pool_mu);
    for (PoolBlock& b : g_pool)
        if (b.stream == s) b.stream = POOL_DRAINED;
}

extern "C" uint64_t bft_gpu_cache_release(void) {
    std::vector<PoolBlock> all;
    uint64_t bytes = 0;
    {
        std::lock_guard<std::mutex> lk(g_pool_mu);
        all.swap(g_pool);
        bytes = g_pool_bytes;
        g_pool_bytes = 0;
    }
    for (const PoolBlock& b : all) {
        if (b.stream != POOL_DRAINED) {  // (released under a live handle's stream: what was enqueued before the release may still read it)
            int cur = -1;
            (void)hipGetDevice(&cur);
            if (cur != b.device) (void)hipSetDevice(b.device);
            (void)hipStreamSynchronize(b.stream);
            if (cur != b.device && cur >= 0) (void)hipSetDevice(cur);
        }
        pool_free_block(b);
    }
    return bytes;
}

// ------------------------------------------------------------------------------------------------
// handle (struct bft_gpu: bft_handle.h)
// ------------------------------------------------------------------------------------------------
int bft_set_device(bft_gpu* h) {
    HIPCK(hipSetDevice(h->device));
    bft_pool_set_stream(h->device, h->stream);
    return 0;
}

#define BFT_MAX_EXT_STREAMS 8
int bft_note_foreign_stream(bft_gpu* h, hipStream_t s) {
    if (s == h->stream) return 0;
    bft_gpu::ExtEv* slot = nullptr;
    for (auto& e : h->ext)
        if (e.stream == s) slot = &e;
    if (!slot && h->ext.size() < BFT_MAX_EXT_STREAMS) {
        hipEvent_t ev = nullptr;
        HIPCK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        h->ext.push_back({s, ev, false});
        slot = &h->ext.back();
    }
    if (!slot) {  // more caller streams than slots: the oldest slot's work is drained and the slot moves on
        slot = &h->ext[0];
        if (slot->pending) HIPCK(hipEventSynchronize(slot->ev));
        slot->stream = s;
    }
    HIPCK(hipEventRecord(slot->ev, s));
    slot->pending = true;
    return 0;
}
int bft_wait_foreign_stream(bft_gpu* h) {
    for (auto& e : h->ext)
        if (e.pending) {
            HIPCK(hipEventSynchronize(e.ev));
            e.pending = false;
        }
    return 0;
}

// ------------------------------------------------------------------------------------------------
// C-ABI: lifecycle
// ------------------------------------------------------------------------------------------------
extern "C" const char* bft_gpu_last_error(void) { return g_err.c_str(); }
extern "C" const char* bft_gpu_version(void) { return "bft-mi355x 0.1 (gfx950)"; }

extern "C" int bft_gpu_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

extern "C" int bft_gpu_create_seeded(int k, int device, int r1, int r2, bft_gpu** out) {
    if (!out) return fail(BFT_GPU_E_ARG, "out is NULL");
    *out = nullptr;
    DeviceScope ds_;
    if (!bft_valid_k(k)) return fail(BFT_GPU_E_ARG, "Length k (for k-mers) must be in [9,126] (a multiple of 9 for reference-compatible indexes, src/main.c:61-63)");
    int ndev = 0;
    HIPCK(hipGetDeviceCount(&ndev));
    if (ndev <= 0) return fail(BFT_GPU_E_HIP, "no HIP device: this library has no CPU fallback");
    if (device < 0 || device >= ndev) return fail(BFT_GPU_E_ARG, "bad device index");
    bft_gpu* h = new bft_gpu();
    h->k = k;
    h->L = k / 9;
    h->W = bft_words_for_k(k);
    h->B = bft_bytes_for_k(k);
    h->device = device;
    h->r1 = r1 > 0 ? r1 : BFT_DEFAULT_R1;
    h->r2 = r2 > 0 ? r2 : BFT_DEFAULT_R2;
    if (hipSetDevice(device) != hipSuccess || hipStreamCreate(&h->stream) != hipSuccess) {
        delete h;
        return fail(BFT_GPU_E_HIP, "hipSetDevice/hipStreamCreate failed");
    }
    bft_pool_set_stream(device, h->stream);
    h->hashmod.resize(16384);
    bft_make_hashmod(h->r1, h->r2, h->hashmod.data());
    if (h->d_hashmod.alloc(16384 * 4) != 0 ||
        hipMemcpy(h->d_hashmod.p, h->hashmod.data(), 16384 * 4, hipMemcpyHostToDevice) != hipSuccess) {
        bft_gpu_free(h);
        return fail(BFT_GPU_E_HIP, "hash table upload failed");
    }
    memset(&h->im, 0, sizeof(h->im));
    *out = h;
    return BFT_GPU_OK;
}

extern "C" int bft_gpu_create(int k, int device, bft_gpu** out) { return bft_gpu_create_seeded(k, device, 0, 0, out); }

static void drain_events(bft_gpu* h) {
    for (auto& pr : h->pending_ev) {
        float ms = 0;
        if (hipEventSynchronize(pr.second) == hipSuccess && hipEventElapsedTime(&ms, pr.first, pr.second) == hipSuccess) {
            h->kernel_ms += ms;
            h->kernel_launches++;
        }
        h->free_ev.push_back(pr.first);  // back to the handle's pool
        h->free_ev.push_back(pr.second);
    }
    h->pending_ev.clear();
}

// Timed launches: a pair of pooled events around the kernel (no event is created on the launch path once the pool is warm).
int bft_timing_begin(bft_gpu* h, hipStream_t s, hipEvent_t* e0, hipEvent_t* e1) {
    *e0 = *e1 = nullptr;
    if (!h->timing) return 0;
    if (h->pending_ev.size() >= 4096) drain_events(h);
    for (hipEvent_t* e : {e0, e1}) {
        if (!h->free_ev.empty()) { *e = h->free_ev.back(); h->free_ev.pop_back(); }
        else HIPCK(hipEventCreate(e));
    }
    HIPCK(hipEventRecord(*e0, s));
    return 0;
}
int bft_timing_end(bft_gpu* h, hipStream_t s, hipEvent_t e0, hipEvent_t e1) {
    if (!e0) return 0;
    HIPCK(hipEventRecord(e1, s));
    h->pending_ev.push_back({e0, e1});
    return 0;
}

extern "C" void bft_gpu_free(bft_gpu* h) {
    if (!h) return;
    DeviceScope ds_;
    (void)hipSetDevice(h->device);
    bft_pool_set_stream(h->device, h->stream);
    drain_events(h);
    (void)bft_wait_foreign_stream(h);
    for (hipEvent_t e : h->free_ev) (void)hipEventDestroy(e);
    h->free_ev.clear();
    for (auto& e : h->ext) (void)hipEventDestroy(e.ev);
    h->ext.clear();
    const hipStream_t s = h->stream;
    if (s) (void)hipStreamSynchronize(s);
    if (h->stream2) { (void)hipStreamSynchronize(h->stream2); (void)hipStreamDestroy(h->stream2); h->stream2 = nullptr; }
    delete h;                      // its buffers go to the cache under this stream's tag ...
    bft_pool_drop_stream(s);       // ... which is replaced by "drained" here (bft_gpu_cache_release gives the cache back to the runtime)
    bft_pool_set_stream(-1, nullptr);
    if (s) (void)hipStreamDestroy(s);
}

extern "C" int bft_gpu_genome_name(bft_gpu* h, uint32_t id_genome, char* out, uint32_t cap) {
    if (!h || !out || cap == 0) return fail(BFT_GPU_E_ARG, "NULL argument");
    const std::string name = id_genome < h->genomes.size() ? h->genomes[id_genome] : "genome_" + std::to_string(id_genome);
    if (name.size() + 1 > cap) return fail(BFT_GPU_E_NOSPACE, "name buffer too small");
    memcpy(out, name.c_str(), name.size() + 1);
    return BFT_GPU_OK;
}

extern "C" int bft_gpu_add_genome(bft_gpu* h, const char* name, uint32_t* id_genome) {
    if (!h || !name) return fail(BFT_GPU_E_ARG, "NULL argument");
    if (h->marking) return fail(BFT_GPU_E_STATE, "add_genome: the graph is locked for vertex marking (bft_gpu_marks_end unlocks it)");
    h->genomes.push_back(name);
    if (id_genome) *id_genome = (uint32_t)h->genomes.size() - 1;
    return BFT_GPU_OK;
}

// ------------------------------------------------------------------------------------------------
// insertion log
// ------------------------------------------------------------------------------------------------
// (the log's format follows bft_run_plan.h, like the road the build takes with it)
static uint32_t log_comp_bits(const bft_gpu* h) { return bft_run_log_comp_bits(h->k, h->W, h->opt_comp_log != 0, !h->opt_no_composite); }
// a log of composites back into T-form k-mers and their ids (in place + the id array)
__global__ void k_log_decompose(uint64_t* __restrict__ log_k, uint64_t n, uint32_t cgb, uint32_t* __restrict__ log_g) {
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t c = log_k[i];
        log_g[i] = (uint32_t)(c & ((1ull << cgb) - 1ull));
        log_k[i] = c >> cgb;
    }
}
// composites -> k-mers + ids, for whatever cannot take composites (the id array is allocated here)
static int log_decompose(bft_gpu* h) {
    if (!h->log_comp) return 0;
    CK(bft_wait_foreign_stream(h));
    DevBuf ng;
    CK(ng.alloc(std::max<uint64_t>(h->log_cap, 1) * 4));
    if (h->log_n) {
        hipLaunchKernelGGL(k_log_decompose, dim3(bft_grid_for((h->log_n + 255) / 256)), dim3(256), 0, h->stream, h->log_k.as<uint64_t>(), h->log_n, h->log_gb, ng.as<uint32_t>());
        HIPCK(hipGetLastError());
    }
    HIPCK(hipStreamSynchronize(h->stream));
    h->log_g.swap(ng);
    h->log_comp = false;
    return 0;
}
int bft_log_reserve(bft_gpu* h, uint64_t need) {
    if (h->log_n == 0 && h->log_cap == 0) {  // an empty log: its format is decided here
        h->log_gb = log_comp_bits(h);
        h->log_comp = h->log_gb != 0;
    }
    if (need <= h->log_cap) return 0;
    uint64_t ncap = std::max<uint64_t>(need, h->log_cap * 2);
    ncap = std::max<uint64_t>(ncap, 1 << 16);
    // The log is about to move: batches still being packed into it on a caller's stream (bft_gpu_insert_kmers_dev_async) finish
    // first -- the copy below would miss their rows and the old block would go back to the cache with writes in flight.
    CK(bft_wait_foreign_stream(h));
    DevBuf nk, ng;
    CK(nk.alloc(ncap * h->W * 8));
    if (!h->log_comp) CK(ng.alloc(ncap * 4));
    if (h->log_n) {
        for (int w = 0; w < h->W; w++)
            HIPCK(hipMemcpyAsync(nk.as<uint64_t>() + (uint64_t)w * ncap, h->log_k.as<uint64_t>() + (uint64_t)w * h->log_cap,
                                 h->log_n * 8, hipMemcpyDeviceToDevice, h->stream));
        if (!h->log_comp) HIPCK(hipMemcpyAsync(ng.p, h->log_g.p, h->log_n * 4, hipMemcpyDeviceToDevice, h->stream));
    }
    // (also without a copy: a fresh block may come from the cache with work of this handle's stream still queued on it, and the
    // next writer may be a caller's stream, which is not ordered behind ours)
    HIPCK(hipStreamSynchronize(h->stream));
    h->log_k.swap(nk);
    h->log_g.swap(ng);
    h->log_cap = ncap;
    return 0;
}

int bft_log_prepare(bft_gpu* h, uint64_t n, uint32_t id_genome) {
    if (h->log_n && h->log_n + n > h->opt_flush_pairs) CK(bft_gpu_build(h));
    CK(bft_log_reserve(h, h->log_n + n));
    if (h->log_comp && !bft_run_log_holds_id(h->log_gb, id_genome)) CK(log_decompose(h));  // (an id the composites have no room for)
    return 0;
}
// n rows for id_genome were written behind the log's end
static void log_appended(bft_gpu* h, uint64_t n, uint32_t id_genome) {
    if (h->log_n > 0 && id_genome < h->log_last_gid) h->log_g_sorted = false;
    h->log_last_gid = id_genome;
    h->log_n += n;
    if (!h->lb_gid.empty() && h->lb_gid.back() == id_genome) h->lb_end.back() = h->log_n;
    else { h->lb_end.push_back(h->log_n); h->lb_gid.push_back(id_genome); }
    h->max_gid_seen = std::max(h->max_gid_seen, id_genome);
    h->any_insert = true;
}
int bft_log_commit(bft_gpu* h, uint64_t n, uint32_t id_genome, hipStream_t s) {
    if (s && s != h->stream) CK(bft_note_foreign_stream(h, s));
    log_appended(h, n, id_genome);
    return 0;
}

template <int W>
static int launch_pack(bft_gpu* h, const uint8_t* d_packed, uint64_t n, uint32_t gid, hipStream_t s) {
    const uint64_t nblk = (n + BFT_BLOCK - 1) / BFT_BLOCK;
    hipLaunchKernelGGL(k_pack_to_tform<W>, dim3(bft_grid_for(nblk)), dim3(BFT_BLOCK), 0, s, d_packed, n, h->B,
                       h->k, h->log_k.as<uint64_t>(), h->log_cap, h->log_n, h->log_g.as<uint32_t>(), gid, h->log_comp ? h->log_gb : 0u);
    HIPCK(hipGetLastError());
    return 0;
}

// insertKmers on a device-resident batch.  !ordered: on the handle's stream, synchronised before returning (the caller may
// reuse d_kmers at once).  ordered: stream-ordered on the caller's stream s (NULL = the null stream): nothing waits; the build waits for s.
// own_async: on the handle's stream, NOT synchronised (the caller keeps d_kmers alive until that stream has passed: the pinned ring).
static int insert_dev(bft_gpu* h, const void* d_kmers, uint64_t n, uint32_t id_genome, hipStream_t s, bool ordered, bool own_async = false) {
    if (!h || (!d_kmers && n)) return fail(BFT_GPU_E_ARG, "NULL argument");
    if (id_genome >= BFT_MAX_GENOME_ID) return fail(BFT_GPU_E_ARG, "id_genome out of range (must be below 2^24)");
    if (h->marking) return fail(BFT_GPU_E_STATE, "insert: the graph is locked for vertex marking (bft_gpu_marks_end unlocks it)");
    if (n == 0) return BFT_GPU_OK;
    ENTER(h);
    // No bound on the pairs an index holds (the reference has none, src/insertNode.c:18-36): a batch beyond what one sort takes is
    // inserted in pieces, and the log is merged into the index before it reaches "flush_pairs".
    if (n > h->opt_flush_pairs) {
        const uint64_t half = n / 2;
        CK(insert_dev(h, d_kmers, half, id_genome, s, ordered, own_async));
        return insert_dev(h, (const uint8_t*)d_kmers + half * (uint64_t)h->B, n - half, id_genome, s, ordered, own_async);
    }
    CK(bft_log_prepare(h, n, id_genome));
    const hipStream_t run = ordered ? s : h->stream;
    const uint8_t* p = (const uint8_t*)d_kmers;
    switch (h->W) {
    case 1: CK(launch_pack<1>(h, p, n, id_genome, run)); break;
    case 2: CK(launch_pack<2>(h, p, n, id_genome, run)); break;
    case 3: CK(launch_pack<3>(h, p, n, id_genome, run)); break;
    default: CK(launch_pack<4>(h, p, n, id_genome, run)); break;
    }
    if (ordered) CK(bft_note_foreign_stream(h, s));
    else if (!own_async) HIPCK(hipStreamSynchronize(h->stream));
    log_appended(h, n, id_genome);
    return BFT_GPU_OK;
}
extern "C" int bft_gpu_insert_kmers_dev(bft_gpu* h, const void* d_kmers, uint64_t n, uint32_t id_genome) { return insert_dev(h, d_kmers, n, id_genome, nullptr, false); }
extern "C" int bft_gpu_insert_kmers_dev_async(bft_gpu* h, const void* d_kmers, uint64_t n, uint32_t id_genome, void* hip_stream) {
    return insert_dev(h, d_kmers, n, id_genome, (hipStream_t)hip_stream, true);
}

extern "C" int bft_gpu_insert_kmers(bft_gpu* h, const uint8_t* kmers, uint64_t n, uint32_t id_genome) {
    if (!h || (!kmers && n)) return fail(BFT_GPU_E_ARG, "NULL argument");
    if (id_genome >= BFT_MAX_GENOME_ID) return fail(BFT_GPU_E_ARG, "id_genome out of range (must be below 2^24)");
    if (h->marking) return fail(BFT_GPU_E_STATE, "insert: the graph is locked for vertex marking (bft_gpu_marks_end unlocks it)");
    if (n == 0) return BFT_GPU_OK;
    ENTER(h);
    if (n * (uint64_t)h->B <= bft_gpu::RING_SLOT) {  // through the pinned ring (see struct bft_gpu)
        if (!h->ring && hipHostMalloc((void**)&h->ring, bft_gpu::RING_SLOT * bft_gpu::RING_SLOTS, hipHostMallocMapped) != hipSuccess) {
            h->ring = nullptr;
            (void)hipGetLastError();
        }
        if (h->ring) {
            const int slot = h->ring_next;
            if (!h->ring_ev[slot]) HIPCK(hipEventCreateWithFlags(&h->ring_ev[slot], hipEventDisableTiming));
            if (h->ring_busy[slot]) HIPCK(hipEventSynchronize(h->ring_ev[slot]));
            uint8_t* dst = h->ring + (size_t)slot * bft_gpu::RING_SLOT;
            memcpy(dst, kmers, n * (uint64_t)h->B);
            CK(insert_dev(h, dst, n, id_genome, nullptr, false, true));
            HIPCK(hipEventRecord(h->ring_ev[slot], h->stream));
            h->ring_busy[slot] = true;
            h->ring_next = (slot + 1) % bft_gpu::RING_SLOTS;
            return BFT_GPU_OK;
        }
    }
    const uint64_t chunk = 1ull << 26;
    DevBuf tmp;
    CK(tmp.alloc(std::min(n, chunk) * h->B));
    for (uint64_t a = 0; a < n; a += chunk) {
        const uint64_t m = std::min(chunk, n - a);
        HIPCK(hipMemcpy(tmp.p, kmers + a * h->B, m * h->B, hipMemcpyHostToDevice));
        CK(bft_gpu_insert_kmers_dev(h, tmp.p, m, id_genome));
    }
    return BFT_GPU_OK;
}

// ------------------------------------------------------------------------------------------------
// bulk build
// ------------------------------------------------------------------------------------------------
StageScope::StageScope(bft_gpu* hh, hipStream_t s) : h(hh) {
    t_stages_on = h->opt_build_stages;
    t_stage_marks.clear();
    if (t_stages_on) bft_stage("start", 0, s ? s : h->stream);
}
StageScope::~StageScope() {
    if (!t_stages_on) return;
    t_stages_on = false;
    h->stages.clear();
    (void)hipStreamSynchronize(h->stream);
    if (h->stream2) (void)hipStreamSynchronize(h->stream2);
    for (size_t i = 0; i < t_stage_marks.size(); i++) {
        float ms = 0;
        // a mark on the second stream ("+name": work that runs beside the main chain) is timed from the build's start
        const bool side = !t_stage_marks[i].name.empty() && t_stage_marks[i].name[0] == '+';
        size_t prev = 0;
        if (!side) for (size_t j = i; j-- > 0;) if (t_stage_marks[j].name[0] != '+') { prev = j; break; }
        if (i > 0 && hipEventSynchronize(t_stage_marks[i].ev) == hipSuccess &&
            hipEventElapsedTime(&ms, t_stage_marks[prev].ev, t_stage_marks[i].ev) == hipSuccess)
            h->stages.push_back({t_stage_marks[i].name, (double)ms, t_stage_marks[i].bytes});
        (void)hipGetLastError();
    }
    for (auto& m : t_stage_marks) t_stage_pool.push_back(m.ev);
    t_stage_marks.clear();
}

int bft_commit_image(bft_gpu* h, BftRunOut& img, uint64_t np, double t0, double t1, BftBuildSide* side) {
    // (a caller that neither interned nor prepared the k-mer hash: nothing prepared, nothing pending)
    if (!side) { BftBuildSide none; return bft_commit_image(h, img, np, t0, t1, &none); }
    KhFill& khf = side->khf;
    BftInternTail& tail = side->tail;
    const uint64_t nk = img.n;
    struct KhStart {  // (from here on the table, the colour set per row and the number of colour sets are final)
        bft_gpu* h; const uint64_t* tk; const uint32_t* tcol; uint64_t nk, n_sets; KhFill* f;
        static void run(void* c, hipStream_t s) { KhStart* k = (KhStart*)c; bft_kh_start(k->h, k->tk, k->tcol, k->nk, k->n_sets, *k->f, s, nullptr); }
    } khs{h, img.tk.as<uint64_t>(), img.tcol.as<uint32_t>(), nk, img.n_sets, &khf};
    // (started HERE instead -- beside the root's table passes -- the sort-based table build was measured too: 17.2-18.4 ms against 17.0)
    // (and earlier still -- behind the root's prefix scans, or before them: 15.7 ms each way, round 5: the build is bound by the device's total work,
    // not by either stream's chain)
    const BftAssembleHook hook{img.tk.p ? &KhStart::run : nullptr, &khs};
    const double t2 = bft_now_ms();

    // 5. containers, level by level, on the GPU
    if (!img.tk.p) CK(img.tk.alloc(8));
    BftDeviceIndex idx;
    CK(bft_assemble_gpu(img.tk.as<uint64_t>(), nk, h->k, h->d_hashmod.as<uint32_t>(), h->stream, idx, &hook));
    bft_trace_mark("containers assembled");
    bft_stage("containers: concatenation", 0, h->stream);
    double t3 = bft_now_ms();
    DevBuf n_ccx, n_f18buf, n_fentbuf;
    uint64_t n_f18 = 0, n_fent = 0;
    CK(bft_flatten_gpu(idx.ccs.as<BftCC>(), idx.n_ccs, idx.f2w.as<uint64_t>(), idx.clus.as<uint64_t>(), idx.child.as<uint64_t>(), h->opt_flat_min, h->stream,
                       n_ccx, n_f18buf, n_fentbuf, n_f18, n_fent));
    bft_trace_mark("flat forms");
    bft_stage("flat forms of the big CCs", (double)(n_f18 + n_fent) * 8, h->stream);
    bool kh_redo = false;
    {   // the interning's deferred tail: done long ago; two lists with one signature (never seen outside the test hook) -> the exact interning
        uint32_t collisions = 0;
        CK(tail.wait(&collisions));
        if (collisions) {
            double ms_ = 0;
            (void)bft_kh_finish(h, khf, &ms_);  // (the table under construction holds the wrong colour sets, and reads the arrays replaced below)
            khf.buf.release();
            kh_redo = true;
            CK(bft_intern_colors_gpu(side->lists.seg_off.as<uint32_t>(), side->lists.ids.as<uint32_t>(), side->lists.nk, side->lists.np, h->stream, img.tcol, img.cs_off, img.cs_ids, img.n_sets, img.n_ids, 0, nullptr, true));
        }
        side->lists.seg_off.release();
        side->lists.ids.release();
    }
    const uint32_t new_cs_w = bft_id_width(h->max_gid_seen);
    DevBuf n_cs_ids_w;
    bool narrowed_here = false;
    if (!kh_redo && tail.narrow.p && tail.narrow_w == new_cs_w) {  // (done by the interning's tail on the side stream)
        n_cs_ids_w.swap(tail.narrow);
        img.cs_ids.release();
    } else {
        CK(bft_narrow_ids(img.cs_ids, img.n_ids, new_cs_w, h->stream, n_cs_ids_w));
        narrowed_here = new_cs_w < 4;
    }
    CK(bft_wait_foreign_stream(h));  // queries a caller still has in flight on its own stream read the arrays released below
    bft_trace_mark("ids narrowed, foreign stream waited");
    bft_stage("dictionary ids narrowed", narrowed_here ? (double)img.n_ids * (4 + new_cs_w) : 0.0, h->stream);
    double kh_ms = 0;
    const bool kh_ok = !kh_redo && bft_kh_finish(h, khf, &kh_ms);
    bft_trace_mark("k-mer hash fill waited");
    bft_stage("wait for the k-mer hash build", 0, h->stream);
    if (h->inject_build_failure) {
        h->inject_build_failure = false;
        return fail(BFT_GPU_E_LIMIT, "injected build failure (test hook)");
    }

    // ---- commit: nothing above touched the handle; from here on nothing can fail before the image is whole ----
    {   // the stored arrays (bft_stored.h), in their order: the containers of the assembly, the table and the dictionary of img, the narrowed ids
        DevBuf* const fresh[BFT_N_STORED] = {&idx.nodes, &idx.bfT, &idx.ccs, &idx.f2w, &idx.clus, &idx.child, &idx.uck, &idx.ucrow,
                                             &img.tk, &img.tcol, &img.cs_off, &n_cs_ids_w};
        const BftStoredRows st = bft_stored_rows(h);
        for (int i = 0; i < BFT_N_STORED; i++) st.row[i].buf->swap(*fresh[i]);
    }
    h->cs_w = new_cs_w;
    h->n_sets = img.n_sets;
    h->n_ids = img.n_ids;
    h->cs_on_host = false;
    h->cs_off.clear();
    h->cs_ids.clear();
    h->d_ccx.swap(n_ccx);
    h->d_f18.swap(n_f18buf);
    h->d_fent.swap(n_fentbuf);
    h->n_f18 = n_f18;
    h->n_fent = n_fent;
    h->log_k.release();
    h->log_g.release();
    h->log_cap = 0;
    h->table_dropped = false;
    h->n_pairs = np;
    h->log_n = 0;
    h->lb_end.clear();
    h->lb_gid.clear();
    h->log_comp = false;
    h->log_g_sorted = true;
    h->n_kmers = nk;
    bft_set_idx_sizes(h, idx, nk);
    h->root_ncc = (uint32_t)idx.root_ncc;
    bft_point_image(h, std::max<uint32_t>((uint32_t)h->genomes.size(), h->any_insert ? h->max_gid_seen + 1 : 0));
    BftImage& im = h->im;

    uint64_t* I = h->info;
    I[0] = h->k;
    I[1] = nk;
    I[2] = idx.n_nodes;
    I[3] = idx.n_ccs;
    I[4] = idx.n_uc;
    I[5] = idx.n_child_nodes;
    I[6] = idx.n_prefixes;
    I[7] = idx.n_ccs_s4;
    I[8] = idx.max_ccs_per_node;
    I[9] = np;
    I[10] = img.n_sets;
    I[11] = im.nb_genomes;  // (I[12], the image's bytes: bft_rederive, below)
    I[13] = idx.root_ncc;
    I[14] = idx.root_uc;
    h->build_ms[0] = t1 - t0;
    h->build_ms[1] = t2 - t1;
    h->build_ms[2] = t3 - t2;
    h->build_ms[3] = (double)h->front_redone;
    h->built = true;
    h->claims.ensure();
    bft_trace_mark("committed (buffers released)");
    const BftCommitKh kh{kh_ok ? &khf : nullptr, kh_ms, kh_redo};
    (void)bft_rederive(h, BFT_DERIVE_ALL & ~BFT_DERIVE_FLAT, &kh);  // (cannot fail in a commit; the flat forms were built aside above)
    bft_trace_mark("launch shape; done");
    bft_stage("node hash, launch shape, compact table", 0, h->stream);
    if (bft_trace_on()) {
        std::lock_guard<std::mutex> lk(g_pool_mu);
        fprintf(stderr, "[bft_gpu build] cache of released blocks: %zu blocks, %.1f MB; this process so far: %llu hipMalloc (%.2f ms), %llu hipFree on release (%.2f ms)\n", g_pool.size(),
                g_pool_bytes / 1048576.0, (unsigned long long)g_malloc_calls, g_malloc_ms, (unsigned long long)g_free_calls, g_free_ms);
    }
    h->build_ms[4] = bft_now_ms() - t3;
    return BFT_GPU_OK;
}

extern "C" int bft_gpu_build(bft_gpu* h) {
    if (!h) return fail(BFT_GPU_E_ARG, "NULL handle");
    if (h->marking) return fail(BFT_GPU_E_STATE, "build: the graph is locked for vertex marking (bft_gpu_marks_end unlocks it)");
    ENTER(h);
    if (h->built && h->log_n == 0) return BFT_GPU_OK;
    CK(bft_wait_foreign_stream(h));  // batches still being packed into the log on a caller's stream (bft_gpu_insert_kmers_dev_async)
    if (h->log_comp && !bft_run_log_stays_composite(h->log_g_sorted, !h->opt_no_composite)) CK(log_decompose(h));  // (only the composite path below takes a log of composites)
    if (h->built) CK(bft_ensure_table(h));  // ("compact_table": the merge reads the index's sorted table)
    const double t0 = bft_now_ms();
    bft_trace_mark(nullptr);
    StageScope stage_scope(h);

    // 1-3. the run: what was inserted since the last build, sorted and de-duplicated (bft_run.hip)
    BftRunOut img;      // built aside, like every array of the new image
    BftBuildSide side;  // (declared behind img: the k-mer hash fill and the interning's tail are waited for before the arrays they read go)
    BftPairRun& run = side.lists;
    CK(bft_make_run(h, run));
    bft_trace_mark("sort + dedupe done");
    bft_stage("sort + dedupe (rest)", 0, h->stream);
    const double t1 = bft_now_ms();

    // 4. colour sets: signature sort + exact run detection + verification, all on the GPU
    img.tk.swap(run.tk);
    img.n = run.nk;
    if (img.n == 0) {
        CK(run.seg_off.alloc_zero(4, h->stream));
        CK(run.ids.alloc(4));
    }
    // (the second stream, made here: the helper thread below and the interning's tail both use it)
    if (img.n > 0) (void)bft_ensure_stream2(h);
    const bool merging = h->built && h->n_kmers > 0 && img.n > 0;
    // (the table's sort by home line started HERE, beside the colour-set interning, was measured: the interning's persistent grids and the
    // sort starve each other -- 4.1 -> 10.5 ms for the interning, 20 -> 25.8 ms for the build; it starts behind the assembly's table passes)
    if (img.n > 0 && !merging) bft_kh_prepare_async(h, img.n, img.n, side.khf);  // (a merge changes the k-mers: kh_start does everything then)
    // (the interning's tail -- dictionary copy + verification of every list -- goes to the second stream, idle until the k-mer hash build starts
    // behind the first level's table passes; its verdict is collected before the commit.  A merge reads the dictionary at once: not deferred.)
    side.tail.side = merging ? nullptr : h->stream2;
    side.tail.narrow_w = bft_id_width(h->max_gid_seen);  // (the tail also leaves the dictionary in the width the image keeps)
    CK(bft_intern_colors_gpu(run.seg_off.as<uint32_t>(), run.ids.as<uint32_t>(), run.nk, run.np, h->stream, img.tcol, img.cs_off, img.cs_ids, img.n_sets, img.n_ids, 0, &side.tail));
    bft_trace_mark("colour sets interned");
    bft_stage("colour sets (rest)", 0, h->stream);
    if (!side.tail.pending) {
        run.seg_off.release();
        run.ids.release();
    }
    // 4b. an index exists already: the run is merged into it (bft_merge.hip) -- k-mers by position, colour sets by union
    uint64_t total_pairs = run.np;
    if (merging) {
        DevBuf wide;
        const uint32_t* old_ids = nullptr;
        CK(bft_dict_ids32(h, 0u, h->stream, nullptr, wide, &old_ids));  // (the resident dictionary as u32: a transient of the merge)
        const BftRun old_run{h->d_tk.as<uint64_t>(), h->d_tcol.as<uint32_t>(), h->n_kmers, h->d_cs_off.as<uint32_t>(), old_ids, h->n_sets};
        const BftRun new_run{img.tk.as<uint64_t>(), img.tcol.as<uint32_t>(), img.n, img.cs_off.as<uint32_t>(), img.cs_ids.as<uint32_t>(), img.n_sets};
        BftRunOut mo;
        CK(bft_merge_runs(h->W, old_run, new_run, h->stream, mo));
        img.swap(mo);
        CK(bft_count_pairs(img.tcol.as<uint32_t>(), img.n, img.cs_off.as<uint32_t>(), h->stream, &total_pairs));
    }
    bft_trace_mark("merge / bookkeeping");
    bft_stage("merge into the index", 0, h->stream);
    return bft_commit_image(h, img, total_pairs, t0, t1, &side);
}

int bft_ensure_built(bft_gpu* h, bool need_table) {
    if (!h->built || h->log_n) CK(bft_gpu_build(h));
    if (need_table) CK(bft_ensure_table(h));
    return 0;
}

// Test hook (tests/test_colour_cases_host.py, tests/test_gpu_colour_retrieval.py): the tile and the division constants the colour-row kernels
// are launched with for rows of `rowbytes` bytes (bft_color_plan.h).  form 0: the dword kernels (k_color_rows_bm<false>, <true>), 1: the 16-byte
// kernel (k_color_rows_bm16), 2: the row kernel of the k-mer hash (k_color_rows_kh); 1 and 2 serve rows of 16 bytes and up.  out: tile_rows, div_m,
// div_l.  No handle, no HIP call.
extern "C" int bft_gpu_debug_color_rows_plan(uint32_t rowbytes, int form, uint32_t out[3]) {
    if (!out) return fail(BFT_GPU_E_ARG, "NULL argument");
    if (form < BFT_ROWS_FORM_DWORD || form > BFT_ROWS_FORM_KH) return fail(BFT_GPU_E_ARG, "form must be 0, 1 or 2");
    if (rowbytes == 0 || (form != BFT_ROWS_FORM_DWORD && rowbytes < 16)) return fail(BFT_GPU_E_ARG, "no such kernel for rows of this width");
    const BftColorRowsPlan plan = bft_color_rows_plan(rowbytes, form);
    out[0] = plan.tile_rows;
    out[1] = plan.div_m;
    out[2] = plan.div_l;
    return BFT_GPU_OK;
}

// An option that changes what the image's derived tables hold: they are re-derived at once where there is an image (else by the first build)
static int rederive_built(bft_gpu* h, unsigned steps) {
    if (!h->built) return 0;
    ENTER(h);
    return bft_rederive(h, steps);
}

extern "C" int bft_gpu_set_option(bft_gpu* h, const char* name, int64_t value) {
    if (!h || !name) return fail(BFT_GPU_E_ARG, "NULL argument");
    const std::string nm(name);
    if (nm == "query_wgs_per_cu") {
        if (value < 0 || value > 3) return fail(BFT_GPU_E_ARG, "query_wgs_per_cu must be 0 (automatic), 1, 2 or 3");
        h->opt_wgs_per_cu = (int)value;
    } else if (nm == "build_composite") {
        if (value != 0 && value != 1) return fail(BFT_GPU_E_ARG, "build_composite must be 0 or 1");
        h->opt_no_composite = value == 0;
    } else if (nm == "build_msd") {
        if (value < 0 || value > 2) return fail(BFT_GPU_E_ARG, "build_msd must be 0, 1 or 2");
        h->opt_msd = (int)value;
    } else if (nm == "sort_ballots") {  // how the library's radix sort ranks the keys of a wavefront (bft_sort.h); process-wide
        if (value != 0 && value != 1) return fail(BFT_GPU_E_ARG, "sort_ballots must be 0 (LDS atomics if the device serves them in lane order: checked once) or 1 (wavefront ballots)");
        bft_rs::g_bft_rs_rank_mode = value ? 1 : -1;
    } else if (nm == "reserve_pairs") {
        // room for this many not-yet-built (k-mer, genome) pairs in the insertion log, so that a long series of insertKmers
        // batches never re-allocates it (a caller usually knows the total: line 2 of a kmers_comp file, README.md:166-170)
        if (value < 0 || (uint64_t)value > h->opt_flush_pairs) return fail(BFT_GPU_E_ARG, "reserve_pairs must be in [0, flush_pairs]");
        ENTER(h);
        CK(bft_log_reserve(h, (uint64_t)value));
    } else if (nm == "ingest_chunk_chars") {  // characters per staged chunk of bft_gpu_insert_sequences' stream path (default 2^26; a test hook below that)
        if (value < (int64_t)BFT_ING_CHUNK_MIN || value > (1ll << 30)) return fail(BFT_GPU_E_ARG, "ingest_chunk_chars must be in [1024, 2^30]");
        h->opt_ingest_chunk = (uint64_t)value;
    } else if (nm == "flush_pairs") {  // the insertion log is merged into the index before it holds this many pairs (default 2^30; a test hook below that)
        if (value < 1024 || value > (1ll << 30)) return fail(BFT_GPU_E_ARG, "flush_pairs must be in [1024, 2^30]");
        h->opt_flush_pairs = (uint64_t)value;
    } else if (nm == "query_probe") {
        if (value != 0 && value != 4 && value != 8) return fail(BFT_GPU_E_ARG, "query_probe must be 0 (automatic), 4 or 8");
        h->opt_probe = (int)value;
        h->im.probe_big = bft_probe_mode(h->opt_probe ? h->opt_probe : h->tuned_probe);
    } else if (nm == "node_hash") {  // 1 (default): levels below the root through the node prefix hash; 0: through the containers
        if (value < 0 || value > 2) return fail(BFT_GPU_E_ARG, "node_hash must be 0, 1 or 2");
        h->opt_node_hash = (int)value;
        CK(rederive_built(h, BFT_DERIVE_NPH));
    } else if (nm == "kmer_hash" || nm == "kmer_hash_load") {  // the k-mer hash: on / off, and the occupancy of its home lines in per cent
        if (nm == "kmer_hash_load") {
            if (value < 10 || value > 80) return fail(BFT_GPU_E_ARG, "kmer_hash_load must be in [10, 80] (per cent)");
            h->opt_kh_load = (uint32_t)value;
        } else
            h->opt_kmer_hash = value != 0;
        CK(rederive_built(h, BFT_DERIVE_KH | BFT_DERIVE_WALK | BFT_DERIVE_NPH));  // (the tuned launch shape stays)
    } else if (nm == "walk_hash") {  // 1: presence / colour queries through the container walk, plain root groups looked up in their regions of the k-mer hash
        h->opt_walk_hash = value != 0;
        CK(rederive_built(h, BFT_DERIVE_NPH));
    } else if (nm == "compact_table") {  // 1: the sorted k-mer table and the colour set per k-mer do not stay resident beside the k-mer hash (ensure_table)
        h->opt_compact = value != 0;
        if (h->built) {
            ENTER(h);
            CK(bft_wait_foreign_stream(h));
            HIPCK(hipStreamSynchronize(h->stream));
            if (h->opt_compact) bft_drop_table(h);
            else CK(bft_ensure_table(h));
        }
    } else if (nm == "root_direct") {  // 2 (default): root level through the derived range + direct tables; 1: direct table only; 0: containers
        if (value < 0 || value > 3) return fail(BFT_GPU_E_ARG, "root_direct must be 0, 1, 2 or 3");
        h->opt_root_direct = (int)value;
        CK(rederive_built(h, BFT_DERIVE_ROOT | BFT_DERIVE_WALK | BFT_DERIVE_SHAPE));  // (the node prefix hash does not depend on the root tables)
    } else if (nm == "root_quartiles") {  // 1 (default): plain root groups are searched quarter by quarter (BFT_RQ_*)
        h->opt_root_quartiles = value != 0;
        CK(rederive_built(h, BFT_DERIVE_ROOT | BFT_DERIVE_WALK | BFT_DERIVE_SHAPE));
    } else if (nm == "tune") {  // measure the launch shape of the container walk on the current image (synchronises)
        if (value != 0 && h->built) {
            ENTER(h);
            CK(bft_wait_foreign_stream(h));
            HIPCK(hipStreamSynchronize(h->stream));
            CK(bft_ensure_table(h));
            CK(bft_tune_residency(h));
        }
    } else if (nm == "query_dynamic") {  // 0: the k-mer hash kernels split their batch by workgroup number (what they did before the claims)
        h->opt_query_dynamic = value != 0;
    } else if (nm == "query_dynamic_min") {
        h->opt_query_dynamic_min = value;
    } else if (nm == "query_chunk") {
        if (value < 1 || value > 64) return fail(BFT_GPU_E_ARG, "query_chunk must be in [1,64]");
        h->opt_query_chunk = (uint32_t)value;
    } else if (nm == "query_grid_mult") {
        if (value < 1 || value > 64) return fail(BFT_GPU_E_ARG, "query_grid_mult must be in [1,64]");
        h->opt_grid_mult = (int)value;
#if defined(BFT_PERF_PROBE)
    } else if (nm == "debug_stop") {  // libbft_gpu_probe.so only (make probe): truncates the walk, results are wrong
        h->im.debug_stop = (uint32_t)value;
#endif
    } else if (nm == "test_front_rank_mode") {  // test hook (tests/test_gpu_build.py): how the root-prefix buckets rank their digits, see k_bucket_sort
        if (value > 2) return fail(BFT_GPU_E_ARG, "test_front_rank_mode must be 0, 1 or 2");
        bft_test_front_rank_mode((int)value);
    } else if (nm == "test_front_wave_cap") {  // test hook (tests/test_gpu_front_edges.py): the one-word buckets a wavefront sorts, see bft_front_wave_cap
        if (value != 0 && value != 512 && value != 1024) return fail(BFT_GPU_E_ARG, "test_front_wave_cap must be 0, 512 or 1024");
        bft_test_front_wave_cap((uint32_t)value);
    } else if (nm == "test_weak_signature") {  // test hook (tests/test_gpu_build.py): colour-set signatures that collide, see bft_intern_colors_gpu
        if (value < 0 || value > 2) return fail(BFT_GPU_E_ARG, "test_weak_signature must be 0, 1 or 2");  // (2: the exact pass's second key is the length too)
        bft_test_weak_signature((int)value);
    } else if (nm == "inject_build_failure") {  // test hook (tests/test_gpu_build.py): exercises the all-or-nothing build
        h->inject_build_failure = value != 0;
    } else if (nm == "timing") {
        h->timing = value != 0;
    } else if (nm == "test_stale_claims") {  // test hook (tests/test_gpu_parity.py): every claim counter as a launch that never finished can leave it --
        // anywhere up to the end of the range it was given, i.e. the next launch's base (1: one below it, 2: exactly there, 3: where it started)
        if (value < 1 || value > 3) return fail(BFT_GPU_E_ARG, "test_stale_claims must be 1, 2 or 3");
        ENTER(h);
        CK(h->claims.stale((int)value));
    } else if (nm == "test_walk_grid") {  // test hook (tests/test_gpu_walk_edges.py): the container walk's launches (k_query*, k_query6h, k_branching*) use
        // at most this many workgroups, so that a batch of test size gives every wavefront several chunks (0: no cap); the claims are sized as ever
        if (value < 0 || value > 65535) return fail(BFT_GPU_E_ARG, "test_walk_grid must be in [0,65535]");
        h->opt_test_walk_grid = (uint32_t)value;
    } else if (nm == "test_no_cs_bitmaps") {  // test hook (tests/test_gpu_setops.py): the bitmap form of the dictionary is not derived (what happens by itself
        // where it would pass 4 GiB); one that exists is released, so the id lists serve the colour rows and the set operations from here on
        ENTER(h);
        CK(bft_wait_foreign_stream(h));
        HIPCK(hipStreamSynchronize(h->stream));
        h->opt_no_cs_bitmaps = value != 0;
        h->d_cs_bm.release();
        h->has_cs_bm = false;
        h->cs_bm_tried = false;
    } else if (nm == "composite_log") {  // 1 (default): one-word keys with room for an id are logged as composites; 0: always k-mers + ids (test hook: same image)
        if (h->log_n) return fail(BFT_GPU_E_STATE, "composite_log: the insertion log is not empty");
        h->opt_comp_log = value != 0;
        if (h->log_cap) { h->log_k.release(); h->log_g.release(); h->log_cap = 0; }  // (a reserved, empty log: its format is decided again)
    } else if (nm == "build_stages") {
        h->opt_build_stages = value != 0;
    } else if (nm == "merge_place") {  // bft_gpu_merge(h, other, ...): 1 = co-ranked placement, 0 = the search of an insertion build (same image)
        if (value != 0 && value != 1) return fail(BFT_GPU_E_ARG, "merge_place must be 0 or 1");
        h->opt_merge_place = (int)value;
    } else if (nm == "test_genome_matrix_road") {  // test hook (tests/test_gpu_genome_matrix.py): the road of bft_gpu_genome_matrix*: 0 = cost model, 1 = sparse, 2 = dense
        if (value < 0 || value > 2) return fail(BFT_GPU_E_ARG, "test_genome_matrix_road must be 0, 1 or 2");
        h->opt_gm_road = (int)value;
    } else if (nm == "flat_min") {
        if (value < 1 || value > 65536) return fail(BFT_GPU_E_ARG, "flat_min must be in [1,65536]");
        h->opt_flat_min = (uint32_t)value;
        CK(rederive_built(h, BFT_DERIVE_ALL));  // the flat arrays of the current image, and everything derived behind them
    } else
        return fail(BFT_GPU_E_ARG, "unknown option");
    return BFT_GPU_OK;
}

extern "C" int bft_gpu_info(bft_gpu* h, uint64_t* out, int n_out) {
    if (!h || !out) return fail(BFT_GPU_E_ARG, "NULL argument");
    h->info[0] = h->k;
    h->info[15] = h->log_n;
    for (int i = 0; i < n_out && i < 16; i++) out[i] = h->info[i];
    return BFT_GPU_OK;
}

extern "C" int bft_gpu_footprint(bft_gpu* h, uint64_t* out, int n_out) {
    if (!h || !out) return fail(BFT_GPU_E_ARG, "NULL argument");
    const BftStoredRows st = bft_stored_rows(h);
    const BftDerivedRows dv = bft_derived_rows(h);
    // table, colour set per k-mer, dictionary, containers; flat forms, root tables, node prefix hash, k-mer hash, bitmap dictionary; the rest
    const uint64_t v[] = {bft_rows_resident(st.row, BFT_S_TK, BFT_S_TCOL), bft_rows_resident(st.row, BFT_S_TCOL, BFT_S_CS_OFF), bft_rows_resident(st.row, BFT_S_CS_OFF, BFT_N_STORED),
                          bft_rows_resident(st.row, 0, BFT_S_TK), bft_rows_resident(dv.row, BFT_D_CCX, BFT_D_RDIR), bft_rows_resident(dv.row, BFT_D_RDIR, BFT_D_NPH),
                          bft_rows_resident(dv.row, BFT_D_NPH, BFT_D_KH), bft_rows_resident(dv.row, BFT_D_KH, BFT_D_CS_BM), bft_rows_resident(dv.row, BFT_D_CS_BM, BFT_N_DERIVED),
                          h->d_hashmod.bytes, 0ull, h->log_k.bytes + h->log_g.bytes};
    for (int i = 0; i < n_out && i < (int)(sizeof(v) / sizeof(v[0])); i++) out[i] = v[i];
    return BFT_GPU_OK;
}

extern "C" int bft_gpu_kernel_time(bft_gpu* h, double* ms, uint64_t* launches, int reset) {
    if (!h) return fail(BFT_GPU_E_ARG, "NULL handle");
    ENTER(h);
    drain_events(h);
    h->timing = true;  // from the first call on, query launches are bracketed by (pooled) events
    if (ms) *ms = h->kernel_ms;
    if (launches) *launches = h->kernel_launches;
    if (reset) {
        h->kernel_ms = 0;
        h->kernel_launches = 0;
    }
    return BFT_GPU_OK;
}

extern "C" int bft_gpu_build_time(bft_gpu* h, double* ms, int n_out) {
    if (!h || !ms) return fail(BFT_GPU_E_ARG, "NULL argument");
    const double v[25] = {h->build_ms[0], h->build_ms[1], h->build_ms[2], h->build_ms[3], h->build_ms[4], (double)bft_query_residency(h), h->tune_ms[0], h->tune_ms[1],
                          h->im.probe_big ? 8.0 : 4.0, (double)h->kh_lines, h->kh_ms, (double)h->msd_max_bucket, (double)bft_test_exact_passes(), g_malloc_ms,
                          (double)(h->im.rdir ? (h->im.rstart ? 2 : 1) : 0), h->rstart_tune_ms[0], h->rstart_tune_ms[1],
                          (double)h->nph_inserted, (double)h->nph_dropped, h->tune_ms[2], (double)h->claims.static_launches,
                          (double)h->im.kh.S, (double)h->im.kh.db, (double)h->im.kh.maxd, (double)h->kh_ovf_n};
    for (int i = 0; i < n_out && i < 25; i++) ms[i] = v[i];
    return BFT_GPU_OK;
}

extern "C" int bft_gpu_build_stages(bft_gpu* h, char* names, uint32_t names_cap, double* ms, double* bytes, int cap, int* n_out) {
    if (!h || !n_out) return fail(BFT_GPU_E_ARG, "NULL argument");
    *n_out = (int)h->stages.size();
    std::string all;
    for (const auto& st : h->stages) { all += st.name; all += '\n'; }
    if (names) {
        if (all.size() + 1 > names_cap) return fail(BFT_GPU_E_NOSPACE, "names buffer too small");
        memcpy(names, all.c_str(), all.size() + 1);
    }
    for (int i = 0; i < cap && i < (int)h->stages.size(); i++) {
        if (ms) ms[i] = h->stages[i].ms;
        if (bytes) bytes[i] = h->stages[i].bytes;
    }
    return BFT_GPU_OK;
}

bool bft_stream_capturing(hipStream_t s) {
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &st) != hipSuccess) { (void)hipGetLastError(); return false; }
    return st != hipStreamCaptureStatusNone;
}
