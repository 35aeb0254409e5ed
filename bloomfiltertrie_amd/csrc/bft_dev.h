// bft_dev.h -- small HIP host-side helpers shared by the translation units of libbft_gpu.so: error macros, device buffers, the pinned block and
// its waits, the launch kit, the build's trace and stage marks.  What a unit offers the others is declared in that unit's own header.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/bft_gpu.h"

int bft_fail(int code, const std::string& msg);  // records the thread's last error, returns code

#define HIPCK(expr)                                                                                           \
    do {                                                                                                      \
        hipError_t e_ = (expr);                                                                               \
        if (e_ != hipSuccess) return bft_fail(BFT_GPU_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)
#define CK(expr)                  \
    do {                          \
        int rc_ = (expr);         \
        if (rc_ != 0) return rc_; \
    } while (0)

// Device-memory cache behind DevBuf (bft_gpu.hip).  hipFree synchronises the device and costs ~0.1 ms per call on
// large blocks; a bulk build releases dozens of temporaries.  Released blocks are kept (per device, tagged with the
// stream of the ABI call that released them) and handed out again to requests of a similar size.  A block released
// under another stream is only reused after that stream has drained; bft_gpu_free drops the blocks of its handle.
int bft_pool_alloc(void** p, size_t n, size_t* cap);
void bft_pool_release(void* p, size_t cap);
void bft_pool_set_stream(int device, hipStream_t s);  // the stream of the current ABI call (thread-local)
void bft_pool_drop_stream(hipStream_t s);             // the stream was synchronised and is about to be destroyed: its blocks stay cached, tagged as drained

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;  // requested size
    size_t cap = 0;    // size of the block behind it
    // the user's (bft_scan.h: launches so far, states the last one used); zero after every alloc.  A block that a scan uses must not be written by
    // anything else -- a kernel, a memset, a sort's scratch -- unless that writer sets tag = 0: the next scan trusts tag and skips its zeroing.
    uint32_t tag = 0, tag2 = 0;
    DevBuf() {}
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes), cap(o.cap), tag(o.tag), tag2(o.tag2) { o.p = nullptr; o.bytes = 0; o.cap = 0; o.tag = 0; o.tag2 = 0; }
    ~DevBuf() { release(); }
    void release() {
        if (p) bft_pool_release(p, cap);
        p = nullptr;
        bytes = 0;
        cap = 0;
        tag = 0;
        tag2 = 0;
    }
    int alloc(size_t n) {
        release();
        if (n == 0) n = 8;
        CK(bft_pool_alloc(&p, n, &cap));
        bytes = n;
        return 0;
    }
    int alloc_zero(size_t n, hipStream_t s) {
        CK(alloc(n));
        // (whole 16-byte words: the runtime fills an odd tail with a second kernel)
        HIPCK(hipMemsetAsync(p, 0, std::min(cap, (bytes + 15) & ~(size_t)15), s));
        return 0;
    }
    template <class T>
    T* as() const { return (T*)p; }
    void swap(DevBuf& o) {
        std::swap(p, o.p);
        std::swap(bytes, o.bytes);
        std::swap(cap, o.cap);
        std::swap(tag, o.tag);
        std::swap(tag2, o.tag2);
    }
};
// a DevBuf of n elements of T: sized by the count (n == 0: DevBuf's 8 bytes), handed to a kernel as a T*
template <class T>
struct DevArr : DevBuf {
    int alloc(uint64_t n) { return DevBuf::alloc(n * sizeof(T)); }
    int alloc_zero(uint64_t n, hipStream_t s) { return DevBuf::alloc_zero(n * sizeof(T), s); }
    operator T*() const { return (T*)p; }
};

// Counts the host needs (array sizes, format limits) come back through a pinned block that kernels write: the scans and checks
// of a stage are enqueued together and share ONE stream synchronisation (a total fetched by hipMemcpyAsync into pageable memory is
// two staged copies and a synchronisation of its own: ~60 us each, sixteen per trie level).
constexpr int PIN_SLOTS = 32;  // (+ one word behind them: the ticket of bft_pin_wait)
struct PinBlock;
// Waits until everything enqueued on `s` so far has run, by POLLING: a one-thread kernel behind it all writes a ticket into the pinned block and the
// host spins on that word.  hipStreamSynchronize / hipEventSynchronize sleep on an interrupt and come back ~0.1 ms after the stream is through --
// eleven such waits a build (array sizes the host needs) were a millisecond of idle GPU.  The stream's state is looked at every few thousand polls:
// an error there ends the wait with that error.  (bft_pin.hip; the scans and publishes that feed the block: bft_counts.h)
int bft_pin_wait(PinBlock& pin, hipStream_t s);
// the same in two steps: the ticket enqueued here, waited for later (what is enqueued in between is not waited for; one ticket in flight per block)
int bft_pin_post(PinBlock& pin, hipStream_t s, uint64_t* ticket);
int bft_pin_wait_for(PinBlock& pin, hipStream_t s, uint64_t ticket);
// Zeroes `bytes` bytes (a multiple of 4, 4-byte aligned) at p with a kernel of the library's own.  For every path a caller may record into a HIP graph:
// a hipMemsetAsync node replays correctly ONCE on this runtime (ROCm 7.0.2: the second replay of a captured memset writes garbage --
// tools/probe_graph_memset.py), a kernel node every time.  (bft_pin.hip)
int bft_zero_async(void* p, size_t bytes, hipStream_t s);
int bft_set32_async(uint32_t* p, uint32_t v, hipStream_t s);  // *p = v, by a kernel as well
uint64_t bft_pin_next_ticket();  // (for a kernel of the caller's that writes the ticket itself, behind its own results: pin.p[PIN_SLOTS], after __threadfence_system())
struct PinBlock {
    uint64_t* p = nullptr;
    PinBlock() {
        {
            std::lock_guard<std::mutex> lk(mu());
            if (!cache().empty()) { p = cache().back(); cache().pop_back(); }
        }
        if (!p && hipHostMalloc((void**)&p, (PIN_SLOTS + 1) * 8, hipHostMallocPortable | hipHostMallocMapped) != hipSuccess) { p = nullptr; (void)hipGetLastError(); }
    }
    ~PinBlock() {
        if (!p) return;
        std::lock_guard<std::mutex> lk(mu());
        cache().push_back(p);  // (a handful of 256-byte blocks per process, kept; portable: any device of the process may write them)
    }
    static std::mutex& mu() { static std::mutex m; return m; }
    static std::vector<uint64_t*>& cache() { static std::vector<uint64_t*> c; return c; }
};


static inline int bft_grid_for(uint64_t nblk) {
    const uint64_t cap = 256ull * 8ull;  // 256 CUs x 8 resident workgroups of 256 threads
    return (int)std::max<uint64_t>(1, std::min<uint64_t>(nblk, cap));
}

// The launch kit of the whole-graph and analysis units (host only): their kernels run grid-stride loops in workgroups of BFT_LAUNCH_THREADS.
constexpr int BFT_LAUNCH_THREADS = 256;
// kernel<<<bft_grid_for(ceil(items / 256)), 256, 0, s>>>(args...); nothing at items == 0.  (The arguments are converted at the launch: a DevArr<T>
// goes in as its T*.)
template <class K, class... A>
static int bft_launch256(K kernel, uint64_t items, hipStream_t s, const A&... args) {
    if (items == 0) return 0;
    hipLaunchKernelGGL(kernel, dim3(bft_grid_for((items + BFT_LAUNCH_THREADS - 1) / BFT_LAUNCH_THREADS)), dim3(BFT_LAUNCH_THREADS), 0, s, args...);
    HIPCK(hipGetLastError());
    return 0;
}
// f(std::integral_constant<int, W>) for the key width W = 1..4 (words per k-mer): the kernels are templates over it.  f launches and returns a code
template <class F>
static int bft_for_w(int W, F&& f) {
    int rc;
    switch (W) {
    case 1: rc = f(std::integral_constant<int, 1>()); break;
    case 2: rc = f(std::integral_constant<int, 2>()); break;
    case 3: rc = f(std::integral_constant<int, 3>()); break;
    default: rc = f(std::integral_constant<int, 4>()); break;
    }
    CK(rc);
    HIPCK(hipGetLastError());
    return 0;
}

bool bft_trace_on(void);
void bft_trace_mark(const char* what);  // BFT_GPU_TRACE_BUILD=1 (nullptr: start of a build)
// "build_stages" 1: a stage of the running build ends here on stream s; bytes = what its algorithm reads + writes (0: not a streaming
// stage).  A name that starts with '+' marks work on a side stream, timed from the build's start.  No-op unless the option is on.
void bft_stage(const char* name, double bytes, hipStream_t s);

