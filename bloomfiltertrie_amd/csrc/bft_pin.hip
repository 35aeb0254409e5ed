// bft_pin.hip -- what every unit of the library waits and zeroes with: the polled wait on a pinned block's ticket (bft_dev.h), the zeroing kernel
// that a captured graph may replay, and the counts channel on top of the block (bft_counts.h): scans whose totals land in it, device words
// published into it, one wait for all of them.

#include <atomic>

#include "bft_counts.h"
#include "bft_dev.h"
#include "bft_scan.h"

__global__ void k_pin_ticket(uint64_t* __restrict__ slot, uint64_t v) {
    __threadfence_system();
    *reinterpret_cast<volatile uint64_t*>(slot) = v;
}
__global__ void k_zero_words(uint32_t* __restrict__ p, uint64_t words) {
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < words; i += (uint64_t)gridDim.x * blockDim.x) p[i] = 0u;
}

namespace {

// (PinBlock, bft_dev.h: counts the host needs come back through a pinned block that kernels write)
__global__ void k_set32(uint32_t* __restrict__ p, uint32_t v) { *p = v; }
__global__ void k_publish(const uint32_t* __restrict__ v, int n, uint64_t* __restrict__ slots) {
    if ((int)threadIdx.x < n) slots[threadIdx.x] = v[threadIdx.x];
}
// the same, and behind the values the block's ticket (bft_pin_wait_for): the launch the host waits for
__global__ void k_publish_ticket(const uint32_t* __restrict__ v, int n, uint64_t* __restrict__ slots, uint64_t* __restrict__ ticket_slot, uint64_t ticket) {
    if ((int)threadIdx.x < n) slots[threadIdx.x] = v[threadIdx.x];
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) *reinterpret_cast<volatile uint64_t*>(ticket_slot) = ticket;
}

}  // namespace

int bft_zero_async(void* p, size_t bytes, hipStream_t s) {
    if (!bytes) return 0;
    if ((bytes & 3u) || ((uintptr_t)p & 3u)) return bft_fail(BFT_GPU_E_ARG, "internal: bft_zero_async wants whole aligned words");
    const uint64_t words = bytes / 4;
    hipLaunchKernelGGL(k_zero_words, dim3(bft_grid_for((words + 255) / 256)), dim3(256), 0, s, (uint32_t*)p, words);
    HIPCK(hipGetLastError());
    return 0;
}
int bft_set32_async(uint32_t* p, uint32_t v, hipStream_t s) {
    hipLaunchKernelGGL(k_set32, dim3(1), dim3(1), 0, s, p, v);
    HIPCK(hipGetLastError());
    return 0;
}
uint64_t bft_pin_next_ticket() {
    static std::atomic<uint64_t> tickets{0};
    return tickets.fetch_add(1) + 1;
}
int bft_pin_post(PinBlock& pin, hipStream_t s, uint64_t* ticket) {
    if (!pin.p) return bft_fail(BFT_GPU_E_HIP, "hipHostMalloc (pinned counts)");
    *ticket = bft_pin_next_ticket();
    hipLaunchKernelGGL(k_pin_ticket, dim3(1), dim3(1), 0, s, pin.p + PIN_SLOTS, *ticket);
    HIPCK(hipGetLastError());
    return 0;
}
int bft_pin_wait_for(PinBlock& pin, hipStream_t s, uint64_t want) {
    volatile uint64_t* t = pin.p + PIN_SLOTS;
    for (uint32_t i = 1;; i++) {
        if (*t == want) break;
        __builtin_ia32_pause();
        if ((i & 0xFFFu) == 0) {  // every 4096 polls: is the stream still at it?
            const hipError_t q = hipStreamQuery(s);
            if (q == hipSuccess) {  // through: the ticket is there
                if (*t == want) break;
                HIPCK(hipStreamSynchronize(s));
                if (*t == want) break;
                return bft_fail(BFT_GPU_E_HIP, "pinned ticket not written");
            }
            if (q != hipErrorNotReady) HIPCK(q);
        }
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    return 0;
}
int bft_pin_wait(PinBlock& pin, hipStream_t s) {
    uint64_t want = 0;
    CK(bft_pin_post(pin, s, &want));
    return bft_pin_wait_for(pin, s, want);
}
int bft_pin_publish(PinBlock& pin, hipStream_t s, const uint32_t* d_vals, int n, int slot) {
    if (!pin.p) return bft_fail(BFT_GPU_E_HIP, "hipHostMalloc (scan totals)");
    hipLaunchKernelGGL(k_publish, dim3(1), dim3(PIN_SLOTS), 0, s, d_vals, n, pin.p + slot);
    HIPCK(hipGetLastError());
    return 0;
}

// ---- BftCounts (bft_counts.h) ----
int BftCounts::enqueue(const uint32_t* in, uint32_t* out, uint64_t n, int slot, bool tail) {
    if (!pin.p) return bft_fail(BFT_GPU_E_HIP, "hipHostMalloc (scan totals)");
    if (n == 0) {  // (the slot is not in flight: wait() precedes every reuse)
        pin.p[slot] = 0;
        if (tail) CK(bft_set32_async(out, 0u, s));
        return 0;
    }
    CK(bft_scan::exclusive_sum_ptr<uint32_t>(in, out, n, s, tmp, (unsigned long long*)(pin.p + slot), tail));  // (the last tile writes the total)
    return 0;
}
int BftCounts::publish(const uint32_t* d_vals, int n, int slot) {
    if (!pin.p) return bft_fail(BFT_GPU_E_HIP, "hipHostMalloc (scan totals)");
    if (pend_vals) CK(bft_pin_publish(pin, s, pend_vals, pend_n, pend_slot));  // (the one before: it rides no ticket)
    pend_vals = d_vals;
    pend_n = n;
    pend_slot = slot;
    return 0;
}
int BftCounts::wait() {
    if (pend_vals) {
        if (!pin.p) return bft_fail(BFT_GPU_E_HIP, "hipHostMalloc (scan totals)");
        const uint64_t ticket = bft_pin_next_ticket();
        hipLaunchKernelGGL(k_publish_ticket, dim3(1), dim3(PIN_SLOTS), 0, s, pend_vals, pend_n, pin.p + pend_slot, pin.p + PIN_SLOTS, ticket);
        pend_vals = nullptr;
        HIPCK(hipGetLastError());
        return bft_pin_wait_for(pin, s, ticket);
    }
    HIPCK(hipGetLastError());
    return bft_pin_wait(pin, s);
}
int BftCounts::run(const uint32_t* in, uint32_t* out, uint64_t n, uint64_t* total) {
    if (!total) {
        if (n == 0) return 0;
        CK(bft_scan::exclusive_sum_ptr<uint32_t>(in, out, n, s, tmp));
        return 0;
    }
    CK(enqueue(in, out, n, 0));
    CK(wait());
    *total = get(0);
    return 0;
}
