// bft_counts.h -- the channel for device counts the host needs (bft_pin.hip): scans whose totals land in a pinned block (PinBlock, bft_dev.h),
// device words published into it, and ONE polled wait for all that was enqueued.
#pragma once
#include "bft_dev.h"

struct BftCounts {
    DevBuf tmp;  // the scans' scratch (bft_scan.h); a caller's own scan on this stream may share it, and write its total to a slot of `pin`
    hipStream_t s;
    PinBlock pin;
    explicit BftCounts(hipStream_t st) : s(st) {}
    // out = exclusive sum of in (u32); the total lands in slot `slot` of the pinned block once the stream gets there
    // tail: out[n] = total as well
    int enqueue(const uint32_t* in, uint32_t* out, uint64_t n, int slot, bool tail = false);
    // n <= PIN_SLOTS device words -> slots [slot, slot + n).  The launch is made by wait() (it carries the ticket the host polls for: one launch
    // instead of two) or by the next publish(): the words are read when it runs, behind everything enqueued until then.
    int publish(const uint32_t* d_vals, int n, int slot);
    int wait();
    uint64_t get(int slot) const { return pin.p[slot]; }
    // the scan alone (total == nullptr: nothing reaches the host), or the scan, a wait and its total
    int run(const uint32_t* in, uint32_t* out, uint64_t n, uint64_t* total);

private:
    const uint32_t* pend_vals = nullptr;
    int pend_n = 0, pend_slot = 0;
};
// n <= PIN_SLOTS device words -> slots [slot, slot + n) of a block of the caller's, on any stream: read by the host once that stream is through
int bft_pin_publish(PinBlock& pin, hipStream_t s, const uint32_t* d_vals, int n, int slot);
