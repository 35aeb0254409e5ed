// bft_front_plan.h -- which kernel sorts a root-prefix bucket: the selection rules of the bulk build's front end (bft_front.hip), one definition
// for the launchers (bft_front_buckets, bft_front2_buckets), for the kernel that lists the two-word buckets by size class (k_bucket2_lists) and for
// bft_gpu_debug_front_plan, which hands the rules to the tests without a handle or a device (tests/test_front_cases_host.py proves with it that
// every case of tests/test_gpu_front_edges.py runs the kernel it is named after).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define BFT_FRONT_HD __host__ __device__
#else
#define BFT_FRONT_HD
#endif

#define FB_BLOCK 256
#define FB_WAVES (FB_BLOCK / 64)
#define FB_EMAX 16                      // composites per thread
#define FB_CAP (FB_BLOCK * FB_EMAX)     // largest one-word bucket sorted in LDS (4096 composites = 32 KB)
#define FB2_CLASSES 6
#define FB2_TINY 5                      // the class of a two-word bucket of up to 64 items (k_bucket2_tiny)
#define FB2_CAP (FB_BLOCK * 32)         // largest two-word bucket sorted in LDS (8192 items)

// ---- one-word keys ---------------------------------------------------------------------------------------------------------------------------------
struct BftFrontPlan {
    uint32_t wave_cap;  // buckets of up to wave_cap composites are k_bucket_sort_wave<wave_cap / 64>'s, a wavefront each
    uint32_t wave_ew;   // that kernel's composites per lane: 8 or 16
    uint32_t wg_e;      // the larger ones are k_bucket_sort<wg_e, false>'s, a workgroup each: 6, 9, 12, 16; 0: there are none, nothing is launched
    bool declines;      // the largest bucket is beyond FB_CAP: nothing is produced, the caller sorts device-wide
};

// The wavefront kernel's variant follows the MEAN bucket (it is launched before the largest bucket is known on the host): n composites in nb buckets.
// forced: 0 = by rule, 512 or 1024 = that value ("test_front_wave_cap").
static inline uint32_t bft_front_wave_cap(uint64_t n, uint32_t nb, uint32_t forced) {
    if (forced) return forced;
    return n / (nb ? nb : 1u) <= 192u ? 512u : 1024u;
}

// mx: the largest bucket.  (The smallest workgroup variant that holds it: the kernel is bound by the latency of its LDS round trips and barriers,
// and both the registers and the LDS of a workgroup go with the composites per thread.)
static inline BftFrontPlan bft_front_plan(uint64_t n, uint32_t nb, uint32_t mx, uint32_t forced_wave_cap) {
    BftFrontPlan p;
    p.wave_cap = bft_front_wave_cap(n, nb, forced_wave_cap);
    p.wave_ew = p.wave_cap / 64u;
    p.declines = mx > FB_CAP;
    p.wg_e = 0;
    if (p.declines || mx <= p.wave_cap) return p;
    p.wg_e = mx <= 256u * 6u ? 6u : mx <= 256u * 9u ? 9u : mx <= 256u * 12u ? 12u : 16u;
    return p;
}

// ---- two-word keys ---------------------------------------------------------------------------------------------------------------------------------
// The size class of a bucket of n items: -1 empty; FB2_TINY up to 64 (k_bucket2_tiny); 0, 1, 2 up to 512 / 1024 / 2048 (k_bucket2_sort_wave<8 | 16 | 32>,
// a wavefront each); 3, 4 up to 4096 / 8192 (k_bucket2_sort<16 | 32, false>, a workgroup each; 4 also what lies beyond: the launcher declines first).
BFT_FRONT_HD static inline int bft_front2_class(uint32_t n) {
    return n == 0 ? -1 : n <= 64u ? FB2_TINY : n <= 512u ? 0 : n <= 1024u ? 1 : n <= 2048u ? 2 : n <= 4096u ? 3 : 4;
}
// items per lane (classes 0..2) / per thread (3, 4) of the class's kernel; 1 for the tiny buckets
static inline uint32_t bft_front2_class_items(int cls) { return cls == FB2_TINY ? 1u : cls == 0 ? 8u : cls == 1 ? 16u : cls == 2 ? 32u : cls == 3 ? 16u : cls == 4 ? 32u : 0u; }

struct BftFront2Plan {
    bool pack;      // every genome id is below 2^18: the ids ride in the 18 free bits on top of hk's 46 (k_bucket2_sort_wave<.., true>)
    bool class3;    // k_bucket2_sort<16, false> is launched (some bucket holds more than 2048 items)
    bool class4;    // k_bucket2_sort<32, false> is launched (more than 4096)
    bool declines;  // the largest bucket is beyond FB2_CAP: nothing is produced, the caller sorts device-wide
};
static inline bool bft_front2_pack(uint32_t max_gid) { return max_gid < (1u << 18); }
static inline BftFront2Plan bft_front2_plan(uint32_t mx, uint32_t max_gid) {
    BftFront2Plan p;
    p.pack = bft_front2_pack(max_gid);
    p.declines = mx > FB2_CAP;
    p.class3 = !p.declines && mx > 2048u;
    p.class4 = !p.declines && mx > 4096u;
    return p;
}
