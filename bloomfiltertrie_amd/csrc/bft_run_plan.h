// bft_run_plan.h -- which road the insertion log takes to become a run: the conditions of the bulk build's run stage (bft_run.hip: bft_make_run) and
// the format of the log (bft_gpu.hip: log_reserve, bft_log_prepare), one definition for both and for bft_gpu_debug_run_plan, which hands the rules to
// the tests without a handle or a device (tests/test_run_cases_host.py proves with it that every case of tests/test_gpu_run_edges.py takes the road
// it is named after).  Plain values in, no device code: k, the words of a key W, whether the ids of the log ascend, "build_composite",
// "build_msd", "composite_log", the largest genome id, the bits of an id gb, the pairs of the log.  See DESIGN.md "Insertion".
#pragma once
#include <stdint.h>

#include <algorithm>

constexpr int BFT_RUN_SPLIT_TOP = 18;                // the root-prefix split sorts on the top 18 bits of the T-form (all of them below k = 9)
constexpr uint64_t BFT_RUN_SPLIT_FROM = 1ull << 20;  // "build_msd" 1: the split from this many pairs on
constexpr uint32_t BFT_RUN_CALL_TABLE_MAX = 1u << 16;  // the multi-word sort reads a pair's id out of the table of insert calls up to this many entries (else out of g[])

static inline int bft_run_id_bits(uint64_t v) {  // bits of the id field that holds ids up to v
    int b = 1;
    while (b < 64 && (v >> b)) b++;
    return b;
}
static inline unsigned bft_run_split_top(int k) { return (unsigned)std::min(BFT_RUN_SPLIT_TOP, 2 * k); }
// one-word keys whose ids arrived ascending: the stable sorts keep the ids in order inside a k-mer ("build_composite" 0: the general road anyway)
static inline bool bft_run_ordered_w1(int W, bool ids_ordered, bool composite) { return W == 1 && ids_ordered && composite; }
// (composites of up to 63 bits: a limit from the time of the library sort -- rocPRIM's radix sort mis-sorts the bit range [2, 64), found by
// test_any_k_against_ground_truth[31-0] -- kept: the paths behind it are the tested ones for such k)
static inline bool bft_run_composite_fits(int k, int W, bool ids_ordered, bool composite, int gb) { return bft_run_ordered_w1(W, ids_ordered, composite) && 2 * k + gb <= 63; }
// "build_msd": the root-prefix split + bucket sorts for 2^20 pairs and more (1), always (2), never (0)
static inline bool bft_run_split_wanted(int msd, uint64_t total) { return msd && (total >= BFT_RUN_SPLIT_FROM || msd == 2); }
// inside a root-prefix bucket the prefix is implied: the bits below it and the id make a composite of one word
static inline bool bft_run_bucket_holds_id(int k, int gb) { return (2 * k - (int)bft_run_split_top(k)) + gb <= 64; }
// ordered one-word keys whose composite does not fit travel as (k-mer, id) pairs, where that beats the general road: ids narrowed to one or
// two bytes, or buckets that hold the id
static inline bool bft_run_pairs_fit(int k, int W, bool ids_ordered, bool composite, uint32_t max_gid, int gb) {
    return bft_run_ordered_w1(W, ids_ordered, composite) && (max_gid < 65536 || bft_run_bucket_holds_id(k, gb));
}
// (not at k = 32: a limit from the time of the library sort, which mis-sorted the bit range [46, 64) the split would sort -- found by
// tools/stress_parity.py, k = 32 with build_msd = 2; bft_rs sorts that very range for two-word keys, but k = 32 stays on its tested path)
static inline bool bft_run_pairs_split_ok(int k, int gb) { return bft_run_bucket_holds_id(k, gb) && 2 * k < 64; }
static inline bool bft_run_ordered_w2(int W, bool ids_ordered, bool composite) { return W == 2 && ids_ordered && composite; }  // ("build_composite" 0: the general road, as for one word)
// what pairs_split / pairs_sort narrow the ids to: bytes of an id beside the keys
static inline uint32_t bft_run_id_width(uint32_t max_gid) { return max_gid < 256 ? 1u : max_gid < 65536 ? 2u : 4u; }

// ---- the log's format ----------------------------------------------------------------------------------------------------------------------
// id bits of a composite log (one-word keys with room for 7 bits and more beside them, at most 24), 0: k-mers + ids are logged
static inline uint32_t bft_run_log_comp_bits(int k, int W, bool composite_log, bool composite) {
    const int room = 63 - 2 * k;
    return (W == 1 && composite_log && composite && room >= 7) ? (uint32_t)std::min(room, 24) : 0u;
}
// an id the composites of the log have room for (else the log is taken apart into k-mers + ids)
static inline bool bft_run_log_holds_id(uint32_t log_gb, uint32_t id_genome) { return (id_genome >> log_gb) == 0; }
// at build time only the composite roads take a log of composites
static inline bool bft_run_log_stays_composite(bool ids_ordered, bool composite) { return ids_ordered && composite; }

// ---- the road ------------------------------------------------------------------------------------------------------------------------------
// {1 + road (1 composites, 2 (k-mer, id) pairs, 3 whatever is left), gb, bytes of an id beside the keys (0: composites), 1: the split is tried}
struct BftRunRoad {
    uint32_t v[4];
};
static inline BftRunRoad bft_run_road(int k, int W, bool ids_ordered, bool composite, int msd, uint32_t max_gid, int gb, uint64_t total) {
    const bool split = bft_run_split_wanted(msd, total);
    if (bft_run_composite_fits(k, W, ids_ordered, composite, gb)) return BftRunRoad{{1u, (uint32_t)gb, 0u, split}};
    if (bft_run_pairs_fit(k, W, ids_ordered, composite, max_gid, gb)) return BftRunRoad{{2u, (uint32_t)gb, bft_run_id_width(max_gid), split && bft_run_pairs_split_ok(k, gb)}};
    return BftRunRoad{{3u, (uint32_t)gb, 4u, split && bft_run_ordered_w2(W, ids_ordered, composite)}};
}
