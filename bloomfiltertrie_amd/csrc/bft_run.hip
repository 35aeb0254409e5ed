// bft_run.hip -- steps 1-3 of the bulk build: the insertion log becomes a run (BftPairRun: sorted distinct T-form k-mers, the offsets of their
// genome-id lists, the ids).  bft_make_run is the list of the roads a log can take, with their conditions and fallbacks; every road is a function
// of its own below it.  Sorts and scans are the library's own (bft_sort.h, bft_scan.h); the buckets behind the root-prefix split are
// bft_front.hip's; the kernels launched here are bft_kernels_build.h's.  bft_sort_pairs, the general permutation sort, is also what
// bft_ensure_table and the sub-graph build order their records with.  See DESIGN.md "Insertion".
#include <hip/hip_runtime.h>

#include <algorithm>

#include "bft_handle.h"
#include "bft_run.h"
#include "bft_scan.h"

#include "bft_kernels_build.h"

static int bits_for(uint64_t v) {
    int b = 1;
    while (b < 64 && (v >> b)) b++;
    return b;
}

int bft_sort_pairs(bft_gpu* h, const uint64_t* keys, uint64_t stride, const uint32_t* g, uint64_t total, uint64_t* okeys, uint64_t ostride, uint32_t* og,
                   bool g_already_ordered, bool is_log) {
    const int W = h->W;
    if (W == 1) {
        // one-word keys: sort the (key, genome) pairs themselves; the radix sort is stable, so a genome-id pass
        // first (skipped when the ids already ascend) followed by the key pass gives (T, genome) order
        DevBuf k2, g2;
        const uint64_t* kin = keys;
        const uint32_t* gin = g;
        if (!g_already_ordered) {
            CK(k2.alloc(total * 8));
            CK(g2.alloc(total * 4));
            const int gb = bits_for(h->max_gid_seen);
            CK((bft_rs::sort_pairs<uint32_t, uint64_t>(gin, kin, total, g2.as<uint32_t>(), k2.as<uint64_t>(), 0, gb, h->stream)));
            kin = k2.as<uint64_t>();
            gin = g2.as<uint32_t>();
        }
        CK((bft_rs::sort_pairs<uint64_t, uint32_t>(kin, gin, total, okeys, og, 0, 2 * h->k, h->stream)));
        HIPCK(hipGetLastError());
        HIPCK(hipStreamSynchronize(h->stream));
        return 0;
    }
    DevBuf perm, perm2, ku, ku2, kg2;
    CK(perm.alloc(total * 4));
    CK(perm2.alloc(total * 4));
    CK(ku.alloc(total * 8));
    CK(ku2.alloc(total * 8));
    const int grid = bft_grid_for((total + 255) / 256);
    hipLaunchKernelGGL(k_iota, dim3(grid), dim3(256), 0, h->stream, perm.as<uint32_t>(), total);
    // pass 0: genome id (least significant); skipped when the input is already in genome-id order
    // (ids inserted in non-decreasing order, as the reference requires: the stable key passes keep it)
    if (!g_already_ordered) {
        CK(kg2.alloc(total * 4));
        const int gb = bits_for(h->max_gid_seen);
        CK((bft_rs::sort_pairs<uint32_t, uint32_t>(g, perm.as<uint32_t>(), total, kg2.as<uint32_t>(), perm2.as<uint32_t>(), 0, gb, h->stream)));
        perm.swap(perm2);
    }
    // passes over the key words, least significant word (W-1) first
    for (int w = W - 1; w >= 0; w--) {
        const int nbits = (w == 0) ? (2 * h->k - 64 * (W - 1)) : 64;
        const uint64_t* kin = keys + (uint64_t)w * stride;
        if (w != W - 1 || !g_already_ordered) {  // (the first pass of an id-ordered log: the permutation is still the identity, the word is sorted where it lies)
            hipLaunchKernelGGL(k_gather<uint64_t>, dim3(grid), dim3(256), 0, h->stream, kin, perm.as<uint32_t>(), ku.as<uint64_t>(), total);
            kin = ku.as<uint64_t>();
        }
        CK((bft_rs::sort_pairs<uint64_t, uint32_t>(kin, perm.as<uint32_t>(), total, ku2.as<uint64_t>(), perm2.as<uint32_t>(), 0, nbits, h->stream)));
        perm.swap(perm2);
    }
    // (one pass over the permutation for every word and the id, instead of a pass each; the ids of the LOG come out of the table of its insert calls)
    DevBuf lbe, lbg;
    uint32_t nlb = 0;
    if (is_log && !h->lb_end.empty() && h->lb_end.size() <= (1u << 16) && h->lb_end.back() == total) {
        nlb = (uint32_t)h->lb_end.size();
        CK(lbe.alloc(nlb * 8));
        CK(lbg.alloc(nlb * 4));
        HIPCK(hipMemcpyAsync(lbe.p, h->lb_end.data(), nlb * 8, hipMemcpyHostToDevice, h->stream));
        HIPCK(hipMemcpyAsync(lbg.p, h->lb_gid.data(), nlb * 4, hipMemcpyHostToDevice, h->stream));
    }
    hipLaunchKernelGGL(k_gather_pairs, dim3(grid), dim3(256), 0, h->stream, keys, stride, W, g, perm.as<uint32_t>(), okeys, ostride, og, total, lbe.as<uint64_t>(), lbg.as<uint32_t>(), nlb);
    HIPCK(hipGetLastError());
    HIPCK(hipStreamSynchronize(h->stream));
    return 0;
}

namespace {
// 1. the pairs to sort: the insertion log
struct LogIn {
    const uint64_t* k;  // SoA: W key arrays `stride` apart (a log of composites: T << gb | genome, and g is not read)
    const uint32_t* g;
    uint64_t stride, total;
    int gb;  // bits of a genome id (a log of composites: their id field as logged)
};

// ---- which road: every condition once ------------------------------------------------------------------------------------------------------
constexpr int SPLIT_TOP = 18;  // the root-prefix split sorts on the top 18 bits of the T-form (all of them below k = 9)
unsigned split_top(const bft_gpu* h) { return (unsigned)std::min(SPLIT_TOP, 2 * h->k); }
// one-word keys whose ids arrived ascending: the stable sorts keep the ids in order inside a k-mer ("build_composite" 0: the general road anyway)
bool ordered_w1(const bft_gpu* h) { return h->W == 1 && h->log_g_sorted && !h->opt_no_composite; }
// (composites of up to 63 bits: a limit from the time of the library sort -- rocPRIM's radix sort mis-sorts the bit range [2, 64), found by
// test_any_k_against_ground_truth[31-0] -- kept: the paths behind it are the tested ones for such k)
bool composite_fits(const bft_gpu* h, int gb) { return ordered_w1(h) && 2 * h->k + gb <= 63; }
// "build_msd": the root-prefix split + bucket sorts for 2^20 pairs and more (1), always (2), never (0)
bool split_wanted(const bft_gpu* h, uint64_t total) { return h->opt_msd && (total >= (1u << 20) || h->opt_msd == 2); }
// inside a root-prefix bucket the prefix is implied: the bits below it and the id make a composite of one word
bool bucket_holds_id(const bft_gpu* h, int gb) { return (2 * h->k - (int)split_top(h)) + gb <= 64; }
// ordered one-word keys whose composite does not fit travel as (k-mer, id) pairs, where that beats the general road: ids narrowed to one or
// two bytes, or buckets that hold the id
bool pairs_fit(const bft_gpu* h, int gb) { return ordered_w1(h) && (h->max_gid_seen < 65536 || bucket_holds_id(h, gb)); }
// (not at k = 32: a limit from the time of the library sort, which mis-sorted the bit range [46, 64) the split would sort -- found by
// tools/stress_parity.py, k = 32 with build_msd = 2; bft_rs sorts that very range for two-word keys, but k = 32 stays on its tested path)
bool pairs_split_ok(const bft_gpu* h, int gb) { return bucket_holds_id(h, gb) && 2 * h->k < 64; }
bool ordered_w2(const bft_gpu* h) { return h->W == 2 && h->log_g_sorted; }

// ---- what the roads share ------------------------------------------------------------------------------------------------------------------
// the run's arrays for nk k-mers of W words and np pairs
int run_alloc(BftPairRun& run, uint64_t nk, uint64_t np, int W) {
    run.nk = nk;
    run.np = np;
    CK(run.tk.alloc(nk * W * 8));
    CK(run.seg_off.alloc((nk + 1) * 4));
    return run.ids.alloc(np * 4);
}
// behind a road's scatter kernel: the end of the last list, the launch check, the stream drained
int run_close(bft_gpu* h, BftPairRun& run) {
    const uint32_t np32 = (uint32_t)run.np;
    HIPCK(hipMemcpyAsync(run.seg_off.as<uint32_t>() + run.nk, &np32, 4, hipMemcpyHostToDevice, h->stream));
    HIPCK(hipGetLastError());
    HIPCK(hipStreamSynchronize(h->stream));
    return 0;
}
// Behind the root-prefix split: the offsets of the 2^top buckets and the size of the largest, on the device.  Allocated in front of the split's
// sort (the counter is zeroed on the stream there), filled behind it.
struct SplitBounds {
    DevBuf boff, maxb;
    int alloc(unsigned top, hipStream_t s) { CK(boff.alloc(((1u << top) + 1) * 4)); return maxb.alloc_zero(4, s); }
};
// keys: sorted on their `top` bits from `shift` up; dbase / dbits: where the last pass of that sort left its digit's bounds (k_msd_bounds)
void split_bounds(bft_gpu* h, const uint64_t* keys, uint64_t total, uint32_t shift, uint32_t top, const uint32_t* dbase, uint32_t dbits, SplitBounds& b) {
    hipLaunchKernelGGL(k_msd_bounds, dim3(((1u << top) + 1 + 255) / 256), dim3(256), 0, h->stream, keys, total, shift, 1u << top, b.boff.as<uint32_t>(), dbase, dbits, top);
    hipLaunchKernelGGL(k_msd_max, dim3(((1u << top) + 255) / 256), dim3(256), 0, h->stream, b.boff.as<uint32_t>(), 1u << top, b.maxb.as<uint32_t>());
}
uint32_t last_digit_bits(const bft_rs::Plan& spl) { return spl.P ? spl.nbits[spl.P - 1] : 0u; }

// ---- composites ----------------------------------------------------------------------------------------------------------------------------
// 2c. MSD first: a stable sort on the top 18 bits of T (the rotated root prefix: 2^18 buckets of ~10^3 composites on a
// pan-genome index), then every bucket on its own on the remaining bits, in LDS, with the duplicates flagged and counted
// on the way (bft_front.hip) -- one read and one write of the array instead of the four or five full passes those
// bits cost a device-wide LSD sort, and no flag scan over the pairs.  Skewed inputs (a bucket beyond what one workgroup
// sorts: done = false) keep the one-sort road.
int composite_split(bft_gpu* h, const LogIn& in, BftPairRun& run, bool& done) {
    const uint64_t total = in.total;
    const int gb = in.gb;
    const unsigned top = split_top(h), rest = (unsigned)(2 * h->k) - top;
    DevBuf cs, tmp, pos;
    CK(cs.alloc(total * 8));
    CK(pos.alloc(total * 8));
    const BftCompose comp{in.k, h->log_comp ? nullptr : in.g, (uint32_t)gb};
    SplitBounds b;
    CK(b.alloc(top, h->stream));
    // (the library's own partition, bft_sort.h: one histogram kernel, a first pass that needs no look-back, a second in 64 chains;
    // the composites are formed from the log by the kernels that read it; `pos` carries them between the two passes)
    const uint32_t* dbase = nullptr;  // (where the last pass's digit -- the top bits of the prefix -- changes: in `tmp`)
    CK((bft_rs::sort<uint64_t, bft_rs::NoVal, BftCompose>(comp, total, cs.as<uint64_t>(), (bft_rs::NoVal*)nullptr, pos.as<uint64_t>(), (bft_rs::NoVal*)nullptr,
                                                          (unsigned)gb + rest, (unsigned)(gb + 2 * h->k), h->stream, tmp, &dbase)));
    split_bounds(h, cs.as<uint64_t>(), total, (uint32_t)(gb + rest), top, dbase, last_digit_bits(bft_rs::make_plan((unsigned)gb + rest, (unsigned)(gb + 2 * h->k))), b);
    // (histogram: the log, 12 B per pair; pass 1: the log in, composites out; pass 2: composites in and out)
    bft_stage("split (root-prefix, 2 x 9 bits)", (double)total * ((h->log_comp ? 8 : 12) * 2 + 8 + 8 + 8), h->stream);
    uint32_t mx = 0;
    CK(bft_front_buckets(cs.as<uint64_t>(), total, b.boff.as<uint32_t>(), 1u << top, (uint32_t)gb, (uint32_t)gb + rest, h->stream, run, b.maxb.as<uint32_t>(), &mx, &done,
                         &h->front_redone));
    h->msd_max_bucket = mx;
    return 0;
}
// 2c + 3c. one device-wide sort of (T << gb | genome) on the T bits, flags on the fly, one scan
int composite_sort(bft_gpu* h, const LogIn& in, BftPairRun& run) {
    const uint64_t total = in.total;
    const int gb = in.gb;
    DevBuf cs, tmp, pos;
    CK(cs.alloc(total * 8));
    CK(pos.alloc(total * 8));
    const BftCompose comp{in.k, h->log_comp ? nullptr : in.g, (uint32_t)gb};
    CK((bft_rs::sort<uint64_t, bft_rs::NoVal, BftCompose>(comp, total, cs.as<uint64_t>(), (bft_rs::NoVal*)nullptr, pos.as<uint64_t>(), (bft_rs::NoVal*)nullptr, (unsigned)gb,
                                                          (unsigned)(gb + 2 * h->k), h->stream, tmp)));
    const BftPairFlags pf{cs.as<uint64_t>(), (uint32_t)gb};
    CK((bft_scan::exclusive_sum<uint64_t>(pf, pos.as<uint64_t>(), total, h->stream, tmp)));
    uint64_t last_pos = 0, last_c[2] = {0, 0};
    HIPCK(hipMemcpyAsync(&last_pos, pos.as<uint64_t>() + total - 1, 8, hipMemcpyDeviceToHost, h->stream));
    HIPCK(hipMemcpyAsync(&last_c[1], cs.as<uint64_t>() + total - 1, 8, hipMemcpyDeviceToHost, h->stream));
    if (total > 1) HIPCK(hipMemcpyAsync(&last_c[0], cs.as<uint64_t>() + total - 2, 8, hipMemcpyDeviceToHost, h->stream));
    HIPCK(hipStreamSynchronize(h->stream));
    const bool last_head = total == 1 || (last_c[1] >> gb) != (last_c[0] >> gb), last_keep = total == 1 || last_c[1] != last_c[0];
    CK(run_alloc(run, (last_pos >> 32) + (last_head ? 1 : 0), (last_pos & 0xFFFFFFFFull) + (last_keep ? 1 : 0), 1));
    hipLaunchKernelGGL(k_scatter_c, dim3(bft_grid_for((total + 255) / 256)), dim3(256), 0, h->stream, cs.as<uint64_t>(), (uint32_t)gb, total, pos.as<uint64_t>(),
                       run.ids.as<uint32_t>(), run.tk.as<uint64_t>(), run.seg_off.as<uint32_t>());
    return run_close(h, run);
}

// ---- (k-mer, id) pairs ---------------------------------------------------------------------------------------------------------------------
// One-word keys, sorted, with their genome ids (GT wide): flags on the fly, one 64-bit scan, scatter into the genome-id lists, the
// distinct-k-mer table and the segment offsets (bft_kernels_build.h).
template <class GT>
int dedupe_w1(bft_gpu* h, const uint64_t* sk, const GT* sg, uint64_t total, BftPairRun& run) {
    DevBuf tmp, pos;
    CK(pos.alloc(total * 8));
    const BftPairFlags2<GT> pf{sk, sg};
    CK((bft_scan::exclusive_sum<uint64_t>(pf, pos.as<uint64_t>(), total, h->stream, tmp)));
    uint64_t last_pos = 0, last_k[2] = {0, 0};
    GT last_g[2] = {0, 0};
    HIPCK(hipMemcpyAsync(&last_pos, pos.as<uint64_t>() + total - 1, 8, hipMemcpyDeviceToHost, h->stream));
    HIPCK(hipMemcpyAsync(&last_k[1], sk + total - 1, 8, hipMemcpyDeviceToHost, h->stream));
    HIPCK(hipMemcpyAsync(&last_g[1], sg + total - 1, sizeof(GT), hipMemcpyDeviceToHost, h->stream));
    if (total > 1) {
        HIPCK(hipMemcpyAsync(&last_k[0], sk + total - 2, 8, hipMemcpyDeviceToHost, h->stream));
        HIPCK(hipMemcpyAsync(&last_g[0], sg + total - 2, sizeof(GT), hipMemcpyDeviceToHost, h->stream));
    }
    HIPCK(hipStreamSynchronize(h->stream));
    const bool last_head = total == 1 || last_k[1] != last_k[0], last_keep = last_head || last_g[1] != last_g[0];
    CK(run_alloc(run, (last_pos >> 32) + (last_head ? 1 : 0), (last_pos & 0xFFFFFFFFull) + (last_keep ? 1 : 0), 1));
    hipLaunchKernelGGL(k_scatter_2<GT>, dim3(bft_grid_for((total + 255) / 256)), dim3(256), 0, h->stream, sk, sg, total, pos.as<uint64_t>(), run.ids.as<uint32_t>(),
                       run.tk.as<uint64_t>(), run.seg_off.as<uint32_t>());
    return run_close(h, run);
}
// Stable sort of ordered one-word keys with their ids narrowed to GT (values through a transform iterator over the log), then dedupe_w1.
template <class GT>
int sort_dedupe_w1_narrow(bft_gpu* h, const LogIn& in, BftPairRun& run) {
    DevBuf sk, sg;
    CK(sk.alloc(in.total * 8));
    CK(sg.alloc(in.total * sizeof(GT)));
    CK((bft_rs::sort_in<uint64_t, GT>(BftPairIn<GT>{in.k, in.g}, in.total, sk.as<uint64_t>(), sg.as<GT>(), 0u, (unsigned)(2 * h->k), h->stream)));
    HIPCK(hipGetLastError());
    return dedupe_w1<GT>(h, sk.as<uint64_t>(), sg.as<GT>(), in.total, run);
}
// The composites' front end for ordered one-word keys whose composite does not fit 63 bits (k = 31 beyond a couple of genomes, k = 27 beyond
// 512): a stable key + value sort on the 18 root-prefix bits -- the ids travel beside the keys, narrowed to VT --, then the buckets
// (bft_front.hip), where the bits a bucket's k-mers share make room for the id.  done = false: a bucket is too large, nothing was built.
template <class VT>
int split_dedupe_w1(bft_gpu* h, const LogIn& in, BftPairRun& run, bool& done) {
    const uint64_t total = in.total;
    const unsigned top = split_top(h), rest = (unsigned)(2 * h->k) - top;
    DevBuf sk, sv;
    SplitBounds b;
    CK(sk.alloc(total * 8));
    CK(sv.alloc(total * sizeof(VT)));
    CK(b.alloc(top, h->stream));
    {
        DevBuf tk2, tv2, scratch;
        const bft_rs::Plan spl = bft_rs::make_plan(rest, (unsigned)(2 * h->k));
        if (spl.P > 1) {
            CK(tk2.alloc(total * 8));
            CK(tv2.alloc(total * sizeof(VT)));
        }
        const uint32_t* dbase = nullptr;
        CK((bft_rs::sort<uint64_t, VT, BftPairIn<VT>>(BftPairIn<VT>{in.k, in.g}, total, sk.as<uint64_t>(), sv.as<VT>(), tk2.as<uint64_t>(), tv2.as<VT>(), rest, (unsigned)(2 * h->k),
                                                      h->stream, scratch, &dbase)));
        split_bounds(h, sk.as<uint64_t>(), total, (uint32_t)rest, top, dbase, last_digit_bits(spl), b);
    }
    bft_stage("split (root-prefix, 2 x 9 bits, pairs)", (double)total * (12 + 12 + 2 * (8 + sizeof(VT)) + (8 + sizeof(VT))), h->stream);
    uint32_t mx = 0;
    CK(bft_front_buckets(sk.as<uint64_t>(), total, b.boff.as<uint32_t>(), 1u << top, (uint32_t)in.gb, (uint32_t)in.gb + rest, h->stream, run, b.maxb.as<uint32_t>(), &mx, &done,
                         &h->front_redone, sv.p, (uint32_t)sizeof(VT)));
    h->msd_max_bucket = mx;
    return 0;
}
// 2s. the root-prefix split with the ids beside the keys, then the buckets -- where the composite does fit, the bucket's number being implied
int pairs_split(bft_gpu* h, const LogIn& in, BftPairRun& run, bool& done) {
    if (h->max_gid_seen < 256) return split_dedupe_w1<uint8_t>(h, in, run, done);
    if (h->max_gid_seen < 65536) return split_dedupe_w1<uint16_t>(h, in, run, done);
    return split_dedupe_w1<uint32_t>(h, in, run, done);
}
// 2n + 3'. one key + value sort over every bit with the ids narrowed to one or two bytes (the values are a third of
// the sort's traffic at four), flags on the fly, one scan
int pairs_sort(bft_gpu* h, const LogIn& in, BftPairRun& run) {
    if (h->max_gid_seen < 256) return sort_dedupe_w1_narrow<uint8_t>(h, in, run);
    if (h->max_gid_seen < 65536) return sort_dedupe_w1_narrow<uint16_t>(h, in, run);
    return sort_dedupe_w1_narrow<uint32_t>(h, in, run);
}

// ---- whatever is left: keys of several words, ids out of order, "build_composite" 0 ----------------------------------------------------------
// 2w. two-word keys (33 <= k <= 64) whose ids arrived ascending: the root-prefix split on the top 18 bits of the T-form -- moving (top 64
// bits, the bits below, id) --, then every bucket on its own: grouped by a hash of its key bits, only the distinct k-mers ordered (bft_front.hip)
int two_word_split(bft_gpu* h, const LogIn& in, BftPairRun& run, bool& done) {
    const uint64_t total = in.total;
    DevBuf hk, items, hk2, items2, scratch;
    SplitBounds b;
    CK(hk.alloc(total * 8));
    CK(items.alloc(total * sizeof(BftSplit2Val)));
    CK(hk2.alloc(total * 8));
    CK(items2.alloc(total * sizeof(BftSplit2Val)));
    CK(b.alloc(SPLIT_TOP, h->stream));
    const BftSplit2In in2{in.k, in.k + in.stride, in.g, (uint32_t)(2 * h->k - 64)};
    const uint32_t* dbase = nullptr;
    CK((bft_rs::sort<uint64_t, BftSplit2Val, BftSplit2In>(in2, total, hk.as<uint64_t>(), items.as<BftSplit2Val>(), hk2.as<uint64_t>(), items2.as<BftSplit2Val>(), 46u, 64u, h->stream,
                                                          scratch, &dbase)));
    split_bounds(h, hk.as<uint64_t>(), total, 46u, SPLIT_TOP, dbase, 9u, b);
    bft_stage("split (root-prefix, 2 x 9 bits, two-word keys)", (double)total * (20 + 8 + 20 * 4), h->stream);
    hk2.release();
    items2.release();
    uint32_t mx = 0;
    CK(bft_front2_buckets(hk.as<uint64_t>(), items.p, total, b.boff.as<uint32_t>(), 1u << SPLIT_TOP, h->k, h->stream, run, b.maxb.as<uint32_t>(), &mx, &done, &h->front_redone, h->max_gid_seen));
    h->msd_max_bucket = mx;
    return 0;
}
// 2 + 3. the permutation sort by (T, genome), then the flags: on the fly for one-word keys, through flag arrays and two scans for more
int general_sort(bft_gpu* h, const LogIn& in, BftPairRun& run) {
    const int W = h->W;
    const uint64_t total = in.total;
    DevBuf sk, sg;
    CK(sk.alloc(total * W * 8));
    CK(sg.alloc(total * 4));
    CK(bft_sort_pairs(h, in.k, in.stride, in.g, total, sk.as<uint64_t>(), total, sg.as<uint32_t>(), h->log_g_sorted, true));
    // (the insertion log stays until the new image is committed: a failed build loses nothing)
    // 3'. one-word keys: flags on the fly, one 64-bit scan (as on the composite road)
    if (W == 1) return dedupe_w1<uint32_t>(h, sk.as<uint64_t>(), sg.as<uint32_t>(), total, run);
    // 3. flags, scans, compaction
    DevBuf head, keep, posK, posP, tmp;
    CK(head.alloc(total * 4));
    CK(keep.alloc(total * 4));
    CK(posK.alloc(total * 4));
    CK(posP.alloc(total * 4));
    const int grid = bft_grid_for((total + 255) / 256);
    hipLaunchKernelGGL(k_flags, dim3(grid), dim3(256), 0, h->stream, sk.as<uint64_t>(), total, W, sg.as<uint32_t>(), total, head.as<uint32_t>(), keep.as<uint32_t>());
    CK(bft_scan::exclusive_sum_ptr<uint32_t>(head.as<uint32_t>(), posK.as<uint32_t>(), total, h->stream, tmp));
    DevBuf tmp2;  // (a scratch of its own: the first scan may still be running on the stream)
    CK(bft_scan::exclusive_sum_ptr<uint32_t>(keep.as<uint32_t>(), posP.as<uint32_t>(), total, h->stream, tmp2));
    uint32_t lastK[2], lastP[2];
    HIPCK(hipMemcpyAsync(&lastK[0], posK.as<uint32_t>() + total - 1, 4, hipMemcpyDeviceToHost, h->stream));
    HIPCK(hipMemcpyAsync(&lastK[1], head.as<uint32_t>() + total - 1, 4, hipMemcpyDeviceToHost, h->stream));
    HIPCK(hipMemcpyAsync(&lastP[0], posP.as<uint32_t>() + total - 1, 4, hipMemcpyDeviceToHost, h->stream));
    HIPCK(hipMemcpyAsync(&lastP[1], keep.as<uint32_t>() + total - 1, 4, hipMemcpyDeviceToHost, h->stream));
    HIPCK(hipStreamSynchronize(h->stream));
    CK(run_alloc(run, (uint64_t)lastK[0] + lastK[1], (uint64_t)lastP[0] + lastP[1], W));
    hipLaunchKernelGGL(k_scatter, dim3(grid), dim3(256), 0, h->stream, sk.as<uint64_t>(), total, W, sg.as<uint32_t>(), total,
                       head.as<uint32_t>(), keep.as<uint32_t>(), posK.as<uint32_t>(), posP.as<uint32_t>(), run.ids.as<uint32_t>(), run.tk.as<uint64_t>(),
                       run.seg_off.as<uint32_t>());
    return run_close(h, run);
}
}  // namespace

// The roads, top to bottom.  A split road may decline: done = false where a bucket is beyond what its front end sorts (h->msd_max_bucket keeps
// that bucket's size); the road behind it sorts device-wide and cannot.
int bft_make_run(bft_gpu* h, BftPairRun& run) {
    h->front_redone = 0;
    h->msd_max_bucket = 0;
    const LogIn in{h->log_k.as<uint64_t>(), h->log_g.as<uint32_t>(), h->log_cap, h->log_n, h->log_comp ? (int)h->log_gb : bits_for(h->max_gid_seen)};
    if (in.total == 0) return 0;
    const bool split = split_wanted(h, in.total);
    bool done = false;
    if (composite_fits(h, in.gb)) {
        if (split) CK(composite_split(h, in, run, done));
        if (!done) CK(composite_sort(h, in, run));
    } else if (pairs_fit(h, in.gb)) {
        if (split && pairs_split_ok(h, in.gb)) CK(pairs_split(h, in, run, done));
        if (!done) CK(pairs_sort(h, in, run));
    } else {
        if (split && ordered_w2(h)) CK(two_word_split(h, in, run, done));
        if (!done) CK(general_sort(h, in, run));
    }
    return 0;
}
