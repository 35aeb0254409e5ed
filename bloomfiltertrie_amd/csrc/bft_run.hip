// bft_run.hip -- steps 1-3 of the bulk build: the insertion log becomes a run (BftPairRun: sorted distinct T-form k-mers, the offsets of their
// genome-id lists, the ids).  bft_make_run is the list of the roads a log can take, with their fallbacks; every road is a function of its own
// below it, and the conditions that choose among them are plain host functions in bft_run_plan.h (bft_run_road; bft_gpu_debug_run_plan hands them
// to the tests).  Sorts and scans are the library's own (bft_sort.h, bft_scan.h); the buckets behind the root-prefix split are
// bft_front.hip's; the kernels launched here are bft_kernels_build.h's.  bft_sort_pairs, the general permutation sort, is also what
// bft_ensure_table and the sub-graph build order their records with.  See DESIGN.md "Insertion".  At the end: the sort and scan test hooks, in the
// unit that instantiates the library's sorts anyway.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "bft_front.h"
#include "bft_handle.h"
#include "bft_paths.h"  // BftSpHead (bft_gpu_test_scan_ex)
#include "bft_run_plan.h"
#include "bft_scan.h"
#include "bft_sort.h"

#include "bft_kernels_build.h"

// What the log looks like to the library's sort and scan: the input functors of bft_rs::sort / bft_scan::exclusive_sum that read it (the test hooks at
// the end run the same instantiations).
// ---- composite path: one-word keys whose genome ids arrive in ascending order and fit the key's spare low bits ----------------
// c = (T << gb) | genome: ONE 8-byte array is sorted (on the T bits only: the sort is stable, so the ids keep their ascending
// order inside a k-mer) instead of 8-byte keys + 4-byte values -- a third less traffic in each of the seven radix passes -- and the
// de-duplication flags come out of neighbouring composites on the fly instead of through two flag arrays and two scans.
struct BftCompose {  // input "iterator" of the sort: composite i from the insertion log
    const uint64_t* k;
    const uint32_t* g;
    uint32_t gb;
    __host__ __device__ uint64_t operator()(uint32_t i) const { return g ? (k[i] << gb) | (uint64_t)g[i] : k[i]; }  // (g == NULL: the log already holds composites)
    __device__ uint64_t key(uint32_t i) const { return (*this)(i); }  // (as the input of bft_rs::sort)
    __device__ bft_rs::NoVal val(uint32_t) const { return bft_rs::NoVal{}; }
};
// two-word keys: what the root-prefix split moves -- the top 64 bits of the T-form (left-aligned: their top 18 bits are the root prefix) as the
// key, the bits below them and the genome id as the value (bft_front.hip: BftItem2)
struct __attribute__((packed, aligned(4))) BftSplit2Val {
    uint64_t lo;
    uint32_t id;
};
struct BftSplit2In {
    const uint64_t* k0;  // word 0 (most significant), word 1 of the log
    const uint64_t* k1;
    const uint32_t* g;
    uint32_t sh;  // 2k - 64: the bits of word 1 that belong to the T-form's low part once the top 64 are taken (2 .. 64)
    __device__ uint64_t key(uint32_t i) const { return sh == 64 ? k0[i] : (k0[i] << (64 - sh)) | (k1[i] >> sh); }
    __device__ BftSplit2Val val(uint32_t i) const {
        BftSplit2Val v;
        v.lo = sh == 64 ? k1[i] : (k1[i] & ((1ull << sh) - 1ull));
        v.id = g[i];
        return v;
    }
};
template <class GT>
struct BftPairIn {  // input of the sorts that move (k-mer, id) pairs: the log's k-mers, its ids narrowed to GT
    const uint64_t* k;
    const uint32_t* g;
    __device__ uint64_t key(uint32_t i) const { return k[i]; }
    __device__ GT val(uint32_t i) const { return (GT)g[i]; }
};
struct BftPairFlags {  // input of the scan: (first pair of its k-mer) << 32 | (first pair of its (k-mer, genome))
    const uint64_t* c;
    uint32_t gb;
    __host__ __device__ uint64_t operator()(uint32_t i) const {
        const uint64_t a = c[i], b = i ? c[i - 1] : ~a;
        const uint64_t head = (a >> gb) != (b >> gb), keep = a != b;
        return (head << 32) | keep;
    }
};

thread_local bft_rs::RunRecord bft_rs::g_bft_rs_last;  // what this thread's last library sort ran (test hooks: bft_gpu_test_sort_last)
int bft_rs::g_bft_rs_rank_mode = -1;  // how bft_sort.h ranks: 0 LDS atomics (lane order checked on the device), 1 ballots ("sort_ballots")

static int bits_for(uint64_t v) { return bft_run_id_bits(v); }

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
    if (is_log && !h->lb_end.empty() && h->lb_end.size() <= BFT_RUN_CALL_TABLE_MAX && h->lb_end.back() == total) {
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

// ---- which road: every condition once, in bft_run_plan.h (plain values in; bft_make_run hands it the handle's) -----------------------------------
constexpr int SPLIT_TOP = BFT_RUN_SPLIT_TOP;
unsigned split_top(const bft_gpu* h) { return bft_run_split_top(h->k); }

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
    const uint32_t vw = bft_run_id_width(h->max_gid_seen);
    if (vw == 1) return split_dedupe_w1<uint8_t>(h, in, run, done);
    if (vw == 2) return split_dedupe_w1<uint16_t>(h, in, run, done);
    return split_dedupe_w1<uint32_t>(h, in, run, done);
}
// 2n + 3'. one key + value sort over every bit with the ids narrowed to one or two bytes (the values are a third of
// the sort's traffic at four), flags on the fly, one scan
int pairs_sort(bft_gpu* h, const LogIn& in, BftPairRun& run) {
    const uint32_t vw = bft_run_id_width(h->max_gid_seen);
    if (vw == 1) return sort_dedupe_w1_narrow<uint8_t>(h, in, run);
    if (vw == 2) return sort_dedupe_w1_narrow<uint16_t>(h, in, run);
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
    const BftRunRoad road = bft_run_road(h->k, h->W, h->log_g_sorted, !h->opt_no_composite, h->opt_msd, h->max_gid_seen, in.gb, in.total);
    std::copy(road.v, road.v + 4, h->run_road);
    const bool split = road.v[3] != 0;
    bool done = false;
    if (road.v[0] == 1u) {
        if (split) CK(composite_split(h, in, run, done));
        if (!done) CK(composite_sort(h, in, run));
    } else if (road.v[0] == 2u) {
        if (split) CK(pairs_split(h, in, run, done));
        if (!done) CK(pairs_sort(h, in, run));
    } else {
        if (split) CK(two_word_split(h, in, run, done));
        if (!done) CK(general_sort(h, in, run));
    }
    return 0;
}

// Test hook (tests/test_run_cases_host.py): the rules of bft_run_plan.h without a handle or a device, for a log of `total` pairs of k-mers of length k
// whose ids ascend (ids_ordered) or not, under "build_composite", "build_msd" and "composite_log"; max_gid: the largest id the handle has seen,
// log_max_gid: the largest id of this log (they differ behind an earlier build).  out = {what bft_gpu_debug_run_road reports [0..3]; the id bits of a
// composite log of such a handle (0: k-mers + ids are logged); 1 when the log is still one of composites at build time; the threads of a capped
// bft_grid_for grid of 256-thread workgroups; the largest table of insert calls the multi-word sort reads ids from}.
extern "C" int bft_gpu_debug_run_plan(int k, int ids_ordered, int build_composite, int build_msd, int composite_log, uint32_t max_gid, uint32_t log_max_gid, uint64_t total,
                                      uint32_t out[8]) {
    if (!out || k < 9 || k > 126 || build_msd < 0 || build_msd > 2 || log_max_gid > max_gid || total == 0) return bft_fail(BFT_GPU_E_ARG, "run plan: argument");
    const int W = (2 * k + 63) / 64;
    const bool ordered = ids_ordered != 0, composite = build_composite != 0;
    const uint32_t log_gb = bft_run_log_comp_bits(k, W, composite_log != 0, composite);
    const bool comp = log_gb != 0 && bft_run_log_holds_id(log_gb, log_max_gid) && bft_run_log_stays_composite(ordered, composite);
    const BftRunRoad road = bft_run_road(k, W, ordered, composite, build_msd, max_gid, comp ? (int)log_gb : bft_run_id_bits(max_gid), total);
    out[0] = road.v[0] - 1;
    for (int i = 1; i < 4; i++) out[i] = road.v[i];
    out[4] = log_gb;
    out[5] = comp;
    out[6] = (uint32_t)bft_grid_for(~0ull) * 256u;
    out[7] = BFT_RUN_CALL_TABLE_MAX;
    return BFT_GPU_OK;
}

// Test hook (tests/test_gpu_front_edges.py): the road the last build's sort took.  out = {0 composites T << gb | id, 1 (k-mer, id) pairs of ordered
// one-word keys, 2 whatever is left (two-word keys, ids out of order, "build_composite" 0); gb, the bits of an id; the bytes of an id beside the keys
// (0: composites); 1 when the root-prefix split was tried}.  BFT_GPU_E_ARG for NULL or a handle that has not sorted yet.
extern "C" int bft_gpu_debug_run_road(bft_gpu* h, uint32_t out[4]) {
    if (!h || !out || h->run_road[0] == 0) return bft_fail(BFT_GPU_E_ARG, "run road: NULL argument or no build yet");
    out[0] = h->run_road[0] - 1;
    for (int i = 1; i < 4; i++) out[i] = h->run_road[i];
    return BFT_GPU_OK;
}

// ------------------------------------------------------------------------------------------------
// test hooks (tests/test_gpu_sort_scan.py; not part of include/bft_gpu.h): the library's own sort and scan on the caller's device arrays
// ------------------------------------------------------------------------------------------------
// kind 0: u64 keys; 1: u64 keys + u32 values; 2: u32 keys + u32 values.  shape: bft_rs::SHAPE_*.  Stable LSD over the bits [begin_bit, end_bit).
extern "C" int bft_gpu_test_sort(int kind, int shape, const void* d_keys, const void* d_vals, uint64_t n, unsigned begin_bit, unsigned end_bit, void* d_out_keys, void* d_out_vals,
                                 void* hip_stream) {
    if ((!d_keys || !d_out_keys) && n) return bft_fail(BFT_GPU_E_ARG, "NULL argument");
    hipStream_t s = (hipStream_t)hip_stream;
    int dev = 0;
    HIPCK(hipGetDevice(&dev));
    bft_pool_set_stream(dev, s);
    int rc = BFT_GPU_E_ARG;
#define BFT_TS(K, V, SH) rc = bft_rs::sort_pairs<K, V, SH>((const K*)d_keys, (const V*)d_vals, n, (K*)d_out_keys, (V*)d_out_vals, begin_bit, end_bit, s)
    if (kind == 0) {
        rc = bft_rs::sort_keys<uint64_t>((const uint64_t*)d_keys, n, (uint64_t*)d_out_keys, begin_bit, end_bit, s);
    } else if (kind == 1) {
        if (shape == bft_rs::SHAPE_LIGHT) BFT_TS(uint64_t, uint32_t, bft_rs::SHAPE_LIGHT);
        else if (shape == bft_rs::SHAPE_BACK) BFT_TS(uint64_t, uint32_t, bft_rs::SHAPE_BACK);
        else BFT_TS(uint64_t, uint32_t, bft_rs::SHAPE_BIG);
    } else if (kind == 2) {
        if (shape == bft_rs::SHAPE_LIGHT) BFT_TS(uint32_t, uint32_t, bft_rs::SHAPE_LIGHT);
        else if (shape == bft_rs::SHAPE_BACK) BFT_TS(uint32_t, uint32_t, bft_rs::SHAPE_BACK);
        else BFT_TS(uint32_t, uint32_t, bft_rs::SHAPE_BIG);
    }
#undef BFT_TS
    if (rc) return rc;
    HIPCK(hipStreamSynchronize(s));
    return BFT_GPU_OK;
}
// kind 0: exclusive sum of u32 (out[n] = the total as well); 1: exclusive sum of u64 (likewise); 2: inclusive max of u64, init 5.  *d_total: the grand total.
// reps scans in a row share one scratch block (nothing is zeroed between them: bft_scan.h).
extern "C" int bft_gpu_test_scan(int kind, const void* d_in, uint64_t n, void* d_out, void* d_total, int reps, void* hip_stream) {
    if ((!d_in || !d_out) && n) return bft_fail(BFT_GPU_E_ARG, "NULL argument");
    hipStream_t s = (hipStream_t)hip_stream;
    int dev = 0;
    HIPCK(hipGetDevice(&dev));
    bft_pool_set_stream(dev, s);
    DevBuf scratch;
    for (int r = 0; r < std::max(1, reps); r++) {
        if (kind == 0) CK(bft_scan::exclusive_sum_ptr<uint32_t>((const uint32_t*)d_in, (uint32_t*)d_out, n, s, scratch, (unsigned long long*)d_total, true));
        else if (kind == 1) CK(bft_scan::exclusive_sum_ptr<uint64_t>((const uint64_t*)d_in, (uint64_t*)d_out, n, s, scratch, (unsigned long long*)d_total, true));
        else if (kind == 2)
            CK((bft_scan::scan<uint64_t, bft_scan::PtrIn<uint64_t>, bft_scan::Max, true>(bft_scan::PtrIn<uint64_t>{(const uint64_t*)d_in}, (uint64_t*)d_out, n, 5ull, bft_scan::Max(), s, scratch,
                                                                                          (unsigned long long*)d_total)));
        else return bft_fail(BFT_GPU_E_ARG, "bad scan kind");
    }
    HIPCK(hipStreamSynchronize(s));
    return BFT_GPU_OK;
}

// Every (key, value, input) the library sorts (tests/test_gpu_sort_scan_edges.py).  kind: 0 u64 keys; 1 u64 + u32; 2 u32 + u32; 3 u32 + u64 (the
// genome-id pass); 4 u64 keys through BftCompose (d_vals NULL: the keys as they are, else (key << param) | id[i]); 5 / 6 u64 + u8 / u16 through
// BftPairIn (d_vals: u32 ids, narrowed); 7 u64 + BftSplit2Val through BftSplit2In (d_keys: word 0; d_vals: word 1 [n] (u64), then the ids [n]
// (u32); param: sh, 0 = 64); 8 .. 11: u32 + KhRec<W>, W = kind - 7 (d_vals: the packed records).  The shapes each kind is built in:
// bft_gpu_test_sort_tile != 0.  h_dbase (NULL or 512 words): the sort's last_dbase table, where it made one.
#define BFT_TSX_KINDS(X)                                                                                        \
    X(0, SHAPE_BIG, uint64_t, bft_rs::NoVal, (bft_rs::PtrIn<uint64_t, bft_rs::NoVal>{(const uint64_t*)d_keys, nullptr}))                 \
    X(1, SHAPE_BIG, uint64_t, uint32_t, (bft_rs::PtrIn<uint64_t, uint32_t>{(const uint64_t*)d_keys, (const uint32_t*)d_vals}))           \
    X(1, SHAPE_LIGHT, uint64_t, uint32_t, (bft_rs::PtrIn<uint64_t, uint32_t>{(const uint64_t*)d_keys, (const uint32_t*)d_vals}))         \
    X(1, SHAPE_BACK, uint64_t, uint32_t, (bft_rs::PtrIn<uint64_t, uint32_t>{(const uint64_t*)d_keys, (const uint32_t*)d_vals}))          \
    X(2, SHAPE_BIG, uint32_t, uint32_t, (bft_rs::PtrIn<uint32_t, uint32_t>{(const uint32_t*)d_keys, (const uint32_t*)d_vals}))           \
    X(2, SHAPE_LIGHT, uint32_t, uint32_t, (bft_rs::PtrIn<uint32_t, uint32_t>{(const uint32_t*)d_keys, (const uint32_t*)d_vals}))         \
    X(2, SHAPE_BACK, uint32_t, uint32_t, (bft_rs::PtrIn<uint32_t, uint32_t>{(const uint32_t*)d_keys, (const uint32_t*)d_vals}))          \
    X(3, SHAPE_BIG, uint32_t, uint64_t, (bft_rs::PtrIn<uint32_t, uint64_t>{(const uint32_t*)d_keys, (const uint64_t*)d_vals}))           \
    X(4, SHAPE_BIG, uint64_t, bft_rs::NoVal, (BftCompose{(const uint64_t*)d_keys, (const uint32_t*)d_vals, param}))                      \
    X(5, SHAPE_BIG, uint64_t, uint8_t, (BftPairIn<uint8_t>{(const uint64_t*)d_keys, (const uint32_t*)d_vals}))                           \
    X(6, SHAPE_BIG, uint64_t, uint16_t, (BftPairIn<uint16_t>{(const uint64_t*)d_keys, (const uint32_t*)d_vals}))                         \
    X(7, SHAPE_BIG, uint64_t, BftSplit2Val, (BftSplit2In{(const uint64_t*)d_keys, (const uint64_t*)d_vals, (const uint32_t*)((const uint64_t*)d_vals + n), param ? param : 64u}))
extern "C" int bft_gpu_test_sort_ex(int kind, int shape, const void* d_keys, const void* d_vals, uint64_t n, unsigned begin_bit, unsigned end_bit, void* d_out_keys, void* d_out_vals,
                                    uint32_t param, uint32_t* h_dbase, void* hip_stream) {
    if (n && (!d_keys || !d_out_keys || (kind != 0 && kind != 4 && (!d_vals || !d_out_vals)))) return bft_fail(BFT_GPU_E_ARG, "NULL argument");
    if (kind == 7 && param > 64) return bft_fail(BFT_GPU_E_ARG, "test sort: sh");
    hipStream_t s = (hipStream_t)hip_stream;
    int dev = 0;
    HIPCK(hipGetDevice(&dev));
    bft_pool_set_stream(dev, s);
    if (kind >= 8 && kind <= 11) return bft_kh_test_sort(kind - 7, shape, (const uint32_t*)d_keys, d_vals, n, begin_bit, end_bit, (uint32_t*)d_out_keys, d_out_vals, s, h_dbase);
#define BFT_TSX(KIND, SH, K, V, IN)                                                                                                                               \
    if (kind == KIND && shape == bft_rs::SH) {                                                                                                                    \
        auto in = IN;  /* (not const: the In type of the product's own instantiations) */                                                                       \
        return bft_rs::sort_test_run<K, V, decltype(in), bft_rs::SH>(in, n, (K*)d_out_keys, (V*)d_out_vals, begin_bit, end_bit, s, h_dbase);                     \
    }
    BFT_TSX_KINDS(BFT_TSX)
#undef BFT_TSX
    return bft_fail(BFT_GPU_E_ARG, "test sort: kind / shape");
}
// entries per tile of bft_gpu_test_sort_ex(kind, shape) (the one-tile / ranged boundary); 0: that kind is not built in that shape
extern "C" uint32_t bft_gpu_test_sort_tile(int kind, int shape) {
    const void *d_keys = nullptr, *d_vals = nullptr;
    const uint64_t n = 0;
    const uint32_t param = 0;
    if (kind >= 8 && kind <= 11) return bft_kh_test_sort_tile(kind - 7, shape);
#define BFT_TSX(KIND, SH, K, V, IN)                                                                                                                               \
    if (kind == KIND && shape == bft_rs::SH) {                                                                                                                    \
        (void)IN;                                                                                                                                                 \
        return bft_rs::tile_entries<K, V, bft_rs::SH>();                                                                                                          \
    }
    BFT_TSX_KINDS(BFT_TSX)
#undef BFT_TSX
    return 0u;
}
#undef BFT_TSX_KINDS
// what the last library sort of the calling thread ran: [0] regime (0 copy, 1 one tile, 2 ranged, 3 chained, 255 nothing), [1] passes, [2] tiles,
// [3] ranges, [4] tiles per range, [5] entries per tile, [6..7] 0; then per pass p < 8, words 8 + 4 p ..: first bit, bits, chains (0: a ranged
// pass), look-back groups launched (1 or THREADS / 128; 0: a ranged pass).  Returns the words written.
extern "C" int bft_gpu_test_sort_last(uint64_t* out, int n) {
    if (!out || n < 0) return bft_fail(BFT_GPU_E_ARG, "NULL argument");
    const bft_rs::RunRecord& r = bft_rs::g_bft_rs_last;
    uint64_t w[8 + 4 * bft_rs::MAXP] = {r.regime, r.P, r.tiles, r.ranges, r.tpr, r.tile, 0, 0};
    for (int p = 0; p < bft_rs::MAXP; p++) {
        w[8 + 4 * p] = r.bit[p];
        w[9 + 4 * p] = r.nbits[p];
        w[10 + 4 * p] = r.nch[p];
        w[11 + 4 * p] = r.lbg[p];
    }
    const int m = std::min<int>(n, (int)(sizeof(w) / 8));
    for (int i = 0; i < m; i++) out[i] = w[i];
    return m;
}

// one scan of bft_gpu_test_scan_ex's kinds: 0 exclusive sum of u32; 1 of u64; 2 inclusive max of u64 from init = param; 3 exclusive sum (u64) of
// BftPairFlags over u64 composites (d_in; gb = param), as the build numbers its k-mers and pairs; 4 exclusive sum (u32) of BftSpHead over uint2
// (d_in), as the simple paths are numbered
static int test_scan_one(int kind, const void* d_in, uint64_t n, void* d_out, void* d_total, bool tail, uint64_t param, hipStream_t s, DevBuf& scratch) {
    unsigned long long* tot = (unsigned long long*)d_total;
    switch (kind) {
    case 0: return bft_scan::exclusive_sum_ptr<uint32_t>((const uint32_t*)d_in, (uint32_t*)d_out, n, s, scratch, tot, tail);
    case 1: return bft_scan::exclusive_sum_ptr<uint64_t>((const uint64_t*)d_in, (uint64_t*)d_out, n, s, scratch, tot, tail);
    case 2:
        return bft_scan::scan<uint64_t, bft_scan::PtrIn<uint64_t>, bft_scan::Max, true>(bft_scan::PtrIn<uint64_t>{(const uint64_t*)d_in}, (uint64_t*)d_out, n, param, bft_scan::Max(), s,
                                                                                         scratch, tot, tail);
    case 3: return bft_scan::exclusive_sum<uint64_t>(BftPairFlags{(const uint64_t*)d_in, (uint32_t)param}, (uint64_t*)d_out, n, s, scratch, tot, tail);
    case 4: return bft_scan::exclusive_sum<uint32_t>(BftSpHead{(const uint2*)d_in, n}, (uint32_t*)d_out, n, s, scratch, tot, tail);
    default: return bft_fail(BFT_GPU_E_ARG, "bad scan kind");
    }
}
// one scan (kinds: test_scan_one) on a block of its own; tail: out[n] receives the total as well (else it is not written)
extern "C" int bft_gpu_test_scan_ex(int kind, const void* d_in, uint64_t n, void* d_out, void* d_total, int tail, uint64_t param, void* hip_stream) {
    if ((!d_in || !d_out) && n) return bft_fail(BFT_GPU_E_ARG, "NULL argument");
    hipStream_t s = (hipStream_t)hip_stream;
    int dev = 0;
    HIPCK(hipGetDevice(&dev));
    bft_pool_set_stream(dev, s);
    DevBuf scratch;
    CK(test_scan_one(kind, d_in, n, d_out, d_total, tail != 0, param, s, scratch));
    HIPCK(hipStreamSynchronize(s));
    return BFT_GPU_OK;
}
// count scans one after the other on ONE scratch block, as the library's long-lived blocks are used: scan i reads d_in[0 .. sizes[i]) and writes
// h_outs[i] (sizes[i] + 1 entries: with the total behind them) and d_totals[i] (u64)
extern "C" int bft_gpu_test_scan_seq(int kind, const void* d_in, const uint64_t* sizes, int count, void* const* h_outs, uint64_t* d_totals, uint64_t param, void* hip_stream) {
    if (!d_in || !sizes || !h_outs || !d_totals || count < 0) return bft_fail(BFT_GPU_E_ARG, "NULL argument");
    hipStream_t s = (hipStream_t)hip_stream;
    int dev = 0;
    HIPCK(hipGetDevice(&dev));
    bft_pool_set_stream(dev, s);
    DevBuf scratch;
    for (int i = 0; i < count; i++) CK(test_scan_one(kind, d_in, sizes[i], h_outs[i], d_totals + i, true, param, s, scratch));
    HIPCK(hipStreamSynchronize(s));
    return BFT_GPU_OK;
}
// The contract of bft_scan.h: a sort that writes a scan's scratch block sets its tag to 0.  An exclusive u32 sum of d_in[0 .. n_scan) into d_out1,
// a sort of the u64 keys d_keys[0 .. n_sort) on [0, 64) into d_sorted with the same block as its scratch, and -- only when the sort left tag == 0 --
// the same scan again into d_out2.  info: {tag after the sort, block bytes before the sort, after it}.  BFT_GPU_E_STATE: the sort left a tag the
// second scan would have trusted (it would have claimed tiles from the sort's words).
extern "C" int bft_gpu_test_scan_sort_scan(const uint32_t* d_in, uint64_t n_scan, const uint64_t* d_keys, uint64_t n_sort, uint32_t* d_out1, uint32_t* d_out2, uint64_t* d_sorted,
                                           uint64_t* info, void* hip_stream) {
    if (!d_in || !d_keys || !d_out1 || !d_out2 || !d_sorted || !info) return bft_fail(BFT_GPU_E_ARG, "NULL argument");
    hipStream_t s = (hipStream_t)hip_stream;
    int dev = 0;
    HIPCK(hipGetDevice(&dev));
    bft_pool_set_stream(dev, s);
    DevBuf scratch, tk;
    CK(tk.alloc(std::max<uint64_t>(n_sort, 1) * 8));
    CK(bft_scan::exclusive_sum_ptr<uint32_t>(d_in, d_out1, n_scan, s, scratch, nullptr, true));
    info[1] = scratch.bytes;
    CK((bft_rs::sort<uint64_t, bft_rs::NoVal, bft_rs::PtrIn<uint64_t, bft_rs::NoVal>>(bft_rs::PtrIn<uint64_t, bft_rs::NoVal>{d_keys, nullptr}, n_sort, (uint64_t*)d_sorted,
                                                                                      (bft_rs::NoVal*)nullptr, tk.as<uint64_t>(), (bft_rs::NoVal*)nullptr, 0u, 64u, s, scratch)));
    info[0] = scratch.tag;
    info[2] = scratch.bytes;
    if (scratch.tag != 0) {
        HIPCK(hipStreamSynchronize(s));
        return bft_fail(BFT_GPU_E_STATE, "the sort wrote the scan's scratch block and left its tag");
    }
    CK(bft_scan::exclusive_sum_ptr<uint32_t>(d_in, d_out2, n_scan, s, scratch, nullptr, true));
    HIPCK(hipStreamSynchronize(s));
    return BFT_GPU_OK;
}
