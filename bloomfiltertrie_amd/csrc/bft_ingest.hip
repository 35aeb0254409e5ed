// bft_ingest.hip -- insertion from sequences: bft_gpu_insert_sequences / _dev / bft_gpu_insert_sequence_file (an extension; the reference inserts k-mers
// that a counter has cut out of the genomes beforehand).  The sequence queries' front end -- k_seq_encode, k_seq_plan, k_seq_tiles
// (bft_kernels_seqenc.h), seq_window (bft_kernels_seqwin.h) -- connected to the insertion log (bft_log_prepare / bft_log_commit, bft_handle.h):
//   stream path (min_abundance == 0)
//     k_ing_count        one wavefront per tile of BFT_ING_TILE positions: the windows without a character outside ACGTU, counted (__ballot, __popcll);
//                        only the "bad" bit stream is read
//     (scan of the counts: the tiles' offsets and the total, which the host waits for -- the log's row count must be exact)
//     k_ing_write        the tiles again: window -> canonical form -> T-form -> row log_n + offset of the tile + valid lanes below, written as
//                        k_pack_to_tform writes it (T-form words + id, or the composite T << cgb | id): no packed k-mer array in between, no hole
//   counting path (min_abundance >= 1)
//     the same two kernels with a scratch array as the target, the library's radix sort over all 2k bits (one word per pass from the least
//     significant word, the permutation carried as the value, as the build sorts multi-word keys), then
//     k_ing_runs_count   a row heads a run when it differs from the row before; it is kept when row + min_abundance - 1 still holds the same key
//                        (the array is sorted: O(1) per row whatever the run's length, nothing carried between wavefronts or tiles)
//     k_ing_runs_write   the kept heads compacted into the log
// Per position the stream path reads ~1 byte of ASCII (+ 3 bits of the code and "bad" streams written once and read twice) and writes 8 W bytes.
#include "bft_ingest.h"

#include <vector>

#include "bft_dev.h"
#include "bft_handle.h"
#include "bft_kernels_seqwin.h"
#include "bft_scan.h"
#include "bft_seqfile.h"
#include "bft_sort.h"
#include "bft_walk.h"

#define BFT_MAX_GENOME_ID (1u << 24)  // (bft_gpu.hip)

namespace {

#include "bft_kernels_seqenc.h"

constexpr int ING_THREADS = 256;
constexpr int ING_WAVES = ING_THREADS / 64;
static_assert(BFT_ING_TILE == 64, "a tile is what one wavefront ballots");

__device__ __forceinline__ uint64_t lanes_below(uint32_t lane) { return lane ? (~0ull >> (64 - lane)) : 0ull; }

// seq_window's validity test alone: none of the k "bad" bits from character c0 on is set
__device__ __forceinline__ bool ing_window_ok(const uint32_t* __restrict__ bad, uint64_t c0, int k) {
    const uint64_t w0 = c0 >> 5;
    const uint32_t bs = (uint32_t)(c0 & 31u);
    int left = k;
    uint32_t first = bad[w0] >> bs;
    if (left < 32 - (int)bs) first &= (1u << left) - 1u;
    bool ok = first == 0;
    left -= 32 - (int)bs;
    for (uint64_t j = w0 + 1; left > 0; j++, left -= 32) {
        uint32_t m = bad[j];
        if (left < 32) m &= (1u << left) - 1u;
        ok = ok && m == 0;
    }
    return ok;
}

// the first character of position p (p < pos_off[n_seqs]): its sequence from the tile table, stepping over sequences without a position
__device__ __forceinline__ uint64_t ing_char_of(const uint64_t* __restrict__ seq_off, const uint64_t* __restrict__ pos_off, const uint32_t* __restrict__ tile_seq,
                                                uint32_t n_seqs, uint64_t p) {
    uint32_t lo = tile_seq[p >> 6];
    while (lo + 1 < n_seqs && pos_off[lo + 1] <= p) lo++;
    return seq_off[lo] + (p - pos_off[lo]);
}

// Tiles [0, ntiles) of the positions [p0, p1) (p0 a multiple of the tile; positions at or beyond the batch's total count as invalid).
__global__ __launch_bounds__(ING_THREADS) void k_ing_count(const uint32_t* __restrict__ bad, const uint64_t* __restrict__ seq_off, const uint64_t* __restrict__ pos_off,
                                                           const uint32_t* __restrict__ tile_seq, uint32_t n_seqs, int k, uint64_t p0, uint64_t p1, uint64_t ntiles,
                                                           uint32_t* __restrict__ cnt) {
    const uint64_t P = min(pos_off[n_seqs], p1);
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t t = (uint64_t)blockIdx.x * ING_WAVES + (threadIdx.x >> 6); t < ntiles; t += (uint64_t)gridDim.x * ING_WAVES) {
        const uint64_t p = p0 + t * BFT_ING_TILE + lane;
        const bool v = p < P && ing_window_ok(bad, ing_char_of(seq_off, pos_off, tile_seq, n_seqs, p), k);
        const uint64_t m = __ballot(v);
        if (lane == 0) cnt[t] = (uint32_t)__popcll(m);
    }
}

// A row of the log (or of the counting path's key array: gout == nullptr, cgb == 0), as k_pack_to_tform writes it.
template <int W>
__device__ __forceinline__ void ing_store(const uint64_t* t, uint64_t* __restrict__ out, uint64_t stride, uint64_t dst, uint32_t* __restrict__ gout, uint32_t gid,
                                          uint32_t cgb) {
    if (W == 1 && cgb) {
        out[dst] = (t[0] << cgb) | (uint64_t)gid;
        return;
    }
#pragma unroll
    for (int w = 0; w < W; w++) out[(uint64_t)w * stride + dst] = t[w];
    if (gout) gout[dst] = gid;
}

template <int W>
__global__ __launch_bounds__(ING_THREADS) void k_ing_write(const uint64_t* __restrict__ codes, const uint32_t* __restrict__ bad, const uint64_t* __restrict__ seq_off,
                                                           const uint64_t* __restrict__ pos_off, const uint32_t* __restrict__ tile_seq, uint32_t n_seqs, int k,
                                                           int canonical, uint64_t p0, uint64_t p1, uint64_t ntiles, const uint32_t* __restrict__ toff,
                                                           uint64_t* __restrict__ out, uint64_t stride, uint64_t base, uint32_t* __restrict__ gout, uint32_t gid,
                                                           uint32_t cgb) {
    const uint64_t P = min(pos_off[n_seqs], p1);
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t t = (uint64_t)blockIdx.x * ING_WAVES + (threadIdx.x >> 6); t < ntiles; t += (uint64_t)gridDim.x * ING_WAVES) {
        const uint64_t p = p0 + t * BFT_ING_TILE + lane;
        uint64_t x[W], tf[W];
        // (k as this turn's own value: the shifts and masks that the window and the T-form derive from it -- all wavefront-uniform -- are then
        // computed where they are used instead of being kept in scalar registers across the loop, where W >= 2 ran out of them)
        int kk = k;
        asm volatile("" : "+s"(kk));
        const bool v = p < P && seq_window<W>(codes, bad, ing_char_of(seq_off, pos_off, tile_seq, n_seqs, p), kk, canonical, x);
        const uint64_t m = __ballot(v);
        if (!v) continue;
        bft_tform_from_x<W>(x, kk, tf);
        ing_store<W>(tf, out, stride, base + toff[t] + (uint64_t)__popcll(m & lanes_below(lane)), gout, gid, cgb);
    }
}

__global__ void k_ing_iota(uint32_t* __restrict__ p, uint64_t n) {
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) p[i] = (uint32_t)i;
}
__global__ void k_ing_gather(const uint64_t* __restrict__ in, const uint32_t* __restrict__ perm, uint64_t* __restrict__ out, uint64_t n) {
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) out[i] = in[perm[i]];
}

template <int W>
__device__ __forceinline__ bool ing_rows_equal(const uint64_t* __restrict__ keys, uint64_t stride, uint64_t a, uint64_t b) {
    bool eq = true;
#pragma unroll
    for (int w = 0; w < W; w++) eq = eq && keys[(uint64_t)w * stride + a] == keys[(uint64_t)w * stride + b];
    return eq;
}
// head: row i starts a run of the sorted keys; kept: the run is at least c rows long (row i + c - 1 still holds the key)
template <int W>
__device__ __forceinline__ void ing_run_flags(const uint64_t* __restrict__ keys, uint64_t stride, uint64_t n, uint64_t c, uint64_t i, bool* head, bool* kept) {
    *head = i < n && (i == 0 || !ing_rows_equal<W>(keys, stride, i, i - 1));
    *kept = *head && c - 1 < n - i && ing_rows_equal<W>(keys, stride, i, i + (c - 1));
}
template <int W>
__global__ __launch_bounds__(ING_THREADS) void k_ing_runs_count(const uint64_t* __restrict__ keys, uint64_t stride, uint64_t n, uint64_t c, uint64_t ntiles,
                                                                uint32_t* __restrict__ cnt, unsigned long long* __restrict__ distinct) {
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t t = (uint64_t)blockIdx.x * ING_WAVES + (threadIdx.x >> 6); t < ntiles; t += (uint64_t)gridDim.x * ING_WAVES) {
        bool head, kept;
        ing_run_flags<W>(keys, stride, n, c, t * BFT_ING_TILE + lane, &head, &kept);
        const uint64_t mh = __ballot(head), mk = __ballot(kept);
        if (lane == 0) {
            cnt[t] = (uint32_t)__popcll(mk);
            if (mh) atomicAdd(distinct, (unsigned long long)__popcll(mh));
        }
    }
}
template <int W>
__global__ __launch_bounds__(ING_THREADS) void k_ing_runs_write(const uint64_t* __restrict__ keys, uint64_t stride, uint64_t n, uint64_t c, uint64_t ntiles,
                                                                const uint32_t* __restrict__ toff, uint64_t* __restrict__ out, uint64_t ostride, uint64_t base,
                                                                uint32_t* __restrict__ gout, uint32_t gid, uint32_t cgb) {
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t t = (uint64_t)blockIdx.x * ING_WAVES + (threadIdx.x >> 6); t < ntiles; t += (uint64_t)gridDim.x * ING_WAVES) {
        const uint64_t i = t * BFT_ING_TILE + lane;
        bool head, kept;
        ing_run_flags<W>(keys, stride, n, c, i, &head, &kept);
        const uint64_t mk = __ballot(kept);
        if (!kept) continue;
        uint64_t tf[W];
#pragma unroll
        for (int w = 0; w < W; w++) tf[w] = keys[(uint64_t)w * stride + i];
        ing_store<W>(tf, out, ostride, base + toff[t] + (uint64_t)__popcll(mk & lanes_below(lane)), gout, gid, cgb);
    }
}

int tile_grid(uint64_t ntiles) { return bft_grid_for((ntiles + ING_WAVES - 1) / ING_WAVES); }

// ---- launches, per key width ----
struct IngPlan {  // the plan of one batch of sequences on the device
    const uint64_t *codes, *seq_off, *pos_off;
    const uint32_t *bad, *tile_seq;
    uint32_t n_seqs;
};
template <int W>
int launch_write(const IngPlan& pl, int k, int canonical, uint64_t p0, uint64_t p1, uint64_t ntiles, const uint32_t* toff, uint64_t* out, uint64_t stride, uint64_t base,
                 uint32_t* gout, uint32_t gid, uint32_t cgb, hipStream_t s) {
    hipLaunchKernelGGL(k_ing_write<W>, dim3(tile_grid(ntiles)), dim3(ING_THREADS), 0, s, pl.codes, pl.bad, pl.seq_off, pl.pos_off, pl.tile_seq, pl.n_seqs, k, canonical, p0, p1,
                       ntiles, toff, out, stride, base, gout, gid, cgb);
    HIPCK(hipGetLastError());
    return 0;
}
int ing_write(int W, const IngPlan& pl, int k, int canonical, uint64_t p0, uint64_t p1, uint64_t ntiles, const uint32_t* toff, uint64_t* out, uint64_t stride, uint64_t base,
              uint32_t* gout, uint32_t gid, uint32_t cgb, hipStream_t s) {
    switch (W) {
    case 1: return launch_write<1>(pl, k, canonical, p0, p1, ntiles, toff, out, stride, base, gout, gid, cgb, s);
    case 2: return launch_write<2>(pl, k, canonical, p0, p1, ntiles, toff, out, stride, base, gout, gid, cgb, s);
    case 3: return launch_write<3>(pl, k, canonical, p0, p1, ntiles, toff, out, stride, base, gout, gid, cgb, s);
    default: return launch_write<4>(pl, k, canonical, p0, p1, ntiles, toff, out, stride, base, gout, gid, cgb, s);
    }
}
template <int W>
int launch_runs(bool write, const uint64_t* keys, uint64_t n, uint64_t c, uint64_t ntiles, uint32_t* cnt, unsigned long long* distinct, const uint32_t* toff, uint64_t* out,
                uint64_t ostride, uint64_t base, uint32_t* gout, uint32_t gid, uint32_t cgb, hipStream_t s) {
    if (!write) hipLaunchKernelGGL(k_ing_runs_count<W>, dim3(tile_grid(ntiles)), dim3(ING_THREADS), 0, s, keys, n, n, c, ntiles, cnt, distinct);
    else hipLaunchKernelGGL(k_ing_runs_write<W>, dim3(tile_grid(ntiles)), dim3(ING_THREADS), 0, s, keys, n, n, c, ntiles, toff, out, ostride, base, gout, gid, cgb);
    HIPCK(hipGetLastError());
    return 0;
}
int ing_runs(int W, bool write, const uint64_t* keys, uint64_t n, uint64_t c, uint64_t ntiles, uint32_t* cnt, unsigned long long* distinct, const uint32_t* toff,
             uint64_t* out, uint64_t ostride, uint64_t base, uint32_t* gout, uint32_t gid, uint32_t cgb, hipStream_t s) {
    switch (W) {
    case 1: return launch_runs<1>(write, keys, n, c, ntiles, cnt, distinct, toff, out, ostride, base, gout, gid, cgb, s);
    case 2: return launch_runs<2>(write, keys, n, c, ntiles, cnt, distinct, toff, out, ostride, base, gout, gid, cgb, s);
    case 3: return launch_runs<3>(write, keys, n, c, ntiles, cnt, distinct, toff, out, ostride, base, gout, gid, cgb, s);
    default: return launch_runs<4>(write, keys, n, c, ntiles, cnt, distinct, toff, out, ostride, base, gout, gid, cgb, s);
    }
}

// n rows of W words (SoA, stride n) in h->ig_keys -> sorted by all 2k bits in h->ig_sorted (stride n), on s
int ing_sort(bft_gpu* h, uint64_t n, hipStream_t s) {
    const int W = h->W, k = h->k;
    uint64_t* keys = h->ig_keys.as<uint64_t>();
    uint64_t* sorted = h->ig_sorted.as<uint64_t>();
    if (W == 1) return bft_rs::sort_keys<uint64_t>(keys, n, sorted, 0, 2 * k, s);
    // least significant word (W - 1) first; word 0 holds the 2k - 64 (W - 1) bits at the top.  The sorted word of a pass is not needed (the last
    // gather fetches every word through the final permutation): it lands in the block the gathers use next.
    DevBuf perm2, ku, ku2;
    CK(perm2.alloc(n * 4));
    CK(ku.alloc(n * 8));
    CK(ku2.alloc(n * 8));
    uint32_t* pa = h->ig_perm.as<uint32_t>();
    uint32_t* pb = perm2.as<uint32_t>();
    const int grid = bft_grid_for((n + 255) / 256);
    hipLaunchKernelGGL(k_ing_iota, dim3(grid), dim3(256), 0, s, pa, n);
    for (int w = W - 1; w >= 0; w--) {
        const int nbits = w == 0 ? 2 * k - 64 * (W - 1) : 64;
        const uint64_t* kin = keys + (uint64_t)w * n;
        if (w != W - 1) {  // (the first pass: the permutation is still the identity)
            hipLaunchKernelGGL(k_ing_gather, dim3(grid), dim3(256), 0, s, kin, pa, ku.as<uint64_t>(), n);
            kin = ku.as<uint64_t>();
        }
        CK((bft_rs::sort_pairs<uint64_t, uint32_t>(kin, pa, n, ku2.as<uint64_t>(), pb, 0, nbits, s)));
        std::swap(pa, pb);
    }
    for (int w = 0; w < W; w++) hipLaunchKernelGGL(k_ing_gather, dim3(grid), dim3(256), 0, s, keys + (uint64_t)w * n, pa, sorted + (uint64_t)w * n, n);
    HIPCK(hipGetLastError());
    return 0;
}

// One batch of sequences resident on the device, on stream s; st: the call's four counters, added to.  The handle's ingest scratch is taken here,
// through the caller's lease (which may hold it already: the host form stages its chunk into the handle's blocks first) and with it released.  Waits for s once per piece (stream path; twice where the piece may not fit the log) or twice (counting path).
int ingest_core(bft_gpu* h, HandleScratch::Lease& lease, const char* d_seqs, const uint64_t* d_seq_off, uint64_t n_seqs, uint64_t total_chars, int canonical, uint32_t min_abundance,
                uint32_t gid, uint64_t st[4], hipStream_t s) {
    if (n_seqs == 0) return 0;
    if (n_seqs >= (1ull << 32)) return bft_fail(BFT_GPU_E_LIMIT, "insert_sequences: at most 2^32 - 1 sequences per call");
    CK(lease.acquire(s, false));
    auto need = [&](DevBuf& b, size_t bytes) { return h->ig.grow(b, bytes, bytes / 8); };
    StageScope stages(h, s);
    PinBlock pin;  // [0] k-mer positions of the batch, [1] valid positions of the piece / kept runs, [2] (a device word beside it: distinct k-mers)
    if (!pin.p) return bft_fail(BFT_GPU_E_HIP, "insert_sequences: no pinned block");
    const int W = h->W, k = h->k;
    const uint64_t n_cw = (total_chars + 31) / 32;
    const uint64_t max_tiles = total_chars / BFT_ING_TILE + 2;  // (k-mer positions <= characters)
    CK(need(h->ig_codes, (n_cw + BFT_MAX_W + 2) * 8));
    CK(need(h->ig_bad, (n_cw + BFT_MAX_W + 2) * 4));
    CK(need(h->ig_npos, (n_seqs + 1) * 8));
    CK(need(h->ig_poff, (n_seqs + 1) * 8));
    CK(need(h->ig_seqtile, max_tiles * 4));
    CK(need(h->ig_tmp, bft_scan::scratch_bytes(std::max(n_seqs + 1, max_tiles) + 1)));
    // (the slack words behind the codes are read by windows at the very end of the blob: keep them defined)
    CK(bft_zero_async(h->ig_codes.as<uint64_t>() + n_cw, (BFT_MAX_W + 2) * 8, s));
    CK(bft_zero_async(h->ig_bad.as<uint32_t>() + n_cw, (BFT_MAX_W + 2) * 4, s));
    if (n_cw)
        CK(bft_timed_launch(h, s, [&] {
            hipLaunchKernelGGL(k_seq_encode, dim3(bft_grid_for((n_cw + 255) / 256)), dim3(256), 0, s, d_seqs, total_chars, n_cw, h->ig_codes.as<uint64_t>(),
                               h->ig_bad.as<uint32_t>());
            HIPCK(hipGetLastError());
            return 0;
        }));
    bft_stage("ingest: encode", (double)total_chars * (1 + 0.375), s);
    CK(bft_timed_launch(h, s, [&] {  // the plan: positions per sequence, their offsets (the total to the host), the tile table
        hipLaunchKernelGGL(k_seq_plan, dim3(bft_grid_for((n_seqs + 256) / 256)), dim3(256), 0, s, d_seq_off, n_seqs, k, h->ig_npos.as<uint64_t>());
        CK(bft_scan::exclusive_sum_ptr<uint64_t>(h->ig_npos.as<uint64_t>(), h->ig_poff.as<uint64_t>(), n_seqs + 1, s, h->ig_tmp, (unsigned long long*)(pin.p + 0)));
        hipLaunchKernelGGL(k_seq_tiles, dim3(256 * 4), dim3(256), 0, s, h->ig_poff.as<uint64_t>(), (uint32_t)n_seqs, h->ig_seqtile.as<uint32_t>());
        HIPCK(hipGetLastError());
        return 0;
    }));
    bft_stage("ingest: plan", (double)n_seqs * 32, s);
    const IngPlan pl{h->ig_codes.as<uint64_t>(), d_seq_off, h->ig_poff.as<uint64_t>(), h->ig_bad.as<uint32_t>(), h->ig_seqtile.as<uint32_t>(), (uint32_t)n_seqs};
    // valid positions of [p0, p1): per tile, scanned, the total in pin.p[1] (enqueued: bft_pin_wait brings it to the host)
    auto count_piece = [&](uint64_t p0, uint64_t p1, uint64_t ntiles) {
        CK(need(h->ig_cnt, ntiles * 4));
        CK(need(h->ig_off, (ntiles + 1) * 4));
        CK(bft_timed_launch(h, s, [&] {
            hipLaunchKernelGGL(k_ing_count, dim3(tile_grid(ntiles)), dim3(ING_THREADS), 0, s, pl.bad, pl.seq_off, pl.pos_off, pl.tile_seq, pl.n_seqs, k, p0, p1, ntiles,
                               h->ig_cnt.as<uint32_t>());
            HIPCK(hipGetLastError());
            return 0;
        }));
        CK(bft_timed_launch(h, s, [&] {
            return bft_scan::exclusive_sum_ptr<uint32_t>(h->ig_cnt.as<uint32_t>(), h->ig_off.as<uint32_t>(), ntiles, s, h->ig_tmp, (unsigned long long*)(pin.p + 1));
        }));
        bft_stage("ingest: valid positions per tile + scan", (double)(p1 - p0) * 0.125, s);
        return 0;
    };
    int rc = 0;
    if (min_abundance == 0) {
        // Pieces of at most "flush_pairs" positions (whole tiles), each appended like a call of bft_gpu_insert_kmers_dev with its valid windows.  The
        // batch's own total reaches the host with the first piece's count; until then the characters bound it.
        const uint64_t piece = h->opt_flush_pairs & ~(uint64_t)(BFT_ING_TILE - 1);
        uint64_t P = total_chars, p0 = 0;
        bool first = true;
        while (p0 < P && rc == 0) {
            const uint64_t p1 = std::min(p0 + piece, P), ntiles = (p1 - p0 + BFT_ING_TILE - 1) / BFT_ING_TILE;
            if ((rc = count_piece(p0, p1, ntiles)) != 0) break;
            // Where the log takes the piece even if every position is valid, nothing depends on the count but the log's new end: room for all of
            // them, the write pass enqueued behind the scan, ONE wait.  Otherwise the count comes first -- it decides about the build in front.
            const bool ahead = h->log_n + (p1 - p0) <= h->opt_flush_pairs;
            auto write_rows = [&] {
                return bft_timed_launch(h, s, [&] {
                    return ing_write(W, pl, k, canonical, p0, p1, ntiles, h->ig_off.as<uint32_t>(), h->log_k.as<uint64_t>(), h->log_cap, h->log_n, h->log_g.as<uint32_t>(), gid,
                                     h->log_comp ? h->log_gb : 0u, s);
                });
            };
            if (ahead && ((rc = bft_log_prepare(h, p1 - p0, gid)) != 0 || (rc = write_rows()) != 0)) break;
            if ((rc = bft_pin_wait(pin, s)) != 0) break;
            if (first) { P = pin.p[0]; st[0] += P; first = false; }
            const uint64_t p1c = std::min(p1, P);
            const uint64_t V = pin.p[1];
            if (p1c > p0) st[1] += (p1c - p0) - V;
            if (V) {
                if (!ahead && ((rc = bft_log_prepare(h, V, gid)) != 0 || (rc = write_rows()) != 0)) break;
                bft_stage("ingest: windows -> log rows", (double)V * 8 * W + (double)(p1c - p0) * 0.375, s);
                if ((rc = bft_log_commit(h, V, gid, s)) != 0) break;
                st[3] += V;
            }
            p0 = p1;
        }
        if (first && rc == 0) {  // (a blob without a character: the plan's total has not been waited for)
            if ((rc = bft_pin_wait(pin, s)) == 0) st[0] += pin.p[0];
        }
    } else {
        do {
            const uint64_t ntiles = (total_chars + BFT_ING_TILE - 1) / BFT_ING_TILE;
            uint64_t P = 0, V = 0;
            if (ntiles) {
                if ((rc = count_piece(0, total_chars, ntiles)) != 0 || (rc = bft_pin_wait(pin, s)) != 0) break;
                P = pin.p[0];
                V = pin.p[1];
            }
            if (P > h->opt_flush_pairs) { rc = bft_fail(BFT_GPU_E_LIMIT, "insert_sequences: more k-mer positions than flush_pairs in one counting call (min_abundance >= 1)"); break; }
            st[0] += P;
            st[1] += P - V;
            if (V == 0) break;
            if ((rc = need(h->ig_keys, V * 8 * W)) != 0 || (rc = need(h->ig_sorted, V * 8 * W + 8)) != 0 || (rc = need(h->ig_perm, V * 4)) != 0) break;
            rc = bft_timed_launch(h, s, [&] {
                return ing_write(W, pl, k, canonical, 0, total_chars, ntiles, h->ig_off.as<uint32_t>(), h->ig_keys.as<uint64_t>(), V, 0, nullptr, 0, 0, s);
            });
            if (rc != 0) break;
            bft_stage("ingest: windows -> keys", (double)V * 8 * W + (double)P * 0.375, s);
            if ((rc = bft_timed_launch(h, s, [&] { return ing_sort(h, V, s); })) != 0) break;
            bft_stage("ingest: sort", 0, s);
            const uint64_t rtiles = (V + BFT_ING_TILE - 1) / BFT_ING_TILE;
            unsigned long long* d_distinct = (unsigned long long*)(h->ig_sorted.as<uint64_t>() + V * W);  // (the word behind the sorted keys)
            if ((rc = need(h->ig_cnt, rtiles * 4)) != 0 || (rc = need(h->ig_off, (rtiles + 1) * 4)) != 0) break;
            if ((rc = bft_zero_async(d_distinct, 8, s)) != 0) break;
            rc = bft_timed_launch(h, s, [&] {
                CK(ing_runs(W, false, h->ig_sorted.as<uint64_t>(), V, min_abundance, rtiles, h->ig_cnt.as<uint32_t>(), d_distinct, nullptr, nullptr, 0, 0, nullptr, 0, 0, s));
                return bft_scan::exclusive_sum_ptr<uint32_t>(h->ig_cnt.as<uint32_t>(), h->ig_off.as<uint32_t>(), rtiles, s, h->ig_tmp, (unsigned long long*)(pin.p + 1));
            });
            if (rc != 0) break;
            uint64_t distinct = 0;
            if (hipMemcpyAsync(&distinct, d_distinct, 8, hipMemcpyDeviceToHost, s) != hipSuccess) { rc = bft_fail(BFT_GPU_E_HIP, "insert_sequences: copy of the distinct count"); break; }
            bft_stage("ingest: run lengths + scan", (double)V * 8 * W * 2, s);
            if ((rc = bft_pin_wait(pin, s)) != 0) break;
            if (hipStreamSynchronize(s) != hipSuccess) { rc = bft_fail(BFT_GPU_E_HIP, "insert_sequences: stream synchronisation"); break; }
            const uint64_t K = pin.p[1];
            st[2] += distinct;
            if (K == 0) break;
            if ((rc = bft_log_prepare(h, K, gid)) != 0) break;
            rc = bft_timed_launch(h, s, [&] {
                return ing_runs(W, true, h->ig_sorted.as<uint64_t>(), V, min_abundance, rtiles, nullptr, nullptr, h->ig_off.as<uint32_t>(), h->log_k.as<uint64_t>(), h->log_cap,
                                h->log_n, h->log_g.as<uint32_t>(), gid, h->log_comp ? h->log_gb : 0u, s);
            });
            if (rc != 0) break;
            bft_stage("ingest: kept k-mers -> log rows", (double)K * 8 * W * 2, s);
            if ((rc = bft_log_commit(h, K, gid, s)) != 0) break;
            st[3] += K;
        } while (false);
    }
    // the caller may reuse its buffers -- and the log's rows are complete -- when the call returns
    if (hipStreamSynchronize(s) != hipSuccess && rc == 0) rc = bft_fail(BFT_GPU_E_HIP, "insert_sequences: stream synchronisation");
    return rc;
}

int check_args(bft_gpu* h, const void* seqs, const void* seq_off, uint64_t n_seqs, uint32_t gid) {
    if (!h || ((!seqs || !seq_off) && n_seqs)) return bft_fail(BFT_GPU_E_ARG, "NULL argument");
    if (gid >= BFT_MAX_GENOME_ID) return bft_fail(BFT_GPU_E_ARG, "id_genome out of range (must be below 2^24)");
    if (h->marking) return bft_fail(BFT_GPU_E_STATE, "insert: the graph is locked for vertex marking (bft_gpu_marks_end unlocks it)");
    return 0;
}

}  // namespace

extern "C" int bft_gpu_debug_ingest_plan(uint64_t out[3]) {
    if (!out) return bft_fail(BFT_GPU_E_ARG, "NULL argument");
    out[0] = BFT_ING_TILE;
    out[1] = BFT_ING_CHUNK_DEFAULT;
    out[2] = BFT_ING_CHUNK_MIN;
    return BFT_GPU_OK;
}

extern "C" int bft_gpu_debug_ingest_chunks(const uint64_t* seq_off, uint64_t nb_seqs, int k, uint64_t chunk_chars, uint64_t* out, uint64_t cap, uint64_t* n_out) {
    if (!n_out || (!seq_off && nb_seqs) || k < 1 || chunk_chars < BFT_ING_CHUNK_MIN || chunk_chars < 2 * (uint64_t)k) return bft_fail(BFT_GPU_E_ARG, "bad argument");
    BftIngCursor cur;
    std::vector<uint64_t> off;
    uint64_t n = 0;
    while (cur.seq < nb_seqs) {
        const uint64_t c0 = bft_ingest_next_chunk(seq_off, nb_seqs, k, chunk_chars, cur, off);
        if (out && n < cap) {
            out[3 * n] = c0;
            out[3 * n + 1] = c0 + off.back();
            out[3 * n + 2] = off.size() - 1;
        }
        n++;
    }
    *n_out = n;
    return BFT_GPU_OK;
}

extern "C" int bft_gpu_insert_sequences_dev(bft_gpu* h, const void* d_seqs, const void* d_seq_off, uint64_t n_seqs, uint64_t total_chars, int canonical,
                                            uint32_t min_abundance, uint32_t id_genome, uint64_t stats[4], void* hip_stream) {
    CK(check_args(h, total_chars ? d_seqs : (const void*)h, d_seq_off, n_seqs, id_genome));
    uint64_t st[4] = {0, 0, 0, 0};
    if (stats) memcpy(stats, st, sizeof(st));
    if (n_seqs == 0) return BFT_GPU_OK;
    ENTER(h);
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : h->stream;
    if (bft_stream_capturing(s)) return bft_fail(BFT_GPU_E_ARG, "insert_sequences: not inside a graph capture (the call waits for its row count)");
    bft_pool_set_stream(h->device, s);  // (the sort's temporaries are used on s: whoever takes them next is ordered behind it or waits for it)
    HandleScratch::Lease lease(h->ig);
    const int rc = ingest_core(h, lease, (const char*)d_seqs, (const uint64_t*)d_seq_off, n_seqs, total_chars, canonical, min_abundance, id_genome, st, s);
    if (stats) memcpy(stats, st, sizeof(st));
    return rc;
}

extern "C" int bft_gpu_insert_sequences(bft_gpu* h, const char* seqs, const uint64_t* seq_off, uint64_t n_seqs, int canonical, uint32_t min_abundance,
                                        uint32_t id_genome, uint64_t stats[4]) {
    CK(check_args(h, (n_seqs && seq_off && seq_off[n_seqs] > seq_off[0]) ? (const void*)seqs : (const void*)h, seq_off, n_seqs, id_genome));
    uint64_t st[4] = {0, 0, 0, 0};
    if (stats) memcpy(stats, st, sizeof(st));
    if (n_seqs == 0) return BFT_GPU_OK;
    uint64_t positions = 0;
    for (uint64_t i = 0; i < n_seqs; i++) {
        if (seq_off[i + 1] < seq_off[i]) return bft_fail(BFT_GPU_E_ARG, "insert_sequences: the offsets decrease");
        const uint64_t len = seq_off[i + 1] - seq_off[i];
        if (len >= (uint64_t)h->k) positions += len - (uint64_t)h->k + 1;
    }
    if (min_abundance && positions > h->opt_flush_pairs)
        return bft_fail(BFT_GPU_E_LIMIT, "insert_sequences: more k-mer positions than flush_pairs in one counting call (min_abundance >= 1)");
    ENTER(h);
    const hipStream_t s = h->stream;
    // The counting path is one unit: the whole blob in one block.  The stream path goes chunk by chunk ("ingest_chunk_chars").
    const uint64_t total = seq_off[n_seqs] - seq_off[0];
    const uint64_t chunk = min_abundance ? std::max<uint64_t>(total, 1) : std::max<uint64_t>(h->opt_ingest_chunk, 2 * (uint64_t)h->k);
    BftIngCursor cur;
    std::vector<uint64_t> off;
    int rc = 0;
    while (cur.seq < n_seqs && rc == 0) {
        const uint64_t c0 = bft_ingest_next_chunk(seq_off, n_seqs, h->k, chunk, cur, off);
        const uint64_t ns = off.size() - 1, nchars = off.back();
        if (ns == 0) return bft_fail(BFT_GPU_E_ARG, "insert_sequences: empty chunk");  // (cannot happen: chunk >= 2k)
        // the staging blocks are the handle's: the chunk before was waited for by ingest_core
        HandleScratch::Lease lease(h->ig);
        CK(lease.acquire(s, false));
        CK(h->ig.grow(h->ig_seq, nchars + 16, nchars / 8));
        CK(h->ig.grow(h->ig_soff, (ns + 1) * 8, ns));
        if (nchars) HIPCK(hipMemcpyAsync(h->ig_seq.p, seqs + c0, nchars, hipMemcpyHostToDevice, s));
        HIPCK(hipMemcpyAsync(h->ig_soff.p, off.data(), (ns + 1) * 8, hipMemcpyHostToDevice, s));
        rc = ingest_core(h, lease, h->ig_seq.as<char>(), h->ig_soff.as<uint64_t>(), ns, nchars, canonical, min_abundance, id_genome, st, s);
    }
    if (stats) memcpy(stats, st, sizeof(st));
    return rc;
}

extern "C" int bft_gpu_insert_sequence_file(bft_gpu* h, const char* path, int canonical, uint32_t min_abundance, uint32_t id_genome, uint64_t stats[4]) {
    if (!h || !path) return bft_fail(BFT_GPU_E_ARG, "NULL argument");
    char* blob = nullptr;
    uint64_t* off = nullptr;
    uint64_t ns = 0;
    const int frc = bft_seqfile_read(path, &blob, &off, &ns);
    if (frc != BFT_SEQFILE_OK)
        return bft_fail(BFT_GPU_E_IO, std::string(frc == BFT_SEQFILE_E_IO ? "cannot read " : "neither FASTA nor four-line FASTQ (or a truncated record): ") + path);
    const int rc = bft_gpu_insert_sequences(h, blob, off, ns, canonical, min_abundance, id_genome, stats);
    bft_seqfile_free(blob, off);
    return rc;
}
