// bft_pangenome.hip -- pan-genome k-mer classes of the index (extract_core_kmers / extract_dispensable_kmers / extract_singleton_kmers through
// extract_pangenome_kmers_to_disk, reference snippets.h, src/snippets.c:10-106) over the sorted T-form table tk (one row per stored k-mer, rows in the
// bft_gpu_extract order), the colour set of every row tcol and the dictionary cs_off / cs_ids.  The genome count of row r is
// cs_off[tcol[r] + 1] - cs_off[tcol[r]]: two dependent 4-byte gathers.
//   (one scan: BftPgSel computes the selection min_count <= count <= max_count on the fly; slot[r] is the output slot of a selected row, slot[n] the total)
//   k_pg_emit     one lane per row: a selected row (slot[r + 1] != slot[r]) below cap writes its row, its packed k-mer and its ASCII k-mer with the NUL,
//                 in whole 4-byte words wherever the output address allows
//   k_pg_usage    usage[cs] = rows that carry cs.  On a pan-genome index ONE set (the core set) owns most rows, and an atomic per lane would pile up on its
//                 counter: a wavefront picks the most frequent of four sampled sets of its stretch as its hot set and counts it in registers (one
//                 shuffle reduction and ONE atomic when the stretch ends or the hot set changes); the other rows are summed per lane over runs of one
//                 set and go to memory once per run
//   k_pg_dict     one pass over the dictionary, not over rows x ids: a lane takes 16 consecutive ids (its set found by one binary search in cs_off, then
//                 followed), adds the set's usage to genome_total (and genome_private for a set of one); a lane per set adds it to the spectrum.
//                 Up to BFT_PG_LDS_GENOMES genomes the 3 G + 1 counters of a workgroup live in LDS (32 bits are enough: no counter exceeds the number
//                 of rows, < 2^31) and reach memory once per workgroup as 64-bit atomics, zeros skipped; beyond, 64-bit atomics straight to memory
// Integer atomics only: the results are exact and do not depend on scheduling.  No kernel needs scratch memory.

#include "bft_dev.h"
#include "bft_handle.h"
#include "bft_pangenome.h"
#include "bft_scan.h"
#include "bft_walk.h"

namespace {

constexpr int PG_ROUNDS = 64;         // rows per lane and stretch in k_pg_usage (64-row rounds of a wavefront's stretch)
constexpr int PG_BATCH = 8;           // rounds loaded before any is counted
constexpr int PG_IDS_PER_LANE = 16;   // consecutive dictionary ids per lane in k_pg_dict
constexpr uint32_t PG_LDS_BINS = 3u * BFT_PG_LDS_GENOMES + 1u;
constexpr int PG_DICT_BLOCKS = 256;   // workgroups of the LDS form: each ends with up to 3 G + 1 atomics

// len bytes c(0) .. c(len - 1) at p: single bytes up to the first 4-byte boundary and behind the last, whole words between
template <class F>
__device__ __forceinline__ void pg_write(uint8_t* p, int len, F&& c) {
    int j = 0;
    for (; j < len && (((uintptr_t)(p + j)) & 3u); j++) p[j] = (uint8_t)c(j);
    for (; j + 4 <= len; j += 4) *reinterpret_cast<uint32_t*>(p + j) = c(j) | (c(j + 1) << 8) | (c(j + 2) << 16) | (c(j + 3) << 24);
    for (; j < len; j++) p[j] = (uint8_t)c(j);
}

template <int W>
__global__ __launch_bounds__(BFT_LAUNCH_THREADS) void k_pg_emit(const uint64_t* __restrict__ tk, uint32_t n, int k, int B, const uint32_t* __restrict__ slot,
                                                        uint8_t* __restrict__ kmers, char* __restrict__ ascii, uint32_t* __restrict__ rows, uint64_t cap) {
    for (uint64_t i = blockIdx.x * (uint64_t)BFT_LAUNCH_THREADS + threadIdx.x; i < n; i += (uint64_t)gridDim.x * BFT_LAUNCH_THREADS) {
        const uint32_t s = slot[i];
        if (slot[i + 1] == s || s >= cap) continue;
        if (rows) rows[s] = (uint32_t)i;
        if (!kmers && !ascii) continue;
        uint64_t t[W], x[W];
        bft_load_row<W>(tk + i * W, t);
        bft_x_from_tform<W>(t, k, x);
        auto word = [&](int w) {
            uint64_t v = 0;
#pragma unroll
            for (int q = 0; q < W; q++)
                if (q == w) v = x[q];
            return v;
        };
        if (kmers) pg_write(kmers + (uint64_t)s * B, B, [&](int b) { return (uint32_t)(word(b >> 3) >> (8 * (b & 7))) & 0xFFu; });
        // ('A' 'C' 'G' 'T' as the bytes of one word; the NUL the reference's strlen + 1 writes)
        if (ascii)
            pg_write(reinterpret_cast<uint8_t*>(ascii) + (uint64_t)s * (uint32_t)(k + 1), k + 1,
                     [&](int j) { return j < k ? (0x54474341u >> (8 * (uint32_t)((word(j >> 5) >> (2 * (j & 31))) & 3ull))) & 0xFFu : 0u; });
    }
}

__device__ __forceinline__ uint32_t pg_wave_sum(uint32_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d);
    return v;
}

__global__ __launch_bounds__(BFT_LAUNCH_THREADS) void k_pg_usage(uint32_t n, const uint32_t* __restrict__ tcol, uint32_t* __restrict__ usage) {
    constexpr uint64_t STRETCH = 64ull * PG_ROUNDS;  // rows per wavefront and pass
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t waves = (uint64_t)gridDim.x * (BFT_LAUNCH_THREADS / 64);
    uint32_t hot = BFT_PG_NONE, hot_cnt = 0;  // (hot is the same in every lane of the wavefront; hot_cnt is the lane's share)
    for (uint64_t base = (blockIdx.x * (uint64_t)(BFT_LAUNCH_THREADS / 64) + (threadIdx.x >> 6)) * STRETCH; base < n; base += waves * STRETCH) {
        // the stretch's hot set: the most frequent of the sets at lanes 0, 16, 32, 48 of its first round
        const uint32_t c0 = base + lane < n ? tcol[base + lane] : BFT_PG_NONE;
        uint32_t best = BFT_PG_NONE;
        int best_n = 0;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const uint32_t cand = (uint32_t)__shfl((int)c0, q * 16);
            const int m = __popcll(__ballot(cand != BFT_PG_NONE && c0 == cand));
            if (m > best_n) {
                best_n = m;
                best = cand;
            }
        }
        if (best != hot) {
            const uint32_t tot = pg_wave_sum(hot_cnt);
            if (lane == 0 && tot) atomicAdd(&usage[hot], tot);
            hot = best;
            hot_cnt = 0;
        }
        uint32_t cur = BFT_PG_NONE, cnt = 0;
        for (int r0 = 0; r0 < PG_ROUNDS; r0 += PG_BATCH) {
            uint32_t v[PG_BATCH];
#pragma unroll
            for (int r = 0; r < PG_BATCH; r++) {
                const uint64_t i = base + (uint64_t)(r0 + r) * 64u + lane;
                v[r] = i < n ? tcol[i] : BFT_PG_NONE;
            }
#pragma unroll
            for (int r = 0; r < PG_BATCH; r++) {
                const uint32_t c = v[r];
                if (c == BFT_PG_NONE) continue;
                if (c == hot) {
                    hot_cnt++;
                    continue;
                }
                if (c != cur) {
                    if (cnt) atomicAdd(&usage[cur], cnt);
                    cur = c;
                    cnt = 0;
                }
                cnt++;
            }
        }
        if (cnt) atomicAdd(&usage[cur], cnt);
    }
    const uint32_t tot = pg_wave_sum(hot_cnt);
    if (lane == 0 && tot) atomicAdd(&usage[hot], tot);
}

// counters: [0, G] spectrum, [G + 1, 2 G] genome_total, [2 G + 1, 3 G] genome_private
template <bool LDS>
__global__ __launch_bounds__(BFT_LAUNCH_THREADS) void k_pg_dict(uint32_t n_sets, uint64_t n_ids, const uint32_t* __restrict__ cs_off, const void* __restrict__ cs_ids,
                                                        uint32_t cs_w, const uint32_t* __restrict__ usage, uint32_t G, unsigned long long* __restrict__ spectrum,
                                                        unsigned long long* __restrict__ total, unsigned long long* __restrict__ priv) {
    __shared__ uint32_t bins[LDS ? PG_LDS_BINS : 1u];
    const uint32_t nbins = 3u * G + 1u;
    auto out = [&](uint32_t b) -> unsigned long long* {
        if (b <= G) return spectrum ? spectrum + b : nullptr;
        if (b <= 2u * G) return total ? total + (b - G - 1u) : nullptr;
        return priv ? priv + (b - 2u * G - 1u) : nullptr;
    };
    auto add = [&](uint32_t b, uint32_t v) {
        if (LDS) atomicAdd(&bins[b], v);
        else if (unsigned long long* o = out(b)) atomicAdd(o, (unsigned long long)v);
    };
    if (LDS) {
        for (uint32_t b = threadIdx.x; b < nbins; b += BFT_LAUNCH_THREADS) bins[b] = 0;
        __syncthreads();
    }
    const uint64_t tid = blockIdx.x * (uint64_t)BFT_LAUNCH_THREADS + threadIdx.x, nthreads = (uint64_t)gridDim.x * BFT_LAUNCH_THREADS;
    for (uint64_t c = tid; c < n_sets; c += nthreads) {
        const uint32_t u = usage[c], sz = cs_off[c + 1] - cs_off[c];
        if (u && sz <= G) add(sz, u);
    }
    for (uint64_t q0 = tid * PG_IDS_PER_LANE; q0 < n_ids; q0 += nthreads * PG_IDS_PER_LANE) {
        // the set of id q0: the last c with cs_off[c] <= q0 (sets are not empty: cs_off ascends strictly)
        uint32_t lo = 0, hi = n_sets;
        while (hi - lo > 1u) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (cs_off[mid] <= q0) lo = mid;
            else hi = mid;
        }
        uint32_t c = lo, a = cs_off[c], e = cs_off[c + 1], u = usage[c];
        const uint64_t q1 = q0 + PG_IDS_PER_LANE < n_ids ? q0 + PG_IDS_PER_LANE : n_ids;
        for (uint64_t q = q0; q < q1; q++) {
            while (q >= e && c + 1u < n_sets) {
                c++;
                a = e;
                e = cs_off[c + 1];
                u = usage[c];
            }
            const uint32_t g = bft_cs_id_at(cs_ids, cs_w, q);
            if (u == 0 || g >= G) continue;
            add(G + 1u + g, u);
            if (e - a == 1u) add(2u * G + 1u + g, u);
        }
    }
    if (LDS) {
        __syncthreads();
        for (uint32_t b = threadIdx.x; b < nbins; b += BFT_LAUNCH_THREADS) {
            const uint32_t v = bins[b];
            if (v == 0) continue;
            if (unsigned long long* o = out(b)) atomicAdd(o, (unsigned long long)v);
        }
    }
}

}  // namespace

int bft_pg_emit(int W, const uint64_t* d_tk, uint64_t n, int k, int B, const BftPgScratch& p, uint8_t* d_kmers, char* d_ascii, uint32_t* d_rows, uint64_t cap,
                hipStream_t s) {
    if (n == 0 || cap == 0 || (!d_kmers && !d_ascii && !d_rows)) return 0;
    return bft_for_w(W, [&](auto KW) { return bft_launch256(k_pg_emit<KW>, n, s, d_tk, (uint32_t)n, k, B, (const uint32_t*)p.slot, d_kmers, d_ascii, d_rows, cap); });
}

int bft_pg_usage(uint64_t n, const uint32_t* d_tcol, const BftPgScratch& p, hipStream_t s) {
    // (the items are lanes: each takes PG_ROUNDS rows)
    return bft_launch256(k_pg_usage, (n + PG_ROUNDS - 1) / PG_ROUNDS, s, (uint32_t)n, d_tcol, p.usage);
}

int bft_pg_dict(uint64_t n_sets, uint64_t n_ids, const uint32_t* d_cs_off, const void* d_cs_ids, uint32_t cs_w, uint32_t G, const BftPgScratch& p,
                unsigned long long* d_spectrum, unsigned long long* d_total, unsigned long long* d_private, hipStream_t s) {
    if (n_sets == 0 || (!d_spectrum && !d_total && !d_private)) return 0;
    const uint64_t lanes = std::max(n_sets, (n_ids + PG_IDS_PER_LANE - 1) / PG_IDS_PER_LANE);
    if (G > BFT_PG_LDS_GENOMES)
        return bft_launch256(k_pg_dict<false>, lanes, s, (uint32_t)n_sets, n_ids, d_cs_off, d_cs_ids, cs_w, (const uint32_t*)p.usage, G, d_spectrum, d_total, d_private);
    // (the LDS form: a grid of its own, every workgroup ends with up to 3 G + 1 atomics)
    const dim3 grid((unsigned)std::min<uint64_t>(PG_DICT_BLOCKS, (lanes + BFT_LAUNCH_THREADS - 1) / BFT_LAUNCH_THREADS));
    hipLaunchKernelGGL(k_pg_dict<true>, grid, dim3(BFT_LAUNCH_THREADS), 0, s, (uint32_t)n_sets, n_ids, d_cs_off, d_cs_ids, cs_w, (const uint32_t*)p.usage, G, d_spectrum,
                       d_total, d_private);
    HIPCK(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------------
// the C-ABI entry points: the handle's scratch, the chain of launches, the host-buffer forms
// ------------------------------------------------------------------------------------------------
// the arrays of a block with room for m rows and `sets` colour sets, from `base` on; returns the block's size
static size_t pg_carve(uint64_t m, uint64_t sets, uint8_t* base, BftPgScratch* p) {
    Carver c{base};
    c.take(p->slot, (m + 1) * 4);
    c.take(p->usage, sets * 4);
    return c.off;
}
// The handle's scratch (h->pg: HandleScratch, bft_handle.h) for an index of n rows and n_sets colour sets on stream s: its own block, shared with no
// other query, sized exactly.
static int pg_scratch(bft_gpu* h, HandleScratch::Lease& lease, uint64_t n, uint64_t n_sets, hipStream_t s, BftPgScratch* p) {
    CK(lease.acquire(s, false));  // (the entry points refuse a capturing stream)
    h->pg_m = std::max(n, h->pg_m);
    h->pg_sets = std::max(n_sets, h->pg_sets);
    CK(h->pg.grow(h->pg_buf, pg_carve(h->pg_m, h->pg_sets, nullptr, p), 0));
    CK(h->pg.grow(h->pg_tmp, bft_scan::scratch_bytes(n + 1), 0));
    pg_carve(h->pg_m, h->pg_sets, h->pg_buf.as<uint8_t>(), p);
    return 0;
}
static int pg_prepare(bft_gpu* h) {
    CK(bft_ensure_built(h));  // ("compact_table": the sorted table comes back, as for rows, prefixes and simple paths)
    if (h->n_kmers >= (1ull << 31)) return bft_fail(BFT_GPU_E_LIMIT, "k-mer classes: at most 2^31 - 1 k-mers");
    return 0;
}
static uint32_t pg_genomes(const bft_gpu* h) { return bft_nb_genomes(h); }  // (bft_handle.h: the genome-by-genome matrix counts them the same way)
// The selection and its scan on stream s: slot[] filled, the number of selected rows at d_count (8 bytes, device).
static int pg_select(bft_gpu* h, uint32_t lo, uint32_t hi, hipStream_t s, unsigned long long* d_count, const BftPgScratch& p) {
    const uint64_t n = h->n_kmers;
    const BftPgSel sel{h->d_tcol.as<uint32_t>(), h->d_cs_off.as<uint32_t>(), lo, hi};
    CK(bft_timed_launch(h, s, [&] { return bft_scan::exclusive_sum<uint32_t>(sel, p.slot, n, s, h->pg_tmp, d_count, true); }));
    bft_stage("k-mer classes: selection and its scan", (double)n * (4 + 8 + 4), s);
    return 0;
}
// the first `cap` selected rows into the outputs; n_sel: how many rows are written at most (the stage's bytes)
static int pg_emit(bft_gpu* h, const BftPgScratch& p, uint8_t* d_kmers, char* d_ascii, uint32_t* d_rows, uint64_t cap, uint64_t n_sel, hipStream_t s) {
    const uint64_t n = h->n_kmers;
    CK(bft_timed_launch(h, s, [&] { return bft_pg_emit(h->W, h->d_tk.as<uint64_t>(), n, h->k, h->B, p, d_kmers, d_ascii, d_rows, cap, s); }));
    const bool spell = d_kmers || d_ascii;
    bft_stage("k-mer classes: emission",
              (double)n * 4 + (double)n_sel * ((spell ? 8.0 * h->W : 0.0) + (d_kmers ? h->B : 0) + (d_ascii ? h->k + 1 : 0) + (d_rows ? 4 : 0)), s);
    return 0;
}

extern "C" int bft_gpu_kmers_by_count_dev(bft_gpu* h, uint32_t min_count, uint32_t max_count, void* d_kmers_out, void* d_ascii_out, void* d_rows_out, uint64_t cap,
                                          void* d_count, void* hip_stream) {
    if (!h || !d_count) return bft_fail(BFT_GPU_E_ARG, "NULL argument");
    ENTER(h);
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : h->stream;
    if (bft_stream_capturing(s)) return bft_fail(BFT_GPU_E_ARG, "k-mer classes recorded into a graph: not supported (the table may have to come back, scratch may grow)");
    CK(pg_prepare(h));
    if (h->n_kmers == 0 || min_count > max_count) {
        CK(bft_zero_async(d_count, 8, s));
        return bft_note_foreign_stream(h, s);
    }
    {
        HandleScratch::Lease lease(h->pg);
        BftPgScratch p;
        CK(pg_scratch(h, lease, h->n_kmers, h->n_sets, s, &p));
        StageScope stage_scope(h, s);
        CK(pg_select(h, min_count, max_count, s, (unsigned long long*)d_count, p));
        CK(pg_emit(h, p, (uint8_t*)d_kmers_out, (char*)d_ascii_out, (uint32_t*)d_rows_out, cap, std::min<uint64_t>(cap, h->n_kmers), s));
    }
    return bft_note_foreign_stream(h, s);
}

// The host-buffer form: the class is counted on the device, and the outputs filled only when cap holds it all.
extern "C" int bft_gpu_kmers_by_count(bft_gpu* h, uint32_t min_count, uint32_t max_count, uint8_t* kmers_out, char* ascii_out, uint32_t* rows_out, uint64_t cap,
                                      uint64_t* n_out) {
    if (!h || !n_out) return bft_fail(BFT_GPU_E_ARG, "NULL argument");
    ENTER(h);
    CK(pg_prepare(h));
    *n_out = 0;
    const uint64_t n = h->n_kmers;
    if (n == 0 || min_count > max_count) return BFT_GPU_OK;
    const hipStream_t s = h->stream;
    DevBuf dcnt;
    CK(dcnt.alloc(8));
    HandleScratch::Lease lease(h->pg);
    BftPgScratch p;
    CK(pg_scratch(h, lease, n, h->n_sets, s, &p));
    StageScope stage_scope(h);
    CK(pg_select(h, min_count, max_count, s, dcnt.as<unsigned long long>(), p));
    unsigned long long cnt = 0;
    HIPCK(hipMemcpyAsync(&cnt, dcnt.p, 8, hipMemcpyDeviceToHost, s));
    HIPCK(hipStreamSynchronize(s));
    *n_out = cnt;
    const bool any = kmers_out || ascii_out || rows_out;
    if (any && cap < cnt) return bft_fail(BFT_GPU_E_NOSPACE, "k-mer class buffers too small");
    if (any && cnt) {
        const size_t kb = (size_t)cnt * h->B, ab = (size_t)cnt * (h->k + 1);
        DevBuf dk, da, dr;
        if (kmers_out) CK(dk.alloc(kb));
        if (ascii_out) CK(da.alloc(ab));
        if (rows_out) CK(dr.alloc(cnt * 4));
        CK(pg_emit(h, p, kmers_out ? dk.as<uint8_t>() : nullptr, ascii_out ? da.as<char>() : nullptr, rows_out ? dr.as<uint32_t>() : nullptr, cnt, cnt, s));
        if (kmers_out) HIPCK(hipMemcpyAsync(kmers_out, dk.p, kb, hipMemcpyDeviceToHost, s));
        if (ascii_out) HIPCK(hipMemcpyAsync(ascii_out, da.p, ab, hipMemcpyDeviceToHost, s));
        if (rows_out) HIPCK(hipMemcpyAsync(rows_out, dr.p, cnt * 4, hipMemcpyDeviceToHost, s));
        HIPCK(hipStreamSynchronize(s));
    }
    return BFT_GPU_OK;
}

// usage per colour set, then the dictionary pass, on stream s; the outputs (G + 1, G, G entries; any may be NULL) are zeroed first
static int pg_stats(bft_gpu* h, uint32_t G, unsigned long long* d_spectrum, unsigned long long* d_total, unsigned long long* d_private, const BftPgScratch& p,
                    hipStream_t s) {
    const uint64_t n = h->n_kmers, ns = h->n_sets;
    if (d_spectrum) CK(bft_zero_async(d_spectrum, ((size_t)G + 1) * 8, s));
    if (d_total && G) CK(bft_zero_async(d_total, (size_t)G * 8, s));
    if (d_private && G) CK(bft_zero_async(d_private, (size_t)G * 8, s));
    if (n == 0) return 0;
    CK(bft_zero_async(p.usage, ns * 4, s));
    CK(bft_timed_launch(h, s, [&] { return bft_pg_usage(n, h->d_tcol.as<uint32_t>(), p, s); }));
    bft_stage("k-mer classes: rows per colour set", (double)n * 4 + (double)ns * 8, s);
    CK(bft_timed_launch(h, s, [&] { return bft_pg_dict(ns, h->n_ids, h->d_cs_off.as<uint32_t>(), h->d_cs_ids.p, h->cs_w, G, p, d_spectrum, d_total, d_private, s); }));
    bft_stage("k-mer classes: spectrum and genomes from the dictionary", (double)ns * 8 + (double)h->n_ids * h->cs_w + ((double)3 * G + 1) * 8, s);
    return 0;
}

extern "C" int bft_gpu_pangenome_stats_dev(bft_gpu* h, void* d_spectrum, void* d_genome_total, void* d_genome_private, uint32_t cap, void* hip_stream) {
    if (!h) return bft_fail(BFT_GPU_E_ARG, "NULL argument");
    ENTER(h);
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : h->stream;
    if (bft_stream_capturing(s)) return bft_fail(BFT_GPU_E_ARG, "pan-genome statistics recorded into a graph: not supported (the table may have to come back, scratch may grow)");
    CK(pg_prepare(h));
    const uint32_t G = pg_genomes(h);
    if (!d_spectrum && !d_genome_total && !d_genome_private) return BFT_GPU_OK;
    if ((uint64_t)cap < (uint64_t)G + 1) return bft_fail(BFT_GPU_E_NOSPACE, "pan-genome statistics: room for nb_genomes + 1 entries is needed");
    {
        HandleScratch::Lease lease(h->pg);  // (held only where there are rows)
        BftPgScratch p{};
        if (h->n_kmers) CK(pg_scratch(h, lease, h->n_kmers, h->n_sets, s, &p));
        StageScope stage_scope(h, s);
        CK(pg_stats(h, G, (unsigned long long*)d_spectrum, (unsigned long long*)d_genome_total, (unsigned long long*)d_genome_private, p, s));
    }
    return bft_note_foreign_stream(h, s);
}

extern "C" int bft_gpu_pangenome_stats(bft_gpu* h, uint64_t* spectrum, uint64_t* genome_total, uint64_t* genome_private, uint32_t cap) {
    if (!h) return bft_fail(BFT_GPU_E_ARG, "NULL argument");
    ENTER(h);
    CK(pg_prepare(h));
    const uint32_t G = pg_genomes(h);
    if (!spectrum && !genome_total && !genome_private) return BFT_GPU_OK;
    if ((uint64_t)cap < (uint64_t)G + 1) return bft_fail(BFT_GPU_E_NOSPACE, "pan-genome statistics: room for nb_genomes + 1 entries is needed");
    const hipStream_t s = h->stream;
    DevBuf out;  // [spectrum G + 1 | genome_total G | genome_private G]
    CK(out.alloc(((size_t)3 * G + 1) * 8));
    unsigned long long* const d = out.as<unsigned long long>();
    HandleScratch::Lease lease(h->pg);  // (held only where there are rows)
    BftPgScratch p{};
    if (h->n_kmers) CK(pg_scratch(h, lease, h->n_kmers, h->n_sets, s, &p));
    StageScope stage_scope(h);
    CK(pg_stats(h, G, d, d + G + 1, d + 2 * (size_t)G + 1, p, s));
    if (spectrum) HIPCK(hipMemcpyAsync(spectrum, d, ((size_t)G + 1) * 8, hipMemcpyDeviceToHost, s));
    if (genome_total && G) HIPCK(hipMemcpyAsync(genome_total, d + G + 1, (size_t)G * 8, hipMemcpyDeviceToHost, s));
    if (genome_private && G) HIPCK(hipMemcpyAsync(genome_private, d + 2 * (size_t)G + 1, (size_t)G * 8, hipMemcpyDeviceToHost, s));
    HIPCK(hipStreamSynchronize(s));
    return BFT_GPU_OK;
}
