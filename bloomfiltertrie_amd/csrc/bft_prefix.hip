// bft_prefix.hip -- batched prefix matching over the sorted T-form table (prefix_matching, reference include/bft.h:135,
// src/bft.c:1087-1147; the reference walks its containers depth first, src/presenceNode.c:1923-2448).
//
// A prefix's answer is a range of `tk` (bft_prefix_range, bft_walk.h), filtered on one 2-bit field when the prefix ends inside a block.
// The batch is worked as ONE stream of candidates -- the concatenation of every prefix's interval -- so that one prefix with 10^7 rows and
// 10^6 prefixes with a handful each spread over every CU alike:
//   k_pm_bounds   one lane per prefix: interval [a, b) by lower / upper bound over tk, its filter, b - a candidates, and the kept count where
//                 no filter applies (b - a); the caller scans the candidate counts into candidate offsets
//   k_pm_count    the candidates cut into one contiguous chunk per workgroup; tiles of 256 candidates, the filter tested per lane and the
//                 kept lanes counted per wavefront (__ballot, __popcll): filtered prefixes get their kept counts by one atomic per prefix
//                 and wavefront, every chunk its total; the caller scans both (per-prefix offsets, chunk offsets)
//   k_pm_emit     the chunks again: a kept candidate's output slot is its chunk's offset + the kept lanes before it (wavefront ballots,
//                 wavefront totals in LDS); rows and colour sets are stored straight, the packed k-mers (B bytes, rarely a multiple of 4)
//                 are staged in LDS and written back as whole dwords
// Nothing here depends on the number of candidates on the host: the chunk size is derived on the device from the last candidate offset,
// so a *_dev call does not synchronise.
#include "bft_dev.h"
#include "bft_handle.h"
#include "bft_image.h"
#include "bft_kernels_load.h"
#include "bft_prefix.h"
#include "bft_scan.h"
#include "bft_walk.h"

namespace {

constexpr int PM_WAVES = PM_THREADS / 64;  // (PM_THREADS, pm_chunk: bft_prefix.h)
constexpr uint32_t PM_NOFILT = 0xFFFFFFFFu;

__device__ __forceinline__ uint64_t lanes_below(uint32_t lane) { return lane ? (~0ull >> (64 - lane)) : 0ull; }  // lane in [0, 64]

// filter word: value (2 bits) | shift inside the row's word (6 bits) << 2 | the word (most significant = 0) << 8
template <int W>
__global__ __launch_bounds__(PM_THREADS) void k_pm_bounds(const uint8_t* __restrict__ prefixes, const uint8_t* __restrict__ lengths, uint64_t n, int k, int B,
                                                          const uint64_t* __restrict__ tk, uint32_t n_rows, uint32_t* __restrict__ a_out,
                                                          uint32_t* __restrict__ filt_out, uint64_t* __restrict__ cand, uint64_t* __restrict__ kept) {
    const uint64_t end_aligned = ((uint64_t)prefixes + n * (uint64_t)B) & ~3ull;
    for (uint64_t i = blockIdx.x * (uint64_t)PM_THREADS + threadIdx.x; i < n; i += (uint64_t)gridDim.x * PM_THREADS) {
        uint64_t x[W], lo[W], hi[W];
        load_x<W>(prefixes, i, B, end_aligned, x);
        int fsh = -1;
        uint32_t fval = 0, a = 0, b = 0;
        if (bft_prefix_range<W>(x, k, lengths[i], lo, hi, &fsh, &fval)) {
            a = bft_rows_lower_bound<W>(tk, n_rows, lo);
            b = a < n_rows ? a + bft_rows_upper_bound<W>(tk + (uint64_t)a * W, n_rows - a, hi) : a;
        }
        a_out[i] = a;
        filt_out[i] = fsh < 0 ? PM_NOFILT : fval | ((uint32_t)(fsh & 63) << 2) | ((uint32_t)(W - 1 - (fsh >> 6)) << 8);
        cand[i] = b - a;
        kept[i] = fsh < 0 ? b - a : 0;
    }
}

// The candidates of one tile of a chunk: which prefix candidate j belongs to (the last i with coff[i] <= j), its row, whether it is kept.
// Two lanes find the prefixes of the tile's first and last candidates over all of coff; every lane then searches between those two.
struct PmLane {
    uint64_t i;
    uint32_t row;
    bool live, kept, filtered;
};
template <int W>
__device__ __forceinline__ PmLane pm_lane(uint64_t j0, uint64_t end, const uint64_t* __restrict__ coff, uint64_t n, const uint32_t* __restrict__ a_in,
                                          const uint32_t* __restrict__ filt, const uint64_t* __restrict__ tk, uint64_t* s_span) {
    const uint32_t tid = threadIdx.x;
    const uint64_t last = min(j0 + PM_THREADS, end) - 1;
    if (tid == 0 || tid == PM_THREADS - 1) {
        const uint64_t j = tid == 0 ? j0 : last;
        uint64_t lo = 0, hi = n - 1;
        while (lo < hi) {
            const uint64_t mid = (lo + hi + 1) >> 1;
            if (coff[mid] <= j) lo = mid;
            else hi = mid - 1;
        }
        s_span[tid == 0 ? 0 : 1] = lo;
    }
    __syncthreads();
    PmLane r{0, 0, false, false, false};
    const uint64_t j = j0 + tid;
    uint64_t lo = s_span[0], hi = s_span[1];
    __syncthreads();  // (s_span is rewritten by the next tile)
    if (j > last) return r;
    while (lo < hi) {
        const uint64_t mid = (lo + hi + 1) >> 1;
        if (coff[mid] <= j) lo = mid;
        else hi = mid - 1;
    }
    r.live = true;
    r.i = lo;
    r.row = a_in[lo] + (uint32_t)(j - coff[lo]);
    const uint32_t f = filt[lo];
    r.filtered = f != PM_NOFILT;
    if (!r.filtered) r.kept = true;
    else {
        const uint32_t wsel = f >> 8;
        uint64_t v = 0;
#pragma unroll
        for (int w = 0; w < W; w++)
            if ((uint32_t)w == wsel) v = tk[(uint64_t)r.row * W + w];
        r.kept = ((v >> ((f >> 2) & 63u)) & 3u) == (f & 3u);
    }
    return r;
}

template <int W>
__global__ __launch_bounds__(PM_THREADS) void k_pm_count(const uint64_t* __restrict__ coff, uint64_t n, const uint32_t* __restrict__ a_in,
                                                         const uint32_t* __restrict__ filt, const uint64_t* __restrict__ tk, unsigned long long* __restrict__ kept,
                                                         uint64_t* __restrict__ chunk_cnt) {
    __shared__ uint64_t s_span[2];
    __shared__ uint64_t s_wave[PM_WAVES];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint64_t begin, end;
    pm_chunk(coff[n], blockIdx.x, gridDim.x, &begin, &end);
    uint64_t total = 0;  // kept candidates of the wavefront's lanes
    for (uint64_t j0 = begin; j0 < end; j0 += PM_THREADS) {
        const PmLane c = pm_lane<W>(j0, end, coff, n, a_in, filt, tk, s_span);
        const uint64_t kept_m = __ballot(c.kept);
        total += (uint64_t)__popcll(kept_m);
        // filtered prefixes: the first lane of each prefix's run inside the wavefront adds the run's kept lanes
        const uint64_t prev_i = __shfl_up(c.i, 1);
        const bool head = c.live && (lane == 0 || prev_i != c.i);
        const uint64_t heads = __ballot(head);
        if (head && c.filtered) {
            const uint64_t above = heads & ~lanes_below(lane + 1);  // heads of the runs after this one
            const uint64_t run = lanes_below(above ? (uint32_t)__builtin_ctzll(above) : 64u) & ~lanes_below(lane);
            const uint32_t cnt = (uint32_t)__popcll(kept_m & run);
            if (cnt) atomicAdd(&kept[c.i], (unsigned long long)cnt);
        }
    }
    if (lane == 0) s_wave[wave] = total;
    __syncthreads();
    if (tid == 0) {
        uint64_t t = 0;
        for (int w = 0; w < PM_WAVES; w++) t += s_wave[w];
        chunk_cnt[blockIdx.x] = t;
    }
}

template <int W>
__global__ __launch_bounds__(PM_THREADS) void k_pm_emit(const uint64_t* __restrict__ coff, uint64_t n, const uint32_t* __restrict__ a_in,
                                                        const uint32_t* __restrict__ filt, const uint64_t* __restrict__ tk, const uint32_t* __restrict__ tcol,
                                                        const uint64_t* __restrict__ chunk_off, int k, int B, uint64_t cap, uint8_t* __restrict__ kmers_out,
                                                        uint32_t* __restrict__ rows_out, uint32_t* __restrict__ cs_out) {
    __shared__ uint64_t s_span[2];
    __shared__ uint32_t s_wave[PM_WAVES];
    __shared__ uint8_t s_kmers[PM_THREADS * BFT_MAX_W * 8];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint64_t begin, end;
    pm_chunk(coff[n], blockIdx.x, gridDim.x, &begin, &end);
    uint64_t base = chunk_off[blockIdx.x];  // output slot of the chunk's first kept candidate
    for (uint64_t j0 = begin; j0 < end && base < cap; j0 += PM_THREADS) {
        const PmLane c = pm_lane<W>(j0, end, coff, n, a_in, filt, tk, s_span);
        const uint64_t kept_m = __ballot(c.kept);
        if (lane == 0) s_wave[wave] = (uint32_t)__popcll(kept_m);
        __syncthreads();
        uint32_t before = 0, tile = 0;
#pragma unroll
        for (int w = 0; w < PM_WAVES; w++) {
            before += (uint32_t)w < wave ? s_wave[w] : 0u;
            tile += s_wave[w];
        }
        const uint32_t rank = before + (uint32_t)__popcll(kept_m & lanes_below(lane));
        const uint64_t pos = base + rank;
        if (c.kept && pos < cap) {
            if (rows_out) rows_out[pos] = c.row;
            if (cs_out) cs_out[pos] = tcol[c.row];
            if (kmers_out) {
                uint64_t t[W], x[W];
                bft_load_row<W>(tk + (uint64_t)c.row * W, t);
                bft_x_from_tform<W>(t, k, x);
                for (int b = 0; b < B; b++) {
                    uint64_t v = 0;
#pragma unroll
                    for (int w = 0; w < W; w++)
                        if (w == (b >> 3)) v = x[w];
                    s_kmers[rank * B + b] = (uint8_t)(v >> (8 * (b & 7)));
                }
            }
        }
        if (kmers_out) {  // the tile's k-mers are one contiguous span of the output: whole dwords, a few bytes at either end
            __syncthreads();
            const uint64_t m = min((uint64_t)tile, cap - base);
            uint8_t* dst = kmers_out + base * (uint64_t)B;
            const uint32_t nbytes = (uint32_t)(m * (uint64_t)B);
            const uint32_t head = min(nbytes, (uint32_t)((4u - ((uintptr_t)dst & 3u)) & 3u));
            const uint32_t ndw = (nbytes - head) >> 2, tail = head + 4 * ndw;
            if (tid < head) dst[tid] = s_kmers[tid];
            if (tid < nbytes - tail) dst[tail + tid] = s_kmers[tail + tid];
            uint32_t* dw = reinterpret_cast<uint32_t*>(dst + head);
            for (uint32_t d = tid; d < ndw; d += PM_THREADS) {
                const uint32_t o = head + 4 * d;
                dw[d] = (uint32_t)s_kmers[o] | ((uint32_t)s_kmers[o + 1] << 8) | ((uint32_t)s_kmers[o + 2] << 16) | ((uint32_t)s_kmers[o + 3] << 24);
            }
        }
        __syncthreads();  // (s_wave and s_kmers are rewritten by the next tile)
        base += tile;
    }
}

}  // namespace

int bft_pm_bounds(int W, const uint8_t* d_prefixes, const uint8_t* d_lengths, uint64_t n, int k, int B, const uint64_t* d_tk, uint64_t n_rows,
                  const BftPmScratch& p, hipStream_t s) {
    if (n == 0) return 0;
    const dim3 grid(bft_grid_for((n + PM_THREADS - 1) / PM_THREADS)), block(PM_THREADS);
    const uint32_t nr = (uint32_t)n_rows;
    switch (W) {
    case 1: hipLaunchKernelGGL(k_pm_bounds<1>, grid, block, 0, s, d_prefixes, d_lengths, n, k, B, d_tk, nr, p.a, p.filt, p.cand, p.kept); break;
    case 2: hipLaunchKernelGGL(k_pm_bounds<2>, grid, block, 0, s, d_prefixes, d_lengths, n, k, B, d_tk, nr, p.a, p.filt, p.cand, p.kept); break;
    case 3: hipLaunchKernelGGL(k_pm_bounds<3>, grid, block, 0, s, d_prefixes, d_lengths, n, k, B, d_tk, nr, p.a, p.filt, p.cand, p.kept); break;
    default: hipLaunchKernelGGL(k_pm_bounds<4>, grid, block, 0, s, d_prefixes, d_lengths, n, k, B, d_tk, nr, p.a, p.filt, p.cand, p.kept); break;
    }
    HIPCK(hipGetLastError());
    return 0;
}

int bft_pm_count(int W, uint64_t n, const uint64_t* d_tk, const BftPmScratch& p, hipStream_t s) {
    if (n == 0) return 0;
    const dim3 grid(BFT_PM_CHUNKS), block(PM_THREADS);
    unsigned long long* kept = reinterpret_cast<unsigned long long*>(p.kept);
    switch (W) {
    case 1: hipLaunchKernelGGL(k_pm_count<1>, grid, block, 0, s, p.coff, n, p.a, p.filt, d_tk, kept, p.chunk); break;
    case 2: hipLaunchKernelGGL(k_pm_count<2>, grid, block, 0, s, p.coff, n, p.a, p.filt, d_tk, kept, p.chunk); break;
    case 3: hipLaunchKernelGGL(k_pm_count<3>, grid, block, 0, s, p.coff, n, p.a, p.filt, d_tk, kept, p.chunk); break;
    default: hipLaunchKernelGGL(k_pm_count<4>, grid, block, 0, s, p.coff, n, p.a, p.filt, d_tk, kept, p.chunk); break;
    }
    HIPCK(hipGetLastError());
    return 0;
}

int bft_pm_emit(int W, uint64_t n, int k, int B, const uint64_t* d_tk, const uint32_t* d_tcol, const BftPmScratch& p, uint64_t cap, uint8_t* d_kmers_out,
                uint32_t* d_rows_out, uint32_t* d_cs_out, hipStream_t s) {
    if (n == 0 || cap == 0 || (!d_kmers_out && !d_rows_out && !d_cs_out)) return 0;
    const dim3 grid(BFT_PM_CHUNKS), block(PM_THREADS);
    switch (W) {
    case 1: hipLaunchKernelGGL(k_pm_emit<1>, grid, block, 0, s, p.coff, n, p.a, p.filt, d_tk, d_tcol, p.chunk_off, k, B, cap, d_kmers_out, d_rows_out, d_cs_out); break;
    case 2: hipLaunchKernelGGL(k_pm_emit<2>, grid, block, 0, s, p.coff, n, p.a, p.filt, d_tk, d_tcol, p.chunk_off, k, B, cap, d_kmers_out, d_rows_out, d_cs_out); break;
    case 3: hipLaunchKernelGGL(k_pm_emit<3>, grid, block, 0, s, p.coff, n, p.a, p.filt, d_tk, d_tcol, p.chunk_off, k, B, cap, d_kmers_out, d_rows_out, d_cs_out); break;
    default: hipLaunchKernelGGL(k_pm_emit<4>, grid, block, 0, s, p.coff, n, p.a, p.filt, d_tk, d_tcol, p.chunk_off, k, B, cap, d_kmers_out, d_rows_out, d_cs_out); break;
    }
    HIPCK(hipGetLastError());
    return 0;
}

// Test hook (tests/test_prefix_cases_host.py, tests/test_gpu_prefix_edges.py): how k_pm_count / k_pm_emit cut C candidates into their
// BFT_PM_CHUNKS chunks (pm_chunk, bft_prefix.h).  out: the chunk size, then [begin, end) of chunk `chunk`.  No handle, no HIP call.
extern "C" int bft_gpu_debug_prefix_plan(uint64_t C, uint32_t chunk, uint64_t out[3]) {
    if (!out) return bft_fail(BFT_GPU_E_ARG, "NULL argument");
    if (chunk >= BFT_PM_CHUNKS) return bft_fail(BFT_GPU_E_ARG, "no such chunk");
    pm_chunk(C, chunk, BFT_PM_CHUNKS, &out[1], &out[2], &out[0]);
    return BFT_GPU_OK;
}

// ------------------------------------------------------------------------------------------------
// the C-ABI entry points: the handle's scratch, the chain of launches, the host-buffer form
// ------------------------------------------------------------------------------------------------
// the arrays of a block with room for m prefixes, from `base` on; returns the block's size
static size_t pm_carve(uint64_t m, uint8_t* base, BftPmScratch* p) {
    Carver c{base};
    c.take(p->a, m * 4);
    c.take(p->filt, m * 4);
    c.take(p->cand, m * 8);
    c.take(p->kept, m * 8);
    c.take(p->coff, (m + 1) * 8);
    c.take(p->chunk, BFT_PM_CHUNKS * 8ull);
    c.take(p->chunk_off, (BFT_PM_CHUNKS + 1) * 8ull);
    return c.off;
}
// The handle's scratch (h->pm: HandleScratch, bft_handle.h) for a batch of n prefixes on stream s; a new block has room for half as many again.
static int pm_scratch(bft_gpu* h, HandleScratch::Lease& lease, uint64_t n, hipStream_t s, bool capturing, BftPmScratch* p) {
    CK(lease.acquire(s, capturing));
    const size_t tb = bft_scan::scratch_bytes(std::max<uint64_t>(n, BFT_PM_CHUNKS) + 1);
    if (h->pm_n < n) h->pm_n = n + n / 2;
    CK(h->pm.grow(h->pm_buf, pm_carve(h->pm_n, nullptr, p), 0));
    CK(h->pm.grow(h->pm_tmp, tb, tb / 2));
    pm_carve(h->pm_n, h->pm_buf.as<uint8_t>(), p);
    return 0;
}
// intervals, candidate offsets, matches per prefix -> d_offsets (n + 1; d_offsets[n] = total, also written to d_needed when it is not NULL) and
// the chunk offsets the emit reads; every launch is timed ("timing")
static int pm_count(bft_gpu* h, const uint8_t* d_pref, const uint8_t* d_len, uint64_t n, uint64_t* d_offsets, uint64_t* d_needed, hipStream_t s,
                    const BftPmScratch& p) {
    const uint64_t* tk = h->d_tk.as<uint64_t>();
    CK(bft_timed_launch(h, s, [&] { return bft_pm_bounds(h->W, d_pref, d_len, n, h->k, h->B, tk, h->n_kmers, p, s); }));
    CK(bft_timed_launch(h, s, [&] { return bft_scan::exclusive_sum_ptr<uint64_t>(p.cand, p.coff, n, s, h->pm_tmp, nullptr, true); }));
    CK(bft_timed_launch(h, s, [&] { return bft_pm_count(h->W, n, tk, p, s); }));
    CK(bft_timed_launch(h, s, [&] { return bft_scan::exclusive_sum_ptr<uint64_t>(p.kept, d_offsets, n, s, h->pm_tmp, (unsigned long long*)d_needed, true); }));
    CK(bft_timed_launch(h, s, [&] { return bft_scan::exclusive_sum_ptr<uint64_t>(p.chunk, p.chunk_off, BFT_PM_CHUNKS, s, h->pm_tmp, nullptr, true); }));
    return 0;
}
static int pm_emit(bft_gpu* h, uint64_t n, const BftPmScratch& p, uint64_t cap, uint8_t* d_kmers, uint32_t* d_rows, uint32_t* d_cs, hipStream_t s) {
    if (cap == 0 || (!d_kmers && !d_rows && !d_cs)) return 0;
    return bft_timed_launch(h, s, [&] { return bft_pm_emit(h->W, n, h->k, h->B, h->d_tk.as<uint64_t>(), h->d_tcol.as<uint32_t>(), p, cap, d_kmers, d_rows, d_cs, s); });
}

extern "C" int bft_gpu_query_prefixes_dev(bft_gpu* h, const void* d_prefixes, const void* d_lengths, uint64_t n, void* d_offsets, void* d_kmers_out,
                                          void* d_rows_out, void* d_colorsets_out, uint64_t cap, void* d_needed, void* hip_stream) {
    if (!h || !d_offsets || ((!d_prefixes || !d_lengths) && n)) return bft_fail(BFT_GPU_E_ARG, "NULL argument");
    ENTER(h);
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : h->stream;
    const bool capturing = bft_stream_capturing(s);
    CK(bft_ensure_built(h, false));
    if (h->table_dropped) {  // ("compact_table": the rows come from the sorted table; bringing it back synchronises)
        if (capturing) return bft_fail(BFT_GPU_E_ARG, "prefix query recorded into a graph: the sorted table is not resident (compact_table); make one direct call first");
        CK(bft_ensure_table(h));
    }
    if (n == 0) {
        CK(bft_zero_async(d_offsets, 8, s));  // (kernels, not memsets, wherever a caller may be capturing: bft_dev.h)
        if (d_needed) CK(bft_zero_async(d_needed, 8, s));
        return bft_note_foreign_stream(h, s);
    }
    {
        HandleScratch::Lease lease(h->pm);
        BftPmScratch p;
        CK(pm_scratch(h, lease, n, s, capturing, &p));
        CK(pm_count(h, (const uint8_t*)d_prefixes, (const uint8_t*)d_lengths, n, (uint64_t*)d_offsets, (uint64_t*)d_needed, s, p));
        CK(pm_emit(h, n, p, cap, (uint8_t*)d_kmers_out, (uint32_t*)d_rows_out, (uint32_t*)d_colorsets_out, s));
    }
    return bft_note_foreign_stream(h, s);
}

// The host-buffer form: lengths are checked first, the matches counted on the device, and the outputs filled only when cap holds them all.
extern "C" int bft_gpu_query_prefixes(bft_gpu* h, const uint8_t* prefixes, const uint8_t* lengths, uint64_t n, uint64_t* offsets, uint8_t* kmers_out,
                                      uint32_t* rows_out, uint32_t* colorsets_out, uint64_t cap, uint64_t* needed) {
    if (!h || !offsets || ((!prefixes || !lengths) && n)) return bft_fail(BFT_GPU_E_ARG, "NULL argument");
    for (uint64_t i = 0; i < n; i++)
        if (lengths[i] < 1 || lengths[i] > h->k) return bft_fail(BFT_GPU_E_ARG, "prefix length outside [1, k]");
    ENTER(h);
    CK(bft_ensure_built(h));
    if (n == 0) {
        offsets[0] = 0;
        if (needed) *needed = 0;
        return BFT_GPU_OK;
    }
    const hipStream_t s = h->stream;
    DevBuf dp, dl, doff, dneed;
    CK(dp.alloc(n * h->B));
    CK(dl.alloc(n));
    CK(doff.alloc((n + 1) * 8));
    CK(dneed.alloc(8));
    HIPCK(hipMemcpyAsync(dp.p, prefixes, n * h->B, hipMemcpyHostToDevice, s));
    HIPCK(hipMemcpyAsync(dl.p, lengths, n, hipMemcpyHostToDevice, s));
    HandleScratch::Lease lease(h->pm);
    BftPmScratch p;
    CK(pm_scratch(h, lease, n, s, false, &p));
    CK(pm_count(h, dp.as<uint8_t>(), dl.as<uint8_t>(), n, doff.as<uint64_t>(), dneed.as<uint64_t>(), s, p));
    uint64_t total = 0;
    HIPCK(hipMemcpyAsync(&total, dneed.p, 8, hipMemcpyDeviceToHost, s));
    HIPCK(hipStreamSynchronize(s));
    if (needed) *needed = total;
    const bool want = kmers_out || rows_out || colorsets_out;
    if (want && total > cap) return bft_fail(BFT_GPU_E_NOSPACE, "prefix match buffers too small");
    if (want && total) {
        DevBuf dk, dr, dc;
        if (kmers_out) CK(dk.alloc(total * h->B));
        if (rows_out) CK(dr.alloc(total * 4));
        if (colorsets_out) CK(dc.alloc(total * 4));
        CK(pm_emit(h, n, p, total, dk.as<uint8_t>(), dr.as<uint32_t>(), dc.as<uint32_t>(), s));
        if (kmers_out) HIPCK(hipMemcpyAsync(kmers_out, dk.p, total * h->B, hipMemcpyDeviceToHost, s));
        if (rows_out) HIPCK(hipMemcpyAsync(rows_out, dr.p, total * 4, hipMemcpyDeviceToHost, s));
        if (colorsets_out) HIPCK(hipMemcpyAsync(colorsets_out, dc.p, total * 4, hipMemcpyDeviceToHost, s));
    }
    HIPCK(hipMemcpyAsync(offsets, doff.p, (n + 1) * 8, hipMemcpyDeviceToHost, s));
    HIPCK(hipStreamSynchronize(s));
    return BFT_GPU_OK;
}
