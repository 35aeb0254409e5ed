// bft_union.hip -- merging two indexes into a new one (merging_BFT, reference include/merge.h:14; its body in src/merge.c is commented out upstream):
// every k-mer of a and of b, genome g of b as genome id_base + g, a k-mer of both with the union of its two colour sets.
//
// An index is a "run" (bft_merge.h): its sorted distinct k-mers, a colour-set id per k-mer and the dictionary.  bft_merge_runs already merges two runs;
// its colour-set half is used as it is.  What differs from an insertion build is the placement of the k-mers.  A build's run is small beside its
// index, so every run row searches the index.  Two indexes are of similar size: 26 dependent gathers for each of 2x10^7 rows, on a chip where a gather
// pays per line requested.  Here both tables are streamed instead, co-ranked tile by tile:
//   k_un_split   one thread per tile boundary: the split (i, j), i + j = t x BFT_UNION_TILE, of the stable merge (a's row first among equals) by a
//                search along the diagonal; a pair of equal keys the boundary would part goes whole into the earlier tile (j + 1)
//   k_un_count   one workgroup per tile: both slices into LDS, every row of b searched in a's slice THERE; the tile's number of distinct keys
//   (bft_scan: where every tile's rows start)
//   k_un_emit    the same staging and search, then every row of a and every row of b that a does not hold goes to its place: the tile's start +
//                its rank in its own slice + the rows of the other slice below it (b's: only those a does not hold, by ballot words kept in LDS)
//   k_un_shift   the genome ids of b's dictionary widened to 32 bits and shifted by id_base in one pass
// No atomics on global memory; LDS: (BFT_UNION_TILE + 1) x 8 W bytes of keys and 17 ballot words.
#include "bft_union.h"

#include "bft_handle.h"
#include "bft_merge.h"
#include "bft_scan.h"
#include "bft_walk.h"

namespace {

constexpr uint32_t UT = BFT_UNION_TILE, UTHREADS = BFT_UNION_THREADS;
constexpr uint32_t UCH = (UT + 1) / 64 + 1;                  // 64-row chunks of a slice of b (at most UT + 1 rows), and one for a rank of UT + 1
constexpr uint32_t UROUNDS = (UCH + UTHREADS / 64 - 1) / (UTHREADS / 64);  // chunks per wavefront
constexpr uint32_t UNONE = 0xFFFFFFFFu;
static_assert(UT % 64 == 0 && UT >= UTHREADS && UT < (1u << 30), "tile: whole wavefronts, ranks that fit 31 bits");

__device__ __forceinline__ uint64_t un_below(uint32_t lane) { return lane ? (~0ull >> (64 - lane)) : 0ull; }

// Rows of a among the first d rows of the stable merge (a's row first among equals); *oj: rows of b, one more when that parts a pair of equal keys
template <int W>
__device__ __forceinline__ uint32_t un_split(const uint64_t* __restrict__ tk_a, uint32_t n_a, const uint64_t* __restrict__ tk_b, uint32_t n_b, uint64_t d, uint32_t* oj) {
    uint32_t lo = d > n_b ? (uint32_t)(d - n_b) : 0u, hi = (uint32_t)min((uint64_t)n_a, d);
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;  // (lo + hi < 2^32: both are below 2^31)
        uint64_t x[W], y[W];
        bft_load_row<W>(tk_a + (uint64_t)mid * W, x);
        bft_load_row<W>(tk_b + (d - 1 - mid) * W, y);
        if (bft_cmp<W>(x, y) <= 0) lo = mid + 1; else hi = mid;
    }
    uint32_t j = (uint32_t)(d - lo);
    if (lo > 0 && j < n_b) {
        uint64_t x[W], y[W];
        bft_load_row<W>(tk_a + (uint64_t)(lo - 1) * W, x);
        bft_load_row<W>(tk_b + (uint64_t)j * W, y);
        if (bft_cmp<W>(x, y) == 0) j++;
    }
    *oj = j;
    return lo;
}

template <int W>
__global__ __launch_bounds__(UTHREADS) void k_un_split(const uint64_t* __restrict__ tk_a, uint32_t n_a, const uint64_t* __restrict__ tk_b, uint32_t n_b, uint32_t n_tiles,
                                                       uint32_t* __restrict__ si, uint32_t* __restrict__ sj) {
    const uint32_t t = blockIdx.x * UTHREADS + threadIdx.x;
    if (t > n_tiles) return;
    const uint64_t d = min((uint64_t)t * UT, (uint64_t)n_a + n_b);
    uint32_t j;
    si[t] = un_split<W>(tk_a, n_a, tk_b, n_b, d, &j);
    sj[t] = j;
}

// One tile: its slices of a (rows [0, na) of s_key) and of b (rows [na, na + nb)) staged, every row of b ranked in a's slice.
// found[r]: for row y = (wave + 4 r) x 64 + lane of b's slice, its rank in a's slice | 1 << 31 when a holds the key.
// s_word[c]: the rows of chunk c of b's slice that a does not hold, a bit per row.
template <int W>
__device__ __forceinline__ void un_stage_rank(const uint64_t* __restrict__ tk_a, const uint64_t* __restrict__ tk_b, uint32_t i0, uint32_t na, uint32_t j0, uint32_t nb,
                                              uint64_t* s_key, unsigned long long* s_word, uint32_t (&found)[UROUNDS]) {
    const uint64_t* ga = tk_a + (uint64_t)i0 * W;
    const uint64_t* gb = tk_b + (uint64_t)j0 * W;
    for (uint32_t q = threadIdx.x; q < na * W; q += UTHREADS) s_key[q] = ga[q];
    for (uint32_t q = threadIdx.x; q < nb * W; q += UTHREADS) s_key[na * W + q] = gb[q];
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
    for (uint32_t r = 0; r < UROUNDS; r++) {
        const uint32_t c = wave + (UTHREADS / 64) * r, y = c * 64 + lane;
        uint32_t lo = 0;
        bool eq = false;
        if (y < nb) {
            uint64_t t[W];
#pragma unroll
            for (int w = 0; w < W; w++) t[w] = s_key[(na + y) * W + w];
            uint32_t hi = na;
            while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                int cmp = 0;
#pragma unroll
                for (int w = 0; w < W; w++) {
                    const uint64_t v = s_key[mid * W + w];
                    if (cmp == 0) cmp = v < t[w] ? -1 : (v > t[w] ? 1 : 0);
                }
                if (cmp < 0) lo = mid + 1; else hi = mid;
            }
            if (lo < na) {
                eq = true;
#pragma unroll
                for (int w = 0; w < W; w++) eq = eq && s_key[lo * W + w] == t[w];
            }
        }
        found[r] = lo | (eq ? 0x80000000u : 0u);
        const unsigned long long word = __ballot(y < nb && !eq);
        if (lane == 0 && c < UCH) s_word[c] = word;
    }
    __syncthreads();
}

template <int W>
__global__ __launch_bounds__(UTHREADS) void k_un_count(const uint64_t* __restrict__ tk_a, const uint64_t* __restrict__ tk_b, const uint32_t* __restrict__ si,
                                                       const uint32_t* __restrict__ sj, uint32_t* __restrict__ cnt) {
    __shared__ uint64_t s_key[(UT + 1) * W];
    __shared__ unsigned long long s_word[UCH];
    const uint32_t t = blockIdx.x, i0 = si[t], j0 = sj[t], na = si[t + 1] - i0, nb = sj[t + 1] - j0;
    uint32_t found[UROUNDS];
    un_stage_rank<W>(tk_a, tk_b, i0, na, j0, nb, s_key, s_word, found);
    if (threadIdx.x == 0) {
        uint32_t only_b = 0;
        for (uint32_t c = 0; c < UCH; c++) only_b += (uint32_t)__popcll(s_word[c]);
        cnt[t] = na + only_b;
    }
}

template <int W>
__global__ __launch_bounds__(UTHREADS) void k_un_emit(const uint64_t* __restrict__ tk_a, const uint32_t* __restrict__ tcol_a, const uint64_t* __restrict__ tk_b,
                                                      const uint32_t* __restrict__ tcol_b, const uint32_t* __restrict__ si, const uint32_t* __restrict__ sj,
                                                      const uint32_t* __restrict__ start, uint64_t* __restrict__ tk_o, uint32_t* __restrict__ pa, uint32_t* __restrict__ pb,
                                                      uint32_t* __restrict__ orow) {
    __shared__ uint64_t s_key[(UT + 1) * W];
    __shared__ unsigned long long s_word[UCH];
    __shared__ uint32_t s_cbase[UCH];
    const uint32_t t = blockIdx.x, i0 = si[t], j0 = sj[t], na = si[t + 1] - i0, nb = sj[t + 1] - j0;
    const uint64_t base = start[t];
    uint32_t found[UROUNDS];
    un_stage_rank<W>(tk_a, tk_b, i0, na, j0, nb, s_key, s_word, found);
    if (threadIdx.x == 0) {
        uint32_t acc = 0;
        for (uint32_t c = 0; c < UCH; c++) { s_cbase[c] = acc; acc += (uint32_t)__popcll(s_word[c]); }
    }
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    // rows of b: one that a does not hold sits behind the rows of a below it and the earlier rows of b that a does not hold; one that a holds sits
    // on a's row, which has the same rows in front of it
#pragma unroll
    for (uint32_t r = 0; r < UROUNDS; r++) {
        const uint32_t c = wave + (UTHREADS / 64) * r, y = c * 64 + lane;
        if (y >= nb) continue;
        const uint32_t la = found[r] & 0x7FFFFFFFu;
        const uint64_t o = base + la + s_cbase[c] + (uint32_t)__popcll(s_word[c] & un_below(lane));
        orow[j0 + y] = (uint32_t)o;
        if (!(found[r] >> 31)) {
#pragma unroll
            for (int w = 0; w < W; w++) tk_o[o * W + w] = s_key[(na + y) * W + w];
            pa[o] = UNONE;
            pb[o] = tcol_b[j0 + y];
        }
    }
    // rows of a: behind the earlier rows of a and the rows of b below it that a does not hold
    for (uint32_t x = threadIdx.x; x < na; x += UTHREADS) {
        uint64_t k[W];
#pragma unroll
        for (int w = 0; w < W; w++) k[w] = s_key[x * W + w];
        uint32_t lo = 0, hi = nb;
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            int cmp = 0;
#pragma unroll
            for (int w = 0; w < W; w++) {
                const uint64_t v = s_key[(na + mid) * W + w];
                if (cmp == 0) cmp = v < k[w] ? -1 : (v > k[w] ? 1 : 0);
            }
            if (cmp < 0) lo = mid + 1; else hi = mid;
        }
        bool eq = lo < nb;
        if (eq) {
#pragma unroll
            for (int w = 0; w < W; w++) eq = eq && s_key[(na + lo) * W + w] == k[w];
        }
        const uint32_t c = lo >> 6;  // (lo <= nb <= UT + 1: c < UCH)
        const uint64_t o = base + x + s_cbase[c] + (uint32_t)__popcll(s_word[c] & un_below(lo & 63u));
#pragma unroll
        for (int w = 0; w < W; w++) tk_o[o * W + w] = k[w];
        pa[o] = tcol_a[i0 + x];
        pb[o] = eq ? tcol_b[j0 + lo] : UNONE;
    }
}

template <class T>
__global__ __launch_bounds__(UTHREADS) void k_un_shift(const T* __restrict__ in, uint64_t n, uint32_t base, uint32_t* __restrict__ out) {
    for (uint64_t i = blockIdx.x * (uint64_t)UTHREADS + threadIdx.x; i < n; i += (uint64_t)gridDim.x * UTHREADS) out[i] = (uint32_t)in[i] + base;
}

template <class F>
int un_launch(bft_gpu* timed, hipStream_t s, F&& launch) {
    if (timed) return bft_timed_launch(timed, s, launch);
    return launch();
}

template <int W>
int place_w(const BftRun& a, const BftRun& b, hipStream_t s, bft_gpu* timed, DevBuf& tk, DevBuf& pa, DevBuf& pb, DevBuf& orow, uint64_t* n_out) {
    const uint64_t n_a = a.n, n_b = b.n;
    if (n_a == 0 || n_b == 0 || n_a >= 0x7FFFFFFFull || n_b >= 0x7FFFFFFFull) return bft_fail(BFT_GPU_E_ARG, "co-ranked placement: a side is empty or beyond 2^31-1 k-mers");
    const uint64_t n_tiles64 = (n_a + n_b + UT - 1) / UT;
    const uint32_t n_tiles = (uint32_t)n_tiles64;
    DevBuf si, sj, cnt, start, tmp;
    CK(si.alloc((n_tiles64 + 1) * 4));
    CK(sj.alloc((n_tiles64 + 1) * 4));
    CK(cnt.alloc(n_tiles64 * 4));
    CK(start.alloc((n_tiles64 + 1) * 4));
    CK(un_launch(timed, s, [&] {
        hipLaunchKernelGGL(k_un_split<W>, dim3((n_tiles + 1 + UTHREADS - 1) / UTHREADS), dim3(UTHREADS), 0, s, a.tk, (uint32_t)n_a, b.tk, (uint32_t)n_b, n_tiles, si.as<uint32_t>(),
                           sj.as<uint32_t>());
        HIPCK(hipGetLastError());
        return 0;
    }));
    CK(un_launch(timed, s, [&] {
        hipLaunchKernelGGL(k_un_count<W>, dim3(n_tiles), dim3(UTHREADS), 0, s, a.tk, b.tk, si.as<uint32_t>(), sj.as<uint32_t>(), cnt.as<uint32_t>());
        HIPCK(hipGetLastError());
        return 0;
    }));
    // (the sum stays below 2^32: at most n_a + n_b rows)
    CK(un_launch(timed, s, [&] { return bft_scan::exclusive_sum_ptr<uint32_t>(cnt.as<uint32_t>(), start.as<uint32_t>(), n_tiles, s, tmp, nullptr, true); }));
    uint32_t n_o32 = 0;
    HIPCK(hipMemcpyAsync(&n_o32, start.as<uint32_t>() + n_tiles, 4, hipMemcpyDeviceToHost, s));
    HIPCK(hipStreamSynchronize(s));
    const uint64_t n_o = n_o32;
    if (n_o < std::max(n_a, n_b) || n_o > n_a + n_b) return bft_fail(BFT_GPU_E_LIMIT, "merge self-check failed (tile counts disagree with the tables)");
    if (n_o >= 0x7FFFFFFFull) return bft_fail(BFT_GPU_E_LIMIT, "more than 2^31-1 distinct k-mers");
    CK(tk.alloc(n_o * W * 8));
    CK(pa.alloc(n_o * 4));
    CK(pb.alloc(n_o * 4));
    CK(orow.alloc(n_b * 4));
    CK(un_launch(timed, s, [&] {
        hipLaunchKernelGGL(k_un_emit<W>, dim3(n_tiles), dim3(UTHREADS), 0, s, a.tk, a.tcol, b.tk, b.tcol, si.as<uint32_t>(), sj.as<uint32_t>(), start.as<uint32_t>(),
                           tk.as<uint64_t>(), pa.as<uint32_t>(), pb.as<uint32_t>(), orow.as<uint32_t>());
        HIPCK(hipGetLastError());
        return 0;
    }));
    HIPCK(hipStreamSynchronize(s));
    *n_out = n_o;
    return 0;
}

}  // namespace

int bft_union_place(int W, const BftRun& a, const BftRun& b, hipStream_t s, bft_gpu* timed, DevBuf& tk, DevBuf& pa, DevBuf& pb, DevBuf& orow, uint64_t* n_o) {
    switch (W) {
    case 1: return place_w<1>(a, b, s, timed, tk, pa, pb, orow, n_o);
    case 2: return place_w<2>(a, b, s, timed, tk, pa, pb, orow, n_o);
    case 3: return place_w<3>(a, b, s, timed, tk, pa, pb, orow, n_o);
    default: return place_w<4>(a, b, s, timed, tk, pa, pb, orow, n_o);
    }
}

int bft_union_shift_ids(const void* d_in, uint32_t w, uint64_t n, uint32_t base, uint32_t* d_out, hipStream_t s) {
    if (n == 0) return 0;
    const dim3 grid(bft_grid_for((n + UTHREADS - 1) / UTHREADS)), block(UTHREADS);
    if (w == 1) hipLaunchKernelGGL(k_un_shift<uint8_t>, grid, block, 0, s, (const uint8_t*)d_in, n, base, d_out);
    else if (w == 2) hipLaunchKernelGGL(k_un_shift<uint16_t>, grid, block, 0, s, (const uint16_t*)d_in, n, base, d_out);
    else hipLaunchKernelGGL(k_un_shift<uint32_t>, grid, block, 0, s, (const uint32_t*)d_in, n, base, d_out);
    HIPCK(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------------
// the C-ABI entry point: both sources whole and resident, b's dictionary shifted, the two runs merged, then the common tail of a build
// ------------------------------------------------------------------------------------------------
namespace {

uint32_t genome_count(const bft_gpu* h) {
    return std::max<uint32_t>(std::max<uint32_t>((uint32_t)h->genomes.size(), h->im.nb_genomes), h->any_insert ? h->max_gid_seen + 1 : 0);
}

// "compact_table": a source whose sorted table was away has it for the call only
struct TableLoan {
    bft_gpu* h = nullptr;
    ~TableLoan() {
        if (!h) return;
        if (bft_set_device(h) == 0) bft_drop_table(h);
    }
};

// one side as it stands (the other holds no k-mer): its table copied, its dictionary as 32-bit ids + base
int copy_side(const bft_gpu* src, uint32_t base, bft_gpu* timed, hipStream_t ds, BftRunOut& mo) {
    const uint64_t n = src->n_kmers;
    CK(mo.tk.alloc(n * src->W * 8));
    CK(mo.tcol.alloc(n * 4));
    CK(mo.cs_off.alloc((src->n_sets + 1) * 4));
    HIPCK(hipMemcpyAsync(mo.tk.p, src->d_tk.p, n * src->W * 8, hipMemcpyDeviceToDevice, ds));
    HIPCK(hipMemcpyAsync(mo.tcol.p, src->d_tcol.p, n * 4, hipMemcpyDeviceToDevice, ds));
    HIPCK(hipMemcpyAsync(mo.cs_off.p, src->d_cs_off.p, (src->n_sets + 1) * 4, hipMemcpyDeviceToDevice, ds));
    CK(bft_dict_ids32(src, base, ds, timed, mo.cs_ids, nullptr));  // (a copy of the merged image's own, whatever the width)
    mo.n = n;
    mo.n_sets = src->n_sets;
    mo.n_ids = src->n_ids;
    return 0;
}

// d: a fresh handle with a's k and seeds; everything runs on d's stream (both sources are synchronised and only read)
int merge_fill(bft_gpu* a, bft_gpu* b, uint32_t id_base, bft_gpu* d) {
    const uint32_t g_a = genome_count(a), g_b = genome_count(b);
    // names: a's, then b's for the ids beyond a's genomes (an id in between that nobody named keeps the name bft_gpu_genome_name gives an unnamed id)
    d->genomes = a->genomes;
    for (size_t g = 0; g < b->genomes.size(); g++) {
        const size_t id = (size_t)id_base + g;
        if (id < g_a) continue;
        while (d->genomes.size() < id) d->genomes.push_back("genome_" + std::to_string(d->genomes.size()));
        d->genomes.push_back(b->genomes[g]);
    }
    const uint32_t g_o = std::max<uint32_t>(g_a, id_base + g_b);
    d->any_insert = g_o > 0;
    d->max_gid_seen = g_o ? g_o - 1 : 0;
    d->opt_build_stages = a->opt_build_stages;
    CK(bft_set_device(d));  // (from here on the cache hands out blocks for d's stream)
    const hipStream_t ds = d->stream;
    StageScope stage_scope(d);
    const double t0 = bft_now_ms();
    const int W = a->W;
    const uint64_t n_a = a->n_kmers, n_b = b->n_kmers;

    BftRunOut mo;
    if (n_a && n_b) {
        DevBuf ids_a, ids_b;
        const uint32_t *a_ids = nullptr, *b_ids = nullptr;
        CK(bft_dict_ids32(a, 0u, ds, a, ids_a, &a_ids));
        CK(bft_dict_ids32(b, id_base, ds, a, ids_b, &b_ids));
        const double moved = (a_ids != a->d_cs_ids.as<uint32_t>() ? (double)a->n_ids * (a->cs_w + 4) : 0.0) + (b_ids != b->d_cs_ids.as<uint32_t>() ? (double)b->n_ids * (b->cs_w + 4) : 0.0);
        bft_stage("merge: dictionaries widened, b's ids shifted", moved, ds);
        const BftRun run_a{a->d_tk.as<uint64_t>(), a->d_tcol.as<uint32_t>(), n_a, a->d_cs_off.as<uint32_t>(), a_ids, a->n_sets};
        const BftRun run_b{b->d_tk.as<uint64_t>(), b->d_tcol.as<uint32_t>(), n_b, b->d_cs_off.as<uint32_t>(), b_ids, b->n_sets};
        BftMergeOpt opt;
        opt.coranked = a->opt_merge_place != 0;
        opt.stages = true;
        opt.timed = a;
        CK(bft_merge_runs(W, run_a, run_b, ds, mo, opt));
    } else if (n_a || n_b) {
        CK(copy_side(n_a ? a : b, n_a ? 0u : id_base, a, ds, mo));
        bft_stage("merge: one side empty, the other copied", (double)mo.n * (16.0 * W + 8) + (double)mo.n_ids * 8, ds);
    } else {
        CK(mo.tcol.alloc(4));
        CK(mo.cs_off.alloc_zero(4, ds));
        CK(mo.cs_ids.alloc(4));
    }
    uint64_t np = 0;
    CK(bft_count_pairs(mo.tcol.as<uint32_t>(), mo.n, mo.cs_off.as<uint32_t>(), ds, &np));
    HIPCK(hipStreamSynchronize(ds));
    bft_stage("merge: pairs counted", (double)mo.n * 12, ds);
    const double t1 = bft_now_ms();

    return bft_commit_image(d, mo, np, t0, t1);  // (nothing deferred: the merge interns on its own stream)
}

}  // namespace

extern "C" int bft_gpu_merge(bft_gpu* a, bft_gpu* b, uint32_t id_base, bft_gpu** out) {
    if (!a || !b || !out) return bft_fail(BFT_GPU_E_ARG, "NULL argument");
    *out = nullptr;
    if (a->k != b->k) return bft_fail(BFT_GPU_E_ARG, "merge: the two indexes differ in k (" + std::to_string(a->k) + " and " + std::to_string(b->k) + ")");
    if (a->device != b->device)
        return bft_fail(BFT_GPU_E_ARG, "merge: the two indexes are on different devices (bft_gpu_image_pack / bft_gpu_image_unpack move a handle to another device)");
    ENTER(a);
    if (bft_stream_capturing(a->stream) || bft_stream_capturing(b->stream)) return bft_fail(BFT_GPU_E_ARG, "merge recorded into a graph: it allocates and synchronises");
    // both sources whole, their sorted tables resident for the call
    TableLoan loan_a, loan_b;
    CK(bft_ensure_built(a, false));
    if (a->table_dropped) { CK(bft_ensure_table(a)); loan_a.h = a; }
    HIPCK(hipStreamSynchronize(a->stream));
    if (b != a) {
        CK(bft_set_device(b));
        CK(bft_ensure_built(b, false));
        if (b->table_dropped) { CK(bft_ensure_table(b)); loan_b.h = b; }
        HIPCK(hipStreamSynchronize(b->stream));
    }
    const uint32_t g_a = genome_count(a), g_b = genome_count(b);
    if (id_base == BFT_GPU_MERGE_APPEND) id_base = g_a;
    if (id_base > g_a) return bft_fail(BFT_GPU_E_ARG, "merge: id_base " + std::to_string(id_base) + " is beyond a's " + std::to_string(g_a) + " genomes");
    if ((uint64_t)id_base + g_b > 0xFFFFFFFFull) return bft_fail(BFT_GPU_E_LIMIT, "merge: genome ids beyond 2^32");
    bft_gpu* d = nullptr;
    CK(bft_gpu_create_seeded(a->k, a->device, a->r1, a->r2, &d));
    const int rc = merge_fill(a, b, id_base, d);
    if (rc) {
        const std::string err = bft_gpu_last_error();
        (void)hipStreamSynchronize(d->stream);  // (copies and kernels that read the sources' tables may be in flight: the loans go back after them)
        bft_gpu_free(d);
        return bft_fail(rc, err);
    }
    *out = d;
    return BFT_GPU_OK;
}
