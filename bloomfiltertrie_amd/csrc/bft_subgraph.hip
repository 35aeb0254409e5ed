// bft_subgraph.hip -- sub-graph builds (create_cdbg_from_bft_kmers, reference include/bft.h:179, src/bft.c:1353-1464): the kernels between the
// source's lookup and the common tail of a build (bft_commit_image, bft_gpu.hip), and the entry points that chain them.
//
// The canonical state of an image is the sorted T-form table tk, a colour-set id per row tcol and the dictionary cs_off / cs_ids.  A sub-graph is a
// sorted subset of tk, its tcol renumbered, and the used part of the dictionary:
//   k_sg_compact  the found k-mers of the batch (presence bit + colour-set id from the source's query kernels) as (T-form key, colour-set id)
//                 records: one atomic per wavefront for the wavefront's slots, the ranks by ballot; absent k-mers leave nothing
//   (the library's radix sort orders the records by key; the de-duplication scan's input is BftSgHeads)
//   k_sg_scatter  the first record of every run of equal keys -> its row of the new table, its colour set
//   k_sg_mark     the colour sets the new table uses (a flag per set of the source)
//   (two scans: new id of every used set, and where its list goes)
//   k_sg_remap    tcol -> the new ids
//   k_sg_dict     one wavefront per used set: its offset and its list, the ids widened to the 32 bits the build works in; the sets keep their
//                 old relative order, so the numbering is deterministic
// None of them needs scratch memory or LDS.
#include "bft_dev.h"
#include "bft_handle.h"
#include "bft_kernels_load.h"
#include "bft_merge.h"
#include "bft_scan.h"
#include "bft_subgraph.h"
#include "bft_walk.h"

namespace {

constexpr int SG_THREADS = 256;

__device__ __forceinline__ uint64_t lanes_below(uint32_t lane) { return lane ? (~0ull >> (64 - lane)) : 0ull; }

// A wavefront takes 64 consecutive k-mers: one word of presence bits.
template <int W>
__global__ __launch_bounds__(SG_THREADS) void k_sg_compact(const uint8_t* __restrict__ kmers, uint64_t n, int k, int B, const uint64_t* __restrict__ bits,
                                                           const uint32_t* __restrict__ cs, uint64_t* __restrict__ keys, uint64_t stride,
                                                           uint32_t* __restrict__ vals, unsigned long long* __restrict__ count) {
    const uint64_t end_aligned = ((uint64_t)kmers + n * (uint64_t)B) & ~3ull;
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t i0 = blockIdx.x * (uint64_t)SG_THREADS + (threadIdx.x & ~63u); i0 < n; i0 += (uint64_t)gridDim.x * SG_THREADS) {
        uint64_t word = bits[i0 >> 6];
        if (n - i0 < 64) word &= ~0ull >> (64 - (n - i0));  // (bits past the batch)
        const uint32_t cnt = (uint32_t)__popcll(word);
        unsigned long long base = 0;
        if (lane == 0 && cnt) base = atomicAdd(count, (unsigned long long)cnt);
        base = __shfl(base, 0);
        if ((word >> lane) & 1ull) {
            const uint64_t i = i0 + lane, r = base + (uint64_t)__popcll(word & lanes_below(lane));
            uint64_t x[W], t[W];
            load_x<W>(kmers, i, B, end_aligned, x);
            bft_tform_from_x<W>(x, k, t);
#pragma unroll
            for (int w = 0; w < W; w++) keys[(uint64_t)w * stride + r] = t[w];
            vals[r] = cs[i];
        }
    }
}

template <int W>
__global__ __launch_bounds__(SG_THREADS) void k_sg_scatter(const uint64_t* __restrict__ keys, uint64_t stride, const uint32_t* __restrict__ vals, uint64_t n,
                                                           const uint32_t* __restrict__ pos, uint64_t* __restrict__ tk, uint32_t* __restrict__ tcol) {
    const BftSgHeads head{keys, stride, n, W};
    for (uint64_t i = blockIdx.x * (uint64_t)SG_THREADS + threadIdx.x; i < n; i += (uint64_t)gridDim.x * SG_THREADS) {
        if (!head(i)) continue;
        const uint64_t p = pos[i];
#pragma unroll
        for (int w = 0; w < W; w++) tk[p * W + w] = keys[(uint64_t)w * stride + i];
        tcol[p] = vals[i];
    }
}

__global__ __launch_bounds__(SG_THREADS) void k_sg_mark(const uint32_t* __restrict__ tcol, uint64_t nk, uint32_t* __restrict__ used) {
    for (uint64_t r = blockIdx.x * (uint64_t)SG_THREADS + threadIdx.x; r < nk; r += (uint64_t)gridDim.x * SG_THREADS) used[tcol[r]] = 1u;
}

__global__ __launch_bounds__(SG_THREADS) void k_sg_remap(uint32_t* __restrict__ tcol, uint64_t nk, const uint32_t* __restrict__ new_id) {
    for (uint64_t r = blockIdx.x * (uint64_t)SG_THREADS + threadIdx.x; r < nk; r += (uint64_t)gridDim.x * SG_THREADS) tcol[r] = new_id[tcol[r]];
}

// wavefront j % waves takes set j; j == n_sets writes the closing offset
template <class T>
__global__ __launch_bounds__(SG_THREADS) void k_sg_dict(const uint32_t* __restrict__ used, const uint32_t* __restrict__ new_id, const uint32_t* __restrict__ id_pos,
                                                        const uint32_t* __restrict__ cs_off, const T* __restrict__ cs_ids, uint64_t n_sets,
                                                        uint32_t* __restrict__ new_off, uint32_t* __restrict__ new_ids) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t waves = (uint64_t)gridDim.x * (SG_THREADS / 64);
    for (uint64_t j = (blockIdx.x * (uint64_t)SG_THREADS + threadIdx.x) >> 6; j <= n_sets; j += waves) {
        if (j == n_sets) {
            if (lane == 0) new_off[new_id[n_sets]] = id_pos[n_sets];
            continue;
        }
        if (!used[j]) continue;
        const uint32_t a = cs_off[j], len = cs_off[j + 1] - a, dst = id_pos[j];
        if (lane == 0) new_off[new_id[j]] = dst;
        for (uint32_t t = lane; t < len; t += 64) new_ids[dst + t] = (uint32_t)cs_ids[a + t];
    }
}

}  // namespace

int bft_sg_compact(int W, const uint8_t* d_kmers, uint64_t n, int k, int B, const uint64_t* d_bits64, const uint32_t* d_cs, uint64_t* d_keys, uint64_t stride,
                   uint32_t* d_vals, unsigned long long* d_count, hipStream_t s) {
    if (n == 0) return 0;
    const dim3 grid(bft_grid_for((n + SG_THREADS - 1) / SG_THREADS)), block(SG_THREADS);
    switch (W) {
    case 1: hipLaunchKernelGGL(k_sg_compact<1>, grid, block, 0, s, d_kmers, n, k, B, d_bits64, d_cs, d_keys, stride, d_vals, d_count); break;
    case 2: hipLaunchKernelGGL(k_sg_compact<2>, grid, block, 0, s, d_kmers, n, k, B, d_bits64, d_cs, d_keys, stride, d_vals, d_count); break;
    case 3: hipLaunchKernelGGL(k_sg_compact<3>, grid, block, 0, s, d_kmers, n, k, B, d_bits64, d_cs, d_keys, stride, d_vals, d_count); break;
    default: hipLaunchKernelGGL(k_sg_compact<4>, grid, block, 0, s, d_kmers, n, k, B, d_bits64, d_cs, d_keys, stride, d_vals, d_count); break;
    }
    HIPCK(hipGetLastError());
    return 0;
}

int bft_sg_scatter(int W, const uint64_t* d_keys, uint64_t stride, const uint32_t* d_vals, uint64_t n, const uint32_t* d_pos, uint64_t* d_tk, uint32_t* d_tcol,
                   hipStream_t s) {
    if (n == 0) return 0;
    const dim3 grid(bft_grid_for((n + SG_THREADS - 1) / SG_THREADS)), block(SG_THREADS);
    switch (W) {
    case 1: hipLaunchKernelGGL(k_sg_scatter<1>, grid, block, 0, s, d_keys, stride, d_vals, n, d_pos, d_tk, d_tcol); break;
    case 2: hipLaunchKernelGGL(k_sg_scatter<2>, grid, block, 0, s, d_keys, stride, d_vals, n, d_pos, d_tk, d_tcol); break;
    case 3: hipLaunchKernelGGL(k_sg_scatter<3>, grid, block, 0, s, d_keys, stride, d_vals, n, d_pos, d_tk, d_tcol); break;
    default: hipLaunchKernelGGL(k_sg_scatter<4>, grid, block, 0, s, d_keys, stride, d_vals, n, d_pos, d_tk, d_tcol); break;
    }
    HIPCK(hipGetLastError());
    return 0;
}

int bft_sg_mark(const uint32_t* d_tcol, uint64_t nk, uint32_t* d_used, hipStream_t s) {
    if (nk == 0) return 0;
    hipLaunchKernelGGL(k_sg_mark, dim3(bft_grid_for((nk + SG_THREADS - 1) / SG_THREADS)), dim3(SG_THREADS), 0, s, d_tcol, nk, d_used);
    HIPCK(hipGetLastError());
    return 0;
}

int bft_sg_remap(uint32_t* d_tcol, uint64_t nk, const uint32_t* d_new_id, hipStream_t s) {
    if (nk == 0) return 0;
    hipLaunchKernelGGL(k_sg_remap, dim3(bft_grid_for((nk + SG_THREADS - 1) / SG_THREADS)), dim3(SG_THREADS), 0, s, d_tcol, nk, d_new_id);
    HIPCK(hipGetLastError());
    return 0;
}

int bft_sg_dict(const uint32_t* d_used, const uint32_t* d_new_id, const uint32_t* d_id_pos, const uint32_t* d_cs_off, const void* d_cs_ids, uint32_t cs_w, uint64_t n_sets,
                uint32_t* d_new_off, uint32_t* d_new_ids, hipStream_t s) {
    const dim3 grid(bft_grid_for((n_sets + 1 + SG_THREADS / 64 - 1) / (SG_THREADS / 64))), block(SG_THREADS);
    if (cs_w == 1) hipLaunchKernelGGL(k_sg_dict<uint8_t>, grid, block, 0, s, d_used, d_new_id, d_id_pos, d_cs_off, (const uint8_t*)d_cs_ids, n_sets, d_new_off, d_new_ids);
    else if (cs_w == 2) hipLaunchKernelGGL(k_sg_dict<uint16_t>, grid, block, 0, s, d_used, d_new_id, d_id_pos, d_cs_off, (const uint16_t*)d_cs_ids, n_sets, d_new_off, d_new_ids);
    else hipLaunchKernelGGL(k_sg_dict<uint32_t>, grid, block, 0, s, d_used, d_new_id, d_id_pos, d_cs_off, (const uint32_t*)d_cs_ids, n_sets, d_new_off, d_new_ids);
    HIPCK(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------------
// the C-ABI entry points: the batch looked up in the source, the found k-mers sorted and de-duplicated, the used part of the dictionary
// renumbered (the kernels above), then the common tail of a build (bft_commit_image)
// ------------------------------------------------------------------------------------------------
struct SgEvent {
    hipEvent_t e = nullptr;
    ~SgEvent() { if (e) (void)hipEventDestroy(e); }
};
// d: a fresh handle with src's k and seeds.  The lookup runs on s (the caller's stream: d_kmers is read in its order), everything after it on
// d's stream; the new launches are timed on src ("timing"), the stages recorded on d when src records them ("build_stages").
static int subgraph_fill(bft_gpu* src, bft_gpu* d, const uint8_t* d_kmers, uint64_t n, bool colors, uint64_t* n_absent, hipStream_t s) {
    const int W = src->W;
    if (colors) {
        d->genomes = src->genomes;
        d->max_gid_seen = src->max_gid_seen;
        d->any_insert = src->any_insert;
    } else {  // (one genome, named after the source's genome 0)
        if (!src->genomes.empty()) d->genomes.push_back(src->genomes[0]);
        d->any_insert = true;
    }
    d->opt_build_stages = src->opt_build_stages;
    CK(bft_set_device(d));  // (from here on the cache hands out blocks for d's stream)
    const hipStream_t ds = d->stream;
    StageScope stage_scope(d);
    const double t0 = bft_now_ms();
    SgEvent ev;
    HIPCK(hipEventCreateWithFlags(&ev.e, hipEventDisableTiming));

    // 1. lookup: the colour-set id of every found k-mer, from the k-mer hash or -- an image without one -- the walk's tcol[row]
    DevBuf bits, cs, cnt, keys, vals;
    CK(bits.alloc(((n + 63) / 64) * 8));
    CK(cs.alloc(n * 4));
    CK(cnt.alloc_zero(8, ds));
    unsigned long long m = 0;
    if (n) {
        HIPCK(hipEventRecord(ev.e, ds));  // (the blocks above may still be in use on d's stream)
        HIPCK(hipStreamWaitEvent(s, ev.e, 0));
        src->im.emit_cs = 1;
        const int rc = bft_launch_query(src, d_kmers, n, bits.as<uint64_t>(), cs.as<uint32_t>(), s);
        src->im.emit_cs = 0;
        CK(rc);
        CK(bft_note_foreign_stream(src, s));
        HIPCK(hipEventRecord(ev.e, s));
        HIPCK(hipStreamWaitEvent(ds, ev.e, 0));
        bft_stage("sub-graph: lookup in the source", (double)n * (src->B + 4) + (double)n / 8, ds);
        // 2. the found ones as (T-form key, colour-set id) records
        CK(keys.alloc(n * W * 8));
        CK(vals.alloc(n * 4));
        CK(bft_timed_launch(src, ds, [&] {
            return bft_sg_compact(W, d_kmers, n, src->k, src->B, bits.as<uint64_t>(), cs.as<uint32_t>(), keys.as<uint64_t>(), n, vals.as<uint32_t>(),
                                  cnt.as<unsigned long long>(), ds);
        }));
        HIPCK(hipMemcpyAsync(&m, cnt.p, 8, hipMemcpyDeviceToHost, ds));
        HIPCK(hipStreamSynchronize(ds));
        bft_stage("sub-graph: found k-mers compacted", (double)n * (src->B + 4) + (double)m * (8 * W + 4), ds);
    }
    bits.release();
    cs.release();
    if (n_absent) *n_absent = n - m;

    // 3. order (the library's sort, keys only: equal keys carry equal ids) and de-duplication (first record of every run: one scan)
    BftRunOut img;  // the new handle's table, colour set per row and dictionary
    if (m) {
        DevBuf sk, sg, pos, tmp;
        CK(sk.alloc(m * W * 8));
        CK(sg.alloc(m * 4));
        CK(bft_timed_launch(src, ds, [&] { return bft_sort_pairs(d, keys.as<uint64_t>(), n, vals.as<uint32_t>(), m, sk.as<uint64_t>(), m, sg.as<uint32_t>(), true); }));
        keys.release();
        vals.release();
        CK(pos.alloc((m + 1) * 4));
        const BftSgHeads heads{sk.as<uint64_t>(), m, m, W};
        CK(bft_timed_launch(src, ds, [&] { return bft_scan::exclusive_sum<uint32_t>(heads, pos.as<uint32_t>(), m, ds, tmp, nullptr, true); }));
        uint32_t nk32 = 0;
        HIPCK(hipMemcpyAsync(&nk32, pos.as<uint32_t>() + m, 4, hipMemcpyDeviceToHost, ds));
        HIPCK(hipStreamSynchronize(ds));
        img.n = nk32;
        CK(img.tk.alloc(img.n * W * 8));
        CK(img.tcol.alloc(img.n * 4));
        CK(bft_timed_launch(src, ds, [&] { return bft_sg_scatter(W, sk.as<uint64_t>(), m, sg.as<uint32_t>(), m, pos.as<uint32_t>(), img.tk.as<uint64_t>(), img.tcol.as<uint32_t>(), ds); }));
        HIPCK(hipStreamSynchronize(ds));
    } else {
        CK(img.tcol.alloc(4));
    }
    const uint64_t nk = img.n;
    bft_stage("sub-graph: sort + dedupe", (double)m * (8 * W + 4) * 6 + (double)nk * (8 * W + 4), ds);

    // 4. the dictionary: the used sets of the source in their old order (colours), or the one set {0}
    uint64_t np = 0;
    if (nk && colors) {
        const uint64_t S = src->n_sets;
        DevBuf used, new_id, id_pos, tmp;
        CK(used.alloc_zero(S * 4, ds));
        CK(new_id.alloc((S + 1) * 4));
        CK(id_pos.alloc((S + 1) * 4));
        const uint32_t* old_off = src->d_cs_off.as<uint32_t>();
        CK(bft_timed_launch(src, ds, [&] { return bft_sg_mark(img.tcol.as<uint32_t>(), nk, used.as<uint32_t>(), ds); }));
        CK(bft_timed_launch(src, ds, [&] { return bft_scan::exclusive_sum_ptr<uint32_t>(used.as<uint32_t>(), new_id.as<uint32_t>(), S, ds, tmp, nullptr, true); }));
        const BftSgUsedLen lens{used.as<uint32_t>(), old_off, S};
        CK(bft_timed_launch(src, ds, [&] { return bft_scan::exclusive_sum<uint32_t>(lens, id_pos.as<uint32_t>(), S, ds, tmp, nullptr, true); }));
        uint32_t tot[2] = {0, 0};
        HIPCK(hipMemcpyAsync(&tot[0], new_id.as<uint32_t>() + S, 4, hipMemcpyDeviceToHost, ds));
        HIPCK(hipMemcpyAsync(&tot[1], id_pos.as<uint32_t>() + S, 4, hipMemcpyDeviceToHost, ds));
        HIPCK(hipStreamSynchronize(ds));
        img.n_sets = tot[0];
        img.n_ids = tot[1];
        CK(img.cs_off.alloc((img.n_sets + 1) * 4));
        CK(img.cs_ids.alloc(img.n_ids * 4));
        CK(bft_timed_launch(src, ds, [&] { return bft_sg_remap(img.tcol.as<uint32_t>(), nk, new_id.as<uint32_t>(), ds); }));
        CK(bft_timed_launch(src, ds, [&] {
            return bft_sg_dict(used.as<uint32_t>(), new_id.as<uint32_t>(), id_pos.as<uint32_t>(), old_off, src->d_cs_ids.p, src->cs_w, S, img.cs_off.as<uint32_t>(),
                               img.cs_ids.as<uint32_t>(), ds);
        }));
        CK(bft_count_pairs(img.tcol.as<uint32_t>(), nk, img.cs_off.as<uint32_t>(), ds, &np));
        bft_stage("sub-graph: used part of the dictionary", (double)nk * 12 + (double)S * 16 + (double)img.n_ids * (src->cs_w + 4), ds);
    } else if (nk) {
        static const uint32_t one_set[3] = {0, 1, 0};  // cs_off = {0, 1}, cs_ids = {0}
        CK(img.cs_off.alloc(8));
        CK(img.cs_ids.alloc(4));
        HIPCK(hipMemsetAsync(img.tcol.p, 0, nk * 4, ds));
        HIPCK(hipMemcpyAsync(img.cs_off.p, one_set, 8, hipMemcpyHostToDevice, ds));
        HIPCK(hipMemcpyAsync(img.cs_ids.p, one_set + 2, 4, hipMemcpyHostToDevice, ds));
        img.n_sets = 1;
        img.n_ids = 1;
        np = nk;
    } else {
        CK(img.cs_off.alloc_zero(4, ds));
        CK(img.cs_ids.alloc(4));
    }
    HIPCK(hipStreamSynchronize(ds));
    const double t1 = bft_now_ms();

    // 5-7. containers, flat forms, k-mer hash, root tables, commit: the build's own tail
    return bft_commit_image(d, img, np, t0, t1);  // (nothing deferred: no interning here)
}

static int subgraph_new(bft_gpu* src, const uint8_t* d_kmers, uint64_t n, int colors, uint64_t* n_absent, bft_gpu** out, hipStream_t s) {
    if (n >= (1ull << 31)) return bft_fail(BFT_GPU_E_LIMIT, "sub-graph batch of 2^31 k-mers or more");
    if (bft_stream_capturing(s)) return bft_fail(BFT_GPU_E_ARG, "sub-graph recorded into a graph: it allocates and synchronises");
    CK(bft_ensure_built(src, false));
    if (!(src->im.kh_lines != nullptr && !src->opt_walk_hash)) CK(bft_ensure_table(src));  // (the walk answers: launch_query would bring the table back itself)
    HIPCK(hipStreamSynchronize(src->stream));
    bft_gpu* d = nullptr;
    CK(bft_gpu_create_seeded(src->k, src->device, src->r1, src->r2, &d));
    const int rc = subgraph_fill(src, d, d_kmers, n, colors != 0, n_absent, s);
    if (rc) {
        const std::string err = bft_gpu_last_error();
        bft_gpu_free(d);
        return bft_fail(rc, err);
    }
    *out = d;
    return BFT_GPU_OK;
}

extern "C" int bft_gpu_subgraph_dev(bft_gpu* src, const void* d_kmers, uint64_t nb_kmers, int colors, uint64_t* n_absent, bft_gpu** out, void* hip_stream) {
    if (!src || !out || (!d_kmers && nb_kmers)) return bft_fail(BFT_GPU_E_ARG, "NULL argument");
    *out = nullptr;
    ENTER(src);
    return subgraph_new(src, (const uint8_t*)d_kmers, nb_kmers, colors, n_absent, out, hip_stream ? (hipStream_t)hip_stream : src->stream);
}

extern "C" int bft_gpu_subgraph(bft_gpu* src, const uint8_t* kmers, uint64_t nb_kmers, int colors, uint64_t* n_absent, bft_gpu** out) {
    if (!src || !out || (!kmers && nb_kmers)) return bft_fail(BFT_GPU_E_ARG, "NULL argument");
    *out = nullptr;
    ENTER(src);
    DevBuf dk;
    if (nb_kmers) {
        CK(dk.alloc(nb_kmers * src->B));
        HIPCK(hipMemcpy(dk.p, kmers, nb_kmers * src->B, hipMemcpyHostToDevice));
    }
    return subgraph_new(src, dk.as<uint8_t>(), nb_kmers, colors, n_absent, out, src->stream);
}
