// bft_subgraph.hip -- sub-graph builds (create_cdbg_from_bft_kmers, reference include/bft.h:179, src/bft.c:1353-1464): the kernels between the
// source's lookup and the common tail of a build (commit_image, bft_gpu.hip).
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
#include "bft_kernels_load.h"
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
