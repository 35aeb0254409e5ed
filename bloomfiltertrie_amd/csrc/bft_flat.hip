// bft_flat.hip -- flat form of the big CCs (bft_image.h): derived from ccs / f2w / clus / child, for the build (bft_gpu.hip) and for a handle that
// re-derives its tables (bft_derive.hip).

#include "bft_assemble.h"
#include "bft_counts.h"
#include "bft_dev.h"
#include "bft_image.h"
#include "bft_walk.h"

#define ABLK 256

namespace {

__global__ void k_flat_flags(const BftCC* __restrict__ ccs, uint32_t C, uint32_t flat_min, uint32_t* __restrict__ flag, uint32_t* __restrict__ cnt) {
    for (uint32_t c = blockIdx.x * blockDim.x + threadIdx.x; c < C; c += gridDim.x * blockDim.x) {
        const uint32_t f = ccs[c].nb_elem >= flat_min ? 1u : 0u;
        flag[c] = f;
        cnt[c] = f ? ccs[c].nb_elem : 0u;
    }
}

__global__ void k_ccx(const BftCC* __restrict__ ccs, const uint32_t* __restrict__ flag, const uint32_t* __restrict__ fidx, const uint32_t* __restrict__ foff,
                      uint32_t C, BftCCX* __restrict__ out) {
    for (uint32_t c = blockIdx.x * blockDim.x + threadIdx.x; c < C; c += gridDim.x * blockDim.x) {
        const BftCC cc = ccs[c];
        BftCCX x;
        x.f2_off = cc.f2_off; x.clus_off = cc.clus_off; x.child_off = cc.child_off; x.nb_elem = cc.nb_elem; x.s = cc.s;
        x.flat = (uint8_t)flag[c];
        x.f18_off = flag[c] ? fidx[c] * BFT_F18_WORDS : 0u;
        x.fent_off = flag[c] ? foff[c] : 0u;
        x.pad[0] = 0; x.pad[1] = 0;
        out[c] = x;
    }
}

#define FLAT_MAX_F2W 352  // filter2 words of one CC: ceil(2^14 / 48) = 342 (s = 4), 22 (s = 8)

// One workgroup per flat CC: walk the clusters in p_u order, emit every prefix entry in r order and set bit r.  A work item is a QUARTER of a
// filter2 word (12 of its 48 prefixes): 1024 threads with a dozen clusters each, where a thread per word walked up to 96 one after the other
// (0.36 ms for config 3's 21 root CCs, all of it latency).
#define FLAT_BLK 1024
#define FLAT_Q 4                                    // items per filter2 word
#define FLAT_QBITS (BFT_F2_BITS_PER_WORD / FLAT_Q)  // 12
static_assert(BFT_F2_BITS_PER_WORD % FLAT_Q == 0, "a filter2 word splits into equal parts");
__global__ __launch_bounds__(FLAT_BLK) void k_flat_fill(const BftCCX* __restrict__ ccx, uint32_t C, const uint64_t* __restrict__ f2w, const uint64_t* __restrict__ clus,
                                                        const uint64_t* __restrict__ child, uint64_t* __restrict__ f18, uint64_t* __restrict__ fent) {
    __shared__ uint32_t ipos[FLAT_MAX_F2W * FLAT_Q];
    __shared__ uint32_t wtot[FLAT_BLK / 64];
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    for (uint32_t c = blockIdx.x; c < C; c += gridDim.x) {
        const BftCCX cc = ccx[c];
        if (!cc.flat) continue;  // uniform over the workgroup
        const uint32_t nw = ((1u << (18 - cc.s)) + BFT_F2_BITS_PER_WORD - 1) / BFT_F2_BITS_PER_WORD, ni = nw * FLAT_Q;
        // entries of every item
        for (uint32_t it = threadIdx.x; it < ni; it += FLAT_BLK) {
            const uint32_t w = it / FLAT_Q, q = it % FLAT_Q;
            const uint64_t fw = f2w[cc.f2_off + w];
            const uint64_t all = fw & ((1ull << BFT_F2_BITS_PER_WORD) - 1ull);
            uint64_t bits = (all >> (q * FLAT_QBITS)) & ((1ull << FLAT_QBITS) - 1ull);
            uint32_t clu = (uint32_t)(fw >> 48) + (uint32_t)__builtin_popcountll(all & ((1ull << (q * FLAT_QBITS)) - 1ull)), n = 0;
            for (; bits; bits &= bits - 1, clu++) {
                const uint64_t e = clus[cc.clus_off + clu];
                n += (e & BFT_CLUS_MULTI) ? (uint32_t)((e >> BFT_CLUS_LEN_SHIFT) & 0xFFFFu) : 1u;
            }
            ipos[it] = n;
        }
        __syncthreads();
        // exclusive scan of ipos[0, ni): a run of `per` items per thread, wavefront scans of the runs' sums, the wavefronts' totals by the first lanes
        {
            const uint32_t per = (ni + FLAT_BLK - 1) / FLAT_BLK, i0 = threadIdx.x * per, i1 = i0 + per < ni ? i0 + per : ni;
            uint32_t sum = 0;
            for (uint32_t i = i0; i < i1; i++) sum += ipos[i];
            uint32_t inc = sum;
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t v = __shfl_up(inc, d);
                if ((int)lane >= d) inc += v;
            }
            if (lane == 63) wtot[wv] = inc;
            __syncthreads();
            uint32_t base = 0;
            for (uint32_t v = 0; v < wv; v++) base += wtot[v];
            uint32_t acc = base + inc - sum;
            for (uint32_t i = i0; i < i1; i++) { const uint32_t n = ipos[i]; ipos[i] = acc; acc += n; }
        }
        __syncthreads();
        for (uint32_t it = threadIdx.x; it < ni; it += FLAT_BLK) {
            const uint32_t w = it / FLAT_Q, q = it % FLAT_Q;
            const uint64_t fw = f2w[cc.f2_off + w];
            const uint64_t all = fw & ((1ull << BFT_F2_BITS_PER_WORD) - 1ull);
            uint64_t bits = (all >> (q * FLAT_QBITS)) & ((1ull << FLAT_QBITS) - 1ull);
            uint32_t clu = (uint32_t)(fw >> 48) + (uint32_t)__builtin_popcountll(all & ((1ull << (q * FLAT_QBITS)) - 1ull)), pos = ipos[it];
            for (; bits; bits &= bits - 1, clu++) {
                const uint32_t pu = w * BFT_F2_BITS_PER_WORD + q * FLAT_QBITS + (uint32_t)__builtin_ctzll(bits);
                const uint64_t e = clus[cc.clus_off + clu];
                const uint32_t len = (e & BFT_CLUS_MULTI) ? (uint32_t)((e >> BFT_CLUS_LEN_SHIFT) & 0xFFFFu) : 1u;
                for (uint32_t j = 0; j < len; j++) {
                    const uint64_t ent = (e & BFT_CLUS_MULTI) ? child[cc.child_off + (uint32_t)e + j] : e;
                    const uint32_t r = (pu << cc.s) | ((uint32_t)(ent >> BFT_CHILD_PV_SHIFT) & 0xFFu);
                    fent[cc.fent_off + pos++] = ent;
                    atomicOr((unsigned long long*)&f18[cc.f18_off + r / BFT_F2_BITS_PER_WORD], 1ull << (r % BFT_F2_BITS_PER_WORD));
                }
            }
        }
        __syncthreads();
    }
}

// running rank into each word of the flat bitmaps (separate launch: the bits were set with atomics)
__global__ __launch_bounds__(ABLK) void k_flat_ranks(const BftCCX* __restrict__ ccx, uint32_t C, uint64_t* __restrict__ f18) {
    __shared__ uint32_t part[ABLK];
    const uint32_t per = (BFT_F18_WORDS + ABLK - 1) / ABLK;
    for (uint32_t c = blockIdx.x; c < C; c += gridDim.x) {
        const BftCCX cc = ccx[c];
        if (!cc.flat) continue;
        uint64_t* f = f18 + cc.f18_off;
        const uint32_t w0 = threadIdx.x * per, w1 = w0 + per < BFT_F18_WORDS ? w0 + per : BFT_F18_WORDS;
        uint32_t n = 0;
        for (uint32_t w = w0; w < w1; w++) n += (uint32_t)__builtin_popcountll(f[w]);
        part[threadIdx.x] = n;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t acc = 0;
            for (uint32_t i = 0; i < ABLK; i++) { const uint32_t v = part[i]; part[i] = acc; acc += v; }
        }
        __syncthreads();
        uint32_t rank = part[threadIdx.x];
        for (uint32_t w = w0; w < w1; w++) {
            const uint64_t v = f[w];
            f[w] = v | ((uint64_t)rank << 48);
            rank += (uint32_t)__builtin_popcountll(v);
        }
        __syncthreads();
    }
}

}  // namespace

int bft_flatten_gpu(const BftCC* d_ccs, uint64_t n_ccs, const uint64_t* d_f2w, const uint64_t* d_clus, const uint64_t* d_child, uint32_t flat_min,
                    hipStream_t s, DevBuf& ccx, DevBuf& f18, DevBuf& fent, uint64_t& n_f18, uint64_t& n_fent) {
    n_f18 = 0;
    n_fent = 0;
    CK(ccx.alloc(n_ccs * sizeof(BftCCX)));
    if (n_ccs == 0) {
        CK(f18.alloc(8));
        CK(fent.alloc(8));
        return 0;
    }
    const uint32_t C = (uint32_t)n_ccs;
    BftCounts counts(s);
    DevArr<uint32_t> flag, cnt, fidx, foff;
    CK(flag.alloc(n_ccs));
    CK(cnt.alloc(n_ccs));
    CK(fidx.alloc(n_ccs));
    CK(foff.alloc(n_ccs));
    CK(bft_launch256(k_flat_flags, n_ccs, s, d_ccs, C, flat_min, flag, cnt));
    CK(counts.enqueue(flag, fidx, n_ccs, 0));
    CK(counts.enqueue(cnt, foff, n_ccs, 1));
    CK(counts.wait());  // (one wait for both counts)
    const uint64_t nflat = counts.get(0);
    n_fent = counts.get(1);
    n_f18 = nflat * BFT_F18_WORDS;
    if (n_f18 > 0xFFFFFFFFull) return bft_fail(BFT_GPU_E_LIMIT, "flat prefix bitmaps exceed 2^32 words");
    CK(f18.alloc_zero(n_f18 * 8, s));
    CK(fent.alloc(n_fent * 8));
    BftCCX* const x = ccx.as<BftCCX>();
    CK(bft_launch256(k_ccx, n_ccs, s, d_ccs, flag, fidx, foff, C, x));
    if (nflat) {  // (a workgroup per CC: grids of their own)
        const dim3 g2((unsigned)std::min<uint64_t>(n_ccs, 65535));
        hipLaunchKernelGGL(k_flat_fill, g2, dim3(FLAT_BLK), 0, s, x, C, d_f2w, d_clus, d_child, f18.as<uint64_t>(), fent.as<uint64_t>());
        HIPCK(hipGetLastError());
        hipLaunchKernelGGL(k_flat_ranks, g2, dim3(ABLK), 0, s, x, C, f18.as<uint64_t>());
        HIPCK(hipGetLastError());
    }
    return 0;  // (no wait: the caller goes on in this stream, and what is released here is handed out again in its order)
}
