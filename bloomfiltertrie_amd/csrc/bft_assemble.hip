// bft_assemble.hip -- GPU construction of the BFT containers (bft_assemble.h).
//
// Bulk counterpart of the reference's per-k-mer insertion work (insertKmer_Node / insertKmer_Node_special
// src/insertNode.c:38-423; transform2CC / insertSP_CC / transform_Filter2n3 src/CC.c:40-1664; annotation
// updates src/retrieveAnnotation.c:232-314), level-synchronous over the sorted T-form table:
//   per depth, for all nodes of that depth at once:
//     k_prefix_flags/scatter   runs of equal 18-bit digit = the node's prefixes; runs of equal r>>4 = Bloom keys
//     k_assign_cc              one workgroup per node: CCs are opened while >= 255 k-mers are unassigned; the
//                              first <= 255 unassigned keys seed the Bloom filter (LDS bitset, atomicOr), every
//                              unassigned key the filter holds is claimed (first-BF-positive rule)
//     radix sort (bft_sort.h)  prefixes grouped by (node, CC), prefix order kept
//     k_runs / k_clusters      CC boundaries, filter2 clusters (runs of equal p_u)
//     k_entries                prefix entries {p_v | count | row-or-child-node}, filter2 bits (atomicOr), child nodes
//     k_ranks                  running rank into each filter2 word
//     k_uc_rows, k_bloom_slice node UC rows; bit-sliced Bloom block of each node
// The arrays are bit-identical to the host restatement bft_index.cpp (tests/test_gpu_build.py).
// Host side: the arrays of one depth are a Depth, a depth is the list of steps in assemble(), and every count the host needs comes through
// the counts channel (bft_counts.h) -- four waits a depth.

#include <atomic>
#include <string>
#include <vector>

#include "bft_assemble.h"
#include "bft_counts.h"
#include "bft_dev.h"
#include "bft_image.h"
#include "bft_index.h"
#include "bft_scan.h"
#include "bft_sort.h"
#include "bft_walk.h"

#define ABLK 256

namespace {

__device__ __forceinline__ uint32_t find_node(const uint32_t* __restrict__ node_off, uint32_t M, uint32_t j) {
    uint32_t lo = 0, hi = M;  // last m with node_off[m] <= j
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (node_off[mid] <= j) lo = mid;
        else hi = mid;
    }
    return lo;
}

__global__ void k_sizes(const uint32_t* lo, const uint32_t* hi, uint32_t* sz, uint32_t M) {
    for (uint32_t m = blockIdx.x * blockDim.x + threadIdx.x; m < M; m += gridDim.x * blockDim.x) sz[m] = hi[m] - lo[m];
}

// Row j of a depth's active rows starts a new prefix of its node (h) / a new Bloom key (kh): the input of ONE exclusive scan, both counts in a
// word -- h << 31 | kh, either sum below 2^31 --, computed from the table's neighbouring rows as the scan reads them (bft_scan.h takes a functor).
// Flag arrays, two scans and their four arrays of positions were 48 bytes per row; this is 8 (the T-form) in and 8 out.
constexpr uint64_t PF_KMASK = (1ull << 31) - 1ull;
template <int W>
struct PrefixFlagsIn {
    const uint64_t* tk;
    int k, d;
    const uint32_t* nd_lo;
    const uint32_t* node_off;
    uint32_t M;
    __device__ __forceinline__ uint64_t operator()(uint64_t j) const {
        const uint32_t m = M == 1 ? 0u : find_node(node_off, M, (uint32_t)j);
        const uint32_t row = nd_lo[m] + ((uint32_t)j - node_off[m]);
        const uint32_t r = bft_digit<W>(tk + (size_t)row * W, k, d);
        uint64_t h = 1, kh = 1;
        if (row != nd_lo[m]) {
            const uint32_t rp = bft_digit<W>(tk + (size_t)(row - 1) * W, k, d);
            h = r != rp;
            kh = (r >> 4) != (rp >> 4);
        }
        return (h << 31) | kh;
    }
};

// pos[j] = prefixes << 31 | keys in front of row j (pos[A] = the totals): a row whose prefix count grows is a prefix's first, likewise its key
template <int W>
__global__ void k_prefix_scatter(const uint64_t* __restrict__ tk, int k, int d, const uint32_t* __restrict__ nd_lo,
                                 const uint32_t* __restrict__ node_off, uint32_t M, uint32_t A, const uint64_t* __restrict__ pos,
                                 uint32_t* __restrict__ pref_r, uint32_t* __restrict__ pref_row, uint32_t* __restrict__ pref_node,
                                 uint32_t* __restrict__ pref_key, uint32_t* __restrict__ key_val, uint32_t* __restrict__ key_row,
                                 uint32_t* __restrict__ key_node, uint32_t* __restrict__ node_kb) {
    // (a row's own word by one coalesced load; the next row's from the neighbouring lane, by a load only in a wavefront's last lane)
    const uint32_t lane = threadIdx.x & 63u;
    for (uint32_t j0 = blockIdx.x * blockDim.x; j0 < A; j0 += gridDim.x * blockDim.x) {  // (whole wavefronts take part in the shuffles)
        const uint32_t j = j0 + threadIdx.x;
        const uint64_t p0 = j <= A ? pos[j] : 0ull;
        uint64_t p1 = ((uint64_t)(uint32_t)__shfl_down((uint32_t)(p0 >> 32), 1) << 32) | (uint32_t)__shfl_down((uint32_t)p0, 1);
        if (lane == 63u && j < A) p1 = pos[j + 1];
        if (j >= A) continue;
        const uint32_t p = (uint32_t)(p0 >> 31), kp = (uint32_t)(p0 & PF_KMASK);
        if ((uint32_t)(p1 >> 31) == p) continue;  // (not the first row of a prefix)
        const bool khd = (uint32_t)(p1 & PF_KMASK) != kp;
        const uint32_t m = M == 1 ? 0u : find_node(node_off, M, j);
        const uint32_t row = nd_lo[m] + (j - node_off[m]);
        const uint32_t r = bft_digit<W>(tk + (size_t)row * W, k, d);
        const uint32_t kk = kp + (khd ? 1u : 0u) - 1u;
        pref_r[p] = r;
        pref_row[p] = row;
        pref_node[p] = m;
        pref_key[p] = kk;
        if (khd) {
            key_val[kk] = r >> 4;
            key_row[kk] = row;
            key_node[kk] = m;
            if (row == nd_lo[m]) node_kb[m] = kk;
        }
    }
}

// count of rows under each prefix / key: next start in the same node, else the node's end
__global__ void k_counts(const uint32_t* __restrict__ start, const uint32_t* __restrict__ node, const uint32_t* __restrict__ nd_hi, uint32_t n,
                         uint32_t* __restrict__ cnt) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const uint32_t m = node[i];
        const uint32_t end = (i + 1 < n && node[i + 1] == m) ? start[i + 1] : nd_hi[m];
        cnt[i] = end - start[i];
    }
}

// format limits and counters, reduced on the device (one atomic per wavefront)
__global__ void k_ncc_limits(const uint32_t* __restrict__ node_ncc, uint32_t M, uint32_t* __restrict__ lim) {
    uint32_t mx = 0;
    for (uint32_t m = blockIdx.x * blockDim.x + threadIdx.x; m < M; m += gridDim.x * blockDim.x) mx = max(mx, node_ncc[m]);
    for (int o = 32; o > 0; o >>= 1) mx = max(mx, (uint32_t)__shfl_down(mx, o));
    if ((threadIdx.x & 63u) == 0 && mx) atomicMax(&lim[0], mx);
    if (blockIdx.x == 0 && threadIdx.x == 0) lim[1] = node_ncc[0];
}
__global__ void k_nb_limits(const uint32_t* __restrict__ cc_nb, uint32_t C, uint32_t* __restrict__ lim) {
    uint32_t mx = 0, sum = 0, big = 0;  // (the prefixes of one depth are fewer than 2^32: they index u32 arrays)
    for (uint32_t c = blockIdx.x * blockDim.x + threadIdx.x; c < C; c += gridDim.x * blockDim.x) {
        const uint32_t v = cc_nb[c];
        mx = max(mx, v);
        sum += v;
        big += v >= BFT_TRESH_SUF_PREF;
    }
    for (int o = 32; o > 0; o >>= 1) {
        mx = max(mx, (uint32_t)__shfl_down(mx, o));
        sum += __shfl_down(sum, o);
        big += __shfl_down(big, o);
    }
    if ((threadIdx.x & 63u) == 0) {
        if (mx) atomicMax(&lim[0], mx);
        if (sum) atomicAdd(&lim[1], sum);
        if (big) atomicAdd(&lim[2], big);
    }
}

__global__ void k_cc_upper(const uint32_t* __restrict__ sz, uint32_t M, uint32_t* __restrict__ ub) {
    for (uint32_t m = blockIdx.x * blockDim.x + threadIdx.x; m < M; m += gridDim.x * blockDim.x) ub[m] = sz[m] / BFT_NB_KMERS_PER_UC + 1u;
}

// One workgroup per node.  node_ccb: first Bloom-bitset slot of the node in cc_bits (an upper-bound layout, see assemble()).
__global__ __launch_bounds__(ABLK) void k_assign_cc(const uint32_t* __restrict__ key_val, const uint32_t* __restrict__ key_cnt,
                                                    const uint32_t* __restrict__ node_kb, const uint32_t* __restrict__ nd_lo,
                                                    const uint32_t* __restrict__ nd_hi, const uint32_t* __restrict__ hashmod,
                                                    int32_t* __restrict__ key_cc, uint32_t* __restrict__ node_ncc,
                                                    const uint32_t* __restrict__ node_ccb, uint32_t* __restrict__ cc_bits, uint32_t M) {
    __shared__ uint32_t bits[48];
    __shared__ uint32_t wsum[ABLK / 64];
    __shared__ uint32_t s_total;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    for (uint32_t m = blockIdx.x; m < M; m += gridDim.x) {
        const uint32_t kb = node_kb[m], ke = node_kb[m + 1];
        uint32_t U = nd_hi[m] - nd_lo[m];
        uint32_t ncc = 0;
        while (U >= BFT_NB_KMERS_PER_UC) {
            if (tid < 48) bits[tid] = 0;
            __syncthreads();
            // seeds: the first <= 255 unassigned keys, in prefix order
            uint32_t running = 0;
            for (uint32_t base = kb; base < ke && running < BFT_NB_KMERS_PER_UC; base += ABLK) {
                const uint32_t idx = base + tid;
                const bool un = idx < ke && key_cc[idx] < 0;
                const uint64_t bal = __ballot(un);
                const uint32_t inwave = (uint32_t)__builtin_popcountll(bal & ((1ull << lane) - 1ull));
                if (lane == 0) wsum[wave] = (uint32_t)__builtin_popcountll(bal);
                __syncthreads();
                uint32_t before = 0, total = 0;
                for (uint32_t w = 0; w < ABLK / 64; w++) {
                    if (w < wave) before += wsum[w];
                    total += wsum[w];
                }
                const uint32_t rank = running + before + inwave;
                if (un && rank < BFT_NB_KMERS_PER_UC) {
                    const uint32_t hm = hashmod[key_val[idx]];
                    const uint32_t h1 = hm & 0xFFFFu, h2 = hm >> 16;
                    atomicOr(&bits[h1 >> 5], 1u << (h1 & 31));
                    atomicOr(&bits[h2 >> 5], 1u << (h2 & 31));
                }
                running += total;
                __syncthreads();
            }
            __syncthreads();
            // claim every unassigned key the Bloom filter holds
            uint32_t local = 0;
            for (uint32_t idx = kb + tid; idx < ke; idx += ABLK) {
                if (key_cc[idx] >= 0) continue;
                const uint32_t hm = hashmod[key_val[idx]];
                const uint32_t h1 = hm & 0xFFFFu, h2 = hm >> 16;
                if (((bits[h1 >> 5] >> (h1 & 31)) & 1u) && ((bits[h2 >> 5] >> (h2 & 31)) & 1u)) {
                    key_cc[idx] = (int32_t)ncc;
                    local += key_cnt[idx];
                }
            }
            if (tid == 0) s_total = 0;
            __syncthreads();
            if (local) atomicAdd(&s_total, local);
            __syncthreads();
            U -= s_total;
            if (cc_bits && tid < 48) cc_bits[(size_t)(node_ccb[m] + ncc) * 48 + tid] = bits[tid];
            ncc++;
            __syncthreads();
        }
        if (tid == 0) node_ncc[m] = ncc;
        __syncthreads();
    }
}

// The same for a level that is ONE node (the root: up to 2^14 Bloom keys, two dozen CCs on a pan-genome index): one workgroup of 1024 threads
// with the node's keys in LDS -- both hash positions of a key in one word, bit 31 = assigned -- so a CC costs the workgroup LDS passes and ballots
// instead of two passes of dependent global loads (key_cc -> key_val -> hashmod) by 256 threads.  Same seeds (the first <= 255 unassigned keys
// in prefix order), same claims, same Bloom bitsets.  (A version with the keys in registers, 16 per thread, spilt 1306 VGPRs at the 128 a
// 1024-thread workgroup may use and was slower than the kernel it replaced.)
#define AONE_BLK 1024
#define AONE_MAXKEYS 16384u
__global__ __launch_bounds__(AONE_BLK) void k_assign_cc_one(const uint32_t* __restrict__ key_val, const uint32_t* __restrict__ key_cnt,
                                                            const uint32_t* __restrict__ node_kb, const uint32_t* __restrict__ nd_lo,
                                                            const uint32_t* __restrict__ nd_hi, const uint32_t* __restrict__ hashmod,
                                                            int32_t* __restrict__ key_cc, uint32_t* __restrict__ node_ncc,
                                                            const uint32_t* __restrict__ node_ccb, uint32_t* __restrict__ cc_bits) {
    extern __shared__ uint32_t hm[];  // AONE_MAXKEYS words
    __shared__ uint32_t bits[48];
    __shared__ uint32_t wsum[AONE_BLK / 64];
    __shared__ uint32_t s_total;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t kb = node_kb[0], ke = node_kb[1], nkeys = ke - kb;
    for (uint32_t i = tid; i < nkeys; i += AONE_BLK) hm[i] = hashmod[key_val[kb + i]];  // (positions below 1504: bit 31 is free)
    uint32_t U = nd_hi[0] - nd_lo[0], ncc = 0;
    __syncthreads();
    while (U >= BFT_NB_KMERS_PER_UC) {
        if (tid < 48) bits[tid] = 0;
        if (tid == 0) s_total = 0;
        __syncthreads();
        uint32_t running = 0;
        for (uint32_t base = 0; base < nkeys && running < BFT_NB_KMERS_PER_UC; base += AONE_BLK) {
            const uint32_t i = base + tid;
            const uint32_t v = i < nkeys ? hm[i] : 0x80000000u;
            const bool un = !(v >> 31);
            const uint64_t bal = __ballot(un);
            const uint32_t inwave = (uint32_t)__builtin_popcountll(bal & ((1ull << lane) - 1ull));
            if (lane == 0) wsum[wave] = (uint32_t)__builtin_popcountll(bal);
            __syncthreads();
            uint32_t before = 0, total = 0;
#pragma unroll
            for (uint32_t w = 0; w < AONE_BLK / 64; w++) {
                const uint32_t x = wsum[w];
                if (w < wave) before += x;
                total += x;
            }
            const uint32_t rank = running + before + inwave;
            if (un && rank < BFT_NB_KMERS_PER_UC) {
                const uint32_t h1 = v & 0xFFFFu, h2 = v >> 16;
                atomicOr(&bits[h1 >> 5], 1u << (h1 & 31));
                atomicOr(&bits[h2 >> 5], 1u << (h2 & 31));
            }
            running += total;
            __syncthreads();
        }
        __syncthreads();
        uint32_t local = 0;
        for (uint32_t i = tid; i < nkeys; i += AONE_BLK) {
            const uint32_t v = hm[i];
            if (v >> 31) continue;
            const uint32_t h1 = v & 0xFFFFu, h2 = v >> 16;
            if (((bits[h1 >> 5] >> (h1 & 31)) & 1u) && ((bits[h2 >> 5] >> (h2 & 31)) & 1u)) {
                key_cc[kb + i] = (int32_t)ncc;
                hm[i] = v | 0x80000000u;
                local += key_cnt[kb + i];  // (read once per key: when it is claimed)
            }
        }
        for (int o = 32; o > 0; o >>= 1) local += __shfl_down(local, o);
        if (lane == 0 && local) atomicAdd(&s_total, local);
        __syncthreads();
        U -= s_total;
        if (cc_bits && tid < 48) cc_bits[(size_t)(node_ccb[0] + ncc) * 48 + tid] = bits[tid];
        ncc++;
        __syncthreads();
    }
    if (tid == 0) node_ncc[0] = ncc;
}

__global__ void k_sort_keys(const uint32_t* __restrict__ pref_node, const uint32_t* __restrict__ pref_key, const int32_t* __restrict__ key_cc,
                            uint32_t P, uint64_t* __restrict__ skey, uint32_t* __restrict__ iota) {
    for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < P; p += gridDim.x * blockDim.x) {
        skey[p] = ((uint64_t)pref_node[p] << 17) | (uint32_t)(key_cc[pref_key[p]] + 1);
        iota[p] = p;
    }
}

// run boundaries of the sorted (node, cc+1) keys: real CCs -> cc_qb/cc_qe, UC pseudo-CC -> uc_qb/uc_qe
__global__ void k_runs(const uint64_t* __restrict__ skey, uint32_t P, const uint32_t* __restrict__ node_ccb, uint32_t* __restrict__ cc_qb,
                       uint32_t* __restrict__ cc_qe, uint32_t* __restrict__ uc_qb, uint32_t* __restrict__ uc_qe) {
    for (uint32_t q = blockIdx.x * blockDim.x + threadIdx.x; q < P; q += gridDim.x * blockDim.x) {
        const uint64_t k = skey[q];
        const uint32_t m = (uint32_t)(k >> 17), c1 = (uint32_t)(k & 0x1FFFFu);
        const bool first = q == 0 || skey[q - 1] != k, last = q + 1 == P || skey[q + 1] != k;
        if (c1 == 0) {
            if (first) uc_qb[m] = q;
            if (last) uc_qe[m] = q + 1;
        } else {
            const uint32_t ci = node_ccb[m] + c1 - 1;
            if (first) cc_qb[ci] = q;
            if (last) cc_qe[ci] = q + 1;
        }
    }
}

__global__ void k_cc_meta(const uint32_t* __restrict__ cc_qb, const uint32_t* __restrict__ cc_qe, uint32_t C, uint32_t* __restrict__ cc_nb,
                          uint32_t* __restrict__ cc_s, uint32_t* __restrict__ cc_nwords) {
    for (uint32_t c = blockIdx.x * blockDim.x + threadIdx.x; c < C; c += gridDim.x * blockDim.x) {
        const uint32_t nb = cc_qe[c] - cc_qb[c];
        const uint32_t s = nb >= BFT_TRESH_SUF_PREF ? 4u : 8u;
        cc_nb[c] = nb;
        cc_s[c] = s;
        cc_nwords[c] = ((1u << (18 - s)) + BFT_F2_BITS_PER_WORD - 1) / BFT_F2_BITS_PER_WORD;
    }
}

// per sorted prefix q: cluster-head flag, child-node flag, UC row count
__global__ void k_cluster_flags(const uint64_t* __restrict__ skey, const uint32_t* __restrict__ sp, const uint32_t* __restrict__ pref_r,
                                const uint32_t* __restrict__ pref_cnt, uint32_t P, const uint32_t* __restrict__ node_ccb,
                                const uint32_t* __restrict__ cc_qb, const uint32_t* __restrict__ cc_s, int last_level,
                                uint32_t* __restrict__ chead, uint32_t* __restrict__ pend, uint32_t* __restrict__ ucn) {
    for (uint32_t q = blockIdx.x * blockDim.x + threadIdx.x; q < P; q += gridDim.x * blockDim.x) {
        const uint64_t k = skey[q];
        const uint32_t m = (uint32_t)(k >> 17), c1 = (uint32_t)(k & 0x1FFFFu);
        const uint32_t p = sp[q];
        if (c1 == 0) {
            chead[q] = 0;
            pend[q] = 0;
            ucn[q] = pref_cnt[p];
            continue;
        }
        const uint32_t ci = node_ccb[m] + c1 - 1, s = cc_s[ci];
        uint32_t h = 1;
        if (q != cc_qb[ci]) h = (pref_r[p] >> s) != (pref_r[sp[q - 1]] >> s);
        chead[q] = h;
        pend[q] = (!last_level && pref_cnt[p] > BFT_NB_KMERS_PER_UC) ? 1u : 0u;
        ucn[q] = 0;
    }
}

__global__ void k_cluster_scatter(const uint32_t* __restrict__ chead, const uint32_t* __restrict__ cidx, uint32_t P, uint32_t* __restrict__ clus_q) {
    for (uint32_t q = blockIdx.x * blockDim.x + threadIdx.x; q < P; q += gridDim.x * blockDim.x)
        if (chead[q]) clus_q[cidx[q]] = q;
}

// cluster length and its number of entries in child[] (0 for a single-prefix cluster)
__global__ void k_cluster_len(const uint32_t* __restrict__ clus_q, uint32_t Q, const uint64_t* __restrict__ skey, const uint32_t* __restrict__ node_ccb,
                              const uint32_t* __restrict__ cc_qe, uint32_t* __restrict__ clus_len, uint32_t* __restrict__ multi) {
    for (uint32_t c = blockIdx.x * blockDim.x + threadIdx.x; c < Q; c += gridDim.x * blockDim.x) {
        const uint32_t q = clus_q[c];
        const uint64_t k = skey[q];
        const uint32_t ci = node_ccb[(uint32_t)(k >> 17)] + (uint32_t)(k & 0x1FFFFu) - 1;
        uint32_t end = cc_qe[ci];
        if (c + 1 < Q && clus_q[c + 1] < end) end = clus_q[c + 1];
        const uint32_t len = end - q;
        clus_len[c] = len;
        multi[c] = len > 1 ? len : 0;
    }
}

__global__ void k_cc_headers(const uint32_t* __restrict__ cc_qb, const uint32_t* __restrict__ cc_nb, const uint32_t* __restrict__ cc_s,
                             const uint32_t* __restrict__ cc_f2, const uint32_t* __restrict__ cidx, const uint32_t* __restrict__ cpos, uint32_t C,
                             uint32_t f2_base, uint32_t clus_base, uint32_t child_base, BftCC* __restrict__ out) {
    for (uint32_t c = blockIdx.x * blockDim.x + threadIdx.x; c < C; c += gridDim.x * blockDim.x) {
        BftCC cc;
        const uint32_t firstc = cidx[cc_qb[c]];
        cc.f2_off = f2_base + cc_f2[c];
        cc.clus_off = clus_base + firstc;
        cc.child_off = child_base + cpos[firstc];
        cc.nb_elem = (uint16_t)cc_nb[c];
        cc.s = (uint8_t)cc_s[c];
        cc.pad0 = 0;
        out[c] = cc;
    }
}

// prefix entries, filter2 bits, child nodes of the next depth
__global__ void k_entries(const uint64_t* __restrict__ skey, const uint32_t* __restrict__ sp, const uint32_t* __restrict__ pref_r,
                          const uint32_t* __restrict__ pref_row, const uint32_t* __restrict__ pref_cnt, uint32_t P,
                          const uint32_t* __restrict__ node_ccb, const uint32_t* __restrict__ cc_qb, const uint32_t* __restrict__ cc_s,
                          const uint32_t* __restrict__ cc_f2, const uint32_t* __restrict__ chead, const uint32_t* __restrict__ cidx,
                          const uint32_t* __restrict__ clus_q, const uint32_t* __restrict__ clus_len, const uint32_t* __restrict__ cpos,
                          const uint32_t* __restrict__ pend, const uint32_t* __restrict__ nrank, int last_level, int rb, uint32_t next_node_base,
                          uint64_t* __restrict__ f2w, uint64_t* __restrict__ clus, uint64_t* __restrict__ child, uint32_t* __restrict__ next_lo,
                          uint32_t* __restrict__ next_hi) {
    for (uint32_t q = blockIdx.x * blockDim.x + threadIdx.x; q < P; q += gridDim.x * blockDim.x) {
        const uint64_t k = skey[q];
        const uint32_t c1 = (uint32_t)(k & 0x1FFFFu);
        if (c1 == 0) continue;
        const uint32_t ci = node_ccb[(uint32_t)(k >> 17)] + c1 - 1, s = cc_s[ci];
        const uint32_t p = sp[q], r = pref_r[p], cnt = pref_cnt[p], row = pref_row[p];
        const uint32_t pu = r >> s, pv = r & ((1u << s) - 1u);
        uint64_t ent = (uint64_t)pv << BFT_CHILD_PV_SHIFT;
        if (last_level && rb == 0) ent |= (1ull << BFT_CHILD_CNT_SHIFT) | row;
        else if (last_level) ent = BFT_REM_ENTRY(pv, cnt, row);
        else if (!pend[q]) ent |= ((uint64_t)cnt << BFT_CHILD_CNT_SHIFT) | row;
        else {
            const uint32_t nn = nrank[q];
            ent |= (uint64_t)(next_node_base + nn);
            next_lo[nn] = row;
            next_hi[nn] = row + cnt;
        }
        const uint32_t c = cidx[q] + chead[q] - 1;  // cluster of q
        const uint32_t len = clus_len[c];
        const uint32_t firstc = cidx[cc_qb[ci]];
        if (len == 1) clus[c] = ent;
        else {
            child[cpos[c] + (q - clus_q[c])] = ent;
            if (chead[q]) clus[c] = BFT_CLUS_MULTI | ((uint64_t)len << BFT_CLUS_LEN_SHIFT) | (uint64_t)(cpos[c] - cpos[firstc]);
        }
        if (chead[q]) atomicOr((unsigned long long*)&f2w[cc_f2[ci] + pu / BFT_F2_BITS_PER_WORD], 1ull << (pu % BFT_F2_BITS_PER_WORD));
    }
}

__global__ void k_ranks(const uint32_t* __restrict__ cc_f2, const uint32_t* __restrict__ cc_nwords, uint32_t C, uint64_t* __restrict__ f2w) {
    for (uint32_t c = blockIdx.x * blockDim.x + threadIdx.x; c < C; c += gridDim.x * blockDim.x) {
        uint64_t* f2 = f2w + cc_f2[c];
        uint32_t rank = 0;
        for (uint32_t w = 0; w < cc_nwords[c]; w++) {
            const uint32_t pc = (uint32_t)__builtin_popcountll(f2[w]);
            f2[w] |= (uint64_t)rank << 48;
            rank += pc;
        }
    }
}

__global__ void k_uc_rows(const uint64_t* __restrict__ tk, int W, const uint64_t* __restrict__ skey, const uint32_t* __restrict__ sp,
                          const uint32_t* __restrict__ pref_row, const uint32_t* __restrict__ pref_cnt, const uint32_t* __restrict__ ucpos, uint32_t P,
                          uint32_t uc_base_unused, uint64_t* __restrict__ uck, uint32_t* __restrict__ ucrow) {
    for (uint32_t q = blockIdx.x * blockDim.x + threadIdx.x; q < P; q += gridDim.x * blockDim.x) {
        if ((uint32_t)(skey[q] & 0x1FFFFu) != 0) continue;
        const uint32_t p = sp[q], row0 = pref_row[p], cnt = pref_cnt[p], o = ucpos[q];
        for (uint32_t i = 0; i < cnt; i++) {
            for (int w = 0; w < W; w++) uck[(size_t)(o + i) * W + w] = tk[(size_t)(row0 + i) * W + w];
            ucrow[o + i] = row0 + i;
        }
    }
}

__global__ void k_node_meta(const uint32_t* __restrict__ node_ncc, const uint32_t* __restrict__ uc_qb, const uint32_t* __restrict__ uc_qe,
                            const uint32_t* __restrict__ ucpos, const uint32_t* __restrict__ ucn, uint32_t M, uint32_t* __restrict__ node_ucn,
                            uint32_t* __restrict__ node_bf8) {
    for (uint32_t m = blockIdx.x * blockDim.x + threadIdx.x; m < M; m += gridDim.x * blockDim.x) {
        uint32_t n = 0;
        if (uc_qe[m] > uc_qb[m]) n = ucpos[uc_qe[m] - 1] + ucn[uc_qe[m] - 1] - ucpos[uc_qb[m]];
        node_ucn[m] = n;
        const uint32_t ncc = node_ncc[m];
        const uint32_t wb = ncc == 0 ? 0 : ncc <= 8 ? 1 : ncc <= 16 ? 2 : ncc <= 32 ? 4 : 8 * ((ncc + 63) / 64);
        node_bf8[m] = (BFT_MODULO_HASH * wb) / 8;
    }
}

__global__ void k_node_records(const uint32_t* __restrict__ node_ncc, const uint32_t* __restrict__ node_ccb, const uint32_t* __restrict__ node_ucn,
                               const uint32_t* __restrict__ node_ucoff, const uint32_t* __restrict__ node_bfoff, uint32_t M, uint32_t cc_base,
                               uint32_t uc_base, uint32_t bf_base8, BftNode* __restrict__ out) {
    for (uint32_t m = blockIdx.x * blockDim.x + threadIdx.x; m < M; m += gridDim.x * blockDim.x) {
        BftNode nd;
        const uint32_t ncc = node_ncc[m];
        const uint32_t wb = ncc == 0 ? 0 : ncc <= 8 ? 1 : ncc <= 16 ? 2 : ncc <= 32 ? 4 : 8 * ((ncc + 63) / 64);
        nd.cc_first = cc_base + node_ccb[m];
        nd.bf_off = ncc ? bf_base8 + node_bfoff[m] : 0;
        nd.uc_first = uc_base + node_ucoff[m];
        nd.ncc = (uint16_t)ncc;
        nd.uc_n = (uint8_t)node_ucn[m];
        nd.bf_wb = (uint8_t)wb;
        out[m] = nd;
    }
}

// one workgroup per node: transpose the CC bitsets into the bit-sliced block
__global__ __launch_bounds__(ABLK) void k_bloom_slice(const uint32_t* __restrict__ node_ncc, const uint32_t* __restrict__ node_ccb,
                                                      const uint32_t* __restrict__ node_bfoff, const uint32_t* __restrict__ cc_bits, uint32_t M,
                                                      uint8_t* __restrict__ bfT) {
    for (uint32_t m = blockIdx.x; m < M; m += gridDim.x) {
        const uint32_t ncc = node_ncc[m];
        if (ncc == 0) continue;
        const uint32_t wb = ncc <= 8 ? 1 : ncc <= 16 ? 2 : ncc <= 32 ? 4 : 8 * ((ncc + 63) / 64);
        uint8_t* blk = bfT + (size_t)node_bfoff[m] * 8;
        const uint32_t* bits = cc_bits + (size_t)node_ccb[m] * 48;
        for (uint32_t h = threadIdx.x; h < BFT_MODULO_HASH; h += ABLK) {
            for (uint32_t b = 0; b < wb; b++) {
                uint32_t v = 0;
                for (uint32_t c = b * 8; c < ncc && c < b * 8 + 8; c++) v |= ((bits[(size_t)c * 48 + (h >> 5)] >> (h & 31)) & 1u) << (c & 7);
                blk[(size_t)h * wb + b] = (uint8_t)v;
            }
        }
    }
}

// the per-depth segments into the final arrays (every size is a multiple of 4 bytes)
struct ConcatJob { uint32_t* dst; const uint32_t* src; uint64_t words; };
struct ConcatJobs { ConcatJob j[8 * 14]; int n; };  // (k <= 126: 14 levels at most, 8 arrays each)
__global__ __launch_bounds__(ABLK) void k_concat(const ConcatJobs jobs) {
    const ConcatJob j = jobs.j[blockIdx.y];
    for (uint64_t i = blockIdx.x * (uint64_t)ABLK + threadIdx.x; i < j.words; i += (uint64_t)gridDim.x * ABLK) j.dst[i] = j.src[i];
}

// several arrays set to a value each in one launch (every size is a multiple of 4 bytes; what a depth would otherwise zero by a memset per array)
struct FillJob { uint32_t* p; uint64_t words; uint32_t val; };
struct FillJobs {
    FillJob j[8];
    int n = 0;
    void add(uint32_t* p, uint64_t words, uint32_t val) { if (words) j[n++] = FillJob{p, words, val}; }
};
__global__ __launch_bounds__(ABLK) void k_fill_many(const FillJobs jobs) {
    const FillJob j = jobs.j[blockIdx.y];
    for (uint64_t i = blockIdx.x * (uint64_t)ABLK + threadIdx.x; i < j.words; i += (uint64_t)gridDim.x * ABLK) j.p[i] = j.val;
}
int fill_many(const FillJobs& jobs, hipStream_t s) {
    if (!jobs.n) return 0;
    uint64_t mx = 1;
    for (int i = 0; i < jobs.n; i++) mx = std::max(mx, jobs.j[i].words);
    hipLaunchKernelGGL(k_fill_many, dim3(bft_grid_for((mx + ABLK - 1) / ABLK), (unsigned)jobs.n), dim3(ABLK), 0, s, jobs);
    HIPCK(hipGetLastError());
    return 0;
}

struct Seg {  // per-depth output segments, concatenated at the end
    DevArr<BftNode> nodes;
    DevArr<uint8_t> bfT;
    DevArr<BftCC> ccs;
    DevArr<uint64_t> f2w, clus, child, uck;
    DevArr<uint32_t> ucrow;
    uint64_t n_nodes = 0, n_bf8 = 0, n_ccs = 0, n_f2w = 0, n_clus = 0, n_child = 0, n_uc = 0;
};

// What the depths of one assembly share.  (The device arrays are released in the reverse of this order, as the locals they were.)
struct Assembly {
    const uint64_t* tk;
    uint64_t n;
    int k, W, L, rb;
    const uint32_t* hashmod;
    hipStream_t s;
    BftDeviceIndex& out;
    const BftAssembleHook* hook;
    BftCounts scan;
    std::vector<Seg> segs;
    DevArr<uint32_t> nd_lo, nd_hi;  // the nodes of the depth at hand: their rows [lo, hi) of the table
    uint64_t M = 1;                 // how many
    uint64_t T_nodes = 0, T_ccs = 0, T_f2w = 0, T_clus = 0, T_child = 0, T_bf8 = 0, T_uc = 0;  // totals of the depths done
    DevArr<uint32_t> nsz_c, node_off_c;  // the next depth's node sizes and their scan, prepared behind this depth's entries
    uint64_t A_c = 0;
    Assembly(const uint64_t* tk_, uint64_t n_, int k_, const uint32_t* hm, hipStream_t st, BftDeviceIndex& o, const BftAssembleHook* h)
        : tk(tk_), n(n_), k(k_), W(bft_words_for_k(k_)), L(k_ / 9), rb(2 * (k_ - 9 * (k_ / 9))), hashmod(hm), s(st), out(o), hook(h), scan(st) {}
};

// The arrays of one depth, all its nodes at once, and the counts the host has read so far.  Waits for counts per depth: prefixes + keys, CCs,
// clusters + child nodes, Bloom blocks (+ the child entries and the NEXT depth's active rows, read with that last one: their arrays are sized by
// an upper bound / prepared a depth early) -- four, where rounds 3-4 took six or seven.
struct Depth {
    int d, last_level;
    std::string lv;  // "containers depth d: "
    uint64_t M, A = 0, P = 0, K = 0, C = 0, F2 = 0, Q = 0, Mnext = 0, UCR = 0, BF8 = 0, E = 0;
    // active rows
    DevArr<uint32_t> nsz, node_off;
    // prefixes and keys
    DevArr<uint64_t> pos;  // [A + 1] prefixes << 31 | keys in front of every active row
    DevArr<uint32_t> pref_r, pref_row, pref_node, pref_key, pref_cnt, key_val, key_row, key_node, key_cnt, node_kb;
    DevArr<int32_t> key_cc;  // key -> CC (-1: unassigned)
    DevArr<uint32_t> lim;    // [0] largest number of CCs in a node, [1] that of node 0, [2] largest CC, [3] prefixes, [4] CCs with >= BFT_TRESH_SUF_PREF, [5] UC rows of node 0
    // CC assignment
    DevArr<uint32_t> node_ncc, node_ccb, cc_bits, ub, ubb;
    // prefixes in (node, CC) order
    DevArr<uint64_t> skey, skey_s;
    DevArr<uint32_t> iota, sp;
    // runs and clusters
    DevArr<uint32_t> cc_qb, cc_qe, uc_qb, uc_qe, cc_nb, cc_s, cc_nwords, cc_f2;
    DevArr<uint32_t> chead, pend, ucn, cidx, nrank, ucpos;
    DevArr<uint32_t> clus_q, clus_len, multi, cpos;
    // outputs
    Seg sg;
    DevArr<uint32_t> next_lo, next_hi;
    // node records
    DevArr<uint32_t> node_ucn, node_bf8, node_ucoff, node_bfoff;
    Depth(int d_, int L, uint64_t M_) : d(d_), last_level(d_ == L - 1), lv("containers depth " + std::to_string(d_) + ": "), M(M_) {}
    dim3 node_grid() const { return dim3((unsigned)std::min<uint64_t>(M, 65535ull * 16)); }  // a workgroup per node
};

int step_active_rows(Assembly& a, Depth& d) {
    d.A = a.n;  // (the root's rows are all of them)
    if (d.d == 0) {
        CK(d.nsz.alloc(d.M));
        CK(d.node_off.alloc(d.M + 1));
        CK(bft_launch256(k_sizes, d.M, a.s, a.nd_lo, a.nd_hi, d.nsz, (uint32_t)d.M));
        CK(a.scan.enqueue(d.nsz, d.node_off, d.M, 0, true));  // (nothing to wait for; the slot is written again only behind this scan)
    } else {
        d.nsz.swap(a.nsz_c);
        d.node_off.swap(a.node_off_c);
        d.A = a.A_c;
    }
    bft_trace_mark("  level: active rows");
    bft_stage((d.lv + "active rows").c_str(), (double)d.M * 12, a.s);
    return 0;
}

template <int W>
int step_prefix_scans(Assembly& a, Depth& d) {
    const uint64_t A = d.A;
    CK(d.pos.alloc(A + 1));
    if (A) {
        if (!a.scan.pin.p) return bft_fail(BFT_GPU_E_HIP, "hipHostMalloc (scan totals)");
        const PrefixFlagsIn<W> pf{a.tk, a.k, d.d, a.nd_lo, d.node_off, (uint32_t)d.M};
        CK((bft_scan::exclusive_sum<uint64_t>(pf, (uint64_t*)d.pos, A, a.s, a.scan.tmp, (unsigned long long*)(a.scan.pin.p + 0), true)));
        CK(a.scan.wait());
        d.P = a.scan.get(0) >> 31;
        d.K = a.scan.get(0) & PF_KMASK;
    }
    bft_trace_mark("  level: prefix flags + scans");
    bft_stage((d.lv + "prefix flags + scans").c_str(), (double)A * (8.0 * W + 8), a.s);
    return 0;
}

template <int W>
int step_scatter(Assembly& a, Depth& d) {
    const uint64_t A = d.A, P = d.P, K = d.K, M = d.M;
    hipStream_t s = a.s;
    CK(d.pref_r.alloc(P));
    CK(d.pref_row.alloc(P));
    CK(d.pref_node.alloc(P));
    CK(d.pref_key.alloc(P));
    CK(d.pref_cnt.alloc(P));
    CK(d.key_val.alloc(K));
    CK(d.key_row.alloc(K));
    CK(d.key_node.alloc(K));
    CK(d.key_cnt.alloc(K));
    CK(d.node_kb.alloc(M + 1));
    // (allocated here so that one launch presets them all) CC assignment: key -> CC; the format's limits
    CK(d.key_cc.alloc(K));
    CK(d.lim.alloc(8));
    {
        FillJobs fj;
        fj.add(d.node_kb, M, 0u);  // nodes of an empty trie (n == 0) have no keys: node_kb = 0
        fj.add(d.node_kb + M, 1, (uint32_t)K);
        if (K) fj.add((uint32_t*)d.key_cc.p, K, 0xFFFFFFFFu);
        fj.add(d.lim, 8, 0u);
        CK(fill_many(fj, s));
    }
    if (A) {
        CK(bft_launch256(k_prefix_scatter<W>, A, s, a.tk, a.k, d.d, a.nd_lo, d.node_off, (uint32_t)M, (uint32_t)A, d.pos, d.pref_r, d.pref_row, d.pref_node,
                         d.pref_key, d.key_val, d.key_row, d.key_node, d.node_kb));
        CK(bft_launch256(k_counts, P, s, d.pref_row, d.pref_node, a.nd_hi, (uint32_t)P, d.pref_cnt));
        CK(bft_launch256(k_counts, K, s, d.key_row, d.key_node, a.nd_hi, (uint32_t)K, d.key_cnt));
    }
    d.pos.release();
    return 0;
}

// hipFuncAttributeMaxDynamicSharedMemorySize of k_assign_cc_one: the attribute is per device, one bit per device it was set on
std::atomic<uint64_t> g_aone_attr_devs{0};
int aone_attr() {
    int dev = 0;
    HIPCK(hipGetDevice(&dev));
    const uint64_t dev_bit = 1ull << (dev & 63);
    if (!(g_aone_attr_devs.load(std::memory_order_acquire) & dev_bit)) {
        HIPCK(hipFuncSetAttribute((const void*)k_assign_cc_one, hipFuncAttributeMaxDynamicSharedMemorySize, AONE_MAXKEYS * 4));
        g_aone_attr_devs.fetch_or(dev_bit, std::memory_order_release);
    }
    return 0;
}

// CC assignment: one pass.  A node opens a CC only while >= 255 k-mers are unassigned and every CC but the last claims at
// least 255, so a node of U k-mers holds at most U / 255 + 1 CCs: the Bloom bitsets are written at those upper-bound slots
// (ubb) and the real CC numbering comes from a scan of the counts afterwards.  (A counting pass used to run first: the same
// kernel twice, 3.0 ms of config 3's assembly.)
int step_assign_ccs(Assembly& a, Depth& d) {
    const uint64_t A = d.A, P = d.P, K = d.K, M = d.M;
    hipStream_t s = a.s;
    BftCounts& scan = a.scan;
    CK(d.node_ncc.alloc(M));
    CK(d.node_ccb.alloc(M + 1));
    CK(d.ub.alloc(M));
    CK(d.ubb.alloc(M + 1));
    CK(bft_launch256(k_cc_upper, M, s, d.nsz, (uint32_t)M, d.ub));
    CK(scan.run(d.ub, d.ubb, M, nullptr));
    CK(d.cc_bits.alloc((A / BFT_NB_KMERS_PER_UC + M) * 48));  // (the sum of the upper bounds is at most that: no count to wait for)
    if (M == 1 && K <= AONE_MAXKEYS) {  // (one node: its keys in the LDS of one large workgroup)
        CK(aone_attr());
        hipLaunchKernelGGL(k_assign_cc_one, dim3(1), dim3(AONE_BLK), AONE_MAXKEYS * 4, s, d.key_val, d.key_cnt, d.node_kb, a.nd_lo, a.nd_hi, a.hashmod, d.key_cc,
                           d.node_ncc, d.ubb, d.cc_bits);
    } else
        hipLaunchKernelGGL(k_assign_cc, d.node_grid(), dim3(ABLK), 0, s, d.key_val, d.key_cnt, d.node_kb, a.nd_lo, a.nd_hi, a.hashmod, d.key_cc, d.node_ncc, d.ubb,
                           d.cc_bits, (uint32_t)M);
    HIPCK(hipGetLastError());
    // limits (format): CCs per node, Bloom slice width
    CK(bft_launch256(k_ncc_limits, M, s, d.node_ncc, (uint32_t)M, d.lim));
    CK(scan.enqueue(d.node_ncc, d.node_ccb, M, 0, true));
    CK(scan.publish(d.lim, 2, 1));
    CK(scan.wait());
    d.C = scan.get(0);
    if (scan.get(1) > 2040) return bft_fail(BFT_GPU_E_LIMIT, "node with too many CCs for bf_wb");
    a.out.max_ccs_per_node = std::max<uint64_t>(a.out.max_ccs_per_node, scan.get(1));
    if (d.d == 0) a.out.root_ncc = scan.get(2);
    bft_trace_mark("  level: scatter, CC assignment");
    bft_stage((d.lv + "prefix scatter, CC assignment").c_str(), (double)A * (8.0 * a.W + 16) + (double)P * 24 + (double)K * 24, s);
    // (the passes over the whole table and the root's CC assignment -- ONE workgroup claiming CC after CC, bound by latency: 0.8 ms
    // alone, 3.5 ms beside a kernel that saturates the memory system -- are done: what follows is a chain of small kernels and
    // counts read back, which leaves most of the GPU to whatever the caller starts beside it now)
    if (d.d == 0 && a.hook && a.hook->after_table_passes) a.hook->after_table_passes(a.hook->ctx, s);
    return 0;
}

// prefixes grouped by (node, cc)
int step_sort(Assembly& a, Depth& d) {
    const uint64_t P = d.P;
    CK(d.skey.alloc(P));
    CK(d.skey_s.alloc(P));
    CK(d.iota.alloc(P));
    CK(d.sp.alloc(P));
    if (P) {
        CK(bft_launch256(k_sort_keys, P, a.s, d.pref_node, d.pref_key, d.key_cc, (uint32_t)P, d.skey, d.iota));
        int mbits = 1;
        while (mbits < 32 && (d.M >> mbits)) mbits++;
        CK((bft_rs::sort_pairs<uint64_t, uint32_t, bft_rs::SHAPE_LIGHT>(d.skey, d.iota, P, d.skey_s, d.sp, 0, 17 + mbits, a.s)));
    }  // (no synchronisation: what is released here is only handed out again in the order of this stream, bft_pool_alloc)
    d.skey.release();
    d.iota.release();
    return 0;
}

// CC runs, cluster flags; the counts of the filter2 words, clusters, child nodes and UC rows
int step_runs(Assembly& a, Depth& d) {
    const uint64_t P = d.P, C = d.C, M = d.M;
    hipStream_t s = a.s;
    BftCounts& scan = a.scan;
    CK(d.cc_qb.alloc(C));
    CK(d.cc_qe.alloc(C));
    CK(d.uc_qb.alloc(M));
    CK(d.uc_qe.alloc(M));
    {
        FillJobs fj;
        fj.add(d.cc_qb, C, 0u);
        fj.add(d.cc_qe, C, 0u);
        fj.add(d.uc_qb, M, 0u);
        fj.add(d.uc_qe, M, 0u);
        CK(fill_many(fj, s));
    }
    CK(d.cc_nb.alloc(C));
    CK(d.cc_s.alloc(C));
    CK(d.cc_nwords.alloc(C));
    CK(d.cc_f2.alloc(C));
    CK(bft_launch256(k_runs, P, s, d.skey_s, (uint32_t)P, d.node_ccb, d.cc_qb, d.cc_qe, d.uc_qb, d.uc_qe));
    CK(bft_launch256(k_cc_meta, C, s, d.cc_qb, d.cc_qe, (uint32_t)C, d.cc_nb, d.cc_s, d.cc_nwords));
    CK(bft_launch256(k_nb_limits, C, s, d.cc_nb, (uint32_t)C, d.lim + 2));
    CK(scan.enqueue(d.cc_nwords, d.cc_f2, C, 0));  // (read with the cluster counts below)
    CK(d.chead.alloc(P));
    CK(d.pend.alloc(P));
    CK(d.ucn.alloc(P));
    CK(d.cidx.alloc(P));
    CK(d.nrank.alloc(P));
    CK(d.ucpos.alloc(P));
    CK(bft_launch256(k_cluster_flags, P, s, d.skey_s, d.sp, d.pref_r, d.pref_cnt, (uint32_t)P, d.node_ccb, d.cc_qb, d.cc_s, d.last_level, d.chead, d.pend, d.ucn));
    CK(scan.enqueue(d.chead, d.cidx, P, 1));
    CK(scan.enqueue(d.pend, d.nrank, P, 2));
    CK(scan.enqueue(d.ucn, d.ucpos, P, 3));
    CK(scan.publish(d.lim + 2, 3, 4));
    CK(scan.wait());
    d.F2 = scan.get(0), d.Q = scan.get(1), d.Mnext = scan.get(2), d.UCR = scan.get(3);
    if (scan.get(4) > 65535) return bft_fail(BFT_GPU_E_LIMIT, "CC with more than 65535 prefixes (nb_elem is uint16, include/CC.h:36)");
    a.out.n_prefixes += scan.get(5);
    a.out.n_ccs_s4 += scan.get(6);
    bft_trace_mark("  level: sort by (node, CC), runs, cluster flags");
    bft_stage((d.lv + "sort by (node, CC), runs, cluster flags").c_str(), (double)P * (12.0 * 2 * 4 + 60), s);
    return 0;
}

int step_clusters(Assembly& a, Depth& d) {
    const uint64_t P = d.P, Q = d.Q;
    CK(d.clus_q.alloc(Q));
    CK(d.clus_len.alloc(Q));
    CK(d.multi.alloc(Q));
    CK(d.cpos.alloc(Q));
    if (Q) {
        CK(bft_launch256(k_cluster_scatter, P, a.s, d.chead, d.cidx, (uint32_t)P, d.clus_q));
        CK(bft_launch256(k_cluster_len, Q, a.s, d.clus_q, (uint32_t)Q, d.skey_s, d.node_ccb, d.cc_qe, d.clus_len, d.multi));
    }
    // (E, the entries of the multi-prefix clusters, is read with the depth's last counts: every prefix lies in one cluster, so P bounds it)
    CK(a.scan.enqueue(d.multi, d.cpos, Q, 2));
    bft_trace_mark("  level: clusters");
    bft_stage((d.lv + "clusters").c_str(), (double)P * 8 + (double)Q * 24, a.s);
    if (a.T_f2w + d.F2 > 0xFFFFFFFFull || a.T_clus + Q > 0xFFFFFFFFull || a.T_uc + d.UCR > 0xFFFFFFFFull)
        return bft_fail(BFT_GPU_E_LIMIT, "index array offset overflow (u32)");
    return 0;
}

// the outputs of this depth: CC headers, prefix entries, filter2 ranks, UC rows; the nodes' UC and Bloom offsets; the next depth's active rows
int step_entries(Assembly& a, Depth& d) {
    const uint64_t P = d.P, C = d.C, M = d.M, Mnext = d.Mnext;
    hipStream_t s = a.s;
    BftCounts& scan = a.scan;
    Seg& sg = d.sg;
    CK(sg.ccs.alloc(C));
    CK(sg.f2w.alloc_zero(d.F2, s));
    CK(sg.clus.alloc(d.Q));
    CK(sg.child.alloc(P));  // (upper bound; E of them are used and concatenated)
    CK(sg.uck.alloc(d.UCR * a.W));
    CK(sg.ucrow.alloc(d.UCR));
    CK(sg.nodes.alloc(M));
    CK(d.next_lo.alloc(Mnext));
    CK(d.next_hi.alloc(Mnext));
    if (C) {
        // cc_f2 is relative to this depth's f2w segment while filling; headers carry global offsets
        CK(bft_launch256(k_cc_headers, C, s, d.cc_qb, d.cc_nb, d.cc_s, d.cc_f2, d.cidx, d.cpos, (uint32_t)C, (uint32_t)a.T_f2w, (uint32_t)a.T_clus, (uint32_t)a.T_child,
                         sg.ccs));
        CK(bft_launch256(k_entries, P, s, d.skey_s, d.sp, d.pref_r, d.pref_row, d.pref_cnt, (uint32_t)P, d.node_ccb, d.cc_qb, d.cc_s, d.cc_f2, d.chead, d.cidx, d.clus_q,
                         d.clus_len, d.cpos, d.pend, d.nrank, d.last_level, a.rb, (uint32_t)(a.T_nodes + M), sg.f2w, sg.clus, sg.child, d.next_lo, d.next_hi));
        CK(bft_launch256(k_ranks, C, s, d.cc_f2, d.cc_nwords, (uint32_t)C, sg.f2w));
    }
    if (d.UCR) CK(bft_launch256(k_uc_rows, P, s, a.tk, a.W, d.skey_s, d.sp, d.pref_row, d.pref_cnt, d.ucpos, (uint32_t)P, 0u, sg.uck, sg.ucrow));
    // nodes
    CK(d.node_ucn.alloc(M));
    CK(d.node_bf8.alloc(M));
    CK(d.node_ucoff.alloc(M));
    CK(d.node_bfoff.alloc(M));
    CK(bft_launch256(k_node_meta, M, s, d.node_ncc, d.uc_qb, d.uc_qe, d.ucpos, d.ucn, (uint32_t)M, d.node_ucn, d.node_bf8));
    CK(scan.run(d.node_ucn, d.node_ucoff, M, nullptr));
    CK(scan.enqueue(d.node_bf8, d.node_bfoff, M, 0));
    if (d.d == 0) CK(scan.publish(d.node_ucn, 1, 1));
    const bool deeper = Mnext && !d.last_level;
    if (deeper) {  // the next depth's node sizes and active rows, a depth early (next_lo / next_hi are k_entries' output)
        CK(a.nsz_c.alloc(Mnext));
        CK(a.node_off_c.alloc(Mnext + 1));
        CK(bft_launch256(k_sizes, Mnext, s, d.next_lo, d.next_hi, a.nsz_c, (uint32_t)Mnext));
        CK(scan.enqueue(a.nsz_c, a.node_off_c, Mnext, 3, true));
    }
    CK(scan.wait());
    d.BF8 = scan.get(0), d.E = scan.get(2);
    a.A_c = deeper ? scan.get(3) : 0;
    if (d.d == 0) a.out.root_uc = scan.get(1);
    if (d.E > P) return bft_fail(BFT_GPU_E_LIMIT, "assembly: more cluster entries than prefixes");  // (cannot happen: the bound above)
    if (a.T_child + d.E > 0xFFFFFFFFull) return bft_fail(BFT_GPU_E_LIMIT, "index array offset overflow (u32)");
    bft_trace_mark("  level: entries, node records");
    bft_stage((d.lv + "entries, ranks, UC rows, node records").c_str(),
              (double)P * 60 + (double)(d.F2 + d.Q + d.E) * 8 + (double)d.UCR * (8.0 * a.W + 4), s);
    return 0;
}

// node records, the bit-sliced Bloom blocks; the depth joins the totals and its child nodes become the nodes at hand
int step_node_records(Assembly& a, Depth& d) {
    const uint64_t M = d.M;
    if (a.T_bf8 + d.BF8 > 0xFFFFFFFFull) return bft_fail(BFT_GPU_E_LIMIT, "Bloom block offset overflow");
    Seg& sg = d.sg;
    CK(sg.bfT.alloc(d.BF8 * 8));
    CK(bft_launch256(k_node_records, M, a.s, d.node_ncc, d.node_ccb, d.node_ucn, d.node_ucoff, d.node_bfoff, (uint32_t)M, (uint32_t)a.T_ccs, (uint32_t)a.T_uc,
                     (uint32_t)a.T_bf8, sg.nodes));
    if (d.BF8) {
        hipLaunchKernelGGL(k_bloom_slice, d.node_grid(), dim3(ABLK), 0, a.s, d.node_ncc, d.ubb, d.node_bfoff, d.cc_bits, (uint32_t)M, sg.bfT);
        HIPCK(hipGetLastError());
    }
    sg.n_nodes = M; sg.n_bf8 = d.BF8; sg.n_ccs = d.C; sg.n_f2w = d.F2; sg.n_clus = d.Q; sg.n_child = d.E; sg.n_uc = d.UCR;
    a.T_nodes += M; a.T_ccs += d.C; a.T_f2w += d.F2; a.T_clus += d.Q; a.T_child += d.E; a.T_bf8 += d.BF8; a.T_uc += d.UCR;
    a.out.n_child_nodes += d.Mnext;
    a.segs.push_back(std::move(sg));
    a.nd_lo.swap(d.next_lo);
    a.nd_hi.swap(d.next_hi);
    a.M = d.Mnext;
    return 0;
}

// the per-depth segments into the final arrays: one kernel for every (depth, array) piece -- up to 8 L stream-ordered copies of a few
// microseconds each cost their launch gaps
int concatenate(Assembly& a) {
    BftDeviceIndex& out = a.out;
    const uint64_t W = a.W;
    CK(out.nodes.alloc(a.T_nodes * sizeof(BftNode)));
    CK(out.bfT.alloc(a.T_bf8 * 8));
    CK(out.ccs.alloc(a.T_ccs * sizeof(BftCC)));
    CK(out.f2w.alloc(a.T_f2w * 8));
    CK(out.clus.alloc(a.T_clus * 8));
    CK(out.child.alloc(a.T_child * 8));
    CK(out.uck.alloc(a.T_uc * W * 8));
    CK(out.ucrow.alloc(a.T_uc * 4));
    uint64_t o_n = 0, o_b = 0, o_c = 0, o_f = 0, o_q = 0, o_e = 0, o_u = 0;
    ConcatJobs jobs;
    jobs.n = 0;
    uint64_t most = 0;
    for (Seg& g : a.segs) {
#define CP(dst, src, off, nbytes) if (nbytes) { jobs.j[jobs.n++] = ConcatJob{(uint32_t*)((uint8_t*)(dst).p + (off)), (const uint32_t*)(src).p, (uint64_t)(nbytes) / 4}; most = std::max<uint64_t>(most, (uint64_t)(nbytes) / 4); }
        CP(out.nodes, g.nodes, o_n * sizeof(BftNode), g.n_nodes * sizeof(BftNode));
        CP(out.bfT, g.bfT, o_b * 8, g.n_bf8 * 8);
        CP(out.ccs, g.ccs, o_c * sizeof(BftCC), g.n_ccs * sizeof(BftCC));
        CP(out.f2w, g.f2w, o_f * 8, g.n_f2w * 8);
        CP(out.clus, g.clus, o_q * 8, g.n_clus * 8);
        CP(out.child, g.child, o_e * 8, g.n_child * 8);
        CP(out.uck, g.uck, o_u * W * 8, g.n_uc * W * 8);
        CP(out.ucrow, g.ucrow, o_u * 4, g.n_uc * 4);
#undef CP
        o_n += g.n_nodes; o_b += g.n_bf8; o_c += g.n_ccs; o_f += g.n_f2w; o_q += g.n_clus; o_e += g.n_child; o_u += g.n_uc;
    }
    if (jobs.n) {
        const unsigned gx = (unsigned)std::min<uint64_t>(1024, std::max<uint64_t>(1, (most + ABLK * 4 - 1) / (ABLK * 4)));
        hipLaunchKernelGGL(k_concat, dim3(gx, (unsigned)jobs.n), dim3(ABLK), 0, a.s, jobs);
        HIPCK(hipGetLastError());
    }
    // (no wait: the segments go back to the cache under this stream's tag, and the caller goes on in this stream)
    out.n_nodes = a.T_nodes; out.n_ccs = a.T_ccs; out.n_f2w = a.T_f2w; out.n_clus = a.T_clus; out.n_child = a.T_child; out.n_bf8 = a.T_bf8; out.n_uc = a.T_uc;
    return 0;
}

int assemble(const uint64_t* tk, uint64_t n, int k, const uint32_t* hashmod, hipStream_t s, BftDeviceIndex& out, const BftAssembleHook* hook) {
    Assembly a(tk, n, k, hashmod, s, out, hook);
    CK(a.nd_lo.alloc(1));
    CK(a.nd_hi.alloc(1));
    CK(bft_set32_async(a.nd_lo, 0u, s));  // (the root: every row)
    CK(bft_set32_async(a.nd_hi, (uint32_t)n, s));
    for (int dp = 0; dp < a.L && a.M > 0; dp++) {
        Depth d(dp, a.L, a.M);
        CK(step_active_rows(a, d));
        CK(bft_for_w(a.W, [&](auto w) { return step_prefix_scans<decltype(w)::value>(a, d); }));
        CK(bft_for_w(a.W, [&](auto w) { return step_scatter<decltype(w)::value>(a, d); }));
        CK(step_assign_ccs(a, d));
        CK(step_sort(a, d));
        CK(step_runs(a, d));
        CK(step_clusters(a, d));
        CK(step_entries(a, d));
        CK(step_node_records(a, d));
    }
    return concatenate(a);
}

}  // namespace

int bft_assemble_gpu(const uint64_t* d_tk, uint64_t n, int k, const uint32_t* d_hashmod, hipStream_t s, BftDeviceIndex& out, const BftAssembleHook* hook) {
    if (!bft_valid_k(k)) return bft_fail(BFT_GPU_E_ARG, "k must be in [9, 126]");
    if (n >= 0x7FFFFFFFull) return bft_fail(BFT_GPU_E_LIMIT, "more than 2^31-1 k-mers");
    return assemble(d_tk, n, k, d_hashmod, s, out, hook);
}
