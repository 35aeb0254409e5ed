// bft_genome_matrix.hip -- the genome-by-genome shared k-mer matrix: shared[i][j] = stored k-mers (or batch entries) whose colour set holds both genome i
// and genome j.  With B the n_sets x G 0/1 membership matrix of the dictionary cs_off / cs_ids and w the weight of every set (the rows that carry it:
// k_pg_usage of bft_pangenome.hip; or its occurrences in a caller's batch: k_gm_usage_ids), M = B^T diag(w) B: the work is proportional to the
// dictionary, not to the rows.
//   k_gm_usage_ids   usage[c] += 1 per batch entry c < n_sets (absent and out-of-range ids are skipped: nothing is written past usage[n_sets - 1])
//   k_gm_weights     a wavefront per step of 64 sets: w[c] = usage[c] where min_count <= |c| <= max_count, else 0; the five 7-bit digits of w as bytes;
//                    per step a mask of the digits that are not all zero; and the two costs of the plan: pair updates sum |c| (|c| + 1) / 2 over the
//                    sets with w != 0, digit steps = the set bits of the step masks
//   k_gm_plan        one lane: the road (forced, or the cheaper by the cost model) into plan[2].  Every kernel below reads it first and leaves when the
//                    road is the other one's: the choice costs no synchronisation
//   k_gm_sparse      the sparse road.  A wavefront takes 64 sets; a lane adds its singleton set itself, the larger sets are enumerated by the whole
//                    wavefront (row i of the set's triangle: i broadcast, j = i .. along the lanes).  Up to BFT_GM_LDS_GENOMES genomes the upper triangle
//                    is a tile of 64-bit LDS counters (ds_add_u64), flushed once per workgroup, zeros skipped; beyond, 64-bit atomics to memory
//   k_gm_clear / k_gm_bits   the dense road's operand: the transposed bit matrix, genome-major, sets along the bits (Gpad x sets_pad / 8 bytes)
//   k_gm_dense_mfma  the dense road: a workgroup owns a 16 x 16 tile pair I <= J and a split of the steps, its four wavefronts every fourth step of it.
//                    A lane's fragment of 16 consecutive sets is one 16-bit load expanded to 16 0/1 bytes; the other operand is that mask ANDed with
//                    the 16 digit bytes of those sets; one v_mfma_i32_16x16x64_i8 per non-zero digit of the step into that digit's i32 accumulators.
//                    They are added into 64-bit registers shifted by 7 d before they can overflow (every flush_sets sets: 127 * 2^24 < 2^31), and reach
//                    memory once per wavefront as 64-bit atomics, the mirror image of an off-diagonal tile with them.
// Integer arithmetic only: both roads give the same bits whatever the scheduling.  No kernel needs scratch memory.
#include <vector>

#include "bft_dev.h"
#include "bft_genome_matrix.h"
#include "bft_handle.h"
#include "bft_pangenome.h"
#include "bft_walk.h"

namespace {

constexpr int GM_THREADS = 256;
constexpr int GM_IDS_PER_LANE = 16;  // consecutive dictionary ids per lane in k_gm_bits
constexpr uint32_t GM_TRI = BFT_GM_LDS_GENOMES * (BFT_GM_LDS_GENOMES + 1u) / 2u;
constexpr int GM_SPARSE_BLOCKS = 256;  // workgroups of the LDS form: each ends with up to G (G + 1) / 2 atomic pairs

typedef int gm_i32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ unsigned long long gm_wave_sum(unsigned long long v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

__global__ __launch_bounds__(GM_THREADS) void k_gm_usage_ids(const uint32_t* __restrict__ ids, uint64_t n, uint32_t n_sets, uint32_t* __restrict__ usage) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t nthreads = (uint64_t)gridDim.x * GM_THREADS;
    // (whole wavefronts stay in the loop together: base is the wavefront's, the ballot below sees every lane)
    for (uint64_t base = blockIdx.x * (uint64_t)GM_THREADS + (threadIdx.x & ~63u); base < n; base += nthreads) {
        const uint64_t i = base + lane;
        const uint32_t c = i < n ? ids[i] : BFT_PG_NONE;
        const bool ok = c < n_sets;
        // a batch of a pan-genome is mostly one set: the lanes that hold the first valid lane's set are counted by one atomic
        const unsigned long long valid = __ballot(ok);
        if (valid == 0) continue;
        const uint32_t hot = (uint32_t)__shfl((int)c, __ffsll((long long)valid) - 1);
        const unsigned long long same = __ballot(ok && c == hot);
        if (ok && c == hot) {
            if (lane == (uint32_t)(__ffsll((long long)same) - 1)) atomicAdd(&usage[hot], (uint32_t)__popcll(same));
        } else if (ok)
            atomicAdd(&usage[c], 1u);
    }
}

__global__ __launch_bounds__(GM_THREADS) void k_gm_weights(uint32_t n_sets, uint32_t sets_pad, const uint32_t* __restrict__ cs_off, const uint32_t* __restrict__ src,
                                                           uint32_t lo, uint32_t hi, uint32_t* __restrict__ w, uint8_t* __restrict__ digit,
                                                           uint8_t* __restrict__ stepmask, unsigned long long* __restrict__ plan) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t c = blockIdx.x * (uint32_t)GM_THREADS + threadIdx.x;  // (the grid covers sets_pad exactly: a wavefront is one step)
    if (c >= sets_pad) return;
    uint32_t v = 0, sz = 0;
    if (c < n_sets) {
        sz = cs_off[c + 1] - cs_off[c];
        v = sz >= lo && sz <= hi ? src[c] : 0u;
    }
    w[c] = v;
    uint32_t mask = 0;
#pragma unroll
    for (int d = 0; d < BFT_GM_DIGITS; d++) {
        const uint32_t dg = (v >> (7 * d)) & 127u;
        digit[(size_t)d * sets_pad + c] = (uint8_t)dg;
        if (__ballot(dg != 0)) mask |= 1u << d;
    }
    const unsigned long long pairs = gm_wave_sum(v ? (unsigned long long)sz * (sz + 1ull) / 2ull : 0ull);
    if (lane == 0) {
        stepmask[c >> 6] = (uint8_t)mask;
        if (pairs) atomicAdd(&plan[0], pairs);
        if (mask) atomicAdd(&plan[1], (unsigned long long)__popc(mask));
    }
}

// dense multiply-adds = digit steps x 64 sets x Gpad^2 / 2; sparse cost = pair updates x pair_cost (BFT_GM_PAIR_COST_LDS with the LDS triangle, else
// BFT_GM_PAIR_COST)
__global__ void k_gm_plan(int forced, int dense_ok, uint32_t Gpad, unsigned long long pair_cost, unsigned long long* __restrict__ plan) {
    if (threadIdx.x || blockIdx.x) return;
    unsigned long long road = (unsigned long long)forced;
    if (forced == BFT_GM_AUTO) {
        const unsigned long long pairs = plan[0] < (1ull << 50) ? plan[0] : (1ull << 50);
        const unsigned long long per_step = 64ull * Gpad * Gpad / 2ull;  // (Gpad <= 16384: < 2^34)
        road = dense_ok && pairs * pair_cost / per_step > plan[1] ? BFT_GM_DENSE : BFT_GM_SPARSE;
    }
    plan[2] = road;
}

template <bool LDS>
__global__ __launch_bounds__(GM_THREADS) void k_gm_sparse(uint32_t n_sets, const uint32_t* __restrict__ cs_off, const void* __restrict__ cs_ids, uint32_t cs_w,
                                                          const uint32_t* __restrict__ w, uint32_t G, const unsigned long long* __restrict__ plan,
                                                          unsigned long long* __restrict__ M) {
    __shared__ unsigned long long tri[LDS ? GM_TRI : 1u];
    if (plan[2] != BFT_GM_SPARSE) return;
    // a <= b < G; the triangle's row a starts at a G - a (a - 1) / 2
    auto add = [&](uint32_t a, uint32_t b, uint32_t v) {
        if (LDS) atomicAdd(&tri[a * G - ((a * (a - 1u)) >> 1) + (b - a)], (unsigned long long)v);
        else {
            atomicAdd(&M[(size_t)a * G + b], (unsigned long long)v);
            if (a != b) atomicAdd(&M[(size_t)b * G + a], (unsigned long long)v);
        }
    };
    if (LDS) {
        for (uint32_t t = threadIdx.x; t < G * (G + 1u) / 2u; t += GM_THREADS) tri[t] = 0;
        __syncthreads();
    }
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t waves = (uint64_t)gridDim.x * (GM_THREADS / 64);
    for (uint64_t base = (blockIdx.x * (uint64_t)(GM_THREADS / 64) + (threadIdx.x >> 6)) * 64u; base < n_sets; base += waves * 64u) {
        const uint64_t c = base + lane;
        uint32_t v = 0, a = 0, e = 0;
        if (c < n_sets) {
            v = w[c];
            a = cs_off[c];
            e = cs_off[c + 1];
        }
        if (v && e - a == 1u) {
            const uint32_t g = bft_cs_id_at(cs_ids, cs_w, a);
            if (g < G) add(g, g, v);
        }
        unsigned long long todo = __ballot(v != 0 && e - a > 1u);
        while (todo) {
            const int src = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const uint32_t sa = (uint32_t)__shfl((int)a, src), se = (uint32_t)__shfl((int)e, src), sv = (uint32_t)__shfl((int)v, src);
            for (uint32_t i = sa; i < se; i++) {
                const uint32_t gi = bft_cs_id_at(cs_ids, cs_w, i);
                if (gi >= G) continue;
                for (uint32_t j = i + lane; j < se; j += 64u) {
                    const uint32_t gj = bft_cs_id_at(cs_ids, cs_w, j);
                    if (gj < G) add(gi < gj ? gi : gj, gi < gj ? gj : gi, sv);
                }
            }
        }
    }
    if (LDS) {
        __syncthreads();
        for (uint32_t i = 0, row = 0; i < G; row += G - i, i++)
            for (uint32_t j = i + threadIdx.x; j < G; j += GM_THREADS) {
                const unsigned long long t = tri[row + (j - i)];
                if (t == 0) continue;
                atomicAdd(&M[(size_t)i * G + j], t);
                if (i != j) atomicAdd(&M[(size_t)j * G + i], t);
            }
    }
}

__global__ __launch_bounds__(GM_THREADS) void k_gm_clear(uint32_t* __restrict__ p, uint64_t words, const unsigned long long* __restrict__ plan) {
    if (plan[2] != BFT_GM_DENSE) return;
    for (uint64_t i = blockIdx.x * (uint64_t)GM_THREADS + threadIdx.x; i < words; i += (uint64_t)gridDim.x * GM_THREADS) p[i] = 0;
}

// bit c of genome g's row (row_words 32-bit words; little-endian: the 16-bit word c >> 4 of the row holds the sets 16 (c >> 4) .. + 15)
__global__ __launch_bounds__(GM_THREADS) void k_gm_bits(uint32_t n_sets, uint64_t n_ids, const uint32_t* __restrict__ cs_off, const void* __restrict__ cs_ids,
                                                        uint32_t cs_w, uint32_t G, uint32_t row_words, uint32_t* __restrict__ bits,
                                                        const unsigned long long* __restrict__ plan) {
    if (plan[2] != BFT_GM_DENSE) return;
    const uint64_t tid = blockIdx.x * (uint64_t)GM_THREADS + threadIdx.x, nthreads = (uint64_t)gridDim.x * GM_THREADS;
    for (uint64_t q0 = tid * GM_IDS_PER_LANE; q0 < n_ids; q0 += nthreads * GM_IDS_PER_LANE) {
        // the set of id q0: the last c with cs_off[c] <= q0 (sets are not empty: cs_off ascends strictly), as k_pg_dict finds it
        uint32_t lo = 0, hi = n_sets;
        while (hi - lo > 1u) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (cs_off[mid] <= q0) lo = mid;
            else hi = mid;
        }
        uint32_t c = lo, e = cs_off[c + 1];
        const uint64_t q1 = q0 + GM_IDS_PER_LANE < n_ids ? q0 + GM_IDS_PER_LANE : n_ids;
        for (uint64_t q = q0; q < q1; q++) {
            while (q >= e && c + 1u < n_sets) {
                c++;
                e = cs_off[c + 1];
            }
            const uint32_t g = bft_cs_id_at(cs_ids, cs_w, q);
            if (g < G) atomicOr(&bits[(size_t)g * row_words + (c >> 5)], 1u << (c & 31u));
        }
    }
}

// the low 4 bits of x as four 0/1 bytes (bit b at byte b: x, x << 7, x << 14, x << 21 do not overlap)
__device__ __forceinline__ uint32_t gm_spread4(uint32_t x) { return ((x & 15u) * 0x00204081u) & 0x01010101u; }

// Lane l of a v_mfma_i32_16x16x64_i8 holds 16 bytes of A's row l & 15 and 16 bytes of B's column l & 15, both at the k indices of its group l >> 4
// (the SAME 16 sets in both operands here: the order of k inside the instruction cannot matter to a sum over k), and the results
// D[4 (l >> 4) + r][l & 15] in its four accumulator registers r.  A = the 0/1 bytes of the tile row I's genomes, B = digit x 0/1 of tile column J's.
__global__ __launch_bounds__(GM_THREADS) void k_gm_dense_mfma(uint32_t sets_pad, uint32_t G, uint32_t flush_steps, const uint16_t* __restrict__ bits,
                                                              const uint8_t* __restrict__ digit, const uint8_t* __restrict__ stepmask,
                                                              const unsigned long long* __restrict__ plan, unsigned long long* __restrict__ M) {
    if (plan[2] != BFT_GM_DENSE) return;
    const uint32_t J = blockIdx.x, I = blockIdx.y;
    if (I > J) return;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, grp = lane >> 4, r16 = lane & 15u;
    const uint32_t nsteps = sets_pad / BFT_GM_STEP, row16 = sets_pad / 16u;
    const uint32_t per = (nsteps + gridDim.z - 1u) / gridDim.z;
    const uint32_t s0 = blockIdx.z * per, s1 = s0 + per < nsteps ? s0 + per : nsteps;
    const uint16_t* const rowA = bits + (size_t)(I * BFT_GM_TILE + r16) * row16 + grp;
    const uint16_t* const rowB = bits + (size_t)(J * BFT_GM_TILE + r16) * row16 + grp;
    gm_i32x4 acc[BFT_GM_DIGITS];
#pragma unroll
    for (int d = 0; d < BFT_GM_DIGITS; d++) acc[d] = gm_i32x4{0, 0, 0, 0};
    unsigned long long tot[4] = {0, 0, 0, 0};
    auto flush = [&]() {
#pragma unroll
        for (int d = 0; d < BFT_GM_DIGITS; d++) {
#pragma unroll
            for (int r = 0; r < 4; r++) tot[r] += (unsigned long long)(uint32_t)acc[d][r] << (7 * d);
            acc[d] = gm_i32x4{0, 0, 0, 0};
        }
    };
    uint32_t since = 0;
    for (uint32_t st = s0 + wave; st < s1; st += GM_THREADS / 64) {
        const uint32_t m = stepmask[st];
        if (m == 0) continue;
        const uint32_t a16 = rowA[(size_t)st * 4u], b16 = rowB[(size_t)st * 4u];
        if (__ballot(a16 != 0) == 0 || __ballot(b16 != 0) == 0) continue;
        gm_i32x4 A, Bm;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            A[q] = (int)gm_spread4(a16 >> (4 * q));
            Bm[q] = (int)(gm_spread4(b16 >> (4 * q)) * 0xFFu);
        }
#pragma unroll
        for (int d = 0; d < BFT_GM_DIGITS; d++) {
            if (!((m >> d) & 1u)) continue;
            const gm_i32x4 dg = *reinterpret_cast<const gm_i32x4*>(digit + (size_t)d * sets_pad + (size_t)st * BFT_GM_STEP + grp * 16u);
            acc[d] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A, dg & Bm, acc[d], 0, 0, 0);
        }
        if (++since >= flush_steps) {
            flush();
            since = 0;
        }
    }
    flush();
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const uint32_t gi = I * BFT_GM_TILE + grp * 4u + r, gj = J * BFT_GM_TILE + r16;
        if (tot[r] == 0 || gi >= G || gj >= G) continue;
        atomicAdd(&M[(size_t)gi * G + gj], tot[r]);
        if (I != J) atomicAdd(&M[(size_t)gj * G + gi], tot[r]);
    }
}

dim3 gm_grid(uint64_t n) { return dim3(bft_grid_for((n + GM_THREADS - 1) / GM_THREADS)); }
uint64_t gm_pad(uint64_t v, uint64_t to) { return (v + to - 1) / to * to; }

}  // namespace

int bft_gm_usage_ids(const uint32_t* d_ids, uint64_t n, uint32_t n_sets, uint32_t* d_usage, hipStream_t s) {
    if (n == 0 || n_sets == 0) return 0;
    hipLaunchKernelGGL(k_gm_usage_ids, gm_grid(n), dim3(GM_THREADS), 0, s, d_ids, n, n_sets, d_usage);
    HIPCK(hipGetLastError());
    return 0;
}

int bft_gm_weights(uint32_t n_sets, const uint32_t* d_cs_off, const uint32_t* d_src, uint32_t lo, uint32_t hi, const BftGmScratch& p, hipStream_t s) {
    const uint32_t sets_pad = (uint32_t)gm_pad(n_sets, BFT_GM_STEP);
    CK(bft_zero_async(p.plan, 32, s));
    hipLaunchKernelGGL(k_gm_weights, dim3(sets_pad / GM_THREADS + (sets_pad % GM_THREADS ? 1 : 0)), dim3(GM_THREADS), 0, s, n_sets, sets_pad, d_cs_off, d_src, lo, hi,
                       p.w, p.digit, p.stepmask, p.plan);
    HIPCK(hipGetLastError());
    return 0;
}

int bft_gm_plan(int forced, bool dense_ok, uint32_t G, const BftGmScratch& p, hipStream_t s) {
    hipLaunchKernelGGL(k_gm_plan, dim3(1), dim3(64), 0, s, forced, dense_ok ? 1 : 0, (uint32_t)gm_pad(G, BFT_GM_TILE),
                       G <= BFT_GM_LDS_GENOMES ? BFT_GM_PAIR_COST_LDS : BFT_GM_PAIR_COST, p.plan);
    HIPCK(hipGetLastError());
    return 0;
}

int bft_gm_sparse(uint32_t n_sets, const uint32_t* d_cs_off, const void* d_cs_ids, uint32_t cs_w, uint32_t G, const BftGmScratch& p,
                  unsigned long long* d_shared, hipStream_t s) {
    const uint64_t blocks = ((uint64_t)n_sets + GM_THREADS - 1) / GM_THREADS;
    if (G <= BFT_GM_LDS_GENOMES)
        hipLaunchKernelGGL(k_gm_sparse<true>, dim3((unsigned)std::min<uint64_t>(GM_SPARSE_BLOCKS, blocks)), dim3(GM_THREADS), 0, s, n_sets, d_cs_off, d_cs_ids, cs_w,
                           (const uint32_t*)p.w, G, (const unsigned long long*)p.plan, d_shared);
    else
        hipLaunchKernelGGL(k_gm_sparse<false>, dim3(bft_grid_for(blocks)), dim3(GM_THREADS), 0, s, n_sets, d_cs_off, d_cs_ids, cs_w, (const uint32_t*)p.w, G,
                           (const unsigned long long*)p.plan, d_shared);
    HIPCK(hipGetLastError());
    return 0;
}

int bft_gm_bits(uint32_t n_sets, uint64_t n_ids, const uint32_t* d_cs_off, const void* d_cs_ids, uint32_t cs_w, uint32_t G, const BftGmScratch& p, hipStream_t s) {
    const uint64_t sets_pad = gm_pad(n_sets, BFT_GM_STEP), words = gm_pad(G, BFT_GM_TILE) * (sets_pad / 32);
    hipLaunchKernelGGL(k_gm_clear, gm_grid((words + 3) / 4), dim3(GM_THREADS), 0, s, (uint32_t*)p.bits, words, (const unsigned long long*)p.plan);
    hipLaunchKernelGGL(k_gm_bits, gm_grid((n_ids + GM_IDS_PER_LANE - 1) / GM_IDS_PER_LANE), dim3(GM_THREADS), 0, s, n_sets, n_ids, d_cs_off, d_cs_ids, cs_w, G,
                       (uint32_t)(sets_pad / 32), (uint32_t*)p.bits, (const unsigned long long*)p.plan);
    HIPCK(hipGetLastError());
    return 0;
}

int bft_gm_dense(uint32_t n_sets, uint32_t G, uint32_t flush_sets, const BftGmScratch& p, unsigned long long* d_shared, hipStream_t s) {
    const uint32_t sets_pad = (uint32_t)gm_pad(n_sets, BFT_GM_STEP), nsteps = sets_pad / BFT_GM_STEP, T = (uint32_t)gm_pad(G, BFT_GM_TILE) / BFT_GM_TILE;
    const uint32_t flush_steps = std::max(1u, std::min(flush_sets, (uint32_t)BFT_GM_FLUSH_SETS) / BFT_GM_STEP);
    // enough workgroups to fill the chip where the tile pairs alone do not, each with eight steps at least
    const uint64_t pairs = (uint64_t)T * (T + 1) / 2;
    const uint32_t z = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(std::max<uint64_t>(1, 4096 / pairs), (nsteps + 7) / 8));
    hipLaunchKernelGGL(k_gm_dense_mfma, dim3(T, T, z), dim3(GM_THREADS), 0, s, sets_pad, G, flush_steps, (const uint16_t*)p.bits, (const uint8_t*)p.digit,
                       (const uint8_t*)p.stepmask, (const unsigned long long*)p.plan, d_shared);
    HIPCK(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------------
// the C-ABI entry points: the handle's scratch, the chain of launches, the host-buffer forms
// ------------------------------------------------------------------------------------------------
// the arrays of a block with room for `sets` colour sets, from `base` on; returns the block's size.  (usage has one word more than it needs: the
// canary of bft_gpu_test_genome_matrix_state -- no launch writes it)
static size_t gm_carve(uint64_t sets, uint8_t* base, BftGmScratch* p) {
    const uint64_t sets_pad = gm_pad(std::max<uint64_t>(sets, 1), BFT_GM_STEP);
    Carver c{base};
    c.take(p->usage, (sets + 1) * 4);
    c.take(p->w, sets_pad * 4);
    c.take(p->digit, sets_pad * BFT_GM_DIGITS);
    c.take(p->stepmask, sets_pad / BFT_GM_STEP);
    c.take(p->plan, 32);
    return c.off;
}
static uint64_t gm_bits_bytes(uint64_t n_sets, uint32_t G) { return gm_pad(G, BFT_GM_TILE) * (gm_pad(n_sets, BFT_GM_STEP) / 8); }
// The handle's scratch (h->gm) for n_sets colour sets and G genomes on stream s.  *dense_ok: the bit matrix is there -- always when the road is
// forced to be the dense one, never when it is forced to be the sparse one, else while it stays below BFT_GM_DENSE_MAX_BYTES.
static int gm_scratch(bft_gpu* h, HandleScratch::Lease& lease, uint64_t n_sets, uint32_t G, int forced, hipStream_t s, BftGmScratch* p, bool* dense_ok) {
    CK(lease.acquire(s, false));  // (the entry points refuse a capturing stream)
    // (the carving depends on the set count: a block carved for more sets than this image has would put the arrays elsewhere, so it is carved for
    // this count and only its size is kept from shrinking)
    h->gm_sets = std::max(n_sets, h->gm_sets);
    CK(h->gm.grow(h->gm_buf, gm_carve(h->gm_sets, nullptr, p), 0));
    gm_carve(n_sets, h->gm_buf.as<uint8_t>(), p);
    const uint64_t bb = gm_bits_bytes(n_sets, G);
    *dense_ok = forced == BFT_GM_DENSE || (forced == BFT_GM_AUTO && bb <= BFT_GM_DENSE_MAX_BYTES);
    if (*dense_ok) CK(h->gm.grow(h->gm_bits, bb, 0));
    p->bits = *dense_ok ? h->gm_bits.as<uint16_t>() : nullptr;
    return 0;
}

// The roads over weights w[c] = d_src[c] where lo <= |c| <= hi (d_src: the scratch's usage, or the hook's weights), into d_shared (zeroed by the caller).
static int gm_roads(bft_gpu* h, uint32_t G, const uint32_t* d_src, uint32_t lo, uint32_t hi, int forced, bool dense_ok, uint32_t flush_sets, const BftGmScratch& p,
                    unsigned long long* d_shared, hipStream_t s) {
    const uint32_t ns = (uint32_t)h->n_sets;
    const uint32_t* const off = h->d_cs_off.as<uint32_t>();
    CK(bft_timed_launch(h, s, [&] { return bft_gm_weights(ns, off, d_src, lo, hi, p, s); }));
    CK(bft_timed_launch(h, s, [&] { return bft_gm_plan(forced, dense_ok, G, p, s); }));
    bft_stage("genome matrix: weights, digits and the road", (double)ns * (8 + 4 + 4 + BFT_GM_DIGITS), s);
    if (dense_ok) {
        CK(bft_timed_launch(h, s, [&] { return bft_gm_bits(ns, h->n_ids, off, h->d_cs_ids.p, h->cs_w, G, p, s); }));
        bft_stage("genome matrix: transposed bit matrix (dense road)", (double)gm_bits_bytes(ns, G) + (double)h->n_ids * (h->cs_w + 8) + (double)ns * 4, s);
        CK(bft_timed_launch(h, s, [&] { return bft_gm_dense(ns, G, flush_sets, p, d_shared, s); }));
        // every tile row reads its genomes' rows once per tile column at or behind it: (T + 1) / 2 times the bit matrix, the digits as often
        const double T = (double)gm_pad(G, BFT_GM_TILE) / BFT_GM_TILE;
        bft_stage("genome matrix: digit products on the matrix cores (dense road)",
                  (T + 1) * ((double)gm_bits_bytes(ns, G) + T * 0.5 * (double)gm_pad(ns, BFT_GM_STEP)) + (double)G * G * 8, s);
    }
    CK(bft_timed_launch(h, s, [&] { return bft_gm_sparse(ns, off, h->d_cs_ids.p, h->cs_w, G, p, d_shared, s); }));
    bft_stage("genome matrix: pair updates per set (sparse road)", (double)ns * 12 + (double)h->n_ids * h->cs_w + (double)G * G * 8, s);
    return 0;
}

// whole index (usage from the colour set of every row) or a batch of n colour-set ids, on stream s; d_shared holds G * G entries
static int gm_matrix(bft_gpu* h, uint32_t G, bool whole, const uint32_t* d_ids, uint64_t n, uint32_t lo, uint32_t hi, unsigned long long* d_shared, hipStream_t s) {
    if (G == 0) return 0;
    CK(bft_zero_async(d_shared, (size_t)G * G * 8, s));
    if (h->n_sets == 0 || lo > hi || (whole ? h->n_kmers == 0 : n == 0)) return 0;
    // (the scratch's use ends with this function: the callers' copies behind it read d_shared alone)
    HandleScratch::Lease lease(h->gm);
    BftGmScratch p{};
    bool dense_ok = false;
    CK(gm_scratch(h, lease, h->n_sets, G, h->opt_gm_road, s, &p, &dense_ok));
    {
        StageScope stage_scope(h, s);
        CK(bft_zero_async(p.usage, (size_t)h->n_sets * 4, s));
        if (!whole) {
            CK(bft_timed_launch(h, s, [&] { return bft_gm_usage_ids(d_ids, n, (uint32_t)h->n_sets, p.usage, s); }));
            bft_stage("genome matrix: batch entries per colour set", (double)n * 4 + (double)h->n_sets * 8, s);
        } else {
            const BftPgScratch pg{nullptr, p.usage};
            CK(bft_timed_launch(h, s, [&] { return bft_pg_usage(h->n_kmers, h->d_tcol.as<uint32_t>(), pg, s); }));
            bft_stage("genome matrix: rows per colour set", (double)h->n_kmers * 4 + (double)h->n_sets * 8, s);
        }
        CK(gm_roads(h, G, p.usage, lo, hi, h->opt_gm_road, dense_ok, BFT_GM_FLUSH_SETS, p, d_shared, s));
    }
    return 0;
}

// whole: the sorted table has to be resident ("compact_table": it comes back); the colour-set form needs the dictionary alone
static int gm_prepare(bft_gpu* h, bool whole, uint32_t* G) {
    CK(bft_ensure_built(h, whole));
    if (h->n_kmers >= (1ull << 31)) return bft_fail(BFT_GPU_E_LIMIT, "genome matrix: at most 2^31 - 1 k-mers");
    *G = bft_nb_genomes(h);
    if (*G > BFT_GM_MAX_GENOMES) return bft_fail(BFT_GPU_E_LIMIT, "genome matrix: at most 16384 genomes");
    return 0;
}

static int gm_dev(bft_gpu* h, bool whole, const void* d_colorsets, uint64_t n, uint32_t lo, uint32_t hi, void* d_shared, uint64_t cap, void* hip_stream) {
    if (!h || !d_shared || (!whole && n && !d_colorsets)) return bft_fail(BFT_GPU_E_ARG, "NULL argument");
    if (n >= (1ull << 31)) return bft_fail(BFT_GPU_E_LIMIT, "genome matrix: at most 2^31 - 1 colour-set ids");
    ENTER(h);
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : h->stream;
    if (bft_stream_capturing(s)) return bft_fail(BFT_GPU_E_ARG, "genome matrix recorded into a graph: not supported (the table may have to come back, scratch may grow)");
    uint32_t G = 0;
    CK(gm_prepare(h, whole, &G));
    if (cap < (uint64_t)G * G) return bft_fail(BFT_GPU_E_NOSPACE, "genome matrix: room for nb_genomes^2 entries is needed");
    CK(gm_matrix(h, G, whole, (const uint32_t*)d_colorsets, n, lo, hi, (unsigned long long*)d_shared, s));
    return bft_note_foreign_stream(h, s);
}

static int gm_host(bft_gpu* h, bool whole, const uint32_t* colorsets, uint64_t n, uint32_t lo, uint32_t hi, uint64_t* shared, uint64_t cap, uint32_t* nb_genomes) {
    if (!h || !nb_genomes || (!whole && n && !colorsets)) return bft_fail(BFT_GPU_E_ARG, "NULL argument");
    if (n >= (1ull << 31)) return bft_fail(BFT_GPU_E_LIMIT, "genome matrix: at most 2^31 - 1 colour-set ids");
    ENTER(h);
    uint32_t G = 0;
    CK(gm_prepare(h, whole, &G));
    *nb_genomes = G;
    if (!shared) return BFT_GPU_OK;
    if (cap < (uint64_t)G * G) return bft_fail(BFT_GPU_E_NOSPACE, "genome matrix: room for nb_genomes^2 entries is needed");
    if (G == 0) return BFT_GPU_OK;
    for (uint64_t i = 0; i < n; i++)
        if (colorsets[i] != BFT_PG_NONE && colorsets[i] >= h->n_sets) return bft_fail(BFT_GPU_E_ARG, "genome matrix: a colour-set id past the dictionary");
    const hipStream_t s = h->stream;
    DevBuf out, ids;
    CK(out.alloc((size_t)G * G * 8));
    if (!whole && n) {
        CK(ids.alloc(n * 4));
        HIPCK(hipMemcpyAsync(ids.p, colorsets, n * 4, hipMemcpyHostToDevice, s));
    }
    CK(gm_matrix(h, G, whole, ids.as<uint32_t>(), n, lo, hi, out.as<unsigned long long>(), s));
    HIPCK(hipMemcpyAsync(shared, out.p, (size_t)G * G * 8, hipMemcpyDeviceToHost, s));
    HIPCK(hipStreamSynchronize(s));
    return BFT_GPU_OK;
}

extern "C" int bft_gpu_genome_matrix(bft_gpu* h, uint32_t min_count, uint32_t max_count, uint64_t* shared, uint64_t cap, uint32_t* nb_genomes) {
    return gm_host(h, true, nullptr, 0, min_count, max_count, shared, cap, nb_genomes);
}
extern "C" int bft_gpu_genome_matrix_dev(bft_gpu* h, uint32_t min_count, uint32_t max_count, void* d_shared, uint64_t cap, void* hip_stream) {
    return gm_dev(h, true, nullptr, 0, min_count, max_count, d_shared, cap, hip_stream);
}
extern "C" int bft_gpu_genome_matrix_colorsets(bft_gpu* h, const uint32_t* colorsets, uint64_t n, uint64_t* shared, uint64_t cap, uint32_t* nb_genomes) {
    return gm_host(h, false, colorsets, n, 0, 0xFFFFFFFFu, shared, cap, nb_genomes);
}
extern "C" int bft_gpu_genome_matrix_colorsets_dev(bft_gpu* h, const void* d_colorsets, uint64_t n, void* d_shared, uint64_t cap, void* hip_stream) {
    return gm_dev(h, false, d_colorsets, n, 0, 0xFFFFFFFFu, d_shared, cap, hip_stream);
}

// Test hook (tests/test_gpu_genome_matrix.py; not in include/bft_gpu.h): one road (1 sparse, 2 dense; 0: the cost model) over the handle's dictionary
// with the caller's 32-bit weights d_weights[n_sets], the dense road's accumulators flushed every flush_sets sets (0: the library's bound).  This is
// how the digit edges and the flush are reached without an index of 2^28 rows.  Enqueues on hip_stream (NULL: the handle's), does not synchronise.
extern "C" int bft_gpu_test_genome_matrix(bft_gpu* h, const void* d_weights, int road, uint32_t flush_sets, void* d_shared, uint64_t cap, void* hip_stream) {
    if (!h || !d_weights || !d_shared) return bft_fail(BFT_GPU_E_ARG, "NULL argument");
    if (road < 0 || road > 2) return bft_fail(BFT_GPU_E_ARG, "road must be 0, 1 or 2");
    ENTER(h);
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : h->stream;
    if (bft_stream_capturing(s)) return bft_fail(BFT_GPU_E_ARG, "genome matrix recorded into a graph: not supported");
    uint32_t G = 0;
    CK(gm_prepare(h, false, &G));
    if (cap < (uint64_t)G * G) return bft_fail(BFT_GPU_E_NOSPACE, "genome matrix: room for nb_genomes^2 entries is needed");
    if (G == 0) return BFT_GPU_OK;
    CK(bft_zero_async(d_shared, (size_t)G * G * 8, s));
    if (h->n_sets == 0) return bft_note_foreign_stream(h, s);
    HandleScratch::Lease lease(h->gm);
    BftGmScratch p{};
    bool dense_ok = false;
    CK(gm_scratch(h, lease, h->n_sets, G, road, s, &p, &dense_ok));
    StageScope stage_scope(h, s);
    CK(gm_roads(h, G, (const uint32_t*)d_weights, 0, 0xFFFFFFFFu, road, dense_ok, flush_sets ? flush_sets : BFT_GM_FLUSH_SETS, p, (unsigned long long*)d_shared, s));
    return bft_note_foreign_stream(h, s);
}

// Test hook: synchronises; out[0] = the road the last call took (1 sparse, 2 dense; 0: none yet, or the call had nothing to do), out[1] = the word
// behind usage's logical end (usage[n_sets]: no launch may write it).  canary != 0: that word is set to it first (the scratch is made if need be).
extern "C" int bft_gpu_test_genome_matrix_state(bft_gpu* h, uint32_t canary, uint32_t* out) {
    if (!h || !out) return bft_fail(BFT_GPU_E_ARG, "NULL argument");
    ENTER(h);
    uint32_t G = 0;
    CK(gm_prepare(h, false, &G));
    out[0] = out[1] = 0;
    if (h->n_sets == 0) return BFT_GPU_OK;
    const hipStream_t s = h->stream;
    BftGmScratch p{};
    bool dense_ok = false;
    const bool fresh = h->gm_buf.bytes == 0;
    HandleScratch::Lease lease(h->gm);
    CK(gm_scratch(h, lease, h->n_sets, G, BFT_GM_SPARSE, s, &p, &dense_ok));
    if (fresh) HIPCK(hipMemsetAsync(p.plan, 0, 32, s));
    if (canary) HIPCK(hipMemcpyAsync(p.usage + h->n_sets, &canary, 4, hipMemcpyHostToDevice, s));
    unsigned long long plan[4] = {0, 0, 0, 0};
    HIPCK(hipMemcpyAsync(plan, p.plan, 32, hipMemcpyDeviceToHost, s));
    HIPCK(hipMemcpyAsync(&out[1], p.usage + h->n_sets, 4, hipMemcpyDeviceToHost, s));
    HIPCK(hipStreamSynchronize(s));
    out[0] = (uint32_t)plan[2];
    return BFT_GPU_OK;
}
