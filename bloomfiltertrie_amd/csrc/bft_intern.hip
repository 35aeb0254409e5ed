// bft_intern.hip -- interning of the colour sets: the sorted genome-id list of every distinct k-mer (CSR seg_off / pg) becomes an id into a
// dictionary of the distinct lists.  Called by the build and by the commit's exact retry (bft_gpu.hip) and by the merge (bft_merge.hip).
//   step 1  k_cs_sig, k_cs_hash_*      a 64-bit signature per list (bft_cs_sig.h); equal signatures found through a hash table, the sets numbered
//                                      in the order of their signatures
//   step 2  k_cs_hash_copy, k_cs_verify the dictionary entries copied out of their representatives' lists, then EVERY k-mer's list compared with the
//                                      entry it was given -- on the caller's stream or, deferred, on a side stream (BftInternTail, bft_intern.h)
//   step 3  k_cs_key2 .. k_cs_assign   the exact pass, when two different lists shared a signature or the caller asks: lists compared, never keys

#include "bft_counts.h"
#include "bft_cs_sig.h"
#include "bft_dev.h"
#include "bft_intern.h"
#include "bft_sort.h"

#define ABLK 256

namespace {

// ---------------------------------------------------------------------------------------------
// colour sets
// ---------------------------------------------------------------------------------------------
// (the signature function itself: bft_cs_sig.h)

// The genome-id lists of the index are bimodal (a k-mer of the shared ancestor sits in most genomes, a k-mer around a SNP in
// one), so one-thread-per-list loops leave most lanes idle for the length of the longest list of the wavefront.  The lists
// of 64 consecutive k-mers are ONE contiguous range of pg: the kernels below let the wavefront stream that range coalesced,
// each element finding its list by a binary search over the lanes' start offsets (6 shuffles).
// lane s owns the list pg[a_s, ...): the largest lane whose start is <= e (starts are non-decreasing over the lanes)
__device__ __forceinline__ uint32_t wave_list_of(uint32_t e, uint32_t a) {
    uint32_t lo = 0, hi = 63;
#pragma unroll
    for (int it = 0; it < 6; it++) {  // every lane takes part in every shuffle
        const uint32_t mid = (lo + hi + 1) >> 1;
        const uint32_t am = __shfl(a, mid);
        if (am <= e) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// signature of the sorted genome-id list of each k-mer: a sum of mixed ids (order-free, so that the elements can be added
// in any order by any lane) mixed with the length
__global__ __launch_bounds__(ABLK) void k_cs_sig(const uint32_t* __restrict__ seg_off, const uint32_t* __restrict__ pg, uint32_t nk, int weak, uint64_t* __restrict__ sig,
                                                 uint32_t* __restrict__ iota) {
    __shared__ unsigned long long acc[ABLK];
    const uint32_t lane = threadIdx.x & 63u, w0 = threadIdx.x & ~63u;
    const uint32_t nblk = (nk + ABLK - 1) / ABLK;
    for (uint32_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {  // whole wavefronts stay in the loop together
        const uint32_t i = blk * ABLK + threadIdx.x;
        const bool valid = i < nk;
        const uint32_t a = seg_off[valid ? i : nk], b = seg_off[valid ? i + 1 : nk];
        const uint32_t base = __shfl(a, 0), end = __shfl(b, 63);
        acc[threadIdx.x] = 0ull;
        for (uint32_t e0 = base; e0 < end; e0 += 64) {
            const uint32_t e = e0 + lane;
            const bool in = e < end;
            const uint32_t s = wave_list_of(in ? e : end - 1, a);
            if (in) atomicAdd(&acc[w0 + s], (unsigned long long)bft_cs_term(pg[e]));
        }
        if (valid) {
            // (weak: a test hook -- the signature of a list is its length, so that different lists collide and the exact pass must run)
            sig[i] = bft_cs_finish((uint64_t)acc[threadIdx.x], b - a, weak);
            iota[i] = i;
        }
    }
}

__device__ __forceinline__ bool same_list(const uint32_t* __restrict__ seg_off, const uint32_t* __restrict__ pg, uint32_t a, uint32_t b) {
    const uint32_t la = seg_off[a + 1] - seg_off[a], lb = seg_off[b + 1] - seg_off[b];
    if (la != lb) return false;
    for (uint32_t i = 0; i < la; i++)
        if (pg[seg_off[a] + i] != pg[seg_off[b] + i]) return false;
    return true;
}

// ---- the exact pass (k_cs_key2 .. k_cs_assign): only when k_cs_verify found two different lists with one signature, or a caller asks ----
// The lists are sorted on (signature, second key, k-mer number) and equal lists found by comparing the lists themselves: never by a key.

// second key of a list (one thread per list: this pass is no hot path).  how 0: a sum of terms mixed independently of bft_cs_sig.h's, so that
// the lists of one signature fall apart by it; 1: bft_cs_sig.h's signature itself (the signatures are the weak hook's lengths); 2: the length
// (weak hook 2: neither key tells lists apart, and k_cs_canon has to)
__global__ void k_cs_key2(const uint32_t* __restrict__ seg_off, const uint32_t* __restrict__ pg, uint32_t nk, int how, uint64_t* __restrict__ key2) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nk; i += gridDim.x * blockDim.x) {
        const uint32_t a = seg_off[i], b = seg_off[i + 1];
        uint64_t sum = 0;
        if (how == 0) for (uint32_t e = a; e < b; e++) sum += bft_mix64(((uint64_t)pg[e] + 1) * 0xD6E8FEB86659FD93ULL);
        if (how == 1) for (uint32_t e = a; e < b; e++) sum += bft_cs_term(pg[e]);
        key2[i] = how == 2 ? (uint64_t)(b - a) : how == 1 ? bft_cs_finish(sum, b - a, 0) : bft_mix64(sum + (uint64_t)(b - a) * 0xA24BAED4963EE407ULL);
    }
}

__global__ void k_cs_gather64(const uint64_t* __restrict__ src, const uint32_t* __restrict__ idx, uint32_t n, uint64_t* __restrict__ out) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) out[i] = src[idx[i]];
}

// a stretch of equal lists starts where the list differs from its predecessor in the sorted order: by either key or, the keys equal, by the
// lists themselves
__global__ void k_cs_heads(const uint64_t* __restrict__ sig_s, const uint64_t* __restrict__ key2_s, const uint32_t* __restrict__ order,
                           const uint32_t* __restrict__ seg_off, const uint32_t* __restrict__ pg, uint32_t nk, uint32_t* __restrict__ head0) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nk; i += gridDim.x * blockDim.x)
        head0[i] = (i > 0 && sig_s[i] == sig_s[i - 1] && key2_s[i] == key2_s[i - 1] && same_list(seg_off, pg, order[i], order[i - 1])) ? 0u : 1u;
}

// position of the r-th stretch's first list (r0_ex: exclusive sum of head0)
__global__ void k_cs_headpos(const uint32_t* __restrict__ head0, const uint32_t* __restrict__ r0_ex, uint32_t nk, uint32_t* __restrict__ headpos) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nk; i += gridDim.x * blockDim.x)
        if (head0[i]) headpos[r0_ex[i]] = i;
}

// Two different lists with BOTH keys equal may alternate -- A B A B is four stretches of two sets --: the first list of every stretch looks for
// its list among the earlier stretches of the same two keys and takes the earliest one's place (canon: position of the list that stands for
// the set; head: this list does).  With the second key independent of the first such a run has one stretch; under weak hook 2 it has many,
// and the test cases are sized for that.
__global__ void k_cs_canon(const uint64_t* __restrict__ sig_s, const uint64_t* __restrict__ key2_s, const uint32_t* __restrict__ order,
                           const uint32_t* __restrict__ head0, const uint32_t* __restrict__ r0_ex, const uint32_t* __restrict__ headpos,
                           const uint32_t* __restrict__ seg_off, const uint32_t* __restrict__ pg, uint32_t nk, uint32_t* __restrict__ canon,
                           uint32_t* __restrict__ head, uint32_t* __restrict__ len) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nk; i += gridDim.x * blockDim.x) {
        uint32_t h = 0, l = 0;
        if (head0[i]) {
            const uint32_t a = order[i];
            const uint64_t s1 = sig_s[i], s2 = key2_s[i];
            uint32_t m = i;
            for (uint32_t r = r0_ex[i]; r-- > 0;) {
                const uint32_t j = headpos[r];
                if (sig_s[j] != s1 || key2_s[j] != s2) break;
                if (same_list(seg_off, pg, a, order[j])) m = j;
            }
            canon[i] = m;
            h = m == i;
            l = h ? seg_off[a + 1] - seg_off[a] : 0;
        }
        head[i] = h;
        len[i] = l;
    }
}

// the other lists of a stretch: what its first list found
__global__ void k_cs_spread(const uint32_t* __restrict__ head0, const uint32_t* __restrict__ r0_ex, const uint32_t* __restrict__ headpos, uint32_t nk,
                            uint32_t* __restrict__ canon) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nk; i += gridDim.x * blockDim.x)
        if (!head0[i]) canon[i] = canon[headpos[r0_ex[i] - 1]];  // (position 0 is always a first list: r0_ex[i] >= 1 here)
}

// tcol of every k-mer (position i of the sorted order; csid_ex: exclusive sum of head) and, for the list that stands for a set, the
// dictionary entry: the lanes of a wavefront copy that list together, 64 ids at a time
__global__ __launch_bounds__(ABLK) void k_cs_assign(const uint32_t* __restrict__ order, const uint32_t* __restrict__ head, const uint32_t* __restrict__ canon,
                                                    const uint32_t* __restrict__ csid_ex, const uint32_t* __restrict__ off_ex, const uint32_t* __restrict__ seg_off,
                                                    const uint32_t* __restrict__ pg, uint32_t nk, uint32_t* __restrict__ tcol, uint32_t* __restrict__ cs_off,
                                                    uint32_t* __restrict__ cs_ids) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t nblk = (nk + ABLK - 1) / ABLK;
    for (uint32_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
        const uint32_t i = blk * ABLK + threadIdx.x;
        uint32_t hd = 0, src = 0, len = 0, dst = 0;
        if (i < nk) {
            const uint32_t a = order[i];
            hd = head[i];
            const uint32_t cs = csid_ex[canon[i]];  // (canon[i] is a position whose head is 1: the sets in front of it number it)
            tcol[a] = cs;
            if (hd) {
                src = seg_off[a];
                len = seg_off[a + 1] - src;
                dst = off_ex[i];
                cs_off[cs] = dst;
            }
        }
        uint64_t heads = __ballot(hd != 0);
        while (heads) {
            const int t = __builtin_ctzll(heads);
            heads &= heads - 1;
            const uint32_t s0 = __shfl(src, t), l0 = __shfl(len, t), d0 = __shfl(dst, t);
            for (uint32_t j = lane; j < l0; j += 64) cs_ids[d0 + j] = pg[s0 + j];
        }
    }
}

// exactness check: every k-mer's list equals the dictionary entry it was assigned (streamed like k_cs_sig)
__global__ __launch_bounds__(ABLK) void k_cs_verify(const uint32_t* __restrict__ tcol, const uint32_t* __restrict__ cs_off, const uint32_t* __restrict__ cs_ids,
                                                    const uint32_t* __restrict__ seg_off, const uint32_t* __restrict__ pg, uint32_t nk, uint32_t* __restrict__ bad) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t nblk = (nk + ABLK - 1) / ABLK;
    for (uint32_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
        const uint32_t i = blk * ABLK + threadIdx.x;
        const bool valid = i < nk;
        const uint32_t a = seg_off[valid ? i : nk], b = seg_off[valid ? i + 1 : nk];
        uint32_t co = 0;
        bool wrong = false;
        if (valid) {
            const uint32_t cs = tcol[i];
            co = cs_off[cs];
            wrong = (cs_off[cs + 1] - co) != (b - a);
        }
        const uint32_t base = __shfl(a, 0), end = __shfl(b, 63);
        for (uint32_t e0 = base; e0 < end; e0 += 64) {
            const uint32_t e = e0 + lane;
            const bool in = e < end;
            const uint32_t s = wave_list_of(in ? e : end - 1, a);
            const uint32_t as = __shfl(a, s), cos = __shfl(co, s);
            if (in && cs_ids[cos + (e - as)] != pg[e]) wrong = true;  // a list of the wrong length is already flagged by its own lane
        }
        if (wrong) atomicAdd(bad, 1u);
    }
}

// ---- interning by a hash of the signatures ----
// The lists of a pan-genome repeat massively (config 3: 4.5 x 10^7 k-mers, 1.6 x 10^6 distinct lists, and nine k-mers in ten carry one
// of the 100 one-genome lists): every k-mer looks its signature up in an open-addressed table -- the popular lists are L2 hits --,
// the few distinct signatures are sorted (that order numbers the sets, whichever thread inserted first), and the first k-mer to claim
// a slot lends the dictionary its list.  Sorting every k-mer's signature instead (6 radix passes over 4.5 x 10^7 pairs, then gathers
// in that order) was 3.5 ms of config 3's 6.5.
struct CsSlot {
    unsigned long long sig;  // 0: free
    uint32_t rep;            // a k-mer with this signature
    uint32_t id;             // number of the set
};
__device__ __forceinline__ unsigned long long cs_key(uint64_t sig) { return sig ? sig : 0x9E3779B97F4A7C15ULL; }

// (Nine lookups in ten ask for one of a hundred slots: as device-scope atomics those queue up at the few memory channels that own
// them -- 13 ms; a run of ONE genome asks 2 x 10^6 times for one slot.  Each workgroup therefore remembers, in LDS, the slot where a
// signature was last found; a remembered slot is confirmed by an ordinary cached load of its signature, which is immutable once
// claimed -- a stale view can only show the slot free and sends the lookup down the atomic path.  And only ONE thread of the workgroup
// at a time takes the atomic path for an entry of that memory (an LDS lock per entry): the others with the same signature find the
// slot remembered when they look again.)
#define CS_CACHE 2048u
__global__ __launch_bounds__(ABLK) void k_cs_hash_insert(const uint64_t* __restrict__ sig, uint32_t nk, CsSlot* __restrict__ tab, uint32_t mask,
                                                         uint32_t* __restrict__ slot_of,
                                                         uint32_t* __restrict__ counters) {  // [0] slots claimed, [1] lookups that gave up (table too full)
    __shared__ uint32_t cache[CS_CACHE];
    __shared__ uint32_t lock[CS_CACHE];
    __shared__ uint32_t s_new, s_fail;  // (one global atomic per workgroup at the end: 10^6 atomics on ONE address take 10 ns each)
    for (uint32_t j = threadIdx.x; j < CS_CACHE; j += blockDim.x) { cache[j] = 0xFFFFFFFFu; lock[j] = 0; }
    if (threadIdx.x == 0) { s_new = 0; s_fail = 0; }
    __syncthreads();
    const uint32_t nblk = (nk + ABLK - 1) / ABLK;
    for (uint32_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
        const uint32_t i = blk * ABLK + threadIdx.x;
        bool done = i >= nk;
        const unsigned long long key = done ? 0ull : cs_key(sig[i]);
        const uint32_t ch = (uint32_t)(key >> 40) & (CS_CACHE - 1u);
        uint32_t found = 0xFFFFFFFFu;
        // (every lane of the wavefront stays in the loop until all are done: a lane that holds a lock finishes its lookup inside the
        // iteration, so the lanes waiting for it -- of this wavefront or another -- see the slot the next time round)
        for (int round = 0; round < 4096 && __any(!done); round++) {
            if (!done) {
                const uint32_t cand = cache[ch];
                if (cand != 0xFFFFFFFFu && tab[cand].sig == key) {
                    found = cand;
                    done = true;
                } else if (atomicCAS(&lock[ch], 0u, 1u) == 0u) {
                    uint32_t pos = (uint32_t)key & mask;
                    for (int probe = 0; probe < 64; probe++) {  // (beyond that the table is too full: the caller retries with a larger one)
                        unsigned long long cur = __hip_atomic_load(&tab[pos].sig, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        if (cur == 0ull) {
                            cur = atomicCAS(&tab[pos].sig, 0ull, key);
                            if (cur == 0ull) {
                                tab[pos].rep = i;
                                atomicAdd(&s_new, 1u);
                                cur = key;
                            }
                        }
                        if (cur == key) { found = pos; break; }
                        pos = (pos + 1u) & mask;
                    }
                    if (found != 0xFFFFFFFFu) cache[ch] = found;
                    __threadfence_block();
                    atomicExch(&lock[ch], 0u);
                    done = true;
                }
            }
        }
        if (i < nk) {
            if (found == 0xFFFFFFFFu) atomicAdd(&s_fail, 1u);
            slot_of[i] = found;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_new) atomicAdd(&counters[0], s_new);
        if (s_fail) atomicAdd(&counters[1], s_fail);
    }
}

// the claimed slots, in any order: every workgroup counts its share of the table, reserves that many places with one atomic, writes
__global__ __launch_bounds__(ABLK) void k_cs_hash_compact(const CsSlot* __restrict__ tab, uint32_t n_slots, uint64_t* __restrict__ keys, uint32_t* __restrict__ slots,
                                                          uint32_t* __restrict__ cnt) {
    __shared__ uint32_t s_cnt, s_base;
    const uint32_t per = (n_slots + gridDim.x - 1) / gridDim.x, p0 = blockIdx.x * per, p1 = min(n_slots, p0 + per);
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    uint32_t mine = 0;
    for (uint32_t p = p0 + threadIdx.x; p < p1; p += blockDim.x) mine += tab[p].sig != 0ull;
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_down(mine, o);
    if ((threadIdx.x & 63u) == 0 && mine) atomicAdd(&s_cnt, mine);
    __syncthreads();
    if (threadIdx.x == 0) { s_base = s_cnt ? atomicAdd(cnt, s_cnt) : 0u; s_cnt = 0; }
    __syncthreads();
    for (uint32_t p = p0 + threadIdx.x; p < p1; p += blockDim.x) {
        const unsigned long long v = tab[p].sig;
        if (v != 0ull) {
            const uint32_t j = s_base + atomicAdd(&s_cnt, 1u);
            keys[j] = v;
            slots[j] = p;
        }
    }
}

// r-th signature in order: the set's number, its representative and the length of its list
__global__ void k_cs_hash_ids(const uint32_t* __restrict__ slots_s, uint32_t n_sets, CsSlot* __restrict__ tab, const uint32_t* __restrict__ seg_off,
                              uint32_t* __restrict__ rep, uint32_t* __restrict__ len) {
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n_sets; r += gridDim.x * blockDim.x) {
        CsSlot* sl = tab + slots_s[r];
        sl->id = r;
        const uint32_t a = sl->rep;
        rep[r] = a;
        len[r] = seg_off[a + 1] - seg_off[a];
    }
}

// the dictionary's ids in the width the resident image keeps them in (behind the verification, on the side stream)
template <class T>
__global__ void k_cs_narrow(const uint32_t* __restrict__ in, uint64_t n, T* __restrict__ out) {
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) out[i] = (T)in[i];
}

// dictionary entries: the lanes of a wavefront copy each representative's list together, 64 ids at a time
__global__ __launch_bounds__(ABLK) void k_cs_hash_copy(const uint32_t* __restrict__ rep, const uint32_t* __restrict__ cs_off, uint32_t n_sets, const uint32_t* __restrict__ seg_off,
                                                       const uint32_t* __restrict__ pg, uint32_t* __restrict__ cs_ids) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t nblk = (n_sets + ABLK - 1) / ABLK;
    for (uint32_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
        const uint32_t r = blk * ABLK + threadIdx.x;
        uint32_t src = 0, len = 0, dst = 0;
        if (r < n_sets) {
            src = seg_off[rep[r]];
            dst = cs_off[r];
            len = cs_off[r + 1] - dst;
        }
        uint64_t todo = __ballot(len != 0);
        while (todo) {
            const int t = __builtin_ctzll(todo);
            todo &= todo - 1;
            const uint32_t s0 = __shfl(src, t), l0 = __shfl(len, t), d0 = __shfl(dst, t);
            for (uint32_t j = lane; j < l0; j += 64) cs_ids[d0 + j] = pg[s0 + j];
        }
    }
}

__global__ void k_cs_hash_tcol(const uint32_t* __restrict__ slot_of, const CsSlot* __restrict__ tab, uint32_t nk, uint32_t* __restrict__ tcol) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nk; i += gridDim.x * blockDim.x) tcol[i] = tab[slot_of[i]].id;
}

}  // namespace

static int g_weak_signature = 0;
static unsigned long long g_exact_passes = 0, g_hash_attempts = 0;
void bft_test_weak_signature(int how) { g_weak_signature = how; }
unsigned long long bft_test_exact_passes(void) { return g_exact_passes; }

namespace {

// what the steps of one interning share: the caller's lists, the counts channel of its stream, the signatures, the outputs as they get allocated
struct Intern {
    const uint32_t* seg_off;
    const uint32_t* pg;
    uint64_t nk, np;
    hipStream_t s;
    BftCounts scan;
    DevArr<uint64_t> sig;
    DevArr<uint32_t> iota, bad;
    uint32_t* tcol = nullptr;  // [nk]
    uint32_t* cs_off = nullptr;  // [n_sets + 1]
    uint32_t* cs_ids = nullptr;  // [n_ids]
    uint64_t n_sets = 0, n_ids = 0;
    Intern(const uint32_t* so, const uint32_t* ids, uint64_t nk_, uint64_t np_, hipStream_t st) : seg_off(so), pg(ids), nk(nk_), np(np_), s(st), scan(st) {}
};
// the arrays of the hash path: steps 1 and 2 (released together, behind step 2's launches)
struct HashPath {
    DevArr<CsSlot> tab;
    DevArr<uint32_t> slot_of, cnt;
    DevArr<uint64_t> keys, keys_s;
    DevArr<uint32_t> slots, slots_s, rep, len;
};

// Step 1 -- by a hash of the signatures (kernels above).  The table starts at nk / 8 slots (a pan-genome has far fewer distinct lists than
// k-mers) and is retried at 2 nk when more than half of it fills: then every list may be distinct.  *found: the sets are numbered, tcol and
// cs_off are written and cs_ids is allocated (n_sets, n_ids); else nothing stands and the exact pass has to run.
int intern_hash(Intern& in, HashPath& hp, uint64_t distinct_hint, DevBuf& d_cs_off, DevBuf& d_cs_ids, bool* found) {
    BftCounts& scan = in.scan;
    const uint64_t nk = in.nk;
    hipStream_t s = in.s;
    bool done = false;
    CK(hp.slot_of.alloc(nk));
    CK(hp.cnt.alloc(3));
    uint64_t n_slots = 1ull << 16;
    while (n_slots < nk / 8 || n_slots < 3 * distinct_hint) n_slots <<= 1;  // (distinct_hint: lists the caller knows to differ -- a merge's old sets)
    for (int attempt = 0; attempt < 2 && !done; attempt++) {
        if (attempt) {
            while (n_slots < 2 * nk) n_slots <<= 1;
        }
        g_hash_attempts++;
        CK(hp.tab.alloc_zero(n_slots, s));
        HIPCK(hipMemsetAsync(hp.cnt.p, 0, 12, s));
        CK(bft_launch256(k_cs_hash_insert, nk, s, in.sig, (uint32_t)nk, hp.tab, (uint32_t)(n_slots - 1), hp.slot_of, hp.cnt));
        CK(scan.publish(hp.cnt, 2, 0));
        bft_stage("colour sets: hash of the signatures", (double)nk * (8 + 4) + (double)n_slots * 16, s);
        CK(scan.wait());
        if (scan.get(1) == 0 && scan.get(0) * 2 <= n_slots) done = true;
        else if (n_slots >= 2 * nk) break;  // (cannot happen: at most nk signatures in 2 nk slots)
    }
    *found = done;
    if (!done) return 0;
    const uint64_t n_sets = in.n_sets = scan.get(0);
    CK(hp.keys.alloc(n_sets));
    CK(hp.keys_s.alloc(n_sets));
    CK(hp.slots.alloc(n_sets));
    CK(hp.slots_s.alloc(n_sets));
    CK(hp.rep.alloc(n_sets));
    CK(hp.len.alloc(n_sets));
    CK(bft_launch256(k_cs_hash_compact, n_slots, s, hp.tab, (uint32_t)n_slots, hp.keys, hp.slots, hp.cnt + 2));
    CK((bft_rs::sort_pairs<uint64_t, uint32_t, bft_rs::SHAPE_LIGHT>(hp.keys, hp.slots, n_sets, hp.keys_s, hp.slots_s, 0, 64, s)));
    CK(bft_launch256(k_cs_hash_ids, n_sets, s, hp.slots_s, (uint32_t)n_sets, hp.tab, in.seg_off, hp.rep, hp.len));
    CK(d_cs_off.alloc((n_sets + 1) * sizeof(uint32_t)));
    in.cs_off = d_cs_off.as<uint32_t>();
    CK(scan.enqueue(hp.len, in.cs_off, n_sets, 0, true));
    CK(bft_launch256(k_cs_hash_tcol, nk, s, hp.slot_of, hp.tab, (uint32_t)nk, in.tcol));
    bft_stage("colour sets: distinct signatures sorted, ids, set per k-mer", (double)n_slots * 16 + (double)n_sets * (12 * 2 * 8 + 24) + (double)nk * 8, s);
    CK(scan.wait());
    in.n_ids = scan.get(0);
    CK(d_cs_ids.alloc(in.n_ids * sizeof(uint32_t)));
    in.cs_ids = d_cs_ids.as<uint32_t>();
    return 0;
}

// Step 2 -- the dictionary entries copied out of their representatives' lists, then every k-mer's list compared with the entry it was given
// (*bad: how many differ), on stream t: the interning's own -- where the copy is a stage of its own and *bad is zeroed here -- or a side stream,
// whose caller has zeroed *bad in front of the event that t waits for.
int intern_copy_verify(const Intern& in, const uint32_t* rep, uint32_t* bad, hipStream_t t) {
    CK(bft_launch256(k_cs_hash_copy, in.n_sets, t, rep, in.cs_off, (uint32_t)in.n_sets, in.seg_off, in.pg, in.cs_ids));
    if (t == in.s) {
        bft_stage("colour sets: dictionary copied", (double)in.n_ids * 8 + (double)in.n_sets * 12, t);
        HIPCK(hipMemsetAsync(bad, 0, 4, t));
    }
    CK(bft_launch256(k_cs_verify, in.nk, t, in.tcol, in.cs_off, in.cs_ids, in.seg_off, in.pg, (uint32_t)in.nk, bad));
    return 0;
}
bool tail_usable(BftInternTail* tail) {
    return tail && tail->side && tail->pin.p && (tail->done || hipEventCreateWithFlags(&tail->done, hipEventDisableTiming) == hipSuccess) &&
           (tail->ready || hipEventCreateWithFlags(&tail->ready, hipEventDisableTiming) == hipSuccess);
}
// step 2 on the tail's side stream, behind everything enqueued so far; the caller collects the verdict later (BftInternTail::wait)
int intern_tail_deferred(Intern& in, HashPath& hp, BftInternTail* tail) {
    hipStream_t s = in.s, t2 = tail->side;
    const uint64_t n_ids = in.n_ids;
    tail->rep.swap(hp.rep);
    CK(tail->bad.alloc_zero(4, s));
    if (tail->narrow_w < 4) CK(tail->narrow.alloc(n_ids * tail->narrow_w));  // (before `ready`: whatever held the block last was enqueued on s)
    HIPCK(hipEventRecord(tail->ready, s));
    HIPCK(hipStreamWaitEvent(t2, tail->ready, 0));
    CK(intern_copy_verify(in, tail->rep.as<uint32_t>(), tail->bad.as<uint32_t>(), t2));
    CK(bft_pin_publish(tail->pin, t2, tail->bad.as<uint32_t>(), 1, 0));
    const dim3 grid(bft_grid_for((in.nk + ABLK - 1) / ABLK)), block(ABLK);  // (the narrowing runs in the shape of the passes over the k-mers)
    if (n_ids && tail->narrow_w == 1) hipLaunchKernelGGL(k_cs_narrow<uint8_t>, grid, block, 0, t2, in.cs_ids, n_ids, tail->narrow.as<uint8_t>());
    if (n_ids && tail->narrow_w == 2) hipLaunchKernelGGL(k_cs_narrow<uint16_t>, grid, block, 0, t2, in.cs_ids, n_ids, tail->narrow.as<uint16_t>());
    HIPCK(hipGetLastError());
    HIPCK(hipEventRecord(tail->done, t2));
    bft_stage("+colour sets: dictionary copied, every list verified, ids narrowed (side stream)",
              (double)n_ids * 8 + (double)in.n_sets * 12 + (double)in.np * 8 + (double)in.nk * 12 + (tail->narrow_w < 4 ? (double)n_ids * (4 + tail->narrow_w) : 0.0), t2);
    tail->pending = true;
    return 0;  // (tab, slot_of ... go back to the cache under this stream's tag: what reads them was enqueued on s before this point)
}
// step 2 on the interning's stream, its verdict waited for.  *ok = false: two different lists with one signature -- the exact pass compares the lists
int intern_tail_here(Intern& in, HashPath& hp, bool* ok) {
    BftCounts& scan = in.scan;
    CK(intern_copy_verify(in, hp.rep, in.bad, in.s));
    CK(scan.publish(in.bad, 1, 1));
    bft_stage("colour sets: every list verified", (double)in.np * 8 + (double)in.nk * 12, in.s);
    CK(scan.wait());
    *ok = (uint32_t)scan.get(1) == 0;
    return 0;
}

// Step 3 -- the exact pass: every k-mer's list sorted on (signature, second key, k-mer number), equal lists found by comparing the lists.
// Both sorts are stable and over all 64 bits, the second key's first: the distinct sets end up numbered by (signature, second key, first
// k-mer that holds the set).  Where no two sets share a signature that is the order of the signatures, the hash path's numbering; where
// two do, k_cs_verify has sent every build of these lists here, so the numbering is still a function of the lists alone.
int intern_exact(Intern& in, DevBuf& d_cs_off, DevBuf& d_cs_ids) {
    BftCounts& scan = in.scan;
    const uint64_t nk = in.nk;
    hipStream_t s = in.s;
    uint32_t nbad = 0;
    g_exact_passes++;
    DevArr<uint64_t> key2, key2_s;
    DevArr<uint32_t> ord1;
    DevArr<uint64_t> sig_g, sig_s;
    DevArr<uint32_t> order, head0, r0, headpos, canon, head, len, csid, off;
    CK(key2.alloc(nk));
    CK(key2_s.alloc(nk));
    CK(ord1.alloc(nk));
    CK(sig_g.alloc(nk));
    CK(sig_s.alloc(nk));
    CK(order.alloc(nk));
    CK(head0.alloc(nk));
    CK(r0.alloc(nk));
    CK(headpos.alloc(nk));
    CK(canon.alloc(nk));
    CK(head.alloc(nk));
    CK(len.alloc(nk));
    CK(csid.alloc(nk));
    CK(off.alloc(nk));
    const uint32_t n32 = (uint32_t)nk;
    CK(bft_launch256(k_cs_key2, nk, s, in.seg_off, in.pg, n32, g_weak_signature, key2));
    CK((bft_rs::sort_pairs<uint64_t, uint32_t, bft_rs::SHAPE_LIGHT>(key2, in.iota, nk, key2_s, ord1, 0, 64, s)));
    CK(bft_launch256(k_cs_gather64, nk, s, in.sig, ord1, n32, sig_g));
    CK((bft_rs::sort_pairs<uint64_t, uint32_t, bft_rs::SHAPE_LIGHT>(sig_g, ord1, nk, sig_s, order, 0, 64, s)));
    CK(bft_launch256(k_cs_gather64, nk, s, key2, order, n32, key2_s));  // (the second key in the final order)
    CK(bft_launch256(k_cs_heads, nk, s, sig_s, key2_s, order, in.seg_off, in.pg, n32, head0));
    CK(scan.run(head0, r0, nk, nullptr));
    CK(bft_launch256(k_cs_headpos, nk, s, head0, r0, n32, headpos));
    CK(bft_launch256(k_cs_canon, nk, s, sig_s, key2_s, order, head0, r0, headpos, in.seg_off, in.pg, n32, canon, head, len));
    CK(bft_launch256(k_cs_spread, nk, s, head0, r0, headpos, n32, canon));
    CK(scan.run(head, csid, nk, &in.n_sets));
    CK(scan.run(len, off, nk, &in.n_ids));
    CK(d_cs_off.alloc((in.n_sets + 1) * sizeof(uint32_t)));
    CK(d_cs_ids.alloc(in.n_ids * sizeof(uint32_t)));
    in.cs_off = d_cs_off.as<uint32_t>();
    in.cs_ids = d_cs_ids.as<uint32_t>();
    {
        const uint32_t t32 = (uint32_t)in.n_ids;
        HIPCK(hipMemcpyAsync(in.cs_off + in.n_sets, &t32, 4, hipMemcpyHostToDevice, s));
    }
    CK(bft_launch256(k_cs_assign, nk, s, order, head, canon, csid, off, in.seg_off, in.pg, n32, in.tcol, in.cs_off, in.cs_ids));
    HIPCK(hipMemsetAsync(in.bad.p, 0, 4, s));
    CK(bft_launch256(k_cs_verify, nk, s, in.tcol, in.cs_off, in.cs_ids, in.seg_off, in.pg, n32, in.bad));
    HIPCK(hipMemcpyAsync(&nbad, in.bad.p, 4, hipMemcpyDeviceToHost, s));
    HIPCK(hipGetLastError());
    HIPCK(hipStreamSynchronize(s));
    if (nbad) return bft_fail(BFT_GPU_E_LIMIT, "colour-set interning self-check failed");
    return 0;
}

}  // namespace

// Interning of the colour sets (sorted genome-id list of each distinct k-mer, CSR seg_off/pg) into a dictionary: a 64-bit signature
// per list, equal signatures found through a hash table (k_cs_hash_*), sets numbered in the order of their signatures, then a
// verification pass that compares EVERY k-mer's list with the dictionary entry it was given.  A mismatch -- two different lists with
// one signature -- sends the build through the exact pass: the lists sorted on (signature, a second key, k-mer number), equal lists found by
// comparing the lists themselves, with their predecessor and, where both keys tie, with the earlier lists of the tie.
// Two different sets can therefore never share an id, and two equal sets always do, on either path (tests/test_gpu_intern_edges.py).
// Numbering: the sets in the order of (signature, second key, first k-mer that holds the set).  The hash path stands only when no two sets share
// a signature, where that is the order of the signatures alone; the same lists take the same path, so an image is a function of its lists.
int bft_intern_colors_gpu(const uint32_t* d_seg_off, const uint32_t* d_pg, uint64_t nk, uint64_t np, hipStream_t s, DevBuf& d_tcol,
                          DevBuf& d_cs_off, DevBuf& d_cs_ids, uint64_t& n_sets, uint64_t& n_ids, uint64_t distinct_hint, BftInternTail* tail, bool exact) {
    n_sets = 0;
    n_ids = 0;
    CK(d_tcol.alloc(nk * sizeof(uint32_t)));
    if (nk == 0) {
        CK(d_cs_off.alloc_zero(4, s));
        CK(d_cs_ids.alloc(4));
        HIPCK(hipStreamSynchronize(s));
        return 0;
    }
    Intern in(d_seg_off, d_pg, nk, np, s);
    in.tcol = d_tcol.as<uint32_t>();
    CK(in.iota.alloc(nk));
    CK(in.bad.alloc(1));
    CK(in.sig.alloc(nk));
    CK(bft_launch256(k_cs_sig, nk, s, d_seg_off, d_pg, (uint32_t)nk, g_weak_signature ? 1 : 0, in.sig, in.iota));
    bft_stage("colour sets: signatures", (double)np * 4 + (double)nk * (4 + 8 + 4), s);
    bool done = false;
    if (!exact) {
        HashPath hp;
        CK(intern_hash(in, hp, distinct_hint, d_cs_off, d_cs_ids, &done));
        if (done && tail_usable(tail)) {
            n_sets = in.n_sets;
            n_ids = in.n_ids;
            return intern_tail_deferred(in, hp, tail);
        }
        if (done) CK(intern_tail_here(in, hp, &done));
    }
    if (!done) CK(intern_exact(in, d_cs_off, d_cs_ids));
    n_sets = in.n_sets;
    n_ids = in.n_ids;
    return 0;
}

// ------------------------------------------------------------------------------------------------
// test hook (tests/test_gpu_intern_edges.py; not part of include/bft_gpu.h): the interning on the caller's CSR lists (device arrays: d_seg_off
// [nk + 1], d_ids [np], ids ascending inside a list).  mode 0: the hash path, everything on the stream; 1: the tail deferred to a side stream
// of the hook's own with narrow_w 1 / 2 / 4, its verdict waited for and, on collisions, the exact call made -- as bft_commit_image does; 2: exact
// at once.  Out: tcol [nk], cs_off [n_sets + 1], cs_ids [n_ids]; d_narrow (mode 1, narrow_w < 4, no collision: what the tail narrowed, n_ids *
// narrow_w bytes; untouched otherwise).  counts: {n_sets, n_ids, exact passes this call took, lists the tail reported as collided, hash tables
// tried}.  A capacity (in entries) too small: nothing is copied, counts are set, BFT_GPU_E_NOSPACE.
// ------------------------------------------------------------------------------------------------
extern "C" int bft_gpu_test_intern(const uint32_t* d_seg_off, const uint32_t* d_ids, uint64_t nk, uint64_t np, int mode, uint32_t narrow_w, uint64_t distinct_hint,
                                   uint32_t* d_tcol, uint32_t* d_cs_off, uint64_t cs_off_cap, uint32_t* d_cs_ids, uint64_t cs_ids_cap, void* d_narrow, uint64_t* counts,
                                   void* hip_stream) {
    if (!d_seg_off || !counts || (nk && (!d_tcol || !d_cs_off)) || (np && (!d_ids || !d_cs_ids))) return bft_fail(BFT_GPU_E_ARG, "NULL argument");
    if (mode < 0 || mode > 2 || (narrow_w != 1 && narrow_w != 2 && narrow_w != 4)) return bft_fail(BFT_GPU_E_ARG, "bad mode or id width");
    if (nk >= 0x7FFFFFFFull || np > 0xFFFFFFFFull) return bft_fail(BFT_GPU_E_LIMIT, "too many lists or ids");
    hipStream_t s = (hipStream_t)hip_stream;
    int dev = 0;
    HIPCK(hipGetDevice(&dev));
    bft_pool_set_stream(dev, s);
    struct Side {  // (declared before the tail: the tail's destructor still synchronises with it)
        hipStream_t st = nullptr;
        ~Side() { if (st) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); } }
    } side;
    const unsigned long long exact0 = g_exact_passes, attempts0 = g_hash_attempts;
    DevBuf tcol, cs_off, cs_ids;
    uint64_t n_sets = 0, n_ids = 0;
    uint32_t collisions = 0;
    bool narrowed = false;
    BftInternTail tail;
    if (mode == 1) {
        HIPCK(hipStreamCreateWithFlags(&side.st, hipStreamNonBlocking));
        tail.side = side.st;
        tail.narrow_w = narrow_w;
        CK(bft_intern_colors_gpu(d_seg_off, d_ids, nk, np, s, tcol, cs_off, cs_ids, n_sets, n_ids, distinct_hint, &tail));
        CK(tail.wait(&collisions));
        if (collisions) CK(bft_intern_colors_gpu(d_seg_off, d_ids, nk, np, s, tcol, cs_off, cs_ids, n_sets, n_ids, 0, nullptr, true));
        else narrowed = narrow_w < 4 && tail.narrow.p && n_ids;
    } else {
        CK(bft_intern_colors_gpu(d_seg_off, d_ids, nk, np, s, tcol, cs_off, cs_ids, n_sets, n_ids, distinct_hint, nullptr, mode == 2));
    }
    counts[0] = n_sets;
    counts[1] = n_ids;
    counts[2] = g_exact_passes - exact0;
    counts[3] = collisions;
    counts[4] = g_hash_attempts - attempts0;
    if (n_sets + 1 > cs_off_cap || n_ids > cs_ids_cap) return bft_fail(BFT_GPU_E_NOSPACE, "dictionary does not fit the caller's arrays");
    if (nk) HIPCK(hipMemcpyAsync(d_tcol, tcol.p, nk * 4, hipMemcpyDeviceToDevice, s));
    if (nk) HIPCK(hipMemcpyAsync(d_cs_off, cs_off.p, (n_sets + 1) * 4, hipMemcpyDeviceToDevice, s));
    if (n_ids) HIPCK(hipMemcpyAsync(d_cs_ids, cs_ids.p, n_ids * 4, hipMemcpyDeviceToDevice, s));
    if (narrowed && d_narrow) HIPCK(hipMemcpyAsync(d_narrow, tail.narrow.p, n_ids * narrow_w, hipMemcpyDeviceToDevice, s));
    HIPCK(hipStreamSynchronize(s));
    return BFT_GPU_OK;
}
