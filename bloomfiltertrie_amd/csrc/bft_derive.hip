// bft_derive.hip -- everything a handle derives from a committed image (bft_derive.h): the image pointed at the handle's arrays, the root direct / range /
// quartile tables (derived with the walk's own root lookup, bft_walk.h), the k-mer hash and its asynchronous fill beside a build (the kernels: bft_kh.hip),
// the walk's root-prefix bits, the node prefix hash, the launch shape by rule and the compact table -- and bft_rederive, the one place that runs these
// steps in the order they depend on each other: for bft_gpu_set_option's re-derive options, bft_gpu_image_unpack and the tail of bft_commit_image.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../include/bft_gpu.h"
#include "bft_assemble.h"
#include "bft_handle.h"
#include "bft_index.h"
#include "bft_sort.h"
#include "bft_walk.h"

// what the image holds of the device's memory: every stored and derived array (bft_stored.h) and the hash table of the Bloom filters
static uint64_t image_bytes(bft_gpu* h) {
    const BftStoredRows st = bft_stored_rows(h);
    const BftDerivedRows dv = bft_derived_rows(h);
    return bft_rows_resident(st.row, 0, BFT_N_STORED) + bft_rows_resident(dv.row, 0, BFT_N_DERIVED) + h->d_hashmod.bytes;
}

// Points h->im at the device arrays of the handle (cannot fail).
void bft_point_image(bft_gpu* h, uint32_t nb_genomes) {
    BftImage& im = h->im;
    im.k = h->k;
    im.L = h->L;
    im.W = h->W;
    im.nb_genomes = nb_genomes;
    im.n_kmers = h->n_kmers;
    im.hashmod = h->d_hashmod.as<uint32_t>();
    im.nodes = h->d_nodes.as<BftNode>();
    im.bfT = h->d_bfT.as<uint8_t>();
    im.ccs = h->d_ccs.as<BftCC>();
    im.f2w = h->d_f2w.as<uint64_t>();
    im.clus = h->d_clus.as<uint64_t>();
    im.child = h->d_child.as<uint64_t>();
    im.tk = h->d_tk.as<uint64_t>();
    im.kh_lines = nullptr;    // (derive_kmer_hash)
    memset(&im.kh, 0, sizeof(im.kh));
    im.kh_ovf = nullptr;
    im.kh_ovf_val = nullptr;
    im.kh_ovf_n = 0;
    im.rspec = nullptr;
    im.walk_kh = 0;
    im.tcol = h->d_tcol.as<uint32_t>();
    im.uck = h->d_uck.as<uint64_t>();
    im.ucrow = h->d_ucrow.as<uint32_t>();
    im.cs_off = h->d_cs_off.as<uint32_t>();
    im.cs_ids = h->d_cs_ids.p;
    im.cs_w = h->cs_w;
    im.ccx = h->d_ccx.as<BftCCX>();
    im.f18 = h->d_f18.as<uint64_t>();
    im.fent = h->d_fent.as<uint64_t>();
    im.rdir = nullptr;  // derived after this call (derive_root_direct)
    im.rstart = nullptr;
    im.rq = nullptr;
    im.nph = nullptr;   // (derive_node_hash)
    im.nph_mask = 0;
    im.nph_no_uc = 0;
    h->has_cs_bm = false;  // the bitmap form of the colour-set dictionary is derived by the first colour-row query (ensure_cs_bitmaps)
    h->cs_bm_tried = false;
    h->d_cs_bm.release();
    im.emit_cs = 0;
    h->tuned_wgs = 0;
    h->tuned_probe = 0;
    h->im.probe_big = bft_probe_mode(h->opt_probe);
}

// Root direct table: one thread per 18-bit prefix evaluates the root level's Bloom probe + CC lookup on the bound image.
__global__ void k_root_direct(BftImage im, uint64_t* __restrict__ out) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= (1u << 18)) return;
    const BftRootGlobal root(im);
    out[r] = bft_root_direct_entry(im, root, im.nodes[0], r);
}

template <int W>
__global__ void k_root_ranges(BftImage im, uint32_t root_uc_n, uint32_t* __restrict__ out) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r > (1u << 18)) return;
    out[r] = bft_root_range_entry<W>(im, r, r < (1u << 18) ? im.rdir[r] : 0ull, root_uc_n);
}
__global__ void k_root_ranges_check(const uint64_t* __restrict__ rdir, uint32_t* __restrict__ rs) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= (1u << 18)) return;
    const uint32_t a = rs[r];
    if (!(a & BFT_RSTART_SPECIAL) && !bft_root_range_ok(a, rs[r + 1], rdir[r])) rs[r] = a | BFT_RSTART_SPECIAL;  // (readers mask the flag)
}

// Root quartile table (BFT_RQ_*): one thread per root prefix; for a plain group three lower-bound searches on the top two of the
// key bits that follow the root digit.
template <int W>
__global__ void k_root_quartiles(BftImage im, const uint32_t* __restrict__ rs, uint32_t* __restrict__ out) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= (1u << 18)) return;
    out[r] = bft_root_quartile_entry<W>(im, rs[r], rs[r + 1]);
}

// Node prefix hash.  k_nph_ccnode: the node of every CC (one thread per node).  k_nph_fill: one WAVEFRONT per CC below the root,
// one lane per filter2 word (48 bits + the running rank of the bits before it, so a word knows its first cluster without
// looking at the others): set bits -> clusters -> entries, each entry claims a slot of its (node, prefix) bucket with atomicCAS;
// keys whose bucket is full are dropped (the lookup then takes the container path).  (One thread per node -- a few thousand
// threads, each a chain of ~10^3 dependent loads -- took 16 ms on config 3.)
// stats: [0] inserted, [1] dropped, [2] nodes below the root that hold UC rows.
__global__ void k_nph_ccnode(const BftNode* __restrict__ nodes, uint32_t n_nodes, uint32_t* __restrict__ cc_node, unsigned long long* __restrict__ stats) {
    for (uint32_t m = blockIdx.x * blockDim.x + threadIdx.x; m < n_nodes; m += gridDim.x * blockDim.x) {
        const BftNode nd = nodes[m];
        if (m > 0 && nd.uc_n) atomicAdd(&stats[2], 1ull);
        for (uint32_t c = 0; c < nd.ncc; c++) cc_node[nd.cc_first + c] = m;
    }
}
__global__ __launch_bounds__(256) void k_nph_fill(BftImage im, const uint32_t* __restrict__ cc_node, uint32_t first_cc, uint32_t n_ccs, uint64_t* __restrict__ tab,
                                                  uint64_t mask, unsigned long long* __restrict__ stats) {
    const uint32_t lane = threadIdx.x & 63u, wpb = blockDim.x >> 6;
    for (uint32_t c = first_cc + blockIdx.x * wpb + (threadIdx.x >> 6); c < n_ccs; c += gridDim.x * wpb) {
        const BftCC cc = im.ccs[c];
        const uint32_t m = cc_node[c];
        const uint32_t nw = ((1u << (18 - cc.s)) + BFT_F2_BITS_PER_WORD - 1) / BFT_F2_BITS_PER_WORD;
        uint32_t placed_n = 0, dropped_n = 0;
        for (uint32_t w = lane; w < nw; w += 64) {
            const uint64_t fw = im.f2w[cc.f2_off + w];
            uint64_t bits = fw & ((1ull << BFT_F2_BITS_PER_WORD) - 1ull);
            uint32_t clu = (uint32_t)(fw >> BFT_F2_BITS_PER_WORD);  // clusters before this word
            while (bits) {
                const uint32_t b = (uint32_t)__builtin_ctzll(bits);
                bits &= bits - 1ull;
                const uint32_t pu = w * BFT_F2_BITS_PER_WORD + b;
                const uint64_t ce = im.clus[cc.clus_off + clu++];
                const uint32_t len = (ce & BFT_CLUS_MULTI) ? (uint32_t)((ce >> BFT_CLUS_LEN_SHIFT) & 0xFFFFu) : 1u;
                for (uint32_t j = 0; j < len; j++) {
                    const uint64_t ent = (ce & BFT_CLUS_MULTI) ? im.child[cc.child_off + (uint32_t)ce + j] : ce;
                    const uint32_t r = (pu << cc.s) | ((uint32_t)(ent >> BFT_CHILD_PV_SHIFT) & 0xFFu);
                    const uint64_t key = bft_nph_key(m, r);
                    unsigned long long* bk = (unsigned long long*)(tab + bft_nph_bucket(key, mask) * (2 * BFT_NPH_SLOTS));
                    bool placed = false;
                    for (int s = 0; s < BFT_NPH_SLOTS && !placed; s++)
                        if (atomicCAS(&bk[2 * s], (unsigned long long)BFT_NPH_EMPTY, (unsigned long long)key) == BFT_NPH_EMPTY) {
                            bk[2 * s + 1] = ent;
                            placed = true;
                        }
                    placed_n += placed;
                    dropped_n += !placed;
                }
            }
        }
        if (placed_n) atomicAdd(&stats[0], (unsigned long long)placed_n);
        if (dropped_n) atomicAdd(&stats[1], (unsigned long long)dropped_n);
    }
}

// Derives the node prefix hash of the image h->im points at.  An accelerator only: without it the walk keeps the container path.
static void derive_node_hash(bft_gpu* h) {
    h->im.nph = nullptr;
    h->im.nph_mask = 0;
    h->im.nph_no_uc = 0;
    h->nph_inserted = h->nph_dropped = 0;
    const uint64_t n_nodes = h->idx_sizes[0] / sizeof(BftNode);
    if (!h->opt_node_hash || (h->opt_node_hash == 1 && h->im.kh_lines != nullptr && !h->opt_walk_hash) || n_nodes <= 1 || h->info[6] == 0) {
        h->d_nph.release();
        return;
    }
    // keys = the prefixes of the nodes below the root = all prefixes (info[6]) minus the root's (nb_elem of its CCs)
    uint64_t root_prefixes = 0;
    {
        std::vector<BftCC> rc(h->root_ncc);
        if (h->root_ncc && hipMemcpy(rc.data(), h->d_ccs.p, rc.size() * sizeof(BftCC), hipMemcpyDeviceToHost) != hipSuccess) return;  // (the root's CCs come first)
        for (const BftCC& c : rc) root_prefixes += c.nb_elem;
    }
    const uint64_t keys = h->info[6] > root_prefixes ? h->info[6] - root_prefixes : 0;
    uint64_t nbk = 1024;
    while (nbk < keys) nbk <<= 1;  // <= 1 key per 4-slot bucket on average
    const size_t bytes = nbk * BFT_NPH_SLOTS * 16;
    DevBuf stats;
    if (h->d_nph.alloc(bytes) != 0 || stats.alloc_zero(24, h->stream) != 0) { h->d_nph.release(); return; }
    if (hipMemsetAsync(h->d_nph.p, 0xFF, bytes, h->stream) != hipSuccess) { h->d_nph.release(); return; }
    BftImage tmp = h->im;
    const uint64_t n_ccs = h->idx_sizes[2] / sizeof(BftCC);
    DevBuf cc_node;
    if (cc_node.alloc(n_ccs * 4) != 0) { h->d_nph.release(); return; }
    hipLaunchKernelGGL(k_nph_ccnode, dim3(bft_grid_for((n_nodes + 255) / 256)), dim3(256), 0, h->stream, h->d_nodes.as<BftNode>(), (uint32_t)n_nodes, cc_node.as<uint32_t>(),
                       stats.as<unsigned long long>());
    hipLaunchKernelGGL(k_nph_fill, dim3(bft_grid_for((n_ccs + 3) / 4)), dim3(256), 0, h->stream, tmp, cc_node.as<uint32_t>(), h->root_ncc, (uint32_t)n_ccs,
                       h->d_nph.as<uint64_t>(), nbk - 1, stats.as<unsigned long long>());
    unsigned long long st[3] = {0, 0, 0};
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(st, stats.p, 24, hipMemcpyDeviceToHost, h->stream) != hipSuccess ||
        hipStreamSynchronize(h->stream) != hipSuccess) {
        h->d_nph.release();
        return;
    }
    h->nph_inserted = st[0];
    h->nph_dropped = st[1];
    h->im.nph = h->d_nph.as<uint64_t>();
    h->im.nph_mask = nbk - 1;
    h->im.nph_no_uc = st[2] == 0 ? 1u : 0u;
}

static bool kh_wanted(const bft_gpu* h, uint64_t nk) { return h->opt_kmer_hash && nk > 0 && nk < (1ull << 31); }
static bool kh_geo_ok(const bft_gpu* h, const BftKhGeo& g) { return bft_kh_has_kernels(h->W, g.S) && g.nl + BFT_KH_TAIL_LINES < (1ull << 32); }
// the handle's second stream (low priority: the k-mer hash fill and the interning's tail run beside the build's own chain), made on first use
bool bft_ensure_stream2(bft_gpu* h) {
    if (h->stream2) return true;
    int lo = 0, hi = 0;  // (numerically larger = lower priority)
    if (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess) { lo = 0; (void)hipGetLastError(); }
    if (hipStreamCreateWithPriority(&h->stream2, hipStreamNonBlocking, lo) != hipSuccess) { h->stream2 = nullptr; (void)hipGetLastError(); }
    return h->stream2 != nullptr;
}
// the host side of the build that needs no table yet: the second stream, the table's memory, the events (a millisecond of driver
// calls for a gigabyte table that is not in the cache).  n_values: the colour sets of the index, or -- before they are known -- a bound
// (sets <= k-mers): fewer slots per line at worst, i.e. a table allocated larger than needed, never smaller.
static void kh_prepare(bft_gpu* h, uint64_t nk, uint64_t n_values, KhFill& f) {
    f.prepared = false;
    if (!kh_wanted(h, nk)) return;
    if (!bft_ensure_stream2(h)) return;
    f.geo = bft_kh_geometry(h->k, nk, std::max<uint64_t>(1, n_values), h->opt_kh_load);
    if (!kh_geo_ok(h, f.geo)) return;
    f.lines_cap = f.geo.nl + BFT_KH_TAIL_LINES;
    if (f.buf.alloc(f.lines_cap * BFT_KH_LINE_WORDS * 8) != 0 || f.status.alloc(16) != 0 || f.ovf_k.alloc((size_t)BFT_KH_OVF_CAP * h->W * 8) != 0 ||
        f.ovf_v.alloc((size_t)BFT_KH_OVF_CAP * 4) != 0)
        return;
    f.prepared = (f.e0 || hipEventCreate(&f.e0) == hipSuccess) && (f.e1 || hipEventCreate(&f.e1) == hipSuccess) &&
                 (f.ew || hipEventCreateWithFlags(&f.ew, hipEventDisableTiming) == hipSuccess);
    if (!f.prepared) { (void)hipGetLastError(); f.buf.release(); }
}
// ... on a thread of its own while the build's stream is busy with the colour sets
void bft_kh_prepare_async(bft_gpu* h, uint64_t nk, uint64_t n_values, KhFill& f) {
    KhFill* fp = &f;
    try {
        f.prep = std::thread([h, nk, n_values, fp] {
            if (hipSetDevice(h->device) != hipSuccess) { (void)hipGetLastError(); return; }
            bft_pool_set_stream(h->device, h->stream);
            kh_prepare(h, nk, n_values, *fp);
        });
    } catch (...) {  // (no thread to be had: kh_start prepares on the caller's)
    }
}
// run: the stream the build is enqueued on (the handle's second stream behind `after`, or the handle's own)
void bft_kh_start(bft_gpu* h, const uint64_t* d_tk, const uint32_t* d_tcol, uint64_t nk, uint64_t n_sets, KhFill& f, hipStream_t after, hipStream_t run) {
    if (f.prep.joinable()) f.prep.join();
    if (!kh_wanted(h, nk)) return;
    const BftKhGeo geo = bft_kh_geometry(h->k, nk, std::max<uint64_t>(1, n_sets), h->opt_kh_load);
    if (!kh_geo_ok(h, geo)) return;
    // (prepared with a bound on the colour sets: keep the block unless the real geometry needs a tenth less)
    const uint64_t need = geo.nl + BFT_KH_TAIL_LINES;
    if (!f.prepared || f.lines_cap < need || f.lines_cap > need + need / 10) kh_prepare(h, nk, n_sets, f);
    if (!f.prepared) return;
    f.geo = geo;
    if (!run) run = h->stream2;
    bool ok = true;
    if (after && after != run) ok = hipEventRecord(f.ew, after) == hipSuccess && hipStreamWaitEvent(run, f.ew, 0) == hipSuccess;
    ok = ok && hipEventRecord(f.e0, run) == hipSuccess;
    if (run != h->stream) bft_stage("+k-mer hash build starts (side stream)", 0, run);
    ok = ok && bft_kh_sort(d_tk, d_tcol, nk, h->k, h->W, f.geo, f.scratch, run) == 0 && bft_kh_lay(nk, h->k, h->W, f.geo, f.buf.as<uint64_t>(), f.ovf_k.as<uint64_t>(), f.ovf_v.as<uint32_t>(), f.status.as<uint32_t>(), f.scratch, run) == 0 &&
         hipEventRecord(f.e1, run) == hipSuccess;
    // (keys: table in, records out; the sort's passes over the records; the lines written once)
    bft_stage(run != h->stream ? "+k-mer hash build ends (side stream)" : "k-mer hash build", (double)nk * (8.0 * h->W + 4) * 8 + (double)f.geo.nl * 64, run);
    f.s2 = run;
    f.started = true;  // (whatever was enqueued is waited for before the buffers go anywhere)
    if (!ok) { (void)hipGetLastError(); (void)hipStreamSynchronize(run); f.started = false; f.buf.release(); }
}
bool bft_kh_finish(bft_gpu* h, KhFill& f, double* ms) {
    bool ok = f.started && hipStreamSynchronize(f.s2) == hipSuccess;
    f.started = false;
    float t = 0;
    if (ok && hipEventElapsedTime(&t, f.e0, f.e1) == hipSuccess && ms) *ms = t;
    if (f.e0) (void)hipEventDestroy(f.e0);
    if (f.e1) (void)hipEventDestroy(f.e1);
    f.e0 = f.e1 = nullptr;
    uint32_t st[4] = {2, 0, 0, 0};
    if (ok) ok = hipMemcpy(st, f.status.p, 16, hipMemcpyDeviceToHost) == hipSuccess && st[0] == 0 && st[3] <= BFT_KH_OVF_CAP;
    for (DevBuf& b : f.scratch.b) b.release();
    f.lines_used = st[1];
    f.geo.maxd = st[2];  // (a lookup looks no further than the table's largest displacement)
    f.ovf_n = ok ? st[3] : 0;
    if (ok && f.ovf_n) {  // the overflow list, sorted by k-mer (a handful: on the host)
        const int W = h->W;
        std::vector<uint64_t> kk((size_t)f.ovf_n * W), k2(kk.size());
        std::vector<uint32_t> vv(f.ovf_n), v2(f.ovf_n), ord(f.ovf_n);
        ok = hipMemcpy(kk.data(), f.ovf_k.p, kk.size() * 8, hipMemcpyDeviceToHost) == hipSuccess && hipMemcpy(vv.data(), f.ovf_v.p, vv.size() * 4, hipMemcpyDeviceToHost) == hipSuccess;
        for (uint32_t i = 0; i < f.ovf_n; i++) ord[i] = i;
        std::sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) { return std::lexicographical_compare(&kk[(size_t)a * W], &kk[(size_t)a * W] + W, &kk[(size_t)b * W], &kk[(size_t)b * W] + W); });
        for (uint32_t i = 0; i < f.ovf_n; i++) {
            for (int w = 0; w < W; w++) k2[(size_t)i * W + w] = kk[(size_t)ord[i] * W + w];
            v2[i] = vv[ord[i]];
        }
        ok = ok && hipMemcpy(f.ovf_k.p, k2.data(), k2.size() * 8, hipMemcpyHostToDevice) == hipSuccess && hipMemcpy(f.ovf_v.p, v2.data(), v2.size() * 4, hipMemcpyHostToDevice) == hipSuccess;
    }
    if (!ok) { (void)hipGetLastError(); f.buf.release(); }
    if (getenv("BFT_GPU_VERBOSE"))
        fprintf(stderr, "[bft_gpu] k-mer hash: %s, %llu home lines (2^%u x %u), %u slots (%u-bit header fields, %u-byte bodies: %u key bits (%u below the hashed %u, %u of q) + %u + %u value bits), largest displacement %u, %u in the overflow list, %.2f ms\n",
                ok ? "built" : "NOT built", (unsigned long long)f.geo.nl, f.geo.hb - f.geo.t, f.geo.m, f.geo.S, f.geo.f, f.geo.wb, f.geo.kb, f.geo.restb, f.geo.hb, f.geo.qb, f.geo.db, f.geo.cb,
                f.geo.maxd, f.ovf_n, t);
    return ok;
}
// the table of a finished build becomes the image's
static void kh_adopt(bft_gpu* h, KhFill& f, double ms) {
    h->d_kh.swap(f.buf);
    h->kh_lines = f.geo.nl;
    h->kh_ms = ms;
    h->im.kh_lines = h->d_kh.as<uint64_t>();
    h->im.kh = f.geo;
    h->d_kh_ovf_k.swap(f.ovf_k);
    h->d_kh_ovf_v.swap(f.ovf_v);
    h->kh_ovf_n = f.ovf_n;
    if (!f.ovf_n) { h->d_kh_ovf_k.release(); h->d_kh_ovf_v.release(); }
    h->im.kh_ovf = f.ovf_n ? h->d_kh_ovf_k.as<uint64_t>() : nullptr;
    h->im.kh_ovf_val = f.ovf_n ? h->d_kh_ovf_v.as<uint32_t>() : nullptr;
    h->im.kh_ovf_n = f.ovf_n;
}
static void kh_drop(bft_gpu* h) {
    h->d_kh.release();
    h->kh_lines = 0;
    h->kh_ms = 0;
    h->im.kh_lines = nullptr;
    memset(&h->im.kh, 0, sizeof(h->im.kh));
    h->d_kh_ovf_k.release();
    h->d_kh_ovf_v.release();
    h->kh_ovf_n = 0;
    h->im.kh_ovf = nullptr;
    h->im.kh_ovf_val = nullptr;
    h->im.kh_ovf_n = 0;
    h->im.walk_kh = 0;
}

// Derives the k-mer hash of the image h->im points at (BFT_KH_*), on the handle's own stream.  An accelerator only: without it every
// query walks the containers.
static void derive_kmer_hash(bft_gpu* h) {
    kh_drop(h);
    if (!kh_wanted(h, h->n_kmers)) return;
    KhFill f;
    bft_kh_start(h, h->d_tk.as<uint64_t>(), h->d_tcol.as<uint32_t>(), h->n_kmers, h->n_sets, f, nullptr, h->stream);
    double ms = 0;
    if (bft_kh_finish(h, f, &ms)) kh_adopt(h, f, ms);
}

// What the walk needs to look plain root groups up in the k-mer hash: one bit per root prefix, "not a plain suffix group of the root"
// (bit 31 of rstart[r]: child Node, UC rows) -- those keep the containers.
__global__ void k_rspec(const uint32_t* __restrict__ rstart, uint32_t* __restrict__ rspec) {
    const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= (1u << 18) / 32) return;
    uint32_t bits = 0;
    for (uint32_t b = 0; b < 32; b++) bits |= ((rstart[32 * w + b] & BFT_RSTART_SPECIAL) ? 1u : 0u) << b;
    rspec[w] = bits;
}
static void sync_walk_kh(bft_gpu* h) {
    h->im.walk_kh = 0;
    h->im.rspec = nullptr;
    if (!h->im.kh_lines || !h->rstart_ok) return;
    if (h->d_rspec.bytes < (1u << 18) / 8 && h->d_rspec.alloc((1u << 18) / 8) != 0) return;
    hipLaunchKernelGGL(k_rspec, dim3((1u << 18) / 32 / 256), dim3(256), 0, h->stream, h->d_rstart.as<uint32_t>(), h->d_rspec.as<uint32_t>());
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess) return;
    h->im.rspec = h->d_rspec.as<uint32_t>();
    h->im.walk_kh = 1;
}

// "compact_table": the k-mer hash holds every (k-mer, colour set) of the index, so the sorted table tk and tcol -- 12 of the image's
// 41 bytes per k-mer on the 100-genome index -- need not stay resident for presence, colour, branching and sequence queries.  They are
// dropped after a build and come back (a dump of the table's slots + one radix sort: milliseconds) when something asks for rows, an
// extraction, a merge, a .bft file, a packed image or the container walk.
__global__ void k_rows_from_words(const uint64_t* __restrict__ words, uint64_t n, int W, uint64_t* __restrict__ rows) {
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
        for (int w = 0; w < W; w++) rows[i * W + w] = words[(uint64_t)w * n + i];
}
static bool compact_possible(const bft_gpu* h) { return h->im.kh_lines != nullptr && h->n_kmers > 0; }
static void drop_table(bft_gpu* h) {
    if (!h->opt_compact || h->table_dropped || !compact_possible(h)) return;
    h->d_tk.release();
    h->d_tcol.release();
    h->table_dropped = true;
    h->im.tk = nullptr;
    h->im.tcol = nullptr;
    h->info[12] = image_bytes(h);
}
void bft_drop_table(bft_gpu* h) { drop_table(h); }
int bft_ensure_table(bft_gpu* h) {
    if (!h->table_dropped) return 0;
    CK(bft_wait_foreign_stream(h));
    const uint64_t n = h->n_kmers;
    const int W = h->W;
    DevBuf keys, vals, cnt, tmp, tk, tcol;
    CK(keys.alloc(n * W * 8));
    CK(vals.alloc(n * 4));
    CK(tk.alloc(n * W * 8));
    CK(tcol.alloc(n * 4));
    CK(cnt.alloc_zero(8, h->stream));
    CK(bft_kh_dump(h->im, keys.as<uint64_t>(), n, vals.as<uint32_t>(), cnt.as<unsigned long long>(), h->stream));
    unsigned long long got = 0;
    HIPCK(hipMemcpyAsync(&got, cnt.p, 8, hipMemcpyDeviceToHost, h->stream));
    HIPCK(hipStreamSynchronize(h->stream));
    if (got != n) return bft_fail(BFT_GPU_E_HIP, "k-mer hash does not hold the index (compact_table)");
    if (W == 1) {
        CK((bft_rs::sort_pairs<uint64_t, uint32_t>(keys.as<uint64_t>(), vals.as<uint32_t>(), n, tk.as<uint64_t>(), tcol.as<uint32_t>(), 0u, (unsigned)(2 * h->k), h->stream)));
    } else {  // two-word keys: the build's permutation sort (words apart, as the dump wrote them), then rows of two words
        DevBuf sorted;
        CK(sorted.alloc(n * W * 8));
        CK(bft_sort_pairs(h, keys.as<uint64_t>(), n, vals.as<uint32_t>(), n, sorted.as<uint64_t>(), n, tcol.as<uint32_t>(), true));
        hipLaunchKernelGGL(k_rows_from_words, dim3(bft_grid_for((n + 255) / 256)), dim3(256), 0, h->stream, sorted.as<uint64_t>(), n, W, tk.as<uint64_t>());
        HIPCK(hipGetLastError());
    }
    HIPCK(hipStreamSynchronize(h->stream));
    h->d_tk.swap(tk);
    h->d_tcol.swap(tcol);
    h->table_dropped = false;
    h->im.tk = h->d_tk.as<uint64_t>();
    h->im.tcol = h->d_tcol.as<uint32_t>();
    h->info[12] = image_bytes(h);
    return 0;
}

// Launch shape of the container walk when nothing was measured ("tune") or fixed by the caller: two 768-thread workgroups per CU (the
// arrangement that was best or within a few per cent of it on every index measured), 8-row probes once suffix groups
// hold dozens of rows, and the root range table unless most root prefixes are child Nodes (their lookups pay it for nothing).
static void default_launch_shape(bft_gpu* h) {
    h->tuned_wgs = 3;
    // (rows per ROOT prefix: the groups most queries end in hang off the root; deeper levels add prefixes, not rows)
    const uint64_t prefixes = std::max<uint64_t>(1, std::min<uint64_t>(h->info[6], 1ull << 18));
    h->tuned_probe = h->n_kmers / prefixes >= 48 ? 8 : 4;
    h->im.probe_big = bft_probe_mode(h->opt_probe ? h->opt_probe : h->tuned_probe);
    if (h->opt_root_direct == 3 && h->rstart_ok) {
        h->tuned_rstart = h->info[5] * 4 < (1u << 18) ? 1 : 0;
        h->im.rstart = h->tuned_rstart ? h->d_rstart.as<uint32_t>() : nullptr;
        h->im.rq = h->tuned_rstart && h->rq_ok ? h->d_rq.as<uint32_t>() : nullptr;
    }
}

// Derives the table for the image h->im points at (after point_image).  An accelerator only: on any failure the walk simply
// keeps the container path (im.rdir == NULL).
static void derive_root_direct(bft_gpu* h) {
    h->im.rdir = nullptr;
    h->im.rstart = nullptr;
    h->im.rq = nullptr;
    h->rstart_ok = false;
    h->rq_ok = false;
    h->tuned_rstart = -1;
    if (!h->opt_root_direct || h->root_ncc == 0 || h->n_kmers == 0) return;
    if (h->d_rdir.bytes < (8u << 18) && h->d_rdir.alloc(8u << 18) != 0) return;
    BftImage tmp = h->im;
    tmp.rdir = nullptr;
    tmp.debug_stop = 0;
    hipLaunchKernelGGL(k_root_direct, dim3((1u << 18) / 256), dim3(256), 0, h->stream, tmp, h->d_rdir.as<uint64_t>());
    if (hipGetLastError() != hipSuccess) { (void)hipStreamSynchronize(h->stream); return; }
    // (ONE wait for the three tables, at whichever point this function is left: the kernels follow each other on the handle's stream, and a caller's
    // stream must not meet a table that is still being written)
    h->im.rdir = h->d_rdir.as<uint64_t>();
    if (h->opt_root_direct < 2) { if (hipStreamSynchronize(h->stream) != hipSuccess) h->im.rdir = nullptr; return; }
    const size_t rs_bytes = ((1u << 18) + 2) * 4;
    if (h->d_rstart.bytes < rs_bytes && h->d_rstart.alloc(rs_bytes) != 0) { if (hipStreamSynchronize(h->stream) != hipSuccess) h->im.rdir = nullptr; return; }
    tmp.rdir = h->im.rdir;
    const uint32_t root_uc_n = (uint32_t)h->info[14];  // rows of the root's UC (BftNode::uc_n of node 0: bft_gpu_info entry 14, set by the build / the blob)
    const dim3 g((1u << 18) / 256 + 1), b(256);
    switch (h->W) {
    case 1: hipLaunchKernelGGL(k_root_ranges<1>, g, b, 0, h->stream, tmp, root_uc_n, h->d_rstart.as<uint32_t>()); break;
    case 2: hipLaunchKernelGGL(k_root_ranges<2>, g, b, 0, h->stream, tmp, root_uc_n, h->d_rstart.as<uint32_t>()); break;
    case 3: hipLaunchKernelGGL(k_root_ranges<3>, g, b, 0, h->stream, tmp, root_uc_n, h->d_rstart.as<uint32_t>()); break;
    default: hipLaunchKernelGGL(k_root_ranges<4>, g, b, 0, h->stream, tmp, root_uc_n, h->d_rstart.as<uint32_t>()); break;
    }
    hipLaunchKernelGGL(k_root_ranges_check, g, b, 0, h->stream, h->im.rdir, h->d_rstart.as<uint32_t>());
    if (hipGetLastError() != hipSuccess) return;  // (no wait here: the stream is synchronised below, or by whoever uses the tables next)
    h->rstart_ok = true;
    h->im.rstart = h->d_rstart.as<uint32_t>();  // (mode 3: bft_tune_residency decides whether it stays)
    h->rq_ok = false;
    if (!h->opt_root_quartiles || h->L < 2 || (h->d_rq.bytes < (4u << 18) && h->d_rq.alloc(4u << 18) != 0)) {
        if (hipStreamSynchronize(h->stream) != hipSuccess) { h->im.rdir = nullptr; h->im.rstart = nullptr; h->rstart_ok = false; }
        return;
    }
    tmp.rstart = h->im.rstart;
    const dim3 gq((1u << 18) / 256);
    switch (h->W) {
    case 1: hipLaunchKernelGGL(k_root_quartiles<1>, gq, b, 0, h->stream, tmp, h->d_rstart.as<uint32_t>(), h->d_rq.as<uint32_t>()); break;
    case 2: hipLaunchKernelGGL(k_root_quartiles<2>, gq, b, 0, h->stream, tmp, h->d_rstart.as<uint32_t>(), h->d_rq.as<uint32_t>()); break;
    case 3: hipLaunchKernelGGL(k_root_quartiles<3>, gq, b, 0, h->stream, tmp, h->d_rstart.as<uint32_t>(), h->d_rq.as<uint32_t>()); break;
    default: hipLaunchKernelGGL(k_root_quartiles<4>, gq, b, 0, h->stream, tmp, h->d_rstart.as<uint32_t>(), h->d_rq.as<uint32_t>()); break;
    }
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess) { h->im.rdir = nullptr; h->im.rstart = nullptr; h->rstart_ok = false; return; }
    h->rq_ok = true;
    h->im.rq = h->d_rq.as<uint32_t>();
}

// The one re-derive path (bft_derive.h).  FLAT builds the flat arrays aside and swaps them in only once complete: a failure leaves the image as it was.
int bft_rederive(bft_gpu* h, unsigned steps, const BftCommitKh* commit) {
    const bool table = !commit && (steps & (BFT_DERIVE_FLAT | BFT_DERIVE_ROOT | BFT_DERIVE_KH)) != 0;  // (k_root_ranges and the hash's fill read the sorted table)
    if (!commit) {
        CK(bft_wait_foreign_stream(h));
        HIPCK(hipStreamSynchronize(h->stream));
        if (table) CK(bft_ensure_table(h));
    }
    if (steps & BFT_DERIVE_FLAT) {
        DevBuf ccx, f18, fent;
        uint64_t n_f18 = 0, n_fent = 0;
        CK(bft_flatten_gpu(h->d_ccs.as<BftCC>(), h->idx_sizes[2] / sizeof(BftCC), h->d_f2w.as<uint64_t>(), h->d_clus.as<uint64_t>(), h->d_child.as<uint64_t>(),
                           h->opt_flat_min, h->stream, ccx, f18, fent, n_f18, n_fent));
        h->d_ccx.swap(ccx);
        h->d_f18.swap(f18);
        h->d_fent.swap(fent);
        h->n_f18 = n_f18;
        h->n_fent = n_fent;
        bft_point_image(h, h->im.nb_genomes);
    }
    if (steps & BFT_DERIVE_ROOT) derive_root_direct(h);
    if (steps & BFT_DERIVE_KH) {
        if (commit && commit->fill) kh_adopt(h, *commit->fill, commit->ms);  // built during the assembly
        else if (commit && !commit->redo) kh_drop(h);
        else derive_kmer_hash(h);  // (in a commit: after the exact interning, from the committed table and colour sets)
    }
    if (steps & BFT_DERIVE_WALK) sync_walk_kh(h);
    if (commit) {
        bft_trace_mark("root tables");
        bft_stage("root tables", 0, h->stream);
    }
    if (steps & BFT_DERIVE_NPH) derive_node_hash(h);  // (by default the node prefix hash exists exactly when the container walk answers queries)
    if (steps & BFT_DERIVE_SHAPE) default_launch_shape(h);
    h->info[12] = image_bytes(h);
    if (table || commit) drop_table(h);  // ("compact_table")
    return 0;
}
