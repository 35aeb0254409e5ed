// bft_image_io.hip -- a handle's image read out and in: .bft files (bft_file.h), the replication blob, the read-outs (bft_gpu_extract, bft_gpu_colorset,
// bft_gpu_colorset_annot, the test hook bft_gpu_debug_get_array) and the width of the dictionary's genome ids (1, 2 or 4 bytes resident; 32 bits
// wherever the build, a merge or the host works on them).  Every list of the image's arrays here is a loop over the tables of bft_stored.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../include/bft_gpu.h"
#include "bft_file.h"
#include "bft_handle.h"
#include "bft_index.h"
#include "bft_union.h"
#include "bft_walk.h"

// ---- the width of the dictionary's genome ids ----
// The genome ids of the dictionary stay resident in the narrowest width that holds every id (a pan-genome of 100 genomes: one byte
// instead of four -- 484 MB -> 121 MB on config 3, 8 of the image's 49 bytes per k-mer); the build and the merge work on 32-bit ids.
template <class T>
__global__ void k_narrow_ids(const uint32_t* __restrict__ in, uint64_t n, T* __restrict__ out) {
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) out[i] = (T)in[i];
}
uint32_t bft_id_width(uint32_t max_gid) { return max_gid < 256u ? 1u : (max_gid < 65536u ? 2u : 4u); }
int bft_narrow_ids(DevBuf& ids32, uint64_t n, uint32_t w, hipStream_t s, DevBuf& out) {
    if (w == 4) { out.swap(ids32); return 0; }
    CK(out.alloc(n * w));
    const dim3 grid(bft_grid_for((n + 255) / 256)), block(256);
    if (n) {
        if (w == 1) hipLaunchKernelGGL(k_narrow_ids<uint8_t>, grid, block, 0, s, ids32.as<uint32_t>(), n, out.as<uint8_t>());
        else hipLaunchKernelGGL(k_narrow_ids<uint16_t>, grid, block, 0, s, ids32.as<uint32_t>(), n, out.as<uint16_t>());
        HIPCK(hipGetLastError());
        HIPCK(hipStreamSynchronize(s));
    }
    return 0;
}

int bft_dict_ids32(const bft_gpu* h, uint32_t base, hipStream_t s, bft_gpu* timed, DevBuf& tmp, const uint32_t** ids) {
    if (ids && h->cs_w == 4 && !base) { *ids = h->d_cs_ids.as<uint32_t>(); return 0; }
    CK(tmp.alloc(std::max<uint64_t>(1, h->n_ids) * 4));
    const auto shift = [&] { return bft_union_shift_ids(h->d_cs_ids.p, h->cs_w, h->n_ids, base, tmp.as<uint32_t>(), s); };
    CK(timed ? bft_timed_launch(timed, s, shift) : shift());
    if (ids) *ids = tmp.as<uint32_t>();
    return 0;
}

int bft_fetch_ids32(bft_gpu* h, uint32_t* out) {
    const uint64_t n = h->n_ids;
    const uint32_t w = h->cs_w;
    if (!n) return 0;
    if (w == 4) { HIPCK(hipMemcpy(out, h->d_cs_ids.p, n * 4, hipMemcpyDeviceToHost)); return 0; }
    BftBigVec<uint8_t> raw;
    raw.resize(n * w);
    HIPCK(hipMemcpy(raw.data(), h->d_cs_ids.p, raw.size(), hipMemcpyDeviceToHost));
    const unsigned nt = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    const uint64_t per = (n + nt - 1) / nt;
    auto widen = [&raw, out, w](uint64_t a, uint64_t b) {
        if (w == 1) for (uint64_t i = a; i < b; i++) out[i] = raw[i];
        else { const uint16_t* r16 = (const uint16_t*)raw.data(); for (uint64_t i = a; i < b; i++) out[i] = r16[i]; }
    };
    std::vector<std::thread> th;
    for (unsigned t = 1; t < nt; t++) {
        const uint64_t a = std::min<uint64_t>(n, t * per), b = std::min<uint64_t>(n, a + per);
        if (a >= b) break;
        try { th.emplace_back(widen, a, b); } catch (...) { widen(a, b); }
    }
    widen(0, std::min<uint64_t>(n, per));
    for (std::thread& x : th) x.join();
    return 0;
}

// ---- one stored array on the host ----
template <class T, class A>
static int download(const BftArrayRow& r, std::vector<T, A>& v) {
    v.resize(r.bytes / sizeof(T));
    if (r.bytes) HIPCK(hipMemcpy(v.data(), r.buf->p, r.bytes, hipMemcpyDeviceToHost));
    return 0;
}

// The colour-set dictionary lives in HBM; only bft_gpu_colorset and bft_gpu_colorset_annot need it on the host (of the image with the log merged in).
static int host_colorsets(bft_gpu* h) {
    CK(bft_ensure_built(h, false));
    if (h->cs_on_host) return 0;
    CK(download(bft_stored_rows(h).row[BFT_S_CS_OFF], h->cs_off));
    h->cs_ids.assign(h->n_ids, 0);
    CK(bft_fetch_ids32(h, h->cs_ids.data()));
    h->cs_on_host = true;
    return 0;
}

// ---- .bft files ----
extern "C" int bft_gpu_load_bft(const char* path, int device, bft_gpu** out) {
    if (!path || !out) return bft_fail(BFT_GPU_E_ARG, "NULL argument");
    *out = nullptr;
    DeviceScope ds_;
    const double t_load0 = bft_now_ms();
    BftFileContent fc;
    std::string err;
    try {  // sizes come from an untrusted file: an allocation failure is an I/O error of this call, not the end of the process
        if (!bft_file_read(path, fc, err)) return bft_fail(BFT_GPU_E_IO, err);
    } catch (const std::bad_alloc&) {
        return bft_fail(BFT_GPU_E_IO, "out of host memory while reading the .bft file (corrupt size field?)");
    } catch (const std::exception& e) {
        return bft_fail(BFT_GPU_E_IO, std::string("malformed .bft file: ") + e.what());
    }
    bft_gpu* h = nullptr;
    CK(bft_gpu_create_seeded(fc.k, device, fc.r1, fc.r2, &h));
    int rc = 0;
    for (const std::string& g : fc.genomes) h->genomes.push_back(g);
    const size_t B = (size_t)h->B;
    {   // the log for every pair of the file at once (it would otherwise grow by doubling: a copy and a synchronisation per step)
        uint64_t pairs = 0;
        for (const auto& v : fc.per_genome) pairs += v.size() / B;
        if (pairs && pairs <= h->opt_flush_pairs && hipSetDevice(device) == hipSuccess) {
            bft_pool_set_stream(device, h->stream);
            (void)bft_log_reserve(h, pairs);  // (a failure here only means the log grows as usual)
        }
    }
    static const bool io_trace = getenv("BFT_GPU_TRACE_IO") != nullptr;
    const double t_io0 = bft_now_ms();
    if (io_trace) fprintf(stderr, "[bft_gpu io] %8.1f ms load: file decoded, handle created, log reserved\n", t_io0 - t_load0);
    for (size_t g = 0; g < fc.per_genome.size() && rc == 0; g++)
        if (!fc.per_genome[g].empty()) rc = bft_gpu_insert_kmers(h, fc.per_genome[g].data(), fc.per_genome[g].size() / B, (uint32_t)g);
    if (io_trace) fprintf(stderr, "[bft_gpu io] %8.1f ms load: every genome's k-mers inserted (host batches)\n", bft_now_ms() - t_io0);
    if (rc == 0) rc = bft_gpu_build(h);
    if (io_trace) fprintf(stderr, "[bft_gpu io] %8.1f ms load: index built\n", bft_now_ms() - t_io0);
    bft_dispose_async(fc);  // (the decoded k-mers of every genome)
    if (rc != 0) {
        const std::string keep = bft_gpu_last_error();
        bft_gpu_free(h);
        return bft_fail(rc, keep);
    }
    *out = h;
    return BFT_GPU_OK;
}

extern "C" int bft_gpu_write_bft(bft_gpu* h, const char* path) {
    if (!h || !path) return bft_fail(BFT_GPU_E_ARG, "NULL argument");
    if (!bft_reference_k(h->k)) return bft_fail(BFT_GPU_E_ARG, "the .bft format requires k % 9 == 0 (reference src/main.c:61-63)");
    ENTER(h);
    static const bool io_trace = getenv("BFT_GPU_TRACE_IO") != nullptr;
    const double t_io0 = bft_now_ms();
    CK(bft_ensure_built(h));
    if (io_trace) fprintf(stderr, "[bft_gpu io] %8.1f ms write: index built, sorted table resident\n", bft_now_ms() - t_io0);
    BftHostImage hi;
    hi.k = h->k; hi.r1 = h->r1; hi.r2 = h->r2;
    hi.genomes = h->genomes;
    while (hi.genomes.size() < h->im.nb_genomes) hi.genomes.push_back("genome_" + std::to_string(hi.genomes.size()));
    const BftStoredRows st = bft_stored_rows(h);
    CK(download(st.row[BFT_S_NODES], hi.nodes));
    CK(download(st.row[BFT_S_CCS], hi.ccs));
    CK(download(st.row[BFT_S_F2W], hi.f2w));
    CK(download(st.row[BFT_S_CLUS], hi.clus));
    CK(download(st.row[BFT_S_CHILD], hi.child));
    CK(download(st.row[BFT_S_UCROW], hi.ucrow));
    CK(download(st.row[BFT_S_TK], hi.tk));
    CK(download(st.row[BFT_S_TCOL], hi.tcol));
    CK(download(st.row[BFT_S_CS_OFF], hi.cs_off));
    hi.cs_ids.resize(h->n_ids);  // the dictionary's ids: 32 bits in the file, resident in 1, 2 or 4 bytes
    CK(bft_fetch_ids32(h, hi.cs_ids.data()));
    if (io_trace) fprintf(stderr, "[bft_gpu io] %8.1f ms write: image arrays on the host\n", bft_now_ms() - t_io0);
    std::string err;
    try {
        if (!bft_file_write(path, hi, err)) return bft_fail(BFT_GPU_E_IO, err);
    } catch (const std::bad_alloc&) {
        return bft_fail(BFT_GPU_E_LIMIT, "out of host memory while serialising the index");
    } catch (const std::exception& e) {
        return bft_fail(BFT_GPU_E_IO, std::string("write_BFT: ") + e.what());
    }
    if (io_trace) fprintf(stderr, "[bft_gpu io] %8.1f ms write: file written and closed\n", bft_now_ms() - t_io0);
    bft_dispose_async(hi);  // (the host copy of the image: gigabytes of vectors)
    return BFT_GPU_OK;
}

// ---- image replication (one contiguous device blob: header, then 256-byte aligned sections) ----
namespace {
constexpr uint64_t BLOB_MAGIC = 0x3430555047544642ull;  // "BFTGPU04"
constexpr int BLOB_HDR_WORDS = 64;
constexpr int BLOB_SECTIONS = BFT_N_STORED + 1, BLOB_NAMES = BFT_N_STORED;  // the stored arrays in their order, then the genome names
constexpr int BLOB_INFO_WORDS = sizeof(bft_gpu::info) / sizeof(uint64_t);
enum { H_MAGIC, H_TOTAL, H_K, H_R1, H_R2, H_NKMERS, H_NPAIRS, H_NSETS, H_NIDS, H_ROOTNCC, H_MAXGID, H_ANYINS, H_NBGEN, H_NNAMES,
       H_CSW, H_STOREANY, H_INFO = 16, H_IDX = H_INFO + BLOB_INFO_WORDS, H_SEC = H_IDX + BFT_N_INDEX };
static_assert(H_IDX == 32 && H_SEC == 41 && H_SEC + BLOB_SECTIONS <= BLOB_HDR_WORDS, "the header's layout is the format BFTGPU04");

inline uint64_t align256(uint64_t v) { return (v + 255ull) & ~255ull; }

// Where the sections of a header start: each at the previous one's end rounded up to 256.  *end: the blob's size.  false: a section does not fit
// below `limit` (a blob read in: its stated size).
bool blob_offsets(const uint64_t* H, uint64_t limit, uint64_t off[BLOB_SECTIONS], uint64_t* end) {
    uint64_t o = BLOB_HDR_WORDS * 8;
    for (int i = 0; i < BLOB_SECTIONS; i++) {
        off[i] = o;
        if (H[H_SEC + i] > limit - o) return false;
        o = align256(o + H[H_SEC + i]);
    }
    *end = o;
    return true;
}

struct BlobPlan {
    uint64_t hdr[BLOB_HDR_WORDS];
    uint64_t off[BLOB_SECTIONS];
    BftStoredRows src;
    std::string names;
};

void plan_blob(bft_gpu* h, BlobPlan& p) {
    uint64_t* H = p.hdr;
    memset(H, 0, sizeof(p.hdr));
    for (const std::string& g : h->genomes) { p.names += g; p.names.push_back('\0'); }
    p.src = bft_stored_rows(h);
    for (int i = 0; i < BFT_N_STORED; i++) H[H_SEC + i] = p.src.row[i].bytes;
    H[H_SEC + BLOB_NAMES] = p.names.size();
    (void)blob_offsets(H, ~0ull, p.off, &H[H_TOTAL]);
    H[H_MAGIC] = BLOB_MAGIC; H[H_K] = h->k; H[H_R1] = h->r1; H[H_R2] = h->r2; H[H_NKMERS] = h->n_kmers; H[H_NPAIRS] = h->n_pairs;
    H[H_NSETS] = h->n_sets; H[H_NIDS] = h->n_ids; H[H_ROOTNCC] = h->root_ncc; H[H_MAXGID] = h->max_gid_seen; H[H_ANYINS] = h->any_insert;
    H[H_NBGEN] = h->im.nb_genomes; H[H_NNAMES] = h->genomes.size(); H[H_CSW] = h->cs_w;  // (word 14: bytes per dictionary id)
    for (int i = 0; i < BLOB_INFO_WORDS; i++) H[H_INFO + i] = h->info[i];
    for (int i = 0; i < BFT_N_INDEX; i++) H[H_IDX + i] = h->idx_sizes[i];
}
}  // namespace

extern "C" int bft_gpu_image_size(bft_gpu* h, uint64_t* nbytes) {
    if (!h || !nbytes) return bft_fail(BFT_GPU_E_ARG, "NULL argument");
    ENTER(h);
    CK(bft_ensure_built(h, false));
    BlobPlan p;
    plan_blob(h, p);
    *nbytes = p.hdr[H_TOTAL];
    return BFT_GPU_OK;
}

extern "C" int bft_gpu_image_pack(bft_gpu* h, void* d_blob, uint64_t cap, void* hip_stream) {
    if (!h || !d_blob) return bft_fail(BFT_GPU_E_ARG, "NULL argument");
    ENTER(h);
    CK(bft_ensure_built(h));
    BlobPlan p;
    plan_blob(h, p);
    if (cap < p.hdr[H_TOTAL]) return bft_fail(BFT_GPU_E_NOSPACE, "blob buffer too small");
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : h->stream;
    uint8_t* d = (uint8_t*)d_blob;
    HIPCK(hipMemcpyAsync(d, p.hdr, sizeof(p.hdr), hipMemcpyHostToDevice, s));
    for (int i = 0; i < BFT_N_STORED; i++)
        if (p.src.row[i].bytes) HIPCK(hipMemcpyAsync(d + p.off[i], p.src.row[i].buf->p, p.src.row[i].bytes, hipMemcpyDeviceToDevice, s));
    if (!p.names.empty()) HIPCK(hipMemcpyAsync(d + p.off[BLOB_NAMES], p.names.data(), p.names.size(), hipMemcpyHostToDevice, s));  // (host)
    HIPCK(hipStreamSynchronize(s));  // the header and the names are host temporaries
    bft_drop_table(h);  // ("compact_table": ensure_built brought the sorted table back for the blob; the source is a group member like the others)
    return BFT_GPU_OK;
}

extern "C" int bft_gpu_image_unpack(const void* d_blob, uint64_t nbytes, int device, bft_gpu** out) {
    if (!d_blob || !out) return bft_fail(BFT_GPU_E_ARG, "NULL argument");
    *out = nullptr;
    DeviceScope ds_;
    if (nbytes < BLOB_HDR_WORDS * 8) return bft_fail(BFT_GPU_E_ARG, "blob shorter than its header");
    int ndev = 0;
    HIPCK(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return bft_fail(BFT_GPU_E_ARG, "bad device index");
    HIPCK(hipSetDevice(device));
    uint64_t H[BLOB_HDR_WORDS];
    HIPCK(hipMemcpy(H, d_blob, sizeof(H), hipMemcpyDeviceToHost));
    if (H[H_MAGIC] != BLOB_MAGIC) return bft_fail(BFT_GPU_E_IO, "not a bft_gpu image blob");
    if (H[H_TOTAL] > nbytes) return bft_fail(BFT_GPU_E_IO, "truncated image blob");
    uint64_t off[BLOB_SECTIONS], end = 0;
    if (!blob_offsets(H, H[H_TOTAL], off, &end)) return bft_fail(BFT_GPU_E_IO, "image blob section out of range");
    bft_gpu* h = nullptr;
    CK(bft_gpu_create_seeded((int)H[H_K], device, (int)H[H_R1], (int)H[H_R2], &h));
    const uint8_t* d = (const uint8_t*)d_blob;
    const BftStoredRows dst = bft_stored_rows(h);  // (for the blocks: the sizes are the header's until the handle has its counts, below)
    int rc = 0;
    for (int i = 0; i < BFT_N_STORED && rc == 0; i++) {
        rc = dst.row[i].buf->alloc(H[H_SEC + i]);
        if (rc == 0 && H[H_SEC + i] &&
            hipMemcpyAsync(dst.row[i].buf->p, d + off[i], H[H_SEC + i], hipMemcpyDeviceToDevice, h->stream) != hipSuccess)
            rc = bft_fail(BFT_GPU_E_HIP, "image blob copy failed");
    }
    std::string names(H[H_SEC + BLOB_NAMES], '\0');
    if (rc == 0 && !names.empty() && hipMemcpyAsync(&names[0], d + off[BLOB_NAMES], names.size(), hipMemcpyDeviceToHost, h->stream) != hipSuccess)
        rc = bft_fail(BFT_GPU_E_HIP, "image blob copy failed");
    if (rc == 0 && hipStreamSynchronize(h->stream) != hipSuccess) rc = bft_fail(BFT_GPU_E_HIP, "image blob copy failed");
    if (rc == 0) {
        size_t a = 0;
        for (uint64_t i = 0; i < H[H_NNAMES] && a < names.size(); i++) {
            const size_t e = names.find('\0', a);
            h->genomes.push_back(names.substr(a, e == std::string::npos ? std::string::npos : e - a));
            a = e == std::string::npos ? names.size() : e + 1;
        }
        h->n_kmers = H[H_NKMERS]; h->n_pairs = H[H_NPAIRS]; h->n_sets = H[H_NSETS]; h->n_ids = H[H_NIDS];
        h->root_ncc = (uint32_t)H[H_ROOTNCC]; h->max_gid_seen = (uint32_t)H[H_MAXGID]; h->any_insert = H[H_ANYINS] != 0;
        h->cs_w = (uint32_t)H[H_CSW];
        if (h->cs_w != 1 && h->cs_w != 2 && h->cs_w != 4) rc = bft_fail(BFT_GPU_E_IO, "image blob: bad dictionary id width");
        for (int i = 0; i < BLOB_INFO_WORDS; i++) h->info[i] = H[H_INFO + i];
        for (int i = 0; i < BFT_N_INDEX; i++) h->idx_sizes[i] = H[H_IDX + i];
        h->cs_on_host = false;
        h->im.nb_genomes = (uint32_t)H[H_NBGEN];
        // ("compact_table", the default: the replica's k-mer hash is derived from the blob's sorted table, which need not stay)
        if (rc == 0) rc = bft_rederive(h, BFT_DERIVE_ALL);
    }
    if (rc != 0) {
        const std::string keep = bft_gpu_last_error();
        bft_gpu_free(h);
        return bft_fail(rc, keep);
    }
    h->built = true;
    h->claims.ensure();
    *out = h;
    return BFT_GPU_OK;
}

// ---- read-outs ----
// Test hook (tests/test_gpu_build.py): raw copy of one array of the image, stored or derived, by its name in the tables of bft_stored.h.
extern "C" int bft_gpu_debug_get_array(bft_gpu* h, const char* name, void* out, uint64_t cap_bytes, uint64_t* nbytes) {
    if (!h || !name) return bft_fail(BFT_GPU_E_ARG, "NULL argument");
    ENTER(h);
    CK(bft_ensure_built(h));
    const BftStoredRows st = bft_stored_rows(h);
    const BftDerivedRows dv = bft_derived_rows(h);
    const BftArrayRow* row = nullptr;
    for (const BftArrayRow& r : st.row) if (!strcmp(name, r.name)) row = &r;
    for (const BftArrayRow& r : dv.row) if (r.name && !strcmp(name, r.name)) row = &r;
    if (!row) return bft_fail(BFT_GPU_E_ARG, "unknown array");
    if (nbytes) *nbytes = row->bytes;
    if (!out) return BFT_GPU_OK;
    if (cap_bytes < row->bytes) return bft_fail(BFT_GPU_E_NOSPACE, "buffer too small");
    if (row->bytes) HIPCK(hipMemcpy(out, row->buf->p, row->bytes, hipMemcpyDeviceToHost));
    return BFT_GPU_OK;
}

// stored T-form rows -> packed k-mers (the reference's layout), on the GPU: bft_gpu_extract copies bytes, not keys
template <int W>
__global__ void k_tform_to_packed(const uint64_t* __restrict__ tk, uint64_t n, int k, int B, uint8_t* __restrict__ out) {
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t t[W], x[W];
#pragma unroll
        for (int w = 0; w < W; w++) t[w] = tk[i * W + w];
        bft_x_from_tform<W>(t, k, x);
        for (int b = 0; b < B; b++) {
            uint64_t v = 0;
#pragma unroll
            for (int w = 0; w < W; w++)
                if (w == (b >> 3)) v = x[w];
            out[i * B + b] = (uint8_t)(v >> (8 * (b & 7)));
        }
    }
}

extern "C" int bft_gpu_extract(bft_gpu* h, uint8_t* kmers_out, uint32_t* colorset_out, uint64_t cap, uint64_t* n_out) {
    if (!h) return bft_fail(BFT_GPU_E_ARG, "NULL handle");
    ENTER(h);
    CK(bft_ensure_built(h));
    if (n_out) *n_out = h->n_kmers;
    if (!kmers_out && !colorset_out) return BFT_GPU_OK;
    if (cap < h->n_kmers) return bft_fail(BFT_GPU_E_NOSPACE, "extract buffer too small");
    const uint64_t n = h->n_kmers;
    if (kmers_out && n) {
        DevBuf packed;
        CK(packed.alloc(n * h->B));
        const dim3 grid(bft_grid_for((n + 255) / 256)), block(256);
        void (*const by_words[4])(const uint64_t*, uint64_t, int, int, uint8_t*) = {k_tform_to_packed<1>, k_tform_to_packed<2>, k_tform_to_packed<3>, k_tform_to_packed<4>};
        hipLaunchKernelGGL(by_words[std::min(h->W, 4) - 1], grid, block, 0, h->stream, h->d_tk.as<uint64_t>(), n, h->k, h->B, packed.as<uint8_t>());
        HIPCK(hipGetLastError());
        HIPCK(hipMemcpyAsync(kmers_out, packed.p, n * h->B, hipMemcpyDeviceToHost, h->stream));
        HIPCK(hipStreamSynchronize(h->stream));
    }
    if (colorset_out && n) HIPCK(hipMemcpy(colorset_out, h->d_tcol.p, n * 4, hipMemcpyDeviceToHost));
    return BFT_GPU_OK;
}

extern "C" int bft_gpu_colorset(bft_gpu* h, uint32_t cs, uint32_t* ids, uint32_t cap, uint32_t* n_out) {
    if (!h) return bft_fail(BFT_GPU_E_ARG, "NULL handle");
    ENTER(h);
    CK(host_colorsets(h));
    if ((uint64_t)cs + 1 >= h->cs_off.size()) return bft_fail(BFT_GPU_E_ARG, "unknown colour set");
    const uint32_t a = h->cs_off[cs], b = h->cs_off[cs + 1];
    if (n_out) *n_out = b - a;
    if (ids) {
        if (cap < b - a) return bft_fail(BFT_GPU_E_NOSPACE, "ids buffer too small");
        memcpy(ids, &h->cs_ids[a], (size_t)(b - a) * 4);
    }
    return BFT_GPU_OK;
}

// The colour set `cs` in the reference's annotation bytes (smallest of modes 0/1/2, compute_best_mode,
// src/annotation.c:634-650) -- what get_annotation hands out as BFT_annotation::annot (src/bft.c:363-387).
extern "C" int bft_gpu_colorset_annot(bft_gpu* h, uint32_t cs, uint8_t* annot, uint32_t cap, uint32_t* n_out) {
    if (!h) return bft_fail(BFT_GPU_E_ARG, "NULL handle");
    ENTER(h);
    CK(host_colorsets(h));
    if ((uint64_t)cs + 1 >= h->cs_off.size()) return bft_fail(BFT_GPU_E_ARG, "unknown colour set");
    const uint32_t a = h->cs_off[cs], b = h->cs_off[cs + 1];
    std::vector<uint8_t> enc;
    bft_annot_encode(b > a ? &h->cs_ids[a] : nullptr, b - a, enc);
    if (n_out) *n_out = (uint32_t)enc.size();
    if (annot) {
        if (cap < enc.size()) return bft_fail(BFT_GPU_E_NOSPACE, "annotation buffer too small");
        memcpy(annot, enc.data(), enc.size());
    }
    return BFT_GPU_OK;
}
