// bft_derive.h -- what a handle DERIVES from a committed image (bft_derive.hip): the flat forms, the root tables, the k-mer hash, the walk's view of it,
// the node prefix hash, the launch shape and the compact table.  The steps depend on each other in one order, kept in one place: bft_rederive.
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>
#include <thread>

#include "bft_dev.h"
#include "bft_kh.h"

// The build of the k-mer hash for a table (tk, tcol) that is complete on the device, started on the handle's second stream: the build
// assembles the containers on `stream` meanwhile.  The build sorts and gathers and starves what runs beside it of memory bandwidth and
// latency (k_prefix_flags over the whole table: 0.2 ms alone, 2.8 ms beside it; the root's single-workgroup k_assign_cc: 0.8 -> 3.5 ms),
// so it starts behind those (`after`: an event of the assembly stream) and overlaps the chain of small kernels and read-back counts that
// follows.  bft_kh_finish waits for it.  Any failure just leaves the image without the table.
struct KhFill {
    DevBuf buf, status, ovf_k, ovf_v;
    BftKhScratch scratch;
    BftKhGeo geo;
    uint64_t lines_cap = 0, lines_used = 0;
    uint32_t ovf_n = 0;
    hipEvent_t e0 = nullptr, e1 = nullptr, ew = nullptr;
    hipStream_t s2 = nullptr;
    bool started = false, prepared = false;
    std::thread prep;  // bft_kh_prepare_async
    KhFill() { memset(&geo, 0, sizeof(geo)); }
    ~KhFill() {  // (a build that fails half-way: the fill must be over before its buffers go back to the cache)
        if (prep.joinable()) prep.join();
        if (started && s2) (void)hipStreamSynchronize(s2);
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
        if (ew) (void)hipEventDestroy(ew);
    }
};
// the handle's second stream (low priority: the k-mer hash fill and the interning's tail run beside the build's own chain), made on first use
bool bft_ensure_stream2(bft_gpu* h);
// the host side of the fill that needs no table yet (the second stream, the table's memory, the events), on a thread of its own
void bft_kh_prepare_async(bft_gpu* h, uint64_t nk, uint64_t n_values, KhFill& f);
// run: the stream the fill is enqueued on (null: the handle's second stream, behind `after`)
void bft_kh_start(bft_gpu* h, const uint64_t* d_tk, const uint32_t* d_tcol, uint64_t nk, uint64_t n_sets, KhFill& f, hipStream_t after, hipStream_t run);
bool bft_kh_finish(bft_gpu* h, KhFill& f, double* ms);

// Points h->im at the device arrays of the handle and forgets every derived table but the flat forms (cannot fail): bft_commit_image, before bft_rederive.
void bft_point_image(bft_gpu* h, uint32_t nb_genomes);

// The steps of a re-derivation. Whichever are asked for run in this order: the root range table comes before the walk's root-prefix bits, the k-mer hash
// before the node prefix hash (which by default exists exactly when the hash does not answer), all of them before the launch shape.
enum : unsigned {
    BFT_DERIVE_FLAT = 1u,    // the flat form of the big CCs, and the image pointed at every array of the handle (resets what the steps below derive)
    BFT_DERIVE_ROOT = 2u,    // root direct, range and quartile tables
    BFT_DERIVE_KH = 4u,      // k-mer hash
    BFT_DERIVE_WALK = 8u,    // the root-prefix bits with which the walk looks plain root groups up in the k-mer hash
    BFT_DERIVE_NPH = 16u,    // node prefix hash
    BFT_DERIVE_SHAPE = 32u,  // launch shape of the walk by rule
    BFT_DERIVE_ALL = 63u
};
// What bft_commit_image puts in the k-mer hash's place: the fill built beside the assembly (fill: finished and good, ms: its GPU time), nothing
// (fill null), or a fresh derivation from the committed table (redo: the exact interning replaced the colour sets the fill had read).
struct BftCommitKh { KhFill* fill; double ms; bool redo; };
// Re-derives `steps` of the image h->im points at (FLAT: of h->im.nb_genomes genomes).  Waits for the callers' streams and the handle's own, brings
// the sorted table back where a step reads it (FLAT, ROOT, KH) and drops it again behind them ("compact_table"), refreshes bft_gpu_info's image_bytes.
// Only the wait, the table and FLAT can fail -- the image is then as it was; the accelerators fail soft (the walk keeps the container path).
// commit: the call is the tail of bft_commit_image -- the handle's new arrays are in place, every stream was waited for and the table is resident, so
// nothing waits and nothing can fail (no FLAT); the build's stage marks are dropped between the steps.
int bft_rederive(bft_gpu* h, unsigned steps, const BftCommitKh* commit = nullptr);
int bft_ensure_table(bft_gpu* h);  // "compact_table": the sorted table and the colour set per row, back from the k-mer hash (synchronises)
void bft_drop_table(bft_gpu* h);   // "compact_table": dropped again where the option and the k-mer hash allow it (nothing may still be reading it)
