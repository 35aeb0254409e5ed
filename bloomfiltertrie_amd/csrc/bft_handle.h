// bft_handle.h -- the handle behind the C-ABI (struct bft_gpu) and the host helpers every entry point needs, for the translation units that hold
// entry points: bft_gpu.hip (lifecycle, pool, log, build and commit, options and info: it defines the helpers), bft_image_io.hip (the image read out and
// in: .bft files, the blob, the read-outs, the width of the dictionary's ids; over the tables of bft_stored.h), bft_derive.hip (what the
// handle derives from a committed image, bft_derive.h: root tables, k-mer hash, node prefix hash, launch shape, compact table), bft_query.hip (the k-mer and
// sequence queries, their tuner, the claim slots), bft_run.hip (the build's run stage, the sort and scan test hooks) and the analysis families
// bft_prefix.hip, bft_paths.hip (the path engine and the simple paths), bft_unitigs.hip (its mirrored family), bft_cgraph.hip (the compacted graph over it), bft_bubbles.hip (bubbles and the k-mer -> segment table over its arrays), bft_thread.hip (sequences threaded through it), bft_components.hip, bft_pangenome.hip, bft_genome_matrix.hip, bft_subgraph.hip, bft_marking.hip, bft_setops.hip, bft_union.hip, bft_ingest.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "bft_derive.h"  // bft_rederive, bft_ensure_table / bft_drop_table, the k-mer hash fill of a build (KhFill)
#include "bft_assemble.h"  // BftDeviceIndex (bft_stored.h)
#include "bft_dev.h"
#include "bft_front.h"   // BftPairRun
#include "bft_image.h"
#include "bft_ingest.h"
#include "bft_intern.h"  // BftInternTail
#include "bft_kh.h"
#include "bft_merge.h"  // BftRunOut

// Scratch of ONE query family of a handle: blocks (DevBufs beside it in struct bft_gpu) that belong to the handle, not to a stream -- one stream uses
// them at a time, they grow and never shrink.  A call takes them through a Lease (acquire(), fallible), sizes each block with grow(), and its use
// ends where the lease leaves scope: behind its last launch, and on every error return as well.  While the stream is being captured nothing waits and nothing allocates: the call is refused (the caller makes one direct
// call of that size first, include/bft_gpu.h), and the scratch stays with that stream -- a graph's replays are not ordered against other streams' calls.
struct HandleScratch {
    explicit HandleScratch(const char* w) : what(w) {}
    HandleScratch(const HandleScratch&) = delete;
    HandleScratch& operator=(const HandleScratch&) = delete;
    ~HandleScratch() { if (ev) (void)hipEventDestroy(ev); }
    // b holds `need` bytes at least (a new block: need + slack).  A block this stream may still be using is not replaced before the stream has drained.
    int grow(DevBuf& b, size_t need, size_t slack) {
        if (b.bytes >= need) return 0;
        if (capturing) return bft_fail(BFT_GPU_E_ARG, std::string(what) + " recorded into a graph: make one direct call of this size first (nothing may allocate in a capture)");
        if (!idle) HIPCK(hipStreamSynchronize(stream));
        idle = true;
        return b.alloc(need + slack);
    }
    // One call's use of the scratch, as a scope -- the only way to it.  acquire() may be called again by a helper of the same call; the use ends once,
    // where the lease leaves scope.  (A call that ends its use before an unrelated tail closes the lease's block there.)
    struct Lease {
        explicit Lease(HandleScratch& o) : owner(o) {}
        Lease(const Lease&) = delete;
        Lease& operator=(const Lease&) = delete;
        ~Lease() { if (held) owner.release(); }
        int acquire(hipStream_t s, bool capturing_) {
            CK(owner.acquire(s, capturing_));
            held = true;
            return 0;
        }
    private:
        HandleScratch& owner;
        bool held = false;
    };
private:
    // In use on another stream: that use ends at an event of the handle's own (the other stream is the caller's and may be gone by now).
    int acquire(hipStream_t s, bool capturing_) {
        if (used && stream != s) {
            if (capturing_) return bft_fail(BFT_GPU_E_ARG, std::string(what) + " recorded into a graph: the handle's scratch is in use on another stream");
            HIPCK(ev ? hipEventSynchronize(ev) : hipDeviceSynchronize());
            used = false;
        }
        idle = !used;
        used = true;
        stream = s;
        capturing = capturing_;
        return 0;
    }
    // where the use that acquire() began ends on its stream (a failed event record is swallowed)
    void release() {
        if (capturing) return;  // (an event recorded there would belong to the graph: the next eager call on another stream would wait on it)
        if (!ev && hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) { ev = nullptr; (void)hipGetLastError(); }
        if (ev && hipEventRecord(ev, stream) != hipSuccess) (void)hipGetLastError();
    }
    const char* what;              // the family, for the messages
    hipStream_t stream = nullptr;  // the last user
    hipEvent_t ev = nullptr;       // where its last eager use ends
    bool used = false;             // the blocks may be in use on `stream`
    bool idle = true, capturing = false;  // of the call between acquire() and release(): nothing in flight touches the blocks; its stream is captured
};

// One block cut into 256-byte-aligned arrays.  The same list of take() calls gives the block's size (`off`, whatever the base -- a null one for the
// size alone) and sets the pointers, so the two cannot disagree.
struct Carver {
    uint8_t* base;
    size_t off = 0;
    template <class T>
    void take(T*& p, size_t bytes) { p = (T*)((uintptr_t)base + off); off += (bytes + 255) & ~(size_t)255; }
};

// The claim counters of a handle.  The k-mer hash kernels and the walk claim their blocks of k-mers from a counter instead of splitting them by
// workgroup number (k_query_kh, bft_kh.hip): one counter per stream that launches them -- launches of one stream follow each other, so a counter has one
// user at a time; it only grows, every launch with a range of its own (bft_claims.h).  A handle keeps a counter for each of KH_CTR_SLOTS streams; queried
// on more, it hands the least recently used slot to the new stream once that slot's last launch is known to be over (an event per slot), else the
// launch runs static rounds and is counted (bft_gpu_build_time, entry 20: nothing is silent).  Defined in bft_query.hip.
struct ClaimSlots {
    static constexpr int KH_CTR_SLOTS = 32;
    ClaimSlots() = default;
    ClaimSlots(const ClaimSlots&) = delete;
    ClaimSlots& operator=(const ClaimSlots&) = delete;
    ~ClaimSlots() {
        if (ctr) (void)hipFree(ctr);
        for (int i = 0; i < KH_CTR_SLOTS; i++)
            if (ev[i]) (void)hipEventDestroy(ev[i]);
    }
    // The counters, allocated and zeroed once, when the first image is committed (bft_commit_image, bft_gpu_image_unpack) -- never on the path of a
    // query call.  A failure is final: every launch of the handle then runs static rounds.
    void ensure();
    // ctr: the counter of stream s with the range this launch may use, or {NULL}: every round of blocks is dealt out by workgroup number (not wanted --
    // the option, the environment, a batch too small to matter: the caller's test --, no counters, s being captured, or every slot busy).  units: what
    // the launch deals out (blocks of 256 k-mers, chunks of 1024) -- the slot's base moves on by that plus what the resident workgroups can claim beyond
    // it, so the next launch starts above anything this one can leave behind, finished or not (bft_claims.h).  slot: for launched().
    struct Claim { BftClaimCtr ctr; int slot; };
    Claim take(hipStream_t s, bool wanted, uint64_t units);
    // behind a launch that was given a counter: where the slot's last use ends (only looked at when the slots run out)
    void launched(int slot, hipStream_t s);
    // test hook ("test_stale_claims"): every counter as a launch that never finished can leave it -- anywhere up to the end of the range it was given,
    // i.e. the next launch's base (mode 1: one below it, 2: exactly there, 3: where it started); synchronises the device
    int stale(int mode);
    uint64_t static_launches = 0;  // launches that wanted a counter and found every slot taken by streams with work still in flight
private:
    unsigned long long* ctr = nullptr;  // (its own hipMalloc, not a block of the cache: nothing that was released while still in flight may write here)
    hipStream_t stream[KH_CTR_SLOTS] = {};
    unsigned long long base[KH_CTR_SLOTS] = {};  // where the next launch's range of the slot's counter starts (bft_claims.h)
    uint64_t tick[KH_CTR_SLOTS] = {};            // last use: a handle queried on more streams than slots recycles the least recently used
    uint64_t clock = 0;
    hipEvent_t ev[KH_CTR_SLOTS] = {};            // end of the slot's last launch (recorded once half of the slots are in use)
    int used = 0;
    bool failed = false;
};

struct bft_gpu {
    int k = 0, L = 0, W = 0, B = 0, device = 0, r1 = 0, r2 = 0;
    hipStream_t stream = nullptr;
    std::vector<std::string> genomes;
    uint32_t max_gid_seen = 0;
    bool any_insert = false;
    bool log_g_sorted = true;   // the log's genome ids are non-decreasing
    uint32_t log_last_gid = 0;
    uint64_t opt_flush_pairs = 1ull << 30;  // "flush_pairs": the log is merged into the index before it holds this many pairs

    // Small host batches (the per-k-mer calls of <bft/bft.h>, 4096-byte file chunks): a pinned, device-mapped staging
    // block the kernels read and write directly -- one launch + one stream wait instead of two staged copies around it.
    uint8_t* pin = nullptr;  // [PIN_IN bytes of k-mers | bits | rows | colour sets]
    // Host batches of insertKmers up to a megabyte (a genome of a many-colour collection: 2000 calls of 20 000 k-mers on config 5): a ring
    // of pinned, device-mapped slots -- the batch is copied into the next slot, the packing kernel reads it there over the link, an
    // event says when the slot is free again; nothing waits for the GPU (95 -> ~35 us per call).
    static constexpr size_t RING_SLOT = (size_t)1 << 20;
    static constexpr int RING_SLOTS = 8;
    uint8_t* ring = nullptr;
    hipEvent_t ring_ev[RING_SLOTS] = {};
    bool ring_busy[RING_SLOTS] = {};
    int ring_next = 0;
    ~bft_gpu() {
        if (pin) (void)hipHostFree(pin);
        for (int i = 0; i < RING_SLOTS; i++)
            if (ring_ev[i]) (void)hipEventDestroy(ring_ev[i]);
        if (ring) (void)hipHostFree(ring);
    }

    // pending insert log (SoA: W key arrays of log_cap entries, then genome ids)
    DevBuf log_k, log_g;
    uint64_t log_n = 0, log_cap = 0;
    // One-word keys with room for a genome id beside them (k <= 28: 63 - 2k >= 7 bits) are logged as the COMPOSITES T << log_gb | genome the build's
    // root-prefix split sorts: 8 bytes per pair written at insert time and read by the split's histogram and first pass instead of 12 (no id array:
    // log_g stays empty).  A genome id beyond 2^log_gb, ids that do not ascend, or the general sort ("build_composite" 0) turn the log back
    // into k-mers + ids first (k_log_decompose).
    bool log_comp = false;
    uint32_t log_gb = 0;
    // the insert calls behind the log: positions [lb_end[j - 1], lb_end[j]) carry genome lb_gid[j] -- the multi-word sort reads a pair's id out of this
    // table (a search in a few cached words) instead of gathering it from the log (a fabric request per pair)
    std::vector<uint64_t> lb_end;
    std::vector<uint32_t> lb_gid;
    int opt_comp_log = 1;  // "composite_log": 0 = always k-mers + ids (a test hook: same image)

    uint64_t n_pairs = 0;  // distinct (k-mer, genome) pairs the index holds = sum of the sizes of its k-mers' colour sets

    // image
    bool built = false;
    uint64_t n_kmers = 0;
    DevBuf d_hashmod, d_nodes, d_bfT, d_ccs, d_f2w, d_clus, d_child, d_tk, d_tcol, d_uck, d_ucrow, d_cs_off, d_cs_ids, d_cs_bm;
    DevBuf d_ccx, d_f18, d_fent;  // derived: flat form of the big CCs (bft_flatten_gpu)
    DevBuf d_rdir, d_rstart;      // derived: root direct table (BFT_RDIR_*, k_root_direct) and root range table (BFT_RSTART_*), optional
    DevBuf d_rq;                  // derived: root quartile table (BFT_RQ_*, k_root_quartiles), optional
    int opt_root_quartiles = 1;   // "root_quartiles"
    bool rq_ok = false;
    DevBuf d_nph;                 // derived: node prefix hash (BFT_NPH_*, k_nph_fill), optional
    int opt_node_hash = 1;        // "node_hash": 1 = derived when the image has no k-mer hash (the walk then answers every query), 2 = always, 0 = never
    uint64_t nph_inserted = 0, nph_dropped = 0;
    DevBuf d_kh, d_rspec;         // derived: k-mer hash (BFT_KH_*, bft_kh_build), optional; one "special" bit per root prefix for the walk (sync_walk_kh)
    DevBuf d_kh_ovf_k, d_kh_ovf_v; // its overflow list (sorted k-mers, values)
    uint32_t kh_ovf_n = 0;
    uint64_t kh_lines = 0;        // home lines
    bool opt_kmer_hash = true;    // "kmer_hash"
    bool opt_walk_hash = false;   // "walk_hash": presence / colour queries through the container walk, which looks plain root groups up in the table's regions
    bool opt_compact = true;      // "compact_table" (default on): the sorted table and the colour set per k-mer are dropped once the k-mer hash holds them (bft_ensure_table)
    bool table_dropped = false;   // d_tk / d_tcol are not resident: the k-mer hash is the only copy
    uint32_t opt_kh_load = 55;    // "kmer_hash_load": per cent of the slots of the home lines in use (55: 47.9 G k-mers/s at 15.0 B per k-mer on the config-4 share;
                                  // 50: 48.4 / 16.6; 60: 45.7 / 13.5; 70: 39.3 / 11.7 -- profiles/r04/kh_forms.jsonl)
    double kh_ms = 0;             // GPU time of the last fill
    hipStream_t stream2 = nullptr; // bft_gpu_build fills the k-mer hash here while the containers are assembled on `stream`
    int opt_root_direct = 3;      // "root_direct": 0 = containers, 1 = direct table, 2 = direct table + range table, 3 = 1 or 2, whichever
                                  // measured faster on this image (bft_tune_residency)
    bool rstart_ok = false;       // d_rstart holds the range table of the current image
    int tuned_rstart = -1;        // result of that measurement (-1 = none)
    double rstart_tune_ms[2] = {0, 0};
    uint64_t n_f18 = 0, n_fent = 0;
    uint32_t opt_flat_min = BFT_TRESH_SUF_PREF;  // CCs with at least this many prefixes get the flat form ("flat_min")
    bool has_cs_bm = false, cs_bm_tried = false;
    bool opt_no_cs_bitmaps = false; // test hook ("test_no_cs_bitmaps"): bft_ensure_cs_bitmaps declines, the id lists serve every consumer of the dictionary
    bool opt_no_composite = false;  // test hook ("build_composite" 0): the general sort + flag-array path also for ordered one- and two-word keys
    uint32_t front_redone = 0;      // root-prefix buckets of the last build whose order check failed (bft_front.hip)
    int opt_msd = 1;                // "build_msd": root-prefix buckets + bucket sorts for 2^20 pairs and more (1), always (2: test hook), never (0)
    uint32_t run_road[4] = {0, 0, 0, 0};  // the last build's sort, for bft_gpu_debug_run_road: {1 + road, id bits gb, id bytes beside the keys, split tried}
    uint32_t msd_max_bucket = 0;    // largest root-prefix bucket of the last build's sort (0: one device-wide sort)
    BftImage im;
    std::vector<uint32_t> hashmod;
    std::vector<uint32_t> cs_off, cs_ids;  // host copy of the colour-set dictionary, fetched on first use (host_colorsets)
    uint64_t n_sets = 0, n_ids = 0;
    uint32_t cs_w = 4;  // bytes per genome id of the resident dictionary d_cs_ids (1 / 2 / 4: narrow_ids)
    bool cs_on_host = false;
    uint64_t info[16] = {0};
    double build_ms[5] = {0, 0, 0, 0, 0};

    // kernel timing: off until bft_gpu_kernel_time / set_option("timing", 1) asks for it; events are pooled per handle
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending_ev;
    std::vector<hipEvent_t> free_ev;
    double kernel_ms = 0;
    uint64_t kernel_launches = 0;
    bool timing = false;
    // last work the *_dev entry points put on a caller's stream: image arrays are not released or rewritten before it is done
    struct ExtEv { hipStream_t stream; hipEvent_t ev; bool pending; };
    std::vector<ExtEv> ext;  // one event per caller stream seen (a double-buffered caller alternates between two: neither call blocks the host)
    uint32_t root_ncc = 0;
    uint64_t idx_sizes[9] = {0};  // true bytes of the container arrays and the sorted table (BFT_N_INDEX, bft_stored.h)
    // The container walk (k_query*): how it sits on a CU and how it probes suffix groups.  0 = by rule from the shape of the index
    // (default_launch_shape), or -- after bft_gpu_set_option("tune", 1) -- as measured on the image (bft_tune_residency).
    int opt_wgs_per_cu = 0;   // 1 / 2 workgroups of 1024 threads per CU, 3 = two of 768
    int tuned_wgs = 0;
    int opt_probe = 0;        // suffix-group probe: 4 or 8 rows per block (BftImage::probe_big)
    int tuned_probe = 0;
    double tune_ms[3] = {0, 0, 0};  // best time of the tuning batch per residency 1 / 2 / 3
    int opt_grid_mult = 1;    // grid = resident workgroups x this
    uint32_t opt_test_walk_grid = 0;  // test hook ("test_walk_grid"): the container walk's launches use at most this many workgroups (0: no cap)
    // The query kernels claim their blocks of k-mers from a counter per stream (ClaimSlots).  Batches too small to matter take the static split.
    int opt_query_dynamic = 1;
    uint64_t opt_query_dynamic_min = (uint64_t)1 << 16;  // batches below this many k-mers (lines of work for the branching kernel) keep the static split
    uint32_t opt_query_chunk = 4;  // largest claim, in blocks of 256 k-mers (4 = every claim: the smaller the window of the query stream the
                                   // resident workgroups read at a time, the better -- 2.61 / 2.62 / 2.65 / 2.70 ms at 4 / 16 / 32 / 64)
    ClaimSlots claims;

    // Scratch of the query families: an owner (HandleScratch) and the blocks it guards -- grown, never shrunk, one stream at a time.
    HandleScratch sq{"sequence query"};
    DevBuf sq_codes, sq_bad, sq_npos, sq_poff, sq_tmp, sq_cs, sq_tile;  // sequence queries: codes, plan, scan temporary, colour set per position
    HandleScratch qc{"colour query"};
    DevBuf qc_cs, qc_tmp;            // resident colour-list queries: colour-set id per k-mer, the scan's temporary
    DevBuf qc_kh;                    // k_colors_kh's tile counter and states (bft_kh_colors_scratch_bytes).  A block of its own, never a part of qc_tmp: the
                                     // kernel writes it raw, and bft_scan trusts DevBuf::tag of its temporary (a raw write there corrupts the next scan)
    HandleScratch pm{"prefix query"};
    DevBuf pm_buf, pm_tmp;           // prefix queries (BftPmScratch, bft_prefix.h) and their scans' temporary
    uint64_t pm_n = 0;               // prefixes pm_buf has room for
    HandleScratch sp{"simple paths"};
    DevBuf sp_buf, sp_tmp;           // simple paths (BftSpScratch, bft_paths.h) and their scans' temporary
    uint64_t sp_m = 0;               // rows sp_buf has room for
    HandleScratch cc{"components"};
    DevBuf cc_buf, cc_tmp;           // connected components (BftCcScratch, bft_components.h) and their scans' temporary
    uint64_t cc_m = 0, cc_sets = 0;  // rows and colour sets cc_buf has room for
    HandleScratch pg{"k-mer classes"};
    DevBuf pg_buf, pg_tmp;           // pan-genome k-mer classes (BftPgScratch, bft_pangenome.h) and their scan's temporary
    uint64_t pg_m = 0, pg_sets = 0;  // rows and colour sets pg_buf has room for
    HandleScratch gm{"genome matrix"};
    DevBuf gm_buf, gm_bits;          // genome-by-genome matrix (BftGmScratch, bft_genome_matrix.h): usage / weights / digits / plan; the dense road's bit matrix
    uint64_t gm_sets = 0;            // colour sets gm_buf has room for
    int opt_gm_road = 0;             // test hook ("test_genome_matrix_road"): 0 = by the cost model, 1 = sparse, 2 = dense (same matrix)
    HandleScratch so{"colour-set algebra"};
    DevBuf so_buf;                   // set operations over groups (BftSoScratch, bft_setops.h): colour set per k-mer, presence bits, accumulators, split list
    HandleScratch bb{"bubbles"};
    DevBuf bb_buf, bb_tmp;           // bubbles on the compacted graph (BftBbScratch, bft_bubbles.h): flag and slot per oriented segment; the scan's temporary
    HandleScratch th{"sequence threading"};
    DevBuf th_buf, th_tmp;           // sequence threading over the compacted graph (BftThScratch, bft_thread.h): codes, plan, bucket starts, per-position arrays; the scans' temporary
    HandleScratch ig{"sequence ingest"};
    DevBuf ig_seq, ig_soff;          // insertion from sequences (bft_ingest.hip): the host form's chunk of the blob and its offsets
    DevBuf ig_codes, ig_bad, ig_npos, ig_poff, ig_seqtile, ig_tmp;  // codes, plan and the scans' temporary (as sq_*)
    DevBuf ig_cnt, ig_off;           // valid positions (kept runs) per tile of 64 and their scan
    DevBuf ig_keys, ig_sorted, ig_perm;  // the counting path: the valid windows' keys, sorted, and the permutation of the multi-word sort
    uint64_t opt_ingest_chunk = BFT_ING_CHUNK_DEFAULT;  // "ingest_chunk_chars": characters of the blob the host form stages per chunk (stream path)
    // Vertex marks (bft_marking.hip): on between bft_gpu_marks_begin and bft_gpu_marks_end; insertions and builds are refused meanwhile, so the rows
    // the flags are indexed by cannot move.
    bool marking = false;
    HandleScratch mk{"marks"};
    DevBuf mk_flags;                 // two bits per stored k-mer, 16 rows per 32-bit word (bft_marking.h)
    DevBuf mk_rows, mk_bits;         // a batch's rows in the table and its presence bits
    DevBuf mk_slot, mk_tmp;          // select: the scan of the selection and its temporary
    DevBuf mk_forest;                // reach: bucket starts, the flattened forest, members among the colour sets, the seed slot per root
    bool mk_forest_ok = false;       // mk_forest holds the forest of the eligible rows for (mk_forest_through, mk_forest_ids)
    uint32_t mk_forest_through = 0;
    std::vector<uint32_t> mk_forest_ids;

    bool inject_build_failure = false;  // test hook: the next bft_gpu_build fails right before its commit point (one shot)
    int opt_merge_place = 1;            // "merge_place": how bft_gpu_merge places the k-mers of (this, other): 1 = co-ranked tiles of both tables (bft_union.hip),
                                        // 0 = every row of `other` searched in this one's table, as an insertion build does
                                        // (the default follows tools/bench_merge.py's placement stages at the 50 / 50 split: DESIGN 16)
    bool opt_build_stages = false;      // "build_stages": the next builds record GPU time and bytes per stage (bft_gpu_build_stages)
    struct Stage { std::string name; double ms, bytes; };
    std::vector<Stage> stages;          // of the last build
};

#include "bft_stored.h"  // the handle's stored and derived arrays as tables

// Every ABI call makes the handle's GPU current; the caller's current device is put back when the call returns.
int bft_set_device(bft_gpu* h);
struct DeviceScope {
    int prev = -1;
    DeviceScope() { if (hipGetDevice(&prev) != hipSuccess) { prev = -1; (void)hipGetLastError(); } }
    ~DeviceScope() { if (prev >= 0) (void)hipSetDevice(prev); }
};
#define ENTER(h)     \
    DeviceScope ds_; \
    CK(bft_set_device(h))

// genomes added, one without k-mers included (graph->nb_genomes of the reference); ids inserted without a name count too
static inline uint32_t bft_nb_genomes(const bft_gpu* h) {
    return std::max<uint32_t>(std::max<uint32_t>((uint32_t)h->genomes.size(), h->im.nb_genomes), h->any_insert ? h->max_gid_seen + 1 : 0);
}

double bft_now_ms();
bool bft_stream_capturing(hipStream_t s);
// A *_dev entry point launched on a caller's stream: remember where that work ends.
int bft_note_foreign_stream(bft_gpu* h, hipStream_t s);
// The log merged into the index; need_table = false: the caller is answered by the k-mer hash alone ("compact_table": the sorted table may be away)
int bft_ensure_built(bft_gpu* h, bool need_table = true);
// The insertion log around a batch of n pairs for id_genome that a kernel of the caller's writes (n <= "flush_pairs"): bft_log_prepare merges the log into
// the index first where it would pass "flush_pairs", makes room for n more rows and takes the log out of its composite form where the id has no room
// there; the caller then writes rows [log_n, log_n + n) as k_pack_to_tform does (log_comp ? T << log_gb | id : T-form words + id) and, with the
// writes enqueued (s: a caller's stream they run on, or null for the handle's), bft_log_commit does the bookkeeping of bft_gpu_insert_kmers_dev.
int bft_log_prepare(bft_gpu* h, uint64_t n, uint32_t id_genome);
int bft_log_commit(bft_gpu* h, uint64_t n, uint32_t id_genome, hipStream_t s);
int bft_log_reserve(bft_gpu* h, uint64_t need);  // room for `need` rows in all (an empty log's format is decided here); the log may move: synchronises
// The bitmap form of the colour-set dictionary (d_cs_bm: one dword-aligned row per set behind CS_BM_SLACK zero bytes), derived on the first call per
// image on the handle's stream (synchronises once); has_cs_bm stays false where it would pass 4 GiB or "test_no_cs_bitmaps" is set.
#define CS_BM_SLACK 32u  // zero bytes in front of and behind the bitmap dictionary
int bft_ensure_cs_bitmaps(bft_gpu* h);
// Before image arrays are released, rewritten or re-derived: the queries the caller still has in flight must have drained.
int bft_wait_foreign_stream(bft_gpu* h);

// Timed launches ("timing"): a pair of pooled events around the kernel (no event is created on the launch path once the pool is warm).
int bft_timing_begin(bft_gpu* h, hipStream_t s, hipEvent_t* e0, hipEvent_t* e1);
int bft_timing_end(bft_gpu* h, hipStream_t s, hipEvent_t e0, hipEvent_t e1);
template <class F>
static int bft_timed_launch(bft_gpu* h, hipStream_t s, F&& launch) {
    hipEvent_t e0, e1;
    CK(bft_timing_begin(h, s, &e0, &e1));
    CK(launch());
    return bft_timing_end(h, s, e0, e1);
}

// "build_stages": the marks of one bft_gpu_build or analysis call (bft_stage) become the handle's stage table when the scope ends, however it ends
struct StageScope {
    bft_gpu* h;
    explicit StageScope(bft_gpu* hh, hipStream_t s = nullptr);  // (s: the stream the first stage runs on, when not the handle's)
    ~StageScope();
};

// ---- bft_image_io.hip: the width of the dictionary's genome ids (bft_gpu::cs_w bytes each, resident; 32 bits everywhere else) ----
uint32_t bft_id_width(uint32_t max_gid);  // the narrowest of 1 / 2 / 4 bytes that holds every id up to max_gid
// ids32 (n u32) -> out in width w, synchronised; w == 4: the buffers are swapped
int bft_narrow_ids(DevBuf& ids32, uint64_t n, uint32_t w, hipStream_t s, DevBuf& out);
// h's dictionary as 32-bit ids + base, enqueued on s (k_un_shift, bft_union.hip; timed on `timed` when not null).  *ids: the resident array itself
// where that is what it holds (cs_w == 4, no base), else `tmp`, allocated here; ids null: always into `tmp` (the caller wants a copy of its own).
int bft_dict_ids32(const bft_gpu* h, uint32_t base, hipStream_t s, bft_gpu* timed, DevBuf& tmp, const uint32_t** ids);
// ... and on the host, widened by a few threads: out holds n_ids of them (the caller's own vector: no second copy of a multi-gigabyte dictionary)
int bft_fetch_ids32(bft_gpu* h, uint32_t* out);

// ---- bft_query.hip ----
// rows per probe block of the suffix-group search ("query_probe": 4 or 8) -> BftImage::probe_big
static inline uint32_t bft_probe_mode(int rows) { return rows == 8 ? 1u : 0u; }
int bft_query_residency(const bft_gpu* h);  // resident walk workgroups per CU the next launch runs with: the option, else the measured / default shape, else 2
int bft_tune_residency(bft_gpu* h);         // "tune": the launch shape of the walk measured on the current image (built, table resident; synchronises)
// presence bits (and rows, or colour sets with im.emit_cs) of n packed k-mers on stream s, by whichever of the k-mer hash and the walk answers
int bft_launch_query(bft_gpu* h, const uint8_t* d_kmers, uint64_t n, uint64_t* d_bits64, uint32_t* d_rows, hipStream_t s, int rec_bytes = 0);
// (bft_run.hip) Steps 1-3 of a build: the run of h's insertion log, on h->stream; sets h->front_redone and h->msd_max_bucket
int bft_make_run(bft_gpu* h, BftPairRun& run);
// (bft_run.hip) Stable LSD sort of `total` entries by (keys word 0..W-1 as one big integer, then g) on the handle's stream, synchronised.  keys: SoA with stride `stride`; result in okeys (stride ostride) / og.
int bft_sort_pairs(bft_gpu* h, const uint64_t* keys, uint64_t stride, const uint32_t* g, uint64_t total, uint64_t* okeys, uint64_t ostride, uint32_t* og,
                   bool g_already_ordered, bool is_log = false);

// What only bft_gpu_build carries into the commit: the run's genome-id lists (the input of the interning: its deferred tail reads them, and the exact
// interning runs on them again where two lists shared a signature), the k-mer hash fill it prepared, and that tail.  (In this order: the fill and
// the tail are waited for by their destructors before the lists they read go back to the cache.)
struct BftBuildSide { BftPairRun lists; KhFill khf; BftInternTail tail; };
// Steps 5-7 of a build, from the point where the image-to-be img -- the sorted table, the colour set per row, the dictionary (32-bit ids), their
// counts -- is final: containers, flat forms, k-mer hash (on the second stream), narrowing, commit into h, root tables.  Shared by bft_gpu_build,
// bft_gpu_subgraph and bft_gpu_merge.  np: the (k-mer, genome) pairs img holds; side: null where nothing was interned or prepared (a default
// one then: nothing pending); t0 / t1: start and end of the sort (bft_gpu_build_time).
int bft_commit_image(bft_gpu* h, BftRunOut& img, uint64_t np, double t0, double t1, BftBuildSide* side = nullptr);
