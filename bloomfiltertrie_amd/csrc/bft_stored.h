// bft_stored.h -- what an image IS: the twelve arrays a handle stores (everything else is derived from them, bft_derive.h) and the twelve it derives, each
// as one table of {name, block, true bytes} rows over the members of struct bft_gpu.  The blob, the .bft writer, the read-out hook (bft_image_io.hip),
// the footprint and the image's byte count are loops over these tables; bft_point_image (bft_derive.hip) stays the typed view.  Included by
// bft_handle.h, behind the handle.
#pragma once

// The stored arrays, in the blob's section order (the genome names are the section behind them: BFT_N_STORED).
enum BftStored {
    BFT_S_NODES, BFT_S_BFT, BFT_S_CCS, BFT_S_F2W, BFT_S_CLUS, BFT_S_CHILD, BFT_S_UCK, BFT_S_UCROW, BFT_S_TK,  // the containers and the sorted table: idx_sizes[]
    BFT_S_TCOL, BFT_S_CS_OFF, BFT_S_CS_IDS,                                                                  // colour set per k-mer, the dictionary
    BFT_N_STORED
};
constexpr int BFT_N_INDEX = BFT_S_TCOL;  // the arrays whose bytes bft_gpu::idx_sizes keeps (the others follow from n_kmers, n_sets, n_ids and cs_w)
static_assert(sizeof(bft_gpu::idx_sizes) == BFT_N_INDEX * sizeof(uint64_t), "idx_sizes: one entry per container array and the table");
// The derived arrays, grouped as bft_gpu_footprint reports them: flat forms, root tables, node prefix hash, k-mer hash, bitmap dictionary.
enum BftDerived {
    BFT_D_CCX, BFT_D_F18, BFT_D_FENT, BFT_D_RDIR, BFT_D_RSTART, BFT_D_RQ, BFT_D_NPH, BFT_D_KH, BFT_D_RSPEC, BFT_D_KH_OVF_K, BFT_D_KH_OVF_V, BFT_D_CS_BM,
    BFT_N_DERIVED
};

// name: what bft_gpu_debug_get_array answers to (null: not read out).  bytes: the array's true size -- buf->bytes is what was asked of the allocator,
// which the assembly rounds up.
struct BftArrayRow { const char* name; DevBuf* buf; uint64_t bytes; };
struct BftStoredRows { BftArrayRow row[BFT_N_STORED]; };
struct BftDerivedRows { BftArrayRow row[BFT_N_DERIVED]; };

static inline BftStoredRows bft_stored_rows(bft_gpu* h) {
    const uint64_t* z = h->idx_sizes;
    return {{{"nodes", &h->d_nodes, z[BFT_S_NODES]}, {"bfT", &h->d_bfT, z[BFT_S_BFT]}, {"ccs", &h->d_ccs, z[BFT_S_CCS]}, {"f2w", &h->d_f2w, z[BFT_S_F2W]},
             {"clus", &h->d_clus, z[BFT_S_CLUS]}, {"child", &h->d_child, z[BFT_S_CHILD]}, {"uck", &h->d_uck, z[BFT_S_UCK]}, {"ucrow", &h->d_ucrow, z[BFT_S_UCROW]},
             {"tk", &h->d_tk, z[BFT_S_TK]}, {"tcol", &h->d_tcol, h->n_kmers * 4}, {"cs_off", &h->d_cs_off, (h->n_sets + 1) * 4},
             {"cs_ids", &h->d_cs_ids, h->n_ids * (uint64_t)h->cs_w}}};
}
static inline BftDerivedRows bft_derived_rows(bft_gpu* h) {
    return {{{"ccx", &h->d_ccx, h->idx_sizes[BFT_S_CCS] / sizeof(BftCC) * sizeof(BftCCX)}, {"f18", &h->d_f18, h->n_f18 * 8}, {"fent", &h->d_fent, h->n_fent * 8},
             {nullptr, &h->d_rdir, 0}, {"rstart", &h->d_rstart, h->rstart_ok ? ((1ull << 18) + 2) * 4 : 0ull}, {"rq", &h->d_rq, h->rq_ok ? (1ull << 18) * 4 : 0ull},
             {nullptr, &h->d_nph, 0}, {"kh", &h->d_kh, h->kh_lines ? (h->kh_lines + BFT_KH_TAIL_LINES) * BFT_KH_LINE_WORDS * 8 : 0ull},
             {"rspec", &h->d_rspec, h->im.rspec ? (1ull << 18) / 8 : 0ull},
             {"kh_ovf_k", &h->d_kh_ovf_k, (uint64_t)h->kh_ovf_n * h->W * 8}, {"kh_ovf_v", &h->d_kh_ovf_v, (uint64_t)h->kh_ovf_n * 4}, {nullptr, &h->d_cs_bm, 0}}};
}
// what rows [a, b) of a table hold of the device's memory
static inline uint64_t bft_rows_resident(const BftArrayRow* r, int a, int b) {
    uint64_t s = 0;
    for (; a < b; a++) s += r[a].buf->bytes;
    return s;
}

// The one place idx_sizes[] is filled from a fresh assembly (bft_commit_image; a replica takes them from its blob's header).
static inline void bft_set_idx_sizes(bft_gpu* h, const BftDeviceIndex& idx, uint64_t nk) {
    uint64_t* z = h->idx_sizes;
    z[BFT_S_NODES] = idx.n_nodes * sizeof(BftNode); z[BFT_S_BFT] = idx.n_bf8 * 8; z[BFT_S_CCS] = idx.n_ccs * sizeof(BftCC);
    z[BFT_S_F2W] = idx.n_f2w * 8; z[BFT_S_CLUS] = idx.n_clus * 8; z[BFT_S_CHILD] = idx.n_child * 8;
    z[BFT_S_UCK] = idx.n_uc * (uint64_t)h->W * 8; z[BFT_S_UCROW] = idx.n_uc * 4; z[BFT_S_TK] = nk * (uint64_t)h->W * 8;
}
