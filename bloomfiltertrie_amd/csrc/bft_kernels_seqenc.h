// bft_kernels_seqenc.h -- the front of a sequence batch: k_seq_encode (ASCII -> code and "not ACGTU" streams), k_seq_plan (k-mer positions per sequence),
// k_seq_tiles (sequence of every 64-position tile).  Device code shared by the translation units that read sequences: bft_query.hip (sequence queries,
// bft_kernels_seq.h) and bft_ingest.hip (insertion from sequences); each includes it once, bft_ingest.hip inside its unnamed namespace.
#pragma once
// ---- query_sequence (src/bft.c:1241-1351, harness src/file_io.c:1464-1574): every k-mer of every sequence ----
// ASCII -> 2-bit code (A C G T/U = 0 1 2 3, either case), -1 for anything else; branch-free: bits 1 and 2 of the character code
// already separate the four letters ((c >> 1) ^ (c >> 2)) & 3, and a 21-bit mask over 'A'..'U' says which letters count.
__device__ __forceinline__ int nt_code(char ch) {
    const uint32_t c = (uint8_t)ch, idx = (c & 0xDFu) - 0x41u;  // upper-cased, 'A' = 0
    const uint32_t valid_mask = (1u << 0) | (1u << 2) | (1u << 6) | (1u << 19) | (1u << 20);  // A C G T U
    const bool ok = idx < 21u && ((valid_mask >> idx) & 1u);
    return ok ? (int)(((c >> 1) ^ (c >> 2)) & 3u) : -1;
}

// Sequence queries, step 0.  The ASCII blob -> 2 bits per character (32 characters per u64, character c at bits 2(c%32) of
// word c/32: the packed layout of src/fasta.c:11-23 continued over the whole blob) + one "not ACGTU" bit per character.
// One thread per 32 characters; characters past n_chars count as 'A' / good (no window of a sequence reaches them).  A blob that
// is 16-byte aligned is read 32 bytes at a time, any other one byte by byte.
__global__ void k_seq_encode(const char* __restrict__ seqs, uint64_t n_chars, uint64_t n_words, uint64_t* __restrict__ codes, uint32_t* __restrict__ bad) {
    const bool aligned = ((uintptr_t)seqs & 15u) == 0;
    for (uint64_t wi = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; wi < n_words; wi += (uint64_t)gridDim.x * blockDim.x) {
        uint32_t d[8];
        if (aligned && wi * 32 + 32 <= n_chars) {
            const uint4* src = (const uint4*)(seqs + wi * 32);
            const uint4 a = src[0], b = src[1];
            d[0] = a.x; d[1] = a.y; d[2] = a.z; d[3] = a.w; d[4] = b.x; d[5] = b.y; d[6] = b.z; d[7] = b.w;
        } else {
#pragma unroll
            for (int j = 0; j < 8; j++) {
                uint32_t v = 0;
                for (int c = 0; c < 4; c++) {
                    const uint64_t at = wi * 32 + 4 * j + c;
                    v |= (uint32_t)(uint8_t)(at < n_chars ? seqs[at] : 'A') << (8 * c);
                }
                d[j] = v;
            }
        }
        uint64_t cw = 0;
        uint32_t bw = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) {
#pragma unroll
            for (int c = 0; c < 4; c++) {
                const int code = nt_code((char)((d[j] >> (8 * c)) & 0xFFu));
                const int i = 4 * j + c;
                cw |= (uint64_t)(code & 3) << (2 * i);
                bw |= (code < 0 ? 1u : 0u) << i;
            }
        }
        codes[wi] = cw;
        bad[wi] = bw;
    }
}

// ---- plan (positions per sequence) -> window + walk + colour set -> counters ------------------------------------------------
// k_seq_plan: k-mer positions of every sequence of a chunk, on the device (the device-resident entry point never sees the offsets
// on the host): npos[s] = max(len - k + 1, 0).  An exclusive scan of npos gives pos_off.
__global__ void k_seq_plan(const uint64_t* __restrict__ seq_off, uint64_t n_seqs, int k, uint64_t* __restrict__ npos) {
    for (uint64_t s = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; s <= n_seqs; s += (uint64_t)gridDim.x * blockDim.x) {
        if (s == n_seqs) { npos[s] = 0; continue; }  // the scan's last element: the total
        const uint64_t len = seq_off[s + 1] - seq_off[s];
        npos[s] = len >= (uint64_t)k ? len - (uint64_t)k + 1 : 0;
    }
}

// k_seq_tiles: the sequence of the first position of every 64-position tile (last s with pos_off[s] <= 64 t), one binary search
// per tile, once -- the wavefronts of k_seq_walk start from there with one load.  (A search per wavefront pass
// in that kernel was measured: a scalar binary search costs 20 dependent loads on the critical path of every pass, a 64-ary
// wavefront-wide search 256 L2 requests per pass -- the path went from 4.9 to 8 ms per 10^6 reads with it.)
__global__ void k_seq_tiles(const uint64_t* __restrict__ pos_off, uint32_t n_seqs, uint32_t* __restrict__ tile_seq) {
    const uint64_t P = pos_off[n_seqs], ntiles = (P + 63) / 64;
    for (uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; t < ntiles; t += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t p0 = t * 64;
        uint32_t lo = 0, hi = n_seqs;
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (pos_off[mid] <= p0) lo = mid; else hi = mid;
        }
        tile_seq[t] = lo;
    }
}
