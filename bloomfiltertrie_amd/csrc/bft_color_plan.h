// bft_color_plan.h -- how a batch of colour rows is cut into tiles, and the magic number of the division by the row width: host code only,
// shared by launch_color_rows (bft_query.hip: k_color_rows_bm<false>, k_color_rows_bm<true>, k_color_rows_bm16) and bft_kh_color_rows
// (bft_kh.hip: k_color_rows_kh), and readable without a device through bft_gpu_debug_color_rows_plan (tests/test_colour_cases_host.py checks the
// division over every byte offset a tile can hold, and the bounds the kernels' LDS arrays rely on).
#pragma once
#include <stdint.h>
#include <algorithm>

// The most k-mers a tile may hold = the size of the kernels' LDS arrays (the device code includes this header for them): k_color_rows_bm,
// k_color_rows_bm16 / cr16_stream_tile (whose turn is 64 x CR16_UNROLL chunks), k_color_rows_kh.
#define CR_MAX_TILE_ROWS 2048
#define CR16_UNROLL 1
#define CR16_WAVE_ROWS 1024u
#ifndef BFT_KH_ROWS_TILE
#define BFT_KH_ROWS_TILE 256u
#endif

enum { BFT_ROWS_FORM_DWORD = 0, BFT_ROWS_FORM_16 = 1, BFT_ROWS_FORM_KH = 2 };

struct BftColorRowsPlan {
    uint32_t tile_rows;  // k-mers per tile: a multiple of 4 (dword kernels), 16 (16-byte kernel) or 64 (k-mer-hash row kernel)
    uint32_t div_m;      // byte / rowbytes = (t + ((byte - t) >> 1)) >> (div_l - 1) with t = mulhi(byte, div_m); byte itself when div_l == 0
    uint32_t div_l;
};

// magic number of the division by rowbytes (round-up method, exact on u32)
static inline void bft_color_rows_magic(uint32_t rowbytes, uint32_t* div_m, uint32_t* div_l) {
    uint32_t l = 0;
    while ((1ull << l) < rowbytes) l++;
    *div_l = l;
    *div_m = l ? (uint32_t)(((1ull << 32) * ((1ull << l) - rowbytes)) / rowbytes + 1ull) : 0u;
}

// form: BFT_ROWS_FORM_DWORD (any rowbytes >= 1), BFT_ROWS_FORM_16 or BFT_ROWS_FORM_KH (rowbytes >= 16)
static inline BftColorRowsPlan bft_color_rows_plan(uint32_t rowbytes, int form) {
    BftColorRowsPlan p;
    if (form == BFT_ROWS_FORM_KH) {
        // tiles of about 16 KiB of output, a multiple of 64 k-mers.  (Config 5, 250-byte rows, 4x10^6 k-mers: tiles of 64 / 128 / 256 k-mers at 4, 5, 6
        // workgroups per CU all take 0.37-0.40 ms, the smallest tiles and the most workgroups the least -- the launch costs what the lookups and the
        // rows cost one after the other, whichever way they are interleaved: DESIGN.md.)
        p.tile_rows = std::max(64u, std::min(BFT_KH_ROWS_TILE, ((16u << 10) / rowbytes) & ~63u));
    } else {
        // tiles of ~32 KiB of output (a multiple of 4 k-mers: tiles start dword aligned)
        uint32_t tile_rows = std::min<uint32_t>(CR_MAX_TILE_ROWS, std::max<uint32_t>(4u, ((32768u / rowbytes) + 3u) & ~3u));
        if (form == BFT_ROWS_FORM_16) {
            // tiles of the 16-byte kernel belong to wavefronts, which answer 64 x CR16_UNROLL chunks of 16 bytes per turn: among the tiles of
            // 16..64 KiB of output (a multiple of 16 k-mers, at most CR16_WAVE_ROWS) the one whose last turn is the fullest
            const uint32_t per_turn = 64u * CR16_UNROLL;
            double best = -1.0;
            tile_rows = 16u;
            for (uint32_t tr = 16u; tr <= CR16_WAVE_ROWS; tr += 16u) {
                const uint64_t bytes = (uint64_t)tr * rowbytes;
                // (tiles of 2-4, 4-8, 8-16 and 128-256 KiB were measured on config 5: 0.29-0.32 ms per GB written, no better than these)
                if (bytes > (64u << 10) && best >= 0.0) break;
                if (bytes < (16u << 10) && tr + 16u <= CR16_WAVE_ROWS && (uint64_t)(tr + 16u) * rowbytes <= (64u << 10)) continue;
                const uint64_t nch = (bytes + 15u) / 16u, turns = (nch + per_turn - 1) / per_turn;
                const double eff = (double)nch / (double)(turns * per_turn);
                if (eff >= best) { best = eff; tile_rows = tr; }
            }
        }
        p.tile_rows = tile_rows;
    }
    bft_color_rows_magic(rowbytes, &p.div_m, &p.div_l);
    return p;
}
