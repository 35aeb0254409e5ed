// bft_marking.h -- vertex marks of the index (bft_marking.hip): the layout of the flag array and the selection functor of the library's scan.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define BFT_MK_NONE 0xFFFFFFFFu  // the row of an absent k-mer; a root no seed has hit
#define BFT_MK_ROWS_PER_WORD 16u // two bits per row: row r sits in bits 2 (r % 16) .. + 1 of word r / 16

static inline uint64_t bft_mk_words(uint64_t n_rows) { return (n_rows + BFT_MK_ROWS_PER_WORD - 1) / BFT_MK_ROWS_PER_WORD; }
static inline uint64_t bft_mk_bytes(uint64_t n_rows) { return (n_rows + 3) / 4; }  // what bft_gpu_marks_read / _write move: 4 rows per byte

__host__ __device__ __forceinline__ uint32_t bft_mk_field(uint32_t word, uint32_t row) { return (word >> (2u * (row & 15u))) & 3u; }

// a row is selected when its flag is in the 4-bit mask (input of the scan that places the selected rows; the emission is bft_pg_emit's)
struct BftMkSel {
    const uint32_t* words;
    uint32_t mask;
    __host__ __device__ uint32_t operator()(uint64_t i) const { return (mask >> bft_mk_field(words[i >> 4], (uint32_t)i)) & 1u; }
};
