// bft_ingest.h -- insertion from sequences (bft_ingest.hip): what its kernels and its tests agree on.
#pragma once
#include <cstdint>

// k-mer positions per tile of the compaction: one wavefront counts (k_ing_count, k_ing_runs_count) and later places (k_ing_write, k_ing_runs_write)
// the valid positions of one tile, by __ballot / __popcll; the library's scan runs over the tiles' counts.  Pieces of a call larger than
// "flush_pairs" start at multiples of it (k_seq_tiles' table is indexed by position / 64 as well).
constexpr uint32_t BFT_ING_TILE = 64;
// "ingest_chunk_chars": characters of the blob the host form of the stream path stages per chunk
constexpr uint64_t BFT_ING_CHUNK_DEFAULT = (uint64_t)1 << 26;
constexpr uint64_t BFT_ING_CHUNK_MIN = 1024;

// One chunk of the host form: characters [c0, c1) of the blob and the offsets, relative to c0, of the (pieces of) sequences inside it.  A sequence
// that does not fit is cut, and its next piece starts k - 1 characters before the cut: every window lies in exactly one piece.
// (bft_ingest_next_chunk is host code without a device: the plan the tests read.)
struct BftIngCursor {
    uint64_t seq = 0, at = 0;  // the next sequence, and how many of its characters earlier chunks have consumed
};
// Fills `off` (cleared first) with the chunk that starts at the cursor and moves the cursor behind it; returns the chunk's first character in the
// blob.  chunk_chars >= max(BFT_ING_CHUNK_MIN, 2k).  An empty `off` (size 1) cannot happen while cur.seq < nb_seqs.
template <class Vec>
static inline uint64_t bft_ingest_next_chunk(const uint64_t* seq_off, uint64_t nb_seqs, int k, uint64_t chunk_chars, BftIngCursor& cur, Vec& off) {
    off.clear();
    off.push_back(0);
    const uint64_t c0 = cur.seq < nb_seqs ? seq_off[cur.seq] + cur.at : 0;
    uint64_t used = 0;
    while (cur.seq < nb_seqs) {
        const uint64_t rest = seq_off[cur.seq + 1] - seq_off[cur.seq] - cur.at;
        if (used + rest <= chunk_chars) {  // the whole (rest of the) sequence
            used += rest;
            off.push_back(used);
            cur.seq++;
            cur.at = 0;
            continue;
        }
        const uint64_t room = chunk_chars - used;
        if (room >= (uint64_t)k) {  // (rest > room >= k: the piece left over is k characters at least)
            used += room;
            off.push_back(used);
            cur.at += room - (uint64_t)(k - 1);
        }
        break;
    }
    return c0;
}
