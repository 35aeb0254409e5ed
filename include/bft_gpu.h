/*
 * bft_gpu.h -- C-ABI of the MI355X-native batched k-mer presence / colour / insertion path of the
 * Bloom Filter Trie.  This is the drop-in boundary: plain pointers and sizes, no C++ or torch
 * types.  Every entry point names the reference interface (GuillaumeHolley/BloomFilterTrie,
 * file:line) it replaces or batches.  Library: bloomfiltertrie_amd/csrc/libbft_gpu.so
 * (hipcc --offload-arch=gfx950).  INTEGRATION.md shows the binding a maintainer adds to the
 * reference's src/file_io.c / src/bft.c.
 *
 * k-mer batches use the reference's packed layout everywhere (parseKmerCount, src/fasta.c:3-53;
 * README.md:171-172): CEIL(2k/8) bytes per k-mer, nucleotide j in byte j/4 bits 2(j%4)..+1,
 * A=0 C=1 G=2 T=3, k-mers contiguous -- the `array_kmers` argument of insertKmers
 * (include/insertNode.h:26) and the 4096-byte chunks of src/file_io.c:726-730.
 *
 * Presence bitmaps: CEIL(n/8) bytes, k-mer i -> bit i%8 of byte i/8.
 *
 * All functions return BFT_GPU_OK (0) or a negative error code; bft_gpu_last_error() gives the
 * message for the calling thread.  (The reference has no error codes: ERROR() prints and exits,
 * include/useful_macros.h:33-43; the C wrapper of INTEGRATION.md keeps that behaviour.)
 * There is NO CPU fallback: without a usable HIP device every call fails with BFT_GPU_E_HIP.
 * A handle is not thread-safe (like BFT_Root, whose scratch fields make insertion and colour decoding non re-entrant,
 * include/Node.h:107-109): use one handle per thread, or serialise calls; distinct handles are independent.
 */
#ifndef BFT_GPU_H
#define BFT_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BFT_GPU_OK 0
#define BFT_GPU_E_ARG (-1)      /* bad argument (k not a multiple of 9, NULL pointer, ...) */
#define BFT_GPU_E_HIP (-2)      /* HIP runtime / device error */
#define BFT_GPU_E_LIMIT (-3)    /* a container limit of the format was exceeded */
#define BFT_GPU_E_STATE (-4)    /* call order (query before anything was built, ...) */
#define BFT_GPU_E_IO (-5)       /* file error / malformed .bft or image blob */
#define BFT_GPU_E_NOSPACE (-6)  /* caller-provided output buffer too small */

typedef struct bft_gpu bft_gpu; /* opaque: one BFT resident on one GPU (replaces BFT_Root, include/Node.h:96-122) */

const char* bft_gpu_last_error(void);
int bft_gpu_device_count(void);
const char* bft_gpu_version(void);

/* createBFT_Root(k, treshold_compression, compressed=0) (include/CC.h:214-258) / create_cdbg
 * (include/bft.h:62).  k in [9,126]; the reference requires a multiple of 9 (src/main.c:61-63) and only such
 * indexes can be written as .bft; other k (e.g. 31) are an extension verified against ground truth.  The Bloom seeds are
 * the reference's un-seeded rand() values (include/CC.h:246-248) unless r1/r2 > 0 are given. */
int bft_gpu_create(int k, int device, bft_gpu** out);
int bft_gpu_create_seeded(int k, int device, int r1, int r2, bft_gpu** out);
/* freeBFT_Root (include/CC.h:260-268) / free_cdbg (include/bft.h:63).  The handle's device blocks go to the library's cache of released
 * blocks (bounded: BFT_GPU_POOL_MAX_MB, by default an eighth of the device's memory), where the next handle's build finds them. */
void bft_gpu_free(bft_gpu* h);
/* Gives every cached device block back to the HIP runtime (for a process that has finished building and wants the memory for something else --
 * torch's allocator cannot see these blocks); returns the bytes released.  No reference counterpart: free() is the reference's only allocator. */
uint64_t bft_gpu_cache_release(void);

/* add_genomes_BFT_Root (include/CC.h:307-338): register a genome name; returns its id in *id_genome
 * (ids are 0-based and increase, as the reference's nb_genomes-1). */
int bft_gpu_add_genome(bft_gpu* h, const char* name, uint32_t* id_genome);

/* BFT_Root::filenames[id] (include/Node.h:97): NUL-terminated genome name ("genome_<id>" if none was registered). */
int bft_gpu_genome_name(bft_gpu* h, uint32_t id_genome, char* out, uint32_t cap);

/* insertKmers(root, array_kmers, nb_kmers, id_genome, size_id_genome) (include/insertNode.h:26,
 * src/insertNode.c:18-36).  The batch is converted on the GPU and appended to a device-side log;
 * the log is merged into the index by bft_gpu_build (or lazily by the first query).  No bound on the number of (k-mer, genome)
 * pairs an index holds (the reference has none): the log is merged on its own before it reaches 2^30 pairs ("flush_pairs"), a
 * larger batch is taken in pieces.  Limits that remain: < 2^31 distinct k-mers, < 2^32 genome ids in the colour-set dictionary.
 * `kmers` is a HOST pointer; the _dev variant takes a DEVICE pointer to the same layout. */
int bft_gpu_insert_kmers(bft_gpu* h, const uint8_t* kmers, uint64_t nb_kmers, uint32_t id_genome);
int bft_gpu_insert_kmers_dev(bft_gpu* h, const void* d_kmers, uint64_t nb_kmers, uint32_t id_genome);
/* The same, stream-ordered on the caller's stream (NULL = the null stream): the batch is converted by a kernel enqueued on hip_stream and the
 * call returns at once -- d_kmers follows stream semantics (it may be reused by later work on hip_stream, not before);
 * bft_gpu_build (or the first query) waits for hip_stream.  A series of insertions costs its kernels, not a host
 * round trip per call. */
int bft_gpu_insert_kmers_dev_async(bft_gpu* h, const void* d_kmers, uint64_t nb_kmers, uint32_t id_genome, void* hip_stream);

/* Bulk construction: what was inserted since the last build is sorted and de-duplicated on the GPU (root-prefix buckets, bucket
 * sorts in LDS), its colour sets interned, and that run is merged into the index (k-mers by position, colour sets by union: the index
 * itself -- sorted k-mers, colour set per k-mer, dictionary -- is the only store); then the containers are assembled level by level.
 * Replaces the per-k-mer work of insertKmer_Node / insertSP_CC / transform2CC / modify_annotations
 * (src/insertNode.c:38-423, src/CC.c:40-1474, src/retrieveAnnotation.c:232-314) with the invariants of SURVEY.md A.7. */
int bft_gpu_build(bft_gpu* h);

/* The loop of src/file_io.c:726-768 over isKmerPresent (include/presenceNode.h:57,
 * src/presenceNode.c:1823): one bit per k-mer.  Host buffers in, host bitmap out. */
int bft_gpu_query_presence(bft_gpu* h, const uint8_t* kmers, uint64_t nb_kmers, uint8_t* present_bits);
/* Same with inputs and outputs resident in HBM; runs on `hip_stream` (a hipStream_t, NULL = the
 * handle's own stream) and does not synchronise. d_present_bits: CEIL(n/64)*8 bytes.
 * Every *_dev entry point records where its work ends on a caller's stream; a later rebuild (insert + query), option
 * change or bft_gpu_free waits for that point before it releases or rewrites image arrays, so the caller need not
 * synchronise its stream first.  Every ABI call restores the calling thread's current HIP device before it returns. */
int bft_gpu_query_presence_dev(bft_gpu* h, const void* d_kmers, uint64_t nb_kmers, void* d_present_bits,
                               void* hip_stream);

/* get_annotation + get_list_id_genomes (include/bft.h:97,115; src/bft.c:363-387, 622-641;
 * src/annotation.c:2086-2250) for a batch: offsets[n+1] into ids (sorted genome ids per k-mer, none
 * for absent k-mers).  If ids_cap is too small nothing is written to ids, *ids_needed is set and
 * BFT_GPU_E_NOSPACE is returned. */
int bft_gpu_query_colors(bft_gpu* h, const uint8_t* kmers, uint64_t nb_kmers, uint8_t* present_bits,
                         uint64_t* offsets, uint32_t* ids, uint64_t ids_cap, uint64_t* ids_needed);
/* The same on a RESIDENT batch, without synchronisation (runs on hip_stream; NULL = the handle's stream): d_present_bits as in
 * bft_gpu_query_presence_dev, d_offsets = nb_kmers + 1 uint64 (offsets[nb_kmers] = the number of ids), d_ids = room for ids_cap uint32; *d_ids_needed
 * (device, may be NULL) receives the number of ids -- when it exceeds ids_cap, d_ids holds the first ids_cap ids only (never a byte beyond
 * ids_cap; offsets and bits are complete): size the buffer and call again, or pass d_ids = NULL / ids_cap = 0 first to learn the size.  (Until
 * round 6 nothing at all was written in that case; lookup, offsets and ids are ONE launch now -- k_colors_kh --, which knows the total only at its
 * end.)  The colour set of every found k-mer comes out of the line of the k-mer hash that answers presence (no row, no sorted table:
 * "compact_table" stays in force), its list's length out of the dictionary's offsets, a tile's place among all ids by a look-back over the tiles
 * before it, and the ids are streamed out wavefront by wavefront.  Scratch (8 bytes per 1024 k-mers) belongs to the handle: calls of one handle
 * on different streams are serialised by the library.  An image without the k-mer hash ("kmer_hash" 0, "walk_hash" 1) takes three launches --
 * the container walk, a scan, the fill -- and keeps the old rule (nothing written to a buffer that is too small). */
int bft_gpu_query_colors_dev(bft_gpu* h, const void* d_kmers, uint64_t nb_kmers, void* d_present_bits, void* d_offsets, void* d_ids, uint64_t ids_cap,
                             void* d_ids_needed, void* hip_stream);
/* Fixed-width variant = the CSV row of src/file_io.c:744-765 before formatting: row i is
 * CEIL(nb_genomes/8) bytes, genome g -> bit g%8 of byte g/8 (all zero for absent k-mers). */
int bft_gpu_query_color_rows(bft_gpu* h, const uint8_t* kmers, uint64_t nb_kmers, uint8_t* present_bits,
                             uint8_t* rows);

/* The loop of src/file_io.c:943-998 (-query_branching): isBranchingRight / isBranchingLeft
 * (src/branchingNode.c:16-112, :240-340) for a batch.  Bit i = k-mer i has more than one successor
 * (present k-mers kmer[1..k-1]+N) or more than one predecessor (present N+kmer[0..k-2]); the sum of the bits is
 * the CLI's "Nb branching k-mers".  counts (optional, n bytes): (successors << 4) | predecessors. */
int bft_gpu_query_branching(bft_gpu* h, const uint8_t* kmers, uint64_t nb_kmers, uint8_t* branching_bits, uint8_t* counts);
int bft_gpu_query_branching_dev(bft_gpu* h, const void* d_kmers, uint64_t nb_kmers, void* d_branching_bits, void* d_counts,
                                void* hip_stream);

/* query_sequence(bft, sequence, threshold, canonical_search) (include/bft.h:127, src/bft.c:1241-1351; CSV harness
 * src/file_io.c:1464-1574) for a batch: sequence i is seqs[seq_off[i] .. seq_off[i+1]) (ASCII, no terminator needed).
 * Every k-mer of a sequence is looked up (its reverse complement instead when canonical != 0 and it is not
 * lexicographically smaller); k-mers with a character outside ACGTU are skipped.  Row i (CEIL(nb_genomes/8) bytes)
 * has bit g set iff genome g holds at least ceil(nb_kmers(i) * threshold) of the sequence's k-mers. */
int bft_gpu_query_sequences(bft_gpu* h, const char* seqs, const uint64_t* seq_off, uint64_t nb_seqs, double threshold,
                            int canonical, uint8_t* rows);
/* The same on device-resident buffers, without synchronisation: d_seqs (total_chars ASCII bytes; any alignment, 16-byte aligned
 * blobs are read faster), d_seq_off (nb_seqs + 1 uint64 offsets into d_seqs, d_seq_off[nb_seqs] <= total_chars), d_rows
 * (nb_seqs x CEIL(nb_genomes/8) bytes).  The k-mer positions of the batch are counted on the device, so the call returns
 * as soon as its kernels are enqueued on hip_stream (NULL = the handle's stream); scratch belongs to the handle. */
int bft_gpu_query_sequences_dev(bft_gpu* h, const void* d_seqs, const void* d_seq_off, uint64_t nb_seqs, uint64_t total_chars,
                                double threshold, int canonical, void* d_rows, void* hip_stream);

/* Insertion from SEQUENCES (an extension: the reference inserts k-mers that a counter has cut out beforehand).  The layout is that of
 * bft_gpu_query_sequences: an ASCII blob and nb_seqs + 1 offsets; no k-mer spans two sequences.  Every window of k characters none of which is
 * outside ACGTU (either case) is a k-mer of genome id_genome; with canonical != 0 the inserted k-mer is the one
 * bft_gpu_query_sequences(..., canonical = 1) looks up (the reverse complement when the window is not lexicographically smaller), so an index
 * ingested canonically is queried canonically.  The effect on the handle is that of bft_gpu_insert_kmers_dev on the selected k-mers: the same log,
 * the same "flush_pairs" rule (a build in front when the log would pass it, pieces for a larger call), BFT_GPU_E_STATE under marking, BFT_GPU_E_ARG
 * for id_genome >= 2^24, for NULL with work to do and -- host form -- for offsets that decrease; nb_seqs == 0 appends nothing.
 *   min_abundance == 0  the stream path: every valid window is appended, duplicates included (the build de-duplicates); windows go from the code
 *                       stream straight into log rows, invalid ones leave no hole.
 *   min_abundance >= 1  the counting path: the valid windows' keys are sorted and a k-mer is appended once when it occurs at least min_abundance
 *                       times in THIS call (both strands together with canonical).  The whole call is one counting unit: a call with more than
 *                       "flush_pairs" k-mer positions returns BFT_GPU_E_LIMIT and inserts nothing; nothing is counted across calls.
 *   stats (may be NULL) [0] k-mer positions = sum over the sequences of max(len - k + 1, 0), [1] positions skipped for a character outside ACGTU,
 *                       [2] distinct k-mers among the valid positions (0 when min_abundance == 0: nothing is counted), [3] pairs appended to the log.
 * The host form stages the blob through device blocks of the handle; on the stream path in chunks of "ingest_chunk_chars" characters
 * (bft_gpu_set_option, default 2^26, at least 1024), a long sequence split with k - 1 characters of overlap -- the result does not depend on it. */
int bft_gpu_insert_sequences(bft_gpu* h, const char* seqs, const uint64_t* seq_off, uint64_t nb_seqs, int canonical, uint32_t min_abundance,
                             uint32_t id_genome, uint64_t stats[4]);
/* The same on device-resident buffers (d_seqs: total_chars bytes, any alignment; d_seq_off: nb_seqs + 1 uint64, the last one <= total_chars), on
 * hip_stream (NULL = the handle's stream).  The call SYNCHRONISES that stream before it returns -- the host's count of log rows must be exact, and
 * the number of appended rows is known on the device only -- once per piece of "flush_pairs" positions.  Not inside a graph capture
 * (BFT_GPU_E_ARG).  Scratch belongs to the handle. */
int bft_gpu_insert_sequences_dev(bft_gpu* h, const void* d_seqs, const void* d_seq_off, uint64_t nb_seqs, uint64_t total_chars, int canonical,
                                 uint32_t min_abundance, uint32_t id_genome, uint64_t stats[4], void* hip_stream);
/* A plain-text FASTA (">" header, sequence lines joined) or four-line FASTQ ("@" header, sequence, "+", quality) file, decided by its first
 * non-blank character, read on the host (CR LF tolerated, empty records kept as sequences of length 0, no gzip, no multi-line FASTQ;
 * BFT_GPU_E_IO for anything else, a truncated FASTQ record included) and inserted by bft_gpu_insert_sequences. */
int bft_gpu_insert_sequence_file(bft_gpu* h, const char* path, int canonical, uint32_t min_abundance, uint32_t id_genome, uint64_t stats[4]);
/* Test hook: out[0] = k-mer positions per tile of the ingest kernels' compaction (pieces of a call beyond "flush_pairs" are whole tiles), out[1] = the
 * default of "ingest_chunk_chars", out[2] = its minimum.  BFT_GPU_E_ARG for a NULL out.  No handle, no device. */
int bft_gpu_debug_ingest_plan(uint64_t out[3]);
/* Test hook: the chunks the host form of the stream path stages for these offsets with "ingest_chunk_chars" = chunk_chars (>= 1024 and 2k):
 * chunk i is the characters [out[3i], out[3i + 1]) of the blob, cut into out[3i + 2] (pieces of) sequences; a sequence that does not fit is cut and
 * its next piece starts k - 1 characters before the cut.  *n_out = the number of chunks; the first `cap` of them are written (out may be NULL). */
int bft_gpu_debug_ingest_chunks(const uint64_t* seq_off, uint64_t nb_seqs, int k, uint64_t chunk_chars, uint64_t* out, uint64_t cap, uint64_t* n_out);

/* load_BFT / read_BFT_Root (include/bft.h:176, src/write_to_disk.c:260-776): parse a reference .bft file
 * (compressed == 0; annotation modes 0/1/2 and extended-annotation bytes) and build the GPU image from its
 * k-mers and colour sets, with the file's Bloom seeds and genome names.  The file is mapped and decoded by a pool of host threads
 * (BFT_GPU_IO_THREADS); it must not be truncated by another process while the call runs (a mapped page that no longer exists is a SIGBUS, as
 * with any mmap reader).  Both calls give the host memory they used back on a detached thread after they have returned. */
int bft_gpu_load_bft(const char* path, int device, bft_gpu** out);
/* write_BFT / write_BFT_Root (include/bft.h:175, src/write_to_disk.c:21-258): serialise the image in the
 * reference's container layout so that the reference's `bft load` reads it back (invariants of SURVEY.md A.7). */
int bft_gpu_write_bft(bft_gpu* h, const char* path);

/* Device-resident variant: d_rows = n * CEIL(nb_genomes/8) bytes, d_scratch_rows_u32 = n * 4 bytes of scratch (the row
 * index of every k-mer), d_present_bits as in bft_gpu_query_presence_dev; runs on hip_stream, does not synchronise.
 * d_rows may have any alignment: the same bytes come out wherever it starts.  A 16-byte aligned d_rows with rows of 16 bytes and up takes
 * the fast kernels (16-byte stores: one launch with the lookup inside when the k-mer hash answers); any other d_rows, and narrower rows,
 * are written 4 bytes at a time. */
int bft_gpu_query_color_rows_dev(bft_gpu* h, const void* d_kmers, uint64_t nb_kmers, void* d_present_bits, void* d_rows,
                                 void* d_scratch_rows_u32, void* hip_stream);

/* Shape / size counters (the walk of src/printMemory.c:255).  out[0]=k, [1]=distinct k-mers,
 * [2]=nodes, [3]=CCs, [4]=node-UC rows, [5]=child nodes, [6]=prefixes, [7]=CCs in s=4 mode,
 * [8]=max CCs per node, [9]=(k-mer,genome) pairs, [10]=distinct colour sets, [11]=genomes,
 * [12]=image bytes in HBM, [13]=root CCs, [14]=root UC rows, [15]=pending (unbuilt) pairs. */
int bft_gpu_info(bft_gpu* h, uint64_t* out, int n_out);
/* Bytes resident in HBM per part of the handle (the walk of src/printMemory.c:255 reports the reference's bytes per container kind):
 * out[0]=sorted k-mer table tk, [1]=colour-set id per k-mer, [2]=colour-set dictionary (offsets + genome ids in 1, 2 or 4 bytes, by the largest id inserted), [3]=containers (nodes, Bloom blocks, CC headers, filter2
 * words, cluster table, prefix entries, node UCs), [4]=flat form of the big CCs, [5]=root tables, [6]=node prefix hash, [7]=k-mer hash,
 * [8]=bitmap form of the dictionary (derived by the first colour-row query), [9]=hash table (hash_v % 1504), [10]=0 (rounds 1-2 kept a sorted
 * (k-mer, genome) pair store for later insertions; the index is its own store now), [11]=pending insertion log. */
int bft_gpu_footprint(bft_gpu* h, uint64_t* out, int n_out);

/* Options.
 * "kmer_hash" (1, default): besides the containers, every stored k-mer also sits in one open-addressed table of 64-byte lines (bft_image.h,
 *   BFT_KH_*: home line from a scattering bijection of the T-form's top 32 bits, which the line then stands for -- a slot stores 2k - 32 + ~9
 *   key bits and the colour-set id, 8 k-mers per line at k = 27 / 31 and 100 genomes); presence, colour, sequence and branching queries then cost
 *   ONE cache line per k-mer instead of a container walk (src/presenceNode.c:1284-1921 costs a line per level and per suffix-group probe).  Any
 *   k; derived when an image is built, loaded or unpacked; rows (bft_gpu_query_rows) always come from the walk.  0: no table, every query walks
 *   the containers and searches the sorted table.
 * "kmer_hash_load" (55): occupancy of the table's home lines in per cent, 10..80 (55: 1.09 lines read per lookup, 15 bytes per k-mer at k = 27).
 * "walk_hash" (0, default; 1: presence / colour queries are answered by the container walk, k_query6h, whose root level looks PLAIN suffix groups up in
 *   their hashed form -- the table above: one line -- and walks the containers for the rest: child Nodes, the root's UC).
 * "query_dynamic" (1, default): the query kernels deal their blocks of k-mers out in rounds: the first by workgroup (wavefront) number, the others
 *   claimed from a counter (one pair per stream that launches them, allocated when the first image is built) -- workgroups are bound to an XCD by
 *   their number, and a static split makes the launch as slow as the XCD that reaches the table slowest; "query_chunk" (4) blocks of 256 per round
 *   of the k-mer hash kernels; batches below "query_dynamic_min" (2^16) k-mers are split statically.  The counter of a (handle, stream) pair is one
 *   64-bit word that only grows: every launch gets its own range of it and raises it to the range's start itself, so a launch that never finished
 *   (a fault, a killed process sharing nothing) cannot make a later one skip blocks -- nothing is reset by anyone (round 5; "test_stale_claims" is
 *   the test hook that leaves the counters where such a launch would).  A handle keeps counters for 32 streams; queried on more, the least recently
 *   used slot moves to the new stream once its last launch has completed, else that launch runs static and is counted (bft_gpu_build_time entry 20).
 *   0: always static.  Launches of ONE handle on ONE stream must not run concurrently (two host threads): they would share a range -- use one stream
 *   per thread, as for any stream-ordered API.  A *_dev call recorded into a HIP graph (its stream is being captured) runs static rounds: a range's
 *   start is a kernel argument, which a replay cannot move (tests/test_gpu_parity.py::test_captured_queries_replay).  The id-list, colour-row and
 *   sequence calls may be recorded too, after one direct call of the same size (which sizes the handle's scratch: nothing may allocate while a stream
 *   is captured); what they zero they zero with kernels of the library's own -- a captured hipMemsetAsync replays correctly only once on ROCm 7.0.2
 *   (test_captured_colour_queries_replay, test_captured_sequence_queries_replay; tools/probe_graph_memset.py).  A recorded call that would have to
 *   grow that scratch, or to wait for its use on another stream, returns BFT_GPU_E_ARG and records nothing; replays of a recorded call are not
 *   ordered against calls on other streams (the handle's scratch is one per query family: the caller keeps them apart).
 * The container walk (k_query*): "query_wgs_per_cu" (how it sits on a CU: 1 = one 1024-thread workgroup, 4 wavefronts per SIMD; 2 = two of them, 8 per
 *   SIMD with 64 VGPRs each; 3 = two 768-thread workgroups, 6 per SIMD with 84 VGPRs each; 0, default = by rule: 3), "query_probe" (rows per probe of the
 *   suffix-group search: 4 = adjacent 32-byte blocks, 8 = 64-byte blocks with a re-interpolated guess, 0 = by rule from the mean group size),
 *   "query_grid_mult" (grid = resident workgroups x value), "node_hash" (the prefix entries of the nodes below the root also go into one hash table keyed
 *   by (node, prefix) -- one cache line per level of a deep trie instead of four: 1, default = when the image has no k-mer hash, i.e. when the walk answers
 *   every query ("kmer_hash" 0, "walk_hash" 1); 2 = always; 0 = never), "root_quartiles" (1, default: a 1 MiB table of the quarter boundaries of every plain root
 *   group: its sorted rows are searched from a guess interpolated inside the k-mer's quarter), "root_direct" (the root level
 *   goes through tables derived from the containers: 1 = a 2 MiB table with one entry per 18-bit prefix; 2 = a 1 MiB table of row ranges for the plain
 *   suffix groups, backed by the 2 MiB table; 3, default = 2 unless most root prefixes are child Nodes; 0 = the containers), "flat_min" (CCs with at
 *   least this many prefixes also get the two-load flat form; default 3584 = the CCs in s=4 mode; 65536 = none), "tune" (1: measure residency, probe
 *   mode and root tables of the walk on the current image with a batch drawn from the index -- the only call that times anything; it synchronises;
 *   nothing is ever tuned implicitly by a build or a query).
 * Footprint: "compact_table" (1, default: the sorted k-mer table and the colour set per k-mer -- 12 bytes per k-mer -- do not stay resident once the
 *   k-mer hash holds every (k-mer, colour set): presence, colour-row, branching and sequence queries never need them; rows, extraction, a merge
 *   of new insertions, .bft files, packed images, the container walk and "tune" bring them back first -- a dump of the table + one sort, milliseconds --
 *   and they stay until the next build or until the option is set again.  No effect on a handle without a k-mer hash ("kmer_hash" 0).  0: the table stays.)
 * Build: "build_composite" (1, default: one-word keys whose genome ids arrive ascending take the root-prefix front end -- as 8-byte composites
 *   k-mer << bits | genome where that fits 63 bits, as (k-mer, id) pairs whose composite is formed inside a bucket otherwise; 0: the general key + value
 *   sort, also for the two-word keys (33 <= k <= 64) whose ascending ids would take the front end -- same image either way, a test hook), "composite_log" (1, default: where a one-word key leaves 7 bits or more for the id, k <= 28, the
 *   insertion log itself holds those composites -- 8 bytes per pending pair instead of 12, and the root-prefix split reads them as they are;
 *   an id beyond the room, ids that do not ascend or "build_composite" 0 turn the log back into k-mers + ids; 0: always k-mers + ids --
 *   same image, a test hook; only while the log is empty), "build_msd"(1, default: root-prefix buckets + bucket sorts from 2^20 pairs on; 0: one
 *   device-wide sort; 2: buckets at any size -- same image, test hooks), "test_front_rank_mode" (process-wide test hook: how a bucket ranks its digits:
 *   0, default = LDS atomics + order check + ballot fallback, 1 = ballots only, 2 = the check always fails), "test_front_wave_cap" (process-wide test hook:
 *   the largest one-word bucket that a single wavefront sorts: 0, default = 512 or 1024 by the mean bucket, 512 / 1024 = that value; same image), "sort_ballots" (process-wide: how the library's own
 *   radix sort -- csrc/bft_sort.h -- ranks the keys of a wavefront: 0, default = one LDS atomic per key once the device has shown that it serves the lanes of such an
 *   instruction in lane order, 1 = wavefront ballots, stable by construction; same image), "reserve_pairs" (room in the insertion log for this many pending (k-mer, genome)
 *   pairs, so that a series of insert calls never re-allocates it), "flush_pairs" (the log is merged into the index before it holds this many pairs:
 *   2^30 by default, 1024..2^30), "ingest_chunk_chars" (characters of the blob that the host form of bft_gpu_insert_sequences stages per chunk on its stream
 *   path: 2^26 by default, 1024..2^30; the result does not depend on it).
 * "test_no_cs_bitmaps" (test hook; 1: the bitmap form of the colour-set dictionary is not derived and one that exists is released -- what happens by itself where
 *   it would pass 4 GiB --, so the colour rows and bft_gpu_combine_* read the sorted id lists; 0: it is derived again by the next call that wants it; same answers).
 * "test_genome_matrix_road" (test hook; the road of bft_gpu_genome_matrix*: 0 = the cost model, 1 = pair updates per colour set, 2 = the matrix cores; same matrix).
 * "test_walk_grid" (test hook; 1..65535: the launches of the container walk -- presence, rows, "walk_hash", branching without the k-mer hash -- use at most this
 *   many workgroups, so that a small batch gives every wavefront several chunks; 0, the default: no cap; same answers).
 * "timing" (0/1: record HIP events around query kernels; off until this option or the first bft_gpu_kernel_time call turns it on).
 * "build_stages" (0/1: bft_gpu_build records GPU time and algorithmic bytes per stage, see bft_gpu_build_stages). */
int bft_gpu_set_option(bft_gpu* h, const char* name, int64_t value);

/* Test hook: raw device->host copy of one array of the image ("nodes", "bfT", "ccs", "f2w", "clus",
 * "child", "uck", "ucrow", "tk", "tcol", and the derived "ccx", "f18", "fent", "kh"); out may be NULL to query the size. */
int bft_gpu_debug_get_array(bft_gpu* h, const char* name, void* out, uint64_t cap_bytes, uint64_t* nbytes);
/* Test hook: how the colour-row kernels cut a batch of rows of `rowbytes` bytes into tiles and divide by the row width.  form 0: the
 * kernels that store 4 bytes at a time (any rowbytes >= 1), 1: the kernel that stores 16 bytes at a time, 2: the row kernel of the k-mer hash
 * (1 and 2: rowbytes >= 16).  out[0] = k-mers per tile, out[1], out[2] = m and l of the division: byte / rowbytes =
 * (t + ((byte - t) >> 1)) >> (l - 1) with t = the high 32 bits of byte * m, and byte itself when l == 0.  No handle, no device. */
int bft_gpu_debug_color_rows_plan(uint32_t rowbytes, int form, uint32_t out[3]);
/* Test hook: how the prefix kernels cut the C candidates of a batch (the rows of every prefix's interval, one after the other) into their
 * 2048 chunks of whole tiles of 256 candidates, one chunk per workgroup.  out[0] = the chunk size, out[1], out[2] = [begin, end) of chunk
 * `chunk` (both C for a chunk behind the last candidate).  BFT_GPU_E_ARG for a NULL out or chunk >= 2048.  No handle, no device. */
int bft_gpu_debug_prefix_plan(uint64_t C, uint32_t chunk, uint64_t out[3]);
/* Test hook: which kernels the build's front end behind the root-prefix split picks (csrc/bft_front_plan.h) for n pairs in nb buckets, the largest
 * of max_bucket pairs, the largest genome id max_gid, "test_front_wave_cap" = wave_cap (0, 512 or 1024), and who sorts a bucket of `bucket` pairs.
 * words 1 (k <= 32): out = {the wavefront kernel's largest bucket, its pairs per lane (8 / 16), the workgroup kernel's pairs per thread (6, 9, 12,
 * 16; 0: not launched), 1 when the call declines (the build then sorts device-wide), the capacity 4096, the owner of `bucket` (0 nobody, 1 the
 * wavefront kernel, 2 the workgroup kernel), 0, 0}.  words 2 (33 <= k <= 64): out = {1 when the ids fit 18 bits (the packed kernels), 1 when the
 * kernel of the buckets beyond 2048 is launched, the same beyond 4096, 1 when the call declines, the capacity 8192, the size class of `bucket`
 * (5: up to 64; 0, 1, 2: up to 512, 1024, 2048; 3, 4: up to 4096, 8192; 0xFFFFFFFF: empty), pairs per lane or thread of the class's kernel, its
 * owner (0 nobody, 1 the wavefront kernel, 2 the workgroup kernel, 3 the kernel of the tiny buckets)}.  BFT_GPU_E_ARG for a NULL out, other words,
 * another wave_cap or bucket > max_bucket.  No handle, no device. */
int bft_gpu_debug_front_plan(int words, uint64_t n, uint32_t nb, uint32_t max_bucket, uint32_t max_gid, uint32_t wave_cap, uint32_t bucket, uint32_t out[8]);
/* Test hook: what the front end launched in its last call of this process (any handle; written where each kernel is launched): out = {words, the
 * largest bucket, 1 when it declined, then words 1: the largest bucket of the wavefront kernel launched, its pairs per lane, the pairs per thread of the
 * workgroup kernel launched (0: none), 0, 0; words 2: 1 when the packed wavefront kernels were launched (ids within 18 bits), the size class of the largest
 * bucket, pairs per lane or thread of the kernel launched on that class's list (0: none), 1 when the kernel of the buckets beyond 2048 was launched, the
 * same beyond 4096}.  Reading clears it: all 0 until the front end runs again.  BFT_GPU_E_ARG for a NULL out. */
int bft_gpu_debug_front_last(uint32_t out[8]);
/* Test hook: the road the sort of h's last build took: out = {0: composites k-mer << gb | id of up to 63 bits, 1: (k-mer, id) pairs of one-word keys
 * whose ids ascend, 2: whatever is left (two-word keys, ids out of order, "build_composite" 0); gb, the bits of a genome id; the bytes of an id beside
 * the keys (0 on road 0; 1, 2 or 4 on road 1; 4 on road 2); 1 when the root-prefix split was tried}.  BFT_GPU_E_ARG for NULL or before the first build. */
int bft_gpu_debug_run_road(bft_gpu* h, uint32_t out[4]);
/* Test hook: the rules behind that road (csrc/bft_run_plan.h) for a log of `total` pairs of k-mers of length k whose genome ids ascend over the insert
 * calls (ids_ordered 1) or not, under "build_composite", "build_msd" and "composite_log" as given; max_gid: the largest id the handle has seen,
 * log_max_gid <= max_gid: the largest id of this log (they differ behind an earlier build).  out = {the four words bft_gpu_debug_run_road would report;
 * the id bits of a composite log of such a handle (0: it logs k-mers + ids); 1 when the log still holds composites at build time; the threads of a
 * capped launch grid (2048 workgroups of 256): a kernel of the run stage takes a second pass beyond that many pairs; the largest table of insert
 * calls the sort of multi-word keys reads a pair's id from (65536 entries: beyond it, from the log's id array)}.  BFT_GPU_E_ARG for a NULL out, k
 * outside 9..126, another build_msd, log_max_gid > max_gid or total 0.  No handle, no device. */
int bft_gpu_debug_run_plan(int k, int ids_ordered, int build_composite, int build_msd, int composite_log, uint32_t max_gid, uint32_t log_max_gid, uint64_t total,
                           uint32_t out[8]);

/* HIP-event timing of the query kernels launched through this handle since the last reset:
 * *ms = summed kernel time, *launches = number of launches.  Timing is off by default (no event on the launch path); the
 * first call of this function turns it on, so call it once (reset = 1) before the region to be timed. */
int bft_gpu_kernel_time(bft_gpu* h, double* ms, uint64_t* launches, int reset);
/* Same for the GPU part and the host part of bft_gpu_build (last call): ms[0]=sort+dedupe (GPU),
 * ms[1]=colour-set interning (GPU), ms[2]=container assembly (GPU), ms[3]=root-prefix buckets of the last sort whose order check failed and that were sorted a second time (expected 0: see k_bucket_sort), ms[4]=derived arrays (flat CC form, root tables, node prefix
 * hash, k-mer hash), ms[5]=resident k_query workgroups per CU in use (1, 2 or 3), ms[6..7]=time of the "tune" batch with 1 / 2 workgroups per CU (0 when not
 * tuned), ms[8]=rows per suffix-group probe in use (4 or 8), ms[9]=lines of the k-mer hash (0 = none), ms[10]=GPU time of its fill, ms[11]=largest root-prefix bucket of the last sort (0: one device-wide sort),
 * ms[12]=times the colour-set interning had to compare lists (signature collisions), ms[13]=ms this process has spent in hipMalloc so far,
 * ms[14]=root tables in use (0 / 1 / 2, see "root_direct"), ms[15..16]="tune": time with the direct table alone / with the range table, ms[17]=keys in the
 * node prefix hash, ms[18]=keys it dropped (full bucket: those lookups take the container path), ms[19]="tune": time with residency 3,
 * ms[20]=query launches that wanted a claim counter and ran static, ms[21..24]=k-mer hash: slots per line, displacement bits, largest displacement, overflow list. */
int bft_gpu_build_time(bft_gpu* h, double* ms, int n_out);
/* The last bft_gpu_build stage by stage, when bft_gpu_set_option(h, "build_stages", 1) was set before it: names = the stage names, one per
 * line (NUL-terminated; names_cap bytes), ms[i] = GPU time of stage i (HIP events on the build's stream: the time the stream spent between the end
 * of the previous stage and the end of this one, the host's waits for counts included), bytes[i] = the bytes the stage's algorithm reads + writes,
 * from its own array sizes (0: a chain of small kernels, not a streaming stage).  Names that start with '+' ran on the build's second stream beside
 * the main chain and are timed from the build's start.  *n_out = number of stages; any of names / ms / bytes may be NULL.  Replaces nothing in the
 * reference (insertKmers has no instrumentation, src/insertNode.c:18-36): this is what bench.py's `insert` block is made of. */
int bft_gpu_build_stages(bft_gpu* h, char* names, uint32_t names_cap, double* ms, double* bytes, int cap, int* n_out);

/* iterate_over_kmers-style dump (include/bft.h:166): copies every stored k-mer (packed layout,
 * ascending T-form order) and its colour-set id; either pointer may be NULL. */
int bft_gpu_extract(bft_gpu* h, uint8_t* kmers_out, uint32_t* colorset_out, uint64_t cap, uint64_t* n_out);
int bft_gpu_colorset(bft_gpu* h, uint32_t colorset, uint32_t* ids, uint32_t cap, uint32_t* n_out);

/* What the reference keeps in resultPresence for a found k-mer (include/Node.h:60-92, filled by isKmerPresent,
 * src/presenceNode.c:1823-1921), as indexes instead of host pointers: rows[i] = position of k-mer i in the stored k-mer
 * table (the order of bft_gpu_extract), colorsets[i] = id of its colour set (argument of bft_gpu_colorset);
 * 0xFFFFFFFF for an absent k-mer.  Any of present_bits / rows / colorsets may be NULL.  Host buffers. */
int bft_gpu_query_rows(bft_gpu* h, const uint8_t* kmers, uint64_t nb_kmers, uint8_t* present_bits, uint32_t* rows,
                       uint32_t* colorsets);

/* prefix_matching(bft, prefix, f, ...) (include/bft.h:135, src/bft.c:1087-1147; the reference's walk: src/presenceNode.c:1923-2448) for a
 * batch: prefix i is the first lengths[i] nucleotides (1 <= lengths[i] <= k) of the packed k-mer prefixes[i] (B = CEIL(2k/8) bytes, the layout
 * of every batch here; nucleotides from lengths[i] on are ignored, whatever they hold).  Its matches -- the stored k-mers whose first
 * lengths[i] nucleotides are the prefix's -- are entries offsets[i] .. offsets[i + 1] of the outputs, in ascending row order (the order of
 * bft_gpu_extract; the reference calls f in the DFS order of its containers instead): the packed k-mer (kmers_out, B bytes each), its row
 * in the stored k-mer table (rows_out, what bft_gpu_query_rows reports) and its colour-set id (colorsets_out, argument of bft_gpu_colorset /
 * bft_gpu_colorset_annot); any output may be NULL.  offsets: nb_prefixes + 1 entries; *needed (may be NULL) = offsets[nb_prefixes], the
 * number of matches.  When an output is given and cap (entries) is below the number of matches, nothing is written -- offsets neither --,
 * *needed is set and BFT_GPU_E_NOSPACE is returned; with every output NULL the call only counts.  A length outside [1, k] is BFT_GPU_E_ARG,
 * before any GPU work.  The matches are a range of the sorted k-mer table: under "compact_table" the table comes back first (as for
 * bft_gpu_query_rows and bft_gpu_extract) and stays until the next build.  Host buffers. */
int bft_gpu_query_prefixes(bft_gpu* h, const uint8_t* prefixes, const uint8_t* lengths, uint64_t nb_prefixes, uint64_t* offsets, uint8_t* kmers_out,
                           uint32_t* rows_out, uint32_t* colorsets_out, uint64_t cap, uint64_t* needed);
/* The same on a RESIDENT batch, without synchronisation (runs on hip_stream; NULL = the handle's stream), the capacity rule of
 * bft_gpu_query_colors_dev: d_offsets (nb_prefixes + 1 uint64) is always written in full, the outputs (device, any may be NULL) receive the
 * first cap matches only (never an entry beyond cap), *d_needed (device, may be NULL) the number of matches -- pass NULL outputs and cap 0
 * first to learn the size.  A length outside [1, k] gives that prefix no match (checking it would cost a host synchronisation).  Scratch
 * (~40 bytes per prefix) belongs to the handle: calls on different streams are serialised by the library.  Recorded into a HIP graph (its
 * stream is being captured), the call needs the sorted table resident and its scratch sized by a direct call of the same size before --
 * else it returns BFT_GPU_E_ARG: nothing synchronises or allocates inside a capture.  d_kmers_out may have any alignment (its entries are
 * B bytes each); d_rows_out, d_colorsets_out (uint32), d_offsets and d_needed (uint64) are naturally aligned. */
int bft_gpu_query_prefixes_dev(bft_gpu* h, const void* d_prefixes, const void* d_lengths, uint64_t nb_prefixes, void* d_offsets, void* d_kmers_out,
                               void* d_rows_out, void* d_colorsets_out, uint64_t cap, void* d_needed, void* hip_stream);

/* create_cdbg_from_bft_kmers(bft_kmers, nb_bft_kmers, bft, add_colors) (include/bft.h:179, src/bft.c:1353-1464) without the genome-by-genome
 * re-insertion: a new handle on src's device holding those of the nb_kmers k-mers (packed, reference layout, like every query) that src stores.
 * colors != 0: each keeps its colour set; the new handle has src's genome names and count.
 * colors == 0: one genome, named after src's genome 0; every k-mer's set is {0}.
 * Duplicates collapse.  Absent k-mers are skipped and counted in *n_absent (may be NULL).  Same k and Bloom seeds as src.
 * Options are the library defaults ("build_stages" follows src: the stages of the call are the new handle's; the new launches are counted in
 * src's bft_gpu_kernel_time).  src is built first if it has pending insertions; its answers are unchanged.  The new handle is a full handle
 * (queries, insertions, merges, bft_gpu_write_bft, bft_gpu_image_pack) and shares no device buffer with src: either may be freed first.
 * At most 2^31 - 1 k-mers per call (BFT_GPU_E_LIMIT).  Synchronous: the handle is whole when the call returns. */
int bft_gpu_subgraph(bft_gpu* src, const uint8_t* kmers, uint64_t nb_kmers, int colors, uint64_t* n_absent, bft_gpu** out);
/* The same on a RESIDENT batch: d_kmers is read in order on hip_stream (NULL = src's stream); not inside a graph capture (BFT_GPU_E_ARG). */
int bft_gpu_subgraph_dev(bft_gpu* src, const void* d_kmers, uint64_t nb_kmers, int colors, uint64_t* n_absent, bft_gpu** out,
                         void* hip_stream);

/* merging_BFT (include/merge.h:14; body commented out in src/merge.c): a new index holding every k-mer of a and of b;
 * genome g of b becomes genome id_base + g, a k-mer of both has the union of its two sets.
 *   id_base   at most a's number of genomes (bft_gpu_info [11] once a's pending insertions are built; beyond it: BFT_GPU_E_ARG).  Equal to it -- or
 *             BFT_GPU_MERGE_APPEND, which stands for it -- b's genomes are appended; one below it, b's first genome is a's last (the reference's
 *             are_genomes_ids_overlapping, include/Node.h:147-155); 0: the same genomes, their k-mers split between the two handles.  An id that
 *             would pass 2^32 is BFT_GPU_E_LIMIT.
 *   sources   same k and same device (BFT_GPU_E_ARG otherwise: bft_gpu_image_pack / bft_gpu_image_unpack move a handle to another device); the Bloom
 *             seeds may differ.  a == b is allowed (with id_base 0 the result is a's own image).  Pending insertions of either are built first; a
 *             sorted table that "compact_table" dropped comes back for the call and is dropped again before it returns.  Otherwise both are
 *             untouched, their answers unchanged, and they share no device buffer with *out: any of the three may be freed first.
 *   *out      a full handle with a's seeds: max(a's genomes, id_base + b's genomes) genomes, a's names and then b's for the ids beyond a's genomes; options at
 *             the library defaults ("build_stages" follows a: the stages of the call are the new handle's; the new launches are counted in a's
 *             bft_gpu_kernel_time); no marking.  At most 2^31 - 1 distinct k-mers in the result (BFT_GPU_E_LIMIT).
 *   "merge_place" on a: 1 (default; DESIGN 16 says on what evidence) = both sorted tables streamed and co-ranked tile by tile, 0 = every k-mer of b searched in a's table, as an
 *             insertion build places its run; the image is the same.
 * Synchronous: the handle is whole when the call returns.  Not while either source's stream is being captured (BFT_GPU_E_ARG). */
#define BFT_GPU_MERGE_APPEND 0xFFFFFFFFu
int bft_gpu_merge(bft_gpu* a, bft_gpu* b, uint32_t id_base, bft_gpu** out);

/* Simple (non-branching) paths, or unitigs: extract_simple_paths_to_disk(bft, filename) and extract_simple_core_paths_to_disk(bft, core_ratio,
 * filename) (reference snippets.h, src/snippets.c:115-603) without the disk, for a threshold t = min_shared on shared genomes (0: plain simple
 * paths; the core form passes (int)(core_ratio * nb_genomes)).
 *   degrees  the successors of a stored k-mer x are the stored x[1..k-1]+N, its predecessors the stored N+x[0..k-2] (not canonical: for the
 *            unitigs of a canonical index see bft_gpu_unitigs); they always count the whole index;
 *   nodes    stored k-mers with in-degree <= 1, out-degree <= 1 and a colour set of t genomes or more (branching k-mers are in no path);
 *   edges    u -> v when v is u's only successor, u is v's only predecessor, both are nodes, v != u and |C(u) & C(v)| >= t;
 *   paths    the maximal chains of edges, spelled as their first k-mer plus the last nucleotide of each following one (a lone node: its k-mer).
 *            A cycle is spelled from its k-mer of smallest row, for m + k - 1 nucleotides (m k-mers); a k-mer that is its own only neighbour
 *            is a lone node.  Paths come in ascending row of their first k-mer (the bft_gpu_extract order).
 * seqs: ASCII ACGT, no separators; offsets: n_paths + 1 entries, in characters (path i is seqs[offsets[i], offsets[i + 1])).
 * Host form (like bft_gpu_query_prefixes): offsets holds paths_cap + 1 entries, seqs chars_cap characters; with both NULL the call only counts;
 * when a cap is too small nothing is written, *n_paths / *n_chars are set and BFT_GPU_E_NOSPACE is returned.
 * min_shared above the number of genomes gives no path.  Pending insertions are built first; the handle's answers do not change ("compact_table":
 * the sorted table comes back, as for rows and prefixes).  Launches are counted in bft_gpu_kernel_time; with "build_stages" on, the call's steps
 * become the stages bft_gpu_build_stages reports.  At most 2^31 - 1 k-mers (BFT_GPU_E_LIMIT). */
int bft_gpu_simple_paths(bft_gpu* h, uint32_t min_shared, uint64_t* offsets, char* seqs, uint64_t paths_cap, uint64_t chars_cap, uint64_t* n_paths,
                         uint64_t* n_chars);
/* The same into device buffers on hip_stream (NULL = the handle's stream), without host synchronisation: d_counts (3 x uint64) always receives
 * {n_paths, n_chars, longest path in characters}; d_offsets (may be NULL) receives the entries j <= paths_cap of the offsets, d_seqs (may be NULL)
 * the characters below chars_cap.  Not inside a graph capture (BFT_GPU_E_ARG). */
int bft_gpu_simple_paths_dev(bft_gpu* h, uint32_t min_shared, void* d_offsets, void* d_seqs, uint64_t paths_cap, uint64_t chars_cap, void* d_counts,
                             void* hip_stream);

/* Canonical (bidirected) unitigs: the compacted de Bruijn graph of a CANONICAL index -- every stored s has s <= rc(s) by nucleotide, A < C < G < T
 * (a palindrome s == rc(s) is canonical): what bft_gpu_insert_sequences(..., canonical = 1) builds.  Rows are those of bft_gpu_extract.
 *   vertices    (s, o), o in {0, 1}, id 2 * row(s) + o; word w(s, 0) = s, w(s, 1) = rc(s); flip(s, o) = (s, 1 - o);
 *   successors  for each N of ACGT the word y = w(v)[1..k-1]+N is represented when y or rc(y) is stored; out(v) counts the represented WORDS (0..4: a
 *               palindromic y once), the successor vertex of y is (y, 0) when y is stored, else (rc(y), 1); in(v) = out(flip(v));
 *   nodes       out(v) <= 1, out(flip(v)) <= 1 and a colour set of t = min_shared genomes or more (as bft_gpu_simple_paths): both orientations of a
 *               row together;
 *   edges       u -> v when v is u's only successor, flip(u) is flip(v)'s only successor, both are nodes, row(u) != row(v) (no self-loop, no hairpin
 *               x -> rc(x)), neither k-mer is a palindrome and |C(u) & C(v)| >= t.  A palindrome counts in its neighbours' degrees and is
 *               always a path of its own;
 *   paths       the maximal chains of edges and the cycles.  Each occurs twice, as P and as its mirror (reversed, every vertex flipped); one is
 *               reported: a chain with head h and tail q iff id(h) < id(flip(q)) (a lone node: its stored k-mer), a cycle in the orientation
 *               that holds the (s, 0) of its smallest row, from that vertex, for m + k - 1 nucleotides.  A path is spelled as the word of its first
 *               vertex plus the last nucleotide of the word of each following one; paths come in ascending id of their first vertex.
 * Buffers, caps, counting with NULL outputs, BFT_GPU_E_NOSPACE, pending insertions, "compact_table", kernel time, "build_stages" and the limit of
 * 2^31 - 1 k-mers: as bft_gpu_simple_paths.  An index that is not canonical gives BFT_GPU_E_STATE, and nothing is written. */
int bft_gpu_unitigs(bft_gpu* h, uint32_t min_shared, uint64_t* offsets, char* seqs, uint64_t paths_cap, uint64_t chars_cap, uint64_t* n_paths,
                    uint64_t* n_chars);
/* The same into device buffers on hip_stream (NULL = the handle's stream), without host synchronisation: d_counts (4 x uint64) always receives
 * {n_paths, n_chars, longest path in characters, rows with s > rc(s)}; d_offsets (may be NULL) receives the entries j <= paths_cap of the offsets,
 * d_seqs (may be NULL) the characters below chars_cap.  When d_counts[3] != 0 the index is not canonical and the other outputs are unspecified
 * (nothing is written beyond the caps).  Scratch (107 bytes per k-mer) is shared with bft_gpu_simple_paths: the two are serialised on a handle.
 * Not inside a graph capture (BFT_GPU_E_ARG). */
int bft_gpu_unitigs_dev(bft_gpu* h, uint32_t min_shared, void* d_offsets, void* d_seqs, uint64_t paths_cap, uint64_t chars_cap, void* d_counts,
                        void* hip_stream);
/* The bidirected degrees of every stored k-mer, the canonical counterpart of bft_gpu_query_branching's counts: degrees[row] =
 * out(s, 0) << 4 | out(s, 1) as defined above (out(s, 1) = in(s, 0)), defined and returned on ANY index; *n_noncanonical = the rows with s > rc(s)
 * (0: the index is canonical).  degrees (may be NULL: the count alone) holds cap bytes, n_kmers are needed: BFT_GPU_E_NOSPACE, with nothing
 * written, when cap is too small.  Pending insertions are built first ("compact_table": the sorted table comes back). */
int bft_gpu_bidirected_degrees(bft_gpu* h, uint8_t* degrees, uint64_t cap, uint64_t* n_noncanonical);
/* The same into device buffers on hip_stream (NULL = the handle's stream), without host synchronisation: d_noncanonical (1 x uint64) always,
 * d_degrees (may be NULL) the bytes of the rows below cap.  Not inside a graph capture (BFT_GPU_E_ARG). */
int bft_gpu_bidirected_degrees_dev(bft_gpu* h, void* d_degrees, uint64_t cap, void* d_noncanonical, void* hip_stream);

/* The compacted coloured graph of a CANONICAL index: the unitigs completed to a cover of the index, the links between them, the k-mers of each (and,
 * through bft_gpu_unitig_colors, a colour row of each).  An extension: the reference has no counterpart.  Vertices 2 * row + o, words, flip,
 * successors, out, nodes, edges, kept paths and t = min_shared are exactly those of bft_gpu_unitigs.
 *   eligible row      |C(s)| >= t (every row at t = 0);
 *   segments          the kept paths of bft_gpu_unitigs(t), plus one segment of the single vertex (s, 0) for every eligible row that is NOT a node
 *                     (the branching k-mers), numbered in ascending id of their first vertex -- the two kinds interleave.  Every eligible row lies in
 *                     exactly one segment; the segments that are not such singles are, in order, byte for byte the output of bft_gpu_unitigs(t);
 *   oriented segment  2 * i + o.  (i, 0) reads segment i = p[0] .. p[-1] as spelled: its first vertex is p[0], its last p[-1].  (i, 1) is its reverse
 *                     complement: first vertex flip(p[-1]), last vertex flip(p[0]);
 *   links             of an oriented segment A with last vertex e: for every successor vertex w of e (over all up to four represented words; a
 *                     palindromic word is the vertex (y, 0), as in the degrees) whose row is eligible and, for t > 0, |C(e) & C(w)| >= t: A -> B, B the
 *                     oriented segment whose first vertex is w (w always is one).  The targets of one A come in ascending id; the overlap is always
 *                     k - 1 nucleotides.  A cycle has the self links S+ -> S+ and S- -> S-, a hairpin gives S+ -> S-, a homopolymer a self loop.  The
 *                     link set is mirror-symmetric (A -> B iff B ^ 1 -> A ^ 1) once the two orientations of a palindromic single-k-mer segment are
 *                     identified: links INTO a palindrome always name its + orientation (2 * i), the only asymmetry; the link lists of its two
 *                     orientations are equal;
 *   members           the vertex ids of a segment in path order: segment i occupies members[seg_off[i] - i (k - 1) .. seg_off[i + 1] - (i + 1) (k - 1)).
 * Outputs: seg_off (n_segments + 1 character offsets into seqs), seqs (ASCII ACGT), link_off (2 * n_segments + 1 entries, indexed by oriented segment),
 * links (links[link_off[A] .. link_off[A + 1]): the targets of A, oriented segments), members.  seg_off and link_off share seg_cap (segments), seqs
 * has chars_cap bytes, links links_cap and members members_cap entries.  Every output may be NULL; with all NULL the call only counts.
 * counts (6 x uint64) = {n_segments, n_chars, longest segment in characters, rows with s > rc(s), n_links, single-k-mer segments that are no unitig};
 * n_members = n_chars - n_segments (k - 1).  A cap too small for an output that is not NULL: BFT_GPU_E_NOSPACE, counts filled, nothing else written.
 * An index that is not canonical: BFT_GPU_E_STATE, counts filled, nothing else written.  The empty index: seg_off[0] = link_off[0] = 0.  Pending
 * insertions, "compact_table", kernel time, "build_stages" (stage names start "unitig graph:") and the limit of 2^31 - 1 k-mers: as bft_gpu_unitigs,
 * whose scratch the call uses (nothing is added to its 107 bytes per k-mer): the calls are serialised on a handle. */
int bft_gpu_unitig_graph(bft_gpu* h, uint32_t min_shared, uint64_t* seg_off, char* seqs, uint64_t* link_off, uint32_t* links, uint32_t* members,
                         uint64_t seg_cap, uint64_t chars_cap, uint64_t links_cap, uint64_t members_cap, uint64_t counts[6]);
/* The same into device buffers on hip_stream (NULL = the handle's stream), without host synchronisation: d_counts (6 x uint64) is always written;
 * d_seg_off receives its entries j <= seg_cap, d_link_off its entries j <= 2 * seg_cap, d_seqs, d_links and d_members what lies below their caps;
 * nothing is written beyond any cap.  When d_counts[3] != 0 the index is not canonical and the other outputs are unspecified.  Not inside a graph
 * capture (BFT_GPU_E_ARG). */
int bft_gpu_unitig_graph_dev(bft_gpu* h, uint32_t min_shared, void* d_seg_off, void* d_seqs, void* d_link_off, void* d_links, void* d_members,
                             uint64_t seg_cap, uint64_t chars_cap, uint64_t links_cap, uint64_t members_cap, void* d_counts, void* hip_stream);
/* One colour row per segment: op (BFT_GPU_SETOP_AND / _OR / _SYMDIFF, below) over the colour sets of its members -- OR: the genomes that hold a k-mer
 * of the segment, AND: those that hold all of it.  members and seg_off are what bft_gpu_unitig_graph returned (segment i: the members from
 * seg_off[i] - i (k - 1) on).  rows (n_segments rows of CEIL(nb_genomes / 8) bytes) and counts (genomes per row) are laid out as by
 * bft_gpu_combine_colorsets, which reduces them; either may be NULL.  Host form: a member >= 2 * n_kmers, offsets that grow by less than k - 1 and a
 * last segment behind n_members are BFT_GPU_E_ARG, and nothing is written.  Device form: such a member is the absent k-mer, such a segment is empty;
 * nothing is read outside the inputs.  Needs the sorted table ("compact_table": it comes back).  Not inside a graph capture (BFT_GPU_E_ARG). */
int bft_gpu_unitig_colors(bft_gpu* h, const uint32_t* members, uint64_t n_members, const uint64_t* seg_off, uint64_t n_segments, int op, uint8_t* rows,
                          uint32_t* counts);
int bft_gpu_unitig_colors_dev(bft_gpu* h, const void* d_members, uint64_t n_members, const void* d_seg_off, uint64_t n_segments, int op, void* d_rows,
                              void* d_counts, void* hip_stream);

/* Simple bubbles (variants) on the compacted coloured graph: two to four parallel segments between the same two flanks.  The call reads the arrays
 * bft_gpu_unitig_graph returned -- seg_off (n_segments + 1), seqs (seg_off[n_segments] characters), link_off (2 * n_segments + 1), links (n_links) --
 * not an index; the handle supplies k, the stream and the scratch.  An extension: the reference has no counterpart.
 *   S = n_segments; the oriented segments are 0 .. 2S - 1; seg(X) = X >> 1; out(X) is the list links[link_off[X] .. link_off[X + 1]).
 *   palindromic segment   a segment of exactly k characters whose string equals its own reverse complement (even k only; read from seqs).
 *   bubble with source A  the oriented segment A is the source of a bubble with sink Z and branches B_1 .. B_m when ALL of these hold:
 *                         - out(A) = [B_1 .. B_m] with 2 <= m <= 4: ALL of A's links, in their stored (ascending) order;
 *                         - for every j: out(B_j) = [Z], the same Z for all j, and out(B_j ^ 1) = [A ^ 1] (one way in, one way out);
 *                         - out(Z ^ 1) has exactly m entries and every entry t has t ^ 1 in {B_j} (the sink has no other way in; evaluated
 *                           literally, not through the mirror symmetry of the table);
 *                         - seg(A), seg(Z), seg(B_1) .. seg(B_m) are pairwise different (no self loop, no cycle through the source, not both
 *                           orientations of one segment as two branches);
 *                         - neither seg(A) nor seg(Z) is palindromic.  (A palindromic branch can never pass the rules above on the links of
 *                           bft_gpu_unitig_graph: links INTO a palindrome always name its + orientation P, so out(A) holds P and out(Z ^ 1) holds P
 *                           too, whose flip P ^ 1 is no branch);
 *                         - max_branch_chars > 0: every branch has at most that many characters (0: no limit).
 *   reported              every bubble exists twice, as A -> B_j -> Z and as its mirror Z ^ 1 -> B_j ^ 1 -> A ^ 1: the one with A < (Z ^ 1) is
 *                         reported.  Bubbles come in ascending A; an oriented segment is the source of at most one bubble.
 * Outputs: bubbles (may be NULL: the call only counts), records of 6 x uint32 {A, Z, B_1, B_2, B_3, B_4}, the branches in A's link order, unused slots
 * 0xFFFFFFFF; it holds cap records.  counts (4 x uint64) = {n_bubbles, branches of all bubbles, bubbles whose branches ALL have exactly 2k - 1
 * characters (k k-mers: the shape of an isolated substitution), the longest branch of a reported bubble in characters}.  cap < n_bubbles:
 * BFT_GPU_E_NOSPACE, counts filled, nothing else written.  The host form validates: link_off that decreases, link_off[2S] != n_links, a target >= 2S
 * and a seg_off step below k are BFT_GPU_E_ARG, with nothing written.  At most 2^31 - 1 segments (BFT_GPU_E_LIMIT).  Kernel time and "build_stages"
 * (stage names start "bubbles:") as everywhere.  The scratch (5 bytes per oriented segment) is the call's own: it interleaves freely with
 * bft_gpu_unitig_graph, the queries and the other families on one handle. */
int bft_gpu_unitig_bubbles(bft_gpu* h, const uint64_t* seg_off, const char* seqs, const uint64_t* link_off, const uint32_t* links, uint64_t n_segments,
                           uint64_t n_links, uint64_t max_branch_chars, uint32_t* bubbles, uint64_t cap, uint64_t counts[4]);
/* The same on device buffers on hip_stream (NULL = the handle's stream), without host synchronisation and without a count read back: d_counts
 * (4 x uint64) is always written, d_bubbles (may be NULL) receives the records below cap.  Nothing is validated up front, but no lane reads outside the
 * given arrays: a list of more than 4 entries, an offset past n_links, a target >= 2S or segment offsets outside seqs make "no bubble" for that lane.
 * Not inside a graph capture (BFT_GPU_E_ARG). */
int bft_gpu_unitig_bubbles_dev(bft_gpu* h, const void* d_seg_off, const void* d_seqs, const void* d_link_off, const void* d_links, uint64_t n_segments,
                               uint64_t n_links, uint64_t max_branch_chars, void* d_bubbles, uint64_t cap, void* d_counts, void* hip_stream);
/* The k-mer -> segment table of a compacted graph, from its members and seg_off: seg_of[row] = 2 * i + o when vertex 2 * row + o is a member of
 * segment i (the stored strand of the row reads along oriented segment (i, o)), pos[row] = its index inside segment i in path order; both
 * 0xFFFFFFFF for a row in no segment (not eligible at the graph's min_shared).  Rows are those of bft_gpu_extract.  Either output may be NULL; both
 * hold cap entries, n_kmers are needed (BFT_GPU_E_NOSPACE, nothing written).  Host form: bad members and offsets are BFT_GPU_E_ARG as for
 * bft_gpu_unitig_colors.  Device form: a member that is no vertex, or whose segment the offsets do not give, is skipped; rows below cap only.  Pending
 * insertions are built first.  Not inside a graph capture (BFT_GPU_E_ARG). */
int bft_gpu_unitig_segment_of(bft_gpu* h, const uint32_t* members, uint64_t n_members, const uint64_t* seg_off, uint64_t n_segments, uint32_t* seg_of,
                              uint32_t* pos, uint64_t cap);
int bft_gpu_unitig_segment_of_dev(bft_gpu* h, const void* d_members, uint64_t n_members, const void* d_seg_off, uint64_t n_segments, void* d_seg_of, void* d_pos,
                                  uint64_t cap, void* hip_stream);

/* Sequence threading: where does a sequence run in the compacted graph?  For a batch of sequences and a compacted graph of the handle's CANONICAL
 * index, the maximal walks over oriented segments that the sequences spell exactly.  An extension: the reference has no counterpart.
 * Inputs: k, the stored table and its rows, as bft_gpu_extract; the graph arrays of bft_gpu_unitig_graph(t): seg_off, link_off, links, S = n_segments,
 * out(X) as in the bubbles' text; seg_of and pos from bft_gpu_unitig_segment_of on that graph (n_rows entries each);
 * m_i = seg_off[i + 1] - seg_off[i] - (k - 1), the members of segment i.  The sequences are seqs / seq_off as for bft_gpu_query_sequences.
 *   position (s, p)  of sequence s, 0 <= p <= len_s - k: its window is the word w of k characters from p.  It is VALID when no character is outside
 *                    ACGTU in either case (U reads as T): the rule of bft_gpu_insert_sequences.  c is the smaller of w and rc(w), A < C < G < T.
 *                    Strand sigma = 0 when w == c, a palindromic w included; else sigma = 1.
 *   located          a valid position whose c is stored at row r with seg_of[r] != 0xFFFFFFFF.  It reads along oriented segment
 *                    X = seg_of[r] ^ sigma, i = X >> 1.  Its index is q = pos[r] when X is even, q = m_i - 1 - pos[r] when X is odd.  A position
 *                    that is invalid, absent from the index, or in no segment is NOT located; each of the three is counted separately.
 *   transition       between located neighbours (s, p) = (X, q) and (s, p + 1) = (Y, r): INSIDE when Y == X and r == q + 1; ACROSS when
 *                    q == m_X - 1, r == 0 and Y is in out(X); otherwise a BREAK.
 *   walk             a maximal run of consecutive located positions of one sequence whose transitions are all inside or across.  Its STEPS are
 *                    the oriented segments visited: the first position opens a step, every across transition opens the next one.  So a sequence
 *                    that runs twice round a cyclic unitig gives S+ S+ S+, a hairpin gives S+ S-, a homopolymer run gives one step per window.
 *                    Walks come in ascending (s, p); no walk spans two sequences.
 * Outputs (every one may be NULL; with all NULL the call counts): walks, 4 x uint64 per walk {s, p0, n_w, q0} = the sequence index, the first
 * position, the number of positions, the index of the first position in the first step; walk_off, n_walks + 1 uint64 offsets into steps; steps, uint32
 * oriented segments.  The walk covers characters [p0, p0 + n_w + k - 1) of the sequence; on its path (the steps spelled with k - 1 overlap) it covers
 * [q0, q0 + n_w + k - 1).  walks and walk_off share walks_cap (walks; walk_off holds walks_cap + 1 entries), steps has steps_cap entries.
 * counts (8 x uint64) = {n_walks, n_steps, positions, invalid positions, valid positions absent from the index, present but in no segment, breaks
 * between two located neighbours, rows with s > rc(s)}.
 * A cap too small for an output that is not NULL: BFT_GPU_E_NOSPACE, counts filled, nothing else written.  counts[7] != 0: the index is not canonical,
 * BFT_GPU_E_STATE, counts filled, nothing else written.  n_rows different from the index's k-mer count: BFT_GPU_E_ARG.  A call with 2^32 characters or
 * more, or 2^32 sequences or more: BFT_GPU_E_LIMIT; at most 2^31 - 1 segments and k-mers (BFT_GPU_E_LIMIT).  Pending insertions are built first;
 * "compact_table": the sorted table comes back.  Kernel time and "build_stages" as everywhere else; stage names start "threading:".
 * The host form validates the graph arrays as bft_gpu_unitig_bubbles and bft_gpu_unitig_segment_of do: link offsets that decrease, link_off[2S] !=
 * n_links, a target >= 2S, segment offsets that grow by less than k, and sequence offsets that decrease are BFT_GPU_E_ARG, with nothing written.  In
 * both forms a seg_of entry >= 2S, or a pos >= m_i, makes the position "in no segment", and a link list longer than 4 entries or past n_links is the
 * empty list.  The scratch (17 bytes per character of the batch, plus 4 bytes per bucket of the table) is the call's own: it interleaves freely with
 * bft_gpu_unitig_graph, the bubbles, the queries and the other families on one handle. */
int bft_gpu_thread_sequences(bft_gpu* h, const char* seqs, const uint64_t* seq_off, uint64_t nb_seqs, const uint32_t* seg_of, const uint32_t* pos,
                             uint64_t n_rows, const uint64_t* seg_off, uint64_t n_segments, const uint64_t* link_off, const uint32_t* links, uint64_t n_links,
                             uint64_t* walks, uint64_t* walk_off, uint64_t walks_cap, uint32_t* steps, uint64_t steps_cap, uint64_t counts[8]);
/* The same on device buffers on hip_stream (NULL = the handle's stream), d_seqs holding total_chars characters, without host synchronisation and
 * without a count read back: d_counts (8 x uint64) is always written; d_walks receives the walks below walks_cap, d_walk_off its entries j <=
 * min(n_walks, walks_cap), d_steps the steps below steps_cap; nothing is written beyond a cap.  When d_counts[7] != 0 the index is not canonical and
 * the other outputs are unspecified.  Nothing is validated up front, but no lane reads outside the given graph arrays and tables; the sequence
 * offsets are trusted as by bft_gpu_query_sequences_dev (they do not decrease and end at total_chars at the most).  Not inside a graph capture
 * (BFT_GPU_E_ARG). */
int bft_gpu_thread_sequences_dev(bft_gpu* h, const void* d_seqs, const void* d_seq_off, uint64_t nb_seqs, uint64_t total_chars, const void* d_seg_of,
                                 const void* d_pos, uint64_t n_rows, const void* d_seg_off, uint64_t n_segments, const void* d_link_off, const void* d_links,
                                 uint64_t n_links, void* d_walks, void* d_walk_off, uint64_t walks_cap, void* d_steps, uint64_t steps_cap, void* d_counts,
                                 void* hip_stream);

/* Connected components:get_nb_connected_component(bft, &nb, BFS | DFS) and (..., BFS_subgraph | DFS_subgraph, nb_id_genomes, ids...) (reference
 * snippets.h, src/snippets.c:605-960) without the walk, over the whole graph (nb_ids = 0) or the sub-graph of genome_ids.
 *   vertices  the stored k-mers; in a sub-graph, only the members: k-mers whose colour set holds EVERY id of genome_ids;
 *   edges     x - y when y is a stored x[1..k-1]+N or a stored N+x[0..k-2] (the 8 neighbours of get_neighbors, undirected; not canonical); in
 *             a sub-graph only between two members (the induced sub-graph: BFS_subgraph / DFS_subgraph mark non-members visited but never expand
 *             or count them);
 *   labels    components are numbered 0 .. n_components - 1 in ascending row of their smallest row (the bft_gpu_extract order); labels[row] is the
 *             component of that row, 0xFFFFFFFF for a non-member.  Labels do not depend on scheduling.
 * genome_ids (host, nb_ids of them) must be strictly increasing (BFT_GPU_E_ARG otherwise); an id at or above the number of genomes matches no k-mer.
 * counts: {n_components, n_members, largest component in k-mers}.
 * Host form: labels holds labels_cap entries (n_kmers are needed), sizes sizes_cap (n_components are needed): sizes[c] is the number of member
 * k-mers of component c; with both NULL the call only counts; when a cap is too small nothing is written, counts is set and BFT_GPU_E_NOSPACE is
 * returned.  Pending insertions are built first; the handle's answers do not change ("compact_table": the sorted table comes back, as for rows and
 * prefixes).  Launches are counted in bft_gpu_kernel_time; with "build_stages" on, the call's steps become the stages bft_gpu_build_stages
 * reports.  An empty index gives {0, 0, 0}.  At most 2^31 - 1 k-mers (BFT_GPU_E_LIMIT). */
int bft_gpu_components(bft_gpu* h, const uint32_t* genome_ids, uint32_t nb_ids, uint32_t* labels, uint64_t labels_cap, uint64_t* sizes, uint64_t sizes_cap,
                       uint64_t* counts);
/* The same into device buffers on hip_stream (NULL = the handle's stream), without host synchronisation (genome_ids stays a host array: the ids
 * travel as kernel arguments): d_counts (3 x uint64) always receives the counts; d_labels (may be NULL) n_kmers labels, d_sizes (may be NULL) the
 * sizes of the components below sizes_cap.  The number of launches does not depend on the data.  Not inside a graph capture (BFT_GPU_E_ARG). */
int bft_gpu_components_dev(bft_gpu* h, const uint32_t* genome_ids, uint32_t nb_ids, void* d_labels, void* d_sizes, uint64_t sizes_cap, void* d_counts,
                           void* hip_stream);

/* The pan-genome k-mer classes: extract_core_kmers / extract_dispensable_kmers / extract_singleton_kmers through extract_pangenome_kmers_to_disk
 * (reference snippets.h, src/snippets.c:10-106) without one annotation fetch per k-mer.  The genome count of a stored k-mer is the size of its colour
 * set; bft_gpu_kmers_by_count selects the k-mers carried by min_count .. max_count genomes (core: both = the number of genomes; dispensable: 0 ..
 * genomes - 1; singleton: 1 .. 1) and writes them in ascending row order (the bft_gpu_extract order, hence that of iterate_over_kmers here; the
 * reference visits its containers in their own order: same set).  Outputs, each may be NULL: kmers_out, packed in the reference's layout (B =
 * CEIL(2k/8) bytes each, as bft_gpu_extract); ascii_out, k + 1 bytes each: the k nucleotides and the terminating NUL (what the reference's callbacks
 * fwrite, src/snippets.c:21); rows_out, the row of each in the stored k-mer table.  cap: entries of room in every output given.
 * Host form: with every output NULL the call only counts; when cap < *n_out nothing is written and BFT_GPU_E_NOSPACE is returned, *n_out set.
 * min_count > max_count, or a range no k-mer falls in, selects nothing (BFT_GPU_OK); max_count may exceed the number of genomes.  The number of
 * genomes counts every genome added, one that received no k-mer included (then no k-mer is core), as graph->nb_genomes does in the reference.
 * Pending insertions are built first; the handle's answers do not change ("compact_table": the sorted table comes back, as for rows, prefixes and
 * simple paths).  Launches are counted in bft_gpu_kernel_time; with "build_stages" on, the call's steps become the stages bft_gpu_build_stages reports.
 * At most 2^31 - 1 k-mers (BFT_GPU_E_LIMIT). */
int bft_gpu_kmers_by_count(bft_gpu* h, uint32_t min_count, uint32_t max_count, uint8_t* kmers_out, char* ascii_out, uint32_t* rows_out, uint64_t cap,
                           uint64_t* n_out);
/* The same into device buffers on hip_stream (NULL = the handle's stream), without host synchronisation: d_count (uint64, required) always receives the
 * number of selected k-mers; the outputs (any may be NULL) receive the first cap of them and nothing beyond -- pass NULL outputs and cap 0 first to
 * learn the size.  Scratch (~4 bytes per stored k-mer) belongs to the handle and is shared with no other query family.  Not inside a graph capture
 * (BFT_GPU_E_ARG). */
int bft_gpu_kmers_by_count_dev(bft_gpu* h, uint32_t min_count, uint32_t max_count, void* d_kmers_out, void* d_ascii_out, void* d_rows_out, uint64_t cap,
                               void* d_count, void* hip_stream);
/* The whole index in one call: spectrum[c], c = 0 .. nb_genomes, the stored k-mers carried by exactly c genomes (spectrum[0] is 0 on every index this
 * library builds: the entry is kept so that the index is the count; the entries sum to the number of stored k-mers); genome_total[g] the k-mers whose
 * colour set holds genome g; genome_private[g] those whose colour set is {g} alone (they sum to spectrum[1]).  spectrum has nb_genomes + 1 entries, the
 * other two nb_genomes; any may be NULL.  cap = entries of room in spectrum (the other two need cap - 1): cap < nb_genomes + 1 with an output given is
 * BFT_GPU_E_NOSPACE.  An empty index gives zeros.  Work is one pass over the colour set of every row plus one over the dictionary. */
int bft_gpu_pangenome_stats(bft_gpu* h, uint64_t* spectrum, uint64_t* genome_total, uint64_t* genome_private, uint32_t cap);
/* The same into device buffers (uint64) on hip_stream (NULL = the handle's stream), without host synchronisation.  Not inside a graph capture. */
int bft_gpu_pangenome_stats_dev(bft_gpu* h, void* d_spectrum, void* d_genome_total, void* d_genome_private, uint32_t cap, void* hip_stream);

/* The genome-by-genome shared k-mer matrix (an extension like <bft/ingest.h>: the reference has no counterpart): what Jaccard similarity, containment,
 * Mash distance and a guide tree are computed from.  G = the number of genomes as bft_gpu_pangenome_stats counts them (a genome without k-mers
 * counts, ids inserted without a name count).  shared is a full, symmetric, row-major G x G matrix of uint64: shared[i * G + j] = the stored k-mers
 * whose colour set holds both i and j; the diagonal is genome_total of bft_gpu_pangenome_stats.  The results are exact: integer arithmetic only,
 * independent of scheduling; no float is accumulated anywhere.  The work is one pass over the colour set of every row plus passes over the
 * colour-set dictionary (M = B^T diag(usage) B), by one of two roads that agree bit for bit: pair updates per colour set, or 7-bit digits of the usage
 * on the i8 matrix cores -- chosen on the device by a cost model, without synchronising ("test_genome_matrix_road" 1 / 2, a test hook of
 * bft_gpu_set_option, forces the sparse / the dense one; 0 = the model).
 * bft_gpu_genome_matrix restricts the matrix to the k-mers whose colour set holds min_count .. max_count genomes: 0, UINT32_MAX is everything; 0, G - 1
 * the accessory genome (the core no longer drowns the signal); min_count > max_count gives all zeros.  cap = entries of room in shared; G * G are
 * needed.  shared == NULL only sets *nb_genomes; a cap too small writes nothing and returns BFT_GPU_E_NOSPACE with *nb_genomes set.  The empty index
 * and G = 0 succeed.  Pending insertions are built first ("compact_table": the sorted table comes back).  At most 2^31 - 1 k-mers and
 * BFT_GPU_GENOME_MATRIX_MAX_GENOMES genomes (2 GiB of matrix): BFT_GPU_E_LIMIT beyond.  Launches are counted in bft_gpu_kernel_time; with
 * "build_stages" on, the call's passes become the stages bft_gpu_build_stages reports. */
#define BFT_GPU_GENOME_MATRIX_MAX_GENOMES 16384u
int bft_gpu_genome_matrix(bft_gpu* h, uint32_t min_count, uint32_t max_count, uint64_t* shared, uint64_t cap, uint32_t* nb_genomes);
/* The same into a device buffer (G * G uint64) on hip_stream (NULL = the handle's stream), without host synchronisation.  cap < G * G is
 * BFT_GPU_E_NOSPACE (G is known on the host).  Scratch (about 13 bytes per colour set, and for the dense road G / 8 bytes per colour set) belongs to
 * the handle and is shared with no other query family.  Not inside a graph capture (BFT_GPU_E_ARG). */
int bft_gpu_genome_matrix_dev(bft_gpu* h, uint32_t min_count, uint32_t max_count, void* d_shared, uint64_t cap, void* hip_stream);
/* The same matrix over a caller's batch of n colour-set ids, each id weighted by how often it occurs in the batch: the colorsets of
 * bft_gpu_query_rows, the colorsets_out of bft_gpu_query_prefixes ("which genomes resemble each other over the k-mers under this prefix") or those of
 * bft_gpu_extract (the whole-index matrix).  0xFFFFFFFF (absent) is skipped.  Any other id at or past the number of colour sets is BFT_GPU_E_ARG in
 * the host form and is skipped in the _dev form.  n >= 2^31 is BFT_GPU_E_LIMIT.  The sorted table is not needed. */
int bft_gpu_genome_matrix_colorsets(bft_gpu* h, const uint32_t* colorsets, uint64_t n, uint64_t* shared, uint64_t cap, uint32_t* nb_genomes);
int bft_gpu_genome_matrix_colorsets_dev(bft_gpu* h, const void* d_colorsets, uint64_t n, void* d_shared, uint64_t cap, void* hip_stream);

/* Colour-set algebra over groups of k-mers: intersection_annotations / union_annotations / sym_difference_annotations (reference include/bft.h:112-114,
 * src/bft.c:421-613) for a batch of groups, reduced on the GPU: one row per GROUP crosses to the caller, not one per k-mer (the route through
 * bft_gpu_query_color_rows and a host loop).  Group g is the k-mers group_off[g] .. group_off[g + 1] of the batch (packed, the layout of every batch
 * here): nb_groups + 1 offsets, as seq_off of bft_gpu_query_sequences; groups may leave k-mers between them uncovered, and those take part in no result.
 *   op       BFT_GPU_SETOP_AND: the genomes that hold every member; _OR: those that hold at least one; _SYMDIFF: OR minus AND -- what src/bft.c:592-601
 *            computes; a group of one member gives that member's set.
 *   absent   skip_absent == 0: a k-mer the index does not store is the empty set (an AND over a group with an absent member is empty);
 *            skip_absent != 0: it is left out of the group.
 *   rows     nb_groups x CEIL(nb_genomes/8) bytes in the bit layout of bft_gpu_query_color_rows; the bits at and past nb_genomes are zero.
 *   counts   counts[g] = the number of genomes in row g.     found   found[g] = the members of group g that the index stores.
 *            Each of the three may be NULL; counts alone is a valid call, and then no row is written anywhere.
 *   empty    a group without members gives a zero row and count 0 under every op; so does a group without a found member under skip_absent.
 *   errors   host forms: an unknown op, offsets that decrease and group_off[nb_groups] > nb_kmers are BFT_GPU_E_ARG, and nothing is written.  The
 *            device forms cannot look at the offsets: a group whose end lies before its start or past nb_kmers is EMPTY there; nothing is ever read
 *            outside the batch or written outside the three outputs.  nb_genomes == 0: nothing is written to rows, counts and found are zero.
 * The colour set of a k-mer comes out of the line of the k-mer hash that answers presence ("compact_table" stays in force: the sorted table is not brought
 * back); an image without the k-mer hash ("kmer_hash" 0) and one with "walk_hash" 1 give the same answers through the container walk.  The dictionary is
 * read in its bitmap form (derived by the first colour-row query or the first call here) or, where that would pass 4 GiB, as its sorted id lists
 * ("test_no_cs_bitmaps" 1, a test hook of bft_gpu_set_option, forces the second; same bytes).  A dictionary row is fetched once per run of equal colour
 * sets, not per member; groups of any size are served (pairs share a wavefront, a read takes one, a group of millions is split over workgroups and met
 * in memory by 32-bit atomics).  Pending insertions are built first.  Launches are counted in bft_gpu_kernel_time; with "build_stages" on, the steps are
 * the stages bft_gpu_build_stages reports.  Scratch (4 bytes per k-mer, ~2 rows per group) belongs to the handle and is shared with no other query
 * family: calls on different streams are serialised by the library, and interleave with every other call on the handle.
 * Host forms stage the whole batch through device blocks of the call's own and synchronise.  The *_dev forms take device buffers (d_group_off: uint64,
 * d_counts / d_found: uint32, d_rows at any alignment), enqueue on hip_stream (NULL = the handle's stream) and do not synchronise.  Not inside a graph
 * capture (BFT_GPU_E_ARG). */
#define BFT_GPU_SETOP_AND     0   /* genomes that hold every member of the group */
#define BFT_GPU_SETOP_OR      1   /* genomes that hold at least one              */
#define BFT_GPU_SETOP_SYMDIFF 2   /* OR minus AND: what src/bft.c:592-601 computes; a group of one member gives that member's set */
int bft_gpu_combine_colors(bft_gpu* h, const uint8_t* kmers, uint64_t nb_kmers, const uint64_t* group_off, uint64_t nb_groups, int op, int skip_absent,
                           uint8_t* rows, uint32_t* counts, uint32_t* found);
int bft_gpu_combine_colors_dev(bft_gpu* h, const void* d_kmers, uint64_t nb_kmers, const void* d_group_off, uint64_t nb_groups, int op, int skip_absent,
                               void* d_rows, void* d_counts, void* d_found, void* hip_stream);
/* The same over colour-set ids (what bft_gpu_query_rows, bft_gpu_extract and bft_gpu_query_prefixes hand out) instead of k-mers: nb ids, grouped by
 * group_off.  An id equal to 0xFFFFFFFF (what bft_gpu_query_rows writes for an absent k-mer) plays the absent k-mer's role with skip_absent == 0; any
 * other id outside the dictionary is BFT_GPU_E_ARG in the host form and the empty set in the device form.  No lookup: the ids are the members. */
int bft_gpu_combine_colorsets(bft_gpu* h, const uint32_t* colorsets, uint64_t nb, const uint64_t* group_off, uint64_t nb_groups, int op, uint8_t* rows,
                              uint32_t* counts);
int bft_gpu_combine_colorsets_dev(bft_gpu* h, const void* d_colorsets, uint64_t nb, const void* d_group_off, uint64_t nb_groups, int op, void* d_rows,
                                  void* d_counts, void* hip_stream);
/* Test hook: out[0] = the largest group that takes a lane per (group, word), out[1] = the largest group one wavefront reduces (larger ones are split),
 * out[2] = members per step of a split group, out[3] = wavefronts of the split kernel's grid, out[4] = lanes of the grid that finishes the split groups,
 * out[5] = lanes of the capped grid of every other kernel.  BFT_GPU_E_ARG for a NULL out.  No handle, no device. */
int bft_gpu_debug_setops_plan(uint64_t out[6]);

/* Vertex marking: set_marking / unset_marking / set_flag_kmer / get_flag_kmer (reference include/bft.h:143-146, src/bft.c:686-765) for batches, and
 * what the reference's traversals do with the marks (BFS / DFS / BFS_subgraph / DFS_subgraph, src/snippets.c:605-812) as ONE call, bft_gpu_marks_reach.
 * A flag is 0, 1, 2 or 3 (anything above is BFT_GPU_E_ARG); every stored k-mer has one, 0 after bft_gpu_marks_begin.  The flags are an array in HBM that
 * belongs to the handle: two bits per stored k-mer, indexed by its row in the stored k-mer table (the bft_gpu_extract order, what bft_gpu_query_rows
 * reports); as bytes, 4 rows per byte, row r in bits 2 (r % 4) .. + 1 of byte r / 4 -- CEIL(n_kmers / 4) bytes, the bits behind the last row 0.
 * bft_gpu_marks_begin (set_marking): pending insertions are built, the sorted table comes back ("compact_table") and the zeroed flags are allocated; on a
 *   handle that is already marking it does nothing and the flags stay (src/bft.c:694).  Until bft_gpu_marks_end (unset_marking: the flags are released;
 *   a no-op on a handle that is not marking), bft_gpu_insert_kmers*, bft_gpu_add_genome and bft_gpu_build return BFT_GPU_E_STATE -- "no insertion can
 *   happen before unlocking" (src/bft.c:686); queries and the analysis calls are unaffected.  bft_gpu_free releases the marks with the handle.
 * Every other call below returns BFT_GPU_E_STATE on a handle that is not marking.  The marks are not carried by bft_gpu_image_pack, .bft files,
 * bft_gpu_subgraph or a device group: they belong to this handle alone.
 * Batches are packed k-mers (the layout of every batch here); their rows come from the lookup of bft_gpu_query_rows.  Absent k-mers are ignored and
 * counted in *n_absent (may be NULL).  Launches are counted in bft_gpu_kernel_time.
 * The *_dev forms take device buffers and run on hip_stream (NULL = the handle's stream) without host synchronisation; their d_n_absent (uint64, device,
 * may be NULL) is always written when given.  Scratch (4 bytes per k-mer of the batch) belongs to the handle: calls on different streams are serialised
 * by the library.  Not inside a graph capture (BFT_GPU_E_ARG). */
int bft_gpu_marks_begin(bft_gpu* h);
int bft_gpu_marks_end(bft_gpu* h);
/* set_flag_kmer (src/bft.c:721-741) for a batch: flags == NULL gives every k-mer `flag`; otherwise k-mer i gets flags[i] (one byte each, 0..3; the
 * resident form cannot look at them without a synchronisation and keeps their two low bits) and `flag` is not read.  A k-mer that appears several
 * times with different flags ends with one of them, never a mixture of their bits. */
int bft_gpu_marks_set(bft_gpu* h, const uint8_t* kmers, uint64_t nb_kmers, const uint8_t* flags, uint8_t flag, uint64_t* n_absent);
int bft_gpu_marks_set_dev(bft_gpu* h, const void* d_kmers, uint64_t nb_kmers, const void* d_flags, uint8_t flag, void* d_n_absent, void* hip_stream);
/* get_flag_kmer (src/bft.c:747-765) for a batch: flags_out[i] = 0..3, or 0xFF for an absent k-mer (the reference exits there). */
int bft_gpu_marks_get(bft_gpu* h, const uint8_t* kmers, uint64_t nb_kmers, uint8_t* flags_out, uint64_t* n_absent);
int bft_gpu_marks_get_dev(bft_gpu* h, const void* d_kmers, uint64_t nb_kmers, void* d_flags_out, void* d_n_absent, void* hip_stream);
/* The step of a frontier of the caller's own (the `get_flag_kmer(...) == V_NOT_VISITED` test followed by set_flag_kmer of src/snippets.c:628-630, as one
 * atomic operation): k-mer i moves to `flag` only if it holds `expect`; won_out[i] = 1 for the ONE entry of the batch that moved it, 0 for every
 * other entry (a repeat of the k-mer, a k-mer that held something else, an absent k-mer).  flag == expect is BFT_GPU_E_ARG. */
int bft_gpu_marks_test_and_set(bft_gpu* h, const uint8_t* kmers, uint64_t nb_kmers, uint8_t expect, uint8_t flag, uint8_t* won_out, uint64_t* n_absent);
int bft_gpu_marks_test_and_set_dev(bft_gpu* h, const void* d_kmers, uint64_t nb_kmers, uint8_t expect, uint8_t flag, void* d_won_out, void* d_n_absent,
                                   void* hip_stream);
/* Every stored k-mer gets `flag` (0: what delete + create_marking would leave, src/bft.c:696,710); the host form synchronises. */
int bft_gpu_marks_fill(bft_gpu* h, uint8_t flag);
int bft_gpu_marks_fill_dev(bft_gpu* h, uint8_t flag, void* hip_stream);
/* counts[f] (4 x uint64) = stored k-mers that hold flag f. */
int bft_gpu_marks_counts(bft_gpu* h, uint64_t* counts);
int bft_gpu_marks_counts_dev(bft_gpu* h, void* d_counts, void* hip_stream);
/* The k-mers whose flag is in `mask` (bit f set: flag f is wanted; 0 .. 15), in ascending row order, with the outputs, the cap and the
 * BFT_GPU_E_NOSPACE rule of bft_gpu_kmers_by_count / _dev: packed k-mers, ASCII k-mers of k + 1 bytes with the NUL, rows; any may be NULL. */
int bft_gpu_marks_select(bft_gpu* h, uint32_t mask, uint8_t* kmers_out, char* ascii_out, uint32_t* rows_out, uint64_t cap, uint64_t* n_out);
int bft_gpu_marks_select_dev(bft_gpu* h, uint32_t mask, void* d_kmers_out, void* d_ascii_out, void* d_rows_out, uint64_t cap, void* d_count, void* hip_stream);
/* Reachability restricted by flag.  A row is ELIGIBLE when its flag is `through` and its colour set holds every id of genome_ids (host array, strictly
 * increasing as for bft_gpu_components; nb_ids = 0: every colour set qualifies).  Every eligible row connected to an eligible seed through eligible rows
 * -- the edges of bft_gpu_components -- gets the flag `to` (`to` == `through` is BFT_GPU_E_ARG).  With through = 0, to = 1 and no ids this is what
 * calling BFS or DFS (src/snippets.c:605-656, 743-762) on each seed in order leaves behind.  boundary != 0 reproduces the marks of BFS_subgraph /
 * DFS_subgraph (:667-735, :773-812), which mark every unvisited k-mer they LOOK at: a seed that holds `through` without being eligible, and every
 * row that holds `through`, is not eligible and is a neighbour of a row this call painted, get `to` as well.
 * seeds: n_seeds packed k-mers.  seed_new[i] (may be NULL) = 1 when seed i is eligible and is the lowest-index seed of its component, else 0: what the
 * reference's traversal would return for the seeds taken in order.  counts (3 x uint64, may be NULL in the host form): {eligible rows painted, boundary
 * rows painted, seeds absent}.  The components are found by the union-find of bft_gpu_components, never level by level: the number of launches depends
 * on the arguments alone.  The flattened forest stays on the handle, keyed by (through, genome_ids): painting removes whole components of eligible rows,
 * so the next reach with the same key starts from it; any set, test-and-set, fill or write of the flags, or a reach with another key, drops it.  That
 * is what makes a traversal of the whole graph, one reach per component, cost one union-find.  At most 2^31 - 1 k-mers (BFT_GPU_E_LIMIT). */
int bft_gpu_marks_reach(bft_gpu* h, const uint8_t* seeds, uint64_t n_seeds, const uint32_t* genome_ids, uint32_t nb_ids, uint8_t through, uint8_t to,
                        int boundary, uint8_t* seed_new, uint64_t* counts);
int bft_gpu_marks_reach_dev(bft_gpu* h, const void* d_seeds, uint64_t n_seeds, const uint32_t* genome_ids, uint32_t nb_ids, uint8_t through, uint8_t to,
                            int boundary, void* d_seed_new, void* d_counts, void* hip_stream);
/* The whole flag array out and in, in the byte layout above.  read: *n_bytes (may be NULL) = CEIL(n_kmers / 4); bytes_out may be NULL to learn it,
 * cap below it is BFT_GPU_E_NOSPACE.  write: n_bytes must be exactly that, and the bits behind the last row 0 (BFT_GPU_E_ARG otherwise). */
int bft_gpu_marks_read(bft_gpu* h, uint8_t* bytes_out, uint64_t cap, uint64_t* n_bytes);
int bft_gpu_marks_write(bft_gpu* h, const uint8_t* bytes_in, uint64_t n_bytes);

/* A colour set as the reference's annotation bytes -- BFT_annotation::annot as get_annotation returns it
 * (include/bft.h:97, src/bft.c:363-387): mode 0 (bitmap, genome g <-> bit g+2), 1 (ranges) or 2 (id list), chosen the way the
 * reference chooses it: compute_best_mode re-decides at every insertion of a genome id and keeps the current mode on a size tie
 * (src/annotation.c:621-653), so the bytes depend on the order the ids arrived in -- ascending -- and the rule is replayed over the
 * sorted id list (e.g. {6,7} stays the id list 1a 1e it started as, although a bitmap would be no longer), the run-end size estimate of the
 * bitmap mode included (:515-523: the end of a run is priced with the byte count of the id one past it).  disabled_flags (:622) is never set
 * anywhere in the reference: nothing to replay.  The same bytes go into the .bft files bft_gpu_write_bft writes.  annot may be NULL to
 * query the size. */
int bft_gpu_colorset_annot(bft_gpu* h, uint32_t colorset, uint8_t* annot, uint32_t cap, uint32_t* n_out);

/* Replication of a built index on another GPU (the query path shards over GPUs with the trie image
 * replicated in each GPU's HBM; the reference has one BFT_Root per process, include/Node.h:96-122).
 * bft_gpu_image_size: bytes of the self-describing device blob; bft_gpu_image_pack: writes it at d_blob (device
 * memory of the handle's GPU, cap >= size) on hip_stream (0 = the handle's stream) and synchronises that stream;
 * bft_gpu_image_unpack: new handle on `device` from a blob resident in that GPU's memory (e.g. the receive buffer
 * of one RCCL broadcast) -- same answers, same bft_gpu_write_bft bytes, and insertion can continue on it. */
int bft_gpu_image_size(bft_gpu* h, uint64_t* nbytes);
int bft_gpu_image_pack(bft_gpu* h, void* d_blob, uint64_t cap, void* hip_stream);
int bft_gpu_image_unpack(const void* d_blob, uint64_t nbytes, int device, bft_gpu** out);

/* One index on several GPUs of ONE process (the loops of src/file_io.c:651-895 and :897-1020 can only ever use one
 * BFT_Root).  bft_gpu_group_create: `src` (a handle on GPU src_device; built if need be) is replicated into the HBM of every device of
 * devices[0..n_devices) -- image blob packed on the source GPU, one peer copy per replica, unpacked there; the first slot naming
 * src_device is served by src itself, further slots (the same device may appear twice) get copies.  The group owns its replicas, not src.
 * The *_query_* calls cut a host batch into contiguous slices whose starts are multiples of 64 k-mers (bft_gpu_group_shard gives slice i
 * of `parts`: the same rule bloomfiltertrie_amd/dist.py applies across processes) and return when every slot has answered its slice into the
 * caller's buffers -- same layouts as the single-GPU calls.  Every slot has a host thread of its own for as long as the group lives, with a
 * stream on its device and two slots of pinned staging memory: a slice moves in chunks (at most 2^22 k-mers / ~64 MiB), chunk c + 1 copied into
 * pinned memory while the GPU answers chunk c through the *_dev entry points -- the caller's arrays may be pageable, the copies never are.
 * Insertion stays single-GPU: insert into src, then create the group again. */
typedef struct bft_gpu_group bft_gpu_group;
int bft_gpu_group_shard(uint64_t n, int parts, int i, uint64_t* begin, uint64_t* end);
int bft_gpu_group_create(bft_gpu* src, int src_device, const int* devices, int n_devices, bft_gpu_group** out);
void bft_gpu_group_free(bft_gpu_group* g);
int bft_gpu_group_size(bft_gpu_group* g);
int bft_gpu_group_query_presence(bft_gpu_group* g, const uint8_t* kmers, uint64_t nb_kmers, uint8_t* present_bits);
int bft_gpu_group_query_color_rows(bft_gpu_group* g, const uint8_t* kmers, uint64_t nb_kmers, uint8_t* present_bits, uint8_t* rows);
int bft_gpu_group_query_branching(bft_gpu_group* g, const uint8_t* kmers, uint64_t nb_kmers, uint8_t* branching_bits, uint8_t* counts);
/* The same on DEVICE-RESIDENT batches: arrays of bft_gpu_group_size(g) entries, entry i = the batch of slot i -- d_kmers[i] (n[i] packed k-mers)
 * and the outputs lie in the memory of GPU bft_gpu_group_member_device(g, i); hip_streams[i] (or NULL: the slot's own stream; hip_streams itself
 * may be NULL) orders the work.  Like the single-GPU *_dev calls these only enqueue: no host thread, no synchronisation, the slots run side by
 * side; the caller synchronises its streams (a caller that owns one shard per GPU -- the partition of bft_gpu_group_shard or any other -- keeps
 * every buffer where it is produced and consumed: the resident rate of every GPU, not the host link's).  n[i] == 0 skips slot i. */
int bft_gpu_group_member_device(bft_gpu_group* g, int i);
/* bft_gpu_footprint / bft_gpu_info of slot i's handle (the replicas belong to the group: this is how their residency is inspected) */
int bft_gpu_group_member_footprint(bft_gpu_group* g, int i, uint64_t* out, int n_out);
int bft_gpu_group_member_info(bft_gpu_group* g, int i, uint64_t* out, int n_out);
int bft_gpu_group_query_presence_dev(bft_gpu_group* g, const void* const* d_kmers, const uint64_t* n, void* const* d_present_bits, void* const* hip_streams);
int bft_gpu_group_query_color_rows_dev(bft_gpu_group* g, const void* const* d_kmers, const uint64_t* n, void* const* d_present_bits, void* const* d_rows,
                                       void* const* d_scratch_rows_u32, void* const* hip_streams);
int bft_gpu_group_query_branching_dev(bft_gpu_group* g, const void* const* d_kmers, const uint64_t* n, void* const* d_branching_bits, void* const* d_counts,
                                      void* const* hip_streams);

#ifdef __cplusplus
}
#endif
#endif
