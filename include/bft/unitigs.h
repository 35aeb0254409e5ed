/*
 * <bft/unitigs.h> -- the canonical (bidirected) unitigs of an index.  An EXTENSION: GuillaumeHolley/BloomFilterTrie has no counterpart -- its
 * extract_simple_paths_to_disk (include/snippets.h, served by <bft/snippets.h>) follows the stored k-mers on one strand only, which cuts the paths
 * of a canonical index wherever the stored strand flips.  Served by bft_gpu_unitigs (include/bft_gpu.h), which defines the paths: maximal
 * non-branching chains and cycles over the k-mers AND their reverse complements, each reported once, on one strand.
 */
#ifndef BFT_GPU_COMPAT_UNITIGS_H
#define BFT_GPU_COMPAT_UNITIGS_H

#include "bft.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The unitigs of a canonical index -- every stored k-mer is the lexicographically smaller of itself and its reverse complement, as
 * insert_genomes_from_sequence_files(..., canonical = 1, ...) of <bft/ingest.h> stores them -- written to filename_output one per line, as
 * extract_simple_paths_to_disk writes its paths; the longest is reported on stdout.  min_shared = t > 0: only k-mers of t genomes or more,
 * joined where they share t or more (0 or less: every k-mer).  Errors (the file cannot be created, the index is not canonical) print a message
 * on stderr and exit(EXIT_FAILURE), as everywhere in <bft/bft.h>. */
void extract_unitigs_to_disk(BFT* graph, int min_shared, char* filename_output);

#ifdef __cplusplus
}
#endif

#endif
