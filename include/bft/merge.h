/*
 * <bft/merge.h> -- merging two Bloom Filter Tries of GuillaumeHolley/BloomFilterTrie (reference include/merge.h:14; the body of merging_BFT in
 * src/merge.c is commented out upstream, its semantics are those of are_genomes_ids_overlapping, include/Node.h:147-155, and of the insertion it
 * performs: the second graph's genomes come after the first graph's, one earlier when the last name of the first equals the first name of the
 * second, and a k-mer of both graphs carries the union of its two colour sets).  Served by one call of bft_gpu_merge (include/bft_gpu.h): the two
 * sorted k-mer tables are merged on the GPU and the colour sets united there, instead of one insertion per k-mer of the second graph.
 */
#ifndef BFT_GPU_COMPAT_MERGE_H
#define BFT_GPU_COMPAT_MERGE_H

#include "bft.h"

#ifdef __cplusplus
extern "C" {
#endif

/* include/merge.h:14.  prefix_bft1 and prefix_bft2 name two files written by write_BFT; they are loaded as load_BFT loads them, merged, and the
 * result is written to output_prefix as write_BFT writes it.  Both graphs must have the same k.  cut_lvl and packed_in_subtries describe the
 * reference's on-disk form split into sub-tries, which this library does not have: they are accepted and ignored.  Errors (a file that cannot be
 * read or written, different k) print a message on stderr and exit(EXIT_FAILURE), as everywhere in <bft/bft.h>. */
void merging_BFT(char* prefix_bft1, char* prefix_bft2, char* output_prefix, int cut_lvl, bool packed_in_subtries);

#ifdef __cplusplus
}
#endif

#endif
