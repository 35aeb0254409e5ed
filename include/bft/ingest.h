/*
 * <bft/ingest.h> -- genomes inserted from their SEQUENCES.  An EXTENSION: GuillaumeHolley/BloomFilterTrie has no counterpart -- its
 * insert_genomes_from_files (include/bft.h) reads k-mers that a k-mer counter has cut out of every genome beforehand.  Served by
 * bft_gpu_insert_sequence_file (include/bft_gpu.h): the windows are cut, put into canonical form and -- with min_abundance -- counted on the GPU.
 */
#ifndef BFT_GPU_COMPAT_INGEST_H
#define BFT_GPU_COMPAT_INGEST_H

#include "bft.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Each of the nb_files plain-text FASTA or four-line FASTQ files becomes one new genome, named as insert_genomes_from_files names it (the
 * file's base name), holding every k-mer of the file's sequences that has no character outside ACGTU (either case).  canonical != 0: the
 * lexicographically smaller of a k-mer and its reverse complement is inserted -- what query_sequence(..., canonical_search = true) looks up.
 * min_abundance >= 1: only k-mers that occur at least that often in their file (both strands together with canonical) are inserted;
 * 0: every k-mer.  Errors (a file that cannot be read or is neither format) print a message on stderr and exit(EXIT_FAILURE), as everywhere
 * in <bft/bft.h>. */
void insert_genomes_from_sequence_files(int nb_files, char** paths, int canonical, uint32_t min_abundance, BFT_Root* root);

#ifdef __cplusplus
}
#endif

#endif
