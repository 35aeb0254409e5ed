/*
 * <bft/snippets_pangenome.h> -- the pan-genome k-mer class snippets of GuillaumeHolley/BloomFilterTrie (reference include/snippets.h:38-41,
 * src/snippets.c:10-106), included by <bft/snippets.h>.  A class is selected, compacted and spelled by one GPU pass over the whole index
 * (bft_gpu_kmers_by_count, include/bft_gpu.h) instead of one annotation fetch per k-mer: only the k-mers of the class cross to the host.
 *
 * The k-mers are written in ascending row order (the order of iterate_over_kmers here); the reference writes them in the order of its containers:
 * the same set, k + 1 bytes per k-mer (the terminating NUL included, no newline), as src/snippets.c:21 does.
 */
#ifndef BFT_GPU_COMPAT_SNIPPETS_PANGENOME_H
#define BFT_GPU_COMPAT_SNIPPETS_PANGENOME_H

#include <stdarg.h>

#include "bft.h"

#ifdef __cplusplus
extern "C" {
#endif

/* src/snippets.c:10-75: callbacks of type BFT_func_ptr whose arguments are a FILE* and an int*: a core k-mer (carried by all graph->nb_genomes
 * genomes), a dispensable k-mer (by fewer) or a singleton k-mer (by exactly one) is written to the file with its NUL and counted in the int.  They
 * return 1 (go on).  extract_pangenome_kmers_to_disk tells them apart by their addresses and serves them from the GPU; called directly, or through
 * iterate_over_kmers(graph, extract_core_kmers, file, &n), they do what the reference's do, one k-mer at a time. */
size_t extract_core_kmers(BFT_kmer* kmer, BFT* graph, va_list args);
size_t extract_dispensable_kmers(BFT_kmer* kmer, BFT* graph, va_list args);
size_t extract_singleton_kmers(BFT_kmer* kmer, BFT* graph, va_list args);
/* src/snippets.c:86-106: the k-mers of the class f selects into filename_output; then "Number of extracted k-mers is %d.\n" on stdout.  f is one of
 * the three callbacks above, or any callback of the caller's with the same arguments (then every k-mer is handed to it through iterate_over_kmers, as
 * in the reference).  A file that cannot be created is an error (message on stderr, exit(EXIT_FAILURE)), as in the reference. */
void extract_pangenome_kmers_to_disk(BFT* graph, char* filename_output, BFT_func_ptr f);

#ifdef __cplusplus
}
#endif

#endif
