/*
 * <bft/snippets_traversal.h> -- the graph traversal snippets of GuillaumeHolley/BloomFilterTrie (reference include/snippets.h, src/snippets.c:605-960),
 * included by <bft/snippets.h>.  The number of connected components is one GPU pass over the whole index (bft_gpu_components, include/bft_gpu.h)
 * instead of a BFS or DFS that marks one k-mer at a time.  The count is the reference's: components do not depend on the order of a walk.
 *
 * Not provided: cdbg_traversal, and nb_connected_components as a callback of iterate_over_kmers (they need marking).  The k-mer class extractors
 * (extract_core_kmers and its kin), which need none, are in <bft/snippets_pangenome.h>.
 */
#ifndef BFT_GPU_COMPAT_SNIPPETS_TRAVERSAL_H
#define BFT_GPU_COMPAT_SNIPPETS_TRAVERSAL_H

#include <stdarg.h>
#include <stdbool.h>

#include "bft.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The traversals a program passes to get_nb_connected_component, which tells them apart by their addresses.  Called directly, or through
 * iterate_over_kmers, they need vertex marking, which this library does not provide: a message naming get_nb_connected_component on stderr,
 * then exit(EXIT_FAILURE). */
size_t BFS(BFT_kmer* kmer, BFT* graph, va_list args);
size_t BFS_subgraph(BFT_kmer* kmer, BFT* graph, va_list args);
size_t DFS(BFT_kmer* kmer, BFT* graph, va_list args);
size_t DFS_subgraph(BFT_kmer* kmer, BFT* graph, va_list args);
/* src/snippets.c:824-881: true when the colour set of kmer holds the nb_id_genomes uint32_t ids of args.  As in the reference, the k-mer's sorted
 * id list is walked against the ids in the order given: nb_id_genomes <= 0, or ids that are not strictly increasing, give false. */
bool is_in_subgraph(BFT_kmer* kmer, BFT* graph, int nb_id_genomes, const va_list args);
/* src/snippets.c:915-960: get_nb_connected_component(graph, int* nb, BFT_func_ptr f) with f = BFS or DFS, or
 * get_nb_connected_component(graph, int* nb, BFT_func_ptr f, int nb_id_genomes, uint32_t id, ...) with f = BFS_subgraph or DFS_subgraph, ADDS to *nb
 * the number of connected components of the graph, or of the sub-graph induced by the k-mers that carry every id (bft_gpu_components defines
 * them).  nb_id_genomes <= 0, or ids that are not strictly increasing, add 0.  Any other f is an error (message on stderr, exit(EXIT_FAILURE)). */
void get_nb_connected_component(BFT* graph, ...);

#ifdef __cplusplus
}
#endif

#endif
