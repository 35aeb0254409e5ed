/*
 * <bft/snippets_traversal.h> -- the graph traversal snippets of GuillaumeHolley/BloomFilterTrie (reference include/snippets.h, src/snippets.c:605-960),
 * included by <bft/snippets.h>.  The number of connected components is one GPU pass over the whole index (bft_gpu_components, include/bft_gpu.h)
 * instead of a BFS or DFS that marks one k-mer at a time.  The count is the reference's: components do not depend on the order of a walk.
 *
 * The traversals themselves (BFS, DFS, BFS_subgraph, DFS_subgraph called on a k-mer of a marking graph, cdbg_traversal, nb_connected_components) are one
 * bft_gpu_marks_reach per call: the marks they leave are the reference's, found by a union-find over the whole index instead of a walk.  The k-mer class
 * extractors (extract_core_kmers and its kin) are in <bft/snippets_pangenome.h>.
 */
#ifndef BFT_GPU_COMPAT_SNIPPETS_TRAVERSAL_H
#define BFT_GPU_COMPAT_SNIPPETS_TRAVERSAL_H

#include <stdarg.h>
#include <stdbool.h>

#include "bft.h"

#ifdef __cplusplus
extern "C" {
#endif

/* src/snippets.c:605-812.  On a graph that is marking (set_marking, <bft/bft.h>), called directly or through iterate_over_kmers / cdbg_traversal: 0 when
 * the k-mer's flag is not 0 (V_NOT_VISITED); otherwise the k-mer and everything the reference's walk would mark from it get the flag 1 (V_VISITED) --
 * the whole component, or for the _subgraph forms (args: int nb_id_genomes, uint32_t id, ...) the component induced by the k-mers that carry every id,
 * plus the unvisited k-mers next to it, plus the k-mer itself when it is not in the sub-graph -- and the result is 1 when a new component was entered.
 * On a graph that is NOT marking they stop the program: a message that starts with the function's name and names get_nb_connected_component (which
 * needs no marks and tells the four apart by their addresses) on stderr, then exit(EXIT_FAILURE). */
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
/* src/snippets.c:883-906: set_marking, f on every k-mer (v_iterate_over_kmers with the arguments behind f), unset_marking.  With the forest kept by
 * bft_gpu_marks_reach the whole traversal costs one union-find, and one painting pass per component. */
void cdbg_traversal(BFT* graph, BFT_func_ptr f, ...);
/* src/snippets.c:915-930: a callback for iterate_over_kmers on a marking graph -- args: int* nb, BFT_func_ptr f, f's own arguments; *nb += f(...) == 1. */
size_t nb_connected_components(BFT_kmer* kmer, BFT* graph, va_list args);

#ifdef __cplusplus
}
#endif

#endif
