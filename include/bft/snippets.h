/*
 * <bft/snippets.h> -- the simple-path, connected-component and pan-genome class snippets of GuillaumeHolley/BloomFilterTrie (reference
 * include/snippets.h, src/snippets.c), served by the MI355X library: one batched GPU pass over the whole index (bft_gpu_simple_paths,
 * bft_gpu_components, bft_gpu_kmers_by_count, include/bft_gpu.h) instead of a walk that asks for the successors, predecessors, marks or annotation
 * of one k-mer at a time.
 *
 * The paths are those bft_gpu_simple_paths defines: maximal chains of k-mers with in- and out-degree <= 1 (degrees over the whole graph),
 * each spelled as its first k-mer plus the last nucleotide of every following one; a cycle is cut before its k-mer of smallest row.  They are
 * written one per line in ascending row of their first k-mer (the order of iterate_over_kmers); the reference writes them in the order its
 * walk happens to reach them, and that order also decides where it starts a cycle (INTEGRATION.md lists every difference).
 *
 * The traversals BFS, DFS, BFS_subgraph, DFS_subgraph, the predicate is_in_subgraph, get_nb_connected_component, cdbg_traversal and
 * nb_connected_components are declared in <bft/snippets_traversal.h>; the k-mer class extractors extract_core_kmers / extract_dispensable_kmers / extract_singleton_kmers and
 * extract_pangenome_kmers_to_disk in <bft/snippets_pangenome.h>.  This header includes both.
 *
 * Not provided: the per-k-mer callbacks extract_simple_paths and extract_core_simple_paths (vertex marking, which they need, is provided by
 * <bft/bft.h>; their reference text has undefined behaviour).  The annotation set operations intersection_annotations /
 * union_annotations / sym_difference_annotations are declared in <bft/bft.h>.
 */
#ifndef BFT_GPU_COMPAT_SNIPPETS_H
#define BFT_GPU_COMPAT_SNIPPETS_H

#include "bft.h"
#include "snippets_pangenome.h"
#include "snippets_traversal.h"

#ifdef __cplusplus
extern "C" {
#endif

/* src/snippets.c:306-344: every simple path of graph into filename_output, one per line; then "Longest simple path has %d nuc.\n" on stdout.
 * A file that cannot be created is an error (message on stderr, exit(EXIT_FAILURE)), as in the reference. */
void extract_simple_paths_to_disk(BFT* graph, char* filename_output);
/* src/snippets.c:563-603: the same over core k-mers, whose colour set holds at least t = (int)(core_ratio * graph->nb_genomes) genomes,
 * and whose edges join k-mers that share t genomes or more; then "Longest simple core path has %d nuc.\n". */
void extract_simple_core_paths_to_disk(BFT* graph, double core_ratio, char* filename_output);

#ifdef __cplusplus
}
#endif

#endif
