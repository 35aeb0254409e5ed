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

/* The compacted coloured graph of a canonical index (bft_gpu_unitig_graph defines it: the unitigs above, one segment more for every branching
 * k-mer, and the links between oriented segments) written to filename_output as GFA 1:
 *   H  VN:Z:1.0  kl:i:<k>
 *   S  <i>  <sequence>  LN:i:<length>              one per segment, in the call's order; with colors also
 *      cu:H:<row>  ci:H:<row>  gc:i:<n>            the genomes that hold a k-mer of the segment (union), those that hold all of them (intersection) --
 *                                                  CEIL(nb_genomes / 8) bytes, genome g at bit g % 8 of byte g / 8, two hexadecimal digits per byte --
 *                                                  and the number of genomes in the union
 *   L  <i>  <+|->  <j>  <+|->  <k-1>M              one per link, in the order of the link lists: both mirror forms are written
 * (fields separated by tabs).  min_shared as for extract_unitigs_to_disk.  Errors print a message on stderr and exit(EXIT_FAILURE). */
void extract_unitig_graph_to_disk(BFT* graph, int min_shared, bool colors, char* filename_output);

/* The simple bubbles (variants) of that graph (bft_gpu_unitig_bubbles defines them: two to four parallel segments between the same two flanks, each
 * reported once) written to filename_output as text, one block per bubble in the call's order, fields separated by tabs:
 *   B  <index>  <source id><+|->  <sink id><+|->  <m>                                        the bubble: its number, source, sink, branches
 *   A  <segment id><+|->  <sequence in that orientation>  <number of genomes>  <genome ids>  one per branch, in the source's link order
 * The genomes of a branch are the intersection row of its segment: the genomes that hold every k-mer of the allele, ascending, separated by commas.
 * Segment ids are those of extract_unitig_graph_to_disk at the same min_shared (- is the reverse complement of the S line), so the file joins to the
 * GFA.  max_branch_length > 0: only bubbles whose branches all have at most that many nucleotides (0 or less: no limit).  min_shared and errors as
 * above. */
void extract_bubbles_to_disk(BFT* graph, int min_shared, int max_branch_length, char* filename_output);

/* Where do sequences run in that graph?  Every record of the plain-text FASTA / FASTQ file filename_sequences is threaded through the compacted graph
 * at min_shared (bft_gpu_thread_sequences defines the walks: the maximal stretches of a sequence whose k-mers are all in segments and follow each
 * other inside a segment or across a link) and written to filename_output as GAF, one line per walk in the call's order, fields separated by tabs:
 *   <name>  <sequence length>  <start>  <end>  +  <path>  <path length>  <path start>  <path end>  <matches>  <block length>  255  cg:Z:<matches>=
 * The name is the record's header up to the first blank (an empty one: the record's number, from 0); the path is >i or <i per step, i a segment id of
 * extract_unitig_graph_to_disk at the same min_shared (<i reads the reverse complement of the S line), so the file joins to the GFA; a walk is an
 * exact match: matches = block length = end - start = path end - path start.  min_shared and errors as above; a sequence file that cannot be read is
 * an error too. */
void thread_sequences_to_disk(BFT* graph, int min_shared, char* filename_sequences, char* filename_output);

#ifdef __cplusplus
}
#endif

#endif
