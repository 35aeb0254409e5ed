/* extract_unitig_graph_to_disk (<bft/unitigs.h>, an extension of this library) used the way a program of the reference uses <bft/bft.h>: written
 * against the headers only, linked with -lbft.
 * usage: ref_cgraph_program k {sequences_canonical|sequences} min_shared colors output_file genome_file...
 *   the genome files are FASTA / FASTQ and go through insert_genomes_from_sequence_files (canonical or not); the compacted coloured graph goes to
 *   output_file as GFA 1, with the colour tags when colors is 1 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <bft/bft.h>
#include <bft/ingest.h>
#include <bft/unitigs.h>

int main(int argc, char** argv) {
    if (argc < 7) {
        fprintf(stderr, "usage: %s k {sequences_canonical|sequences} min_shared colors output_file genome_file...\n", argv[0]);
        return 2;
    }
    const int k = atoi(argv[1]), n_files = argc - 6;
    BFT* bft = create_cdbg(k, 0);
    insert_genomes_from_sequence_files(n_files, argv + 6, strcmp(argv[2], "sequences_canonical") == 0, 0, bft);
    extract_unitig_graph_to_disk(bft, atoi(argv[3]), atoi(argv[4]) != 0, argv[5]);
    free_cdbg(bft);
    return 0;
}
