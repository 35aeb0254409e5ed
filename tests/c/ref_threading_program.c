/* thread_sequences_to_disk (<bft/unitigs.h>, an extension of this library) used the way a program of the reference uses <bft/bft.h>: written
 * against the headers only, linked with -lbft.
 * usage: ref_threading_program k {sequences_canonical|sequences} min_shared sequence_file gaf_file gfa_file genome_file...
 *   the genome files are FASTA / FASTQ and go through insert_genomes_from_sequence_files (canonical or not); the records of sequence_file are
 *   threaded through the compacted coloured graph and their walks go to gaf_file, the graph itself at the same min_shared to gfa_file as GFA 1
 *   (- : no GFA file) */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <bft/bft.h>
#include <bft/ingest.h>
#include <bft/unitigs.h>

int main(int argc, char** argv) {
    if (argc < 8) {
        fprintf(stderr, "usage: %s k {sequences_canonical|sequences} min_shared sequence_file gaf_file gfa_file genome_file...\n", argv[0]);
        return 2;
    }
    const int k = atoi(argv[1]), n_files = argc - 7;
    BFT* bft = create_cdbg(k, 0);
    insert_genomes_from_sequence_files(n_files, argv + 7, strcmp(argv[2], "sequences_canonical") == 0, 0, bft);
    thread_sequences_to_disk(bft, atoi(argv[3]), argv[4], argv[5]);
    if (strcmp(argv[6], "-") != 0) extract_unitig_graph_to_disk(bft, atoi(argv[3]), false, argv[6]);
    free_cdbg(bft);
    return 0;
}
