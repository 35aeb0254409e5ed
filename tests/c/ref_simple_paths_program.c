/* extract_simple_paths_to_disk / extract_simple_core_paths_to_disk (reference snippets.h, src/snippets.c:306-603) used the way a program of
 * the reference uses them: written against <bft/bft.h> and <bft/snippets.h> only, linked with -lbft.
 * usage: ref_simple_paths_program k plain|core core_ratio output_file kmer_file...
 *   plain  extract_simple_paths_to_disk(bft, output_file)
 *   core   extract_simple_core_paths_to_disk(bft, core_ratio, output_file) */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <bft/bft.h>
#include <bft/snippets.h>

int main(int argc, char** argv) {
    if (argc < 6) {
        fprintf(stderr, "usage: %s k plain|core core_ratio output_file kmer_file...\n", argv[0]);
        return 2;
    }
    BFT* bft = create_cdbg(atoi(argv[1]), 0);
    insert_genomes_from_files(argc - 5, argv + 5, bft, NULL);
    if (strcmp(argv[2], "plain") == 0) extract_simple_paths_to_disk(bft, argv[4]);
    else extract_simple_core_paths_to_disk(bft, atof(argv[3]), argv[4]);
    free_cdbg(bft);
    return 0;
}
