/* get_nb_connected_component and is_in_subgraph (reference snippets.h, src/snippets.c:605-960) used the way a program of the reference uses them:
 * written against <bft/bft.h> and <bft/snippets.h> only, linked with -lbft.
 * usage: ref_components_program k mode kmer_file...
 *   count      one line per call: "BFS n", "DFS n" (whole graph), "BFS_subgraph n", "DFS_subgraph n" (ids {0}, then {0, 1}, then {1, 2}), each
 *              counted from *nb = 0; then "acc n": BFS, DFS and BFS_subgraph {0} added to one *nb that starts at 1000; then "zero n": nb_id_genomes 0,
 *              ids {1, 0} and ids {1, 1} added to *nb = 5
 *   member     "kmer ids": for every k-mer of the first file, is_in_subgraph with {0}, {0, 1}, {1, 2}, {2, 1} and nb_id_genomes 0 as 0/1 digits
 *   bad        get_nb_connected_component with iterate_over_kmers's own callback: an error
 *   direct     iterate_over_kmers with BFS: an error (BFS needs marking) */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <bft/bft.h>
#include <bft/snippets.h>

static bool call_is_in_subgraph(BFT_kmer* kmer, BFT* bft, int nb, ...) {
    va_list args;
    va_start(args, nb);
    const bool r = is_in_subgraph(kmer, bft, nb, args);
    va_end(args);
    return r;
}

static size_t print_member(BFT_kmer* kmer, BFT* bft, va_list args) {
    (void)args;
    printf("%s %d%d%d%d%d\n", kmer->kmer, call_is_in_subgraph(kmer, bft, 1, 0u), call_is_in_subgraph(kmer, bft, 2, 0u, 1u),
           call_is_in_subgraph(kmer, bft, 2, 1u, 2u), call_is_in_subgraph(kmer, bft, 2, 2u, 1u), call_is_in_subgraph(kmer, bft, 0, 0u));
    return 1;
}

int main(int argc, char** argv) {
    if (argc < 4) {
        fprintf(stderr, "usage: %s k count|member|bad|direct kmer_file...\n", argv[0]);
        return 2;
    }
    BFT* bft = create_cdbg(atoi(argv[1]), 0);
    insert_genomes_from_files(argc - 3, argv + 3, bft, NULL);
    if (strcmp(argv[2], "count") == 0) {
        int nb = 0;
        get_nb_connected_component(bft, &nb, BFS);
        printf("BFS %d\n", nb);
        nb = 0;
        get_nb_connected_component(bft, &nb, DFS);
        printf("DFS %d\n", nb);
        nb = 0;
        get_nb_connected_component(bft, &nb, BFS_subgraph, 1, 0u);
        printf("BFS_subgraph %d\n", nb);
        nb = 0;
        get_nb_connected_component(bft, &nb, DFS_subgraph, 2, 0u, 1u);
        printf("DFS_subgraph %d\n", nb);
        nb = 0;
        get_nb_connected_component(bft, &nb, BFS_subgraph, 2, 1u, 2u);
        printf("BFS_subgraph %d\n", nb);
        nb = 1000;
        get_nb_connected_component(bft, &nb, BFS);
        get_nb_connected_component(bft, &nb, DFS);
        get_nb_connected_component(bft, &nb, BFS_subgraph, 1, 0u);
        printf("acc %d\n", nb);
        nb = 5;
        get_nb_connected_component(bft, &nb, BFS_subgraph, 0);
        get_nb_connected_component(bft, &nb, DFS_subgraph, 2, 1u, 0u);
        get_nb_connected_component(bft, &nb, BFS_subgraph, 2, 1u, 1u);
        printf("zero %d\n", nb);
    } else if (strcmp(argv[2], "member") == 0)
        iterate_over_kmers(bft, print_member);
    else if (strcmp(argv[2], "direct") == 0)
        iterate_over_kmers(bft, BFS);
    else
        get_nb_connected_component(bft, &(int){0}, print_member);
    free_cdbg(bft);
    return 0;
}
