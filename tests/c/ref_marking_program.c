/* Vertex marking and the traversal snippets (reference bft.h: set_marking, unset_marking, set_flag_kmer, get_flag_kmer; snippets.h: BFS, DFS,
 * BFS_subgraph, nb_connected_components, cdbg_traversal) used the way a program of the reference uses them: written against <bft/bft.h> and
 * <bft/snippets.h> only, linked with -lbft.
 * usage: ref_marking_program k mode kmer_file...
 *   flags      set_marking; through iterate_over_kmers every third k-mer (0, 3, 6 ..) gets the flag 1 + (i / 3) % 3; "kmer flag" for every k-mer; then
 *              unset_marking, set_marking and "again flag-sum" (0)
 *   traverse   set_marking, then iterate_over_kmers(nb_connected_components, &nb, f) as the reference's get_nb_connected_component does: "BFS n", and
 *              "direct r": BFS called on the first k-mer again (visited: 0); "count n": get_nb_connected_component's own count; from fresh marks
 *              "DFS n"; from fresh marks "BFS_subgraph n" with ids {0, 1} and "flags <one digit per k-mer>" behind it
 *   cdbg       cdbg_traversal(bft, BFS_subgraph, 1, 0u): "marked m" (bit 0 of bft->marked behind it); cdbg_traversal(bft, nb_connected_components,
 *              &nb, BFS): "cdbg n"
 *   flag4 | unmarked | absent   set_flag_kmer with the flag 4, on a graph that is not marking, on a k-mer that is not in the graph: errors */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <bft/bft.h>
#include <bft/snippets.h>

static size_t set_third(BFT_kmer* kmer, BFT* bft, va_list args) {
    int* i = va_arg(args, int*);
    if (*i % 3 == 0) set_flag_kmer((uint8_t)(1 + (*i / 3) % 3), kmer, bft);
    *i += 1;
    return 1;
}

static size_t print_flag(BFT_kmer* kmer, BFT* bft, va_list args) {
    (void)args;
    printf("%s %d\n", kmer->kmer, (int)get_flag_kmer(kmer, bft));
    return 1;
}

static size_t sum_flag(BFT_kmer* kmer, BFT* bft, va_list args) {
    int* sum = va_arg(args, int*);
    *sum += get_flag_kmer(kmer, bft);
    return 1;
}

static size_t digit_flag(BFT_kmer* kmer, BFT* bft, va_list args) {
    (void)args;
    putchar('0' + get_flag_kmer(kmer, bft));
    return 1;
}

static size_t first_kmer(BFT_kmer* kmer, BFT* bft, va_list args) {
    (void)bft;
    char* out = va_arg(args, char*);
    strcpy(out, kmer->kmer);
    return 0;
}

static size_t call(BFT_func_ptr f, BFT_kmer* kmer, BFT* bft, ...) {
    va_list args;
    va_start(args, bft);
    const size_t r = f(kmer, bft, args);
    va_end(args);
    return r;
}

int main(int argc, char** argv) {
    if (argc < 4) {
        fprintf(stderr, "usage: %s k flags|traverse|cdbg|flag4|unmarked|absent kmer_file...\n", argv[0]);
        return 2;
    }
    const int k = atoi(argv[1]);
    const char* mode = argv[2];
    BFT* bft = create_cdbg(k, 0);
    insert_genomes_from_files(argc - 3, argv + 3, bft, NULL);
    char* first = malloc((size_t)k + 1);
    iterate_over_kmers(bft, first_kmer, first);
    if (strcmp(mode, "flags") == 0) {
        int i = 0, sum = 0;
        set_marking(bft);
        set_marking(bft); /* (already marking: nothing changes) */
        iterate_over_kmers(bft, set_third, &i);
        iterate_over_kmers(bft, print_flag);
        unset_marking(bft);
        set_marking(bft);
        iterate_over_kmers(bft, sum_flag, &sum);
        printf("again %d\n", sum);
        unset_marking(bft);
    } else if (strcmp(mode, "traverse") == 0) {
        int nb = 0;
        set_marking(bft);
        iterate_over_kmers(bft, nb_connected_components, &nb, BFS);
        printf("BFS %d\n", nb);
        BFT_kmer* km = get_kmer(first, bft);
        printf("direct %d\n", (int)call(BFS, km, bft));
        free_BFT_kmer(km, 1);
        nb = 0;
        get_nb_connected_component(bft, &nb, BFS);
        printf("count %d\n", nb);
        unset_marking(bft);
        set_marking(bft);
        nb = 0;
        iterate_over_kmers(bft, nb_connected_components, &nb, DFS);
        printf("DFS %d\n", nb);
        unset_marking(bft);
        set_marking(bft);
        nb = 0;
        iterate_over_kmers(bft, nb_connected_components, &nb, BFS_subgraph, 2, 0u, 1u);
        printf("BFS_subgraph %d\n", nb);
        printf("flags ");
        iterate_over_kmers(bft, digit_flag);
        printf("\n");
        unset_marking(bft);
    } else if (strcmp(mode, "cdbg") == 0) {
        int nb = 0;
        cdbg_traversal(bft, BFS_subgraph, 1, 0u);
        printf("marked %d\n", bft->marked & 1);
        cdbg_traversal(bft, nb_connected_components, &nb, BFS);
        printf("cdbg %d\n", nb);
        printf("marked %d\n", bft->marked & 1);
    } else if (strcmp(mode, "flag4") == 0) {
        BFT_kmer* km = get_kmer(first, bft);
        set_marking(bft);
        set_flag_kmer(4, km, bft);
    } else if (strcmp(mode, "unmarked") == 0) {
        BFT_kmer* km = get_kmer(first, bft);
        set_flag_kmer(1, km, bft);
    } else if (strcmp(mode, "absent") == 0) {
        memset(first, 'A', (size_t)k);
        first[0] = 'C';
        first[k - 1] = 'G';
        BFT_kmer* km = get_kmer(first, bft); /* (C A..A G: not in the random genomes of the test) */
        set_marking(bft);
        set_flag_kmer(1, km, bft);
    } else {
        fprintf(stderr, "unknown mode %s\n", mode);
        return 2;
    }
    free(first);
    free_cdbg(bft);
    return 0;
}
