/* prefix_matching (include/bft.h:135, src/bft.c:1087-1147) used the way a program of the reference uses it: written against <bft/bft.h>
 * only, linked with -lbft.
 * usage: ref_prefix_program k list|stop3 prefix kmer_file...
 *   list   one line "<k-mer> <genome id>,<genome id>,..." per match (get_annotation + get_list_id_genomes inside the callback), then
 *          "matched <0|1> calls <n>"
 *   stop3  the callback returns 0 on its third call: "matched <0|1> calls <n>" */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <bft/bft.h>

static size_t print_match(BFT_kmer* bft_kmer, BFT* bft, va_list args) {
    FILE* out = va_arg(args, FILE*);
    int* calls = va_arg(args, int*);
    BFT_annotation* annot = get_annotation(bft_kmer);
    uint32_t* ids = get_list_id_genomes(annot, bft);
    fprintf(out, "%s ", bft_kmer->kmer);
    for (uint32_t i = 1; i <= ids[0]; i++) fprintf(out, i > 1 ? ",%u" : "%u", ids[i]);
    fprintf(out, "\n");
    free(ids);
    free_BFT_annotation(annot);
    (*calls)++;
    return 1;
}

static size_t stop_at_three(BFT_kmer* bft_kmer, BFT* bft, va_list args) {
    (void)bft_kmer;
    (void)bft;
    int* calls = va_arg(args, int*);
    (*calls)++;
    return *calls < 3;
}

int main(int argc, char** argv) {
    if (argc < 5) {
        fprintf(stderr, "usage: %s k list|stop3 prefix kmer_file...\n", argv[0]);
        return 2;
    }
    BFT* bft = create_cdbg(atoi(argv[1]), 0);
    insert_genomes_from_files(argc - 4, argv + 4, bft, NULL);
    int calls = 0;
    bool matched;
    if (strcmp(argv[2], "list") == 0) matched = prefix_matching(bft, argv[3], print_match, stdout, &calls);
    else matched = prefix_matching(bft, argv[3], stop_at_three, &calls);
    printf("matched %d calls %d\n", matched ? 1 : 0, calls);
    free_cdbg(bft);
    return 0;
}
