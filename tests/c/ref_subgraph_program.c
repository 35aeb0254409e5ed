/* create_cdbg_from_bft_kmers and add_id_genomes (include/bft.h:179-180, src/bft.c:1353-1684) used the way a program of the reference uses
 * them: written against <bft/bft.h> only, linked with -lbft.
 * usage: ref_subgraph_program k colors|plain|add query_file kmer_file...   (the graph is built from the kmer files, one genome each)
 *   colors / plain  create_cdbg_from_bft_kmers over the k-mers of query_file (one per line) with add_colors true / false; prints
 *                   "genomes <n> <name of genome 0>", then one line "<k-mer> <genome id>,<genome id>,..." per k-mer of the new graph
 *                   (iterate_over_kmers, get_annotation + get_list_id_genomes)
 *   add             add_id_genomes(k-mer, NULL, bft, {2, 2, 0}) on the first k-mer of query_file: prints its ids through the same BFT_kmer,
 *                   then through a fresh get_kmer
 *   addbad          add_id_genomes with the id nb_genomes: the reference's message and exit */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <bft/bft.h>

static void print_ids(BFT_kmer* bft_kmer, BFT* bft, FILE* out) {
    BFT_annotation* annot = get_annotation(bft_kmer);
    uint32_t* ids = get_list_id_genomes(annot, bft);
    fprintf(out, "%s ", bft_kmer->kmer);
    for (uint32_t i = 1; i <= ids[0]; i++) fprintf(out, i > 1 ? ",%u" : "%u", ids[i]);
    fprintf(out, "\n");
    free(ids);
    free_BFT_annotation(annot);
}

static size_t print_kmer(BFT_kmer* bft_kmer, BFT* bft, va_list args) {
    print_ids(bft_kmer, bft, va_arg(args, FILE*));
    return 1;
}

int main(int argc, char** argv) {
    if (argc < 5) {
        fprintf(stderr, "usage: %s k colors|plain|add|addbad query_file kmer_file...\n", argv[0]);
        return 2;
    }
    const int k = atoi(argv[1]);
    BFT* bft = create_cdbg(k, 0);
    insert_genomes_from_files(argc - 4, argv + 4, bft, NULL);
    FILE* f = fopen(argv[3], "r");
    if (f == NULL) return 2;
    size_t cap = 1024, n = 0;
    BFT_kmer** kmers = malloc(cap * sizeof(BFT_kmer*));
    char line[512];
    while (fgets(line, sizeof line, f) != NULL) {
        if (strlen(line) < (size_t)k) continue;
        line[k] = '\0';
        if (n == cap) kmers = realloc(kmers, (cap *= 2) * sizeof(BFT_kmer*));
        kmers[n++] = get_kmer(line, bft);
    }
    fclose(f);
    if (strcmp(argv[2], "colors") == 0 || strcmp(argv[2], "plain") == 0) {
        BFT* sub = create_cdbg_from_bft_kmers(kmers, (uint32_t)n, bft, strcmp(argv[2], "colors") == 0);
        printf("genomes %d %s\n", sub->nb_genomes, sub->filenames[0]);
        iterate_over_kmers(sub, print_kmer, stdout);
        free_cdbg(sub);
    } else if (n > 0) {
        uint32_t list[3] = {2, 2, 0};
        if (strcmp(argv[2], "addbad") == 0) list[1] = (uint32_t)bft->nb_genomes;
        add_id_genomes(kmers[0], NULL, bft, list);
        print_ids(kmers[0], bft, stdout);
        BFT_kmer* again = get_kmer(kmers[0]->kmer, bft);
        print_ids(again, bft, stdout);
        free_BFT_kmer(again, 1);
    }
    for (size_t i = 0; i < n; i++) free_BFT_kmer(kmers[i], 1);
    free(kmers);
    free_cdbg(bft);
    return 0;
}
