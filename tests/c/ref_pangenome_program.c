/* The pan-genome k-mer class snippets (reference snippets.h, src/snippets.c:10-106) used the way a program of the reference uses them: written against
 * <bft/snippets.h> only, linked with -lbft.
 * usage: ref_pangenome_program k mode out_prefix kmer_file...
 *   disk       out_prefix.core / .dispensable / .singleton through extract_pangenome_kmers_to_disk (one "Number of extracted k-mers is N." line each)
 *   iterate    the same three files through iterate_over_kmers(graph, extract_*_kmers, file, &n); then "core n", "dispensable n", "singleton n"
 *   own        out_prefix.two: the k-mers of exactly two genomes through a callback of this program handed to extract_pangenome_kmers_to_disk
 *   unwritable extract_pangenome_kmers_to_disk into out_prefix itself, which the caller makes uncreatable: an error */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <bft/snippets.h>

static size_t extract_two_genome_kmers(BFT_kmer* kmer, BFT* graph, va_list args) {
    FILE* file = va_arg(args, FILE*);
    int* nb = va_arg(args, int*);
    BFT_annotation* annot = get_annotation(kmer);
    if (get_count_id_genomes(annot, graph) == 2) {
        fwrite(kmer->kmer, sizeof(char), strlen(kmer->kmer) + 1, file);
        *nb += 1;
    }
    free_BFT_annotation(annot);
    return 1;
}

static char* name_of(const char* prefix, const char* what) {
    char* s = malloc(strlen(prefix) + strlen(what) + 2);
    if (s == NULL) exit(3);
    sprintf(s, "%s.%s", prefix, what);
    return s;
}

int main(int argc, char** argv) {
    if (argc < 5) {
        fprintf(stderr, "usage: %s k disk|iterate|own|unwritable out_prefix kmer_file...\n", argv[0]);
        return 2;
    }
    static const char* const what[3] = {"core", "dispensable", "singleton"};
    const BFT_func_ptr f[3] = {extract_core_kmers, extract_dispensable_kmers, extract_singleton_kmers};
    BFT* bft = create_cdbg(atoi(argv[1]), 0);
    insert_genomes_from_files(argc - 4, argv + 4, bft, NULL);
    if (strcmp(argv[2], "disk") == 0) {
        for (int i = 0; i < 3; i++) {
            char* name = name_of(argv[3], what[i]);
            extract_pangenome_kmers_to_disk(bft, name, f[i]);
            free(name);
        }
    } else if (strcmp(argv[2], "iterate") == 0) {
        for (int i = 0; i < 3; i++) {
            char* name = name_of(argv[3], what[i]);
            FILE* file = fopen(name, "w");
            if (file == NULL) return 3;
            int n = 0;
            iterate_over_kmers(bft, f[i], file, &n);
            fclose(file);
            printf("%s %d\n", what[i], n);
            free(name);
        }
    } else if (strcmp(argv[2], "own") == 0) {
        char* name = name_of(argv[3], "two");
        extract_pangenome_kmers_to_disk(bft, name, extract_two_genome_kmers);
        free(name);
    } else
        extract_pangenome_kmers_to_disk(bft, argv[3], extract_core_kmers);
    free_cdbg(bft);
    return 0;
}
