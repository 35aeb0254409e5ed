/* merging_BFT (include/merge.h:14) used the way a program of the reference uses it: written against <bft/bft.h> and <bft/merge.h> only, linked
 * with -lbft.
 * usage: ref_merge_program k query_file out_prefix n1 kmer_file...
 *   the first n1 kmer files (one genome each) make graph 1, the others graph 2; both are written with write_BFT to <out_prefix>.1 and
 *   <out_prefix>.2 and freed; merging_BFT(<out_prefix>.1, <out_prefix>.2, <out_prefix>.m, 0, false); the result is loaded with load_BFT.
 *   prints "genomes <n>", one line "name <id> <name>" per genome, then per k-mer of query_file (one per line)
 *   "<k-mer> <genome id>,<genome id>,..." or "<k-mer> -" when the merged graph does not hold it. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <bft/bft.h>
#include <bft/merge.h>

int main(int argc, char** argv) {
    if (argc < 6) {
        fprintf(stderr, "usage: %s k query_file out_prefix n1 kmer_file...\n", argv[0]);
        return 2;
    }
    const int k = atoi(argv[1]), n1 = atoi(argv[4]), n_files = argc - 5;
    if (n1 < 0 || n1 > n_files) return 2;
    char p1[4096], p2[4096], pm[4096];
    snprintf(p1, sizeof p1, "%s.1", argv[3]);
    snprintf(p2, sizeof p2, "%s.2", argv[3]);
    snprintf(pm, sizeof pm, "%s.m", argv[3]);
    BFT* g1 = create_cdbg(k, 0);
    insert_genomes_from_files(n1, argv + 5, g1, NULL);
    write_BFT(g1, p1, false);
    free_cdbg(g1);
    BFT* g2 = create_cdbg(k, 0);
    insert_genomes_from_files(n_files - n1, argv + 5 + n1, g2, NULL);
    write_BFT(g2, p2, false);
    free_cdbg(g2);

    merging_BFT(p1, p2, pm, 0, false);

    BFT* bft = load_BFT(pm);
    printf("genomes %d\n", bft->nb_genomes);
    for (int i = 0; i < bft->nb_genomes; i++) printf("name %d %s\n", i, bft->filenames[i]);
    FILE* f = fopen(argv[2], "r");
    if (f == NULL) return 2;
    char line[512];
    while (fgets(line, sizeof line, f) != NULL) {
        if (strlen(line) < (size_t)k) continue;
        line[k] = '\0';
        BFT_kmer* bft_kmer = get_kmer(line, bft);
        if (!is_kmer_in_cdbg(bft_kmer)) {
            printf("%s -\n", line);
        } else {
            BFT_annotation* annot = get_annotation(bft_kmer);
            uint32_t* ids = get_list_id_genomes(annot, bft);
            printf("%s ", line);
            for (uint32_t i = 1; i <= ids[0]; i++) printf(i > 1 ? ",%u" : "%u", ids[i]);
            printf("\n");
            free(ids);
            free_BFT_annotation(annot);
        }
        free_BFT_kmer(bft_kmer, 1);
    }
    fclose(f);
    free_cdbg(bft);
    return 0;
}
