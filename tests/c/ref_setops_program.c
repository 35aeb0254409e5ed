/* The annotation set operations (reference include/bft.h:100-114, src/bft.c:421-613) used the way a program of the reference uses them: written against
 * <bft/bft.h> only, linked with -lbft.
 * usage: ref_setops_program k mode groups_file kmer_file...
 *   ops        groups_file holds one group of 1 to 3 stored k-mers per line.  For every group: "in" lines with the annotation of each k-mer as
 *              get_annotation returns it, then each of intersection / union / sym_difference over its first 1, 2, .. members, then results nested as
 *              arguments of further operations.  A line is: tag, size_annot, the bytes in hexadecimal, the count and the ids of get_list_id_genomes.
 *   zero-i | zero-u | zero-s   the operation with nb_annotations == 0: an error
 *   null-i | null-u | null-s   the operation with a NULL annotation as its second argument: an error
 *   helpers    the three byte helpers over a few bytes */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <bft/bft.h>

static void show(const char* tag, BFT_annotation* a, BFT* bft) {
    if (a->annot_ext != NULL || a->annot_cplx != NULL) exit(4);
    printf("%s %d ", tag, a->size_annot);
    for (int i = 0; i < a->size_annot; i++) printf("%02x", a->annot[i]);
    uint32_t* ids = get_list_id_genomes(a, bft);
    printf(" %u", ids[0]);
    for (uint32_t i = 1; i <= ids[0]; i++) printf(" %u", ids[i]);
    printf("\n");
    free(ids);
}

typedef BFT_annotation* (*op_fn)(BFT*, uint32_t, ...);

int main(int argc, char** argv) {
    if (argc < 5) {
        fprintf(stderr, "usage: %s k mode groups_file kmer_file...\n", argv[0]);
        return 2;
    }
    static const char* const names[3] = {"and", "or", "sym"};
    const op_fn ops[3] = {intersection_annotations, union_annotations, sym_difference_annotations};
    const int k = atoi(argv[1]);
    BFT* bft = create_cdbg(k, 0);
    insert_genomes_from_files(argc - 4, argv + 4, bft, NULL);
    if (strcmp(argv[2], "helpers") == 0) {
        printf("%u %u %u\n", intersection_annots(0xF0, 0x3C), union_annots(0xF0, 0x3C), sym_difference_annots(0xF0, 0x3C));
    } else if (strncmp(argv[2], "zero-", 5) == 0 || strncmp(argv[2], "null-", 5) == 0) {
        const op_fn f = ops[argv[2][5] == 'i' ? 0 : argv[2][5] == 'u' ? 1 : 2];
        BFT_annotation* a = create_BFT_annotation();
        a->annot = calloc(1, 1);
        a->size_annot = 1;
        BFT_annotation* r = argv[2][0] == 'z' ? f(bft, 0) : f(bft, 2, a, (BFT_annotation*)NULL);
        show("unreachable", r, bft);
    } else {
        FILE* g = fopen(argv[3], "r");
        if (g == NULL) return 3;
        char line[1024];
        while (fgets(line, sizeof line, g) != NULL) {
            BFT_kmer* km[3];
            BFT_annotation* a[3];
            int n = 0;
            for (char* tok = strtok(line, " \n"); tok != NULL && n < 3; tok = strtok(NULL, " \n")) {
                km[n] = get_kmer(tok, bft);
                a[n] = get_annotation(km[n]);
                show("in", a[n], bft);
                n++;
            }
            char tag[32];
            for (int o = 0; o < 3; o++)
                for (int m = 1; m <= n; m++) {
                    BFT_annotation* r = m == 1 ? ops[o](bft, 1, a[0]) : m == 2 ? ops[o](bft, 2, a[0], a[1]) : ops[o](bft, 3, a[0], a[1], a[2]);
                    sprintf(tag, "%s%d", names[o], m);
                    show(tag, r, bft);
                    free_BFT_annotation(r);
                }
            if (n == 3) { /* results as arguments: (a0 | a1) & a2, (a0 & a1) ^ (a1 | a2) with a stored annotation beside them, and a result of a result */
                BFT_annotation* u = union_annotations(bft, 2, a[0], a[1]);
                BFT_annotation* i = intersection_annotations(bft, 2, a[0], a[1]);
                BFT_annotation* v = union_annotations(bft, 2, a[1], a[2]);
                BFT_annotation* r1 = intersection_annotations(bft, 2, u, a[2]);
                BFT_annotation* r2 = sym_difference_annotations(bft, 3, i, v, a[0]);
                BFT_annotation* r3 = union_annotations(bft, 1, r1);
                show("nest1", r1, bft);
                show("nest2", r2, bft);
                show("nest3", r3, bft);
                free_BFT_annotation(u);
                free_BFT_annotation(i);
                free_BFT_annotation(v);
                free_BFT_annotation(r1);
                free_BFT_annotation(r2);
                free_BFT_annotation(r3);
            }
            for (int j = 0; j < n; j++) {
                free_BFT_annotation(a[j]);
                free_BFT_kmer(km[j], 1);
            }
            printf("end\n");
        }
        fclose(g);
    }
    free_cdbg(bft);
    return 0;
}
