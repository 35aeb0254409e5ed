/* insert_genomes_from_sequence_files (<bft/ingest.h>, an extension of this library) used the way a program of the reference uses <bft/bft.h>:
 * written against the headers only, linked with -lbft.
 * usage: ref_ingest_program k {sequences|sequences_canonical|kmers} min_abundance query_file genome_file...
 *   sequences / sequences_canonical: the genome files are FASTA / FASTQ and go through insert_genomes_from_sequence_files;
 *   kmers: they are k-mer files (one k-mer per line) and go through the reference's insert_genomes_from_files.
 *   prints "genomes <n>", one line "name <id> <name>" per genome, then per k-mer of query_file (one per line)
 *   "<k-mer> <genome id>,<genome id>,..." or "<k-mer> -" when the graph does not hold it. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <bft/bft.h>
#include <bft/ingest.h>

int main(int argc, char** argv) {
    if (argc < 6) {
        fprintf(stderr, "usage: %s k {sequences|sequences_canonical|kmers} min_abundance query_file genome_file...\n", argv[0]);
        return 2;
    }
    const int k = atoi(argv[1]), n_files = argc - 5;
    const uint32_t min_abundance = (uint32_t)strtoul(argv[3], NULL, 10);
    BFT* bft = create_cdbg(k, 0);
    if (strcmp(argv[2], "kmers") == 0) insert_genomes_from_files(n_files, argv + 5, bft, NULL);
    else if (strcmp(argv[2], "sequences") == 0) insert_genomes_from_sequence_files(n_files, argv + 5, 0, min_abundance, bft);
    else if (strcmp(argv[2], "sequences_canonical") == 0) insert_genomes_from_sequence_files(n_files, argv + 5, 1, min_abundance, bft);
    else return 2;
    printf("genomes %d\n", bft->nb_genomes);
    for (int i = 0; i < bft->nb_genomes; i++) printf("name %d %s\n", i, bft->filenames[i]);
    FILE* f = fopen(argv[4], "r");
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
