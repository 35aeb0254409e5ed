/* seqfile_main.c -- a stand-alone program around the FASTA / FASTQ reader (csrc/bft_seqfile.cpp), for tests/test_ingest_cases_host.py, which also
 * builds it with -fsanitize=address,undefined.  Usage: seqfile_main file.  Prints "rc n" and then one line "length:sequence" per sequence. */
#include <stdio.h>
#include <stdlib.h>

#include "bft_seqfile.h"

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s file\n", argv[0]);
        return 2;
    }
    char* blob = NULL;
    uint64_t* off = NULL;
    uint64_t n = 0;
    const int rc = bft_seqfile_read(argv[1], &blob, &off, &n);
    printf("%d %llu\n", rc, (unsigned long long)n);
    if (rc == BFT_SEQFILE_OK) {
        for (uint64_t i = 0; i < n; i++) {
            printf("%llu:", (unsigned long long)(off[i + 1] - off[i]));
            fwrite(blob + off[i], 1, (size_t)(off[i + 1] - off[i]), stdout);
            fputc('\n', stdout);
        }
        bft_seqfile_free(blob, off);
    } else if (blob != NULL || off != NULL || n != 0) {
        return 3; /* an error must leave nothing behind */
    }
    return 0;
}
