/* bft_bubbles_io.h -- the simple bubbles (variants) of a canonical index (bft_gpu_unitig_graph -> bft_gpu_unitig_bubbles -> bft_gpu_unitig_colors)
 * written as text, for the two host programs that offer it: libbft.so (extract_bubbles_to_disk, <bft/unitigs.h>) and the bft_gpu command line
 * (-bubbles).  Plain C, header only.  One block per bubble, in the call's order, fields separated by tabs:
 *   B  <index>  <source id><+|->  <sink id><+|->  <m>                                        the bubble: its number, source, sink, branches
 *   A  <segment id><+|->  <sequence in that orientation>  <number of genomes>  <genome ids>  one per branch, in the source's link order
 * The genomes of a branch are its AND row: the genomes that hold every k-mer of the allele, ascending, separated by commas (none: an empty field).
 * Segment ids are those of the GFA file (bft_gfa.h) at the same min_shared; - is the reverse complement of the segment as written there. */
#ifndef BFT_BUBBLES_IO_H
#define BFT_BUBBLES_IO_H

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../include/bft_gpu.h"

/* Returns 0, a BFT_GPU_E_* code of the library (bft_gpu_last_error has the message), or 1: out of memory, 2: the file could not be written. */
static int bft_bubbles_write(bft_gpu* h, int k, uint32_t min_shared, uint64_t max_branch_chars, FILE* f) {
    uint64_t cnt[6], bcnt[4], info[16], nb = 0;
    int rc = bft_gpu_unitig_graph(h, min_shared, NULL, NULL, NULL, NULL, NULL, 0, 0, 0, 0, cnt);
    if (!rc) rc = bft_gpu_info(h, info, 16); /* (behind the first call: pending insertions are built, info[11] is the width of the colour rows) */
    if (rc) return rc;
    const uint32_t nb_genomes = (uint32_t)info[11];
    const uint64_t ns = cnt[0], nc = cnt[1], nl = cnt[4], nm = nc - ns * (uint64_t)(k - 1);
    const uint32_t rb = (nb_genomes + 7) / 8;
    uint64_t* seg_off = calloc((size_t)ns + 1, 8);
    uint64_t* link_off = calloc(2 * (size_t)ns + 1, 8);
    char* seqs = malloc((size_t)(nc ? nc : 1));
    uint32_t* links = malloc((size_t)(nl ? nl : 1) * 4);
    uint32_t* members = malloc((size_t)(nm ? nm : 1) * 4);
    uint32_t* recs = NULL;
    uint8_t* rows = NULL;
    int out = 1;
    if (!seg_off || !link_off || !seqs || !links || !members) goto done;
    rc = bft_gpu_unitig_graph(h, min_shared, seg_off, seqs, link_off, links, members, ns, nc, nl, nm, cnt);
    if (!rc) rc = bft_gpu_unitig_bubbles(h, seg_off, seqs, link_off, links, ns, nl, max_branch_chars, NULL, 0, bcnt);
    if (rc) { out = rc; goto done; }
    nb = bcnt[0];
    if (nb) {
        recs = malloc((size_t)nb * 24);
        rows = malloc((size_t)ns * (rb ? rb : 1));
        if (!recs || !rows) goto done;
        rc = bft_gpu_unitig_bubbles(h, seg_off, seqs, link_off, links, ns, nl, max_branch_chars, recs, nb, bcnt);
        if (!rc) rc = bft_gpu_unitig_colors(h, members, nm, seg_off, ns, BFT_GPU_SETOP_AND, rows, NULL);
        if (rc) { out = rc; goto done; }
    }
    out = 2;
    for (uint64_t i = 0; i < nb; i++) {
        const uint32_t* r = recs + 6 * i;
        int m = 0;
        while (m < 4 && r[2 + m] != 0xFFFFFFFFu) m++;
        if (fprintf(f, "B\t%llu\t%u%c\t%u%c\t%d\n", (unsigned long long)i, r[0] >> 1, r[0] & 1u ? '-' : '+', r[1] >> 1, r[1] & 1u ? '-' : '+', m) < 0) goto done;
        for (int j = 0; j < m; j++) {
            const uint32_t b = r[2 + j], s = b >> 1;
            const uint64_t lo = seg_off[s], len = seg_off[s + 1] - lo;
            if (fprintf(f, "A\t%u%c\t", s, b & 1u ? '-' : '+') < 0) goto done;
            if (b & 1u) { /* the reverse complement */
                for (uint64_t c = len; c-- > 0;) {
                    const char x = seqs[lo + c];
                    fputc(x == 'A' ? 'T' : x == 'C' ? 'G' : x == 'G' ? 'C' : 'A', f);
                }
            } else if (fwrite(seqs + lo, 1, (size_t)len, f) != len)
                goto done;
            uint32_t n = 0;
            for (uint32_t g = 0; g < nb_genomes; g++) n += rows[(size_t)s * rb + (g >> 3)] >> (g & 7u) & 1u;
            fprintf(f, "\t%u\t", n);
            for (uint32_t g = 0, first = 1; g < nb_genomes; g++)
                if (rows[(size_t)s * rb + (g >> 3)] >> (g & 7u) & 1u) {
                    fprintf(f, first ? "%u" : ",%u", g);
                    first = 0;
                }
            if (fputc('\n', f) == EOF) goto done;
        }
    }
    out = ferror(f) ? 2 : 0;
done:
    free(seg_off);
    free(link_off);
    free(seqs);
    free(links);
    free(members);
    free(recs);
    free(rows);
    return out;
}

#endif
