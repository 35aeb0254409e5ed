/* bft_gfa.h -- the compacted coloured graph of a canonical index (bft_gpu_unitig_graph, bft_gpu_unitig_colors) written as GFA 1, for the two host
 * programs that offer it: libbft.so (extract_unitig_graph_to_disk, <bft/unitigs.h>) and the bft_gpu command line (-gfa).  Plain C, header only.
 *   H  VN:Z:1.0  kl:i:<k>
 *   S  <i>  <sequence>  LN:i:<length>  [cu:H:<union row>  ci:H:<intersection row>  gc:i:<genomes in the union>]     one per segment, in order
 *   L  <i>  <+|->  <j>  <+|->  <k-1>M                                                  one per entry of the link lists, in their order (both mirror forms)
 * A colour row is CEIL(nb_genomes / 8) bytes, bit g % 8 of byte g / 8 = genome g, two upper-case hexadecimal digits per byte (the H type of GFA). */
#ifndef BFT_GFA_H
#define BFT_GFA_H

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../include/bft_gpu.h"

/* Returns 0, a BFT_GPU_E_* code of the library (bft_gpu_last_error has the message), or 1: out of memory, 2: the file could not be written. */
static int bft_gfa_write(bft_gpu* h, int k, uint32_t min_shared, int colors, FILE* f) {
    uint64_t cnt[6], info[16];
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
    uint8_t *cu = NULL, *ci = NULL;
    uint32_t* gc = NULL;
    int out = 1;
    if (!seg_off || !link_off || !seqs || !links || !members) goto done;
    rc = bft_gpu_unitig_graph(h, min_shared, seg_off, seqs, link_off, links, members, ns, nc, nl, nm, cnt);
    if (rc) { out = rc; goto done; }
    if (colors && ns) {
        cu = malloc((size_t)ns * (rb ? rb : 1));
        ci = malloc((size_t)ns * (rb ? rb : 1));
        gc = malloc((size_t)ns * 4);
        if (!cu || !ci || !gc) goto done;
        rc = bft_gpu_unitig_colors(h, members, nm, seg_off, ns, BFT_GPU_SETOP_OR, cu, gc);
        if (!rc) rc = bft_gpu_unitig_colors(h, members, nm, seg_off, ns, BFT_GPU_SETOP_AND, ci, NULL);
        if (rc) { out = rc; goto done; }
    }
    out = 2;
    if (fprintf(f, "H\tVN:Z:1.0\tkl:i:%d\n", k) < 0) goto done;
    for (uint64_t i = 0; i < ns; i++) {
        const uint64_t len = seg_off[i + 1] - seg_off[i];
        if (fprintf(f, "S\t%llu\t", (unsigned long long)i) < 0 || fwrite(seqs + seg_off[i], 1, (size_t)len, f) != len ||
            fprintf(f, "\tLN:i:%llu", (unsigned long long)len) < 0)
            goto done;
        if (colors) {
            fputs("\tcu:H:", f);
            for (uint32_t b = 0; b < rb; b++) fprintf(f, "%02X", cu[i * rb + b]);
            fputs("\tci:H:", f);
            for (uint32_t b = 0; b < rb; b++) fprintf(f, "%02X", ci[i * rb + b]);
            fprintf(f, "\tgc:i:%u", gc[i]);
        }
        if (fputc('\n', f) == EOF) goto done;
    }
    for (uint64_t a = 0; a < 2 * ns; a++)
        for (uint64_t j = link_off[a]; j < link_off[a + 1]; j++)
            if (fprintf(f, "L\t%llu\t%c\t%u\t%c\t%dM\n", (unsigned long long)(a >> 1), a & 1 ? '-' : '+', links[j] >> 1, links[j] & 1u ? '-' : '+', k - 1) < 0) goto done;
    out = ferror(f) ? 2 : 0;
done:
    free(seg_off);
    free(link_off);
    free(seqs);
    free(links);
    free(members);
    free(cu);
    free(ci);
    free(gc);
    return out;
}

#endif
