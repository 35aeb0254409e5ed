/* bft_gaf.h -- the sequences of a FASTA / FASTQ file threaded through the compacted coloured graph of a canonical index (bft_gpu_unitig_graph ->
 * bft_gpu_unitig_segment_of -> bft_gpu_thread_sequences) and written as GAF, for the two host programs that offer it: libbft.so
 * (thread_sequences_to_disk, <bft/unitigs.h>) and the bft_gpu command line (-thread).  Plain C, header only.  One line per walk, in the call's order,
 * the twelve fields of GAF and a cg tag, separated by tabs:
 *   <name>  <sequence length>  <p0>  <p0 + n_w + k - 1>  +  <path: >i or <i per step>  <path length>  <q0>  <q0 + n_w + k - 1>  <matches>  <block length>  255
 *   cg:Z:<matches>=
 * The name is the record's header up to the first blank (bft_seqfile_read_named); the path length is the sum of the steps' segment lengths minus
 * (steps - 1)(k - 1); matches = block length = n_w + k - 1: a walk is an exact match.  Segment ids are those of the GFA file (bft_gfa.h) at the same
 * min_shared; <i reads the reverse complement of the segment as written there. */
#ifndef BFT_GAF_H
#define BFT_GAF_H

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../include/bft_gpu.h"
#include "bft_seqfile.h"

/* Returns 0, a BFT_GPU_E_* code of the library (bft_gpu_last_error has the message), or 1: out of memory, 2: the file could not be written,
 * 3: the sequence file cannot be opened or read, 4: it is neither FASTA nor FASTQ. */
static int bft_gaf_write(bft_gpu* h, int k, uint32_t min_shared, const char* sequence_file, FILE* f) {
    char *blob = NULL, *names = NULL;
    uint64_t *soff = NULL, *noff = NULL, nb_seqs = 0;
    const int rd = bft_seqfile_read_named(sequence_file, &blob, &soff, &names, &noff, &nb_seqs);
    if (rd != BFT_SEQFILE_OK) return rd == BFT_SEQFILE_E_IO ? 3 : 4;
    uint64_t cnt[6], tc[8], info[16];
    uint64_t *seg_off = NULL, *link_off = NULL, *walks = NULL, *walk_off = NULL;
    char* seqs = NULL;
    uint32_t *links = NULL, *members = NULL, *seg_of = NULL, *pos = NULL, *steps = NULL;
    int out = 1;
    int rc = bft_gpu_unitig_graph(h, min_shared, NULL, NULL, NULL, NULL, NULL, 0, 0, 0, 0, cnt);
    if (!rc) rc = bft_gpu_info(h, info, 16); /* (behind the first call: pending insertions are built, info[1] is the number of rows) */
    if (rc) { out = rc; goto done; }
    {
        const uint64_t ns = cnt[0], nc = cnt[1], nl = cnt[4], nm = nc - ns * (uint64_t)(k - 1), n = info[1];
        seg_off = calloc((size_t)ns + 1, 8);
        link_off = calloc(2 * (size_t)ns + 1, 8);
        seqs = malloc((size_t)(nc ? nc : 1));
        links = malloc((size_t)(nl ? nl : 1) * 4);
        members = malloc((size_t)(nm ? nm : 1) * 4);
        seg_of = malloc((size_t)(n ? n : 1) * 4);
        pos = malloc((size_t)(n ? n : 1) * 4);
        if (!seg_off || !link_off || !seqs || !links || !members || !seg_of || !pos) goto done;
        rc = bft_gpu_unitig_graph(h, min_shared, seg_off, seqs, link_off, links, members, ns, nc, nl, nm, cnt);
        if (!rc) rc = bft_gpu_unitig_segment_of(h, members, nm, seg_off, ns, seg_of, pos, n);
        if (!rc) rc = bft_gpu_thread_sequences(h, blob, soff, nb_seqs, seg_of, pos, n, seg_off, ns, link_off, links, nl, NULL, NULL, 0, NULL, 0, tc);
        if (rc) { out = rc; goto done; }
        const uint64_t nw = tc[0], nst = tc[1];
        walks = malloc((size_t)(nw ? nw : 1) * 32);
        walk_off = malloc(((size_t)nw + 1) * 8);
        steps = malloc((size_t)(nst ? nst : 1) * 4);
        if (!walks || !walk_off || !steps) goto done;
        rc = bft_gpu_thread_sequences(h, blob, soff, nb_seqs, seg_of, pos, n, seg_off, ns, link_off, links, nl, walks, walk_off, nw, steps, nst, tc);
        if (rc) { out = rc; goto done; }
        out = 2;
        for (uint64_t w = 0; w < nw; w++) {
            const uint64_t s = walks[4 * w], p0 = walks[4 * w + 1], span = walks[4 * w + 2] + (uint64_t)(k - 1), q0 = walks[4 * w + 3];
            uint64_t plen = 0;
            if (fprintf(f, "%s\t%llu\t%llu\t%llu\t+\t", names + noff[s], (unsigned long long)(soff[s + 1] - soff[s]), (unsigned long long)p0,
                        (unsigned long long)(p0 + span)) < 0)
                goto done;
            for (uint64_t j = walk_off[w]; j < walk_off[w + 1]; j++) {
                const uint32_t x = steps[j];
                plen += seg_off[(x >> 1) + 1] - seg_off[x >> 1] - (j > walk_off[w] ? (uint64_t)(k - 1) : 0);
                if (fprintf(f, "%c%u", x & 1u ? '<' : '>', x >> 1) < 0) goto done;
            }
            if (fprintf(f, "\t%llu\t%llu\t%llu\t%llu\t%llu\t255\tcg:Z:%llu=\n", (unsigned long long)plen, (unsigned long long)q0, (unsigned long long)(q0 + span),
                        (unsigned long long)span, (unsigned long long)span, (unsigned long long)span) < 0)
                goto done;
        }
        out = ferror(f) ? 2 : 0;
    }
done:
    free(blob);
    free(soff);
    free(names);
    free(noff);
    free(seg_off);
    free(link_off);
    free(seqs);
    free(links);
    free(members);
    free(seg_of);
    free(pos);
    free(walks);
    free(walk_off);
    free(steps);
    return out;
}

#endif
