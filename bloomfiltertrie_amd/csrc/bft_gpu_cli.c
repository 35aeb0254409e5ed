/*
 * bft_gpu_cli.c -- host-side C harness over the C-ABI of include/bft_gpu.h, with the command line of the reference's
 * `bft` binary for the hot path (src/main.c:40-47, :180-316):
 *
 *   bft_gpu build k {kmers|kmers_comp|sequences|sequences_canonical} list_genome_files output_file [-min_abundance N]
 *   bft_gpu load file_bft [-add_genomes {kmers|kmers_comp|sequences|sequences_canonical} list_genome_files output_file [-min_abundance N]]
 *                         [-query_kmers {kmers|kmers_comp} list_kmer_files]
 *                         [-query_branching {kmers|kmers_comp} list_kmer_files]
 *                         [-query_sequences threshold {canonical|non_canonical} list_sequence_files]
 *                         [-extract_kmers {kmers|kmers_comp} output_file]
 *                         [-genome_matrix {shared|jaccard|mash} output_file]
 *                         [-unitigs min_shared output_file]
 *                         [-gfa min_shared colors output_file]
 *                         [-bubbles min_shared max_branch_chars output_file]
 *                         [-thread min_shared sequence_file output_file]
 *
 * It is the per-k-mer loops of src/file_io.c:89-213 (build), :651-895 (presence CSV) and :897-1020 (branching)
 * rewired to one batched GPU call per file; file reading, ASCII parsing (parseKmerCount, src/fasta.c:3-53) and CSV
 * formatting stay host C exactly as in the reference, so the outputs are byte-identical:
 *   - CSV name = basename(query file) with its extension replaced by ".csv", in the current directory;
 *   - line 1 = genome names joined by ','; one "0,1,..." line per input line (an all-0 line for a line that is not
 *     a valid k-mer, src/file_io.c:844-850); the final '\n' is overwritten by '\0' (src/file_io.c:873-876);
 *   - stdout: "Nb k-mers present = <n>" (src/main.c:266), "Nb branching k-mers = <n>" (src/main.c:312).
 * An extension: with `sequences` / `sequences_canonical` the listed files are plain-text FASTA or four-line FASTQ and their k-mers are cut on the
 * GPU (bft_gpu_insert_sequence_file); -min_abundance N keeps the k-mers a file holds at least N times.
 * Another: -unitigs writes the canonical (bidirected) unitigs of a canonical index (bft_gpu_unitigs; min_shared 0: every k-mer) as FASTA records
 * `>unitig_<i> length=<L>`, in the call's order.
 * Another: -gfa writes the compacted coloured graph of a canonical index (bft_gpu_unitig_graph: the unitigs, the branching k-mers as segments of their
 * own, the links between them) as GFA 1 (bft_gfa.h); colors 1 adds the union row, the intersection row and the number of genomes of every segment.
 * Another: -bubbles writes the simple bubbles (variants) of that graph (bft_gpu_unitig_bubbles; max_branch_chars 0: no limit) as text, one block per
 * bubble with the genomes of every allele (bft_bubbles_io.h); the segment ids are those of -gfa at the same min_shared.
 * Another: -thread lays the sequences of one FASTA / FASTQ file onto that graph (bft_gpu_thread_sequences: the maximal walks the sequences spell exactly)
 * and writes one GAF line per walk (bft_gaf.h); the segment ids are those of -gfa at the same min_shared.
 * Another: -genome_matrix writes the genome-by-genome shared k-mer matrix (bft_gpu_genome_matrix) as tab-separated text: a header line of the genome
 * names behind an empty first cell, then one line per genome, its name and its row -- the counts (shared, %llu) or the distances computed from
 * them (jaccard, mash: %.6f).
 */
#define _GNU_SOURCE
#include <libgen.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/bft_gpu.h"
#include "bft_bubbles_io.h"
#include "bft_gaf.h"
#include "bft_gfa.h"

#define DIE(...) do { fprintf(stderr, __VA_ARGS__); exit(EXIT_FAILURE); } while (0) /* ERROR(), include/useful_macros.h:33-43 */
static void ck(int rc) { if (rc) DIE("%s\n", bft_gpu_last_error()); }

/* parseKmerCount, src/fasta.c:3-53 */
static int parse_kmer(const char* line, int k, uint8_t* out) {
    for (int j = 0; j < k; j++) {
        uint8_t c;
        switch (line[j]) {
        case 'a': case 'A': c = 0; break;
        case 'c': case 'C': c = 1; break;
        case 'g': case 'G': c = 2; break;
        case 'u': case 'U': case 't': case 'T': c = 3; break;
        default: memset(out, 0, (size_t)((j + 1) / 4)); return 0;
        }
        out[j / 4] |= (uint8_t)(c << (2 * (j % 4)));
    }
    return 1;
}

typedef struct { uint8_t* kmers; uint8_t* valid; uint64_t n_lines, n_kmers; } batch;

/* One k-mer file -> packed batch.  ASCII: one k-mer per line (invalid lines are remembered, they still get a CSV row).
 * kmers_comp: two header lines (k, count) then packed k-mers (src/file_io.c:134-156). */
static batch read_kmer_file(const char* path, int k, int binary) {
    const int nb = (2 * k + 7) / 8;
    batch b = {NULL, NULL, 0, 0};
    FILE* f = fopen(path, "r");
    if (!f) DIE("Cannot open %s\n", path);
    size_t cap = 1 << 16;
    b.kmers = calloc(cap, (size_t)nb);
    b.valid = calloc(cap, 1);
    if (binary) {
        char line[100];
        if (!fgets(line, 100, f) || !fgets(line, 100, f)) DIE("Cannot read header of the file\n");
        for (;;) {
            if (b.n_lines == cap) { cap *= 2; b.kmers = realloc(b.kmers, cap * nb); b.valid = realloc(b.valid, cap); }
            if (fread(b.kmers + b.n_lines * nb, (size_t)nb, 1, f) != 1) break;
            b.valid[b.n_lines++] = 1;
        }
    } else {
        char* line = NULL;
        size_t lcap = 0;
        while (getline(&line, &lcap, f) != -1) {
            if (b.n_lines == cap) {
                b.kmers = realloc(b.kmers, 2 * cap * nb);
                memset(b.kmers + cap * nb, 0, cap * nb);
                b.valid = realloc(b.valid, 2 * cap);
                cap *= 2;
            }
            memset(b.kmers + b.n_lines * nb, 0, (size_t)nb);
            b.valid[b.n_lines] = (uint8_t)(strlen(line) >= (size_t)k && parse_kmer(line, k, b.kmers + b.n_lines * nb));
            b.n_lines++;
        }
        free(line);
    }
    fclose(f);
    for (uint64_t i = 0; i < b.n_lines; i++) b.n_kmers += b.valid[i];
    return b;
}

/* BFT_GPU_DEVICES="0,1,2,...": the -query_kmers / -query_branching batches are sharded over these GPUs of the node, the index replicated
 * on each (bft_gpu_group_*; the reference's loops, src/file_io.c:651-895 and :897-1020, have one BFT_Root).  Unset: the one GPU of `h`. */
static bft_gpu_group* group_from_env(bft_gpu* h) {
    const char* e = getenv("BFT_GPU_DEVICES");
    if (!e || !*e) return NULL;
    int devs[64], n = 0;
    for (const char* p = e; *p && n < 64;) {
        devs[n++] = atoi(p);
        while (*p && *p != ',') p++;
        if (*p == ',') p++;
    }
    if (n < 2 && !(n == 1 && devs[0] != 0)) return NULL;
    bft_gpu_group* g = NULL;
    ck(bft_gpu_group_create(h, 0, devs, n, &g));
    return g;
}

static void query_kmers(bft_gpu* h, const char* path, int k, int binary, uint32_t nb_genomes, char** names) {
    batch b = read_kmer_file(path, k, binary);
    const uint32_t rowbytes = (nb_genomes + 7) / 8;
    uint8_t* present = calloc((b.n_lines + 7) / 8 + 1, 1);
    uint8_t* rows = calloc(b.n_lines ? b.n_lines : 1, rowbytes ? rowbytes : 1);
    bft_gpu_group* grp = group_from_env(h);
    if (grp) {
        ck(bft_gpu_group_query_color_rows(grp, b.kmers, b.n_lines, present, rows));
        bft_gpu_group_free(grp);
    } else
        ck(bft_gpu_query_color_rows(h, b.kmers, b.n_lines, present, rows)); /* invalid lines are all-zero k-mers: masked below */
    char* tmp = strdup(path);
    char* base = basename(tmp);
    char* outname = malloc(strlen(base) + 5);
    strcpy(outname, base);
    char* dot = strrchr(outname, '.');
    if (dot) strcpy(dot, ".csv"); else strcat(outname, ".csv");
    FILE* out = fopen(outname, "w");
    if (!out) DIE("Cannot create %s\n", outname);
    printf("\nQuerying BFT for k-mers in %s\n\n", path);
    for (uint32_t g = 0; g < nb_genomes; g++) fprintf(out, "%s%c", names[g], g + 1 < nb_genomes ? ',' : '\n');
    int nb_present = 0;
    char* line = malloc((size_t)nb_genomes * 2 + 1);
    for (uint64_t i = 0; i < b.n_lines; i++) {
        const int ok = b.valid[i] && ((present[i >> 3] >> (i & 7)) & 1);
        nb_present += ok;
        for (uint32_t g = 0; g < nb_genomes; g++) {
            line[2 * g] = (ok && ((rows[i * rowbytes + (g >> 3)] >> (g & 7)) & 1)) ? '1' : '0';
            line[2 * g + 1] = g + 1 < nb_genomes ? ',' : '\n';
        }
        fwrite(line, 1, (size_t)nb_genomes * 2, out);
    }
    fseek(out, -1L, SEEK_CUR); /* src/file_io.c:873-876 */
    fputc('\0', out);
    fclose(out);
    printf("\nNb k-mers present = %d\n", nb_present);
    free(line); free(outname); free(tmp); free(present); free(rows); free(b.kmers); free(b.valid);
}

static void query_branching(bft_gpu* h, const char* path, int k, int binary) {
    batch b = read_kmer_file(path, k, binary);
    const int nb = (2 * k + 7) / 8;
    /* only valid k-mers are queried (src/file_io.c:963: parseKmerCount(...) == 1) */
    uint64_t m = 0;
    for (uint64_t i = 0; i < b.n_lines; i++)
        if (b.valid[i]) { if (m != i) memmove(b.kmers + m * nb, b.kmers + i * nb, (size_t)nb); m++; }
    uint8_t* bits = calloc((m + 7) / 8 + 1, 1);
    printf("\nQuerying BFT for branching k-mers in %s\n\n", path);
    bft_gpu_group* grp = group_from_env(h);
    if (grp) {
        ck(bft_gpu_group_query_branching(grp, b.kmers, m, bits, NULL));
        bft_gpu_group_free(grp);
    } else
        ck(bft_gpu_query_branching(h, b.kmers, m, bits, NULL));
    int count = 0;
    for (uint64_t i = 0; i < m; i++) count += (bits[i >> 3] >> (i & 7)) & 1;
    printf("\nNb branching k-mers = %d\n", count);
    free(bits); free(b.kmers); free(b.valid);
}

/* query_sequences_outputCSV (src/file_io.c:1464-1574): one sequence per line, one CSV row per line */
static void query_sequences(bft_gpu* h, const char* path, double threshold, int canonical, uint32_t nb_genomes, char** names) {
    FILE* f = fopen(path, "r");
    if (!f) DIE("Cannot open %s\n", path);
    char* blob = NULL;
    size_t blen = 0, bcap = 0, ns = 0, ocap = 1024;
    uint64_t* off = malloc(ocap * sizeof(uint64_t));
    off[0] = 0;
    char* line = NULL;
    size_t lcap = 0;
    while (getline(&line, &lcap, f) != -1) {
        line[strcspn(line, "\r\n")] = 0;
        const size_t l = strlen(line);
        if (blen + l + 1 > bcap) { bcap = (blen + l + 1) * 2; blob = realloc(blob, bcap); }
        memcpy(blob + blen, line, l);
        blen += l;
        if (ns + 2 > ocap) { ocap *= 2; off = realloc(off, ocap * sizeof(uint64_t)); }
        off[++ns] = blen;
    }
    free(line);
    fclose(f);
    if (!blob) blob = calloc(1, 1);
    const uint32_t rowbytes = (nb_genomes + 7) / 8;
    uint8_t* rows = calloc(ns ? ns : 1, rowbytes ? rowbytes : 1);
    ck(bft_gpu_query_sequences(h, blob, off, ns, threshold, canonical, rows));
    char* tmp = strdup(path);
    char* base = basename(tmp);
    char* outname = malloc(strlen(base) + 5);
    strcpy(outname, base);
    char* dot = strrchr(outname, '.');
    if (dot) strcpy(dot, ".csv"); else strcat(outname, ".csv");
    FILE* out = fopen(outname, "w");
    if (!out) DIE("Cannot create %s\n", outname);
    for (uint32_t g = 0; g < nb_genomes; g++) fprintf(out, "%s%c", names[g], g + 1 < nb_genomes ? ',' : '\n');
    char* row = malloc((size_t)nb_genomes * 2 + 1);
    for (size_t i = 0; i < ns; i++) {
        for (uint32_t g = 0; g < nb_genomes; g++) {
            row[2 * g] = ((rows[i * rowbytes + (g >> 3)] >> (g & 7)) & 1) ? '1' : '0';
            row[2 * g + 1] = g + 1 < nb_genomes ? ',' : '\n';
        }
        fwrite(row, 1, (size_t)nb_genomes * 2, out);
    }
    fseek(out, -1L, SEEK_CUR);
    fputc('\0', out);
    fclose(out);
    printf("\nFile %s has been processed.\n", path);
    free(row); free(outname); free(tmp); free(rows); free(off); free(blob);
}

/* file-type word of build / -add_genomes: 0 kmers, 1 kmers_comp, 2 sequences, 3 sequences_canonical (anything else is `kmers`, as before) */
static int genome_file_type(const char* word) {
    if (strcmp(word, "kmers_comp") == 0) return 1;
    if (strcmp(word, "sequences") == 0) return 2;
    if (strcmp(word, "sequences_canonical") == 0) return 3;
    return 0;
}
/* the optional "-min_abundance N" at argv[i]: *used = arguments consumed */
static uint32_t min_abundance_arg(int argc, char** argv, int i, int type, int* used) {
    *used = 0;
    if (i + 1 >= argc || strcmp(argv[i], "-min_abundance") != 0) return 0;
    if (type < 2) DIE("-min_abundance applies to sequences and sequences_canonical only.\n");
    char* end = NULL;
    const long v = strtol(argv[i + 1], &end, 10);
    if (end == argv[i + 1] || *end || v < 0) DIE("Could not parse the count of -min_abundance.\n");
    *used = 2;
    return (uint32_t)v;
}

/* one genome per listed FASTA / FASTQ file, ids in file order: the k-mers are cut on the GPU */
static void insert_sequence_genomes(bft_gpu* h, const char* list_path, int canonical, uint32_t min_abundance) {
    char buffer[2048];
    FILE* lst = fopen(list_path, "r");
    if (!lst) DIE("Invalid list_genome_files.\n");
    while (fgets(buffer, sizeof buffer, lst)) {
        buffer[strcspn(buffer, "\r\n")] = 0;
        if (!buffer[0]) continue;
        uint32_t gid;
        char* tmp = strdup(buffer);
        ck(bft_gpu_add_genome(h, basename(tmp), &gid));
        free(tmp);
        printf("\nFile %u: %s\n\n", gid, buffer);
        ck(bft_gpu_insert_sequence_file(h, buffer, canonical, min_abundance, gid, NULL));
    }
    fclose(lst);
    ck(bft_gpu_build(h));
}

/* insert_Genomes_from_KmerFiles (src/file_io.c:89-213): one genome per listed file, ids in file order */
static void insert_genomes(bft_gpu* h, const char* list_path, int k, int binary) {
    char buffer[2048];
    FILE* lst = fopen(list_path, "r");
    if (!lst) DIE("Invalid list_genome_files.\n");
    while (fgets(buffer, sizeof buffer, lst)) {
        buffer[strcspn(buffer, "\r\n")] = 0;
        if (!buffer[0]) continue;
        uint32_t gid;
        char* tmp = strdup(buffer);
        ck(bft_gpu_add_genome(h, basename(tmp), &gid));
        free(tmp);
        printf("\nFile %u: %s\n\n", gid, buffer);
        batch b = read_kmer_file(buffer, k, binary);
        const int nb = (2 * k + 7) / 8;
        uint64_t m = 0; /* invalid lines are skipped on insertion (src/file_io.c:159) */
        for (uint64_t q = 0; q < b.n_lines; q++)
            if (b.valid[q]) { if (m != q) memmove(b.kmers + m * nb, b.kmers + q * nb, (size_t)nb); m++; }
        ck(bft_gpu_insert_kmers(h, b.kmers, m, gid));
        free(b.kmers); free(b.valid);
    }
    fclose(lst);
    ck(bft_gpu_build(h));
}

/* extract_kmers_to_disk (src/bft.c:255-290): every stored k-mer, ASCII one per line or "k\ncount\n" + packed k-mers.
 * The reference writes them in its trie iteration order; the set is the same, the order here is the image's. */
static void extract_kmers(bft_gpu* h, const char* path, int k, int compressed) {
    uint64_t n = 0;
    ck(bft_gpu_extract(h, NULL, NULL, 0, &n));
    const int nb = (2 * k + 7) / 8;
    uint8_t* km = malloc(n ? n * nb : 1);
    ck(bft_gpu_extract(h, km, NULL, n, &n));
    FILE* f = fopen(path, "w");
    if (!f) DIE("extract_kmers_to_disk(): failed to create/open output file.\n");
    if (compressed) {
        fprintf(f, "%d\n%llu\n", k, (unsigned long long)n);
        fwrite(km, (size_t)nb, n, f);
    } else {
        char* line = malloc((size_t)k + 2);
        for (uint64_t i = 0; i < n; i++) {
            for (int j = 0; j < k; j++) line[j] = "ACGT"[(km[i * nb + j / 4] >> (2 * (j % 4))) & 3];
            line[k] = '\n';
            fwrite(line, 1, (size_t)k + 1, f);
        }
        free(line);
    }
    fclose(f);
    free(km);
}

/* -genome_matrix: S = shared[i][j], n_i the diagonal; jaccard = S / (n_i + n_j - S), 0 for an empty union; mash = -ln(2 J / (1 + J)) / k, capped at
 * 1 and 1 for J = 0 */
static void genome_matrix(bft_gpu* h, const char* what, const char* path, int k, uint32_t nb_names, char** names) {
    const int mode = strcmp(what, "shared") == 0 ? 0 : strcmp(what, "jaccard") == 0 ? 1 : strcmp(what, "mash") == 0 ? 2 : -1;
    if (mode < 0) DIE("Unrecognized type of matrix for -genome_matrix: %s.\n", what);
    uint32_t G = 0;
    ck(bft_gpu_genome_matrix(h, 0, UINT32_MAX, NULL, 0, &G));
    uint64_t* m = calloc((size_t)G * G + 1, 8);
    ck(bft_gpu_genome_matrix(h, 0, UINT32_MAX, m, (uint64_t)G * G, &G));
    FILE* f = fopen(path, "w");
    if (!f) DIE("Cannot create %s\n", path);
    for (uint32_t j = 0; j < G; j++) {
        if (j < nb_names) fprintf(f, "\t%s", names[j]);
        else fprintf(f, "\tgenome_%u", j);
    }
    fputc('\n', f);
    for (uint32_t i = 0; i < G; i++) {
        if (i < nb_names) fputs(names[i], f);
        else fprintf(f, "genome_%u", i);
        for (uint32_t j = 0; j < G; j++) {
            const uint64_t s = m[(size_t)i * G + j];
            if (mode == 0) { fprintf(f, "\t%llu", (unsigned long long)s); continue; }
            const uint64_t un = m[(size_t)i * G + i] + m[(size_t)j * G + j] - s;
            const double jac = un ? (double)s / (double)un : 0.0;
            double d = jac;
            if (mode == 2) {
                d = jac > 0 ? -log(2.0 * jac / (1.0 + jac)) / k : 1.0;
                if (d > 1.0) d = 1.0;
                if (d <= 0) d = 0.0;
            }
            fprintf(f, "\t%.6f", d);
        }
        fputc('\n', f);
    }
    fclose(f);
    free(m);
}

/* -unitigs: one count call, one fetch, FASTA records in the order of bft_gpu_unitigs */
static void unitigs(bft_gpu* h, const char* min_shared, const char* path) {
    char* end = NULL;
    const long t = strtol(min_shared, &end, 10);
    if (end == min_shared || *end || t < 0) DIE("Could not parse min_shared for command -unitigs.\n");
    uint64_t n_paths = 0, n_chars = 0;
    ck(bft_gpu_unitigs(h, (uint32_t)t, NULL, NULL, 0, 0, &n_paths, &n_chars));
    uint64_t* offsets = calloc((size_t)n_paths + 1, 8);
    char* seqs = malloc((size_t)(n_chars ? n_chars : 1));
    if (!offsets || !seqs) DIE("-unitigs: out of memory\n");
    ck(bft_gpu_unitigs(h, (uint32_t)t, offsets, seqs, n_paths, n_chars, &n_paths, &n_chars));
    FILE* f = fopen(path, "w");
    if (!f) DIE("Cannot create %s\n", path);
    for (uint64_t i = 0; i < n_paths; i++) {
        const uint64_t len = offsets[i + 1] - offsets[i];
        fprintf(f, ">unitig_%llu length=%llu\n", (unsigned long long)i, (unsigned long long)len);
        fwrite(seqs + offsets[i], 1, (size_t)len, f);
        fputc('\n', f);
    }
    if (fclose(f) != 0) DIE("Cannot write %s\n", path);
    free(offsets);
    free(seqs);
}

/* -gfa: the compacted graph as GFA 1 (bft_gfa.h) */
static void gfa(bft_gpu* h, const char* min_shared, const char* colors, const char* path, int k) {
    char* end = NULL;
    const long t = strtol(min_shared, &end, 10);
    if (end == min_shared || *end || t < 0) DIE("Could not parse min_shared for command -gfa.\n");
    if (strcmp(colors, "0") != 0 && strcmp(colors, "1") != 0) DIE("colors must be 0 or 1 for command -gfa.\n");
    FILE* f = fopen(path, "w");
    if (!f) DIE("Cannot create %s\n", path);
    const int rc = bft_gfa_write(h, k, (uint32_t)t, colors[0] == '1', f);
    if (rc < 0 || rc == 1) { /* (nothing was written: no empty file stays behind) */
        fclose(f);
        remove(path);
    }
    if (rc < 0) ck(rc);
    if (rc == 1) DIE("-gfa: out of memory\n");
    if (fclose(f) != 0 || rc) DIE("Cannot write %s\n", path);
}

/* -bubbles: the variants of the compacted graph as text (bft_bubbles_io.h) */
static void bubbles(bft_gpu* h, const char* min_shared, const char* max_chars, const char* path, int k) {
    char* end = NULL;
    const long t = strtol(min_shared, &end, 10);
    if (end == min_shared || *end || t < 0) DIE("Could not parse min_shared for command -bubbles.\n");
    const long long mc = strtoll(max_chars, &end, 10);
    if (end == max_chars || *end || mc < 0) DIE("Could not parse max_branch_chars for command -bubbles.\n");
    FILE* f = fopen(path, "w");
    if (!f) DIE("Cannot create %s\n", path);
    const int rc = bft_bubbles_write(h, k, (uint32_t)t, (uint64_t)mc, f);
    if (rc < 0 || rc == 1) { /* (nothing was written: no empty file stays behind) */
        fclose(f);
        remove(path);
    }
    if (rc < 0) ck(rc);
    if (rc == 1) DIE("-bubbles: out of memory\n");
    if (fclose(f) != 0 || rc) DIE("Cannot write %s\n", path);
}

/* -thread: the walks of a file's sequences over the compacted graph as GAF (bft_gaf.h) */
static void thread_sequences(bft_gpu* h, const char* min_shared, const char* seq_path, const char* path, int k) {
    char* end = NULL;
    const long t = strtol(min_shared, &end, 10);
    if (end == min_shared || *end || t < 0) DIE("Could not parse min_shared for command -thread.\n");
    FILE* f = fopen(path, "w");
    if (!f) DIE("Cannot create %s\n", path);
    const int rc = bft_gaf_write(h, k, (uint32_t)t, seq_path, f);
    if (rc < 0 || rc == 1 || rc >= 3) { /* (nothing was written: no empty file stays behind) */
        fclose(f);
        remove(path);
    }
    if (rc < 0) ck(rc);
    if (rc == 1) DIE("-thread: out of memory\n");
    if (rc == 3) DIE("-thread: cannot read %s\n", seq_path);
    if (rc == 4) DIE("-thread: %s is neither FASTA nor FASTQ\n", seq_path);
    if (fclose(f) != 0 || rc) DIE("Cannot write %s\n", path);
}

int main(int argc, char** argv) {
    if (argc >= 2 && (strcmp(argv[1], "--version") == 0 || strcmp(argv[1], "-v") == 0)) { /* src/main.c:51-55 */
        fprintf(stderr, "0.8 (%s)\n", bft_gpu_version());
        return 0;
    }
    if (argc < 3)
        DIE("\nUsage:\n"
            "bft_gpu build k {kmers|kmers_comp|sequences|sequences_canonical} list_genome_files output_file [-min_abundance N]\n"
            "bft_gpu load file_bft [-add_genomes {kmers|kmers_comp|sequences|sequences_canonical} list_genome_files output_file [-min_abundance N]] [Options]\n\nOptions:\n"
            "[-query_kmers {kmers|kmers_comp} list_kmer_files]\n"
            "[-query_branching {kmers|kmers_comp} list_kmer_files]\n"
            "[-query_sequences threshold {canonical|non_canonical} list_sequence_files]\n"
            "[-extract_kmers {kmers|kmers_comp} output_file]\n"
            "[-genome_matrix {shared|jaccard|mash} output_file]\n"
            "[-unitigs min_shared output_file]\n"
            "[-gfa min_shared colors output_file]\n"
            "[-bubbles min_shared max_branch_chars output_file]\n"
            "[-thread min_shared sequence_file output_file]\n\n");
    bft_gpu* h = NULL;
    int k = 0, i = 0;
    char buffer[2048];
    if (strcmp(argv[1], "build") == 0) {
        if (argc < 6) DIE("bft_gpu build k {kmers|kmers_comp} list_genome_files output_file\n");
        k = atoi(argv[2]);
        if (k <= 0) DIE("Provided length k (for k-mers) is either <= 0 or not a number.\n");
        if (k % 9 != 0) DIE("Length k (for k-mers) must be a multiple of 9.\n"); /* src/main.c:63 */
        const int type = genome_file_type(argv[3]);
        int used = 0;
        const uint32_t min_abundance = min_abundance_arg(argc, argv, 6, type, &used);
        ck(bft_gpu_create(k, 0, &h));
        if (type >= 2) insert_sequence_genomes(h, argv[4], type == 3, min_abundance);
        else insert_genomes(h, argv[4], k, type == 1);
        ck(bft_gpu_write_bft(h, argv[5]));
        i = 6 + used;
    } else if (strcmp(argv[1], "load") == 0) {
        ck(bft_gpu_load_bft(argv[2], 0, &h));
        i = 3;
        if (i + 3 < argc && strcmp(argv[i], "-add_genomes") == 0) { /* src/main.c:217-246 */
            uint64_t inf[16];
            ck(bft_gpu_info(h, inf, 16));
            const int type = genome_file_type(argv[i + 1]);
            int used = 0;
            const uint32_t min_abundance = min_abundance_arg(argc, argv, i + 4, type, &used);
            if (type >= 2) insert_sequence_genomes(h, argv[i + 2], type == 3, min_abundance);
            else insert_genomes(h, argv[i + 2], (int)inf[0], type == 1);
            ck(bft_gpu_write_bft(h, argv[i + 3]));
            i += 4 + used;
        }
    } else
        DIE("Unrecognized command %s.\n", argv[1]);

    uint64_t info[16];
    ck(bft_gpu_info(h, info, 16));
    k = (int)info[0];
    const uint32_t nb_genomes = (uint32_t)info[11];
    char** names = calloc(nb_genomes ? nb_genomes : 1, sizeof(char*));
    for (uint32_t g = 0; g < nb_genomes; g++) {
        names[g] = malloc(4096);
        ck(bft_gpu_genome_name(h, g, names[g], 4096));
    }
    for (; i + 2 < argc; i += 3) {
        if (strcmp(argv[i], "-query_sequences") == 0) { /* src/main.c:270-296: four arguments */
            if (i + 3 >= argc) DIE("-query_sequences threshold {canonical|non_canonical} list_sequence_files\n");
            const double threshold = atof(argv[i + 1]);
            if (threshold == 0) DIE("Could not parse threshold for command -query_sequences.\n");
            if (strcmp(argv[i + 2], "canonical") != 0 && strcmp(argv[i + 2], "non_canonical") != 0)
                DIE("Unrecognized type of k-mers to search for %s.\n", argv[i]);
            FILE* lst = fopen(argv[i + 3], "r");
            if (!lst) DIE("Invalid sequence query file list.\n");
            while (fgets(buffer, sizeof buffer, lst)) {
                buffer[strcspn(buffer, "\r\n")] = 0;
                if (buffer[0]) query_sequences(h, buffer, threshold, strcmp(argv[i + 2], "canonical") == 0, nb_genomes, names);
            }
            fclose(lst);
            i++;
            continue;
        }
        if (strcmp(argv[i], "-genome_matrix") == 0) { genome_matrix(h, argv[i + 1], argv[i + 2], k, nb_genomes, names); continue; }
        if (strcmp(argv[i], "-unitigs") == 0) { unitigs(h, argv[i + 1], argv[i + 2]); continue; }
        if (strcmp(argv[i], "-gfa") == 0) { /* four arguments */
            if (i + 3 >= argc) DIE("-gfa min_shared colors output_file\n");
            gfa(h, argv[i + 1], argv[i + 2], argv[i + 3], k);
            i++;
            continue;
        }
        if (strcmp(argv[i], "-bubbles") == 0) { /* four arguments */
            if (i + 3 >= argc) DIE("-bubbles min_shared max_branch_chars output_file\n");
            bubbles(h, argv[i + 1], argv[i + 2], argv[i + 3], k);
            i++;
            continue;
        }
        if (strcmp(argv[i], "-thread") == 0) { /* four arguments */
            if (i + 3 >= argc) DIE("-thread min_shared sequence_file output_file\n");
            thread_sequences(h, argv[i + 1], argv[i + 2], argv[i + 3], k);
            i++;
            continue;
        }
        const int binary = strcmp(argv[i + 1], "kmers_comp") == 0;
        if (!binary && strcmp(argv[i + 1], "kmers") != 0) DIE("Unrecognized type of input files for %s.\n", argv[i]);
        if (strcmp(argv[i], "-extract_kmers") == 0) { extract_kmers(h, argv[i + 2], k, binary); continue; }
        FILE* lst = fopen(argv[i + 2], "r");
        if (!lst) DIE("Invalid k-mer queries files list.\n");
        while (fgets(buffer, sizeof buffer, lst)) {
            buffer[strcspn(buffer, "\r\n")] = 0;
            if (!buffer[0]) continue;
            if (strcmp(argv[i], "-query_kmers") == 0) query_kmers(h, buffer, k, binary, nb_genomes, names);
            else if (strcmp(argv[i], "-query_branching") == 0) query_branching(h, buffer, k, binary);
            else DIE("Unrecognized command %s.\n", argv[i]);
        }
        fclose(lst);
    }
    bft_gpu_free(h);
    return 0;
}
