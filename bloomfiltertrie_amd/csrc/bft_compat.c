/*
 * bft_compat.c -- host-side C layer that serves the reference's public API (<bft/bft.h>, include/bft/bft.h here) from
 * the C-ABI of include/bft_gpu.h.  Built as libbft.so so that a program of the reference links with `-lbft` as
 * README.md:91-111 says.  Nothing is computed here: every lookup, colour-set decode, neighbour test and sequence query
 * is a (small) batch handed to libbft_gpu.so; this file only converts between the reference's objects (BFT_kmer,
 * BFT_annotation, uint32_t id lists with the count in [0]) and the batch layouts, and keeps the reference's
 * exit-on-error behaviour (ERROR(), include/useful_macros.h:33-43).
 */
#define _GNU_SOURCE
#include <libgen.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/bft/bft.h"
#include "../../include/bft/ingest.h"
#include "../../include/bft/merge.h"
#include "../../include/bft/snippets.h"
#include "../../include/bft/unitigs.h"
#include "bft_bubbles_io.h"
#include "bft_gaf.h"
#include "bft_gfa.h"

#define DIE(...) do { fprintf(stderr, __VA_ARGS__); exit(EXIT_FAILURE); } while (0)
#define NOT_NULL(p, where) do { if ((p) == NULL) DIE("%s: NULL pointer\n", where); } while (0)
#define ABSENT 0xFFFFFFFFu

static void ck(int rc, const char* where) {
    if (rc != BFT_GPU_OK) DIE("%s: %s\n", where, bft_gpu_last_error());
}

static int bytes_of(int k) { return (2 * k + 7) / 8; }

/* parseKmerCount (src/fasta.c:3-53): 1 if the first k characters are all in ACGTU (either case) */
static int pack_kmer(const char* s, int k, uint8_t* out) {
    memset(out, 0, (size_t)bytes_of(k));
    for (int j = 0; j < k; j++) {
        unsigned c;
        switch (s[j]) {
        case 'a': case 'A': c = 0; break;
        case 'c': case 'C': c = 1; break;
        case 'g': case 'G': c = 2; break;
        case 't': case 'T': case 'u': case 'U': c = 3; break;
        default: memset(out, 0, (size_t)bytes_of(k)); return 0;
        }
        out[j >> 2] |= (uint8_t)(c << (2 * (j & 3)));
    }
    return 1;
}

static void unpack_kmer(const uint8_t* in, int k, char* s) { /* kmer_comp_to_ascii, src/fasta.c:55-87 */
    for (int j = 0; j < k; j++) s[j] = "ACGT"[(in[j >> 2] >> (2 * (j & 3))) & 3];
    s[k] = '\0';
}

/* ---------------------------------------------------------------- graph */

static int device_from_env(void) {
    const char* d = getenv("BFT_GPU_DEVICE");
    return d ? atoi(d) : 0;
}

static BFT* new_root(int k, int treshold_compression, bft_gpu* g) {
    BFT* bft = calloc(1, sizeof(BFT));
    NOT_NULL(bft, "createBFT_Root()");
    bft->k = k;
    bft->treshold_compression = treshold_compression;
    bft->gpu = g;
    return bft;
}

static void push_name(BFT* bft, const char* name) { /* add_genomes_BFT_Root, include/CC.h:307-338 */
    bft->filenames = realloc(bft->filenames, (size_t)(bft->nb_genomes + 1) * sizeof(char*));
    NOT_NULL(bft->filenames, "add_genomes_BFT_Root()");
    bft->filenames[bft->nb_genomes] = strdup(name);
    NOT_NULL(bft->filenames[bft->nb_genomes], "add_genomes_BFT_Root()");
    bft->nb_genomes++;
}

BFT* create_cdbg(int k, int treshold_compression) {
    if (k <= 0 || k % 9 != 0) DIE("create_cdbg(): k must be a positive multiple of 9.\n"); /* src/main.c:61-63 */
    bft_gpu* g = NULL;
    ck(bft_gpu_create(k, device_from_env(), &g), "create_cdbg()");
    return new_root(k, treshold_compression, g);
}

void free_cdbg(BFT* bft) {
    if (bft == NULL) return;
    for (int i = 0; i < bft->nb_genomes; i++) free(bft->filenames[i]);
    free(bft->filenames);
    free(bft->marks);
    bft_gpu_free(bft->gpu);
    free(bft);
}

bft_gpu* bft_device_index(BFT* bft) {
    NOT_NULL(bft, "bft_device_index()");
    return bft->gpu;
}

static uint32_t new_genome(BFT* bft, const char* name) {
    uint32_t gid = 0;
    ck(bft_gpu_add_genome(bft->gpu, name, &gid), "add_genomes_BFT_Root()");
    push_name(bft, name);
    return gid;
}

static void insert_strings(int nb_kmers, char** kmers, uint32_t gid, BFT* bft, const char* where) {
    if (nb_kmers <= 0) return;
    NOT_NULL(kmers, where);
    const int nb = bytes_of(bft->k);
    uint8_t* batch = malloc((size_t)nb_kmers * (size_t)nb);
    NOT_NULL(batch, where);
    for (int i = 0; i < nb_kmers; i++)
        if (kmers[i] == NULL || strlen(kmers[i]) < (size_t)bft->k || !pack_kmer(kmers[i], bft->k, batch + (size_t)i * nb))
            DIE("%s: could not insert k-mer in graph, it probably contains unvalid characters.\n", where); /* src/bft.c:67 */
    ck(bft_gpu_insert_kmers(bft->gpu, batch, (uint64_t)nb_kmers, gid), where);
    free(batch);
}

void insert_kmers_new_genome(int nb_kmers, char** kmers, char* genome_name, BFT* bft) {
    NOT_NULL(bft, "insert_kmers_new_genome()");
    NOT_NULL(genome_name, "insert_kmers_new_genome()");
    insert_strings(nb_kmers, kmers, new_genome(bft, genome_name), bft, "insert_kmers_new_genome()");
}

void insert_kmers_last_genome(int nb_kmers, char** kmers, BFT* bft) {
    NOT_NULL(bft, "insert_kmers_last_genome()");
    if (bft->nb_genomes <= 0) DIE("insert_kmers_last_genome(): the graph is empty, there is no last genome.\n");
    insert_strings(nb_kmers, kmers, (uint32_t)bft->nb_genomes - 1, bft, "insert_kmers_last_genome()");
}

/* insert_Genomes_from_KmerFiles with binary_files = 0 (src/bft.c:31-37, src/file_io.c:89-213): lines that are not a
 * k-mer are skipped; the whole file goes to the GPU as one batch. */
void insert_genomes_from_files(int nb_files, char** paths, BFT* bft, char* prefix_bft_filename) {
    (void)prefix_bft_filename; /* only used by the reference's colour compression */
    NOT_NULL(bft, "insert_genomes_from_files()");
    if (nb_files > 0) NOT_NULL(paths, "insert_genomes_from_files()");
    const int nb = bytes_of(bft->k);
    for (int i = 0; i < nb_files; i++) {
        NOT_NULL(paths[i], "insert_genomes_from_files()");
        char* tmp = strdup(paths[i]);
        const uint32_t gid = new_genome(bft, basename(tmp));
        free(tmp);
        FILE* f = fopen(paths[i], "r");
        if (f == NULL) DIE("insert_Genomes_from_KmerFiles(): cannot open %s\n", paths[i]);
        size_t cap = 1 << 16, n = 0;
        uint8_t* batch = malloc(cap * (size_t)nb);
        NOT_NULL(batch, "insert_genomes_from_files()");
        char* line = NULL;
        size_t lcap = 0;
        while (getline(&line, &lcap, f) != -1) {
            if (n == cap) {
                cap *= 2;
                batch = realloc(batch, cap * (size_t)nb);
                NOT_NULL(batch, "insert_genomes_from_files()");
            }
            if (strlen(line) >= (size_t)bft->k && pack_kmer(line, bft->k, batch + n * (size_t)nb)) n++;
        }
        free(line);
        fclose(f);
        ck(bft_gpu_insert_kmers(bft->gpu, batch, (uint64_t)n, gid), "insert_genomes_from_files()");
        free(batch);
    }
    ck(bft_gpu_build(bft->gpu), "insert_genomes_from_files()");
}

/* <bft/ingest.h>: one genome per FASTA / FASTQ file, its k-mers cut (and counted) on the GPU */
void insert_genomes_from_sequence_files(int nb_files, char** paths, int canonical, uint32_t min_abundance, BFT_Root* root) {
    NOT_NULL(root, "insert_genomes_from_sequence_files()");
    if (nb_files > 0) NOT_NULL(paths, "insert_genomes_from_sequence_files()");
    for (int i = 0; i < nb_files; i++) {
        NOT_NULL(paths[i], "insert_genomes_from_sequence_files()");
        char* tmp = strdup(paths[i]);
        const uint32_t gid = new_genome(root, basename(tmp));
        free(tmp);
        ck(bft_gpu_insert_sequence_file(root->gpu, paths[i], canonical, min_abundance, gid, NULL), "insert_genomes_from_sequence_files()");
    }
    ck(bft_gpu_build(root->gpu), "insert_genomes_from_sequence_files()");
}

/* ---------------------------------------------------------------- k-mers */

static resultPresence* new_res(BFT* bft, int present, uint32_t row, uint32_t colorset) {
    resultPresence* r = malloc(sizeof(resultPresence));
    NOT_NULL(r, "create_resultPresence()");
    r->link_child = present ? (void*)bft : NULL;
    r->bft = bft;
    r->row = present ? row : ABSENT;
    r->colorset = present ? colorset : ABSENT;
    return r;
}

static void fill_kmer(BFT_kmer* km, const char* ascii, int k) {
    km->kmer = malloc((size_t)k + 1);
    km->kmer_comp = malloc((size_t)bytes_of(k));
    if (km->kmer == NULL || km->kmer_comp == NULL) DIE("create_kmer(): out of memory\n");
    memcpy(km->kmer, ascii, (size_t)k);
    km->kmer[k] = '\0';
    km->res = NULL;
}

BFT_kmer* create_kmer(const char* kmer, int k) {
    NOT_NULL(kmer, "create_kmer()");
    if (strlen(kmer) != (size_t)k) DIE("create_kmer(): k-mer length is not the one used in the graph.\n");
    BFT_kmer* km = malloc(sizeof(BFT_kmer));
    NOT_NULL(km, "create_kmer()");
    fill_kmer(km, kmer, k);
    if (!pack_kmer(km->kmer, k, km->kmer_comp)) DIE("create_kmer(): Unexpected character encountered in k-mer.\n");
    km->res = new_res(NULL, 0, ABSENT, ABSENT);
    return km;
}

BFT_kmer* create_empty_kmer(void) {
    BFT_kmer* km = malloc(sizeof(BFT_kmer));
    NOT_NULL(km, "create_empty_kmer()");
    km->kmer = NULL;
    km->kmer_comp = NULL;
    km->res = NULL;
    return km;
}

void free_BFT_kmer_content(BFT_kmer* bft_kmer, int nb_bft_kmer) {
    NOT_NULL(bft_kmer, "free_BFT_kmer_content()");
    for (int i = 0; i < nb_bft_kmer; i++) {
        free(bft_kmer[i].kmer);
        free(bft_kmer[i].kmer_comp);
        free(bft_kmer[i].res);
    }
}

void free_BFT_kmer(BFT_kmer* bft_kmer, int nb_bft_kmer) {
    NOT_NULL(bft_kmer, "free_BFT_kmer()");
    free_BFT_kmer_content(bft_kmer, nb_bft_kmer);
    free(bft_kmer);
}

/* One batch of packed k-mers -> their resultPresence (isKmerPresent for each, src/presenceNode.c:1823-1921). */
static void locate(BFT* bft, const uint8_t* packed, int n, BFT_kmer* out, const char* where) {
    uint8_t bits[8] = {0};
    uint32_t rows[64], sets[64];
    ck(bft_gpu_query_rows(bft->gpu, packed, (uint64_t)n, bits, rows, sets), where);
    for (int i = 0; i < n; i++) out[i].res = new_res(bft, (bits[i >> 3] >> (i & 7)) & 1, rows[i], sets[i]);
}

BFT_kmer* get_kmer(const char* kmer, BFT* bft) {
    NOT_NULL(kmer, "get_kmer()");
    NOT_NULL(bft, "get_kmer()");
    if (strlen(kmer) < (size_t)bft->k) DIE("get_kmer(): Unexpected character encountered in k-mer.\n");
    BFT_kmer* km = malloc(sizeof(BFT_kmer));
    NOT_NULL(km, "get_kmer()");
    fill_kmer(km, kmer, bft->k);
    if (!pack_kmer(km->kmer, bft->k, km->kmer_comp)) DIE("get_kmer(): Unexpected character encountered in k-mer.\n");
    locate(bft, km->kmer_comp, 1, km, "get_kmer()");
    return km;
}

bool is_kmer_in_cdbg(BFT_kmer* bft_kmer) {
    NOT_NULL(bft_kmer, "is_kmer_in_cdbg()");
    NOT_NULL(bft_kmer->res, "is_kmer_in_cdbg()");
    return bft_kmer->res->link_child != NULL;
}

/* ---------------------------------------------------------------- the harness seam (src/file_io.c loops) */

int parseKmerCount(const char* line, int size_kmer, uint8_t* tab, int pos_tab) { /* src/fasta.c:3-53 */
    NOT_NULL(line, "parseKmerCount()");
    NOT_NULL(tab, "parseKmerCount()");
    uint8_t* t = tab + pos_tab;
    int j = 0;
    for (; j < size_kmer; j++) {
        unsigned c;
        switch (line[j]) {
        case 'a': case 'A': c = 0; break;
        case 'c': case 'C': c = 1; break;
        case 'g': case 'G': c = 2; break;
        case 't': case 'T': case 'u': case 'U': c = 3; break;
        default: /* IUPAC codes, end of line, anything else: the bytes touched so far are cleared (:49) */
            memset(t, 0, (size_t)((j + 1) / 4));
            return 0;
        }
        t[j >> 2] |= (uint8_t)(c << (2 * (j & 3)));
    }
    return 1;
}

void kmer_comp_to_ascii(const uint8_t* kmer_comp, int k, char* kmer) {
    NOT_NULL(kmer_comp, "kmer_comp_to_ascii()");
    NOT_NULL(kmer, "kmer_comp_to_ascii()");
    unpack_kmer(kmer_comp, k, kmer);
}

int get_nb_bytes_power2_annot(uint32_t pos) { /* include/log2.h:45-50: CEIL(bits needed for pos, 6), 1 for pos = 0 */
    const int bits = pos ? 32 - __builtin_clz(pos) : 1;
    return (bits + 5) / 6;
}

void add_genomes_BFT_Root(int nb_files, char** filenames, BFT_Root* root) { /* include/CC.h:307-338 */
    NOT_NULL(root, "add_genomes_BFT_Root()");
    if (nb_files < 0) DIE("add_genomes_BFT_Root(): the number of genomes to insert cannot be less than 0.\n");
    if (nb_files > 0) NOT_NULL(filenames, "add_genomes_BFT_Root()");
    for (int i = 0; i < nb_files; i++) {
        NOT_NULL(filenames[i], "add_genomes_BFT_Root()");
        new_genome(root, filenames[i]);
    }
}

void insertKmers(BFT_Root* root, uint8_t* array_kmers, int nb_kmers, uint32_t id_genome, int size_id_genome) {
    (void)size_id_genome; /* width of the id inside the reference's annotation bytes: the colour sets here are id lists */
    NOT_NULL(root, "insertKmers()");
    if (nb_kmers <= 0) return;
    NOT_NULL(array_kmers, "insertKmers()");
    ck(bft_gpu_insert_kmers(root->gpu, array_kmers, (uint64_t)nb_kmers, id_genome), "insertKmers()");
}

resultPresence* isKmerPresent(Node* node, BFT_Root* root, int lvl_node, uint8_t* kmer, int size_kmer) {
    NOT_NULL(root, "isKmerPresent()");
    NOT_NULL(kmer, "isKmerPresent()");
    if ((node != NULL && node != &root->node) || size_kmer != root->k || lvl_node != root->k / 9 - 1)
        DIE("isKmerPresent(): only whole k-mers from the root vertex (&root->node, level k/9-1, size k) can be looked up.\n");
    BFT_kmer tmp;
    locate(root, kmer, 1, &tmp, "isKmerPresent()");
    return tmp.res;
}

/* ---------------------------------------------------------------- annotations */

BFT_annotation* create_BFT_annotation(void) {
    BFT_annotation* a = malloc(sizeof(BFT_annotation));
    NOT_NULL(a, "create_BFT_annotation()");
    a->annot = a->annot_ext = a->annot_cplx = NULL;
    a->size_annot = a->size_annot_cplx = -1;
    a->from_BFT = 0;
    return a;
}

void free_BFT_annotation(BFT_annotation* bft_annot) {
    NOT_NULL(bft_annot, "free_BFT_annotation()");
    /* the reference's from_BFT annotations alias the trie; here the bytes are always a private copy */
    free(bft_annot->annot);
    free(bft_annot->annot_ext);
    free(bft_annot->annot_cplx);
    free(bft_annot);
}

BFT_annotation* get_annotation(BFT_kmer* bft_kmer) {
    NOT_NULL(bft_kmer, "get_annotation()");
    if (!is_kmer_in_cdbg(bft_kmer)) DIE("get_annotation(): k-mer is not present in the graph.\n");
    BFT* bft = bft_kmer->res->bft;
    uint32_t n = 0;
    ck(bft_gpu_colorset_annot(bft->gpu, bft_kmer->res->colorset, NULL, 0, &n), "get_annotation()");
    BFT_annotation* a = create_BFT_annotation();
    a->annot = malloc(n ? n : 1);
    NOT_NULL(a->annot, "get_annotation()");
    ck(bft_gpu_colorset_annot(bft->gpu, bft_kmer->res->colorset, a->annot, n, &n), "get_annotation()");
    a->size_annot = (int)n;
    a->from_BFT = 1;
    return a;
}

/* get_id_genomes_from_annot, modes 0/1/2 (src/annotation.c:2086-2250): the byte codec of one annotation object, the
 * inverse of what bft_gpu_colorset_annot produced.  ids may be NULL to count only. */
static uint32_t decode_annot(const BFT_annotation* a, uint32_t* ids) {
    const uint8_t* b = a->annot;
    const int size = a->size_annot;
    uint32_t n = 0;
    if (b == NULL || size <= 0) return 0;
    const int mode = b[0] & 3;
    int i = 0;
    if (mode == 0) {
        for (int bit = 2; bit < size * 8; bit++)
            if (b[bit >> 3] & (1u << (bit & 7))) { if (ids) ids[n] = (uint32_t)bit - 2; n++; }
    } else if (mode == 1) { /* inclusive ranges: start byte flag 1, continuation flag 2 */
        while (i < size && (b[i] & 1)) {
            uint32_t lo = b[i++] >> 2, hi;
            while (i < size && (b[i] & 2)) lo = (lo << 6) | (b[i++] >> 2);
            if (i >= size || !(b[i] & 1)) break;
            hi = b[i++] >> 2;
            while (i < size && (b[i] & 2)) hi = (hi << 6) | (b[i++] >> 2);
            for (uint32_t v = lo; v <= hi; v++) { if (ids) ids[n] = v; n++; }
        }
    } else if (mode == 2) { /* id list: start byte flag 2, continuation flag 1 */
        while (i < size && (b[i] & 2)) {
            uint32_t v = b[i++] >> 2;
            while (i < size && (b[i] & 1)) v = (v << 6) | (b[i++] >> 2);
            if (ids) ids[n] = v;
            n++;
        }
    } else
        DIE("get_id_genomes_from_annot(): compressed annotations (mode 3) are not produced by this library.\n");
    return n;
}

uint32_t* get_list_id_genomes(BFT_annotation* bft_annot, BFT* bft) {
    NOT_NULL(bft_annot, "get_list_id_genomes()");
    NOT_NULL(bft, "get_list_id_genomes()");
    const uint32_t n = decode_annot(bft_annot, NULL);
    uint32_t* ids = malloc(((size_t)n + 1) * sizeof(uint32_t));
    NOT_NULL(ids, "get_list_id_genomes()");
    ids[0] = n;
    decode_annot(bft_annot, ids + 1);
    return ids;
}

uint32_t get_count_id_genomes(BFT_annotation* bft_annot, BFT* bft) {
    NOT_NULL(bft_annot, "get_count_id_genomes()");
    NOT_NULL(bft, "get_count_id_genomes()");
    return decode_annot(bft_annot, NULL);
}

bool presence_genome(uint32_t id_genome, BFT_annotation* bft_annot, BFT* bft) {
    NOT_NULL(bft_annot, "is_genome_present()");
    NOT_NULL(bft, "is_genome_present()");
    if (id_genome >= (uint32_t)bft->nb_genomes) return false;
    uint32_t* ids = get_list_id_genomes(bft_annot, bft);
    bool found = false;
    for (uint32_t i = 1; i <= ids[0] && !found; i++) found = ids[i] == id_genome;
    free(ids);
    return found;
}

/* intersection_annotations / union_annotations / sym_difference_annotations (src/bft.c:421-613) on the host: the annotations are host bytes already.
 * Every argument is decoded into a bitmap in cmp_annots' result layout (src/annotation.c:2358-2551: mode 0, genome g at bit g + 2, MAX(CEIL(nb_genomes + 2,
 * 8), 1) bytes); the AND and the OR of those bitmaps give the three results.  op: 0 intersection, 1 union, 2 symmetric difference = union minus
 * intersection (one argument: its set). */
static BFT_annotation* combine_annotations(BFT* bft, uint32_t nb_annotations, va_list args, int op, const char* name) {
    if (nb_annotations == 0) DIE("%s(): no annotations given as parameters.\n", name);
    if (bft == NULL) DIE("usage of a null pointer in function %s()\n \n", name);
    const uint32_t G = bft->nb_genomes > 0 ? (uint32_t)bft->nb_genomes : 0;
    const size_t len = ((size_t)G + 2 + 7) / 8 > 1 ? ((size_t)G + 2 + 7) / 8 : 1;
    uint8_t* all = malloc(len);
    uint8_t* any = calloc(len, 1);
    uint8_t* cur = malloc(len);
    if (all == NULL || any == NULL || cur == NULL) DIE("%s(): out of memory\n", name);
    memset(all, 0xFF, len);
    for (uint32_t i = 0; i < nb_annotations; i++) {
        const BFT_annotation* a = va_arg(args, BFT_annotation*);
        if (a == NULL) DIE("usage of a null pointer in function %s()\n \n", name); /* (ASSERT_NULL_PTR, include/useful_macros.h:38-43) */
        const uint32_t n = decode_annot(a, NULL);
        uint32_t* ids = malloc(((size_t)n + 1) * sizeof(uint32_t));
        if (ids == NULL) DIE("%s(): out of memory\n", name);
        decode_annot(a, ids);
        memset(cur, 0, len);
        for (uint32_t j = 0; j < n; j++)
            if (ids[j] < G) cur[(ids[j] + 2) >> 3] |= (uint8_t)(1u << ((ids[j] + 2) & 7));
        free(ids);
        for (size_t q = 0; q < len; q++) {
            all[q] = intersection_annots(all[q], cur[q]);
            any[q] = union_annots(any[q], cur[q]);
        }
    }
    if (op == 0) memcpy(cur, all, len);
    else if (op == 1 || nb_annotations == 1) memcpy(cur, any, len);
    else
        for (size_t q = 0; q < len; q++) cur[q] = sym_difference_annots(all[q], any[q]);
    free(all);
    free(any);
    BFT_annotation* out = create_BFT_annotation();
    out->annot = cur;
    out->size_annot = (int)len;
    return out;
}

BFT_annotation* intersection_annotations(BFT* bft, uint32_t nb_annotations, ...) {
    va_list args;
    va_start(args, nb_annotations);
    BFT_annotation* out = combine_annotations(bft, nb_annotations, args, 0, "intersection_annotations");
    va_end(args);
    return out;
}

BFT_annotation* union_annotations(BFT* bft, uint32_t nb_annotations, ...) {
    va_list args;
    va_start(args, nb_annotations);
    BFT_annotation* out = combine_annotations(bft, nb_annotations, args, 1, "union_annotations");
    va_end(args);
    return out;
}

BFT_annotation* sym_difference_annotations(BFT* bft, uint32_t nb_annotations, ...) {
    va_list args;
    va_start(args, nb_annotations);
    BFT_annotation* out = combine_annotations(bft, nb_annotations, args, 2, "sym_difference_annotations");
    va_end(args);
    return out;
}

uint32_t* intersection_list_id_genomes(uint32_t* list_a, uint32_t* list_b) { /* src/bft.c:659-688 */
    NOT_NULL(list_a, "intersection_list_id_genomes()");
    NOT_NULL(list_b, "intersection_list_id_genomes()");
    const uint32_t na = list_a[0], nb = list_b[0];
    uint32_t* out = malloc(((size_t)(na < nb ? na : nb) + 1) * sizeof(uint32_t));
    NOT_NULL(out, "intersection_list_id_genomes()");
    uint32_t i = 1, j = 1, n = 0;
    while (i <= na && j <= nb) {
        if (list_a[i] < list_b[j]) i++;
        else if (list_b[j] < list_a[i]) j++;
        else { out[++n] = list_a[i]; i++; j++; }
    }
    out[0] = n;
    return out;
}

/* ---------------------------------------------------------------- sequence query */

uint32_t* query_sequence(BFT* bft, char* sequence, double threshold, bool canonical_search) {
    NOT_NULL(bft, "query_sequence()");
    NOT_NULL(sequence, "query_sequence()");
    if (threshold <= 0) DIE("query_sequence(): the threshold must be superior to 0.\n");
    if (threshold > 1) DIE("query_sequence(): the threshold must be inferior or equal to 1.\n");
    const size_t len = strlen(sequence);
    if (len < (size_t)bft->k) printf("query_sequence(): query %s is too small and must be at least of length k.\n", sequence);
    const uint32_t G = (uint32_t)bft->nb_genomes, rowbytes = (G + 7) / 8;
    uint8_t* row = calloc(rowbytes ? rowbytes : 1, 1);
    NOT_NULL(row, "query_sequence()");
    const uint64_t off[2] = {0, (uint64_t)len};
    if (G) ck(bft_gpu_query_sequences(bft->gpu, sequence, off, 1, threshold, canonical_search ? 1 : 0, row), "query_sequence()");
    uint32_t n = 0;
    for (uint32_t g = 0; g < G; g++) n += (row[g >> 3] >> (g & 7)) & 1;
    uint32_t* ids = malloc(((size_t)n + 1) * sizeof(uint32_t));
    NOT_NULL(ids, "query_sequence()");
    ids[0] = n;
    for (uint32_t g = 0, j = 0; g < G; g++)
        if ((row[g >> 3] >> (g & 7)) & 1) ids[++j] = g;
    free(row);
    return ids;
}

/* ---------------------------------------------------------------- neighbours */

void set_neighbors_traversal(BFT* bft) { NOT_NULL(bft, "set_neighbors_traversal()"); }
void unset_neighbors_traversal(BFT* bft) { NOT_NULL(bft, "unset_neighbors_traversal()"); }

/* side 0: N + kmer[0..k-2] (predecessors), side 1: kmer[1..k-1] + N (successors); N = A, C, G, T */
static void neighbours_of(const BFT_kmer* km, BFT* bft, int side, BFT_kmer* out, uint8_t* packed) {
    const int k = bft->k, nb = bytes_of(k);
    for (int i = 0; i < 4; i++) {
        out[i].kmer = malloc((size_t)k + 1);
        out[i].kmer_comp = malloc((size_t)nb);
        if (out[i].kmer == NULL || out[i].kmer_comp == NULL) DIE("get_neighbors(): out of memory\n");
        if (side == 0) {
            out[i].kmer[0] = "ACGT"[i];
            memcpy(out[i].kmer + 1, km->kmer, (size_t)k - 1);
        } else {
            memcpy(out[i].kmer, km->kmer + 1, (size_t)k - 1);
            out[i].kmer[k - 1] = "ACGT"[i];
        }
        out[i].kmer[k] = '\0';
        pack_kmer(out[i].kmer, k, out[i].kmer_comp);
        memcpy(packed + (size_t)i * nb, out[i].kmer_comp, (size_t)nb);
    }
}

static BFT_kmer* neighbours(BFT_kmer* km, BFT* bft, int first_side, int n_sides, const char* where) {
    NOT_NULL(km, where);
    NOT_NULL(bft, where);
    if (!is_kmer_in_cdbg(km)) DIE("%s: k-mer is not present in the graph.\n", where);
    const int nb = bytes_of(bft->k), n = 4 * n_sides;
    BFT_kmer* out = malloc((size_t)n * sizeof(BFT_kmer));
    uint8_t* packed = malloc((size_t)n * (size_t)nb);
    if (out == NULL || packed == NULL) DIE("%s: out of memory\n", where);
    for (int s = 0; s < n_sides; s++) neighbours_of(km, bft, first_side + s, out + 4 * s, packed + (size_t)(4 * s) * nb);
    locate(bft, packed, n, out, where);
    free(packed);
    return out;
}

BFT_kmer* get_neighbors(BFT_kmer* bft_kmer, BFT* bft) { return neighbours(bft_kmer, bft, 0, 2, "get_neighbors()"); }
BFT_kmer* get_predecessors(BFT_kmer* bft_kmer, BFT* bft) { return neighbours(bft_kmer, bft, 0, 1, "get_predecessors()"); }
BFT_kmer* get_successors(BFT_kmer* bft_kmer, BFT* bft) { return neighbours(bft_kmer, bft, 1, 1, "get_successors()"); }

/* ---------------------------------------------------------------- iteration, extraction */

void v_iterate_over_kmers(BFT* bft, BFT_func_ptr f, va_list args) {
    NOT_NULL(bft, "v_iterate_over_kmers()");
    NOT_NULL(f, "v_iterate_over_kmers()");
    uint64_t n = 0;
    ck(bft_gpu_extract(bft->gpu, NULL, NULL, 0, &n), "iterate_over_kmers()");
    if (n == 0) return;
    const int k = bft->k, nb = bytes_of(k);
    uint8_t* packed = malloc((size_t)n * (size_t)nb);
    uint32_t* sets = malloc((size_t)n * sizeof(uint32_t));
    if (packed == NULL || sets == NULL) DIE("iterate_over_kmers(): out of memory\n");
    ck(bft_gpu_extract(bft->gpu, packed, sets, n, &n), "iterate_over_kmers()");
    BFT_kmer* km = create_empty_kmer();
    km->kmer = malloc((size_t)k + 1);
    km->kmer_comp = malloc((size_t)nb);
    km->res = new_res(bft, 1, 0, 0);
    if (km->kmer == NULL || km->kmer_comp == NULL) DIE("iterate_over_kmers(): out of memory\n");
    for (uint64_t i = 0; i < n; i++) {
        memcpy(km->kmer_comp, packed + i * (size_t)nb, (size_t)nb);
        unpack_kmer(km->kmer_comp, k, km->kmer);
        km->res->row = (uint32_t)i;
        km->res->colorset = sets[i];
        va_list copy; /* f consumes its arguments with va_arg on every call (src/extract_kmers.c does the same) */
        va_copy(copy, args);
        const size_t go_on = f(km, bft, copy);
        va_end(copy);
        if (go_on == 0) break;
    }
    free_BFT_kmer(km, 1);
    free(packed);
    free(sets);
}

void iterate_over_kmers(BFT* bft, BFT_func_ptr f, ...) {
    va_list args;
    va_start(args, f);
    v_iterate_over_kmers(bft, f, args);
    va_end(args);
}

/* ---------------------------------------------------------------- pattern matching */

/* src/bft.c:1087-1147.  The matches are one batch query (bft_gpu_query_prefixes): counted first, then fetched, and f is called on them in
 * ascending row order -- the reference calls it in the DFS order of its containers. */
bool prefix_matching(BFT* bft, char* prefix, BFT_func_ptr f, ...) {
    NOT_NULL(bft, "prefix_matching()");
    NOT_NULL(prefix, "prefix_matching()");
    const int k = bft->k, nb = bytes_of(k);
    const size_t len = strlen(prefix);
    if (len > (size_t)k) DIE("prefix_matching(): Prefix length is larger than k-mer length.\n");
    if (len == 0) DIE("prefix_matching(): Prefix length is 0.\n");
    NOT_NULL(f, "prefix_matching()");
    uint8_t* packed = calloc((size_t)nb, 1);
    NOT_NULL(packed, "prefix_matching()");
    if (!parseKmerCount(prefix, (int)len, packed, 0)) DIE("prefix_matching(): Non-ACGT char. encountered in prefix.\n");
    const uint8_t length = (uint8_t)len;
    uint64_t offsets[2] = {0, 0}, n = 0;
    ck(bft_gpu_query_prefixes(bft->gpu, packed, &length, 1, offsets, NULL, NULL, NULL, 0, &n), "prefix_matching()");
    if (n == 0) {
        free(packed);
        return false;
    }
    uint8_t* kmers = malloc((size_t)n * (size_t)nb);
    uint32_t* rows = malloc((size_t)n * sizeof(uint32_t));
    uint32_t* sets = malloc((size_t)n * sizeof(uint32_t));
    if (kmers == NULL || rows == NULL || sets == NULL) DIE("prefix_matching(): out of memory\n");
    ck(bft_gpu_query_prefixes(bft->gpu, packed, &length, 1, offsets, kmers, rows, sets, n, &n), "prefix_matching()");
    BFT_kmer* km = create_empty_kmer();
    km->kmer = malloc((size_t)k + 1);
    km->kmer_comp = malloc((size_t)nb);
    km->res = new_res(bft, 1, 0, 0);
    if (km->kmer == NULL || km->kmer_comp == NULL) DIE("prefix_matching(): out of memory\n");
    va_list args;
    va_start(args, f);
    for (uint64_t i = 0; i < n; i++) {
        memcpy(km->kmer_comp, kmers + i * (size_t)nb, (size_t)nb);
        unpack_kmer(km->kmer_comp, k, km->kmer);
        km->res->row = rows[i];
        km->res->colorset = sets[i];
        va_list copy; /* a fresh copy per call, as v_iterate_over_kmers */
        va_copy(copy, args);
        const size_t go_on = f(km, bft, copy);
        va_end(copy);
        if (go_on == 0) break;
    }
    va_end(args);
    free_BFT_kmer(km, 1);
    free(kmers);
    free(rows);
    free(sets);
    free(packed);
    return true;
}

/* ---------------------------------------------------------------- sub-graphs */

/* src/bft.c:1353-1464.  add_colors: one call of bft_gpu_subgraph -- the k-mers of the source with their colour sets, built on the GPU from the
 * source's sorted table and dictionary instead of genome-id insertions one k-mer at a time; k-mers the source does not store are skipped (the
 * reference's behaviour there is undefined: it reads the annotation of a k-mer that has none).  Otherwise, as the reference: every given k-mer
 * goes into one new genome named bft->filenames[0], stored in the source or not. */
BFT* create_cdbg_from_bft_kmers(BFT_kmer** bft_kmers, uint32_t nb_bft_kmers, BFT* bft, bool add_colors) {
    NOT_NULL(bft, "create_sub_cdbg()");
    NOT_NULL(bft_kmers, "create_sub_cdbg()");
    const int k = bft->k, nb = bytes_of(k);
    if (!add_colors) {
        if (bft->nb_genomes <= 0) DIE("create_sub_cdbg(): the graph has no genome to name the new one after.\n");
        char** kmers = malloc((size_t)(nb_bft_kmers ? nb_bft_kmers : 1) * sizeof(char*));
        NOT_NULL(kmers, "create_sub_cdbg()");
        for (uint32_t i = 0; i < nb_bft_kmers; i++) {
            NOT_NULL(bft_kmers[i], "create_sub_cdbg()");
            kmers[i] = bft_kmers[i]->kmer;
        }
        BFT* sub = create_cdbg(k, bft->treshold_compression);
        insert_kmers_new_genome((int)nb_bft_kmers, kmers, bft->filenames[0], sub);
        free(kmers);
        return sub;
    }
    uint8_t* batch = malloc((size_t)(nb_bft_kmers ? nb_bft_kmers : 1) * (size_t)nb);
    NOT_NULL(batch, "create_sub_cdbg()");
    for (uint32_t i = 0; i < nb_bft_kmers; i++) {
        NOT_NULL(bft_kmers[i], "create_sub_cdbg()");
        NOT_NULL(bft_kmers[i]->kmer, "create_sub_cdbg()");
        if (strlen(bft_kmers[i]->kmer) < (size_t)k || !pack_kmer(bft_kmers[i]->kmer, k, batch + (size_t)i * nb))
            DIE("create_sub_cdbg(): Unexpected character encountered in k-mer.\n");
    }
    bft_gpu* g = NULL;
    ck(bft_gpu_subgraph(bft->gpu, batch, nb_bft_kmers, 1, NULL, &g), "create_sub_cdbg()");
    free(batch);
    BFT* sub = new_root(k, bft->treshold_compression, g);
    for (int i = 0; i < bft->nb_genomes; i++) push_name(sub, bft->filenames[i]); /* add_genomes_BFT_Root(bft->nb_genomes, bft->filenames, sub) */
    return sub;
}

static int cmp_u32(const void* a, const void* b) {
    const uint32_t x = *(const uint32_t*)a, y = *(const uint32_t*)b;
    return x < y ? -1 : (x > y);
}

/* src/bft.c:1466-1684: list_id_genomes[0] ids follow in list_id_genomes[1..]; they are sorted in place, as the reference does, and every one
 * must name an inserted genome.  The (k-mer, id) pairs are inserted; bft_kmer->res is looked up again, so that get_annotation(bft_kmer)
 * answers the widened set.  bft_annot is not needed here (the reference reads the current set out of it). */
void add_id_genomes(BFT_kmer* bft_kmer, BFT_annotation* bft_annot, BFT* bft, uint32_t* list_id_genomes) {
    (void)bft_annot;
    NOT_NULL(bft_kmer, "add_id_genomes()");
    NOT_NULL(bft, "add_id_genomes()");
    NOT_NULL(list_id_genomes, "add_id_genomes()");
    if (list_id_genomes[0] == 0) return;
    NOT_NULL(bft_kmer->kmer, "add_id_genomes()");
    qsort(&list_id_genomes[1], list_id_genomes[0], sizeof(uint32_t), cmp_u32);
    for (uint32_t j = list_id_genomes[0]; j >= 1; j--)
        if (bft->nb_genomes <= 0 || list_id_genomes[j] > (uint32_t)bft->nb_genomes - 1)
            DIE("add_id_genomes(): An attempt to update a k-mer with a genome id that has not been inserted in the BFT yet has been made.\n");
    const int nb = bytes_of(bft->k);
    uint8_t* packed = malloc((size_t)nb);
    NOT_NULL(packed, "add_id_genomes()");
    if (strlen(bft_kmer->kmer) < (size_t)bft->k || !pack_kmer(bft_kmer->kmer, bft->k, packed))
        DIE("add_id_genomes(): Unexpected character encountered in k-mer.\n");
    for (uint32_t j = 1; j <= list_id_genomes[0]; j++)
        if (j == 1 || list_id_genomes[j] != list_id_genomes[j - 1]) ck(bft_gpu_insert_kmers(bft->gpu, packed, 1, list_id_genomes[j]), "add_id_genomes()");
    BFT_kmer fresh;
    locate(bft, packed, 1, &fresh, "add_id_genomes()");
    if (bft_kmer->res != NULL) {
        *bft_kmer->res = *fresh.res;
        free(fresh.res);
    } else
        bft_kmer->res = fresh.res;
    free(packed);
}

size_t write_kmer_ascii_to_disk(BFT_kmer* bft_kmer, BFT* bft, va_list args) { /* src/bft.c:299-308 */
    FILE* file = va_arg(args, FILE*);
    bft_kmer->kmer[bft->k] = '\n';
    fwrite(bft_kmer->kmer, sizeof(char), (size_t)bft->k + 1, file);
    bft_kmer->kmer[bft->k] = '\0';
    return 1;
}

size_t write_kmer_comp_to_disk(BFT_kmer* bft_kmer, BFT* bft, va_list args) { /* src/bft.c:316-324 */
    (void)bft;
    const int nb_bytes_kmer_comp = va_arg(args, int);
    FILE* file = va_arg(args, FILE*);
    fwrite(bft_kmer->kmer_comp, sizeof(uint8_t), (size_t)nb_bytes_kmer_comp, file);
    return 1;
}

void extract_kmers_to_disk(BFT* bft, char* filename_output, bool compressed_output) { /* src/bft.c:255-290 */
    NOT_NULL(bft, "extract_kmers_to_disk()");
    NOT_NULL(filename_output, "extract_kmers_to_disk()");
    FILE* f = fopen(filename_output, "w");
    if (f == NULL) DIE("extract_kmers_to_disk(): failed to create/open output file.\n");
    if (compressed_output) {
        uint64_t n = 0;
        ck(bft_gpu_extract(bft->gpu, NULL, NULL, 0, &n), "extract_kmers_to_disk()");
        fprintf(f, "%d\n%llu\n", bft->k, (unsigned long long)n);
        iterate_over_kmers(bft, write_kmer_comp_to_disk, bytes_of(bft->k), f);
    } else
        iterate_over_kmers(bft, write_kmer_ascii_to_disk, f);
    fclose(f);
}

/* ---------------------------------------------------------------- disk */

void write_BFT(BFT* bft, char* filename, bool compress_annotations) {
    (void)compress_annotations;
    NOT_NULL(bft, "write_BFT()");
    NOT_NULL(filename, "write_BFT()");
    ck(bft_gpu_write_bft(bft->gpu, filename), "write_BFT()");
}

BFT* load_BFT(char* filename) {
    NOT_NULL(filename, "load_BFT()");
    bft_gpu* g = NULL;
    ck(bft_gpu_load_bft(filename, device_from_env(), &g), "load_BFT()");
    uint64_t info[16];
    ck(bft_gpu_info(g, info, 16), "load_BFT()");
    BFT* bft = new_root((int)info[0], 0, g);
    char name[4096];
    for (uint64_t i = 0; i < info[11]; i++) {
        ck(bft_gpu_genome_name(g, (uint32_t)i, name, sizeof name), "load_BFT()");
        push_name(bft, name);
    }
    return bft;
}

/* ---------------------------------------------------------------- merge (<bft/merge.h>) */

/* include/merge.h:14.  The second graph's genomes follow the first graph's; they start on its last one when that name is the second graph's first
 * (are_genomes_ids_overlapping, include/Node.h:147-155).  One bft_gpu_merge call instead of an insertion per k-mer of the second graph. */
void merging_BFT(char* prefix_bft1, char* prefix_bft2, char* output_prefix, int cut_lvl, bool packed_in_subtries) {
    (void)cut_lvl;
    (void)packed_in_subtries;
    NOT_NULL(prefix_bft1, "merging_BFT()");
    NOT_NULL(prefix_bft2, "merging_BFT()");
    NOT_NULL(output_prefix, "merging_BFT()");
    BFT* bft1 = load_BFT(prefix_bft1);
    BFT* bft2 = load_BFT(prefix_bft2);
    uint32_t id_base = (uint32_t)bft1->nb_genomes;
    if (bft1->nb_genomes > 0 && bft2->nb_genomes > 0 && strcmp(bft1->filenames[bft1->nb_genomes - 1], bft2->filenames[0]) == 0) id_base--;
    bft_gpu* g = NULL;
    ck(bft_gpu_merge(bft1->gpu, bft2->gpu, id_base, &g), "merging_BFT()");
    ck(bft_gpu_write_bft(g, output_prefix), "merging_BFT()");
    bft_gpu_free(g);
    free_cdbg(bft2);
    free_cdbg(bft1);
}

/* ---------------------------------------------------------------- simple paths (<bft/snippets.h>) */

/* src/snippets.c:306-344 and :563-603 without the walk: the file is opened first (the reference's ERROR on failure), then one
 * bft_gpu_simple_paths call counts the paths and a second one fetches them; they are written one per line and the longest is reported.
 * paths: bft_gpu_simple_paths, or bft_gpu_unitigs for <bft/unitigs.h> (the same arguments, the same host rules). */
typedef int (*paths_call)(bft_gpu*, uint32_t, uint64_t*, char*, uint64_t, uint64_t, uint64_t*, uint64_t*);
static void paths_to_disk(BFT* bft, paths_call paths, uint32_t t, const char* filename, const char* open_error, const char* report, const char* where) {
    FILE* file = fopen(filename, "w");
    if (file == NULL) DIE("%s", open_error);
    uint64_t n_paths = 0, n_chars = 0;
    ck(paths(bft->gpu, t, NULL, NULL, 0, 0, &n_paths, &n_chars), where);
    uint64_t* offsets = malloc((size_t)(n_paths + 1) * sizeof(uint64_t));
    char* seqs = malloc((size_t)(n_chars ? n_chars : 1));
    if (offsets == NULL || seqs == NULL) DIE("%s: out of memory\n", where);
    ck(paths(bft->gpu, t, offsets, seqs, n_paths, n_chars, &n_paths, &n_chars), where);
    uint64_t longest = 0;
    for (uint64_t i = 0; i < n_paths; i++) {
        const uint64_t len = offsets[i + 1] - offsets[i];
        if (len > longest) longest = len;
        if (fwrite(seqs + offsets[i], 1, (size_t)len, file) != len || fputc('\n', file) == EOF) DIE("%s: failed to write the output file.\n", where);
    }
    if (fclose(file) != 0) DIE("%s: failed to write the output file.\n", where);
    free(offsets);
    free(seqs);
    printf(report, (int)longest);
}
static void simple_paths_to_disk(BFT* bft, uint32_t t, const char* filename, const char* open_error, const char* what, const char* where) {
    char report[64];
    snprintf(report, sizeof report, "Longest simple %spath has %%d nuc.\n", what);
    paths_to_disk(bft, bft_gpu_simple_paths, t, filename, open_error, report, where);
}

void extract_simple_paths_to_disk(BFT* graph, char* filename_output) {
    NOT_NULL(graph, "extract_simple_paths_to_disk()");
    NOT_NULL(filename_output, "extract_simple_paths_to_disk()");
    simple_paths_to_disk(graph, 0, filename_output, "extract_simple_paths_to_disk(): failed to create output file.\n", "", "extract_simple_paths_to_disk()");
}

void extract_simple_core_paths_to_disk(BFT* graph, double core_ratio, char* filename_output) {
    NOT_NULL(graph, "extract_simple_core_paths_to_disk()");
    NOT_NULL(filename_output, "extract_simple_core_paths_to_disk()");
    const int t = (int)(core_ratio * graph->nb_genomes); /* (truncated, as src/snippets.c:366; a negative threshold holds for every k-mer) */
    simple_paths_to_disk(graph, t > 0 ? (uint32_t)t : 0u, filename_output, "extract_simple_core_paths_to_disk(): failed to create/open output file.\n", "core ",
                         "extract_simple_core_paths_to_disk()");
}

/* <bft/unitigs.h>: the same file, from bft_gpu_unitigs */
void extract_unitigs_to_disk(BFT* graph, int min_shared, char* filename_output) {
    NOT_NULL(graph, "extract_unitigs_to_disk()");
    NOT_NULL(filename_output, "extract_unitigs_to_disk()");
    paths_to_disk(graph, bft_gpu_unitigs, min_shared > 0 ? (uint32_t)min_shared : 0u, filename_output, "extract_unitigs_to_disk(): failed to create output file.\n",
                  "Longest unitig has %d nuc.\n", "extract_unitigs_to_disk()");
}

/* <bft/unitigs.h>: the compacted coloured graph as GFA 1 (bft_gfa.h), from bft_gpu_unitig_graph and bft_gpu_unitig_colors */
void extract_unitig_graph_to_disk(BFT* graph, int min_shared, bool colors, char* filename_output) {
    NOT_NULL(graph, "extract_unitig_graph_to_disk()");
    NOT_NULL(filename_output, "extract_unitig_graph_to_disk()");
    FILE* file = fopen(filename_output, "w");
    if (file == NULL) DIE("extract_unitig_graph_to_disk(): failed to create output file.\n");
    const int rc = bft_gfa_write(graph->gpu, graph->k, min_shared > 0 ? (uint32_t)min_shared : 0u, colors ? 1 : 0, file);
    if (rc < 0) ck(rc, "extract_unitig_graph_to_disk()");
    if (rc == 1) DIE("extract_unitig_graph_to_disk(): out of memory\n");
    if (fclose(file) != 0 || rc) DIE("extract_unitig_graph_to_disk(): failed to write the output file.\n");
}

/* <bft/unitigs.h>: the simple bubbles (variants) of that graph as text (bft_bubbles_io.h), from bft_gpu_unitig_bubbles and bft_gpu_unitig_colors */
void extract_bubbles_to_disk(BFT* graph, int min_shared, int max_branch_length, char* filename_output) {
    NOT_NULL(graph, "extract_bubbles_to_disk()");
    NOT_NULL(filename_output, "extract_bubbles_to_disk()");
    FILE* file = fopen(filename_output, "w");
    if (file == NULL) DIE("extract_bubbles_to_disk(): failed to create output file.\n");
    const int rc = bft_bubbles_write(graph->gpu, graph->k, min_shared > 0 ? (uint32_t)min_shared : 0u, max_branch_length > 0 ? (uint64_t)max_branch_length : 0u, file);
    if (rc < 0) ck(rc, "extract_bubbles_to_disk()");
    if (rc == 1) DIE("extract_bubbles_to_disk(): out of memory\n");
    if (fclose(file) != 0 || rc) DIE("extract_bubbles_to_disk(): failed to write the output file.\n");
}

/* <bft/unitigs.h>: the sequences of a FASTA / FASTQ file threaded through that graph, one GAF line per walk (bft_gaf.h), from bft_gpu_thread_sequences */
void thread_sequences_to_disk(BFT* graph, int min_shared, char* filename_sequences, char* filename_output) {
    NOT_NULL(graph, "thread_sequences_to_disk()");
    NOT_NULL(filename_sequences, "thread_sequences_to_disk()");
    NOT_NULL(filename_output, "thread_sequences_to_disk()");
    FILE* file = fopen(filename_output, "w");
    if (file == NULL) DIE("thread_sequences_to_disk(): failed to create output file.\n");
    const int rc = bft_gaf_write(graph->gpu, graph->k, min_shared > 0 ? (uint32_t)min_shared : 0u, filename_sequences, file);
    if (rc < 0 || rc >= 3) { /* (nothing was written: no empty file stays behind) */
        fclose(file);
        remove(filename_output);
    }
    if (rc < 0) ck(rc, "thread_sequences_to_disk()");
    if (rc == 1) DIE("thread_sequences_to_disk(): out of memory\n");
    if (rc == 3) DIE("thread_sequences_to_disk(): failed to read the sequence file.\n");
    if (rc == 4) DIE("thread_sequences_to_disk(): the sequence file is neither FASTA nor FASTQ.\n");
    if (fclose(file) != 0 || rc) DIE("thread_sequences_to_disk(): failed to write the output file.\n");
}

/* ---------------------------------------------------------------- marking (include/bft.h:143-146, src/bft.c:686-765) */

/* While the graph is marking, bft->marks is a host copy of the handle's packed flag array (4 rows per byte, bft_gpu_marks_read): set_flag_kmer and
 * get_flag_kmer touch only the copy, by the row the k-mer's res already holds -- no GPU round trip per k-mer.  The copy goes to the GPU before a GPU
 * operation if it changed (marks_push), and comes back after one that painted (marks_pull). */
static void marks_push(BFT* bft, const char* where) {
    if (!bft->marks_dirty) return;
    ck(bft_gpu_marks_write(bft->gpu, bft->marks, bft->marks_bytes), where);
    bft->marks_dirty = 0;
}
static void marks_pull(BFT* bft, const char* where) {
    ck(bft_gpu_marks_read(bft->gpu, bft->marks, bft->marks_bytes, NULL), where);
}

void set_marking(BFT* bft) {
    NOT_NULL(bft, "set_marking()");
    if ((bft->marked & 0x1) == 0) {
        ck(bft_gpu_marks_begin(bft->gpu), "set_marking()");
        ck(bft_gpu_marks_read(bft->gpu, NULL, 0, &bft->marks_bytes), "set_marking()");
        free(bft->marks);
        bft->marks = calloc(bft->marks_bytes ? (size_t)bft->marks_bytes : 1, 1); /* (every flag is 0 after bft_gpu_marks_begin) */
        NOT_NULL(bft->marks, "set_marking()");
        bft->marks_dirty = 0;
        bft->marked |= 0x1;
    }
}

void unset_marking(BFT* bft) {
    NOT_NULL(bft, "unset_marking()");
    ck(bft_gpu_marks_end(bft->gpu), "unset_marking()");
    free(bft->marks);
    bft->marks = NULL;
    bft->marks_bytes = 0;
    bft->marks_dirty = 0;
    bft->marked &= 0xfe;
}

void set_flag_kmer(uint8_t flag, BFT_kmer* bft_kmer, BFT* bft) {
    NOT_NULL(bft_kmer, "set_flag_kmer()");
    NOT_NULL(bft, "set_flag_kmer()");
    if (flag > 3) DIE("set_flag_kmer(): a flag can only have as value 0, 1, 2 or 3.\n");
    if ((bft->marked & 0x1) == 0) DIE("set_flag_kmer(): the graph is not initialized for marking.\n");
    if (!is_kmer_in_cdbg(bft_kmer) || ((uint64_t)bft_kmer->res->row >> 2) >= bft->marks_bytes) DIE("set_flag_kmer(): k-mer is not present in the graph.\n");
    const uint32_t row = bft_kmer->res->row, sh = 2 * (row & 3);
    uint8_t* b = &bft->marks[row >> 2];
    const uint8_t v = (uint8_t)((*b & ~(3u << sh)) | ((uint32_t)flag << sh));
    if (v != *b) {
        *b = v;
        bft->marks_dirty = 1;
    }
}

uint8_t get_flag_kmer(BFT_kmer* bft_kmer, BFT* bft) {
    NOT_NULL(bft_kmer, "get_flag_kmer()");
    NOT_NULL(bft, "get_flag_kmer()");
    if ((bft->marked & 0x1) == 0) DIE("get_flag_kmer(): the graph is not initialized for marking.\n");
    if (!is_kmer_in_cdbg(bft_kmer) || ((uint64_t)bft_kmer->res->row >> 2) >= bft->marks_bytes) DIE("get_flag_kmer(): k-mer is not present in the graph.\n");
    const uint32_t row = bft_kmer->res->row;
    return (uint8_t)((bft->marks[row >> 2] >> (2 * (row & 3))) & 3);
}

/* ---------------------------------------------------------------- connected components (<bft/snippets.h>) */

/* BFS, DFS, BFS_subgraph and DFS_subgraph (src/snippets.c:605-822) on a graph that is marking: a k-mer whose flag is not 0 gives 0; otherwise ONE
 * bft_gpu_marks_reach from it (through 0, to 1) paints what the reference's walk would mark -- the _subgraph forms with the boundary rows and the ids
 * read as the reference reads them -- and the result is what the reach says of the seed.  On a graph that is NOT marking they stop the program (the
 * reference would, in get_flag_kmer); the message names get_nb_connected_component, which counts components without marks. */
#define NEEDS_MARKING(where) DIE("%s: vertex marking is not set (set_marking()); pass it to get_nb_connected_component() to count components.\n", where)
static size_t traverse(BFT_kmer* kmer, BFT* graph, va_list args, int sub, const char* where) {
    NOT_NULL(kmer, where);
    NOT_NULL(graph, where);
    if ((graph->marked & 0x1) == 0) NEEDS_MARKING(where);
    if (get_flag_kmer(kmer, graph) != 0) return 0;
    uint32_t* ids = NULL;
    int nb_ids = 0;
    if (sub) {
        va_list cpy;
        va_copy(cpy, args);
        nb_ids = va_arg(cpy, int);
        bool in_order = nb_ids > 0;
        if (nb_ids > 0) {
            ids = malloc((size_t)nb_ids * sizeof(uint32_t));
            NOT_NULL(ids, where);
            for (int i = 0; i < nb_ids; i++) {
                ids[i] = va_arg(cpy, uint32_t);
                if (i && ids[i] <= ids[i - 1]) in_order = false;
            }
        }
        va_end(cpy);
        if (!in_order) { /* is_in_subgraph is false for every k-mer: the k-mer is marked visited and starts nothing (src/snippets.c:683-731) */
            free(ids);
            set_flag_kmer(1, kmer, graph);
            return 0;
        }
    }
    marks_push(graph, where);
    uint8_t seed_new = 0;
    uint64_t counts[3] = {0, 0, 0};
    ck(bft_gpu_marks_reach(graph->gpu, kmer->kmer_comp, 1, ids, (uint32_t)nb_ids, 0, 1, sub, &seed_new, counts), where);
    free(ids);
    if (counts[0] + counts[1]) marks_pull(graph, where);
    return seed_new;
}
size_t BFS(BFT_kmer* kmer, BFT* graph, va_list args) { return traverse(kmer, graph, args, 0, "BFS()"); }
size_t BFS_subgraph(BFT_kmer* kmer, BFT* graph, va_list args) { return traverse(kmer, graph, args, 1, "BFS_subgraph()"); }
size_t DFS(BFT_kmer* kmer, BFT* graph, va_list args) { return traverse(kmer, graph, args, 0, "DFS()"); }
size_t DFS_subgraph(BFT_kmer* kmer, BFT* graph, va_list args) { return traverse(kmer, graph, args, 1, "DFS_subgraph()"); }

/* src/snippets.c:883-906: marking on, f on every k-mer, marking off. */
void cdbg_traversal(BFT* graph, BFT_func_ptr f, ...) {
    NOT_NULL(graph, "cdbg_traversal()");
    va_list args;
    va_start(args, f);
    set_neighbors_traversal(graph);
    set_marking(graph);
    v_iterate_over_kmers(graph, f, args);
    unset_marking(graph);
    unset_neighbors_traversal(graph);
    va_end(args);
}

/* src/snippets.c:915-930: the callback of iterate_over_kmers on a marking graph -- args: int* nb, the traversal, the traversal's own arguments. */
size_t nb_connected_components(BFT_kmer* kmer, BFT* graph, va_list args) {
    int* nb_connected_comp = va_arg(args, int*);
    BFT_func_ptr f = va_arg(args, BFT_func_ptr);
    NOT_NULL(nb_connected_comp, "nb_connected_components()");
    NOT_NULL(f, "nb_connected_components()");
    *nb_connected_comp += f(kmer, graph, args) == true;
    return 1;
}

/* src/snippets.c:824-881: the k-mer's sorted id list is walked against the requested ids in the order given, and the walk stops at the first list
 * id above the one looked for.  True only when nb_id_genomes > 0, the ids are strictly increasing and all of them are in the k-mer's set. */
bool is_in_subgraph(BFT_kmer* kmer, BFT* graph, int nb_id_genomes, const va_list args) {
    NOT_NULL(kmer, "is_in_subgraph()");
    NOT_NULL(graph, "is_in_subgraph()");
    BFT_annotation* annot = get_annotation(kmer);
    uint32_t* list_ids = get_list_id_genomes(annot, graph);
    free_BFT_annotation(annot);
    int j = 0;
    if (nb_id_genomes > 0 && list_ids[0] >= (uint32_t)nb_id_genomes) {
        va_list cpy;
#pragma GCC diagnostic push
#pragma GCC diagnostic ignored "-Wdiscarded-qualifiers"
        va_copy(cpy, args); /* (the reference's signature takes a const va_list; va_copy only reads it) */
#pragma GCC diagnostic pop
        uint32_t curr = va_arg(cpy, uint32_t);
        for (uint32_t i = 1; i <= list_ids[0]; i++) {
            if (list_ids[i] == curr) {
                if (++j == nb_id_genomes) break;
                curr = va_arg(cpy, uint32_t);
            } else if (list_ids[i] > curr)
                break;
        }
        va_end(cpy);
    }
    free(list_ids);
    return nb_id_genomes > 0 && j == nb_id_genomes;
}

/* src/snippets.c:915-960: get_nb_connected_component(graph, int* nb, BFT_func_ptr f[, int nb_id_genomes, uint32_t id...]) ADDS the number of
 * connected components to *nb.  One bft_gpu_components count instead of one traversal per k-mer: f = BFS or DFS counts the whole graph,
 * BFS_subgraph or DFS_subgraph the sub-graph induced by the k-mers that carry every id.  As in the reference, nb_id_genomes <= 0 or ids that are
 * not strictly increasing match no k-mer (is_in_subgraph): they add 0. */
void get_nb_connected_component(BFT* graph, ...) {
    NOT_NULL(graph, "get_nb_connected_component()");
    va_list args;
    va_start(args, graph);
    int* nb = va_arg(args, int*);
    BFT_func_ptr f = va_arg(args, BFT_func_ptr);
    NOT_NULL(nb, "get_nb_connected_component()");
    uint64_t counts[3] = {0, 0, 0};
    if (f == BFS || f == DFS)
        ck(bft_gpu_components(graph->gpu, NULL, 0, NULL, 0, NULL, 0, counts), "get_nb_connected_component()");
    else if (f == BFS_subgraph || f == DFS_subgraph) {
        const int nb_ids = va_arg(args, int);
        if (nb_ids > 0) {
            uint32_t* ids = malloc((size_t)nb_ids * sizeof(uint32_t));
            NOT_NULL(ids, "get_nb_connected_component()");
            bool increasing = true;
            for (int i = 0; i < nb_ids; i++) {
                ids[i] = va_arg(args, uint32_t);
                if (i && ids[i] <= ids[i - 1]) increasing = false;
            }
            if (increasing) ck(bft_gpu_components(graph->gpu, ids, (uint32_t)nb_ids, NULL, 0, NULL, 0, counts), "get_nb_connected_component()");
            free(ids);
        }
    } else
        DIE("get_nb_connected_component(): the traversal function must be BFS, DFS, BFS_subgraph or DFS_subgraph.\n");
    va_end(args);
    *nb += (int)counts[0];
}

/* ---------------------------------------------------------------- pan-genome k-mer classes (<bft/snippets.h>) */

/* src/snippets.c:10-75: the callback's arguments are a FILE* and an int*; a k-mer whose genome count is in the class is written with its NUL
 * (strlen + 1 bytes) and counted.  The annotation is fetched as the reference fetches it, and freed (the reference leaks it). */
static size_t class_callback(BFT_kmer* kmer, BFT* graph, va_list args, int which, const char* where) {
    NOT_NULL(kmer, where);
    NOT_NULL(graph, where);
    FILE* file = va_arg(args, FILE*);
    int* nb_kmers = va_arg(args, int*);
    BFT_annotation* annot = get_annotation(kmer);
    const uint32_t count = get_count_id_genomes(annot, graph);
    free_BFT_annotation(annot);
    const uint32_t nb_genomes = (uint32_t)graph->nb_genomes;
    if (which == 0 ? count == nb_genomes : which == 1 ? count < nb_genomes : count == 1) {
        fwrite(kmer->kmer, sizeof(char), strlen(kmer->kmer) + 1, file);
        *nb_kmers += 1;
    }
    return true;
}
size_t extract_core_kmers(BFT_kmer* kmer, BFT* graph, va_list args) { return class_callback(kmer, graph, args, 0, "extract_core_kmers()"); }
size_t extract_dispensable_kmers(BFT_kmer* kmer, BFT* graph, va_list args) { return class_callback(kmer, graph, args, 1, "extract_dispensable_kmers()"); }
size_t extract_singleton_kmers(BFT_kmer* kmer, BFT* graph, va_list args) { return class_callback(kmer, graph, args, 2, "extract_singleton_kmers()"); }

/* src/snippets.c:86-106.  The three callbacks above are told apart by their addresses (as get_nb_connected_component tells BFS from DFS) and become a
 * range of genome counts: one bft_gpu_kmers_by_count call counts the class, a second one fetches it as ASCII with the NULs, and the file is one
 * fwrite.  Any other f is handed every k-mer through iterate_over_kmers, as in the reference.  Both routes visit the k-mers in row order. */
void extract_pangenome_kmers_to_disk(BFT* graph, char* filename_output, BFT_func_ptr f) {
    NOT_NULL(graph, "extract_pangenome_kmers_to_disk()");
    NOT_NULL(filename_output, "extract_pangenome_kmers_to_disk()");
    FILE* file = fopen(filename_output, "w");
    if (file == NULL) DIE("extract_pangenome_kmers_to_disk(): failed to create/open output file.\n");
    int nb_kmers = 0;
    if (f == extract_core_kmers || f == extract_dispensable_kmers || f == extract_singleton_kmers) {
        const uint32_t nb_genomes = graph->nb_genomes > 0 ? (uint32_t)graph->nb_genomes : 0u;
        uint32_t lo = 1, hi = 1;
        if (f == extract_core_kmers) lo = hi = nb_genomes;
        else if (f == extract_dispensable_kmers) { lo = 0; hi = nb_genomes - 1; }
        uint64_t n = 0;
        if (f != extract_dispensable_kmers || nb_genomes > 0) { /* (no genome: nothing is below 0, and 0 - 1 would wrap) */
            ck(bft_gpu_kmers_by_count(graph->gpu, lo, hi, NULL, NULL, NULL, 0, &n), "extract_pangenome_kmers_to_disk()");
            if (n) {
                const size_t bytes = (size_t)n * ((size_t)graph->k + 1);
                char* ascii = malloc(bytes);
                if (ascii == NULL) DIE("extract_pangenome_kmers_to_disk(): out of memory\n");
                ck(bft_gpu_kmers_by_count(graph->gpu, lo, hi, NULL, ascii, NULL, n, &n), "extract_pangenome_kmers_to_disk()");
                if (fwrite(ascii, 1, bytes, file) != bytes) DIE("extract_pangenome_kmers_to_disk(): failed to write the output file.\n");
                free(ascii);
            }
        }
        nb_kmers = (int)n;
    } else
        iterate_over_kmers(graph, f, file, &nb_kmers);
    if (fclose(file) != 0) DIE("extract_pangenome_kmers_to_disk(): failed to write the output file.\n");
    printf("Number of extracted k-mers is %d.\n", nb_kmers);
}
