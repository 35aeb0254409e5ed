// bft_seqfile.h -- plain-text FASTA / four-line FASTQ reader (host code, no GPU call): the file's sequences as one ASCII blob and nb_seqs + 1 offsets,
// the layout of bft_gpu_insert_sequences.
#pragma once
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define BFT_SEQFILE_OK 0
#define BFT_SEQFILE_E_IO (-1)      /* the file cannot be opened or read */
#define BFT_SEQFILE_E_FORMAT (-2)  /* neither '>' nor '@' first, a malformed or truncated FASTQ record */
/* The format is decided by the first non-blank character: '>' FASTA (header line, then sequence lines joined up to the next line that starts with
 * '>'), '@' FASTQ (header, ONE sequence line, a line that starts with '+', one quality line -- which may be empty for an empty sequence, but not
 * missing).  CR LF is tolerated (a CR in front of a line feed or at the end of the file is dropped), a last line needs no line feed, empty
 * records are kept as sequences of length 0, an empty (or all-blank) file gives zero sequences.  No gzip.  *blob and *offsets are malloc'ed
 * (free() them, or bft_seqfile_free); on an error nothing is allocated.  The characters are not interpreted: what is not ACGTU is the kernels' business. */
int bft_seqfile_read(const char* path, char** blob, uint64_t** offsets, uint64_t* nb_seqs);
/* The same with the records' names: the header line behind '>' / '@' up to the first blank or tab; an empty name becomes the record's ordinal in the
 * file, counted from 0 (the sequence index of the calls that take the blob).  *names holds them one after the other, each ended by a NUL,
 * *name_offsets nb_seqs + 1 offsets into it (name i starts at name_offsets[i]); both are malloc'ed (free() them). */
int bft_seqfile_read_named(const char* path, char** blob, uint64_t** offsets, char** names, uint64_t** name_offsets, uint64_t* nb_seqs);
void bft_seqfile_free(char* blob, uint64_t* offsets);
#ifdef __cplusplus
}
#endif
