// bft_seqfile.cpp -- plain-text FASTA / four-line FASTQ reader (bft_seqfile.h).  Host code only.
#include "bft_seqfile.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace {
// the line that starts at `at` (at < n): [at, end) without its line feed and without a CR in front of it; *next = the start of the next line
inline size_t line_end(const char* d, size_t n, size_t at, size_t* next) {
    const char* nl = (const char*)memchr(d + at, '\n', n - at);
    size_t end = nl ? (size_t)(nl - d) : n;
    *next = nl ? end + 1 : n;
    if (end > at && d[end - 1] == '\r') end--;
    return end;
}
int read_all(const char* path, std::string& out) {
    FILE* f = fopen(path, "rb");
    if (!f) return BFT_SEQFILE_E_IO;
    char buf[1 << 16];
    size_t got;
    while ((got = fread(buf, 1, sizeof(buf), f)) > 0) out.append(buf, got);
    const bool bad = ferror(f) != 0;
    fclose(f);
    return bad ? BFT_SEQFILE_E_IO : BFT_SEQFILE_OK;
}
}  // namespace

namespace {
// the name of the record whose header line is [at, end): what follows '>' / '@' up to the first blank; an empty one becomes the record's ordinal
void add_name(const char* d, size_t at, size_t end, std::string* names, std::vector<uint64_t>* name_off) {
    if (!names) return;
    size_t e = at + 1;
    while (e < end && d[e] != ' ' && d[e] != '\t') e++;
    if (e > at + 1) names->append(d + at + 1, e - at - 1);
    else names->append(std::to_string(name_off->size() - 1));
    names->push_back('\0');
    name_off->push_back(names->size());
}

// the reader behind both entry points; names / name_off: null, or the records' names, each ended by a NUL, and nb_seqs + 1 offsets into them
int read_records(const char* path, char** blob, uint64_t** offsets, uint64_t* nb_seqs, std::string* names, std::vector<uint64_t>* name_off) {
    std::string data;
    const int rc = read_all(path, data);
    if (rc != BFT_SEQFILE_OK) return rc;
    const char* d = data.data();
    const size_t n = data.size();
    std::string seqs;
    std::vector<uint64_t> off(1, 0);
    size_t at = 0;
    while (at < n && (d[at] == ' ' || d[at] == '\t' || d[at] == '\r' || d[at] == '\n')) at++;
    if (at < n) {
        if (d[at] == '>') {
            seqs.reserve(n - at);
            bool open = false;
            while (at < n) {
                size_t next;
                const size_t end = line_end(d, n, at, &next);
                if (d[at] == '>') {  // (at < n: d[at] is the line's first character, or its line feed)
                    if (open) off.push_back(seqs.size());
                    open = true;
                    add_name(d, at, end, names, name_off);
                } else {
                    seqs.append(d + at, end - at);
                }
                at = next;
            }
            if (open) off.push_back(seqs.size());
        } else if (d[at] == '@') {
            seqs.reserve((n - at) / 2);
            while (at < n) {
                size_t next, end = line_end(d, n, at, &next);
                if (end == at) { at = next; continue; }  // blank lines between records
                if (d[at] != '@') return BFT_SEQFILE_E_FORMAT;
                if (next >= n) return BFT_SEQFILE_E_FORMAT;  // no sequence line
                add_name(d, at, end, names, name_off);
                at = next;
                end = line_end(d, n, at, &next);
                const size_t s0 = at, s1 = end;
                if (next >= n) return BFT_SEQFILE_E_FORMAT;  // no '+' line
                at = next;
                end = line_end(d, n, at, &next);
                if (end == at || d[at] != '+') return BFT_SEQFILE_E_FORMAT;
                // the quality line: it must be there -- begun, or announced by the line feed that ends the '+' line -- and as long as the sequence
                const bool plus_ended = next > end && d[next - 1] == '\n';
                if (!plus_ended) return BFT_SEQFILE_E_FORMAT;
                at = next;
                size_t q0 = at, q1 = at;
                if (at < n) { q1 = line_end(d, n, at, &next); at = next; }
                if (q1 - q0 != s1 - s0) return BFT_SEQFILE_E_FORMAT;
                seqs.append(d + s0, s1 - s0);
                off.push_back(seqs.size());
            }
        } else {
            return BFT_SEQFILE_E_FORMAT;
        }
    }
    char* b = (char*)malloc(seqs.size() ? seqs.size() : 1);
    uint64_t* o = (uint64_t*)malloc(off.size() * sizeof(uint64_t));
    if (!b || !o) { free(b); free(o); return BFT_SEQFILE_E_IO; }
    if (!seqs.empty()) memcpy(b, seqs.data(), seqs.size());
    memcpy(o, off.data(), off.size() * sizeof(uint64_t));
    *blob = b;
    *offsets = o;
    *nb_seqs = off.size() - 1;
    return BFT_SEQFILE_OK;
}

}  // namespace

extern "C" int bft_seqfile_read(const char* path, char** blob, uint64_t** offsets, uint64_t* nb_seqs) {
    if (!path || !blob || !offsets || !nb_seqs) return BFT_SEQFILE_E_IO;
    *blob = nullptr;
    *offsets = nullptr;
    *nb_seqs = 0;
    return read_records(path, blob, offsets, nb_seqs, nullptr, nullptr);
}

extern "C" int bft_seqfile_read_named(const char* path, char** blob, uint64_t** offsets, char** names, uint64_t** name_offsets, uint64_t* nb_seqs) {
    if (!path || !blob || !offsets || !names || !name_offsets || !nb_seqs) return BFT_SEQFILE_E_IO;
    *blob = nullptr;
    *offsets = nullptr;
    *names = nullptr;
    *name_offsets = nullptr;
    *nb_seqs = 0;
    std::string nm;
    std::vector<uint64_t> no(1, 0);
    const int rc = read_records(path, blob, offsets, nb_seqs, &nm, &no);
    if (rc != BFT_SEQFILE_OK) return rc;
    char* b = (char*)malloc(nm.size() ? nm.size() : 1);
    uint64_t* o = (uint64_t*)malloc(no.size() * sizeof(uint64_t));
    if (!b || !o || no.size() != *nb_seqs + 1) {
        free(b);
        free(o);
        bft_seqfile_free(*blob, *offsets);
        *blob = nullptr;
        *offsets = nullptr;
        *nb_seqs = 0;
        return BFT_SEQFILE_E_IO;
    }
    if (!nm.empty()) memcpy(b, nm.data(), nm.size());
    memcpy(o, no.data(), no.size() * sizeof(uint64_t));
    *names = b;
    *name_offsets = o;
    return BFT_SEQFILE_OK;
}

extern "C" void bft_seqfile_free(char* blob, uint64_t* offsets) {
    free(blob);
    free(offsets);
}
