"""Insertion from sequences (bft_gpu_insert_sequences, csrc/bft_ingest.hip): the ground truth, the case generator that
tests/test_gpu_ingest.py runs on the GPU, and -- here, without a GPU -- the proof that every case is what its name says, plus the tests of the
FASTA / FASTQ reader (csrc/bft_seqfile.cpp), which is host code.

Truth, in plain Python (nothing of the library's): every window of k characters of every sequence; a window with a byte outside ACGTUacgtu is
skipped; the k-mer is the window upper-cased with U -> T, or -- canonical -- the smaller of that string and its reverse complement by string
comparison; counts come from a dictionary.  It is pinned against the project's own packing (bft_hosttest_roundtrip) at one k per key width.

Tile and chunk sizes are read from the library (bft_gpu_debug_ingest_plan / bft_gpu_debug_ingest_chunks: csrc/bft_ingest.h, no device needed).

A note on "the deciding nucleotide": a k-mer x and its reverse complement r satisfy r[i] = comp(x[k - 1 - i]), so x[i] != r[i] implies
x[k - 1 - i] != r[k - 1 - i]: the FIRST differing position, which decides the string comparison, is always below k / 2.  With W >= 2 words of
32 nucleotides it therefore never lies in the last word.  The cases put it at position 0 (word 0) and at the last position it can take, the
largest i below k / 2, which is in the highest word it can reach."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from bloomfiltertrie_amd import _lib, synth as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VALID = b"ACGTUacgtu"
_NORM = bytearray(b"N" * 256)
for _a, _b in zip(VALID, b"ACGTTACGTT"):
    _NORM[_a] = _b
_NORM = bytes(_NORM)
_COMP = str.maketrans("ACGT", "TGCA")
KEYS = (9, 27, 31, 32, 33, 63, 64, 72, 126)  # W = 1 .. 4; 2k % 64 == 0 at 32 and 64 (dn == 0 in the reverse complement)


def words(k):
    return (2 * k + 63) // 64


def plan():
    """(tile, default chunk, minimum chunk) from the library"""
    out = (C.c_uint64 * 3)()
    assert _lib.load().bft_gpu_debug_ingest_plan(out) == 0
    return int(out[0]), int(out[1]), int(out[2])


def chunks(lengths, k, chunk_chars):
    """[(first char, end char, pieces)] of the host form's chunks for sequences of these lengths"""
    off = np.zeros(len(lengths) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lengths)
    n = C.c_uint64()
    lib = _lib.load()
    assert lib.bft_gpu_debug_ingest_chunks(off.ctypes.data, len(lengths), k, chunk_chars, None, 0, C.byref(n)) == 0
    out = np.zeros(3 * max(n.value, 1), dtype=np.uint64)
    assert lib.bft_gpu_debug_ingest_chunks(off.ctypes.data, len(lengths), k, chunk_chars, out.ctypes.data, n.value, C.byref(n)) == 0
    return [tuple(int(x) for x in out[3 * i:3 * i + 3]) for i in range(n.value)]


# ---- truth -----------------------------------------------------------------------------------------------------------------------------------
def normalise(seq):
    return bytes(seq).translate(_NORM).decode("ascii")


def revcomp(x):
    return x[::-1].translate(_COMP)


def canon(x):
    r = revcomp(x)
    return r if x >= r else x  # strcmp(kmer, revcomp) >= 0: the reverse complement (src/bft.c:1290-1296)


class Truth:
    """positions, skipped, distinct, appended as stats[4] reports them; `kmers`: what is appended, in order (stream path: every valid window,
    duplicates included; counting path: each kept k-mer once); `valid`: one flag per position, in position order"""

    def __init__(self, seqs, k, canonical, min_abundance):
        self.valid, sel, self._packed = [], [], None
        for s in seqs:
            r = normalise(s)
            for i in range(max(len(r) - k + 1, 0)):
                x = r[i:i + k]
                ok = "N" not in x
                self.valid.append(ok)
                if ok:
                    sel.append(canon(x) if canonical else x)
        self.positions, self.skipped = len(self.valid), len(self.valid) - len(sel)
        self.counts = {}
        if min_abundance == 0:
            self.kmers, self.distinct = sel, 0
        else:
            for x in sel:
                self.counts[x] = self.counts.get(x, 0) + 1
            self.kmers, self.distinct = [x for x, c in self.counts.items() if c >= min_abundance], len(self.counts)
        self.appended = len(self.kmers)

    def stats(self):
        return {"positions": self.positions, "skipped": self.skipped, "distinct": self.distinct, "appended": self.appended}

    def packed(self, k):
        """the appended k-mers in the reference's packed layout (computed once)"""
        if self._packed is None:
            codes = S._CODE[np.frombuffer("".join(self.kmers).encode(), dtype=np.uint8)].reshape(len(self.kmers), k)
            assert codes.max(initial=0) < 4
            self._packed = np.ascontiguousarray(S.pack_codes(codes)) if len(codes) else np.zeros((0, S.kmer_bytes(k)), np.uint8)
        return self._packed


class Case:
    def __init__(self, name, k, seqs, canonical=False, min_abundance=0):
        self.name, self.k, self.seqs, self.canonical, self.min_abundance = name, k, [bytes(s) for s in seqs], bool(canonical), int(min_abundance)
        self._truth = None

    @property
    def truth(self):  # computed once, shared by every test that needs it
        if self._truth is None:
            self._truth = Truth(self.seqs, self.k, self.canonical, self.min_abundance)
        return self._truth

    def starts(self):
        return np.concatenate([[0], np.cumsum([len(s) for s in self.seqs])]).astype(np.int64)

    def __repr__(self):
        return self.name


def rand_text(n, rng):
    return bytes(S._ASCII[rng.integers(0, 4, n).astype(np.uint8)])


def mixed(t, rng):
    out = bytearray(t)
    for i, c in enumerate(out):
        if c == ord("T") and rng.random() < 0.5:
            c = ord("U")
        out[i] = c | 0x20 if rng.random() < 0.5 else c
    return bytes(out)


def with_bad(t, at, ch=b"N"):
    out = bytearray(t)
    for a in np.atleast_1d(at):
        out[int(a)] = ch[0]
    return bytes(out)


# ---- the cases -------------------------------------------------------------------------------------------------------------------------------
def geometry_cases(k):
    rng = np.random.default_rng(1000 + k)
    out = []
    out.append(Case(f"lengths-k{k}", k, [rand_text(n, rng) for n in (0, k - 1, k, k + 1, 0, k + 1, k, k - 1, 0)]))
    ln = k + ((1 - k) % 32)  # >= k and = 1 mod 32: 33 sequences start at every c0 % 32
    out.append(Case(f"c0mod32-k{k}", k, [rand_text(ln, rng) for _ in range(33)]))
    out.append(Case(f"c0mod32-canonical-k{k}", k, [rand_text(ln, rng) for _ in range(33)], canonical=True))
    # a bad character as the first and as the last character of a window; one in every 32-character word of a sequence that starts on a word
    L = ((k + 31) // 32 + 2) * 32
    seqs = [with_bad(rand_text(2 * k + 1, rng), k)]
    seqs[0] += rand_text((-len(seqs[0])) % 32, rng)  # (the sequences behind it start on a word: their length is a multiple of 32)
    seqs += [with_bad(rand_text(L, rng), 32 * j) for j in range(L // 32)]  # (a word's first character: the last word of a window may hold no other)
    out.append(Case(f"bad-edges-k{k}", k, seqs))
    out.append(Case(f"n-runs-k{k}", k, [rand_text(2 * k, rng) + b"N" * (k + 5) + rand_text(k + 3, rng) + b"n" * (3 * k) + rand_text(k, rng), b"N" * (k + 10)]))
    out.append(Case(f"case-u-k{k}", k, [mixed(rand_text(300, rng), rng), mixed(rand_text(k, rng), rng)], canonical=bool(k & 1)))
    mid = rand_text(k, rng)
    out.append(Case(f"all-bytes-k{k}", k, [with_bad(mid, k // 2, bytes([b])) for b in range(256)]))
    return out


def compaction_cases(k):
    tile = plan()[0]
    rng = np.random.default_rng(2000 + k)
    out = [Case(f"valid-{v}-k{k}", k, [rand_text(v + k - 1, rng)] if v else [b"N" * (k + 10)]) for v in sorted({0, 1, 63, 64, 65, tile - 1, tile, tile + 1})]
    if k <= tile:  # positions [tile, 2 tile) all invalid between two full tiles: bad characters at [tile + k - 1, 2 tile)
        out.append(Case(f"empty-tile-k{k}", k, [with_bad(rand_text(3 * tile + k - 1, rng), np.arange(tile + k - 1, 2 * tile))]))
    out.append(Case(f"alternating-k{k}", k, [rand_text(k, rng) if i % 2 == 0 else with_bad(rand_text(k, rng), int(rng.integers(0, k))) for i in range(3 * tile + 5)]))
    reads = []
    for i in range(5000):
        r = rand_text(int(rng.integers(1, 201)), rng)
        if i % 7 == 0:
            r = with_bad(r, int(rng.integers(0, len(r))))
        reads.append(r)
    out.append(Case(f"reads5000-k{k}", k, reads))
    return out


def canonical_cases(k):
    rng = np.random.default_rng(3000 + k)

    def deciding_at(j, smaller):
        """a k-mer that agrees with its reverse complement below position j and is smaller / larger there"""
        while True:
            x = bytearray(rand_text(k, rng))
            for i in range(j):
                x[k - 1 - i] = ord(chr(x[i]).translate(_COMP))
            x = x.decode()
            r = revcomp(x)
            if x[:j] == r[:j] and x[j] != r[j] and (x[j] < r[j]) == smaller:
                return x.encode()

    seqs = []
    if k % 2 == 0:
        h = rand_text(k // 2, rng).decode()
        seqs.append((h + revcomp(h)).encode())  # a palindrome: its own reverse complement
    jl = (k - 1) // 2 if k % 2 else k // 2 - 1  # the last position that can decide
    for j in (0, jl):
        seqs += [deciding_at(j, True), deciding_at(j, False)]
    x = rand_text(k, rng)
    seqs += [x, revcomp(x.decode()).encode()]  # a k-mer and its reverse complement in different sequences
    seqs.append(rand_text(3 * k, rng))
    return [Case(f"canonical-k{k}", k, seqs, canonical=True), Case(f"canonical-off-k{k}", k, seqs, canonical=False)]


def counting_cases(k, full=True):
    rng = np.random.default_rng(4000 + k)
    out = []
    for c in ((1, 2, 3) if full else (2,)):
        below, at, above = rand_text(k, rng), rand_text(k, rng), rand_text(k, rng)
        seqs = [below] * (c - 1) + [at] * c + [above] * (c + 1) + [rand_text(k + 30, rng)]
        order = rng.permutation(len(seqs))
        out.append(Case(f"count-c{c}-k{k}", k, [seqs[i] for i in order], min_abundance=c))
        out.append(Case(f"count-c{c}-canonical-k{k}", k, [seqs[i] for i in order] + [revcomp(at.decode()).encode()], canonical=True, min_abundance=c))
    if full:
        out.append(Case(f"count-above-all-k{k}", k, [rand_text(200, rng), rand_text(k, rng)] * 2, min_abundance=1000))
        out.append(Case(f"count-polyA-k{k}", k, [rand_text(k + 20, rng), b"A" * (5000 + k - 1), rand_text(k + 20, rng)], min_abundance=2))
        out.append(Case(f"count-polyA-canonical-k{k}", k, [rand_text(k + 20, rng), b"A" * (5000 + k - 1), b"T" * (k + 2), rand_text(k + 20, rng)], canonical=True, min_abundance=5003))
        x = canonical_cases(k)[0].seqs[-4]  # (deciding_at(jl, ...): differs from its reverse complement)
        strands = [x, revcomp(x.decode()).encode()]
        out.append(Case(f"count-strands-canonical-k{k}", k, strands, canonical=True, min_abundance=2))
        out.append(Case(f"count-strands-k{k}", k, strands, canonical=False, min_abundance=2))
        reads = [rand_text(int(rng.integers(1, 120)), rng) for _ in range(300)]
        out.append(Case(f"count-reads-k{k}", k, reads + reads[::2] + reads[::3], min_abundance=2))
    return out


def chunk_cases(k):
    cmin = plan()[2]
    rng = np.random.default_rng(5000 + k)
    long_seq = rand_text(20000, rng)
    return [Case(f"chunk-long-k{k}", k, [long_seq]),
            Case(f"chunk-long-canonical-k{k}", k, [long_seq], canonical=True),
            Case(f"chunk-edge-at-k{k}", k, [rand_text(cmin - 500, rng), rand_text(500, rng), rand_text(300, rng)]),
            Case(f"chunk-edge-before-k{k}", k, [rand_text(cmin - 1, rng), rand_text(300, rng)]),
            Case(f"chunk-edge-after-k{k}", k, [rand_text(cmin + 1, rng), rand_text(300, rng)]),
            Case(f"chunk-bad-in-overlap-k{k}", k, [with_bad(rand_text(3 * cmin, rng), [cmin - 2, 2 * cmin - (k - 1) - 2])])]


def all_cases():
    out = []
    for k in KEYS:
        out += geometry_cases(k) + canonical_cases(k)
    for k in (27, 33):
        out += compaction_cases(k)
    for k in (27, 63):
        out += counting_cases(k, True)
    for k in (72, 126):
        out += counting_cases(k, False)
    for k in (27, 63):
        out += chunk_cases(k)
    return out


CASES = all_cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


# ---- the truth is pinned against the project's own packing ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hostlib():
    subprocess.check_call(["make", "-C", _lib.CSRC, "all"], stdout=subprocess.DEVNULL)
    lib = C.CDLL(os.path.join(_lib.CSRC, "libbft_hosttest.so"))
    lib.bft_hosttest_roundtrip.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p]
    return lib


@pytest.mark.parametrize("k", [27, 63, 72, 126])
def test_truth_kmers_survive_the_projects_codec(hostlib, k):
    assert words(k) == {27: 1, 63: 2, 72: 3, 126: 4}[k]
    rng = np.random.default_rng(k)
    seqs = [mixed(rand_text(400, rng), rng), with_bad(rand_text(3 * k, rng), k + 1)]
    for canonical in (False, True):
        t = Truth(seqs, k, canonical, 0)
        km = t.packed(k)
        out = np.zeros_like(km)
        tf = np.zeros((len(km), words(k)), dtype=np.uint64)
        hostlib.bft_hosttest_roundtrip(km.ctypes.data, len(km), k, out.ctypes.data, tf.ctypes.data)
        assert (out == km).all()
        assert [x.decode() if isinstance(x, bytes) else x for x in S.packed_to_ascii(out, k)] == t.kmers
        # packed layout (src/fasta.c:11-23): nucleotide i at bits 2 (i % 4) of byte i / 4, A C G T = 0 1 2 3
        for x, row in list(zip(t.kmers, km))[:20]:
            assert ["ACGT"[(row[i // 4] >> (2 * (i % 4))) & 3] for i in range(k)] == list(x)


def test_truth_rules():
    assert canon("ACGT") == "ACGT" and revcomp("ACGT") == "ACGT"            # a palindrome
    assert canon("TTTT") == "AAAA" and canon("AAAA") == "AAAA"
    assert canon("CA") == "CA" and canon("TG") == "CA"                      # revcomp(TG) = CA
    t = Truth([b"ACGTNACGT", b"acgu", b"AC"], 4, False, 0)
    assert t.stats() == {"positions": 7, "skipped": 4, "distinct": 0, "appended": 3} and t.kmers == ["ACGT", "ACGT", "ACGT"]
    t = Truth([b"ACGTNACGT", b"acgu", b"AC"], 4, False, 3)
    assert t.stats() == {"positions": 7, "skipped": 4, "distinct": 1, "appended": 1}
    t = Truth([b"AAAC", b"GTTT"], 4, True, 2)
    assert t.kmers == ["AAAC"] and Truth([b"AAAC", b"GTTT"], 4, False, 2).kmers == []
    for b in range(256):
        assert (normalise(bytes([b])) != "N") == (bytes([b]) in [VALID[i:i + 1] for i in range(10)])


def test_plan_constants_match_the_header():
    tile, dflt, cmin = plan()
    txt = open(os.path.join(_lib.CSRC, "bft_ingest.h")).read()
    assert int(re.search(r"BFT_ING_TILE = (\d+);", txt).group(1)) == tile == 64
    assert re.search(r"BFT_ING_CHUNK_DEFAULT = \(uint64_t\)1 << (\d+);", txt).group(1) == str(dflt.bit_length() - 1) and dflt == 1 << (dflt.bit_length() - 1)
    assert int(re.search(r"BFT_ING_CHUNK_MIN = (\d+);", txt).group(1)) == cmin == 1024
    hdr = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER).read(), flags=re.S)
    for name in ("bft_gpu_insert_sequences", "bft_gpu_insert_sequences_dev", "bft_gpu_insert_sequence_file", "bft_gpu_debug_ingest_plan", "bft_gpu_debug_ingest_chunks"):
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in _lib.SIGNATURES


def test_chunk_plan_covers_every_window_once():
    """every window of every sequence lies in exactly one piece of one chunk, whatever the chunk size"""
    rng = np.random.default_rng(7)
    for k, csize in ((27, 1024), (63, 1024), (126, 1024), (27, 4096)):
        lengths = [int(x) for x in rng.integers(0, 3000, 40)] + [20000, 0, k - 1, k, 1024, 1023, 1025]
        ch = chunks(lengths, k, csize)
        assert all(c1 - c0 <= csize for c0, c1, _ in ch)
        starts = np.concatenate([[0], np.cumsum(lengths)])
        want = sum(max(n - k + 1, 0) for n in lengths)
        # windows of a chunk: those that lie inside it and inside one sequence, minus those the chunk before already held (the overlap)
        seen = set()
        got = 0
        for c0, c1, _ in ch:
            for s, n in zip(starts[:-1], lengths):
                a, b = max(c0, int(s)), min(c1, int(s) + n)
                for w in range(a, b - k + 1):
                    if w not in seen:
                        seen.add(w)
                        got += 1
        assert got == want == len(seen)
        for (a0, a1, _), (b0, b1, _) in zip(ch, ch[1:]):
            assert b0 in (a1, a1 - (k - 1))  # the next chunk starts at the cut, or k - 1 characters before it


# ---- every case is what its name says ---------------------------------------------------------------------------------------------------
def test_key_widths():
    assert sorted({words(k) for k in KEYS}) == [1, 2, 3, 4]
    assert {k for k in KEYS if (2 * k) % 64 == 0} == {32, 64} and any((2 * k) % 64 for k in KEYS)


@pytest.mark.parametrize("k", KEYS)
def test_geometry_cases(k):
    c = BY_NAME[f"lengths-k{k}"]
    assert sorted({len(s) for s in c.seqs}) == [0, k - 1, k, k + 1] and c.truth.positions == 2 + 2 * 2
    for name in (f"c0mod32-k{k}", f"c0mod32-canonical-k{k}"):
        c = BY_NAME[name]
        assert {int(s) % 32 for s in c.starts()[:-1]} == set(range(32)) and all(len(s) >= k for s in c.seqs)  # sh == 0 and sh == 62 occur
    c = BY_NAME[f"bad-edges-k{k}"]
    st = c.starts()
    blob = normalise(b"".join(c.seqs))
    first = last = False
    touched = set()
    for s, seq in zip(st[:-1], c.seqs):
        for i in range(max(len(seq) - k + 1, 0)):
            w = blob[s + i:s + i + k]
            if w.count("N") == 1:
                first |= w[0] == "N"
                last |= w[-1] == "N"
                touched.add((int(s) + i + w.index("N")) // 32 - (int(s) + i) // 32)  # which of the window's `bad` words holds it
    assert first and last and touched == set(range((k + 30) // 32 + 1))
    c = BY_NAME[f"n-runs-k{k}"]
    assert max(len(m.group()) for m in re.finditer("N+", normalise(c.seqs[0]))) > k and 0 < c.truth.appended < c.truth.positions
    c = BY_NAME[f"case-u-k{k}"]
    raw = b"".join(c.seqs)
    assert any(ch in raw for ch in b"acgt") and (b"U" in raw or b"u" in raw) and c.truth.skipped == 0
    c = BY_NAME[f"all-bytes-k{k}"]
    assert [s[k // 2] for s in c.seqs] == list(range(256)) and c.truth.positions == 256 and c.truth.appended == 10


@pytest.mark.parametrize("k", (27, 33))
def test_compaction_cases(k):
    tile = plan()[0]
    for v in (0, 1, 63, 64, 65, tile - 1, tile, tile + 1):
        assert BY_NAME[f"valid-{v}-k{k}"].truth.appended == v
    assert BY_NAME[f"valid-0-k{k}"].truth.positions > 0
    if k <= tile:
        v = BY_NAME[f"empty-tile-k{k}"].truth.valid
        assert [sum(v[i:i + tile]) for i in range(0, len(v), tile)] == [tile, 0, tile]
    v = BY_NAME[f"alternating-k{k}"].truth.valid
    assert len(v) > 3 * tile and all(a != b for a, b in zip(v, v[1:])) and len(v) % tile  # ... and a ragged last wavefront
    c = BY_NAME[f"reads5000-k{k}"]
    lens = [len(s) for s in c.seqs]
    assert len(lens) == 5000 and min(lens) == 1 and max(lens) == 200 and sum(n < k for n in lens) > 100 and c.truth.skipped > 0 and c.truth.positions % tile


@pytest.mark.parametrize("k", KEYS)
def test_canonical_cases(k):
    c, off = BY_NAME[f"canonical-k{k}"], BY_NAME[f"canonical-off-k{k}"]
    xs = [normalise(s) for s in c.seqs if len(s) == k]
    if k % 2 == 0:
        assert any(x == revcomp(x) for x in xs)
    decide = lambda x: next(i for i in range(k) if x[i] != revcomp(x)[i])
    where = {(decide(x), x < revcomp(x)) for x in xs if x != revcomp(x)}
    jl = (k - 1) // 2 if k % 2 else k // 2 - 1
    assert {(0, True), (0, False), (jl, True), (jl, False)} <= where
    assert jl // 32 == (k // 2 - 1 if k % 2 == 0 else (k - 1) // 2) // 32 and max(j for j, _ in where) < (k + 1) // 2  # (the module's note)
    assert any(revcomp(x) in xs and x != revcomp(x) for x in xs)
    assert set(c.truth.kmers) != set(off.truth.kmers) and all(x <= revcomp(x) for x in c.truth.kmers)


@pytest.mark.parametrize("k,full", ((27, True), (63, True), (72, False), (126, False)))
def test_counting_cases(k, full):
    for cmin in ((1, 2, 3) if full else (2,)):
        c = BY_NAME[f"count-c{cmin}-k{k}"]
        assert c.min_abundance == cmin and {cmin - 1, cmin, cmin + 1} - {0} <= set(c.truth.counts.values())
        assert all(v >= cmin for x, v in c.truth.counts.items() if x in c.truth.kmers) and c.truth.appended < c.truth.distinct + (cmin == 1)
        cc = BY_NAME[f"count-c{cmin}-canonical-k{k}"]
        assert cmin + 1 in cc.truth.counts.values() and cc.canonical
    if not full:
        return
    c = BY_NAME[f"count-above-all-k{k}"]
    assert c.truth.appended == 0 and c.truth.distinct > 0 and max(c.truth.counts.values()) < c.min_abundance
    c = BY_NAME[f"count-polyA-k{k}"]
    assert c.truth.counts["A" * k] == 5000 and c.truth.kmers == ["A" * k] and c.truth.distinct > 40
    c = BY_NAME[f"count-polyA-canonical-k{k}"]
    assert c.truth.counts["A" * k] == 5003 and c.truth.kmers == ["A" * k]  # both strands count together: 5000 + 3 windows of the poly-T
    a, b = BY_NAME[f"count-strands-canonical-k{k}"], BY_NAME[f"count-strands-k{k}"]
    assert a.seqs == b.seqs and a.truth.appended == 1 and b.truth.appended == 0 and b.truth.distinct == 2
    c = BY_NAME[f"count-reads-k{k}"]
    assert 0 < c.truth.appended < c.truth.distinct and c.truth.positions > 4 * plan()[0]


@pytest.mark.parametrize("k", (27, 63))
def test_chunk_cases(k):
    cmin = plan()[2]
    assert [len(s) for s in BY_NAME[f"chunk-long-k{k}"].seqs] == [20000]
    assert len(chunks([20000], k, cmin)) > 19
    ends = lambda name: np.cumsum([len(s) for s in BY_NAME[name].seqs]).tolist()
    assert cmin in ends(f"chunk-edge-at-k{k}") and cmin - 1 in ends(f"chunk-edge-before-k{k}") and cmin + 1 in ends(f"chunk-edge-after-k{k}")
    c = BY_NAME[f"chunk-bad-in-overlap-k{k}"]
    ch = chunks([len(c.seqs[0])], k, cmin)
    bad = [i for i, x in enumerate(normalise(c.seqs[0])) if x == "N"]
    overlaps = [(b0, a1) for (a0, a1, _), (b0, b1, _) in zip(ch, ch[1:])]
    assert all(a1 - b0 == k - 1 for b0, a1 in overlaps) and all(any(b0 <= i < a1 for b0, a1 in overlaps) for i in bad) and len(bad) == 2


# ---- the reader ------------------------------------------------------------------------------------------------------------------------------
READER_FILES = {
    "multi.fa": (b">one desc\nACGT\nTTGA\n\n>two\nGG\n>three\n", [b"ACGTTTGA", b"GG", b""]),
    "crlf.fa": (b">a\r\nACGT\r\nNN\r\n>b\r\nTT\r\n", [b"ACGTNN", b"TT"]),
    "nonl.fa": (b">a\nACGT\n>b\nTTA", [b"ACGT", b"TTA"]),
    "blank_first.fa": (b"\n\n  \n>a\nAC\n", [b"AC"]),
    "reads.fq": (b"@r1\nACGT\n+\nIIII\n@r2 x\nGGN\n+r2\n@@@\n", [b"ACGT", b"GGN"]),  # (a quality line may start with '@')
    "crlf.fq": (b"@r1\r\nACGT\r\n+\r\nIIII\r\n", [b"ACGT"]),
    "nonl.fq": (b"@r1\nACGT\n+\nIIII", [b"ACGT"]),
    "empty_record.fq": (b"@r1\n\n+\n\n@r2\nAC\n+\nII\n", [b"", b"AC"]),
    "empty.fa": (b"", []),
    "blank.fa": (b"\n\r\n \n", []),
    "truncated.fq": (b"@r1\nACGT\n+\nIIII\n@r2\nACGT\n+\n", None),
    "truncated2.fq": (b"@r1\nACGT\n", None),
    "short_quality.fq": (b"@r1\nACGT\n+\nII\n", None),
    "neither.txt": (b"ACGT\n>a\nACGT\n", None),
}


def write_reader_files(d):
    for name, (data, _) in READER_FILES.items():
        with open(os.path.join(d, name), "wb") as f:
            f.write(data)


def _reader_program(tmp, flags, name):
    """tests/c/seqfile_main.c + csrc/bft_seqfile.cpp as a stand-alone program: prints 'rc n' and one line 'length:sequence' per sequence"""
    exe = os.path.join(tmp, name)
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", *flags, "-I", _lib.CSRC, "-x", "c++", os.path.join(ROOT, "tests", "c", "seqfile_main.c"),
           os.path.join(_lib.CSRC, "bft_seqfile.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    return (exe if r.returncode == 0 else None), r.stderr


def _run_reader(exe, path):
    r = subprocess.run([exe, path], capture_output=True)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
    lines = r.stdout.split(b"\n")
    rc, n = (int(x) for x in lines[0].split())
    seqs = []
    for ln in lines[1:1 + n]:
        length, _, s = ln.partition(b":")
        assert int(length) == len(s)
        seqs.append(s)
    return rc, seqs


@pytest.fixture(scope="module")
def reader_dir(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("seqfiles"))
    write_reader_files(d)
    return d


def test_reader(reader_dir):
    exe, err = _reader_program(reader_dir, [], "seqfile_plain")
    assert exe, err
    for name, (_, want) in READER_FILES.items():
        rc, seqs = _run_reader(exe, os.path.join(reader_dir, name))
        if want is None:
            assert rc == -2 and seqs == [], name
        else:
            assert rc == 0 and seqs == want, name
    assert _run_reader(exe, os.path.join(reader_dir, "does_not_exist.fa")) == (-1, [])


def test_reader_under_sanitizers(reader_dir):
    """the same files through the reader built with -fsanitize=address,undefined, as a program of its own (never loaded into Python)"""
    exe, err = _reader_program(reader_dir, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"], "seqfile_san")
    assert exe, "the sanitizer runtime does not link here:\n" + err[-2000:]
    for name, (_, want) in READER_FILES.items():
        rc, seqs = _run_reader(exe, os.path.join(reader_dir, name))  # (asserts a clean exit: a sanitizer report is a non-zero exit)
        assert (rc, seqs) == ((0, want) if want is not None else (-2, [])), name
