"""CPU-side tests (no GPU) of the case sets that tests/test_gpu_sequences.py runs through the sequence queries (k_seq_encode, k_seq_plan,
k_seq_tiles, k_seq_kh / k_seq_walk8 / k_seq_walk6, k_seq_tally: csrc/bft_kernels_seq.h, csrc/bft_kernels_seqwin.h, csrc/bft_kh.hip).
Every generator and the ground truth live here, so that a machine without a GPU can check that the cases still reach what they are there
for: a read that starts at position 64 t, a run of one colour set across lane 63, a count of exactly the threshold.  The truth is plain
Python over a dict {k-mer string: set of genome ids} of what was inserted; it calls neither the oracle nor the library.  Where the oracle
can answer (ASCII reads without a NUL, sets of at most 4096 ids, the small cases) the truth is compared with it."""
import math
from fractions import Fraction

import numpy as np
import pytest

from bloomfiltertrie_amd import synth as S

VALID = b"ACGTUacgtu"  # the ten bytes that count as a nucleotide (nt_code)
_NORM = bytearray(b"N" * 256)
for _a, _b in zip(VALID, b"ACGTTACGTT"):
    _NORM[_a] = _b
_NORM = bytes(_NORM)
_COMP = str.maketrans("ACGT", "TGCA")
TILE, TURN, TALLY_G, TALLY_STRIDE = 64, 128, 2048, 4096 * 4  # positions per tile / per tally turn, genomes per tally window, reads per tally sweep


def text(codes):
    return bytes(S._ASCII[np.asarray(codes, dtype=np.uint8)]).decode()


def rand_text(n, rng):
    return text(rng.integers(0, 4, n))


def revcomp(x):
    return x[::-1].translate(_COMP)


def canon(x):
    return min(x, revcomp(x))


def normalise(read):
    """upper case, U -> T, every other byte -> N.  Mixed-case reads are compared upper-cased: the project's stated choice (oracle/bft_oracle.c,
    orc_query_sequence), which the truth follows."""
    return bytes(read).translate(_NORM).decode("ascii")


def mixed(t, rng):
    """the text in random case, every T at random as U"""
    out = bytearray(t.encode())
    for i, c in enumerate(out):
        if c == ord("T") and rng.random() < 0.5:
            c = ord("U")
        out[i] = c | 0x20 if rng.random() < 0.5 else c
    return bytes(out)


class Stored:
    """What is inserted: {k-mer string: set of genome ids}"""

    def __init__(self, k):
        self.k, self.sets = k, {}

    def add_kmer(self, x, ids):
        assert len(x) == self.k
        self.sets.setdefault(x, set()).update(int(g) for g in ids)

    def add(self, seq, ids, canonical=True):
        """every k-mer of seq (its canonical form: the smaller of the k-mer and its reverse complement)"""
        for i in range(len(seq) - self.k + 1):
            x = seq[i:i + self.k]
            self.add_kmer(canon(x) if canonical else x, ids)

    def n_genomes(self):
        return 1 + max(max(v) for v in self.sets.values())

    def phases(self):
        """insert calls genome by genome, ascending: [(genome id, packed k-mers)]"""
        by = {}
        for x, ids in self.sets.items():
            for g in ids:
                by.setdefault(g, []).append(x)
        out = []
        for g in sorted(by):
            packed, valid = S.ascii_to_packed(by[g], self.k)
            assert valid.all()
            out.append((g, np.ascontiguousarray(packed)))
        return out


def counts(st, read, canonical):
    """(m, {genome: k-mers of the read it holds}): m = max(len - k + 1, 0) windows, those with a byte outside ACGTUacgtu skipped"""
    r, k = normalise(read), st.k
    m = max(len(r) - k + 1, 0)
    cnt = {}
    for i in range(m):
        x = r[i:i + k]
        if "N" in x:
            continue
        for g in st.sets.get(canon(x) if canonical else x, ()):
            cnt[g] = cnt.get(g, 0) + 1
    return m, cnt


def answer(m, cnt, thr):
    """cnt > 0 and cnt >= ceil(m * thr), the product taken in double (reference src/bft.c:1279-1281)"""
    minv = math.ceil(m * thr)
    return sorted(g for g, c in cnt.items() if c > 0 and c >= minv)


class Case:
    """One batch: the index content, the reads (bytes), and the thresholds to ask per strand mode {canonical: [thresholds]}"""

    def __init__(self, stored, reads, thresholds, canonicals=(False, True)):
        self.stored, self.reads = stored, [bytes(r) for r in reads]
        self.thresholds = thresholds if isinstance(thresholds, dict) else {c: list(thresholds) for c in canonicals}
        self._counts = {}

    def counts(self, canonical):
        if canonical not in self._counts:
            self._counts[canonical] = [counts(self.stored, r, canonical) for r in self.reads]
        return self._counts[canonical]

    def truth(self, thr, canonical):
        return [answer(m, cnt, thr) for m, cnt in self.counts(canonical)]

    def runs(self):
        """(canonical, threshold) pairs in a fixed order"""
        return [(c, t) for c in sorted(self.thresholds) for t in self.thresholds[c]]


def oracle_agrees(oracle_mod, case, max_reads=400):
    """truth == oracle on the reads the oracle can take (it reads a C string and decodes at most 4096 ids per set)"""
    st = case.stored
    assert max(len(v) for v in st.sets.values()) <= 4096
    o = oracle_mod.OracleBFT(st.k)
    for g, packed in st.phases():
        o.insert_kmers(packed, g)
    G = st.n_genomes()
    idx = [i for i, r in enumerate(case.reads) if r and all(0 < b < 128 for b in r)]
    step = max(1, len(idx) // max_reads)
    n = 0
    for canonical, thr in case.runs():
        want = case.truth(thr, canonical)
        for i in idx[::step]:
            assert o.query_sequence(case.reads[i].decode("ascii"), thr, canonical, G) == want[i], (i, canonical, thr)
            n += 1
    o.close()
    return n


# ---- 1. the encoder's byte table ---------------------------------------------------------------------------------------------------------
ENCODER_KS = (9, 31)
ENCODER_TAILS = (0, 1, 31)  # total characters of the blob modulo 32: no ragged word, one real character in it, one filler in it
ENCODER_SHIFTS = (0, 1, 15, 16)  # bytes between a 32-byte boundary and the blob: the 32-byte loads (0, 16) and the byte path (1, 15)
_ENCODER = {}


def encoder_case(k, tail):
    """256 reads left + byte + right, flanks of k + 3 characters in random case with U for T.  Genome 0 holds every k-mer of left + X + right
    for the four X, genome 1 + x the k windows over the X of code x: a byte that counts as X gives {0, 1 + x} with every window counted for
    genome 0; any other byte leaves genome 0 exactly m - k windows.  In front stands one read (cut from left + A + right, repeated) whose
    length brings the blob's total to `tail` modulo 32."""
    if (k, tail) in _ENCODER:
        return _ENCODER[(k, tail)]
    rng = np.random.default_rng(900 + k)
    left, right = rand_text(k + 3, rng), rand_text(k + 3, rng)
    p, L = k + 3, 2 * k + 7
    m = L - k + 1
    st = Stored(k)
    for x, X in enumerate("ACGT"):
        s = left + X + right
        st.add(s, [0], canonical=False)
        for i in range(p - k + 1, p + 1):
            st.add_kmer(s[i:i + k], [1 + x])
    reads = [mixed(left, rng) + bytes([b]) + mixed(right, rng) for b in range(256)]
    front = ((left + "A" + right) * 2)[:(tail - 256 * L) % 32].encode()
    case = Case(st, [front] + reads, [1e-9, (m - k - 0.5) / m, (m - k + 0.5) / m, 1.0], canonicals=(False,))
    case.m, case.flank = m, p
    _ENCODER[(k, tail)] = case
    return case


@pytest.mark.parametrize("k", ENCODER_KS)
def test_encoder_case_pins_every_byte(k, oracle_mod):
    for tail in ENCODER_TAILS:
        case = encoder_case(k, tail)
        m, st = case.m, case.stored
        assert sum(len(r) for r in case.reads) % 32 == tail and len(case.reads) == 257
        assert len(st.sets) == (m - k) + 4 * k  # the windows beside the byte once, those over it once per X: no k-mer twice
        lo, below, above, one = case.thresholds[False]
        assert [math.ceil(m * t) for t in (lo, below, above, one)] == [1, m - k, m - k + 1, m]
        t_lo, t_below, t_above, t_one = (case.truth(t, False)[1:] for t in (lo, below, above, one))
        code = dict(zip(VALID, [0, 1, 2, 3, 3] * 2))
        for b in range(256):
            if b in code:
                assert t_lo[b] == [0, 1 + code[b]] and t_one[b] == [0] and 0 in t_above[b]
            else:  # exactly the k windows over the byte are gone
                assert t_lo[b] == [0] and t_below[b] == [0] and t_above[b] == [] and t_one[b] == []
        # every valid byte and some other byte stands at every one of the 32 places of a code word
        at = np.cumsum([len(r) for r in case.reads])[:-1] + case.flank
        assert len({int(a) % 32 for a in at}) == 32
        flanks = b"".join(r[:case.flank] + r[case.flank + 1:] for r in case.reads[1:])
        assert set(flanks) == set(VALID)
    if k % 9 == 0:  # (the oracle, like the reference, takes k = 9 j only; bytes 1 .. 127: it reads a C string)
        assert oracle_agrees(oracle_mod, encoder_case(k, 1)) > 400


# ---- 2. a bad character at every offset of the 32-character "bad" words -------------------------------------------------------------------
BADCHAR_KS = (9, 27, 32, 33, 63, 64, 99, 126)
BADCHAR_OFFSETS = (0, 1, 31)  # first character of every read, modulo 32, within the blob
BADCHAR_EXTRA = 70  # a read has k + 70 characters: 71 windows
_BADCHAR = {}


def badchar_positions(k):
    last = k + BADCHAR_EXTRA - 1
    return sorted({0, 1, 30, 31, 32, 33, 63, 64, 65, last - 1, last})


def badchar_case(k):
    """One stored sequence of k + 70 characters (canonical k-mers, genome 0).  Reads: the sequence, the sequence with an N at p for every p of
    badchar_positions, its first k characters alone and with an N first / last -- each at the offsets 0, 1 and 31 (mod 32) of the blob, reached
    by a read of 1 .. 32 N in front; an N read ends the blob.  So every read has an N right before its first and right behind its last
    character.  The windows over p are stored with every nucleotide at p: a window that wrongly lives is counted whatever the N decodes to."""
    if k in _BADCHAR:
        return _BADCHAR[k]
    rng = np.random.default_rng(1700 + k)
    Lr = k + BADCHAR_EXTRA
    m = Lr - k + 1
    base = rand_text(Lr, rng)
    st = Stored(k)
    st.add(base, [0])
    ps = badchar_positions(k)
    for p in ps:
        for X in "ACGT":
            v = base[:p] + X + base[p + 1:]
            for i in range(max(0, p - k + 1), min(p, Lr - k) + 1):
                st.add_kmer(canon(v[i:i + k]), [0])
    bodies = [(base, None)] + [(base[:p] + "N" + base[p + 1:], p) for p in ps]
    bodies += [(base[:k], None), ("N" + base[1:k], 0), (base[:k - 1] + "N", k - 1)]
    reads, meta, at = [], [], 0  # meta: None for a padding read, else (N position or None, read length)
    for o in BADCHAR_OFFSETS:
        for body, p in bodies:
            pad = (o - at - 1) % 32 + 1
            reads.append(b"N" * pad)
            meta.append(None)
            at += pad
            assert at % 32 == o
            reads.append(body.encode())
            meta.append((p, len(body), o))
            at += len(body)
    reads.append(b"N" * 3)
    meta.append(None)
    case = Case(st, reads, [1.0])
    thr = {1.0, 1.0 / m}
    for canonical in (False, True):
        for (mm, cnt), info in zip(case.counts(canonical), meta):
            if info is not None and mm == m and cnt.get(0, 0) > 0:
                c = cnt[0]
                thr |= {t for t in ((c - 0.5) / m, (c + 0.5) / m) if t <= 1.0}
    case.thresholds = {c: sorted(thr) for c in (False, True)}
    case.meta, case.m = meta, m
    _BADCHAR[k] = case
    return case


@pytest.mark.parametrize("k", BADCHAR_KS)
def test_badchar_case_kills_exactly_the_windows_over_the_character(k, oracle_mod):
    case = badchar_case(k)
    m = case.m
    starts = np.concatenate([[0], np.cumsum([len(r) for r in case.reads])])
    seen = set()
    for i, info in enumerate(case.meta):
        mm, cnt = case.counts(True)[i]
        if info is None:
            assert set(case.reads[i]) == {ord("N")} and not cnt
            continue
        p, ln, o = info
        assert starts[i] % 32 == o and case.reads[i - 1][-1:] == b"N" and case.reads[i + 1][:1] == b"N"
        dead = 0 if p is None else sum(1 for w in range(mm) if w <= p < w + k)  # window w is dead iff w <= p < w + k
        assert cnt.get(0, 0) == mm - dead, (i, p)
        if ln > k:
            assert mm == m and (p is None or 1 <= dead <= k)
            seen.add((p, o))
        else:
            assert mm == 1 and dead == (0 if p is None else 1)
    assert seen == {(p, o) for p in [None] + badchar_positions(k) for o in BADCHAR_OFFSETS}
    # one wrongly dead or wrongly live window flips a bit: thresholds right below and right above every true count
    mins = {math.ceil(m * t) for t in case.thresholds[True]}
    for i, info in enumerate(case.meta):
        c = case.counts(True)[i][1].get(0, 0)
        if info is not None and info[1] > k and c:
            assert c in mins and (c + 1 in mins or c == m)
    if k in (9, 63, 126):  # (the oracle, like the reference, takes k = 9 j only)
        assert oracle_agrees(oracle_mod, case, max_reads=60) > 100


# ---- 3. plan and tiles: where reads start, reads without a position, long reads, many reads --------------------------------------------------
PLAN_KS = (27, 63)
PLAN_SHORT_RUN = 300
_PLAN = {}


def plan_lengths(k, big=6000):
    """Read lengths of the `edges` batch.  Positions (k-mers) per read in brackets: 300 reads without one | [64] -> a read starts at 64 | [1]
    -> 65 | [62] -> 127 | [1] -> 128 | [128] -> 256 | [700] [68] -> 1024 | 300 without one, in front of tile 16 and of the fifth 256-block
    | [1] at 1024 | the long read | reads of exactly k and a few others | 300 without one."""
    short = [k - 1, 0, 1]
    run = [short[i % 3] for i in range(PLAN_SHORT_RUN)]
    npos = [64, 1, 62, 1, 128, 700, 68]
    lens = run + [n + k - 1 for n in npos] + run + [k, big, k, k, k + 1, k + 62, k, 150, 400, k + 63] + run
    return lens


def _draw(src, ln, rng):
    a = int(rng.integers(0, len(src) - ln + 1))
    return src[a:a + ln]


def plan_reads(k, lens, srcs, rng, genome_of=lambda i: i & 1, snp=True):
    """reads of the given lengths cut from srcs[genome_of(i)]; every third one reverse-complemented, every seventh and every long one
    with one substitution"""
    reads = []
    for i, ln in enumerate(lens):
        r = _draw(srcs[genome_of(i)], ln, rng)
        if i % 3 == 2:
            r = revcomp(r)
        if snp and ln >= k and (i % 7 == 3 or ln > 8 * k):
            q = ln // 2
            r = r[:q] + "ACGT"[("ACGT".index(r[q]) + 1) % 4] + r[q + 1:]
        reads.append(r.encode())
    return reads


def stride_genome(i):
    """alternates from read to read, and differs between the reads i and i + 16384 that one wavefront of k_seq_tally handles in turn"""
    return ((i >> 14) ^ i) & 1


def plan_case(k, src_len=6100, big=6000, stride_reads=20000):
    """{batch name: Case} over one index: genome 0 holds the canonical k-mers of one random sequence, genome 1 those of another."""
    key = (k, src_len, big, stride_reads)
    if key in _PLAN:
        return _PLAN[key]
    rng = np.random.default_rng(2300 + k)
    srcs = [rand_text(src_len, rng), rand_text(src_len, rng)]
    st = Stored(k)
    st.add(srcs[0], [0])
    st.add(srcs[1], [1])
    thr = [1e-9, 0.8, 1.0]
    short = [k - 1, 0, 1]
    out = {
        "edges": Case(st, plan_reads(k, plan_lengths(k, big), srcs, rng), thr),
        "none": Case(st, plan_reads(k, [short[i % 3] for i in range(500)], srcs, rng), thr),
        "empty": Case(st, [b""] * 40, thr),
        "one_long": Case(st, plan_reads(k, [min(200, src_len)], srcs, rng), thr),
        "one_k": Case(st, plan_reads(k, [k], srcs, rng), thr),
        "one_short": Case(st, plan_reads(k, [k - 1], srcs, rng), thr),
    }
    if stride_reads:
        out["stride"] = Case(st, plan_reads(k, [k + int(x) for x in rng.integers(0, 6, stride_reads)], srcs, rng, stride_genome, snp=False), [1e-9, 1.0])
    _PLAN[key] = out
    return out


def positions_of(case, k):
    """(npos per read, pos_off): what k_seq_plan and the scan compute"""
    npos = np.array([max(len(r) - k + 1, 0) for r in case.reads], dtype=np.int64)
    return npos, np.concatenate([[0], np.cumsum(npos)])


def _zero_runs(npos):
    """[(first read, reads)] of the maximal runs of reads without a position"""
    runs, i = [], 0
    while i < len(npos):
        if npos[i] == 0:
            j = i
            while j < len(npos) and npos[j] == 0:
                j += 1
            runs.append((i, j - i))
            i = j
        else:
            i += 1
    return runs


@pytest.mark.parametrize("k", PLAN_KS)
def test_plan_case_reaches_every_start_and_run(k, oracle_mod):
    cases = plan_case(k)
    edges = cases["edges"]
    npos, off = positions_of(edges, k)
    starts = {int(off[i]) for i in range(len(npos)) if npos[i] > 0}  # first position of the reads that own one
    assert {64, 256, 1024} <= starts and {65, 127} <= starts  # 64 t, 256 t, 1024 t, 64 t + 1, 64 t - 1
    runs = _zero_runs(npos)
    assert [n for _, n in runs] == [PLAN_SHORT_RUN] * 3 and runs[0][0] == 0 and runs[2][0] + runs[2][1] == len(npos)
    assert off[runs[1][0]] == 1024 and npos[runs[1][0] + PLAN_SHORT_RUN] == 1  # 300 reads share the offset 1024 with the read of k characters behind them
    assert {len(edges.reads[i]) for i in range(*[runs[1][0], runs[1][0] + 3])} == {k - 1, 0, 1}
    assert (npos == 1).sum() >= 5 and max(len(r) for r in edges.reads) == 6000
    big = int(np.argmax(npos))
    assert off[big + 1] // 64 - off[big] // 64 > 90 and off[big + 1] // 256 - off[big] // 256 > 20  # many tiles, many 256-blocks, several 1024-blocks
    assert off[-1] > 7 * 1024
    for name in ("none", "empty"):
        assert positions_of(cases[name], k)[1][-1] == 0 and all(x == [] for x in cases[name].truth(1e-9, True))
    assert sum(len(r) for r in cases["none"].reads) > 0 and sum(len(r) for r in cases["empty"].reads) == 0
    assert [len(cases[n].reads) for n in ("one_long", "one_k", "one_short")] == [1, 1, 1]
    assert cases["one_k"].truth(1.0, True) in ([[0]], [[1]]) and cases["one_short"].truth(1e-9, True) == [[]]
    stride = cases["stride"]
    assert len(stride.reads) == 20000 > TALLY_STRIDE and {len(r) for r in stride.reads} == set(range(k, k + 6))
    t = stride.truth(1e-9, True)
    for i in range(len(t)):
        assert t[i] == [stride_genome(i)]  # one genome per read ...
        if i + TALLY_STRIDE < len(t):
            assert t[i] != t[i + TALLY_STRIDE] and t[i] != t[i + 1]  # ... the other one in the same wavefront's next read
    # reads of both strands, reads with a substitution that miss the threshold 1.0 and pass 0.8 or not
    assert any(a and not b for a, b in zip(edges.truth(1e-9, True), edges.truth(1e-9, False)))
    assert any(a and not b for a, b in zip(edges.truth(0.8, True), edges.truth(1.0, True)))
    sub = Case(edges.stored, edges.reads[280:330] + edges.reads[600:640], edges.thresholds[True])
    assert oracle_agrees(oracle_mod, sub) > 100


# ---- 4. the tally: runs of one colour set, set sizes, thresholds ----------------------------------------------------------------------------
TALLY_K = 27
TALLY_GENOMES = 150
# (k-mer positions, genomes of their colour set), in the order of the stored sequence: a run over 60..70 (lane 63 | 64), one over 120..135
# (the turn's end 127 | 128), runs of 1, 2, 64, 65, 129 and 300 positions; sets of 1, 7, 8, 9, 16, 17, 64 and 65 genomes
TALLY_SEGMENTS = ((60, 1), (11, 7), (49, 8), (16, 9), (1, 16), (2, 17), (64, 64), (65, 65), (129, 2), (300, 3), (40, 1))
# 0.1 at m = 30 and m = 10: both products are exact in double (30 * 0.1 == 3.0, ceil 3).  0.28 at m = 25 and m = 50 is where the double product
# lies above the rational one: 25 * 0.28 == 7.000000000000001, so 8 k-mers are asked for where 7 / 25 is exactly 28 %
TALLY_FIXED = (1.0, 0.1, 1e-9, 0.28)
_TALLY = {}


def tally_case():
    if "c" in _TALLY:
        return _TALLY["c"]
    k = TALLY_K
    rng = np.random.default_rng(4100)
    npos = sum(n for n, _ in TALLY_SEGMENTS)
    T = rand_text(npos + k - 1, rng)
    st = Stored(k)
    seg_sets, j = [], 0
    for n, size in TALLY_SEGMENTS:
        ids = sorted(int(g) for g in rng.choice(TALLY_GENOMES, size, replace=False))
        seg_sets.append(ids)
        for p in range(j, j + n):
            st.add_kmer(canon(T[p:p + k]), ids)
        j += n
    cut = lambda a, m: T[a:a + m + k - 1]
    spans = [(0, npos), (0, 64), (0, 65), (0, 128), (0, 129), (0, 136), (0, 200), (1, 200), (7, 130), (57, 30), (60, 10), (60, 30), (66, 10), (3, 10),
             (115, 30), (120, 16), (136, 1), (137, 2), (139, 64), (139, 65), (203, 65), (268, 129), (268, 130), (397, 300), (390, 310), (397, 128),
             (690, 47), (100, 500), (8, 150), (53, 25), (46, 50)]
    reads = [cut(a, m) for a, m in spans]
    whole = cut(0, npos)
    reads += [revcomp(whole), whole[:450] + "N" + whole[451:], whole[:130] + "n" + whole[131:600]]
    case = Case(st, [r.encode() for r in reads], TALLY_FIXED)
    extra = set()
    for m, cnt in case.counts(True):  # per read: c / m of one genome's true count, and the doubles next to it
        if cnt:
            c = sorted(cnt.values())[len(cnt) // 2]
            extra |= {t for t in (np.nextafter(c / m, 0.0), c / m, np.nextafter(c / m, 2.0)) if 0 < t <= 1.0}
    case.thresholds[True] = list(TALLY_FIXED) + sorted(float(t) for t in extra - set(TALLY_FIXED))
    case.seg_sets, case.spans, case.T = seg_sets, spans, T
    _TALLY["c"] = case
    return case


def colour_runs(st, read, canonical=True):
    """[(first position, positions, colour set or None)]: the maximal runs of equal colour sets along the read"""
    r, k = normalise(read), st.k
    per = []
    for i in range(max(len(r) - k + 1, 0)):
        x = r[i:i + k]
        ids = None if "N" in x else st.sets.get(canon(x) if canonical else x)
        per.append(None if ids is None else tuple(sorted(ids)))
    runs, i = [], 0
    while i < len(per):
        j = i
        while j < len(per) and per[j] == per[i]:
            j += 1
        runs.append((i, j - i, per[i]))
        i = j
    return runs


def test_tally_case_runs_sizes_and_thresholds(oracle_mod):
    case = tally_case()
    st = case.stored
    assert len({tuple(s) for s in case.seg_sets}) == len(TALLY_SEGMENTS) and len(st.sets) == sum(n for n, _ in TALLY_SEGMENTS)
    runs = colour_runs(st, case.reads[0])
    assert [(n, len(s)) for _, n, s in runs] == list(TALLY_SEGMENTS)
    spans = {(a, a + n - 1) for a, n, _ in runs}
    assert (60, 70) in spans and (120, 135) in spans and any(n >= 130 for _, n, _ in runs)  # lane 63 | 64, turn 127 | 128, longer than a turn
    assert {1, 2, 64, 65, 129, 300} <= {n for _, n, _ in runs}
    assert {1, 7, 8, 9, 16, 17, 64, 65} <= {len(s) for _, _, s in runs}
    # the other reads move the runs against the lanes: a run that ends at lane 63, starts at lane 0 of the second half, is cut by the read's end
    ends = set()
    for r in case.reads:
        for a, n, s in colour_runs(st, r):
            if s is not None:
                ends |= {("first", a % 64), ("last", (a + n - 1) % 64)}
    assert {("last", 63), ("first", 0), ("first", 63), ("last", 0)} <= ends
    assert any(s is None for r in case.reads[-2:] for _, _, s in colour_runs(st, r))  # no k-mer over the N: a gap between two runs of one set
    ms = {m for m, _ in case.counts(True)}
    assert {10, 30, 25, 50} <= ms and math.ceil(30 * 0.1) == 3 and math.ceil(10 * 0.1) == 1
    # ceil(m thr) in double differs from the exact ceiling of m times the decimal threshold, and a genome holds exactly the exact ceiling:
    # it is left out (as by the reference, which multiplies in double too)
    for m, c in ((25, 7), (50, 14)):
        assert math.ceil(m * 0.28) == c + 1 and math.ceil(m * Fraction(28, 100)) == c
        hit = [(mm, cnt) for mm, cnt in case.counts(True) if mm == m and c in cnt.values()]
        assert hit and all(g not in answer(mm, cnt, 0.28) for mm, cnt in hit for g, x in cnt.items() if x == c)
    at, below = 0, 0
    for thr in case.thresholds[True]:
        for m, cnt in case.counts(True):
            minv = math.ceil(m * thr)
            at += sum(1 for c in cnt.values() if c == minv)
            below += sum(1 for c in cnt.values() if c == minv - 1)
    assert at > 20 and below > 20  # counts of exactly minv and of minv - 1
    assert 40 < len(case.thresholds[True]) < 120
    assert oracle_agrees(oracle_mod, case, max_reads=8) > 100


# ---- 5. the tally's genome windows and the width of the resident ids ---------------------------------------------------------------------------
WINDOW_GS = (2047, 2048, 2049, 4096, 4097)
WIDE_IDS = (0, 1, 255, 256, 65535, 65536, 70001)
SETS_SEG = 40  # k-mer positions per colour set along the stored sequence
_SETS = {}


def window_sets(G):
    """The colour sets of the G-genome case: the genomes next to every 2048-genome window's edge and the last one; genome j of one window
    without genome j of the next (5 / 2053, 2048 / 4096) and the reverse; one set across an edge."""
    cand = [[0], [5], [7, 8], [2039, 2040], [2046], [2047], [2048], [2053], [2047, 2048], [2049], [4087, 4088], [4095], [4096], [4095, 4096],
            list(range(2040, 2060)), [G - 1], [0, G - 1], [G - 2]]
    out = []
    for s in cand:
        s = sorted({g for g in s if 0 <= g < G})
        if s and s not in out:
            out.append(s)
    return out


def sets_case(name, k, id_sets, seed):
    """One stored sequence, SETS_SEG positions per colour set.  Reads: one inside every set's stretch, one across every boundary (half the
    positions each: a count of exactly ceil(m / 2)), the whole sequence, its reverse complement, the whole with an N, ten positions inside
    every stretch, and 10 + 30 positions across every boundary."""
    if name in _SETS:
        return _SETS[name]
    rng = np.random.default_rng(seed)
    n = SETS_SEG * len(id_sets)
    T = rand_text(n + k - 1, rng)
    st = Stored(k)
    for p in range(n):
        st.add_kmer(canon(T[p:p + k]), id_sets[p // SETS_SEG])
    cut = lambda a, m: T[a:a + m + k - 1]
    reads = [cut(SETS_SEG * s, SETS_SEG) for s in range(len(id_sets))]
    reads += [cut(SETS_SEG * s + SETS_SEG // 2, SETS_SEG) for s in range(len(id_sets) - 1)]
    reads += [T, revcomp(T), T[:n // 2] + "N" + T[n // 2 + 1:]]
    reads += [cut(SETS_SEG * s + 7, 10) for s in range(len(id_sets))]
    reads += [cut(SETS_SEG * s + 30, SETS_SEG) for s in range(len(id_sets) - 1)]
    case = Case(st, [r.encode() for r in reads], [1e-9, 0.5, 1.0])
    case.id_sets = id_sets
    _SETS[name] = case
    return case


def window_case(G):
    return sets_case(("G", G), 27, window_sets(G), 5000 + G)


def wide_case():
    w = WIDE_IDS
    return sets_case("wide", 27, [[w[0]], [w[1], w[2]], [w[3], w[4]], [w[5]], [w[6]], [w[0], w[5], w[6]], sorted(w), [w[4], w[5]]], 6000)


def expected_rows(lists, G):
    """the rows of the device call: bit g % 8 of byte g // 8; the padding bits of the last byte stay 0"""
    rows = np.zeros((len(lists), (G + 7) // 8), dtype=np.uint8)
    for i, ids in enumerate(lists):
        for g in ids:
            rows[i, g >> 3] |= 1 << (g & 7)
    return rows


@pytest.mark.parametrize("G", WINDOW_GS)
def test_window_case_has_the_genomes_at_every_edge(G, oracle_mod):
    case = window_case(G)
    st = case.stored
    assert st.n_genomes() == G and 30 <= len(case.reads) <= 75
    used = {g for s in case.id_sets for g in s}
    edges = [g for w in range(TALLY_G, G + 1, TALLY_G) for g in (w - 1, w)] + [0, G - 1]
    assert {g for g in edges if g < G} <= used
    t = case.truth(1e-9, True)
    hit = {tuple(x) for x in t}
    assert (5,) in hit and ((2053,) in hit) == (G > 2053)  # counter 5 of window 0 without counter 5 of window 1, and the reverse
    if G > 4096:
        assert (2048,) in hit and (4096,) in hit
    half = case.truth(0.5, True)
    n = len(case.id_sets)
    for s in range(n - 1):  # across a boundary: both sets at exactly ceil(40 * 0.5)
        assert half[n + s] == sorted(set(case.id_sets[s]) | set(case.id_sets[s + 1]))
    assert (expected_rows(t, G)[:, -1] >> ((G - 1) % 8 + 1)).max() == 0 and expected_rows(t, G)[:, -1].max() > 0
    if G in (2049, 4097):
        assert oracle_agrees(oracle_mod, case) > 50


def test_wide_case_needs_four_byte_ids(oracle_mod):
    case = wide_case()
    assert case.stored.n_genomes() == 70002 and {g for s in case.id_sets for g in s} == set(WIDE_IDS)
    t = case.truth(1e-9, True)
    assert [65536] in t and [70001] in t and sorted(WIDE_IDS) in t
    assert oracle_agrees(oracle_mod, case) > 50


# ---- 6. the container walk's sequence kernels at one and two key words ---------------------------------------------------------------------------
WALK_KS = (18, 27, 31, 36, 63)
WALK_SHAPES = ("tiny", "normal", "deep")
ROOT_MAX_CC = 64  # BFT_LDS_ROOT_MAX_CC: a root with more CCs would not be staged -- no index has one: the 4^9 prefixes of the root fill 22 CCs
ROOT_CCS_FULL = 22
WALK_DEEP_KMERS = 6000
_WALK = {}


def walk_case(k, shape):
    """The Case of a shape.  tiny: two sequences of 90 positions, fewer than 255 k-mers -- the root has no CC.  normal: the index and the
    `edges` reads of plan_case.  deep: the same, and as genome 2 the k-mers of S.low_entropy_kmers under six 9-mer prefixes (child nodes),
    300 of which are asked for as reads of exactly k characters, each also with one substitution."""
    if (k, shape) in _WALK:
        return _WALK[(k, shape)]
    rng = np.random.default_rng(7000 + k)
    if shape == "tiny":
        srcs = [rand_text(90 + k - 1, rng), rand_text(90 + k - 1, rng)]
        st = Stored(k)
        st.add(srcs[0], [0])
        st.add(srcs[1], [1])
        lens = ([k - 1, 0, 1] * 3 + [k + 63, k, k + 61, k, k + 80, k + 40, k - 1, k + 89, k + 89, k + 10, 0, k]) * 2
        case = Case(st, plan_reads(k, lens, srcs, rng), [1e-9, 0.8, 1.0])
    else:
        edges = plan_case(k)["edges"]
        st = Stored(k)
        st.sets = {x: set(v) for x, v in edges.stored.sets.items()}
        reads = list(edges.reads)
        if shape == "deep":
            below = S.packed_to_ascii(S.low_entropy_kmers(WALK_DEEP_KMERS, k, 6, seed=k, levels=1), k)
            for x in below:
                st.add_kmer(x, [2])
            for i, x in enumerate(below[:: max(1, len(below) // 300)]):
                q = (7 * i) % k
                reads += [x.encode(), (x[:q] + "ACGT"[("ACGT".index(x[q]) + 1) % 4] + x[q + 1:]).encode()]
        case = Case(st, reads, [1e-9, 0.8, 1.0])
    _WALK[(k, shape)] = case
    return case


@pytest.mark.parametrize("k", WALK_KS)
def test_walk_cases_have_their_shapes(k, oracle_mod):
    G = 3
    for shape in WALK_SHAPES:
        case = walk_case(k, shape)
        st = case.stored
        assert positions_of(case, k)[1][-1] > 512
        if shape == "tiny":
            assert len(st.sets) < 255 and sum(1 for x in case.truth(1.0, True) if x) >= 8
        o = None
        if k % 9 == 0:  # (the oracle, like the reference, takes k = 9 j only: at the other k the GPU test asserts the shape on the built index)
            o = oracle_mod.OracleBFT(k)
            for g, packed in st.phases():
                o.insert_kmers(packed, g)
            stats = o.stats()
            assert stats["kmers"] == len(st.sets)
            if shape == "tiny":
                assert stats["root_ccs"] == 0
            else:
                assert 1 <= stats["root_ccs"] <= ROOT_MAX_CC
            if shape == "deep":
                assert stats["child_nodes"] > 0
        if shape == "deep":
            t = case.truth(1e-9, False)
            assert sum(1 for x in t if x == [2]) >= 250  # the k-mers below the root are asked for, and their neighbours are absent
        # both strands are asked: reads that only the canonical search answers
        assert any(a and not b for a, b in zip(case.truth(1e-9, True), case.truth(1e-9, False)))
        if o is not None:
            sub = Case(st, case.reads[-40:] + case.reads[300:320], case.thresholds[True])
            for c, thr in sub.runs():
                for r, x in zip(sub.reads, sub.truth(thr, c)):
                    if r:
                        assert o.query_sequence(r.decode(), thr, c, G) == x
            o.close()
