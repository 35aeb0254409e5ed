"""The cases of the prefix-matching edge tests (tests/test_gpu_prefix_edges.py runs them on the GPU), their ground truth, and -- here, without
a GPU -- the proof that each case reaches the regime it is named after.

Truth, in numpy and Python integers only (nothing of the library's): the T-form key of a k-mer with codes c[0..k), L = k // 9, is, most
significant first, for each block j < L the 18 bits c[9j+1] .. c[9j+8], c[9j], then c[9L..k) -- pinned against bft_hosttest_roundtrip for every
k used.  The stored k-mers sorted by that key are "the table", a k-mer's row is its rank, the matches of (prefix, len) are the rows whose first
len codes are the prefix's, in rank order, and a row's colour set is the set of genomes that inserted it.  The *candidates* of a prefix -- what
k_pm_bounds hands k_pm_count / k_pm_emit -- are the rows that agree with it on the T-form digits in front of the one the filter reads; they are
computed here from the digit order alone, and `Truth.brute` (the definition, row by row) checks the matches drawn from them.

How the kernels cut the candidates into chunks is read from the library (bft_gpu_debug_prefix_plan: csrc/bft_prefix.h, no device needed) and
pinned to the rule as DESIGN section 9 states it.

Sizes: the family index of a k has 4 base k-mers, their 3 k substitutions twice (tail kept / tail random), 4100 k-mers under one 9-mer head
(k >= 18), all-A, all-T and 3000 random k-mers: 3.2e3 rows at k = 9 and 13, 7.5e3 (k = 18) to 1.01e4 (k = 126), in 3 genomes; the two G indexes 10236 / 10240 rows."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from bloomfiltertrie_amd import _lib, synth as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS_EDGE = (9, 13, 18, 22, 27, 31, 36, 63, 64, 72, 80, 90, 99, 126)  # (22: six bytes, the one B mod 4 == 2 that a one-word key has)
CHUNKS, TILE = 2048, 256  # BFT_PM_CHUNKS, PM_THREADS: test_plan_is_the_stated_rule pins them to the library
N_GENOMES = 3
N_BASES, HEAD_FAMILY, N_RANDOM = 4, 4100, 3000
A, CC, G, T = 0, 1, 2, 3
TAG_BASE, TAG_SNP, TAG_TAIL, TAG_HEAD, TAG_END, TAG_RANDOM, TAG_G = range(7)


_LIB = []


# ---- the chunk rule, from the library ------------------------------------------------------------------------------------------------------------
def plan(Ccand, chunk):
    """(chunk size, begin, end) of chunk `chunk` of Ccand candidates"""
    out = (C.c_uint64 * 3)()
    if not _LIB:
        _LIB.append(_lib.load())
    _lib.check(_LIB[0].bft_gpu_debug_prefix_plan(Ccand, chunk, out))
    return int(out[0]), int(out[1]), int(out[2])


def chunks(Ccand):
    """(chunk size, begins [CHUNKS], ends [CHUNKS]) of Ccand candidates, every chunk asked of the library"""
    p = [plan(Ccand, g) for g in range(CHUNKS)]
    assert len({x[0] for x in p}) == 1
    return p[0][0], np.array([x[1] for x in p], dtype=np.int64), np.array([x[2] for x in p], dtype=np.int64)


# ---- truth ---------------------------------------------------------------------------------------------------------------------------------------
def t_order(k):
    """source position of each T-form digit, most significant first"""
    L = k // 9
    cols = []
    for j in range(L):
        cols += list(range(9 * j + 1, 9 * j + 9)) + [9 * j]
    return np.array(cols + list(range(9 * L, k)), dtype=np.int64)


def t_key_ints(codes, k):
    """the T-form keys as Python integers"""
    out = []
    for row in np.asarray(codes)[:, t_order(k)].tolist():
        v = 0
        for c in row:
            v = (v << 2) | c
        out.append(v)
    return out


def _void(a):
    a = np.ascontiguousarray(a, dtype=np.uint8)
    return a.view(np.dtype((np.void, a.shape[1]))).ravel()


def rule(k, ln):
    """(d, fpos): a prefix of ln nucleotides fixes the first d T-form digits of its candidates; fpos = the source position of the digit the
    filter then reads (the first nucleotide of the block the prefix ends in), or -1 when the candidates are the matches"""
    L = k // 9
    f, m = divmod(int(ln), 9)
    if m and f < L:
        return 9 * f + m - 1, 9 * f
    return int(ln), -1


class Answer:
    """the truth of one batch: per prefix a (first candidate row), cand, filt, kept; coff / offsets (exclusive sums); per candidate of the
    stream owner, row, keep; per match rows"""


class Truth:
    def __init__(self, k, codes, member, tags):
        codes = np.asarray(codes, dtype=np.uint8)
        _, first = np.unique(_void(codes), return_index=True)  # distinct k-mers: the first occurrence decides tag and genomes
        first.sort()
        codes, member, tags = codes[first], np.asarray(member, dtype=bool)[first], np.asarray(tags)[first]
        tc = codes[:, t_order(k)]
        order = np.lexsort(tc.T[::-1])
        self.k, self.nb, self.W, self.N = k, S.kmer_bytes(k), (2 * k + 63) // 64, len(codes)
        self.codes, self.tc, self.member, self.tags = codes[order], np.ascontiguousarray(tc[order]), member[order], tags[order]
        self.packed = S.pack_codes(self.codes)
        v = _void(self.tc)
        assert (v[1:] != v[:-1]).all() and (np.sort(v) == v).all()  # (the byte order of numpy's void is the digit order)
        assert self.member.any(axis=1).all()
        self.setmask = (self.member * (1 << np.arange(member.shape[1]))).sum(axis=1)

    def insert_into(self, t):
        for g in range(self.member.shape[1]):
            t.insert_kmers(np.ascontiguousarray(self.packed[self.member[:, g]]), g)

    def brute(self, pcodes, ln):
        """the definition: rows whose first ln codes are the prefix's"""
        return np.flatnonzero((self.codes[:, :ln] == np.asarray(pcodes)[:ln]).all(axis=1))

    def answer(self, pref, lens):
        k, n = self.k, len(pref)
        pc = S.unpack_codes(pref, k) if n else np.zeros((0, k), np.uint8)
        ptc = pc[:, t_order(k)]
        r = Answer()
        r.a, b = np.zeros(n, np.int64), np.zeros(n, np.int64)
        fpos = np.full(n, -1, np.int64)
        for ln in np.unique(lens):
            if not 1 <= ln <= k:
                continue
            sel = np.flatnonzero(lens == ln)
            d, fp = rule(k, ln)
            fpos[sel] = fp
            if d == 0:
                r.a[sel], b[sel] = 0, self.N
            else:
                tv, qv = _void(self.tc[:, :d]), _void(ptc[sel, :d])
                r.a[sel], b[sel] = np.searchsorted(tv, qv, side="left"), np.searchsorted(tv, qv, side="right")
        r.cand = b - r.a
        r.filt = fpos >= 0
        r.coff = np.concatenate([[0], np.cumsum(r.cand)])
        r.C = int(r.coff[-1])
        r.owner = np.repeat(np.arange(n), r.cand)
        r.row = r.a[r.owner] + (np.arange(r.C) - r.coff[r.owner])
        fcol = np.maximum(fpos, 0)
        r.keep = ~r.filt[r.owner] | (self.codes[r.row, fcol[r.owner]] == pc[r.owner, fcol[r.owner]])
        r.kept = np.bincount(r.owner[r.keep], minlength=n).astype(np.int64)
        r.offsets = np.concatenate([[0], np.cumsum(r.kept)]).astype(np.uint64)
        r.rows = r.row[r.keep].astype(np.uint32)
        r.total = len(r.rows)
        return r


# ---- the indexes ---------------------------------------------------------------------------------------------------------------------------------
def _members(n, rng):
    m = rng.integers(1, 1 << N_GENOMES, n)
    return ((m[:, None] >> np.arange(N_GENOMES)) & 1).astype(bool)


@functools.lru_cache(maxsize=None)
def family(k):
    """the family index of k: every prefix of a base k-mer has candidates that only the filter tells apart (the substitutions at the first
    nucleotide of the block it ends in)"""
    rng = np.random.default_rng(1000 + k)
    bases = rng.integers(0, 4, (N_BASES, k), dtype=np.uint8)
    rows, tags = [bases], [np.full(N_BASES, TAG_BASE)]
    for p in bases:
        for j in range(k):
            for s in (1, 2, 3):
                q = p.copy()
                q[j] = (p[j] + s) & 3
                r = q.copy()
                r[j + 1:] = rng.integers(0, 4, k - j - 1, dtype=np.uint8)
                rows += [q[None], r[None]]
                tags += [[TAG_SNP], [TAG_TAIL]]
    if k >= 18:
        h = rng.integers(0, 4, (HEAD_FAMILY, k), dtype=np.uint8)
        h[:, :9] = rng.integers(0, 4, 9, dtype=np.uint8)
        rows.append(h)
        tags.append(np.full(HEAD_FAMILY, TAG_HEAD))
    rows += [np.zeros((1, k), np.uint8), np.full((1, k), 3, np.uint8), rng.integers(0, 4, (N_RANDOM, k), dtype=np.uint8)]
    tags += [[TAG_END], [TAG_END], np.full(N_RANDOM, TAG_RANDOM)]
    codes = np.concatenate(rows)
    tr = Truth(k, codes, _members(len(codes), rng), np.concatenate([np.asarray(x).ravel() for x in tags]))
    tr.bases = bases
    return tr


G_K, G_BASE_ROWS, G_RANKS, G_REPEATS = 27, 10236, (767, 1087, 1536, 2112), 103


def _g_base(rng):
    """G_BASE_ROWS 27-mers that start with A or C, no two with the same nucleotides 1..8: a k-mer's G-initial twin is the row right behind it"""
    grp = rng.choice(4 ** 8, G_BASE_ROWS, replace=False)
    codes = rng.integers(0, 4, (G_BASE_ROWS, G_K), dtype=np.uint8)
    codes[:, 1:9] = (grp[:, None] >> (2 * np.arange(8))) & 3
    codes[:, 0] = rng.integers(0, 2, G_BASE_ROWS)
    return codes


@functools.lru_cache(maxsize=None)
def no_g():
    """no k-mer starts with G (or T): the prefix "G" has the whole table as candidates and keeps none"""
    rng = np.random.default_rng(77)
    codes = _g_base(rng)
    return Truth(G_K, codes, _members(len(codes), rng), np.full(len(codes), TAG_RANDOM))


@functools.lru_cache(maxsize=None)
def one_g():
    """the same rows plus four G-initial k-mers, each the twin of the row in front of the rank it is to take: ranks G_RANKS of 10240"""
    rng = np.random.default_rng(77)
    codes = _g_base(rng)
    base = Truth(G_K, codes, np.ones((len(codes), 1), bool), np.zeros(len(codes))).codes  # in table order
    twins = base[[r - i - 1 for i, r in enumerate(G_RANKS)]].copy()
    twins[:, 0] = G
    allc = np.concatenate([codes, twins])
    return Truth(G_K, allc, _members(len(allc), rng), np.concatenate([np.full(len(codes), TAG_RANDOM), np.full(len(twins), TAG_G)]))


@functools.lru_cache(maxsize=None)
def single():
    """an index of one k-mer"""
    rng = np.random.default_rng(5)
    return Truth(27, rng.integers(0, 4, (1, 27), dtype=np.uint8), np.array([[True, False, True]]), [TAG_RANDOM])


INDEXES = {"family": family, "no_g": lambda k: no_g(), "one_g": lambda k: one_g(), "single": lambda k: single()}


def index(name, k):
    tr = INDEXES[name](k)
    assert tr.k == k
    return tr


# ---- batches -------------------------------------------------------------------------------------------------------------------------------------
def pack(pcodes, lens, seed=0):
    """packed prefixes with garbage behind every length and in the padding bits of the last byte"""
    pcodes, lens = np.asarray(pcodes, dtype=np.uint8), np.asarray(lens, dtype=np.uint8)
    n, k = pcodes.shape
    rng = np.random.default_rng(seed)
    keep = np.arange(k)[None, :] < lens[:, None]
    pref = S.pack_codes(np.where(keep, pcodes, rng.integers(0, 4, (n, k), dtype=np.uint8)))
    if (2 * k) % 8 and n:
        pref[:, -1] |= rng.integers(0, 256, n).astype(np.uint8) & np.uint8((0xFF << ((2 * k) % 8)) & 0xFF)
    return pref, lens


def _stored(tr, n, seed, tag=TAG_RANDOM):
    """n distinct stored k-mers of the random class (tag None: of any), in random order"""
    pool = np.flatnonzero(tr.tags == tag) if tag is not None else np.arange(tr.N)
    return tr.codes[np.random.default_rng(seed).choice(pool, n, replace=False)]


def _absent(tr, codes, seed):
    """one nucleotide of each changed; the few that are stored are changed again"""
    rng = np.random.default_rng(seed)
    out = codes.copy()
    todo = np.arange(len(out))
    have = set(_void(tr.codes).tolist())
    while len(todo):
        pos = rng.integers(0, tr.k, len(todo))
        out[todo, pos] = (out[todo, pos] + rng.integers(1, 4, len(todo))) & 3
        todo = todo[[x in have for x in _void(out[todo]).tolist()]]
    return out


def _flen(k):
    """a length at which a random stored k-mer is its prefix's only candidate and the filter applies: two nucleotides into the last block"""
    return 9 * (k // 9 - 1) + 2


def geometry(tr, Ccand):
    """exactly Ccand candidates: length-1 prefixes (the whole table each) and full-length stored k-mers (one each), the long ones in the middle"""
    if Ccand == 0:
        return _absent(tr, _stored(tr, 1, 3), 4), np.array([tr.k])
    r, s = divmod(Ccand, tr.N)
    ones = _stored(tr, s, 6, None) if s else np.zeros((0, tr.k), np.uint8)
    longs = np.zeros((r, tr.k), np.uint8)
    longs[:, 0] = np.arange(r) & 3
    return np.concatenate([ones[:s // 2], longs, ones[s // 2:]]), np.array([tr.k] * (s // 2) + [1] * r + [tr.k] * (s - s // 2))


# expected (tiles per chunk, empty chunks, candidates of the last chunk that has any) per candidate count
GEOMETRY = {0: (0, 2048, 0), 1: (1, 2047, 1), 255: (1, 2047, 255), 256: (1, 2047, 256), 257: (1, 2046, 1),
            524287: (1, 0, 255), 524288: (1, 0, 256), 524289: (2, 1023, 1), 1048576: (2, 0, 512), 1048577: (3, 682, 257),
            1572865: (4, 511, 1)}


def repeated(tr, pcode_rows, lens, more_than):
    """the prefixes over and over, until the batch has more than `more_than` candidates"""
    pref, ln = pack(pcode_rows, lens)
    per = int(tr.answer(pref, ln).C)
    assert per > 0
    reps = more_than // per + 1
    return np.tile(np.asarray(pcode_rows), (reps, 1)), np.tile(np.asarray(lens), reps)


def _head(tr):
    return tr.codes[np.flatnonzero(tr.tags == TAG_HEAD)[0]]


def runs(tr, what):
    """the run shapes of pm_lane and of the per-prefix atomics"""
    k, fl = tr.k, _flen(tr.k)
    base = tr.bases[0]
    nine_f = 9 * (fl // 9)
    if what in ("ones256", "ones257"):  # one candidate each, every one a filtered prefix: a head at every lane
        n = int(what[4:])
        return _stored(tr, n, 11), np.full(n, fl)
    if what == "alternating":  # filtered / unfiltered, one candidate each
        x = _stored(tr, 300, 12)
        return x, np.where(np.arange(300) & 1, k, fl)
    if what == "duplicates":  # adjacent duplicates of one-candidate, many-candidate and empty prefixes
        x = np.concatenate([_stored(tr, 40, 13), np.tile(base, (40, 1)), _absent(tr, _stored(tr, 20, 14), 15)])
        ln = np.concatenate([np.full(40, fl), np.arange(1, 41) % k + 1, np.full(20, k)])
        rep = np.tile([2, 3, 1, 2], 25)
        return np.repeat(x, rep, axis=0), np.repeat(ln, rep)
    if what == "hit_miss":  # hit, no candidate, hit, a candidate the filter rejects
        x = _stored(tr, 400, 16)
        ln = np.full(400, fl)
        x[1::4] = _absent(tr, x[1::4], 17)
        ln[1::4] = k
        x[3::4, nine_f] = (x[3::4, nine_f] + 1) & 3
        return x, ln
    if what == "empty_runs":  # 300 prefixes without a candidate (more than a tile of prefixes) at the start, in the middle, at the end
        e = lambda s: _absent(tr, _stored(tr, 300, s), s + 1)
        x = np.concatenate([e(20), _stored(tr, 70, 26), base[None], e(22), base[None], _stored(tr, 70, 27), e(24)])
        ln = np.concatenate([np.full(300, k), np.full(70, fl), [fl], np.full(300, k), [nine_f + 1], np.full(70, fl), np.full(300, k)])
        return x, ln
    if what == "one":
        return base[None].copy(), np.array([nine_f + 1])
    if what == "spanning":  # one filtered prefix over the whole table between one-candidate neighbours
        x = np.concatenate([_stored(tr, 5, 30), base[None], _stored(tr, 5, 31)])
        return x, np.array([fl] * 5 + [1] + [fl] * 5)
    if what == "heads":  # a filtered prefix of several candidates with its first candidate at chosen places of the stream
        many = pack(base[None], [k - 1])
        cm = int(tr.answer(*many).cand[0])
        assert 2 <= cm <= 62
        pad = _stored(tr, 1200, 32)
        x, ln, at, used = [], [], 0, 0
        for target in HEAD_TARGETS:
            assert target >= at
            x += [pad[used:used + target - at], base[None]]
            ln += [np.full(target - at, fl), [k - 1]]
            used += target - at
            at = target + cm
        return np.concatenate(x), np.concatenate(ln)
    raise KeyError(what)


HEAD_TARGETS = (63, 128, 193, 255, 511, 767 + 64)  # lane 63, 0, 1; tile position 255 twice (the run goes on in the next chunk); lane 63
RUN_SHAPES = ("ones256", "ones257", "alternating", "duplicates", "hit_miss", "empty_runs", "one", "spanning", "heads")
GRID_STRIDE_N = CHUNKS * TILE + 300


def bounds(tr, what):
    k = tr.k
    if what == "outside":  # (the G index: nothing below CAAAAAAAA.. or above its last row) intervals at row 0 and at n_rows, both empty
        x = np.zeros((4, k), np.uint8)
        x[1], x[3] = 3, 3
        return x, np.array([9, 9, k, k])
    if what == "whole":
        x = np.zeros((4, k), np.uint8)
        x[:, 0] = np.arange(4)
        return x, np.full(4, 1)
    if what == "single":  # every length of the one stored k-mer, of a k-mer that differs in its first and in its last nucleotide, and A C G T
        p = tr.codes[0]
        q, r = p.copy(), p.copy()
        q[0] ^= 1
        r[-1] ^= 2
        x = np.concatenate([np.tile(p, (k, 1)), np.tile(q, (k, 1)), np.tile(r, (k, 1)), np.zeros((4, k), np.uint8)])
        x[3 * k:, 0] = np.arange(4)
        return x, np.concatenate([np.arange(1, k + 1)] * 3 + [np.full(4, 1)])
    if what == "grid_stride":  # more prefixes than k_pm_bounds has lanes: full length, half stored, half one substitution away
        rng = np.random.default_rng(40)
        x = tr.codes[rng.integers(0, tr.N, GRID_STRIDE_N)]
        half = np.arange(GRID_STRIDE_N) & 1 == 1
        pos = rng.integers(0, k, GRID_STRIDE_N)
        x[half, pos[half]] = (x[half, pos[half]] + rng.integers(1, 4, int(half.sum()))) & 3
        return x, np.full(GRID_STRIDE_N, k)
    raise KeyError(what)


def every_length(tr):
    """per length 1..k: the base k-mer's prefix, the same with the first nucleotide of the block it ends in changed (same interval, other
    filter value; garbage where the prefix ends on a block boundary) and the same with its last nucleotide changed"""
    k, p = tr.k, tr.bases[0]
    x, ln = [], []
    for n in range(1, k + 1):
        f = n // 9
        q, r = p.copy(), p.copy()
        if 9 * f < k:
            q[9 * f] = (q[9 * f] + 1) & 3
        r[n - 1] = (r[n - 1] + 2) & 3
        x += [p, q, r]
        ln += [n, n, n]
    return np.array(x), np.array(ln)


# (name, index, k, builder): every batch of the GPU file.  Built on demand, cached with their truth.
def _cases():
    out = []
    for Ccand in GEOMETRY:
        out.append(("geometry-%d" % Ccand, "family", 27, lambda tr, c=Ccand: geometry(tr, c)))
    for k in (126, 27):
        out.append(("all_kept-%d" % k, "family", k, lambda tr: repeated(tr, [_head(tr)], [9], 4 * CHUNKS * TILE // 2)))
    for k in (27, 90):
        out.append(("quarter_kept-%d" % k, "family", k, lambda tr: repeated(tr, np.arange(4)[:, None] * np.ones((1, tr.k), np.uint8), [1] * 4, 2 * CHUNKS * TILE)))
    out.append(("none_kept", "no_g", G_K, lambda tr: (np.full((G_REPEATS, G_K), G, np.uint8), np.full(G_REPEATS, 1))))
    out.append(("one_kept", "one_g", G_K, lambda tr: (np.full((G_REPEATS, G_K), G, np.uint8), np.full(G_REPEATS, 1))))
    for k in (27, 90):
        for what in RUN_SHAPES:
            out.append(("runs-%s-%d" % (what, k), "family", k, lambda tr, w=what: runs(tr, w)))
    out.append(("bounds-outside", "no_g", G_K, lambda tr: bounds(tr, "outside")))
    for k in (27, 90):
        out.append(("bounds-whole-%d" % k, "family", k, lambda tr: bounds(tr, "whole")))
    out.append(("bounds-single", "single", 27, lambda tr: bounds(tr, "single")))
    out.append(("bounds-grid_stride", "family", 27, lambda tr: bounds(tr, "grid_stride")))
    for k in KS_EDGE:
        out.append(("every_length-%d" % k, "family", k, every_length))
    return {name: (idx, k, fn) for name, idx, k, fn in out}


CASES = _cases()


class Case:
    pass


@functools.lru_cache(maxsize=4)
def case(name):
    """the batch (packed prefixes, lengths), its index's truth and its answer"""
    idx, k, fn = CASES[name]
    c = Case()
    c.name, c.index, c.k, c.tr = name, idx, k, index(idx, k)
    x, ln = fn(c.tr)
    c.pref, c.lens = pack(x, ln, seed=len(name))
    c.ans = c.tr.answer(c.pref, c.lens)
    return c


def names(prefix):
    return [n for n in CASES if n.startswith(prefix)]


def tiles_of(ans):
    """per tile of the stream (in chunk order): (chunk, first candidate, candidates, kept) -- the chunks from the library's plan"""
    cs, begins, ends = chunks(ans.C)
    ck = np.concatenate([[0], np.cumsum(ans.keep)])
    out = []
    for g in np.flatnonzero(ends > begins):
        for j0 in range(int(begins[g]), int(ends[g]), TILE):
            j1 = min(j0 + TILE, int(ends[g]))
            out.append((int(g), j0, j1 - j0, int(ck[j1] - ck[j0])))
    return cs, begins, ends, out


# ---- tests: the truth itself ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hostlib():
    subprocess.check_call(["make", "-C", _lib.CSRC, "all"], stdout=subprocess.DEVNULL)
    lib = C.CDLL(os.path.join(_lib.CSRC, "libbft_hosttest.so"))
    lib.bft_hosttest_roundtrip.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p]
    return lib


@pytest.mark.parametrize("k", KS_EDGE)
def test_t_form_key_is_the_librarys(hostlib, k):
    tr = family(k)
    pick = np.unique(np.concatenate([np.arange(0, tr.N, 97), [tr.N - 1]]))
    packed = np.ascontiguousarray(tr.packed[pick])
    W = tr.W
    out, tf = np.zeros_like(packed), np.zeros(len(packed) * W, dtype=np.uint64)
    hostlib.bft_hosttest_roundtrip(packed.ctypes.data, len(packed), k, out.ctypes.data, tf.ctypes.data)
    assert (out == packed).all()
    got = [sum(int(w) << (64 * (W - 1 - j)) for j, w in enumerate(tf[i * W:(i + 1) * W])) for i in range(len(packed))]
    want = t_key_ints(tr.codes[pick], k)
    assert got == want
    assert all(a < b for a, b in zip(want, want[1:]))  # and the table is in the order of those keys
    assert (tr.codes[0] == 0).all() and (tr.codes[-1] == 3).all()  # all-A and all-T: lo / hi touch both ends


@pytest.mark.parametrize("k", KS_EDGE)
def test_every_length_matches_are_the_definition(k):
    """The matches drawn from the candidates are the rows the definition names, for every length, with garbage behind the prefix; and the
    filter alone decides: every prefix of the base k-mer that ends inside a block has candidates it keeps and candidates it rejects."""
    c = case("every_length-%d" % k)
    tr, ans = c.tr, c.ans
    pc = S.unpack_codes(c.pref, k)
    x, ln = every_length(tr)
    assert len(c.pref) == 3 * k and (c.lens == ln).all() and (c.lens.reshape(k, 3) == np.arange(1, k + 1)[:, None]).all()
    for i in range(len(c.pref)):
        n = int(c.lens[i])
        assert (pc[i, :n] == x[i, :n]).all()
        want = tr.brute(x[i], n)
        got = ans.rows[int(ans.offsets[i]):int(ans.offsets[i + 1])]
        assert len(got) == len(want) and (got == want).all(), (k, i, n)
    assert (pc != x).any()  # there is garbage
    L = k // 9
    for n in range(1, k + 1):
        f, m = divmod(n, 9)
        i = 3 * (n - 1)
        assert ans.kept[i] >= 1
        if m and f < L:
            assert ans.filt[i] and ans.cand[i] > ans.kept[i] > 0, (k, n)
            assert ans.filt[i + 1] and ans.cand[i + 1] == ans.cand[i] and ans.a[i + 1] == ans.a[i] and ans.kept[i + 1] > 0  # the SNP twin
            assert set(ans.rows[int(ans.offsets[i]):int(ans.offsets[i + 1])]).isdisjoint(ans.rows[int(ans.offsets[i + 1]):int(ans.offsets[i + 2])])
        else:
            assert not ans.filt[i] and ans.cand[i] == ans.kept[i]
    assert ans.a.min() == 0 and (ans.a + ans.cand).max() == tr.N


def test_key_widths_filter_words_and_shifts_all_occur():
    """B mod 4 takes every value at W = 1; W = 1..4; the filter's field lies in every word of every width, at bit 62 of a word and at bit 0"""
    assert {S.kmer_bytes(k) % 4 for k in KS_EDGE if 2 * k <= 64} == {0, 1, 2, 3}
    assert {(2 * k + 63) // 64 for k in KS_EDGE} == {1, 2, 3, 4}
    seen, shifts, by_k = set(), set(), {}
    for k in KS_EDGE:
        W, order = (2 * k + 63) // 64, t_order(k).tolist()
        for n in range(1, k + 1):
            d, fpos = rule(k, n)
            if fpos < 0:
                continue
            fsh = 2 * (k - 1 - order.index(fpos))  # the digit's bit in the key, from the least significant
            seen.add((W, W - 1 - (fsh >> 6)))
            by_k.setdefault(k, set()).add(W - 1 - (fsh >> 6))
            shifts |= {"zero"} if fsh == 0 else {fsh % 64}
            if k == 72 and n < 9:
                assert fsh % 64 == 62
    assert seen == {(W, w) for W in (1, 2, 3, 4) for w in range(W)}, seen
    assert 0 in by_k[90] and by_k[126] == {0, 1, 2, 3}  # k = 90: word 0 of 3; k = 126: all four
    assert 62 in shifts and "zero" in shifts
    for k in KS_EDGE:
        assert family(k).member.sum(axis=0).min() > 0 and len(np.unique(family(k).setmask)) == 7  # several colour sets


# ---- tests: the plan -----------------------------------------------------------------------------------------------------------------------------
def test_plan_is_the_stated_rule():
    """chunk size = ceil(C / 2048) rounded up to whole tiles of 256; chunk g = [min(C, g cs), min(C, (g + 1) cs))"""
    lib = _lib.load()
    out = (C.c_uint64 * 3)()
    assert lib.bft_gpu_debug_prefix_plan(1000, CHUNKS - 1, out) == 0
    for Ccand in (0, 1, 255, 256, 257, 524287, 524288, 524289, 1048576, 1048577, 1572865, 10 ** 7 + 3, 2 ** 32 + 5, 2 ** 40):
        cs, begins, ends = chunks(Ccand)
        want = -(-(-(-Ccand // CHUNKS)) // TILE) * TILE
        assert cs == want and cs % TILE == 0
        g = np.arange(CHUNKS, dtype=object)
        assert begins.tolist() == [min(Ccand, int(x) * cs) for x in g] and ends.tolist() == [min(Ccand, (int(x) + 1) * cs) for x in g]
        assert ends[-1] == Ccand and begins[0] == 0


def test_prefix_plan_symbol_errors_and_header():
    subprocess.check_call(["make", "-C", _lib.CSRC, "all"], stdout=subprocess.DEVNULL)
    hdr = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+bft_gpu_debug_prefix_plan\s*\(\s*uint64_t\s+C\s*,\s*uint32_t\s+chunk\s*,\s*uint64_t\s+out\s*\[\s*3\s*\]\s*\)\s*;", hdr)
    assert "bft_gpu_debug_prefix_plan" in _lib.SIGNATURES
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert "bft_gpu_debug_prefix_plan" in set(re.findall(r" T (bft_gpu_[a-z_0-9]+)", out))
    lib = _lib.load()
    buf = (C.c_uint64 * 3)()
    assert lib.bft_gpu_debug_prefix_plan(16, 0, None) == -1  # BFT_GPU_E_ARG
    assert lib.bft_gpu_debug_prefix_plan(16, CHUNKS, buf) == -1 and lib.bft_gpu_debug_prefix_plan(16, 0xFFFFFFFF, buf) == -1
    assert lib.bft_gpu_debug_prefix_plan(16, CHUNKS - 1, buf) == 0 and list(buf) == [TILE, 16, 16]
    # one definition of the rule for the kernels and the hook
    src = open(os.path.join(_lib.CSRC, "bft_prefix.hip")).read()
    inc = open(os.path.join(_lib.CSRC, "bft_prefix.h")).read()
    assert len(re.findall(r"\bvoid\s+pm_chunk\s*\(", inc)) == 1 and not re.search(r"\bvoid\s+pm_chunk\s*\(", src)
    assert len(re.findall(r"\bpm_chunk\s*\(", src)) == 3 and "PM_THREADS =" not in src and "PM_THREADS = %d" % TILE in inc
    # the header's sentence on alignment, at the device call
    full = open(_lib.HEADER).read()
    doc = full[full.index("The same on a RESIDENT batch, without synchronisation (runs on hip_stream"):full.index("int bft_gpu_query_prefixes_dev(")]
    doc = " ".join(doc.replace("*", " ").split())
    assert "d_kmers_out may have any alignment" in doc
    assert re.search(r"d_rows_out, d_colorsets_out \(uint32\), d_offsets and d_needed \(uint64\) are naturally aligned", doc)


# ---- tests: every batch is what it claims --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Ccand", sorted(GEOMETRY))
def test_geometry_batches(Ccand):
    c = case("geometry-%d" % Ccand)
    assert c.ans.C == Ccand
    cs, begins, ends, tiles = tiles_of(c.ans)
    full = ends - begins
    want_tiles, want_empty, want_last = GEOMETRY[Ccand]
    assert int((full == 0).sum()) == want_empty
    if Ccand:
        assert cs == want_tiles * TILE and full.max() == min(cs, Ccand) and int(full[full > 0][-1]) == want_last
        assert max(np.bincount([t[0] for t in tiles])) == -(-min(cs, Ccand) // TILE)
        assert sum(t[2] for t in tiles) == Ccand
        r, s = divmod(Ccand, c.tr.N)
        assert int((c.lens == 1).sum()) == r and int((c.lens == c.k).sum()) == s and (c.ans.cand[c.lens == c.k] == 1).all()
    else:
        assert len(c.pref) == 1 and c.ans.total == 0
    if Ccand == 1048577:  # three tiles, the last chunk ragged, its last tile holding one candidate
        assert [t[2] for t in tiles if t[0] == tiles[-1][0]] == [256, 1]
    if Ccand == 1572865:
        assert want_tiles >= 4


@pytest.mark.parametrize("name", names("all_kept") + names("quarter_kept") + ["none_kept", "one_kept"])
def test_density_batches(name):
    c = case(name)
    ans = c.ans
    cs, begins, ends, tiles = tiles_of(ans)
    assert ans.C > 2 * CHUNKS * TILE and cs >= 3 * TILE  # three tiles per chunk and more
    frac = ans.total / ans.C
    kept_per_tile = np.array([t[3] for t in tiles])
    if name.startswith("all_kept"):
        assert ans.keep.all() and not ans.filt.any() and (c.lens == 9).all() and len(c.pref) > 250
        assert ans.cand[0] % TILE != 0 and ans.cand[0] >= HEAD_FAMILY - 2  # the runs' edges move through the tiles
        if c.k == 126:
            assert TILE * c.tr.nb == 8192  # the k-mers of a full tile fill s_kmers
    elif name.startswith("quarter_kept"):
        assert ans.filt.all() and 0.15 < frac < 0.35 and (ans.cand == c.tr.N).all()
        assert kept_per_tile.min() == 0 or kept_per_tile.min() < 64  # (tiles of every density)
    elif name == "none_kept":
        assert ans.total == 0 and ans.filt.all() and (ans.cand == c.tr.N).all()
    else:
        assert c.tr.N == 10240 and ans.total == len(G_RANKS) * G_REPEATS and cs == 3 * TILE
        j = np.flatnonzero(ans.keep)
        assert (np.diff(j) > 50).all() and kept_per_tile.max() == 1  # exactly one kept between long runs of rejected ones
        assert {0, 63, 64, 255} <= set((j % TILE).tolist())  # the tile positions (chunks begin on multiples of a tile)
        assert np.isin(j, begins[ends > begins]).any() and np.isin(j, ends[ends > begins] - 1).any()  # first / last candidate of a chunk
        assert sorted(set(ans.rows.tolist())) == list(G_RANKS) and (c.tr.tags[list(G_RANKS)] == TAG_G).all()


@pytest.mark.parametrize("k", (27, 90))
@pytest.mark.parametrize("what", RUN_SHAPES)
def test_run_shape_batches(what, k):
    c = case("runs-%s-%d" % (what, k))
    ans, lens, n = c.ans, c.lens, len(c.pref)
    fhead = ans.coff[:-1][(ans.cand > 0) & ans.filt]  # the stream position of the first candidate of every filtered prefix that has one
    pc = S.unpack_codes(c.pref, k)
    same = lambda i, j: lens[i] == lens[j] and (pc[i, :lens[i]] == pc[j, :lens[i]]).all()
    if what in ("ones256", "ones257"):
        assert n == int(what[4:]) and (ans.cand == 1).all() and ans.filt.all() and (ans.kept == 1).all()
        assert set((fhead % 64).tolist()) == set(range(64)) and 255 in fhead and ((256 in fhead) == (n == 257))
    elif what == "alternating":
        assert (ans.cand == 1).all() and (ans.filt == (np.arange(n) % 2 == 0)).all() and (ans.kept == 1).all()
    elif what == "duplicates":
        d = np.array([same(i, i + 1) for i in range(n - 1)])
        assert d.sum() >= 50 and (ans.kept[:-1][d] == ans.kept[1:][d]).all()
        assert (ans.cand[:-1][d] == 0).any() and (ans.cand[:-1][d] == 1).any() and (ans.cand[:-1][d] > 64).any() and (ans.filt[:-1][d] & (ans.kept[:-1][d] > 1)).any()
    elif what == "hit_miss":
        assert (ans.kept[0::2] == 1).all() and (ans.kept[1::2] == 0).all() and (ans.cand[1::4] == 0).all() and (ans.cand[3::4] == 1).all()
    elif what == "empty_runs":
        z = ans.cand == 0
        assert z[:300].all() and z[-300:].all() and z[371:671].all() and not z[300:371].any() and not z[671:742].any() and n == 1042
        assert ans.kept[370] >= 1 and ans.kept[671] >= 1 and ans.cand[671] > ans.kept[671]
    elif what == "one":
        assert n == 1 and ans.filt[0] and ans.cand[0] > ans.kept[0] > 0
    elif what == "spanning":
        cs, begins, ends, tiles = tiles_of(ans)
        assert ans.cand[5] == c.tr.N and ans.filt[5] and (np.delete(ans.cand, 5) == 1).all()
        assert len({t[0] for t in tiles}) >= 20 and cs == TILE  # the one prefix's candidates lie in that many workgroups
    elif what == "heads":
        many = lens == k - 1
        mh = ans.coff[:-1][many]
        assert mh.tolist() == list(HEAD_TARGETS) and ans.filt[many].all() and (ans.cand[many] == ans.cand[many][0]).all() and 2 <= ans.cand[many][0] <= 62
        assert (ans.kept[many] >= 1).all() and (ans.kept[many] < ans.cand[many]).all()
        assert {0, 1, 63} <= set((mh % 64).tolist()) and 255 in (mh % TILE).tolist()
        cs, begins, ends = chunks(ans.C)
        assert cs == TILE  # so a run that starts at tile position 255 goes on at position 0 of the next workgroup's chunk (stream position 256)
        assert ((mh % 64) + ans.cand[many] > 64).any()  # and a run that goes on in the next wavefront


def test_bounds_batches():
    c = case("bounds-outside")
    assert (c.ans.cand == 0).all() and sorted(set(c.ans.a.tolist())) == [0, c.tr.N]  # a == 0 and a == n_rows
    for k in (27, 90):
        c = case("bounds-whole-%d" % k)
        assert (c.ans.cand == c.tr.N).all() and c.ans.total == c.tr.N and (c.ans.kept > 0).all()
    c = case("bounds-single")
    assert c.tr.N == 1 and c.ans.total == 27 + 26 + 1 and set(c.ans.kept.tolist()) == {0, 1}
    assert (c.ans.kept[:27] == 1).all() and (c.ans.kept[27:54] == 0).all() and (c.ans.kept[54:80] == 1).all() and c.ans.kept[80] == 0
    c = case("bounds-grid_stride")
    n = len(c.pref)
    assert n == GRID_STRIDE_N > CHUNKS * TILE  # more prefixes than the capped grid of k_pm_bounds has lanes: the stride loop runs twice
    assert (c.lens == 27).all() and (c.ans.kept[0::2] == 1).all() and 0.9 < (c.ans.kept[1::2] == 0).mean() <= 1.0
    assert c.ans.kept[CHUNKS * TILE:].sum() >= 100  # hits among the prefixes of the second turn
