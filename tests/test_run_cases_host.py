"""The cases of the run-stage edge tests (tests/test_gpu_run_edges.py runs them on the GPU), their ground truth, and -- here, without a GPU -- the proof
that each case is what its name says.

The run stage (csrc/bft_run.hip) turns the insertion log into a run: sorted distinct k-mers, the offsets of their genome-id lists, the ids.  A log takes
one of three families of roads -- composites k-mer << gb | id of up to 63 bits, (k-mer, id) pairs of ordered one-word keys with the ids in 1, 2 or 4
bytes, and "whatever is left" (keys of 2 .. 4 words, ids out of order, "build_composite" 0) --, each behind the root-prefix split or device-wide.  The
split variants are tests/test_gpu_front_edges.py's; the cases here take the DEVICE-WIDE variants (what every build below 2^20 pairs takes and what every
split road falls back to), each at the edges of its host-side arithmetic, of its key and id widths, of the table of insert calls and of the log's format.

A case is (k, the list of insert calls (id, k-mers), options, the intended road).  The road is written by hand as [road, gb, id bytes, split tried] from
the rules as DESIGN.md section 4 and the comments of csrc/bft_run_plan.h state them; test_the_plan_agrees_with_every_road asks the library's own rules
(bft_gpu_debug_run_plan: no handle, no device) about every case, and test_condition_table counts, over all cases, every line of the table of
conditions: each must be met at least once.

Truth, in Python only and from the list of insert calls alone (test_front_cases_host.Truth): a dict k-mer -> sorted distinct ids, the k-mers in the
order of their T-form keys, the numbers of distinct k-mers and pairs.  The T-form key is that of test_graph_cases_host (t_order, keys_u64), here in
pieces of 32 digits for k > 64, pinned to bft_hosttest_roundtrip for every k used.  The four cases beyond 5 x 10^5 pairs compute the same truth with
numpy (NpTruth: a lexicographic sort over (key words, id)), pinned to the dict truth on small cases.

An insert call of no k-mers: BFT.insert_kmers hands it to the library, and the library returns before it looks at the log (bft_gpu_insert_kmers,
bft_gpu_insert_kmers_dev: `if (n == 0) return BFT_GPU_OK`; the sequence ingest commits only non-empty pieces).  So the table of insert calls never
holds two equal ends, and an empty call's id neither widens gb or the dictionary's ids nor ends the ascending order of the ids.  The cases with empty
calls state exactly that: their roads and their truth are those of the same calls without the empty ones, whatever id the empty calls name.  The GPU
file makes those calls through _lib with n = 0.

Sizes: a case is one to a few thousand pairs, except the table cases (65 536 | 65 537 insert calls), the logs that grow after they were taken apart
(> 65 536 pairs behind the id without room) and the four large ones: (threads of a capped grid + 300) pairs on the composite and on the W = 3 road, and
2^20 - 1 | 2^20 pairs at k = 27 under "build_msd" 1."""
import collections
import ctypes as C
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_front_cases_host as H  # noqa: E402  (Truth, keys_of, codes_of, bits_for)
import test_graph_cases_host as G  # noqa: E402  (pack, keys_u64; G.P.t_order)

from bloomfiltertrie_amd import _lib  # noqa: E402  (the road rules and the host test library of the pin, nothing else)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMPOSITE, PAIRS, GENERAL = 0, 1, 2  # bft_gpu_debug_run_road's first word
SPLIT_FROM = 1 << 20                 # "build_msd" 1: the root-prefix split from this many pairs on
GRID_THREADS = 2048 * 256            # a capped launch grid: 2048 workgroups of 256 threads (held against the library below)
GRID_LOOSE = 300
CALL_TABLE_MAX = 1 << 16             # the multi-word sort reads ids from the table of insert calls up to this many entries
IDS4 = (0, 3, 5, 300)
CL0 = {"composite_log": 0}


# ---- the road rules, from the library ---------------------------------------------------------------------------------------------------------------
def plan(k, ordered, composite, msd, comp_log, max_gid, log_max_gid, total):
    """bft_gpu_debug_run_plan: [road, gb, id bytes, split tried, id bits of a composite log, 1: still composites at build, grid threads, table limit]"""
    out = (C.c_uint32 * 8)()
    _lib.check(_lib.load().bft_gpu_debug_run_plan(k, int(ordered), int(composite), int(msd), int(comp_log), max_gid, log_max_gid, total, out))
    return [int(x) for x in out]


def words_of(k):
    return (2 * k + 63) // 64


# ---- keys ---------------------------------------------------------------------------------------------------------------------------------------------
def keys_of(codes, k):
    """the T-form keys of [n, k] codes as Python integers, any k: keys_u64 over pieces of 32 digits, most significant first"""
    order = G.P.t_order(k).tolist()
    out = [0] * len(codes)
    for a in range(0, k, 32):
        piece = order[a:a + 32]
        out = [(x << (2 * len(piece))) | y for x, y in zip(out, G.keys_u64(codes, piece).tolist())]
    return out


def key_words(codes, k):
    """the same keys as the library holds them: W uint64 arrays, word 0 the most significant (2k - 64 (W - 1) bits)"""
    order = G.P.t_order(k).tolist()
    W = words_of(k)
    top = k - 32 * (W - 1)
    return [G.keys_u64(codes, order[:top])] + [G.keys_u64(codes, order[top + 32 * j:top + 32 * (j + 1)]) for j in range(W - 1)]


def _absent(tr, n, seed):
    """packed one-base mutants of a sample of the stored k-mers, none of them stored (any k)"""
    rng = np.random.default_rng(seed)
    have, out = set(tr.order), []
    for i in rng.integers(0, tr.kmers, 4 * n).tolist():
        x = tr.codes[i].copy()
        j = int(rng.integers(0, tr.k))
        x[j] = (x[j] + int(rng.integers(1, 4))) & 3
        if keys_of(x[None], tr.k)[0] not in have:
            out.append(x)
        if len(out) == n:
            break
    return G.pack(np.array(out, dtype=np.uint8))


# ---- truth --------------------------------------------------------------------------------------------------------------------------------------------
class Truth(H.Truth):
    """test_front_cases_host.Truth (a dict k-mer -> sorted distinct ids from the inserted pairs alone) with the keys of any k"""

    def __init__(self, k, codes, gids):
        super().__init__(k, keys_of(codes, k), gids, codes)

    def absent(self, n, seed):
        return _absent(self, n, seed)


class NpTruth:
    """the same truth for the large cases: one lexicographic sort over (key words, id), a new k-mer where a key word changes, a new pair where the
    id changes as well"""

    def __init__(self, k, codes, gids):
        gids = np.asarray(gids, dtype=np.uint32)
        w = key_words(codes, k)
        perm = np.lexsort([gids] + w[::-1])  # (the last key is the primary one: word 0)
        ws, gs = [x[perm] for x in w], gids[perm]
        head = np.ones(len(gs), dtype=bool)
        head[1:] = np.logical_or.reduce([x[1:] != x[:-1] for x in ws])
        keep = head.copy()
        keep[1:] |= gs[1:] != gs[:-1]
        self.k, self.kmers, self.pairs = k, int(head.sum()), int(keep.sum())
        first = np.flatnonzero(head)
        self.codes = np.ascontiguousarray(codes[perm[first]])
        self.packed = G.pack(self.codes)
        words = [x[first].tolist() for x in ws]
        self.order = [functools.reduce(lambda a, b: (a << 64) | b, t) for t in zip(*words)]
        ids, off = gs[keep].tolist(), np.concatenate([np.flatnonzero(head[keep]), [self.pairs]]).tolist()
        self.sets = {x: tuple(ids[a:b]) for x, a, b in zip(self.order, off[:-1], off[1:])}

    def absent(self, n, seed):
        return _absent(self, n, seed)


# ---- the comparison (tests/test_gpu_run_edges.py hands it what the handle returns) ---------------------------------------------------------------------
def compare(tr, kmers, cs, sets, n_kmers, n_pairs):
    """What is wrong with a built index, as a list of findings (empty: nothing).  kmers [n, bytes] and cs [n]: the k-mers and their colour-set ids as
    extract() returns them; sets: {colour-set id: the ids as colorset() returns them, not re-sorted}; n_kmers, n_pairs: info()'s counts."""
    bad = []
    cs = [int(c) for c in cs]
    if tuple(kmers.shape) != tuple(tr.packed.shape):
        bad.append(f"k-mers: {kmers.shape[0]} extracted, {tr.kmers} inserted")
    else:
        d = np.flatnonzero((kmers != tr.packed).any(axis=1))
        if len(d):
            bad.append(f"k-mers: not the inserted ones in key order, first at row {int(d[0])}")
    for c in sorted(set(cs)):
        s = list(sets[c])
        if any(b <= a for a, b in zip(s, s[1:])):
            bad.append(f"colour set {c}: ids not strictly ascending {s[:8]}")
    want = [tr.sets[x] for x in tr.order]
    got = [tuple(sets[c]) for c in cs]
    if len(got) == len(want):
        d = [i for i, (a, b) in enumerate(zip(got, want)) if a != b]
        if d:
            bad.append(f"colour sets: {len(d)} k-mers under other ids, first at row {d[0]}: {got[d[0]][:8]} for {want[d[0]][:8]}")
    if sum(len(g) for g in got) != tr.pairs:
        bad.append(f"pairs: the lists hold {sum(len(g) for g in got)}, {tr.pairs} inserted")
    if (int(n_kmers), int(n_pairs)) != (tr.kmers, tr.pairs):
        bad.append(f"info: {int(n_kmers)} k-mers and {int(n_pairs)} pairs for {tr.kmers} and {tr.pairs}")
    return bad


def ideal(tr):
    """what a correct index returns for this truth: (kmers, cs, sets, kmers, pairs) -- the colour sets numbered in the order of their first k-mer"""
    ids = {}
    cs = np.array([ids.setdefault(tr.sets[x], len(ids)) for x in tr.order], dtype=np.uint32)
    return tr.packed.copy(), cs, {i: list(s) for s, i in ids.items()}, tr.kmers, tr.pairs


# ---- cases ----------------------------------------------------------------------------------------------------------------------------------------------
class Case:
    """calls: [(genome id, codes [m, k])] in the order of the insert calls (m = 0: an empty call); road: [road, gb, id bytes, split tried] of the LAST build,
    by hand; options: what the handle is set to ("composite_log", "build_composite", "build_msd", "flush_pairs"); first: the calls in front of an
    earlier build() on the same handle (a two-step case) with that build's road; big: truth by numpy, no per-pair facts; dev: (table of codes, [(id, first
    row, rows)]) for the cases that insert from one resident array"""

    def __init__(self, name, k, calls, road, options=None, first=None, first_road=None, big=False, ids=None, dev=None):
        self.name, self.k, self.W, self.road, self.big, self.dev = name, k, words_of(k), list(road), big, dev
        self.calls = [(int(g), np.asarray(c, dtype=np.uint8).reshape(-1, k)) for g, c in calls]
        self.first = None if first is None else [(int(g), np.asarray(c, dtype=np.uint8).reshape(-1, k)) for g, c in first]
        self.first_road = None if first_road is None else list(first_road)
        self.options = {"composite_log": 1, "build_composite": 1, "build_msd": 1}
        self.options.update(options or {})
        self.ids = tuple(ids) if ids is not None else tuple(sorted({g for g, c in (self.first or []) + self.calls if len(c)}))

    @staticmethod
    def _flat(calls):
        return np.concatenate([c for _, c in calls]), np.concatenate([np.full(len(c), g, dtype=np.uint32) for g, c in calls])

    def _truth(self, calls):
        codes, gids = self._flat(calls)
        return NpTruth(self.k, codes, gids) if self.big else Truth(self.k, codes, gids.tolist())

    @functools.cached_property
    def truth(self):
        """of everything inserted (both steps of a two-step case)"""
        return self._truth((self.first or []) + self.calls)

    @functools.cached_property
    def truth_first(self):
        return self._truth(self.first)

    def inserts(self, calls=None):
        """[(genome id, packed k-mers [m, bytes])]"""
        return [(g, G.pack(c)) for g, c in (self.calls if calls is None else calls)]

    # -- what the log of the last build looks like: from the calls and "flush_pairs" (the log is merged into the index before it would pass it)
    def last_log(self):
        """(the non-empty calls of the last build's log, the largest id the handle has seen)"""
        log, seen, n = [], [g for g, c in (self.first or []) if len(c)], 0
        for g, c in self.calls:
            if len(c) == 0:
                continue
            if n and n + len(c) > self.options.get("flush_pairs", 1 << 30):
                log, n = [], 0
            log.append((g, c))
            seen.append(g)
            n += len(c)
        return log, max(seen)

    def plan(self, calls=None, max_gid=None):
        if calls is None:
            calls, max_gid = self.last_log()
        g = [x for x, _ in calls]
        o = self.options
        return plan(self.k, g == sorted(g), o["build_composite"], o["build_msd"], o["composite_log"], max_gid, max(g), sum(len(c) for _, c in calls))

    def plan_first(self):
        calls = [(g, c) for g, c in self.first if len(c)]
        return self.plan(calls, max(g for g, _ in calls))

    @property
    def family(self):
        return {COMPOSITE: "composite", PAIRS: "pairs", GENERAL: f"general_w{self.W}"}[self.road[0]]


def _fresh(rng, k, n):
    """n distinct keys strictly inside the key range (neither in its lowest nor in its highest eighth), ascending"""
    lo, hi = 1 << (2 * k - 3), (1 << (2 * k)) - (1 << (2 * k - 3))
    out = set()
    while len(out) < n:
        out.add(lo + int.from_bytes(rng.bytes(40), "little") % (hi - lo))
    return sorted(out)


def _shuffled(rng, keys):
    return [keys[i] for i in rng.permutation(len(keys)).tolist()]


def _body(rng, k, S, m=120):
    """{slot: keys}: m k-mers, a third of them under every id, a third under one, a third under two; every fifth with a duplicate pair"""
    per = {s: [] for s in range(S)}
    for i, x in enumerate(_fresh(rng, k, m)):
        slots = list(range(S)) if i % 3 == 0 else [i % S] if i % 3 == 1 else sorted({i % S, S - 1})
        for s in slots:
            per[s].append(x)
        if i % 5 == 4:
            per[slots[-1]].append(x)
    return per


def _rows(rng, per, split=1):
    """[(slot, keys)] in ascending slot order, the keys of a call shuffled, slot `split` in two consecutive calls"""
    rows = []
    for s in sorted(per):
        keys = _shuffled(rng, per[s])
        if not keys:
            continue
        cut = len(keys) // 3 if s == split and len(keys) >= 3 else 0
        rows += [(s, keys[:cut]), (s, keys[cut:])] if cut else [(s, keys)]
    return rows


SHAPES = ("mixed", "edge_new_kmer", "edge_new_id", "edge_dup", "total_1", "total_2", "total_255", "total_256", "total_257", "same_pair", "one_kmer",
          "distinct_one_id", "dup_far", "low_bit", "high_bit", "word_bits")
ONE_ID_SHAPES = ("total_1", "same_pair", "distinct_one_id")


def shape_rows(shape, k, S, rng, unordered=False):
    """[(slot, keys)] in the order of the calls: the ids ascend unless `unordered` (then: where the shape has more than one id)"""
    lowest, highest = 0, (1 << (2 * k)) - 1  # the two ends of the key range
    last = S - 1
    if shape == "mixed":
        rows = _rows(rng, _body(rng, k, S))
    elif shape.startswith("edge_"):
        per = _body(rng, k, S)
        if shape == "edge_new_kmer":  # the first and the last sorted pair are alone with their k-mer
            per[1].append(lowest)
            per[last].append(highest)
        elif shape == "edge_new_id":  # ... share their k-mer with one more id
            for s in (0, last):
                per[s] += [lowest, highest]
        else:  # ... are there twice
            per[0] += [lowest, lowest]
            per[last] += [highest, highest]
        rows = _rows(rng, per)
    elif shape.startswith("total_"):
        n = int(shape[6:])
        if n == 1:
            rows = [(last, _fresh(rng, k, 1))]
        elif n == 2:
            x = _fresh(rng, k, 1)
            rows = [(0, x), (last, x)]
        else:
            m = (2 * n + 2) // 3
            keys = _fresh(rng, k, m)
            per = {s: [] for s in range(S)}
            for i, x in enumerate(keys):
                per[(last - i) % S].append(x)
            for j in range(n - m):
                per[(last - 1 - j) % S].append(keys[j])
            rows = _rows(rng, per)
    elif shape == "same_pair":
        x = _fresh(rng, k, 1)
        rows = [(last, x * 120), (last, x * 80)]
    elif shape == "one_kmer":
        x = _fresh(rng, k, 1)
        rows = [(s, x * (1 + s % 2)) for s in range(S)]
    elif shape == "distinct_one_id":
        rows = [(last, _shuffled(rng, _fresh(rng, k, 300)))]
    elif shape == "dup_far":  # one pair in several calls, other pairs between its copies in the log
        keys = _fresh(rng, k, 81)
        x, fill = keys[40], _shuffled(rng, keys[:40] + keys[41:])
        if unordered:  # ids 5, 3, 5 (slots 2, 1, 2 of 0, 3, 5, ..): the two (x, 5) only become neighbours through the id pass
            return [(2, [x] + fill[:20]), (1, [x] + fill[20:40]), (2, fill[40:60] + [x]), (last, fill[60:] + [x])]
        return [(1, [x] + fill[:20]), (1, fill[20:40] + [x]), (2, [x] + fill[40:60]), (last, fill[60:] + [x])]
    else:
        if shape == "low_bit":
            bits = [0] * 40
        elif shape == "high_bit":
            bits = [2 * k - 1] * 40
        else:  # both sides of every word border: the lowest bit of a word and the highest bit of the word below it
            bits = [b - d for b in range(64, 2 * k, 64) for d in (0, 1)] * 10
        per = {s: [] for s in range(S)}
        for i, (x, b) in enumerate(zip(_fresh(rng, k, len(bits)), bits)):
            a, c = x & ~(1 << b), x | (1 << b)
            per[i % S] += [a, c] if i % 4 else [a]
            if i % 4 == 0:
                per[last].append(c)
        rows = _rows(rng, per)
    if unordered and len({s for s, _ in rows}) > 1:
        first = next(i for i, (s, _) in enumerate(rows) if s != rows[0][0])
        rows = rows[first:] + rows[:first]
    return rows


def _calls(k, ids, rows):
    return [(ids[s], H.codes_of(keys, k) if keys else np.zeros((0, k), dtype=np.uint8)) for s, keys in rows]


# the cells of the shape table: name -> (k, ids, options, unordered, the road by hand).  One-word keys whose ids do not ascend, or with one id under
# "build_composite" 0, take the general road; keys of several words take it whatever the order.
CELLS = {
    "c27log": (27, IDS4, {}, False, [COMPOSITE, 9, 0, 0]),               # the log itself holds composites: 63 - 54 = 9 id bits
    "c20": (20, IDS4, CL0, False, [COMPOSITE, 9, 0, 0]),                 # composites formed from k-mers + ids: 300 takes 9 bits
    "p31": (31, (0, 3, 5, 255, 256, 300), {}, False, [PAIRS, 9, 2, 0]),  # 62 + 9 > 63: pairs, the ids in two bytes
    "g27u": (27, IDS4, {}, True, [GENERAL, 9, 4, 0]),
    "g45": (45, IDS4, {}, False, [GENERAL, 9, 4, 0]), "g45u": (45, IDS4, {}, True, [GENERAL, 9, 4, 0]),
    "g72": (72, IDS4, {}, False, [GENERAL, 9, 4, 0]), "g72u": (72, IDS4, {}, True, [GENERAL, 9, 4, 0]),
    "g126": (126, IDS4, {}, False, [GENERAL, 9, 4, 0]), "g126u": (126, IDS4, {}, True, [GENERAL, 9, 4, 0]),
}

# the roads and key shapes, each with the "mixed" shape: name -> (k, ids, options, unordered, the road by hand)
M18, M20, M23 = (1 << 18) - 1, (1 << 20) - 1, (1 << 23) - 1
ROADS = {
    # composites: 2k + gb <= 63
    "c9": (9, IDS4, CL0, False, [COMPOSITE, 9, 0, 0]),
    "c27_511": (27, (0, 3, 5, 511), CL0, False, [COMPOSITE, 9, 0, 0]),        # 54 + 9 = 63 | p27_512: 64
    "c28_127": (28, (0, 3, 5, 127), CL0, False, [COMPOSITE, 7, 0, 0]),        # 56 + 7 = 63 | p28_128: 64
    "c31_01": (31, (0, 1), CL0, False, [COMPOSITE, 1, 0, 0]),                 # 62 + 1 = 63 | p31_2: 64
    "c27log_511": (27, (0, 3, 5, 511), {}, False, [COMPOSITE, 9, 0, 0]),      # a log of composites with the id 2^gb - 1
    "c19log": (19, IDS4, {}, False, [COMPOSITE, 24, 0, 0]),                   # 63 - 38 = 25 bits of room: 24 are used
    "c20log": (20, (0, 3, 5, M23), {}, False, [COMPOSITE, 23, 0, 0]),         # 63 - 40 = 23, and the id 2^23 - 1
    # (k-mer, id) pairs: ordered one-word keys beyond 63 bits; ids below 65536 in 1 or 2 bytes, wider ones while a bucket's composite holds them
    "p31_2": (31, (0, 2), {}, False, [PAIRS, 2, 1, 0]),
    "p31_255": (31, (0, 3, 5, 255), {}, False, [PAIRS, 8, 1, 0]),             # one byte | two
    "p31_256": (31, (0, 3, 255, 256), {}, False, [PAIRS, 9, 2, 0]),
    "p31_65535": (31, (0, 255, 256, 65535), {}, False, [PAIRS, 16, 2, 0]),    # two bytes | four
    "p31_65536": (31, (0, 256, 65535, 65536), {}, False, [PAIRS, 17, 4, 0]),
    "p31_2e20m1": (31, (0, 65535, 65536, M20), {}, False, [PAIRS, 20, 4, 0]),  # 62 - 18 + 20 = 64 | g31_2e20: 65
    "p27_512": (27, (0, 3, 511, 512), CL0, False, [PAIRS, 10, 2, 0]),
    "p27_65536": (27, (0, 3, 65535, 65536), CL0, False, [PAIRS, 17, 4, 0]),
    "p28_128": (28, (0, 3, 127, 128), CL0, False, [PAIRS, 8, 1, 0]),
    "p29_2e18m1": (29, (0, 3, 65536, M18), {}, False, [PAIRS, 18, 4, 0]),
    "p32_2e18m1": (32, (0, 3, 65536, M18), {}, False, [PAIRS, 18, 4, 0]),      # 64 - 18 + 18 = 64 | g32_2e18: 65
    # whatever is left, one word
    "g27u_log": (27, IDS4, {}, True, [GENERAL, 9, 4, 0]),                      # a log of composites whose ids stop ascending: taken apart at build time
    "g27u": (27, IDS4, CL0, True, [GENERAL, 9, 4, 0]),
    "g31u": (31, IDS4, {}, True, [GENERAL, 9, 4, 0]),
    "g27_nocomp": (27, IDS4, {"build_composite": 0}, False, [GENERAL, 9, 4, 0]),
    "g31_2e20": (31, (0, 65536, M20, 1 << 20), {}, False, [GENERAL, 21, 4, 0]),
    "g32_2e18": (32, (0, 65536, M18, 1 << 18), {}, False, [GENERAL, 19, 4, 0]),
}
WIDE_KS = (33, 45, 64, 65, 72, 96, 97, 126)
for _k in WIDE_KS:  # keys of 2, 3 and 4 words: ordered ids, ids out of order, "build_msd" 0
    ROADS[f"g{_k}"] = (_k, IDS4, {}, False, [GENERAL, 9, 4, 0])
    ROADS[f"g{_k}u"] = (_k, IDS4, {}, True, [GENERAL, 9, 4, 0])
    ROADS[f"g{_k}_msd0"] = (_k, IDS4, {"build_msd": 0}, False, [GENERAL, 9, 4, 0])


def _seed(*parts):
    return sum((i + 1) * sum(str(p).encode()) for i, p in enumerate(parts))


def _cell_case(cell, shape):
    k, ids, options, unordered, road = CELLS[cell]
    rng = np.random.default_rng(_seed(cell, shape))
    rows = shape_rows(shape, k, len(ids), rng, unordered)
    options = dict(options)
    if unordered and shape in ONE_ID_SHAPES:
        options["build_composite"] = 0  # (one id cannot be out of order: the other way onto the general road for one-word keys)
    return Case(f"{cell}-{shape}", k, _calls(k, ids, rows), road, options, ids=ids)


def _road_case(name):
    k, ids, options, unordered, road = ROADS[name]
    rng = np.random.default_rng(_seed(name))
    return Case(f"road-{name}", k, _calls(k, ids, shape_rows("mixed", k, len(ids), rng, unordered)), road, options, ids=ids)


# -- the table of insert calls (keys of several words read a pair's id out of it)
def _empty_case(name):
    """empty calls in front, in the middle and at the end, under ids that would change the road if they counted"""
    k, ids, options, road, big_id = {"w2": (45, IDS4, {}, [GENERAL, 9, 4, 0], 70000), "w1": (27, IDS4, {}, [COMPOSITE, 9, 0, 0], 600),
                                     "p31": (31, (0, 3, 5, 255), {}, [PAIRS, 8, 1, 0], 70000)}[name]
    rng = np.random.default_rng(_seed("empty", name))
    calls = _calls(k, ids, shape_rows("edge_new_id", k, len(ids), rng))
    none = np.zeros((0, k), dtype=np.uint8)
    mid = len(calls) // 2
    return Case(f"empty-{name}", k, [(big_id, none)] + calls[:mid] + [(1, none)] + calls[mid:] + [(big_id, none)], road, options, ids=ids)


def _call_edges_case(k, unordered):
    """six calls, the first and the last row of each a k-mer that no other call holds, the rows between them shared with other calls"""
    rng = np.random.default_rng(_seed("edges", k, unordered))
    keys = _shuffled(rng, _fresh(rng, k, 52))
    own, shared = keys[:12], keys[12:]
    slots = [0, 1, 1, 2, 3, 3]
    rows = [(s, [own[2 * j]] + _shuffled(rng, shared)[:15 + j] + [own[2 * j + 1]]) for j, s in enumerate(slots)]
    if unordered:
        rows = rows[3:] + rows[:3]
    return Case(f"call_edges-k{k}" + ("u" if unordered else ""), k, _calls(k, IDS4, rows), [GENERAL, 9, 4, 0], ids=IDS4)


def _one_call_case(k):
    rng = np.random.default_rng(_seed("one_call", k))
    keys = _fresh(rng, k, 200)
    return Case(f"one_call-k{k}", k, _calls(k, (7,), [(0, _shuffled(rng, keys + keys[:30]))]), [GENERAL, 3, 4, 0], ids=(7,))


TABLE_KMERS = 4096


def _table_case(entries):
    """`entries` insert calls under the ids 0, 1, 2, .. at k = 45, one k-mer in the even calls and two in the odd ones, out of a table of 4096 k-mers:
    65 536 entries are the last table the sort reads its ids from, 65 537 the first it does not"""
    k = 45
    rng = np.random.default_rng(_seed("table"))
    base = H.codes_of(_shuffled(rng, _fresh(rng, k, TABLE_KMERS + 1)), k)
    dev = [(j, j % TABLE_KMERS, 1 + j % 2) for j in range(entries)]
    calls = [(g, base[a:a + n]) for g, a, n in dev]
    return Case(f"table-{entries}", k, calls, [GENERAL, H.bits_for(entries - 1), 4, 0], dev=(base, dev))


# -- the log's format
def _decompose_case(k):
    """a log of composites, then an id without room (the log is taken apart mid-way), then more than 65 536 further pairs (the log grows)"""
    small, big, gb, vw = {27: ((0, 3, 5, 511), 512, 10, 2), 28: ((0, 3, 5, 127), 128, 8, 1)}[k]
    rng = np.random.default_rng(_seed("decompose", k))
    calls = _calls(k, small, shape_rows("mixed", k, 4, rng))
    more = _fresh(rng, k, 33100)
    tail = [(big, H.codes_of(_shuffled(rng, more[:100] + [0, (1 << (2 * k)) - 1]), k)), (big, H.codes_of(_shuffled(rng, more + more[:33000]), k))]
    return Case(f"decompose_grow-k{k}", k, calls + tail, [PAIRS, gb, vw, 0], ids=small + (big,))


def _flush_case(name):
    """"flush_pairs" 1024: the second half of the calls is a run of its own, merged into the index the first half built"""
    k, ids, road, unordered = {"c27log": (27, IDS4, [COMPOSITE, 9, 0, 0], False), "p31": (31, (0, 3, 5, 255, 256, 300), [PAIRS, 9, 2, 0], False),
                               "g72u": (72, IDS4, [GENERAL, 9, 4, 0], True)}[name]
    rng = np.random.default_rng(_seed("flush", name))
    a = shape_rows("edge_dup", k, len(ids), rng, unordered)
    b = shape_rows("edge_new_id", k, len(ids), rng, unordered)
    again = [(len(ids) - 1, [x for _, keys in a for x in keys][::3])]  # pairs the index holds, and stored k-mers under one more id
    more = [(0, _fresh(rng, k, 600))]
    return Case(f"flush-{name}", k, _calls(k, ids, more + a + b + again), road, {"flush_pairs": 1024}, ids=ids)


def _two_step_case(name):
    """two builds on one handle: the second log brings new k-mers, stored k-mers under new ids and pairs the index holds"""
    k, ids1, opt, road1, ids2, road2, un = {
        "c27log": (27, IDS4, {}, [COMPOSITE, 9, 0, 0], (0, 3, 5), [COMPOSITE, 9, 0, 0], False),
        # the first log meets an id without room and goes as pairs; the second is a log of composites again, though the handle has seen 600
        "p27_then_c": (27, (0, 3, 5, 600), {}, [PAIRS, 10, 2, 0], (0, 3, 5), [COMPOSITE, 9, 0, 0], False),
        # without the composite log the second run's gb follows the largest id the handle has seen: 54 + 10 > 63
        "p27_cl0": (27, (0, 3, 5, 600), CL0, [PAIRS, 10, 2, 0], (0, 3, 5), [PAIRS, 10, 2, 0], False),
        "p31": (31, (0, 3, 5, 255, 256, 300), {}, [PAIRS, 9, 2, 0], (0, 3, 5), [PAIRS, 9, 2, 0], False),
        "g27u": (27, IDS4, {}, [GENERAL, 9, 4, 0], (0, 3, 5), [GENERAL, 9, 4, 0], True),
        "g45u": (45, IDS4, {}, [GENERAL, 9, 4, 0], (0, 3, 5), [GENERAL, 9, 4, 0], True),
        "g126u": (126, IDS4, {}, [GENERAL, 9, 4, 0], (0, 3, 5), [GENERAL, 9, 4, 0], True),
        "g72": (72, IDS4, {}, [GENERAL, 9, 4, 0], (0, 3, 5), [GENERAL, 9, 4, 0], False),
    }[name]
    rng = np.random.default_rng(_seed("two_step", name))
    a = shape_rows("edge_new_kmer", k, len(ids1), rng, un)
    b = shape_rows("edge_dup", k, len(ids2), rng, un)
    again = [(len(ids2) - 1, [x for _, keys in a for x in keys][::3])]
    return Case(f"two_step-{name}", k, _calls(k, ids2, b + again), road2, opt, first=_calls(k, ids1, a), first_road=road1, ids=ids1)


# -- the four large ones
def _large_codes(k, m, seed):
    """m distinct random k-mers"""
    rng = np.random.default_rng(seed)
    codes = np.unique(rng.integers(0, 4, (m + m // 8, k), dtype=np.uint8), axis=0)
    assert len(codes) >= m
    return np.ascontiguousarray(codes[rng.permutation(len(codes))[:m]])


def _threshold_case(total):
    """k = 27 under "build_msd" 1 with 2^20 - 1 | 2^20 pairs: 2^18 k-mers under the ids 0 and 1, each pair twice -- all but one of them below the border"""
    A = _large_codes(27, 1 << 18, 27)
    x = total - 3 * (1 << 18)
    calls = [(0, A), (0, A[:x]), (1, A), (1, A[::-1])]
    return Case(f"threshold-{total}", 27, calls, [COMPOSITE, 9, 0, int(total >= SPLIT_FROM)], big=True, ids=(0, 1))


def _grid_case(name):
    """(threads of a capped grid + 300) pairs: every kernel of the road takes a second pass over the last 300"""
    m = GRID_THREADS // 4
    if name == "composite":
        A = _large_codes(27, m, 5)
        return Case("grid-composite", 27, [(0, A), (1, A), (1, A[::-1]), (3, A), (3, A[:GRID_LOOSE])], [COMPOSITE, 9, 0, 0], big=True, ids=(0, 1, 3))
    A = _large_codes(72, m, 6)
    return Case("grid-w3u", 72, [(1, A), (0, A), (1, A[::-1]), (0, A), (2, A[:GRID_LOOSE])], [GENERAL, 2, 4, 0], big=True, ids=(0, 1, 2))


SMALL = {}
for _cell in CELLS:
    for _shape in SHAPES:
        if _shape == "word_bits" and CELLS[_cell][0] <= 32:
            continue  # (one word: no border)
        if CELLS[_cell][3] and CELLS[_cell][0] > 32 and _shape in ONE_ID_SHAPES + ("total_2", "one_kmer"):
            continue  # (no order to break that would change anything: the ordered cell of the same k has the case)
        SMALL[f"{_cell}-{_shape}"] = functools.partial(_cell_case, _cell, _shape)
for _name in ROADS:
    SMALL[f"road-{_name}"] = functools.partial(_road_case, _name)
for _name in ("w2", "w1", "p31"):
    SMALL[f"empty-{_name}"] = functools.partial(_empty_case, _name)
for _k, _un in ((45, False), (45, True), (72, True), (126, False)):
    SMALL[f"call_edges-k{_k}" + ("u" if _un else "")] = functools.partial(_call_edges_case, _k, _un)
for _k in (45, 72):
    SMALL[f"one_call-k{_k}"] = functools.partial(_one_call_case, _k)
for _name in ("c27log", "p31", "g72u"):
    SMALL[f"flush-{_name}"] = functools.partial(_flush_case, _name)
SMALL["log_unordered-k27"] = lambda: Case("log_unordered-k27", 27, _calls(27, IDS4, shape_rows("dup_far", 27, 3, np.random.default_rng(11), True)[:3]), [GENERAL, 3, 4, 0],
                                          ids=(3, 5))  # (ids 5, 3, 5 in a log of composites: taken apart at build time, gb from the largest id seen)
TWO_STEP = {f"two_step-{n}": functools.partial(_two_step_case, n) for n in ("c27log", "p27_then_c", "p27_cl0", "p31", "g27u", "g45u", "g72", "g126u")}
MEDIUM = {"table-65536": functools.partial(_table_case, CALL_TABLE_MAX), "table-65537": functools.partial(_table_case, CALL_TABLE_MAX + 1),
          "decompose_grow-k27": functools.partial(_decompose_case, 27), "decompose_grow-k28": functools.partial(_decompose_case, 28)}
LARGE = {"grid-composite": functools.partial(_grid_case, "composite"), "grid-w3u": functools.partial(_grid_case, "w3u"),
         f"threshold-{SPLIT_FROM - 1}": functools.partial(_threshold_case, SPLIT_FROM - 1), f"threshold-{SPLIT_FROM}": functools.partial(_threshold_case, SPLIT_FROM)}
BUILDERS = {**SMALL, **TWO_STEP, **MEDIUM, **LARGE}
QUICK = list(SMALL) + list(TWO_STEP)  # a few thousand pairs at the most


@functools.lru_cache(maxsize=None)
def _small_case(name):
    return BUILDERS[name]()


@functools.lru_cache(maxsize=2)
def _big_case(name):
    return BUILDERS[name]()


def case(name):
    c = (_small_case if name in SMALL or name in TWO_STEP else _big_case)(name)
    assert c.name == name
    return c


# ---- what a case is: facts read off its calls ---------------------------------------------------------------------------------------------------------
def _edge_kind(a, b):
    """the sorted pair a beside its neighbour b"""
    return "new_kmer" if b is None or a[0] != b[0] else "dup" if a == b else "new_id"


def facts(c):
    """the conditions a case meets, from its calls alone (the last build's log; a large case: only what needs no list of its pairs)"""
    f = set()
    log, max_gid = c.last_log()
    total = sum(len(x) for _, x in log)
    g = [x for x, _ in log]
    f.add("ids_ordered" if g == sorted(g) else "ids_unordered")
    if total in (1, 2, 255, 256, 257):
        f.add(f"total:{total}")
    entries = 1 + sum(1 for a, b in zip(g, g[1:]) if a != b)  # consecutive calls of one id share an entry of the table
    f.add("calls:one" if len(log) == 1 else "calls:several")
    if any(a == b for a, b in zip(g, g[1:])):
        f.add("calls:two_of_one_id")
    if entries in (CALL_TABLE_MAX, CALL_TABLE_MAX + 1):
        f.add(f"table:{entries}")
    where = [i for i, (_, x) in enumerate(c.calls) if len(x) == 0]
    f |= {"empty:first"} if 0 in where else set()
    f |= {"empty:last"} if len(c.calls) - 1 in where else set()
    f |= {"empty:middle"} if any(0 < i < len(c.calls) - 1 for i in where) else set()
    if where:
        other = [x for i, (x, _) in enumerate(c.calls) if i in where]
        f |= {"empty:larger_id"} if max(other) > max_gid else set()
        for i in where:
            prior = [x for x, y in c.calls[:i] if len(y)]
            f |= {"empty:lower_id_behind"} if prior and c.calls[i][0] < max(prior) else set()
    if total > GRID_THREADS:
        f.add("grid:second_pass")
    if c.options["build_msd"] == 1 and total in (SPLIT_FROM - 1, SPLIT_FROM):
        f.add(f"msd:{total}")
    if "flush_pairs" in c.options and len(log) < sum(1 for _, x in c.calls if len(x)):
        f.add("log:flushed")
    if c.first is not None:
        f.add("two_step")
        f |= {"two_step:smaller_ids"} if max(g) < max_gid else set()
    tb = 2 * c.k - 64 * (c.W - 1)
    f.add(f"top_bits:{tb}")
    if c.big:
        return f
    flat, ends = keys_of(np.concatenate([x for _, x in log]), c.k), np.cumsum([len(x) for _, x in log]).tolist()
    keys = [flat[a:b] for a, b in zip([0] + ends[:-1], ends)]
    pairs = [(x, gid) for (gid, _), ks in zip(log, keys) for x in ks]
    s = sorted(pairs)
    f.add("end:" + _edge_kind(s[-1], s[-2] if total > 1 else None))
    f.add("first:" + _edge_kind(s[0], s[1] if total > 1 else None))
    distinct, have, ids = set(pairs), {x for x, _ in pairs}, {x for _, x in pairs}
    if len(distinct) == 1 and total >= 100:
        f.add("same_pair")
    if len(have) == 1 and ids == set(c.ids) and len(ids) >= 3:
        f.add("one_kmer_every_id")
    if len(distinct) == total >= 100 and len(ids) == 1:
        f.add("distinct_one_id")
    if len(distinct) < total:
        f.add("duplicates")
    if len(have) < len(distinct):
        f.add("shared_kmers")
    # one pair in two calls with other pairs between its copies
    pos, call_of, n = collections.defaultdict(list), [], 0
    for j, ks in enumerate(keys):
        for x in ks:
            pos[(x, g[j])].append((n, j))
            n += 1
    if any(b[1] != a[1] and b[0] - a[0] > 1 for p in pos.values() for a, b in zip(p, p[1:])):
        f.add("dup_far")
    seqs = collections.defaultdict(list)  # ids 5, 3, 5 on one k-mer, in that order of calls
    for j, ks in enumerate(keys):
        for x in set(ks):
            seqs[x].append(g[j])
    if any(seq[i:i + 3] == [5, 3, 5] for seq in seqs.values() for i in range(len(seq) - 2)):
        f.add("ids_5_3_5")
    # the first and the last row of every entry of the table: a k-mer no other entry holds
    if entries >= 3:
        ent, cur = [], None
        for gid, ks in zip(g, keys):
            if gid == cur:
                ent[-1] = ent[-1] + ks
            else:
                ent.append(list(ks))
            cur = gid
        cnt = collections.Counter(x for e in ent for x in set(e))
        if all(cnt[e[0]] == 1 and cnt[e[-1]] == 1 for e in ent):
            f.add("calls:own_first_and_last_row")
    bit = lambda b: any((x ^ (1 << b)) in have for x in have)
    f |= {"low_bit"} if bit(0) else set()
    f |= {"high_bit"} if bit(2 * c.k - 1) else set()
    if c.W > 1 and all(bit(b) and bit(b - 1) for b in range(64, 2 * c.k, 64)):
        f.add("word_bits")
    # an id width whose smallest and largest id share a k-mer's list
    lists = collections.defaultdict(set)
    for x, gid in distinct:
        lists[x].add(gid)
    for w, lo, hi in ((1, 0, 255), (2, 256, 65535), (4, 65536, max_gid)):
        if hi >= lo and any(lo in v and hi in v for v in lists.values()) and (w < 4 or hi > lo):
            f.add(f"list_spans_width:{w}")
    return f


# the table of conditions: every (family, condition) below is met by at least one case
FAMILIES = ("composite", "pairs", "general_w1", "general_w2", "general_w3", "general_w4")
EVERYWHERE = ("end:new_kmer", "end:new_id", "end:dup", "first:new_kmer", "first:new_id", "first:dup", "total:1", "total:2", "total:255", "total:256", "total:257", "same_pair",
              "one_kmer_every_id", "distinct_one_id", "dup_far", "low_bit", "high_bit", "duplicates", "shared_kmers", "calls:one", "calls:two_of_one_id", "two_step")
LINES = [(fam, cond) for fam in FAMILIES for cond in EVERYWHERE]
LINES += [(f"general_w{w}", cond) for w in (1, 2, 3, 4) for cond in ("ids_5_3_5", "ids_ordered", "ids_unordered")]
LINES += [(f"general_w{w}", cond) for w in (2, 3, 4) for cond in ("word_bits", "calls:own_first_and_last_row", "build_msd:0", "top_bits:2")]
LINES += [("general_w2", "top_bits:64"), ("general_w3", "top_bits:64"), ("general_w2", "table:65536"), ("general_w2", "table:65537"), ("general_w3", "grid:second_pass"),
          ("composite", "grid:second_pass"), ("composite", f"msd:{SPLIT_FROM - 1}"), ("composite", f"msd:{SPLIT_FROM}"), ("composite", "split_tried"),
          ("composite", "composite_log"), ("composite", "composite_log:id_fills_gb"), ("composite", "no_composite_log"), ("composite", "2k+gb:63"),
          ("pairs", "2k+gb:64"), ("pairs", "bucket+gb:64"), ("general_w1", "bucket+gb:65"), ("pairs", "id_bytes:1"), ("pairs", "id_bytes:2"), ("pairs", "id_bytes:4"),
          ("pairs", "list_spans_width:1"), ("pairs", "list_spans_width:2"), ("pairs", "list_spans_width:4"), ("pairs", "max_id:255"), ("pairs", "max_id:256"),
          ("pairs", "max_id:65535"), ("pairs", "max_id:65536"), ("pairs", "log:taken_apart_then_grown"), ("general_w1", "log:taken_apart_at_build"),
          ("general_w1", "build_composite:0"), ("composite", "log:flushed"), ("pairs", "log:flushed"), ("general_w3", "log:flushed"),
          ("composite", "two_step:smaller_ids"), ("pairs", "two_step:smaller_ids"),
          ("composite", "empty:first"), ("composite", "empty:middle"), ("composite", "empty:last"), ("composite", "empty:larger_id"), ("composite", "empty:lower_id_behind"),
          ("pairs", "empty:larger_id"), ("general_w2", "empty:first"), ("general_w2", "empty:middle"), ("general_w2", "empty:last"), ("general_w2", "empty:larger_id")]


@functools.lru_cache(maxsize=None)
def conditions_of(name):
    return frozenset(conditions(case(name)))


def conditions(c):
    """facts(c) and what the case's options and its hand-written road add"""
    f = facts(c)
    log, max_gid = c.last_log()
    road, gb, vw, split = c.road
    o = c.options
    f |= {f"build_msd:{o['build_msd']}", f"build_composite:{o['build_composite']}"}
    f |= {"split_tried"} if split else set()
    ordered1 = c.W == 1 and "ids_ordered" in f and o["build_composite"]
    comp_log = c.W == 1 and o["composite_log"] and o["build_composite"] and 63 - 2 * c.k >= 7  # (the log holds composites where 7 id bits and more fit)
    if road == COMPOSITE:
        f.add(f"2k+gb:{2 * c.k + gb}")
        f.add("composite_log" if comp_log else "no_composite_log")
        if comp_log and max(x for x, _ in log) == (1 << gb) - 1:
            f.add("composite_log:id_fills_gb")
    if road == PAIRS:
        f |= {f"2k+gb:{2 * c.k + gb}", f"bucket+gb:{2 * c.k - 18 + gb}", f"id_bytes:{vw}", f"max_id:{max_gid}"}
        if comp_log and sum(len(x) for g, x in log if g == max_gid) > 65536:
            f.add("log:taken_apart_then_grown")
    if road == GENERAL and ordered1:
        f.add(f"bucket+gb:{2 * c.k - 18 + gb}")
    if road == GENERAL and comp_log and "ids_unordered" in f:
        f.add("log:taken_apart_at_build")
    return f


# ---- tests: the key is the library's --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hostlib():
    subprocess.check_call(["make", "-C", _lib.CSRC, "all"], stdout=subprocess.DEVNULL)
    lib = C.CDLL(os.path.join(_lib.CSRC, "libbft_hosttest.so"))
    lib.bft_hosttest_roundtrip.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p]
    return lib


KS_USED = sorted({v[0] for v in CELLS.values()} | {v[0] for v in ROADS.values()})


def test_every_k_is_pinned():
    assert KS_USED == sorted({case(n).k for n in QUICK}) and {case(n).k for n in list(MEDIUM) + list(LARGE)} <= set(KS_USED)


@pytest.mark.parametrize("k", KS_USED)
def test_t_form_key_is_the_librarys(hostlib, k):
    rng = np.random.default_rng(k)
    edge = [0, (1 << (2 * k)) - 1, 1, 1 << (2 * k - 1)] + [1 << b for b in range(63, 2 * k, 64)] + [1 << b for b in range(64, 2 * k, 64)]
    codes = np.concatenate([H.codes_of(edge + _fresh(rng, k, 40), k), rng.integers(0, 4, (40, k), dtype=np.uint8)])
    keys = keys_of(codes, k)
    assert keys[:len(edge)] == edge  # codes_of and keys_of are each other's inverse
    packed = G.pack(codes)
    W = words_of(k)
    out, tf = np.zeros_like(packed), np.zeros(len(packed) * W, dtype=np.uint64)
    hostlib.bft_hosttest_roundtrip(packed.ctypes.data, len(packed), k, out.ctypes.data, tf.ctypes.data)
    assert (out == packed).all()
    got = [sum(int(w) << (64 * (W - 1 - j)) for j, w in enumerate(tf[i * W:(i + 1) * W])) for i in range(len(packed))]
    assert got == keys == G.P.t_key_ints(codes, k)
    if k <= 64:
        assert keys == H.keys_of(codes, k)
    kw = key_words(codes, k)
    assert len(kw) == W and [sum(int(w[i]) << (64 * (W - 1 - j)) for j, w in enumerate(kw)) for i in range(len(codes))] == keys


@pytest.mark.parametrize("name", ("c27log-mixed", "g72u-edge_dup", "g126-word_bits", "g45u-dup_far", "p31-total_1"))
def test_numpy_truth_is_the_dict_truth(name):
    c = case(name)
    codes, gids = c._flat(c.calls)
    a, b = Truth(c.k, codes, gids.tolist()), NpTruth(c.k, codes, gids)
    assert (a.kmers, a.pairs, a.order, a.sets) == (b.kmers, b.pairs, b.order, b.sets) and (a.packed == b.packed).all() and (a.codes == b.codes).all()
    assert len(b.absent(16, 0)) == 16


# ---- tests: the hook ------------------------------------------------------------------------------------------------------------------------------------
def test_hook_symbol_errors_and_header():
    hdr = open(_lib.HEADER).read()
    assert re.search(r"\bint\s+bft_gpu_debug_run_plan\s*\(\s*int\s+k\s*,\s*int\s+ids_ordered\s*,\s*int\s+build_composite\s*,\s*int\s+build_msd\s*,\s*int\s+composite_log\s*,"
                     r"\s*uint32_t\s+max_gid\s*,\s*uint32_t\s+log_max_gid\s*,\s*uint64_t\s+total\s*,\s*uint32_t\s+out\s*\[\s*8\s*\]\s*\)\s*;", hdr)
    assert "bft_gpu_debug_run_plan" in _lib.SIGNATURES and len(_lib.SIGNATURES["bft_gpu_debug_run_plan"][1]) == 9
    lib = _lib.load()
    out = (C.c_uint32 * 8)()
    assert lib.bft_gpu_debug_run_plan(27, 1, 1, 1, 1, 5, 5, 10, None) == -1  # BFT_GPU_E_ARG
    for k, msd, mx, lmx, total in ((8, 1, 5, 5, 10), (127, 1, 5, 5, 10), (27, 3, 5, 5, 10), (27, -1, 5, 5, 10), (27, 1, 5, 6, 10), (27, 1, 5, 5, 0)):
        assert lib.bft_gpu_debug_run_plan(k, 1, 1, msd, 1, mx, lmx, total, out) == -1, (k, msd, mx, lmx, total)
    assert plan(27, 1, 1, 1, 1, 300, 300, 1000) == [COMPOSITE, 9, 0, 0, 9, 1, GRID_THREADS, CALL_TABLE_MAX]
    assert GRID_THREADS == G.GRID_CAP


def test_each_condition_is_defined_once():
    """bft_make_run and the log take their decisions from csrc/bft_run_plan.h only: no other source of the library restates a limit of the roads"""
    src = {f: open(os.path.join(_lib.CSRC, f)).read() for f in os.listdir(_lib.CSRC) if f.endswith((".hip", ".h", ".cpp"))}
    for name in ("bft_run_split_top", "bft_run_ordered_w1", "bft_run_composite_fits", "bft_run_split_wanted", "bft_run_bucket_holds_id", "bft_run_pairs_fit",
                 "bft_run_pairs_split_ok", "bft_run_ordered_w2", "bft_run_id_width", "bft_run_log_comp_bits", "bft_run_road"):
        defs = [f for f, text in src.items() if re.search(r"\b(?:bool|unsigned|uint32_t|int|BftRunRoad)\s+" + name + r"\s*\(", text)]
        assert defs == ["bft_run_plan.h"], (name, defs)
    run, gpu = src["bft_run.hip"], src["bft_gpu.hip"]
    assert "bft_run_road(" in run and "bft_run_log_comp_bits(" in gpu and "bft_run_log_holds_id(" in gpu and "bft_run_log_stays_composite(" in gpu
    for text in (run, gpu):  # none of the limits is written out beside the header
        assert not re.search(r"<=\s*63\b|max_gid_seen\s*<\s*(?:256|65536)|1u?\s*<<\s*20\b|63\s*-\s*2\s*\*", text)
    assert "BFT_RUN_CALL_TABLE_MAX" in run and not re.search(r"lb_end\.size\(\)\s*<=\s*\(", run)


def test_the_rules_at_their_borders():
    """the rules as DESIGN.md section 4 and csrc/bft_run_plan.h state them, asked of the library at both sides of every border"""
    road = lambda *a: plan(*a)[:4]
    # 2k + gb = 63 | 64 (ordered one-word keys, k-mers + ids logged)
    assert [road(31, 1, 1, 1, 0, m, m, 100) for m in (1, 2)] == [[COMPOSITE, 1, 0, 0], [PAIRS, 2, 1, 0]]
    assert [road(27, 1, 1, 1, 0, m, m, 100) for m in (511, 512)] == [[COMPOSITE, 9, 0, 0], [PAIRS, 10, 2, 0]]
    assert [road(28, 1, 1, 1, 0, m, m, 100) for m in (127, 128)] == [[COMPOSITE, 7, 0, 0], [PAIRS, 8, 1, 0]]
    # the bytes of an id beside the keys
    assert [road(31, 1, 1, 1, 1, m, m, 100)[1:3] for m in (255, 256, 65535, 65536)] == [[8, 1], [9, 2], [16, 2], [17, 4]]
    # ids of 65536 and more stay pairs while a root-prefix bucket's composite holds them: 2k - 18 + gb = 64 | 65
    assert [road(31, 1, 1, 1, 1, m, m, 100) for m in (M20, M20 + 1)] == [[PAIRS, 20, 4, 0], [GENERAL, 21, 4, 0]]
    assert [road(32, 1, 1, 1, 1, m, m, 100) for m in (M18, M18 + 1)] == [[PAIRS, 18, 4, 0], [GENERAL, 19, 4, 0]]
    assert road(32, 1, 1, 1, 1, 65535, 65535, 100) == [PAIRS, 16, 2, 0] and road(32, 1, 1, 2, 1, 65535, 65535, 100) == [PAIRS, 16, 2, 0]  # (k = 32: never behind the split)
    # "build_msd" 1: the split from 2^20 pairs on; 0 never; 2 always -- for composites, pairs and ordered two-word keys only
    assert [road(27, 1, 1, 1, 1, 5, 5, t)[3] for t in (SPLIT_FROM - 1, SPLIT_FROM)] == [0, 1]
    assert [road(27, 1, 1, m, 1, 5, 5, t)[3] for m, t in ((0, SPLIT_FROM), (2, 1))] == [0, 1]
    assert [road(k, o, c, 2, 1, 5, 5, 100) for k, o, c in ((45, 1, 1), (45, 0, 1), (45, 1, 0), (72, 1, 1), (27, 0, 1), (27, 1, 0), (31, 1, 1))] == [
        [GENERAL, 3, 4, 1], [GENERAL, 3, 4, 0], [GENERAL, 3, 4, 0], [GENERAL, 3, 4, 0], [GENERAL, 3, 4, 0], [GENERAL, 3, 4, 0], [PAIRS, 3, 1, 1]]
    # the log holds composites where 7 id bits and more fit beside a one-word key, 24 at the most; they stay while the ids fit and ascend
    assert [plan(k, 1, 1, 1, 1, 5, 5, 100)[4:6] for k in (9, 19, 20, 27, 28, 29, 31, 33)] == [[24, 1], [24, 1], [23, 1], [9, 1], [7, 1], [0, 0], [0, 0], [0, 0]]
    assert plan(27, 1, 1, 1, 0, 5, 5, 100)[4:6] == [0, 0] and plan(27, 1, 0, 1, 1, 5, 5, 100)[4:6] == [0, 0] and plan(27, 0, 1, 1, 1, 5, 5, 100)[4:6] == [9, 0]
    assert [plan(27, 1, 1, 1, 1, m, m, 100)[:6] for m in (511, 512)] == [[COMPOSITE, 9, 0, 0, 9, 1], [PAIRS, 10, 2, 0, 9, 0]]
    # behind an earlier build: a log of composites keeps its own id bits, a log of k-mers + ids takes those of the largest id the handle has seen
    assert plan(27, 1, 1, 1, 1, 600, 5, 100)[:6] == [COMPOSITE, 9, 0, 0, 9, 1] and plan(27, 1, 1, 1, 0, 600, 5, 100)[:6] == [PAIRS, 10, 2, 0, 0, 0]


# ---- tests: every case is what it is named after --------------------------------------------------------------------------------------------------------
def _check_case(c):
    assert c.plan()[:4] == c.road, (c.name, c.plan(), c.road)
    if c.first is not None:
        assert c.plan_first()[:4] == c.first_road, (c.name, c.plan_first(), c.first_road)
    log, max_gid = c.last_log()
    p = c.plan()
    assert p[6] == GRID_THREADS and p[7] == CALL_TABLE_MAX
    assert max_gid == max(c.ids)  # the id that decides gb and the id width is inserted
    return conditions_of(c.name)


@pytest.mark.parametrize("name", list(BUILDERS))
def test_the_plan_agrees_with_every_road(name):
    c = case(name)
    cond = _check_case(c)
    tr = c.truth
    assert tr.kmers <= tr.pairs <= sum(len(x) for _, x in (c.first or []) + c.calls)
    if name in QUICK:
        assert tr.pairs <= 4000
    if max(c.ids) >= 1 << 18:
        assert tr.kmers <= 400  # (ids this large: a few hundred k-mers)
    shape = name.split("-", 1)[1]
    want = {"edge_new_kmer": {"first:new_kmer", "end:new_kmer"}, "edge_new_id": {"first:new_id", "end:new_id"}, "edge_dup": {"first:dup", "end:dup"},
            "same_pair": {"same_pair", "end:dup", "first:dup"}, "one_kmer": {"one_kmer_every_id"}, "distinct_one_id": {"distinct_one_id", "calls:one"}, "dup_far": {"dup_far"},
            "low_bit": {"low_bit"}, "high_bit": {"high_bit"}, "word_bits": {"word_bits"}, "mixed": {"duplicates", "shared_kmers", "calls:two_of_one_id"}}
    if name.split("-", 1)[0] in CELLS:
        assert want.get(shape, {f"total:{shape[6:]}"} if shape.startswith("total_") else set()) <= cond, (name, cond)
        if CELLS[name.split("-", 1)[0]][3] and shape == "dup_far":
            assert "ids_5_3_5" in cond
    if name.startswith("call_edges"):
        assert "calls:own_first_and_last_row" in cond
    if name.startswith("empty-"):
        assert {"empty:first", "empty:middle", "empty:last", "empty:larger_id", "empty:lower_id_behind"} <= cond
        plain = Case("plain", c.k, [(g, x) for g, x in c.calls if len(x)], c.road, c.options)
        assert plain.plan() == c.plan() and plain.truth.sets == tr.sets  # as if the empty calls had not been made
    if name.startswith("table-"):
        assert f"table:{name[6:]}" in cond and tr.kmers == TABLE_KMERS + 1 and len(c.dev[1]) == int(name[6:])
    if name.startswith("decompose_grow"):
        assert "log:taken_apart_then_grown" in cond and plan(c.k, 1, 1, 1, 1, max(c.ids) - 1, max(c.ids) - 1, 100)[5] == 1 and c.plan()[5] == 0
    if name.startswith("flush-"):
        assert "log:flushed" in cond and len(c.last_log()[0]) >= 2
    if name.startswith("grid-"):
        assert "grid:second_pass" in cond and sum(len(x) for _, x in c.calls) == GRID_THREADS + GRID_LOOSE
    if name.startswith("threshold-"):
        assert f"msd:{name[10:]}" in cond and tr.kmers == 1 << 18 and tr.pairs == 1 << 19 and set(tr.sets.values()) == {(0, 1)}
    if name.startswith("two_step-"):
        a, b = c.truth_first, c._truth(c.calls)
        assert set(a.order) & set(b.order) and set(b.order) - set(a.order) and a.pairs < tr.pairs < a.pairs + b.pairs and tr.kmers > a.kmers


def test_threshold_cases_share_their_truth():
    a, b = case(f"threshold-{SPLIT_FROM - 1}").truth, case(f"threshold-{SPLIT_FROM}").truth
    assert a.order == b.order and a.sets == b.sets and (a.packed == b.packed).all()


@functools.lru_cache(maxsize=None)
def _family_of(name):
    return case(name).family


def test_condition_table():
    """every line of the table is met by at least one case (the counts: CHANGES.md)"""
    table = collections.Counter()
    for name in BUILDERS:
        for cond in conditions_of(name):
            table[(_family_of(name), cond)] += 1
    missing = [line for line in LINES if table[line] < 1]
    assert not missing, missing
    assert len(set(LINES)) == len(LINES)
    if os.environ.get("BFT_RUN_TABLE"):  # (the counts, for CHANGES.md)
        for line in LINES:
            print(line, table[line])


# ---- tests: the checker -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("c27log-mixed", "p31-edge_new_id", "g72u-mixed", "g126-edge_dup"))
def test_the_checker_rejects_wrong_runs(name):
    """compare() finds nothing in what a correct index returns, and reports each of: a duplicate pair kept, a pair lost at the end, two ids of a list
    swapped, two neighbouring k-mers swapped, a k-mer under its neighbour's list"""
    tr = case(name).truth
    kmers, cs, sets, nk, npairs = ideal(tr)
    assert compare(tr, kmers, cs, sets, nk, npairs) == []
    fresh = max(sets) + 1
    multi = next(i for i in range(tr.kmers) if len(sets[int(cs[i])]) >= 2)
    # a duplicate pair kept
    s2, c2 = dict(sets), cs.copy()
    s2[fresh] = sets[int(cs[multi])][:1] + sets[int(cs[multi])]
    c2[multi] = fresh
    bad = compare(tr, kmers, c2, s2, nk, npairs + 1)
    assert any("not strictly ascending" in b for b in bad) and any(b.startswith("pairs:") for b in bad) and any(b.startswith("info:") for b in bad)
    # a pair lost at the end: the last id of the last k-mer, or the last k-mer with its only id
    last = sets[int(cs[-1])]
    if len(last) > 1:
        s2, c2 = dict(sets), cs.copy()
        s2[fresh] = last[:-1]
        c2[-1] = fresh
        bad = compare(tr, kmers, c2, s2, nk, npairs - 1)
        assert any(b.startswith("colour sets:") and f"row {tr.kmers - 1}" in b for b in bad) and any(b.startswith("pairs:") for b in bad)
    else:
        bad = compare(tr, kmers[:-1], cs[:-1], sets, nk - 1, npairs - 1)
        assert any(b.startswith("k-mers:") for b in bad) and any(b.startswith("pairs:") for b in bad) and any(b.startswith("info:") for b in bad)
    bad = compare(tr, kmers, cs, sets, nk, npairs - 1)  # (the count alone)
    assert len(bad) == 1 and bad[0].startswith("info:")
    # two ids of a list swapped
    s2, c2 = dict(sets), cs.copy()
    s2[fresh] = [sets[int(cs[multi])][1], sets[int(cs[multi])][0]] + sets[int(cs[multi])][2:]
    c2[multi] = fresh
    bad = compare(tr, kmers, c2, s2, nk, npairs)
    assert any("not strictly ascending" in b for b in bad) and any(b.startswith("colour sets:") and f"row {multi}" in b for b in bad)
    # two neighbouring k-mers swapped, their lists with them
    i = tr.kmers // 2
    k2, c2 = kmers.copy(), cs.copy()
    k2[[i, i + 1]], c2[[i, i + 1]] = kmers[[i + 1, i]], cs[[i + 1, i]]
    bad = compare(tr, k2, c2, sets, nk, npairs)
    assert any(b.startswith("k-mers:") and f"row {i}" in b for b in bad)
    # a k-mer under its neighbour's list
    j = next(i for i in range(tr.kmers - 1) if cs[i] != cs[i + 1])
    c2 = cs.copy()
    c2[j] = cs[j + 1]
    bad = compare(tr, kmers, c2, sets, nk, npairs)
    assert any(b.startswith("colour sets:") and f"row {j}" in b for b in bad)
