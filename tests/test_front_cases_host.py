"""The cases of the front-end edge tests (tests/test_gpu_front_edges.py runs them on the GPU), their ground truth, and -- here, without a GPU -- the
proof that each case reaches the regime it is named after.

The front end (csrc/bft_front.hip) takes over behind the root-prefix split: the (k-mer, genome) pairs of a build grouped by the top 18 bits of their
T-form, in insertion order inside a bucket, become the sorted distinct k-mers with their genome ids.  Which kernel sorts a bucket follows from its
size, from the largest and the mean bucket and from the largest genome id (csrc/bft_front_plan.h); a case here is a list of buckets (root prefix,
exact number of pairs, content shape) under one key width and one labelling of the genomes, and the selection rules are read from the library
(bft_gpu_debug_front_plan: no device needed), never restated.

Truth, in Python only (nothing of the library's): the T-form key of a k-mer is that of test_prefix_cases_host / test_graph_cases_host (t_order,
keys_u64; pinned here to bft_hosttest_roundtrip for every k used); from the inserted (k-mer, id) list, duplicates included, a dict k-mer -> sorted
distinct ids, the k-mers in key order, the numbers of distinct k-mers and pairs, and the size of every bucket as inserted (what the split counts).

Inside a bucket the kernels lay the sorted pairs out by position: position i of a bucket sorted by one wavefront is (round i // 64, lane i % 64); of
one sorted by a workgroup of four wavefronts with E = ceil(n / 256) rounds, (wave i // 64E, round (i % 64E) // 64, lane i % 64); the emit kernels walk
a bucket 256 positions at a time.  test_run_shapes_cross_the_borders computes from that where the runs of equal k-mers begin and end.

Sizes: a case holds its largest bucket (64 .. 8193 pairs), one bucket on every class border beneath it and three small ones: 1.5e2 .. 2e4 pairs."""
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
import test_graph_cases_host as G  # noqa: E402  (keys_u64, shape_of, pack; G.P.t_order)

from bloomfiltertrie_amd import _lib  # noqa: E402  (the selection rules and the host test library of the pin, nothing else)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPLIT_TOP = 18
DBITS = 9  # the radix passes' digit
SHAPES = ("distinct", "one_pair", "one_kmer", "shared", "low_bit", "high_bit", "top_digit")
RUN_CYCLE = (64, 63, 65, 2)  # pairs per k-mer of the "shared" shape, in key order

_MANY = tuple(range(65))  # 65 genomes and one more: a k-mer can be held by 2, 63, 64 and 65 of them
# name -> (k, genome ids, "composite_log"); one word: gb = the bits of the largest id ("composite_log" 0: the composites are formed from k-mers + ids)
ROADS1 = {
    "k9_gb1": (9, (0, 1), 0), "k9_gb9": (9, _MANY + (511,), 0),
    "k10_gb1": (10, (0, 1), 0), "k10_gb9": (10, _MANY + (511,), 0),
    "k20_gb1": (20, (0, 1), 0), "k20_gb9": (20, _MANY + (511,), 0),
    "k27_gb1": (27, (0, 1), 0), "k27_gb9": (27, _MANY + (511,), 0),
    "k27_log": (27, _MANY + (300,), 1),  # the log itself holds composites, the id field as wide as the word leaves room: 9 bits
    "k31_b1": (31, _MANY + (255,), 0), "k31_b2": (31, _MANY + (65535,), 0), "k31_b4": (31, _MANY + (70000,), 0),
    "k27_b4": (27, (0, 300, 70000), 0),
}
ROADS2 = {
    "k33": (33, _MANY + ((1 << 18) - 1,), 0), "k36": (36, _MANY + (300,), 0), "k37": (37, _MANY + (70000,), 0), "k45": (45, _MANY + (255,), 0),
    "k63": (63, _MANY + ((1 << 18) - 1,), 0), "k64": (64, _MANY + (65535,), 0),
    "k63_big": (63, _MANY + (1 << 18,), 0),  # one id that does not fit 18 bits: the kernels that keep the id in a register of its own
    "k36_big": (36, _MANY + (300000,), 0),
}
# what every road is meant to reach: gb (one word) / sh and PACK (two words), the width of an id beside the keys (0: composites)
ROAD_FACTS = {
    "k9_gb1": {"rest": 0, "gb": 1, "vw": 0}, "k9_gb9": {"rest": 0, "gb": 9, "vw": 0}, "k10_gb1": {"rest": 2, "gb": 1, "vw": 0}, "k10_gb9": {"rest": 2, "gb": 9, "vw": 0},
    "k20_gb1": {"rest": 22, "gb": 1, "vw": 0}, "k20_gb9": {"rest": 22, "gb": 9, "vw": 0}, "k27_gb1": {"rest": 36, "gb": 1, "vw": 0}, "k27_gb9": {"rest": 36, "gb": 9, "vw": 0},
    "k27_log": {"rest": 36, "gb": 9, "vw": 0},
    "k31_b1": {"rest": 44, "gb": 8, "vw": 1}, "k31_b2": {"rest": 44, "gb": 16, "vw": 2}, "k31_b4": {"rest": 44, "gb": 17, "vw": 4}, "k27_b4": {"rest": 36, "gb": 17, "vw": 4},
    "k33": {"sh": 2, "pack": True}, "k36": {"sh": 8, "pack": True}, "k37": {"sh": 10, "pack": True}, "k45": {"sh": 26, "pack": True}, "k63": {"sh": 62, "pack": True},
    "k64": {"sh": 64, "pack": True}, "k63_big": {"sh": 62, "pack": False}, "k36_big": {"sh": 8, "pack": False},
}
SIZES1 = (512, 513, 1536, 1537, 2304, 2305, 3072, 3073, 4096, 4097)  # the largest bucket, "test_front_wave_cap" by rule (512 at these sizes)
SIZES1_1024 = (1024, 1025, 1536)                                       # "test_front_wave_cap" 1024
SIZES2 = (64, 65, 512, 513, 1024, 1025, 2048, 2049, 4096, 4097, 8192, 8193)
# intended: size -> the kernel of the largest bucket (None: the call declines and the device-wide sort builds the index)
WANT1 = {512: "k_bucket_sort_wave<8>", 513: "k_bucket_sort<6, false>", 1536: "k_bucket_sort<6, false>", 1537: "k_bucket_sort<9, false>", 2304: "k_bucket_sort<9, false>",
         2305: "k_bucket_sort<12, false>", 3072: "k_bucket_sort<12, false>", 3073: "k_bucket_sort<16, false>", 4096: "k_bucket_sort<16, false>", 4097: None}
WANT1_1024 = {1024: "k_bucket_sort_wave<16>", 1025: "k_bucket_sort<6, false>", 1536: "k_bucket_sort<6, false>"}
WANT2 = {64: "k_bucket2_tiny", 65: "k_bucket2_sort_wave<8, {p}>", 512: "k_bucket2_sort_wave<8, {p}>", 513: "k_bucket2_sort_wave<16, {p}>", 1024: "k_bucket2_sort_wave<16, {p}>",
         1025: "k_bucket2_sort_wave<32, {p}>", 2048: "k_bucket2_sort_wave<32, {p}>", 2049: "k_bucket2_sort<16, false>", 4096: "k_bucket2_sort<16, false>",
         4097: "k_bucket2_sort<32, false>", 8192: "k_bucket2_sort<32, false>", 8193: None}
# every instantiation the launchers can choose (test_every_instantiation_is_covered holds it against the built library and against the cases)
INSTANTIATIONS = {"k_bucket_sort_wave<8>", "k_bucket_sort_wave<16>", "k_bucket_sort<6, false>", "k_bucket_sort<9, false>", "k_bucket_sort<12, false>", "k_bucket_sort<16, false>",
                  "k_bucket_sort<16, true>", "k_bucket_emit", "k_bucket2_lists", "k_bucket2_tiny", "k_bucket2_sort_wave<8, true>", "k_bucket2_sort_wave<16, true>",
                  "k_bucket2_sort_wave<32, true>", "k_bucket2_sort_wave<8, false>", "k_bucket2_sort_wave<16, false>", "k_bucket2_sort_wave<32, false>", "k_bucket2_sort<16, false>",
                  "k_bucket2_sort<32, false>", "k_bucket2_sort<32, true>", "k_bucket2_emit"}
# the cases that also run under "test_front_rank_mode" 1 and 2 (the fallback launch: k_bucket_sort<16, true> / k_bucket2_sort<32, true>)
MODE_ROADS = ("k10_gb1", "k27_gb9", "k31_b2", "k9_gb9", "k37", "k63", "k63_big")
CAP_ROADS = tuple(ROADS1)  # the rule cases of every one-word road also run under "test_front_wave_cap" 512 and 1024


# ---- the selection rules, from the library ----------------------------------------------------------------------------------------------------------
def plan(words, n, nb, max_bucket, max_gid, wave_cap, bucket):
    out = (C.c_uint32 * 8)()
    _lib.check(_lib.load().bft_gpu_debug_front_plan(words, n, nb, max_bucket, max_gid, wave_cap, bucket, out))
    return [int(x) for x in out]


def kernel_of(words, p):
    """the instantiation that owns the bucket the plan was asked about (None: nobody -- an empty bucket, or the call declines)"""
    if words == 1:
        return {0: None, 1: f"k_bucket_sort_wave<{p[1]}>", 2: f"k_bucket_sort<{p[2]}, false>"}[p[5]]
    pack = "true" if p[0] else "false"
    return {0: None, 1: f"k_bucket2_sort_wave<{p[6]}, {pack}>", 2: f"k_bucket2_sort<{p[6]}, false>", 3: "k_bucket2_tiny"}[p[7]]


def last_raw():
    """bft_gpu_debug_front_last: what the front end launched in its last call of this process; reading clears it"""
    out = (C.c_uint32 * 8)()
    _lib.check(_lib.load().bft_gpu_debug_front_last(out))
    return [int(x) for x in out]


def run_road(handle):
    """bft_gpu_debug_run_road of a BFT: [road (0 composites, 1 pairs, 2 the rest), gb, bytes of an id beside the keys, 1 when the split was tried]"""
    out = (C.c_uint32 * 4)()
    _lib.check(_lib.load().bft_gpu_debug_run_road(handle._h, out))
    return [int(x) for x in out]


def want_road(road):
    """what run_road must report for a case of this road, from ROAD_FACTS"""
    f = ROAD_FACTS[road]
    if road in ROADS1:
        return [0 if f["vw"] == 0 else 1, f["gb"], f["vw"], 1]
    return [2, bits_for(max(ROADS2[road][1])), 4, 1]


def last_kernel():
    """the kernel of the largest bucket in the front end's last call of this process (bft_gpu_debug_front_last), None where it declined"""
    out = (C.c_uint32 * 8)()
    _lib.check(_lib.load().bft_gpu_debug_front_last(out))
    words, mx, declined = out[0], out[1], out[2]
    if declined:
        return None, mx
    if words == 1:
        return (f"k_bucket_sort_wave<{out[4]}>" if mx <= out[3] else f"k_bucket_sort<{out[5]}, false>"), mx
    pack = "true" if out[3] else "false"
    return ("k_bucket2_tiny" if out[4] == 5 else f"k_bucket2_sort_wave<{out[5]}, {pack}>" if out[4] <= 2 else f"k_bucket2_sort<{out[5]}, false>"), mx


def want_kernel(road, size, wave_cap=0):
    """the kernel of a largest bucket of `size` pairs by the rules as DESIGN.md section 4 states them ("Which kernel sorts a bucket"), written out here
    (None: the call declines); nothing of the library's"""
    if road in ROADS1:
        cap = wave_cap or 512
        if size > 4096:
            return None
        if size <= cap:
            return f"k_bucket_sort_wave<{cap // 64}>"
        return "k_bucket_sort<%d, false>" % (6 if size <= 1536 else 9 if size <= 2304 else 12 if size <= 3072 else 16)
    pack = "true" if max(ROADS2[road][1]) < (1 << 18) else "false"
    if size > 8192:
        return None
    if size <= 64:
        return "k_bucket2_tiny"
    if size <= 2048:
        return "k_bucket2_sort_wave<%d, %s>" % (8 if size <= 512 else 16 if size <= 1024 else 32, pack)
    return "k_bucket2_sort<%d, false>" % (16 if size <= 4096 else 32)


def bits_for(v):
    """bits of the id field that holds ids up to v"""
    return max(1, int(v).bit_length())


# ---- keys -------------------------------------------------------------------------------------------------------------------------------------------
def digits_of(vals, nd):
    """Python integers below 4^nd -> [n, nd] base-4 digits, most significant first"""
    m64 = (1 << 64) - 1
    w = [np.array([(v >> (64 * j)) & m64 for v in vals], dtype=np.uint64) for j in range((2 * nd + 63) // 64 or 1)]
    out = np.zeros((len(vals), nd), dtype=np.uint8)
    for i in range(nd):
        sh = 2 * (nd - 1 - i)
        out[:, i] = ((w[sh // 64] >> np.uint64(sh % 64)) & np.uint64(3)).astype(np.uint8)
    return out


def codes_of(tkeys, k):
    """T-form keys (Python integers) -> [n, k] nucleotide codes: digit i of the key is the nucleotide t_order(k)[i]"""
    codes = np.zeros((len(tkeys), k), dtype=np.uint8)
    codes[:, G.P.t_order(k)] = digits_of(tkeys, k)
    return codes


def keys_of(codes, k):
    """the T-form keys of [n, k] codes as Python integers: keys_u64 over the first 32 digits and over the rest"""
    order = G.P.t_order(k).tolist()
    hi = G.keys_u64(codes, order[:32]).tolist()
    if k <= 32:
        return hi
    lo = G.keys_u64(codes, order[32:]).tolist()
    return [(a << (2 * (k - 32))) | b for a, b in zip(hi, lo)]


# ---- truth ------------------------------------------------------------------------------------------------------------------------------------------
class Truth:
    """from the inserted pairs alone: keys [(T-form key, genome id)] in insertion order, codes [n, k] beside them"""

    def __init__(self, k, keys, gids, codes):
        sets, first = {}, {}
        for i, (x, g) in enumerate(zip(keys, gids)):
            if x not in sets:
                sets[x] = set()
                first[x] = i
            sets[x].add(g)
        self.k = k
        self.sets = {x: tuple(sorted(s)) for x, s in sets.items()}
        self.order = sorted(sets)
        self.kmers = len(self.order)
        self.pairs = sum(len(s) for s in self.sets.values())
        shift = max(2 * k - SPLIT_TOP, 0)
        self.buckets = dict(collections.Counter(x >> shift for x in keys))  # as inserted, before de-duplication
        self.max_bucket = max(self.buckets.values())
        self.codes = np.ascontiguousarray(codes[[first[x] for x in self.order]])  # the distinct k-mers in key order
        self.packed = G.pack(self.codes)

    def colour_map(self):
        """{packed k-mer bytes: ids}"""
        return {self.packed[i].tobytes(): self.sets[x] for i, x in enumerate(self.order)}

    def absent(self, n, seed):
        """packed one-base mutants of a sample of the stored k-mers, none of them stored"""
        rng = np.random.default_rng(seed)
        have, out = set(self.order), []
        for i in rng.integers(0, self.kmers, 4 * n).tolist():
            x = self.codes[i].copy()
            j = int(rng.integers(0, self.k))
            x[j] = (x[j] + int(rng.integers(1, 4))) & 3
            if keys_of(x[None], self.k)[0] not in have:
                out.append(x)
            if len(out) == n:
                break
        return G.pack(np.array(out, dtype=np.uint8))


# ---- bucket contents ----------------------------------------------------------------------------------------------------------------------------------
def _distinct_rests(rng, R, m):
    """min(m, 2^R) distinct R-bit values, ascending"""
    if R <= 16:
        pool = list(range(1 << R))
        if len(pool) > m:
            pool = sorted(rng.choice(len(pool), m, replace=False).tolist())
        return pool
    out = set()
    while len(out) < m:
        out.add(int.from_bytes(rng.bytes(16), "little") % (1 << R))
    return sorted(out)


def _spread(n, m):
    """n pairs over m k-mers, as evenly as they go"""
    return [n // m + (1 if i < n % m else 0) for i in range(m)]


def _slots(L, S, rng, dup=False):
    """the genomes (positions in the labelling) of a k-mer held by L pairs: L distinct genomes where there are that many (one of them twice, one
    fewer, for `dup`), else every genome, some more than once"""
    if L > S:
        return sorted(i % S for i in range(L))
    if dup and L >= 2:
        s = sorted(rng.choice(S, L - 1, replace=False).tolist())
        return sorted(s + [s[int(rng.integers(0, len(s)))]])
    return sorted(rng.choice(S, L, replace=False).tolist())


def bucket_runs(shape, n, R, S, rng):
    """[(the R key bits below the root prefix, [genome slot of every pair])], n pairs in all"""
    if R == 0 or shape == "one_pair":
        r = _distinct_rests(rng, R, 1)[0]
        return [(r, [int(rng.integers(0, S))] * n if shape == "one_pair" else sorted(i % S for i in range(n)))]
    if shape == "one_kmer":
        return [(_distinct_rests(rng, R, 1)[0], sorted(i % S for i in range(n)))]
    if shape == "distinct":
        rests = _distinct_rests(rng, R, n)
        if len(rests) == n:
            return [(r, [int(rng.integers(0, S))]) for r in rests]
        return [(r, _slots(L, S, rng)) for r, L in zip(rests, _spread(n, len(rests))) if L]
    if shape == "shared":
        lens, i = [], 0
        while sum(lens) < n:
            lens.append(min(RUN_CYCLE[i % 4], n - sum(lens)))
            i += 1
        avail = min(1 << R, 1 << 20)
        if len(lens) > avail:
            lens = lens[:avail - 1] + [n - sum(lens[:avail - 1])]
        rests = _distinct_rests(rng, R, len(lens))
        return [(r, _slots(L, S, rng, dup=j % 5 == 4 and L > 2)) for j, (r, L) in enumerate(zip(rests, lens))]
    # k-mers that differ in chosen bits only, one or a few pairs each
    base = _distinct_rests(rng, R, 1)[0]
    if shape == "low_bit":
        m = min(max(n // 2, 1), 1 << (R - 1))
        rests = sorted({(x << 1 | b) for x in _distinct_rests(rng, R - 1, m) for b in (0, 1)})
    elif shape == "high_bit":
        m = min(max(n // 2, 1), 1 << (R - 1))
        rests = sorted({x | (b << (R - 1)) for x in _distinct_rests(rng, R - 1, m) for b in (0, 1)})
    else:  # top_digit: the bits of the last, partial pass
        pb = R % DBITS or DBITS
        rests = [(base & ((1 << (R - pb)) - 1)) | (v << (R - pb)) for v in range(1 << pb)]
    rests = rests[:n]
    return [(r, _slots(L, S, rng)) for r, L in zip(rests, _spread(n, len(rests))) if L]


# ---- cases --------------------------------------------------------------------------------------------------------------------------------------------
class Case:
    """buckets: [(root prefix, pairs, shape)], the first the largest"""

    def __init__(self, name, road, buckets, wave_cap=0, seed=0):
        self.name, self.road, self.buckets, self.wave_cap = name, road, buckets, wave_cap
        self.k, self.gids, self.comp_log = (ROADS1.get(road) or ROADS2[road])
        self.words = 1 if self.k <= 32 else 2
        k, S = self.k, len(self.gids)
        R = 2 * k - SPLIT_TOP
        rng = np.random.default_rng(seed)
        tkeys, slot = [], []
        self.runs = {}
        for prefix, n, shape in buckets:
            runs = bucket_runs(shape, n, R, S, rng)
            if shape == "one_pair" and prefix == buckets[-1][0]:
                runs = [(runs[0][0], [S - 1] * n)]  # the last genome of the labelling holds something: its id decides gb, the id width and PACK
            assert sum(len(s) for _, s in runs) == n and len({r for r, _ in runs}) == len(runs)
            self.runs[prefix] = runs
            for r, slots in runs:
                tkeys += [(prefix << R) | r] * len(slots)
                slot += slots
        slot = np.array(slot)
        codes = codes_of(tkeys, k)
        # genome by genome (the ids ascend, as the ordered roads want them), the k-mers of a genome shuffled; some genomes in two calls
        self._inserts, order = [], []
        for s in range(S):
            mine = rng.permutation(np.flatnonzero(slot == s))
            if len(mine) == 0:
                continue
            cut = len(mine) // 3 if s % 3 == 1 else 0
            for part in ((mine[:cut], mine[cut:]) if cut else (mine,)):
                self._inserts.append((self.gids[s], G.pack(codes[part])))
                order.append(part)
        order = np.concatenate(order)
        self.ins_codes = codes[order]
        self.ins_gids = [self.gids[s] for s in slot[order].tolist()]
        self.n = len(order)

    def inserts(self):
        """[(genome id, packed k-mers)] in the order of the calls"""
        return self._inserts

    @functools.cached_property
    def truth(self):
        return Truth(self.k, keys_of(self.ins_codes, self.k), self.ins_gids, self.ins_codes)

    # -- what the library's rules make of it (the truth's own bucket sizes)
    def plan(self, bucket=0, wave_cap=None):
        nb = 1 << min(SPLIT_TOP, 2 * self.k)
        return plan(self.words, self.n, nb, self.truth.max_bucket, max(self.ins_gids), self.wave_cap if wave_cap is None else wave_cap, bucket)

    def owner(self, n):
        return kernel_of(self.words, self.plan(n))

    def declines(self):
        return bool(self.plan()[3])

    def kernels(self):
        """every instantiation that sorts some bucket of the case"""
        return {self.owner(n) for n in self.truth.buckets.values()} - {None}

    def redone(self):
        """buckets the fallback launch sorts under "test_front_rank_mode" 1 and 2: every non-empty bucket a radix kernel owns -- not the tiny
        two-word buckets (ranked by comparison), not k = 9 (the split covers every bit: nothing is sorted), none when the call declines"""
        if self.declines() or 2 * self.k <= SPLIT_TOP:
            return 0
        return sum(1 for n in self.truth.buckets.values() if self.owner(n) not in (None, "k_bucket2_tiny"))


def _prefixes(rng, m):
    """m root prefixes with empty buckets on both sides of each, in no order"""
    while True:
        p = rng.choice(np.arange(3, (1 << SPLIT_TOP) - 3), m, replace=False)
        s = np.sort(p)
        if (np.diff(s) >= 2).all():
            return p.tolist()


def _beneath(words, size, cap):
    """a bucket on the lower edge of every class beneath the largest (1 and 63 among them), and on the upper edge of the wavefronts'"""
    edges = (1, 63, 64, 65, cap, cap + 1) if words == 1 else (1, 63, 64, 65, 512, 513, 1024, 1025, 2048, 2049, 4097)
    return [e for e in edges if e < size]


@functools.lru_cache(maxsize=4)
def case(road, size, wave_cap=0):
    roads = list(ROADS1) + list(ROADS2)
    words = 1 if road in ROADS1 else 2
    sizes = (SIZES1 + SIZES1_1024) if words == 1 else SIZES2
    seed = 1000 * roads.index(road) + 10 * sizes.index(size) + (wave_cap == 1024)
    rng = np.random.default_rng(seed)
    first = (roads.index(road) + sizes.index(size)) % len(SHAPES)  # the shape of the largest bucket; those beneath it take the others in turn
    sizes_all = [size] + _beneath(words, size, wave_cap or 512) + [2, 17, 40]
    pre = _prefixes(rng, len(sizes_all) - 2) + [0, (1 << SPLIT_TOP) - 1]  # (the first and the last bucket of the split hold two of the small ones)
    buckets = [(p, n, SHAPES[(first + i) % len(SHAPES)]) for i, (p, n) in enumerate(zip(pre, sizes_all))]
    buckets[-1] = buckets[-1][:2] + ("one_pair",)  # (duplicate pairs in every case)
    return Case(f"{road}-{size}" + (f"-cap{wave_cap}" if wave_cap else ""), road, buckets, wave_cap, seed)


CASES1 = [(road, size, 0) for road in ROADS1 for size in SIZES1] + [(road, size, 1024) for road in ROADS1 for size in SIZES1_1024]
CASES2 = [(road, size, 0) for road in ROADS2 for size in SIZES2]
CASES = CASES1 + CASES2
MODE_CASES = [c for c in CASES if c[0] in MODE_ROADS]
CAP_CASES = [(road, size, cap) for road in CAP_ROADS for size in SIZES1 for cap in (512, 1024)]  # the rule cases, the cap forced


@functools.lru_cache(maxsize=2)
def two_step(road):
    """(the first case; the calls of the second build; the truth of the second build's own pairs; the truth of the index): the second build brings
    new buckets beside the first's, new k-mers into the first's buckets, and every third k-mer of the first again under the last genome"""
    a = case(road, 1537 if road in ROADS1 else 2049)
    b = Case(f"{road}-second", road, [(p + 1 if i % 2 else p, max(n // 2, 1), s) for i, (p, n, s) in enumerate(a.buckets[:-2])], 0, 77)
    g, again = a.gids[-1], a.truth.codes[::3]
    codes2, gids2 = np.concatenate([b.ins_codes, again]), b.ins_gids + [g] * len(again)
    second = Truth(a.k, keys_of(codes2, a.k), gids2, codes2)
    codes = np.concatenate([a.ins_codes, codes2])
    return a, b.inserts() + [(g, G.pack(again))], second, Truth(a.k, keys_of(codes, a.k), a.ins_gids + gids2, codes)


@functools.lru_cache(maxsize=None)
def digest(road, size, wave_cap=0):
    """what the coverage tests need of a case, kept small: [(prefix, pairs, shape, owner, events)], declines, redone"""
    c = case(road, size, wave_cap)
    return {"buckets": [(p, n, s, c.owner(n), frozenset(_events(c, p, n))) for p, n, s in c.buckets], "declines": c.declines(), "redone": c.redone(), "k": c.k, "words": c.words,
            "kernels": c.kernels(), "nonempty": len(c.truth.buckets), "sizes": sorted(c.truth.buckets.values())}


# ---- tests: the key is the library's --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hostlib():
    subprocess.check_call(["make", "-C", _lib.CSRC, "all"], stdout=subprocess.DEVNULL)
    lib = C.CDLL(os.path.join(_lib.CSRC, "libbft_hosttest.so"))
    lib.bft_hosttest_roundtrip.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p]
    return lib


@pytest.mark.parametrize("road", list(ROADS1) + list(ROADS2))
def test_t_form_key_is_the_librarys(hostlib, road):
    c = case(road, 513)
    k, tr = c.k, c.truth
    pick = np.unique(np.concatenate([np.arange(0, tr.kmers, 7), [tr.kmers - 1]]))
    packed = np.ascontiguousarray(tr.packed[pick])
    W = G.shape_of(k)["W"]
    out, tf = np.zeros_like(packed), np.zeros(len(packed) * W, dtype=np.uint64)
    hostlib.bft_hosttest_roundtrip(packed.ctypes.data, len(packed), k, out.ctypes.data, tf.ctypes.data)
    assert (out == packed).all()
    got = [sum(int(w) << (64 * (W - 1 - j)) for j, w in enumerate(tf[i * W:(i + 1) * W])) for i in range(len(packed))]
    assert got == [tr.order[i] for i in pick.tolist()] == G.P.t_key_ints(tr.codes[pick], k)
    assert W == c.words


def test_hook_symbol_errors_and_header():
    hdr = open(_lib.HEADER).read()
    assert re.search(r"\bint\s+bft_gpu_debug_front_plan\s*\(\s*int\s+words\s*,\s*uint64_t\s+n\s*,\s*uint32_t\s+nb\s*,\s*uint32_t\s+max_bucket\s*,\s*uint32_t\s+max_gid\s*,"
                     r"\s*uint32_t\s+wave_cap\s*,\s*uint32_t\s+bucket\s*,\s*uint32_t\s+out\s*\[\s*8\s*\]\s*\)\s*;", hdr)
    assert re.search(r"\bint\s+bft_gpu_debug_front_last\s*\(\s*uint32_t\s+out\s*\[\s*8\s*\]\s*\)\s*;", hdr) and "bft_gpu_debug_front_last" in _lib.SIGNATURES
    assert re.search(r"\bint\s+bft_gpu_debug_run_road\s*\(\s*bft_gpu\s*\*\s*h\s*,\s*uint32_t\s+out\s*\[\s*4\s*\]\s*\)\s*;", hdr) and "bft_gpu_debug_run_road" in _lib.SIGNATURES
    assert "bft_gpu_debug_front_plan" in _lib.SIGNATURES and '"test_front_wave_cap"' in hdr
    lib = _lib.load()
    out = (C.c_uint32 * 8)()
    assert lib.bft_gpu_debug_front_plan(1, 100, 1 << 18, 10, 0, 0, 5, None) == -1 and lib.bft_gpu_debug_front_last(None) == -1  # BFT_GPU_E_ARG
    assert lib.bft_gpu_debug_run_road(None, out) == -1
    for words, cap, bucket in ((0, 0, 5), (3, 0, 5), (1, 256, 5), (1, 2048, 5), (1, 0, 11), (2, 0, 11)):
        assert lib.bft_gpu_debug_front_plan(words, 100, 1 << 18, 10, 0, cap, bucket, out) == -1, (words, cap, bucket)
    assert lib.bft_gpu_debug_front_plan(1, 100, 1 << 18, 10, 0, 0, 5, out) == 0 and list(out) == [512, 8, 0, 0, 4096, 1, 0, 0]


def test_the_rules_at_their_borders():
    """the rules as DESIGN.md section 4 states them (one word: a wavefront up to 512 or 1024 by the mean bucket, a workgroup of 6 / 9 / 12 / 16 pairs per
    thread up to 1536 / 2304 / 3072 / 4096; two words: classes up to 64 / 512 / 1024 / 2048 / 4096 / 8192), asked of the library at both sides of every border"""
    nb = 1 << 18
    cap = lambda n, forced=0: plan(1, n, nb, 1, 0, forced, 1)[0]
    assert [cap(192 * nb + nb - 1), cap(193 * nb), cap(193 * nb, 512), cap(0, 1024), cap(5000)] == [512, 1024, 512, 1024, 512]
    e = lambda mx, forced=0: plan(1, 5000, nb, mx, 0, forced, mx)[1:4] + [plan(1, 5000, nb, mx, 0, forced, mx)[5]]
    assert [e(m) for m in (1, 512, 513, 1536, 1537, 2304, 2305, 3072, 3073, 4096, 4097)] == [
        [8, 0, 0, 1], [8, 0, 0, 1], [8, 6, 0, 2], [8, 6, 0, 2], [8, 9, 0, 2], [8, 9, 0, 2], [8, 12, 0, 2], [8, 12, 0, 2], [8, 16, 0, 2], [8, 16, 0, 2], [8, 0, 1, 0]]
    assert [e(m, 1024) for m in (512, 1024, 1025, 1536, 1537, 4097)] == [[16, 0, 0, 1], [16, 0, 0, 1], [16, 6, 0, 2], [16, 6, 0, 2], [16, 9, 0, 2], [16, 0, 1, 0]]
    cls = lambda n: plan(2, 5000, nb, 8192, 0, 0, n)[5:8]
    assert [cls(n) for n in (0, 1, 64, 65, 512, 513, 1024, 1025, 2048, 2049, 4096, 4097, 8192)] == [
        [0xFFFFFFFF, 0, 0], [5, 1, 3], [5, 1, 3], [0, 8, 1], [0, 8, 1], [1, 16, 1], [1, 16, 1], [2, 32, 1], [2, 32, 1], [3, 16, 2], [3, 16, 2], [4, 32, 2], [4, 32, 2]]
    launched = lambda mx, gid=0: plan(2, 5000, nb, mx, gid, 0, 1)[:5]
    assert [launched(m) for m in (2048, 2049, 4096, 4097, 8192, 8193)] == [[1, 0, 0, 0, 8192], [1, 1, 0, 0, 8192], [1, 1, 0, 0, 8192], [1, 1, 1, 0, 8192], [1, 1, 1, 0, 8192],
                                                                             [1, 0, 0, 1, 8192]]
    assert launched(100, (1 << 18) - 1)[0] == 1 and launched(100, 1 << 18)[0] == 0


# ---- tests: every case is what it is named after --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("road,size,wave_cap", CASES, ids=lambda x: str(x))
def test_case_reaches_its_regime(road, size, wave_cap):
    c = case(road, size, wave_cap)
    tr = c.truth
    # the buckets are exactly the intended ones, the largest among them, with empty buckets on both sides of all but the split's first and last
    assert tr.buckets == {p: n for p, n, _ in c.buckets} and tr.max_bucket == size == c.buckets[0][1]
    assert sorted(tr.buckets.values())[-2] < size and sum(tr.buckets.values()) == c.n <= 26000
    for p, _, _ in c.buckets[:-2]:
        assert p - 1 not in tr.buckets and p + 1 not in tr.buckets and 0 < p < (1 << SPLIT_TOP) - 1
    assert 0 in tr.buckets and (1 << SPLIT_TOP) - 1 in tr.buckets
    # the plan names the intended kernel, or the decline
    want = (WANT1_1024 if wave_cap else WANT1)[size] if c.words == 1 else WANT2[size]
    want = want and want.format(p="true" if ROAD_FACTS[road].get("pack") else "false")
    assert c.owner(size) == want == want_kernel(road, size, wave_cap) and c.declines() == (want is None)
    p = c.plan()
    if c.words == 1:
        assert p[0] == (wave_cap or 512) and p[4] == 4096
        for n in (1, 63, 64, 65, p[0]):
            if n < size:
                assert n in tr.buckets.values() and (c.declines() or c.owner(n) == f"k_bucket_sort_wave<{p[0] // 64}>")
        if p[0] + 1 < size and not c.declines():
            assert p[0] + 1 in tr.buckets.values() and c.owner(p[0] + 1) == want  # the workgroup kernel's smallest bucket beside its largest
    else:
        assert p[4] == 8192 and p[1] == (2048 < size <= 8192) and p[2] == (4096 < size <= 8192)
        for n, cls in ((1, 5), (63, 5), (64, 5), (65, 0), (512, 0), (513, 1), (1024, 1), (1025, 2), (2048, 2), (2049, 3), (4097, 4)):
            if n < size:
                assert n in tr.buckets.values() and c.plan(n)[5] == cls
    # pairs, k-mers and duplicates
    assert tr.pairs <= c.n and tr.kmers <= tr.pairs and tr.kmers >= len(c.buckets)
    assert tr.pairs < c.n  # duplicate pairs somewhere
    if c.k >= 20:
        assert tr.kmers < tr.pairs  # a k-mer under several ids somewhere
    # the ids ascend over the calls, and the k-mers of a call are not in key order
    g = [gid for gid, _ in c.inserts()]
    assert max(c.ins_gids) == max(c.gids)  # the id that decides gb, the id width and PACK is inserted
    assert g == sorted(g) and len(g) > len(set(g)) and c.ins_gids == sorted(c.ins_gids)
    keys = keys_of(c.ins_codes, c.k)
    assert keys != sorted(keys) or c.k == 9


@pytest.mark.parametrize("road", list(ROADS1) + list(ROADS2))
def test_id_labellings_give_the_intended_widths(road):
    """ROAD_FACTS against the rules of csrc/bft_run.hip written out once more (tests/test_gpu_front_edges.py holds them against the library itself:
    bft_gpu_debug_run_road after every build)"""
    k, gids, comp_log = ROADS1.get(road) or ROADS2[road]
    f = ROAD_FACTS[road]
    mx = max(gids)
    assert list(gids) == sorted(set(gids)) and (len(gids) >= 66 or road.endswith("gb1") or road == "k27_b4")
    if road in ROADS1:
        # csrc/bft_run.hip: a composite T << gb | id of up to 63 bits; else pairs, the id in 1, 2 or 4 bytes beside the key, and a bucket's composite in 64
        gb = min(63 - 2 * k, 24) if comp_log else bits_for(mx)
        assert gb == f["gb"] and 2 * k - SPLIT_TOP == f["rest"]
        fits = 2 * k + gb <= 63
        assert fits == (f["vw"] == 0)
        if comp_log:
            assert 63 - 2 * k >= 7 and mx < (1 << gb)
        if not fits:
            assert f["vw"] == (1 if mx < 256 else 2 if mx < 65536 else 4) and f["rest"] + gb <= 64 and 2 * k < 64
    else:
        assert 2 * k - 64 == f["sh"] and (mx < (1 << 18)) == f["pack"] and 33 <= k <= 64
        assert plan(2, 100, 1 << 18, 10, mx, 0, 1)[0] == f["pack"]
    # the key bits of a bucket in passes of 9: 22 = 9 + 9 + 4 at k = 20, four whole passes at k = 27, a last pass of 8 bits at k = 31, ...
    R = 2 * k - SPLIT_TOP
    passes = [min(DBITS, R - b) for b in range(0, R, DBITS)]
    assert {9: [], 10: [2], 20: [9, 9, 4], 27: [9] * 4, 31: [9] * 4 + [8], 33: [9] * 5 + [3], 36: [9] * 6, 37: [9] * 6 + [2], 45: [9] * 8, 63: [9] * 12, 64: [9] * 12 + [2]}[k] == passes
    if k == 37:
        assert f["sh"] == 10 and 9 < f["sh"] < 18  # the second pass takes the last bit of lo and eight of hk


def test_roads_cover_the_key_and_id_table():
    assert {ROADS1[r][0] for r in ROADS1} == {9, 10, 20, 27, 31} and {ROADS2[r][0] for r in ROADS2} == {33, 36, 37, 45, 63, 64}
    assert {(ROADS1[r][0], ROAD_FACTS[r]["gb"]) for r in ROADS1 if ROAD_FACTS[r]["vw"] == 0} >= {(k, gb) for k in (9, 10, 20, 27) for gb in (1, 9)}
    assert {ROAD_FACTS[r]["vw"] for r in ROADS1 if ROADS1[r][0] == 31} == {1, 2, 4} and ROADS1["k27_b4"][1] == (0, 300, 70000)
    assert {ROAD_FACTS[r]["sh"] for r in ROADS2} >= {2, 10, 64} and [r for r in ROADS2 if not ROAD_FACTS[r]["pack"]] == ["k63_big", "k36_big"]
    assert max(ROADS2["k63"][1]) == (1 << 18) - 1 and max(ROADS2["k63_big"][1]) == 1 << 18  # both sides of PACK's border


# ---- tests: the shapes ----------------------------------------------------------------------------------------------------------------------------------
def _sorted_runs(c, prefix):
    """[(first, last)] positions of every k-mer's pairs in the sorted bucket"""
    out, pos = [], 0
    for _, slots in sorted(c.runs[prefix]):
        out.append((pos, pos + len(slots) - 1))
        pos += len(slots)
    return out


def _slot(i, n, owner):
    """(wave, round, lane) of position i of a bucket of n pairs"""
    if "sort_wave" in owner or owner.endswith("tiny"):
        return 0, i // 64, i % 64
    E = (n + 255) // 256
    return i // (64 * E), (i % (64 * E)) // 64, i % 64


def _events(c, prefix, n):
    owner = c.owner(n) or ("k_bucket_sort<16, false>" if c.words == 1 else "k_bucket2_sort<32, false>")
    ev = set()
    for a, b in _sorted_runs(c, prefix):
        (wa, ra, la), (wb, rb, lb) = _slot(a, n, owner), _slot(b, n, owner)
        if b > a:
            ev |= {"end63"} if lb == 63 else set()
            ev |= {"start0"} if la == 0 and a > 0 else set()
            ev |= {"round"} if (wa, ra) != (wb, rb) else set()
            ev |= {"wbase"} if wa != wb else set()
            ev |= {"chunk"} if a // 256 != b // 256 else set()
            ev |= {"whole_wave"} if b - a >= 127 else set()  # a run that holds every lane of some round
        ev |= {"chunk_head"} if a and a % 256 == 0 else set()  # a k-mer that begins where the emit kernels begin a turn
    return ev


@pytest.mark.parametrize("road,size,wave_cap", [c for c in CASES if c[0] not in ("k9_gb1", "k9_gb9", "k10_gb1", "k10_gb9")], ids=lambda x: str(x))
def test_shapes_are_what_they_are_named(road, size, wave_cap):
    c = case(road, size, wave_cap)
    R = 2 * c.k - SPLIT_TOP
    for prefix, n, shape in c.buckets:
        runs = sorted(c.runs[prefix])
        rests = [r for r, _ in runs]
        if shape == "distinct":
            assert len(runs) == n and all(len(s) == 1 for _, s in runs)
        elif shape == "one_pair":
            assert len(runs) == 1 and len(set(runs[0][1])) == 1 and len(runs[0][1]) == n
        elif shape == "one_kmer":
            assert len(runs) == 1 and len(set(runs[0][1])) == min(n, len(c.gids))
        elif shape == "shared":
            assert [len(s) for _, s in runs][:-1] == [RUN_CYCLE[i % 4] for i in range(len(runs) - 1)]
            if len(c.gids) >= 66:
                held = {len(set(s)) for _, s in runs[:-1]}
                assert held <= {2, 62, 63, 64, 65} and (n < 260 or held >= {2, 63, 64, 65})
                assert n < 322 or any(len(set(s)) < len(s) for _, s in runs)  # a duplicate pair beside them
        elif shape == "low_bit" and n >= 2:
            assert all(a ^ b == 1 for a, b in zip(rests[0::2], rests[1::2])) and len(rests) >= 2
        elif shape == "high_bit" and n >= 2:
            half = len(rests) // 2
            assert half >= 1 and all(a ^ b == 1 << (R - 1) for a, b in zip(rests[:half], rests[half:]))
        elif shape == "top_digit" and n >= 2:
            pb = R % DBITS or DBITS
            assert len({r & ((1 << (R - pb)) - 1) for r in rests}) == 1 and len(rests) == min(n, 1 << pb)


def test_run_shapes_cross_the_borders():
    """in the largest bucket of every "shared" case, and over the buckets each kernel owns: runs of equal k-mers that end at lane 63, start at lane 0,
    cross a round, the slots of a wavefront (workgroup kernels) and the emit's 256 positions; "one_kmer" / "one_pair": runs over whole wavefronts"""
    by_kernel = collections.defaultdict(set)
    for road, size, cap in CASES:
        if ROAD_FACTS[road].get("rest", 99) < 20 or len(ROADS1.get(road, ROADS2.get(road))[1]) < 66:
            continue
        for prefix, n, shape, owner, ev in digest(road, size, cap)["buckets"]:
            if owner:
                by_kernel[owner] |= {(shape, e) for e in ev}
            if shape == "shared" and n == size:
                want = {"end63", "start0", "round"} if n >= 192 else set()
                want |= {"chunk"} if n >= 322 else set()
                want |= {"wbase"} if owner and "sort<" in owner else set()
                assert want <= ev, (road, size, cap, want - ev)
            if shape in ("one_kmer", "one_pair") and n >= 128:
                assert {"whole_wave", "round"} <= ev
    for kern, seen in by_kernel.items():
        if kern == "k_bucket2_tiny":
            continue
        assert {("shared", e) for e in ("end63", "start0", "round")} <= seen, kern
        assert ("one_kmer", "whole_wave") in seen or ("one_pair", "whole_wave") in seen, kern
        if "sort<" in kern:
            assert ("shared", "wbase") in seen and ("shared", "chunk") in seen, kern
    # the emit kernels: in every road some k-mer begins on a turn's first position, and some k-mer's pairs lie across it
    for road in list(ROADS1) + list(ROADS2):
        ev = set().union(*[b[4] for size in (SIZES1 if road in ROADS1 else SIZES2) for b in digest(road, size)["buckets"]])
        assert {"chunk_head", "chunk"} <= ev or (2 * (ROADS1.get(road) or ROADS2[road])[0] - SPLIT_TOP < 20 and "chunk" in ev), road  # (k = 9, 10: one and four k-mers)
    assert set(by_kernel) == INSTANTIATIONS - {"k_bucket_sort<16, true>", "k_bucket2_sort<32, true>", "k_bucket_emit", "k_bucket2_emit", "k_bucket2_lists"}


def test_every_shape_meets_every_kernel():
    seen = collections.defaultdict(set)
    for x in CASES:
        for prefix, n, shape, owner, _ in digest(*x)["buckets"]:
            if owner and n >= 2:
                seen[owner].add(shape)
    for kern, shapes in seen.items():
        assert shapes == set(SHAPES), (kern, set(SHAPES) - shapes)


# ---- tests: coverage ------------------------------------------------------------------------------------------------------------------------------------
def test_every_instantiation_is_covered():
    """the k_bucket* kernels of the built library are exactly the instantiations named here, and the cases' plans name every one of them"""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "k_bucket"], capture_output=True, text=True).stdout
    built = set(re.findall(r"(k_bucket[a-z0-9_]*(?:<[^>]*>)?)\(", out))
    assert built == INSTANTIATIONS, built ^ INSTANTIATIONS
    named = set()
    for x in CASES:
        d = digest(*x)
        named |= d["kernels"]
        if not d["declines"]:
            named.add("k_bucket_emit" if d["words"] == 1 else "k_bucket2_emit")
        if d["words"] == 2:
            named.add("k_bucket2_lists")
    # the fallback launch sorts the buckets of the mode cases that a radix kernel owns
    assert any(digest(*x)["redone"] for x in MODE_CASES if digest(*x)["words"] == 1) and any(digest(*x)["redone"] for x in MODE_CASES if digest(*x)["words"] == 2)
    named |= {"k_bucket_sort<16, true>", "k_bucket2_sort<32, true>"}
    assert named == INSTANTIATIONS, named ^ INSTANTIATIONS
    # and each of them owns the largest bucket of some case on both of its borders
    largest = collections.defaultdict(set)
    for road, size, cap in CASES:
        largest[digest(road, size, cap)["buckets"][0][3]].add(size)
    assert {k: sorted(v) for k, v in largest.items() if k} == {
        "k_bucket_sort_wave<8>": [512], "k_bucket_sort_wave<16>": [1024], "k_bucket_sort<6, false>": [513, 1025, 1536], "k_bucket_sort<9, false>": [1537, 2304],
        "k_bucket_sort<12, false>": [2305, 3072], "k_bucket_sort<16, false>": [3073, 4096], "k_bucket2_tiny": [64],
        "k_bucket2_sort_wave<8, true>": [65, 512], "k_bucket2_sort_wave<16, true>": [513, 1024], "k_bucket2_sort_wave<32, true>": [1025, 2048],
        "k_bucket2_sort_wave<8, false>": [65, 512], "k_bucket2_sort_wave<16, false>": [513, 1024], "k_bucket2_sort_wave<32, false>": [1025, 2048],
        "k_bucket2_sort<16, false>": [2049, 4096], "k_bucket2_sort<32, false>": [4097, 8192]}
    assert sorted(largest[None]) == [4097, 8193]


def test_mode_and_cap_cases():
    """the redo counts are stated from the plan: none at k = 9 and where the call declines, every non-empty bucket of one-word keys otherwise, the
    buckets beyond 64 items of two-word keys"""
    assert {c[0] for c in MODE_CASES} == set(MODE_ROADS) and {c[2] for c in MODE_CASES} == {0, 1024}
    for x in MODE_CASES:
        d = digest(*x)
        if d["k"] == 9 or d["declines"]:
            assert d["redone"] == 0
        elif d["words"] == 1:
            assert d["redone"] == d["nonempty"] == len(d["buckets"])
        else:
            assert d["redone"] == sum(1 for n in d["sizes"] if n > 64) < d["nonempty"]
    assert any(digest(*x)["declines"] for x in MODE_CASES) and any(digest(*x)["k"] == 9 for x in MODE_CASES)
    # the rule cases under a forced cap: 1024 hands the buckets of 513 .. 1024 pairs to k_bucket_sort_wave<16>
    for road, size, cap in CAP_CASES:
        c = case(road, size)
        p = c.plan(size, wave_cap=cap)
        assert kernel_of(1, p) == want_kernel(road, size, cap)
        assert p[0] == cap and p[1] == cap // 64 and p[3] == (size > 4096)
        if cap == 1024 and 513 <= size <= 4096:
            assert kernel_of(1, c.plan(513, wave_cap=cap)) == "k_bucket_sort_wave<16>" and kernel_of(1, c.plan(513, wave_cap=512)).startswith("k_bucket_sort<")


TWO_STEP_ROADS = ("k27_gb9", "k31_b2", "k37", "k63_big")


@pytest.mark.parametrize("road", TWO_STEP_ROADS)
def test_two_step_cases(road):
    a, calls, second, tr = two_step(road)
    shared = set(a.truth.order) & set(second.order)
    assert len(shared) >= a.truth.kmers // 3 and set(second.order) - set(a.truth.order)  # k-mers the second build adds ids to, and new ones
    assert tr.kmers == len(set(a.truth.order) | set(second.order)) and a.truth.pairs < tr.pairs < a.truth.pairs + second.pairs  # (new ids on stored k-mers, and pairs the index held)
    g = [gid for gid, _ in calls]
    assert g == sorted(g) and second.max_bucket > (64 if a.words == 2 else 512) and not a.declines()
    assert set(second.buckets) & set(a.truth.buckets) and set(second.buckets) - set(a.truth.buckets)
