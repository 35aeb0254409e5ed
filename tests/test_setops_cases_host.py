"""The colour-set algebra over groups (csrc/bft_setops.hip): the case generator and the truth that tests/test_gpu_setops_edges.py runs on the
GPU, and -- here, without a GPU -- the proof that every case reaches the regime it is named after.

Truth.  A family is a hand-made index of one row width: K-mers of about 40 sets of sparse genome ids, and k-mers that no genome holds.  `own`
[set, genome] is the ownership matrix of what the test inserts.  A group is a tuple of runs (set, members); its result is numpy set algebra over
the rows of its DISTINCT sets plus its absent count (an 8-million-member group costs nothing), under the rules tests/test_gpu_setops.py states in
Pool.truth: a genome is in the AND when every member that counts holds it, in the OR when one does; SYMDIFF is OR minus AND, and the OR itself for
a group of one counting member; an absent member counts as the empty set, or not at all under skip_absent.  The product only names colour-set ids.

The plan model (klass, steps, loads, heads, rounds, passes) restates how the kernels cut a batch, from the six constants of
bft_gpu_debug_setops_plan (no literal of bft_setops.h is repeated here).  It is only used to prove where the cases land; it is never the truth."""
import ctypes as C
from collections import namedtuple

import numpy as np
import pytest

from bloomfiltertrie_amd import _lib, synth as S

AND, OR, SYMDIFF = 0, 1, 2
OPS = {AND: "and", OR: "or", SYMDIFF: "symdiff"}
K = 27
WIDTHS = (4, 40, 65, 2049, 70001)  # nw = 1, 2 (narrow; 5-byte rows in a stride of 8), 3 (smallest wide), 65 (second round, one lane), 2188 (4-byte list ids)
ABS, BAD_TOP, BAD_N = -1, -2, -3   # members that are no set: an absent k-mer (0xFFFFFFFF), and -- colour-set form only -- the ids 0xFFFFFFFE and n_sets
N_ABSENT, N_SETS = 40, 40
LANES = 64

Plan = namedtuple("Plan", "small wave_max chunk split_waves finish_lanes grid_lanes")


def plan():
    out = (C.c_uint64 * 6)()
    assert _lib.load().bft_gpu_debug_setops_plan(out) == 0
    return Plan(*(int(x) for x in out))


# ---- the plan model ------------------------------------------------------------------------------------------------------------------------
def klass(n, P):
    return "empty" if n == 0 else "small" if n <= P.small else "wave" if n <= P.wave_max else "split"


def steps(n, P):
    """[(first, end)] of the wavefront reductions of a group of n members: one for a wave group, CHUNK members each for a split one"""
    c = klass(n, P)
    return [(0, n)] if c == "wave" else [(a, min(n, a + P.chunk)) for a in range(0, n, P.chunk)] if c == "split" else []


def loads(a, e):
    return [(i, min(e, i + LANES)) for i in range(a, e, LANES)]


def heads(mem, a, e):
    """heads of runs per 64-member load of the step mem[a:e], as the wide reduction's ballot sees them (prev: the last lane of the load before)"""
    out, prev = [], None
    for i, j in loads(a, e):
        c = mem[i:j]
        up = np.concatenate([[-9 if prev is None else prev], c[:-1]])
        out.append(int(((c >= 0) & (c != up)).sum()))
        prev = int(c[-1]) if j - i == LANES and c[-1] >= 0 else None
    return out


def rounds(nw):
    """w0 rounds of the wide reduction; 0: the narrow form (a lane per member)"""
    return 0 if nw <= 2 else (nw + LANES - 1) // LANES


def _passes(items, lanes_per_item, cap):
    if items == 0:
        return 0
    lanes = min(-(-items * lanes_per_item // 256) * 256, cap)
    return -(-items // (lanes // lanes_per_item))


def passes(P, ng, nw, rb, sizes):
    """grid passes of every kernel over a batch of ng groups of these sizes"""
    split = [n for n in sizes if klass(n, P) == "split"]
    L = 1
    while L < LANES and L < nw:
        L *= 2
    return dict(plan=_passes(ng, 1, P.grid_lanes), small=_passes(ng * nw, 1, P.grid_lanes), wave=_passes(ng, LANES, P.grid_lanes),
                split=max([-(-len(steps(n, P)) // P.split_waves) for n in split], default=0), finish=-(-len(split) * nw // P.finish_lanes),
                emit=_passes((ng * rb + 3) // 4, 1, P.grid_lanes), count=_passes(ng, L, P.grid_lanes))


# ---- families: one hand-made index per row width -----------------------------------------------------------------------------------------------
def edge_ids(G):
    """bit 0 and bit 31 of word 0, words 1 and 2, 255 | 256, words 63 | 64, words 127 | 128, 65535 | 65536, the last id -- where G has them"""
    return sorted({i for i in (0, 31, 32 + 5, 64 + 9, 255, 256, 2047, 2048, 4095, 4096, 65535, 65536, G - 1) if i < G})


class Family:
    """sets[s] = sorted genome ids; own[s, g]; cd[p] = (C, D) of the pair (a, b) = pairs[p]: C = core + {a}, D = core + {b}; kmers_of[s] = rows of
    `packed` that carry set s; absent = rows no genome holds"""

    def __init__(self, G):
        rng = np.random.default_rng(G)
        self.G, self.nw, self.rb = G, (G + 31) // 32, (G + 7) // 8
        e = self.edges = edge_ids(G)
        rest = np.setdiff1d(np.arange(G), e)
        core = set(rng.choice(rest, min(10, len(rest)), replace=False).tolist()) | ({G - 100} if G > 65536 else set())
        self.core = sorted(core)
        self.pairs = sorted(set(zip(e[:-1], e[1:])) | {(e[0], e[-1])}, key=lambda p: (p[1], p[0]))
        self.high = len(self.pairs) - 1 if G <= 2049 else next(i for i, (a, b) in enumerate(self.pairs) if a // 32 >= LANES)
        used = sorted(core | set(e))
        sets = [tuple(sorted(core | {x})) for x in e]  # (one set per edge id: the D of one pair is the C of another)
        self.cd = [(e.index(a), e.index(b)) for a, b in self.pairs]
        self.singles = (len(sets), len(sets) + 1)
        sets += [(e[0],), (e[-1],)]
        for _ in range(400):
            if len(sets) >= N_SETS:
                break
            s = tuple(g for g in used if rng.random() < 0.5)
            if s and s not in sets:
                sets.append(s)
        self.randoms = list(range(self.singles[1] + 1, len(sets)))
        self.sets, self.ids = sets, used
        self.own = np.zeros((len(sets), G), dtype=bool)
        for s, ids in enumerate(sets):
            self.own[s, list(ids)] = True
        per = self.per = 560 // len(sets)
        n = per * len(sets) + N_ABSENT
        self.packed = np.ascontiguousarray(S.distinct(S.pack_codes(rng.integers(0, 4, (n + 50, K), dtype=np.uint8)))[:n])
        assert len(self.packed) == n
        self.kmers_of = rng.permutation(per * len(sets)).reshape(len(sets), per)
        self.absent = np.arange(per * len(sets), n)

    def inserts(self):
        """[(genome id, packed k-mers)] ascending: what the index is built from"""
        return [(g, np.ascontiguousarray(self.packed[np.sort(self.kmers_of[self.own[:, g]].reshape(-1))])) for g in self.ids]

    def set_of_kmer(self):
        """{k-mer bytes: its set} of every stored k-mer (the sets are distinct: a set stands for its ownership row)"""
        return {self.packed[i].tobytes(): s for s in range(len(self.sets)) for i in self.kmers_of[s]}

    def row_of_kmer(self):
        """{k-mer bytes: ownership row bytes} of every stored k-mer"""
        return {self.packed[i].tobytes(): self.own[s].tobytes() for s in range(len(self.sets)) for i in self.kmers_of[s]}


_FAMILIES = {}


def family(G):
    if G not in _FAMILIES:
        _FAMILIES[G] = Family(G)
    return _FAMILIES[G]


# ---- batches ---------------------------------------------------------------------------------------------------------------------------------
def rle(mem):
    """a member array as runs ((set, members), ...)"""
    mem = np.asarray(mem, dtype=np.int64)
    if len(mem) == 0:
        return ()
    cut = np.concatenate([[0], np.nonzero(mem[1:] != mem[:-1])[0] + 1, [len(mem)]])
    return tuple(zip(mem[cut[:-1]].tolist(), np.diff(cut).tolist()))


def runs(*pairs):
    return tuple((int(s), int(n)) for s, n in pairs if n > 0)


def expand(g):
    return np.repeat(np.array([s for s, _ in g], dtype=np.int64), np.array([n for _, n in g], dtype=np.int64))


def size_of(g):
    return sum(n for _, n in g)


class Batch:
    """groups: run tuples, in batch order; equal groups share one pattern"""

    def __init__(self, groups):
        pats = {}
        self.which = np.array([pats.setdefault(g, len(pats)) for g in groups], dtype=np.int64)
        self.patterns = list(pats)
        self.psize = np.array([size_of(g) for g in self.patterns], dtype=np.int64)
        self.sizes = self.psize[self.which] if len(groups) else np.zeros(0, np.int64)
        self.off = np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.uint64)
        self.ng, self.n = len(groups), int(self.off[-1])

    def group(self, g):
        return self.patterns[self.which[g]]

    def members(self):
        """the set (or ABS / BAD_*) of every member, int32 [n]"""
        flat = np.concatenate([expand(g) for g in self.patterns] + [np.zeros(0, np.int64)]).astype(np.int32)
        pstart = np.concatenate([[0], np.cumsum(self.psize)])[:-1]
        first = np.asarray(self.off[:-1], dtype=np.int64)
        return flat[np.repeat(pstart[self.which] - first, self.sizes) + np.arange(self.n)]

    def kmer_rows(self, fam):
        """a row of fam.packed per member: the k-mers of a run differ, their set does not"""
        mem = self.members()
        assert (mem >= ABS).all()
        i = np.arange(self.n)
        return np.where(mem >= 0, fam.kmers_of[np.maximum(mem, 0), i % fam.per], fam.absent[i % len(fam.absent)])

    def colorsets(self, id_of_set, n_sets):
        lut = np.concatenate([[n_sets, 0xFFFFFFFE, 0xFFFFFFFF], id_of_set]).astype(np.uint32)
        return lut[self.members() + 3]


def truth_of(fam, g, op, skip):
    """(row bool [G], found) of one group"""
    sets = sorted({s for s, _ in g if s >= 0})
    e = size_of(g)
    found = sum(n for s, n in g if s >= 0)
    neff = found if skip else e
    any_ = fam.own[sets].any(axis=0) if sets else np.zeros(fam.G, bool)
    all_ = fam.own[sets].all(axis=0) if sets and neff > 0 and (skip or found == e) else np.zeros(fam.G, bool)
    return (all_ if op == AND else any_ if op == OR else any_ if neff == 1 else any_ & ~all_), found


def truth(fam, batch, op, skip):
    """(rows uint8 [ng, rb] in the library's bit layout, counts, found)"""
    per = [truth_of(fam, g, op, skip) for g in batch.patterns]
    rows = np.zeros((len(per), fam.rb), np.uint8)
    for i, (r, _) in enumerate(per):
        rows[i] = np.packbits(r, bitorder="little")
    counts = np.array([int(r.sum()) for r, _ in per] + [0], dtype=np.uint32)[:-1]
    found = np.array([f for _, f in per] + [0], dtype=np.uint32)[:-1]
    return rows[batch.which], counts[batch.which], found[batch.which]


# ---- the cases -------------------------------------------------------------------------------------------------------------------------------
def ladder(P):
    """the group sizes, by name"""
    return {"0": 0, "1": 1, "2": 2, "small-1": P.small - 1, "small": P.small, "small+1": P.small + 1, "63": 63, "64": 64, "65": 65, "128": 128,
            "chunk-1": P.chunk - 1, "chunk": P.chunk, "chunk+1": P.chunk + 1, "wave_max-1": P.wave_max - 1, "wave_max": P.wave_max,
            "wave_max+1": P.wave_max + 1, "whole_steps": P.wave_max + P.chunk, "last_step_of_one": P.wave_max + P.chunk + 1}


def positions(e, P):
    """where the lone member sits, by name"""
    out = {"0": 0, "small-1": P.small - 1, "63": 63, "64": 64, "chunk-1": P.chunk - 1, "chunk": P.chunk, "last": e - 1}
    return {k: p for k, p in out.items() if p < e}


def _fill(fam, rng, n):
    """n members drawn from the C / D sets (their AND is the core: no result is trivial).  Random order on narrow rows; on wide rows, where a
    wavefront visits the heads one after the other, short random runs up to CHUNK-sized groups of 3-word rows and a few long runs beyond"""
    pool = np.array(fam.cd).reshape(-1)
    if n <= 128 or fam.nw <= 2:
        return rle(rng.choice(pool, n))
    mean = 4 if fam.nw == 3 else max(4, n // 6)
    lens, left = [], n
    while left:
        lens.append(int(min(left, 1 + rng.integers(0, 2 * mean))))
        left -= lens[-1]
    return rle(np.repeat(rng.choice(pool, len(lens)), lens))


def sizes_batch(fam, P):
    rng = np.random.default_rng(fam.G + 1)
    lad = ladder(P)
    order = [n for k, n in lad.items() if k not in ("0", "whole_steps", "last_step_of_one")]
    groups = [()] + [_fill(fam, rng, n) for n in order] + [()] + [_fill(fam, rng, lad["whole_steps"]), _fill(fam, rng, lad["last_step_of_one"])]
    # enough split groups that the kernel which finishes them takes a second pass over (split group, word) on the widest rows
    while fam.G > 65536 and (sum(1 for g in groups if klass(size_of(g), P) == "split")) * fam.nw <= P.finish_lanes:
        groups.append(_fill(fam, rng, P.wave_max + 1))
    return Batch(groups + [()])


def lone_groups(fam, P, other):
    """[(group, pair, position name)]: every member is C of a pair but one at position p, which is D (other = "D") or absent (other = ABS).
    Small, wave (one below and one above CHUNK + 1) and split groups; and groups of 64 m members whose first and last member are both D of the
    pair in the highest words (the run head of the next round must not be mistaken for a repeat of the last member of this one)."""
    out, q = [], 0
    for e in (P.small, 130, P.chunk + 2, P.wave_max + P.chunk + 1):
        for name, p in positions(e, P).items():
            pair = q % len(fam.pairs)
            q += 1
            c, d = fam.cd[pair]
            out.append((runs((c, p), (d if other == "D" else ABS, 1), (c, e - p - 1)), pair, name))
    c, d = fam.cd[fam.high]
    for e in (LANES, 2 * LANES, P.chunk, P.wave_max + P.chunk):
        out.append((runs((d if other == "D" else ABS, 1), (c, e - 2), (d if other == "D" else ABS, 1)), fam.high, "first_and_last"))
    return out


def absent_extra(fam, P):
    """split groups: absent in exactly one whole step; all absent; exactly one found member"""
    c = fam.cd[0][0]
    e = P.wave_max + P.chunk + 1
    return [runs((c, P.chunk), (ABS, P.chunk), (c, e - 2 * P.chunk)), runs((ABS, e)), runs((ABS, 2 * P.chunk + 7), (fam.cd[-1][1], 1), (ABS, e - 2 * P.chunk - 8))]


def runs_groups(fam, P):
    c, d = fam.cd[fam.high]
    c2, d2 = fam.cd[0]
    big = P.wave_max + P.chunk
    out = {"alternating_small": rle(np.tile([c, d], P.small // 2)), "alternating_wave": rle(np.tile([c, d], 3 * LANES // 2 + 1)),
           "straddle_load": runs((c, LANES - 4), (d, 9), (c, 70)),
           "straddle_step": runs((c2, P.chunk - 3), (d2, 7), (c2, big - P.chunk - 4)),
           "straddle_second_step_and_load": runs((c, 2 * P.chunk - 1), (d, 2), (c, big - 2 * P.chunk - 1 + 1)),
           "absent_lane63_then_repeat": runs((d, LANES - 1), (ABS, 1), (d, LANES + 2)),
           "absent_lane63_then_repeat_split": runs((d2, P.chunk + LANES - 1), (ABS, 1), (d2, big - P.chunk - LANES + 1))}
    for e in (P.small, LANES, 2 * LANES, P.chunk, big):  # one set throughout, at whole loads: the only run head is the group's first member
        out[f"one_set_{e}"] = runs((d, e))
        out[f"one_set_c_{e}"] = runs((c, e))
    if fam.nw <= 3:  # (every member a head in a split group: a wavefront visits them one by one on wide rows -- kept to 3-word rows)
        out["alternating_split"] = rle(np.tile([c, d], (P.wave_max + 2) // 2))
    return out


def bad_id_groups(fam, P):
    """colour-set form: 0xFFFFFFFE and n_sets beside valid ids, in a small, a wave and a split group; and groups of nothing else"""
    c, d = fam.cd[0]
    return [runs((c, 3), (BAD_TOP, 1), (d, 2), (BAD_N, 1)), runs((BAD_N, 1), (c, 5)), runs((c, 70), (BAD_N, 1), (d, 70), (BAD_TOP, 2), (c, 9)),
            runs((c, P.chunk + 5), (BAD_TOP, 1), (c, P.wave_max), (BAD_N, 1), (d, 3)), runs((BAD_N, 2)), runs((BAD_TOP, P.small + 1)), runs((c, 4), (ABS, 1))]


def batches(fam, P):
    """{name: Batch} of one row width; "bad_ids" is for the colour-set form alone"""
    return {"sizes": sizes_batch(fam, P), "dissent": Batch([g for g, _, _ in lone_groups(fam, P, "D")]),
            "absent": Batch([g for g, _, _ in lone_groups(fam, P, ABS)] + absent_extra(fam, P)), "runs": Batch(list(runs_groups(fam, P).values())),
            "bad_ids": Batch(bad_id_groups(fam, P))}


GRID_G = 2049  # the batches of many groups: 65-word rows


def grid_groups_needed(P, fam):
    """groups for a second pass of k_so_wave (a wavefront per group), k_so_count (64 lanes per group at 65 words), k_so_emit (a lane per output
    dword) and k_so_small (a lane per (group, word))"""
    return max(P.grid_lanes // LANES, 4 * P.grid_lanes // fam.rb, P.grid_lanes // fam.nw) + 100


def grid_wave_batch(fam, P):
    rng = np.random.default_rng(7)
    pats = [runs((fam.cd[p][0], j), (fam.cd[p][1], P.small + 1 - j)) for p in range(len(fam.pairs)) for j in (0, 1, 5, P.small)]
    pats += [runs((fam.cd[0][0], 3), (ABS, 1), (fam.cd[0][0], P.small - 3))]
    return Batch([pats[i] for i in rng.integers(0, len(pats), grid_groups_needed(P, fam))])


def grid_small_batch(fam, P):
    rng = np.random.default_rng(8)
    pats = [runs((fam.cd[p][0], j), (fam.cd[p][1], n - j)) for p in range(len(fam.pairs)) for n in (1, 2, P.small) for j in (0, 1)] + [(), runs((ABS, 1))]
    return Batch([pats[i] for i in rng.integers(0, len(pats), grid_groups_needed(P, fam))])


def split_stride_batch(fam, P):
    """one group of split_waves x CHUNK + 1 members: the last step is the first of the split kernel's second pass, and holds the only D"""
    c, d = fam.cd[0]
    return Batch([runs((c, P.split_waves * P.chunk), (d, 1))])


def plan_cap_batch(fam, P):
    """more groups than k_so_plan's grid has lanes, mostly empty or of one member; split groups in the first and in the second pass"""
    rng = np.random.default_rng(9)
    c, d = fam.cd[0]
    pats = [(), (), runs((c, 1)), runs((d, 1)), runs((ABS, 1)), runs((c, 1), (d, 1))]
    groups = [pats[i] for i in rng.integers(0, len(pats), P.grid_lanes + 300)]
    big = runs((c, P.wave_max - 5), (d, 6))
    groups[7] = groups[P.grid_lanes + 11] = groups[-1] = big
    return Batch(groups)


# ---- the conditions the cases must meet ------------------------------------------------------------------------------------------------------
def _lone(g):
    """(position, what) of a group that is one set throughout but for one member: what = "D" or "absent" """
    if len(g) not in (2, 3):
        return None
    ones = [i for i, (s, n) in enumerate(g) if n == 1]
    for i in ones:
        rest = {s for j, (s, _) in enumerate(g) if j != i}
        if len(rest) == 1 and min(rest) >= 0 and g[i][0] not in rest:
            return sum(n for _, n in g[:i]), "absent" if g[i][0] < 0 else "D"
    return None


def regime_conditions(fam, P):
    """{condition: number of groups (or batches) of this width's cases that meet it}; every one must be >= 1"""
    B = batches(fam, P)
    out = {}

    def hit(name, yes=True):
        out[name] = out.get(name, 0) + bool(yes)

    lad = ladder(P)
    sz = B["sizes"]
    for name, n in lad.items():
        hit("size_" + name, (sz.sizes == n).any())
    for c in ("empty", "small", "wave", "split"):
        hit("class_" + c, any(klass(int(n), P) == c for n in sz.sizes))
    split_at = [i for i, n in enumerate(sz.sizes) if klass(int(n), P) == "split"]
    hit("empty_first_and_last", sz.sizes[0] == 0 and sz.sizes[-1] == 0)
    hit("empty_between_two_split", any(sz.sizes[i] == 0 and klass(int(sz.sizes[i - 1]), P) == klass(int(sz.sizes[i + 1]), P) == "split" for i in range(1, sz.ng - 1)))
    hit("three_split_groups_in_one_batch", len(split_at) >= 3)
    hit("whole_steps", any(n % P.chunk == 0 for n in sz.sizes[split_at]))
    hit("last_step_of_one", any(n % P.chunk == 1 for n in sz.sizes[split_at]))
    hit("step_of_exactly_chunk_in_a_wave_group", (sz.sizes == P.chunk).any())
    for g in sz.patterns:  # the carry across loads: lane 0 of a later load repeats the last member of the load before, and does not
        mem = expand(g)
        for a_, e_ in steps(size_of(g), P):
            first = np.arange(a_ + LANES, e_, LANES)
            hit("lane_0_repeats_the_load_before", (mem[first] == mem[first - 1]).any())
            hit("lane_0_is_a_head_after_another_set", (mem[first] != mem[first - 1]).any())
    for what, key in (("D", "dissent"), ("absent", "absent")):
        for c in ("small", "wave", "split"):
            for name in positions(P.wave_max + P.chunk + 1 if c == "split" else P.chunk + 2 if c == "wave" else P.small, P):
                out.setdefault(f"lone_{what}_{c}_at_{name}", 0)
        for g in B[key].patterns:
            lone = _lone(g)
            if lone is None:
                continue
            e = size_of(g)
            for name, p in positions(e, P).items():
                if p == lone[0] and lone[1] == what:
                    out[f"lone_{what}_{klass(e, P)}_at_{name}"] = out.get(f"lone_{what}_{klass(e, P)}_at_{name}", 0) + 1
        for c in ("wave", "split"):
            hit(f"{what}_first_and_last_of_whole_loads_{c}", any(
                klass(size_of(g), P) == c and size_of(g) % LANES == 0 and len(g) == 3 and g[0] == g[2] and g[0][1] == 1 and (g[0][0] < 0) == (what == "absent")
                for g in B[key].patterns))
    a, b = fam.pairs[fam.high]
    hit("high_pair_reaches_past_the_first_round", fam.nw <= LANES or max(a, b) // 32 >= LANES)
    ab = B["absent"].patterns
    hit("split_absent_in_one_whole_step", any(klass(size_of(g), P) == "split" and any(s < 0 and n == P.chunk and sum(m for _, m in g[:i]) % P.chunk == 0
                                                                                          for i, (s, n) in enumerate(g)) for g in ab))
    hit("split_all_absent", any(klass(size_of(g), P) == "split" and all(s < 0 for s, _ in g) for g in ab))
    hit("split_one_found", any(klass(size_of(g), P) == "split" and sum(n for s, n in g if s >= 0) == 1 for g in ab))
    R = runs_groups(fam, P)
    for name, g in R.items():
        e, mem = size_of(g), expand(g)
        st = steps(e, P)
        h = [x for a_, e_ in st for x in heads(mem, a_, e_)]
        if name.startswith("alternating") and st:
            hit("every_member_a_head_" + klass(e, P), all(x == min(LANES, e) or x == e % LANES for x in h) and sum(h) == e)
        if name.startswith("one_set") and st:
            hit("one_head_whole_loads_" + klass(e, P), e % LANES == 0 and sum(h) == len(st))
        if name.startswith("straddle"):
            for i, (s, n) in enumerate(g[1:-1], 1):
                q = sum(m for _, m in g[:i])
                hit("short_run_straddles_a_load", n < LANES and q % LANES + n > LANES)
                hit("short_run_straddles_a_step", klass(e, P) == "split" and q // P.chunk != (q + n - 1) // P.chunk)
        if name.startswith("absent_lane63"):
            q = g[0][1]
            hit("absent_at_lane_63_then_repeat_" + klass(e, P), g[1] == (ABS, 1) and g[0][0] == g[2][0] and (q % P.chunk if klass(e, P) == "split" else q) % LANES == LANES - 1)
    bad = B["bad_ids"].patterns
    for c in ("small", "wave", "split"):
        hit("bad_ids_beside_valid_" + c, any(klass(size_of(g), P) == c and {BAD_TOP, BAD_N} <= {s for s, _ in g} and any(s >= 0 for s, _ in g) for g in bad))
    return out


def global_conditions(P):
    out = {}
    for G in WIDTHS:
        fam = family(G)
        out[f"rounds_{rounds(fam.nw)}"] = out.get(f"rounds_{rounds(fam.nw)}", 0) + 1
        w = 1 if max(fam.ids) < 256 else 2 if max(fam.ids) < 65536 else 4
        out[f"list_ids_of_{w}_bytes"] = out.get(f"list_ids_of_{w}_bytes", 0) + 1
    out["second_round_with_one_active_lane"] = sum(family(G).nw % LANES == 1 and family(G).nw > LANES for G in WIDTHS)
    out["last_word_partial_on_wide_rows"] = sum(G % 32 != 0 and family(G).nw > 2 for G in WIDTHS)
    out["row_bytes_inside_a_wider_stride"] = sum(family(G).rb % 4 == 1 and family(G).nw == 2 for G in WIDTHS)
    fam = family(GRID_G)
    for name, b, kernels in (("grid_wave", grid_wave_batch(fam, P), ("wave", "count", "emit")), ("grid_small", grid_small_batch(fam, P), ("small",))):
        ps = passes(P, b.ng, fam.nw, fam.rb, b.sizes.tolist())
        for k in kernels:
            out[f"second_pass_{k}"] = int(ps[k] >= 2)
    out["grid_wave_groups_are_wave_class"] = int(all(klass(int(n), P) == "wave" for n in grid_wave_batch(fam, P).sizes))
    out["grid_small_groups_are_small_or_empty"] = int(all(klass(int(n), P) in ("small", "empty") for n in grid_small_batch(fam, P).sizes))
    f4 = family(WIDTHS[0])
    b = split_stride_batch(f4, P)
    out["second_pass_split"] = int(passes(P, b.ng, f4.nw, f4.rb, b.sizes.tolist())["split"] >= 2)
    b = plan_cap_batch(f4, P)
    out["second_pass_plan"] = int(passes(P, b.ng, f4.nw, f4.rb, b.sizes.tolist())["plan"] >= 2)
    out["split_group_in_plans_second_pass"] = int(any(klass(int(n), P) == "split" for n in b.sizes[P.grid_lanes:]))
    out["split_group_in_plans_first_pass"] = int(any(klass(int(n), P) == "split" for n in b.sizes[:P.grid_lanes]))
    fw = family(WIDTHS[-1])
    b = sizes_batch(fw, P)
    out["second_pass_finish"] = int(passes(P, b.ng, fw.nw, fw.rb, b.sizes.tolist())["finish"] >= 2)
    return out


# ---- tests (no GPU) --------------------------------------------------------------------------------------------------------------------------
def test_plan_call_hands_out_the_constants():
    P = plan()
    assert 1 < P.small < LANES < P.chunk < P.wave_max and P.chunk % LANES == 0 and P.wave_max % P.chunk == 0
    assert P.split_waves >= 1 and P.finish_lanes % 256 == 0 and P.grid_lanes % 256 == 0 and P.finish_lanes < P.grid_lanes
    assert _lib.load().bft_gpu_debug_setops_plan(None) == -1
    # the model at the class bounds
    assert [klass(n, P) for n in (0, 1, P.small, P.small + 1, P.wave_max, P.wave_max + 1)] == ["empty", "small", "small", "wave", "wave", "split"]
    assert steps(P.wave_max + P.chunk + 1, P)[-1] == (P.wave_max + P.chunk, P.wave_max + P.chunk + 1) and len(steps(P.wave_max + P.chunk, P)) == P.wave_max // P.chunk + 1
    assert steps(P.chunk, P) == [(0, P.chunk)] and steps(P.small, P) == []
    assert loads(3, 3 + LANES + 1) == [(3, 3 + LANES), (3 + LANES, 3 + LANES + 1)]
    assert heads(np.array([5] * 64 + [5, 5, -1, 5]), 0, 68) == [1, 1] and heads(np.array([5] * 63 + [-1] + [5, 6]), 0, 66) == [1, 2]
    assert [rounds(nw) for nw in (1, 2, 3, 64, 65, 2188)] == [0, 0, 1, 1, 2, 35]


@pytest.mark.parametrize("G", WIDTHS)
def test_family_is_what_the_table_says(G):
    fam = family(G)
    assert fam.nw == {4: 1, 40: 2, 65: 3, 2049: 65, 70001: 2188}[G] and fam.rb == {4: 1, 40: 5, 65: 9, 2049: 257, 70001: 8751}[G]
    assert max(fam.ids) == G - 1 and len(fam.ids) <= 30 and (G <= 40 or len(fam.ids) < G // 2)  # sparse ids; the genome count is max id + 1
    assert len(set(fam.sets)) == len(fam.sets) and all(s == tuple(sorted(set(s))) and s for s in fam.sets)
    assert len(fam.sets) == (N_SETS if G > 4 else 15) and 590 <= len(fam.packed) <= 640 or G == 4 and len(fam.packed) == 15 * 37 + N_ABSENT
    assert len(S.distinct(fam.packed)) == len(fam.packed) and len(fam.absent) == N_ABSENT
    e = set(fam.edges)
    assert {0, G - 1} <= e and (G <= 31 or {31, 37} <= e) and (G <= 2048 or {73, 255, 256, 2047, 2048} <= e) and (G <= 65536 or {4095, 4096, 65535, 65536} <= e)
    assert fam.core and not (set(fam.core) & e)
    for (a, b), (c, d) in zip(fam.pairs, fam.cd):
        C_, D_ = set(fam.sets[c]), set(fam.sets[d])
        assert a != b and D_ == (C_ - {a}) | {b} and C_ & D_ == set(fam.core) and C_ ^ D_ == {a, b}
    assert not (set(fam.sets[fam.singles[0]]) & set(fam.sets[fam.singles[1]])) and len(fam.randoms) >= 5
    a, b = fam.pairs[fam.high]
    assert max(a, b) // 32 == fam.nw - 1 or min(a, b) // 32 >= LANES
    # the insert calls carry exactly the ownership matrix
    back = {}
    for g, part in fam.inserts():
        for row in part:
            back.setdefault(row.tobytes(), set()).add(g)
    want = fam.row_of_kmer()
    assert set(back) == set(want) and len(want) == fam.per * len(fam.sets)
    for key, ids in back.items():
        assert np.flatnonzero(np.frombuffer(want[key], dtype=bool)).tolist() == sorted(ids)


@pytest.mark.parametrize("G", WIDTHS)
def test_cases_reach_every_regime(G):
    P = plan()
    table = regime_conditions(family(G), P)
    assert len(table) > 50
    for name, n in table.items():
        assert n >= 1, name


def test_widths_and_big_batches_reach_every_regime():
    P = plan()
    table = global_conditions(P)
    assert {f"rounds_{r}" for r in (0, 1, 2, 35)} <= set(table) and {f"list_ids_of_{w}_bytes" for w in (1, 2, 4)} <= set(table)
    assert {f"second_pass_{k}" for k in ("plan", "small", "wave", "split", "finish", "emit", "count")} <= set(table)
    for name, n in table.items():
        assert n >= 1, name
    b = split_stride_batch(family(4), P)
    assert b.n == P.split_waves * P.chunk + 1 and b.n * 4 < 40 << 20
    assert abs(grid_groups_needed(P, family(GRID_G)) - P.grid_lanes // LANES) < 300


@pytest.mark.parametrize("G", WIDTHS)
def test_truth_of_the_lone_member_cases(G):
    """AND = C & D, OR = C | D, SYMDIFF = {a, b}, none of them trivial; an absent member empties the AND unless it is skipped"""
    P = plan()
    fam = family(G)
    for g, pair, name in lone_groups(fam, P, "D"):
        a, b = fam.pairs[pair]
        r = [np.flatnonzero(truth_of(fam, g, op, 0)[0]).tolist() for op in (AND, OR, SYMDIFF)]
        assert r[0] == fam.core and r[1] == sorted(set(fam.core) | {a, b}) and r[2] == sorted((a, b)), (name, pair)
        assert 0 < len(r[0]) < len(r[1]) and truth_of(fam, g, AND, 0)[1] == size_of(g)
    for g, pair, name in lone_groups(fam, P, ABS):
        e, nabs = size_of(g), sum(n for s, n in g if s < 0)
        c = sorted(fam.sets[fam.cd[pair][0]])
        for op, skip, want in ((AND, 1, c), (AND, 0, []), (OR, 0, c), (OR, 1, c), (SYMDIFF, 0, c), (SYMDIFF, 1, c if e - nabs == 1 else [])):
            row, found = truth_of(fam, g, op, skip)
            assert np.flatnonzero(row).tolist() == want and found == e - nabs, (name, op, skip)
    one_step, nothing, one = absent_extra(fam, P)
    assert not any(truth_of(fam, nothing, op, skip)[0].any() or truth_of(fam, nothing, op, skip)[1] for op in OPS for skip in (0, 1))
    assert truth_of(fam, one, SYMDIFF, 1)[0].any() and truth_of(fam, one, AND, 1)[0].any() and truth_of(fam, one, AND, 1)[1] == 1
    assert truth_of(fam, one_step, AND, 1)[0].any() and not truth_of(fam, one_step, AND, 0)[0].any() and truth_of(fam, one_step, AND, 0)[1] == size_of(one_step) - P.chunk


def test_batches_expand_to_their_runs():
    P = plan()
    fam = family(40)
    b = batches(fam, P)["runs"]
    mem = b.members()
    assert len(mem) == b.n == int(b.off[-1])
    for g in (0, 3, b.ng - 1):
        assert (mem[int(b.off[g]):int(b.off[g + 1])] == expand(b.group(g))).all() and rle(expand(b.group(g))) == b.group(g)
    rows = b.kmer_rows(fam)
    stored = mem >= 0
    assert (fam.kmers_of[mem[stored]] == rows[stored][:, None]).any(axis=1).all() and np.isin(rows[~stored], fam.absent).all()
    assert len(np.unique(rows[:fam.per])) > 1  # the k-mers of a run differ
    cs = batches(fam, P)["bad_ids"].colorsets(np.arange(100, 100 + len(fam.sets)), 777)
    assert {0xFFFFFFFF, 0xFFFFFFFE, 777} <= set(cs.tolist()) and cs.dtype == np.uint32
    rows_, counts, found = truth(fam, b, OR, 0)
    assert rows_.shape == (b.ng, fam.rb) and (counts == np.unpackbits(rows_, axis=1).sum(axis=1)).all() and (found <= b.sizes).all()
