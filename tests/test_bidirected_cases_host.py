"""The cases of the bidirected edge tests (tests/test_gpu_bidirected_edges.py runs them on the GPU), their ground truth, and -- here, without a
GPU -- the proof that each case reaches the regime it is named after.

Truth: test_unitigs_host.Model and test_cgraph_host.Graph, unchanged -- the definition of include/bft_gpu.h over {k-mer string: genome set} and the
row order, nothing of the library's.  Model.invariants and Graph.invariants hold on every case at every threshold it is run at.  The one index that
is too large for dicts (every canonical 10-mer) has a numpy restatement over integer keys (VectorTruth: rows in the order of the T-form key, the
successors of every vertex by searchsorted, the four words counted once each); test_dict_and_vector_truths_agree holds it against Model.succ.

What the kernels derive from k -- W, the bits of word 0 (tb), the bucket bits (sb), sp_top's branch, R = k % 9, dn = 64 W - 2k of bft_x_revcomp --
is restated from csrc/bft_succ.h (shape_of), and the two searches of every oriented vertex (the interval of the four successor words from ONE
lower bound, bft_for_each_successor_of; the bucketed exact lookup of each reverse complement the interval did not hold, bft_find_row) are restated
over the rows' T-form keys (probe): which rows each search hits, where its lower bound lands, which bucket it reads.  probe() is held against
Model.succ on every case it is used on.  Each regime below is a counter of such a restatement that a test requires to be non-zero; a generator
that cannot reach its regime raises.

Sizes: no index but the dense one has more than about 4e3 rows; the dense one has (4^10 + 4^5) / 2 = 524 800."""
import collections
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_cgraph_host as G  # noqa: E402
import test_graph_cases_host as GC  # noqa: E402  (the constants of the row model's edge cases: KEY_SHAPES, CUT_KS, CYCLE_PS, SHARED_TS, ID_LABELLINGS)
import test_prefix_cases_host as P  # noqa: E402
import test_unitigs_host as H  # noqa: E402

from bloomfiltertrie_amd import synth as S  # noqa: E402

KEY_SHAPES = GC.KEY_SHAPES
KEY_SHAPE_LENGTH = 1500
DECIDE_KS = (33, 64, 72, 96, 97, 126)
PAL_KS = (10, 18, 42, 72, 96, 126)
HAIRPIN_KS = (13, 33, 63, 65, 97, 117)
LATE_KS = (72, 97, 126)
ENDS_KS = (10, 27, 42, 72, 126)
# table -> the counter of probe() that names its situation
ENDS_TABLES = {
    "above": "interval from row n",
    "last by the interval": "only successor is the last row, by the interval",
    "last by the lookup": "only successor is the last row, by the lookup",
    "first by the interval": "only successor is row 0, by the interval",
    "first by the lookup": "only successor is row 0, by the lookup",
    "empty bucket": "lookup in an empty bucket behind the last row's",
}
ID_K = 27
ID_KINDS = ("hand", "width")
ID_LABELLINGS = GC.ID_LABELLINGS
SHARED_TS = GC.SHARED_TS
SHARED_K, SHARED_G = 27, 40
SHARED_KINDS = ("interleaved", "nested", "disjoint then equal", "equal then disjoint")
CUT_KS = GC.CUT_KS
CUT_CYCLE, CUT_CHAIN, CUT_GAP, CUT_RUN = 40, 30, 7, (12, 15)  # rows of the cycle and the chain; the cycle's row of genome 0 only; the chain's rows of {1, 2}
CYCLE_PS = GC.CYCLE_PS
CYCLE_KS = (27, 72)
CYCLE_CHAINS = (5, 18, 1)
DENSE_K = 10
DENSE_ROWS = (4 ** 10 + 4 ** 5) // 2
GRID_CAP = 2048 * 256  # (bft_grid_for: 2048 workgroups of 256 lanes)

_CODE = {"A": 0, "C": 1, "G": 2, "T": 3}
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
rc, canon = H.rc, H.canon


# ---- what the kernels derive from k (csrc/bft_succ.h) ------------------------------------------------------------------------------------------------
def shape_of(k):
    """test_graph_cases_host.shape_of, and dn: the shift of bft_x_revcomp (0: its words are taken as they are)"""
    s = dict(GC.shape_of(k))
    s["dn"] = 64 * s["W"] - 2 * k
    return s


@functools.lru_cache(maxsize=None)
def _order(k):
    return tuple(P.t_order(k).tolist())


def tkey(s):
    """the T-form key of a k-mer string, as a Python integer"""
    v = 0
    for j in _order(len(s)):
        v = (v << 2) | _CODE[s[j]]
    return v


def bucket(s):
    """sp_top of the k-mer's T-form: its top sb bits"""
    k = len(s)
    return tkey(s) >> (2 * k - shape_of(k)["sb"])


def probe(m):
    """The two searches of every oriented vertex of Model m, restated over the T-form keys of its rows.  A Counter of what they meet."""
    n, keys = len(m.rows), [tkey(s) for s in m.rows]
    assert all(a < b for a, b in zip(keys, keys[1:]))  # (the rows are in the order of their keys)
    occupied = {bucket(s) for s in m.rows}
    last_bucket = bucket(m.rows[-1])
    c = collections.Counter()
    for v in range(2 * n):
        w = m.words[v]
        if tkey(w[1:] + "A") > keys[-1]:
            c["interval from row n"] += 1  # (the lower bound of the word with nucleotide 0 last: every stored T-form is below it)
        hits = []
        for ch in "ACGT":
            y = w[1:] + ch
            if y in m.row:
                hits.append(("interval", 2 * m.row[y]))
                continue
            z = rc(y)
            b = bucket(z)
            if b == last_bucket:
                c["lookup in the last bucket"] += 1
            if b not in occupied:
                c["lookup in an empty bucket"] += 1
                if b > last_bucket:
                    c["lookup in an empty bucket behind the last row's"] += 1
            if z in m.row:
                hits.append(("lookup", 2 * m.row[z] + 1))
        assert [u for _, u in hits] == m.succ[v]  # the restatement is the model's adjacency
        for how, u in hits:
            c[how] += 1
            c[f"{how} hits row 0"] += (u >> 1) == 0
            c[f"{how} hits the last row"] += (u >> 1) == n - 1
        if len(hits) == 1:
            how, u = hits[0]
            if u >> 1 == n - 1:
                c[f"only successor is the last row, by the {how}"] += 1
            if u >> 1 == 0:
                c[f"only successor is row 0, by the {how}"] += 1
    return c


# ---- a case: a model, the genome ids of its slots, its graphs -----------------------------------------------------------------------------------
class Case:
    """Model m over genome slots 0 .. slots - 1; labels[s] is the genome id slot s is inserted under (the model works on slots)."""

    def __init__(self, m, labels=None, **facts):
        self.m, self.k = m, m.k
        self.slots = max(g for s in m.owners.values() for g in s) + 1
        self.labels = tuple(labels) if labels is not None else tuple(range(self.slots))
        assert len(self.labels) == self.slots and list(self.labels) == sorted(set(self.labels))
        self.thresholds = (0, 1, 2, self.slots, self.slots + 1)
        self._graphs = m.__dict__.setdefault("_graphs", {})  # (one truth per model, whatever its slots are labelled)
        self.__dict__.update(facts)

    def inserts(self):
        """[(genome id, packed k-mers)]: what each slot holds, in row order"""
        out = []
        for s, gid in enumerate(self.labels):
            mine = [x for x in self.m.rows if s in self.m.owners[x]]
            if mine:
                out.append((gid, S.ascii_to_packed(mine, self.k)[0]))
        return out

    def graph(self, t):
        if t not in self._graphs:
            self._graphs[t] = G.Graph(self.m, t)
        return self._graphs[t]

    def colour_rows(self, t, op):
        """(rows: uint8 [segments, ceil(genomes / 8)], counts) of unitig_colors: bit labels[s] of a row for every slot s of the model's set"""
        sets = self.graph(t).colour_sets(op)
        rows = np.zeros((len(sets), (self.labels[-1] + 1 + 7) // 8), dtype=np.uint8)
        for i, x in enumerate(sets):
            for s in x:
                rows[i, self.labels[s] >> 3] |= 1 << (self.labels[s] & 7)
        return rows, np.array([len(x) for x in sets], dtype=np.uint32)

    def check(self, thresholds=None):
        """the invariants of both models at every threshold the case is run at"""
        for t in thresholds if thresholds is not None else self.thresholds:
            self.m.invariants(t)
            self.graph(t).invariants()


def _rand(rng, n):
    return "".join(rng.choice(list("ACGT"), n)) if n > 0 else ""


def _windows(q, k):
    return [q[i:i + k] for i in range(len(q) - k + 1)]


# ---- key shapes --------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def key_shape(k):
    """four related genomes of 1500 letters (test_unitigs_host.width_case's recipe) at a key shape of the row model's edge suite"""
    _, m = H.width_case(k, KEY_SHAPE_LENGTH)
    return Case(m)


# ---- the deciding nucleotide -------------------------------------------------------------------------------------------------------------------
def first_difference(x):
    """the first position at which x and rc(x) differ; None for a palindrome"""
    r = rc(x)
    return next((i for i in range(len(x)) if x[i] != r[i]), None)


def decide_ps(k):
    return tuple(sorted({p for p in (0, 31, 32, k // 2 - 1) if p < k / 2}))


def deciding_kmer(rng, k, p, smaller):
    """x with x[i] == rc(x)[i] below p and x[p] < rc(x)[p] (smaller) or > (not): x[k - 1 - i] = comp(x[i]) below p, a forced difference at p"""
    x = list(_rand(rng, k))
    for i in range(p):
        x[k - 1 - i] = _COMP[x[i]]
    x[p], x[k - 1 - p] = ("A" if smaller else "T"), "G"  # rc(x)[p] = comp(G) = C
    x = "".join(x)
    if first_difference(x) != p or (x < rc(x)) != smaller:
        raise AssertionError((k, p, smaller))
    return x


@functools.lru_cache(maxsize=None)
def deciding(k):
    """per p of decide_ps(k) and per outcome one k-mer decided at p, 40 random letters on either side; the smaller read strands in genome 0"""
    rng = np.random.default_rng(30000 + k)
    pairs, genomes = [], [[], []]
    for p in decide_ps(k):
        for smaller in (True, False):
            x = deciding_kmer(rng, k, p, smaller)
            pairs.append((x, p, smaller))
            genomes[0 if smaller else 1].append(_rand(rng, 40) + x + _rand(rng, 40))
    return Case(H.Model(H.owners_of(genomes, k), k), pairs=pairs)


# ---- palindromes and hairpins -------------------------------------------------------------------------------------------------------------------
def situation_problems(case):
    """what the hand-made situations of `case` do not show (empty: every one is there, isolated)"""
    m, k, parts, out = case.m, case.k, case.parts, []
    got, deg = m.unitigs(0), m.degrees()
    g = case.graph(0)
    where = {s: i for i, s in enumerate(g.seqs)}
    if k % 2 == 0:
        pal1, pal2 = parts["palindrome, one neighbour word"][1:-1], parts["palindrome between two neighbours"][1:-1]
        if not (pal1 == rc(pal1) and pal1 in got and deg[m.row[pal1]] == 0x11):
            out.append("palindrome with one neighbour word: a path of its own, degrees 0x11")
        if not (pal2 == rc(pal2) and not any(pal2 in s for s in got) and deg[m.row[pal2]] == 0x22):
            out.append("palindrome between two neighbours: in no path, degrees 0x22")
        i = where.get(pal2)
        if i is None or not (g.is_single[i] and g.palindromic(i) and len(g.links[2 * i]) == 2 and g.links[2 * i] == g.links[2 * i + 1]):
            out.append("palindrome between two neighbours: a single segment, the same two links from both orientations")
        q = parts["palindromic successor"]
        x = q[-k - 1:-1]
        v = 2 * m.row[canon(x)] + (canon(x) != x)
        if not (q[-k:] == rc(q[-k:]) and len(m.succ[v]) == 1 and m.words[m.succ[v][0]] == q[-k:] and m.succ[v][0] & 1 == 0):
            out.append("palindromic successor: counted once, as its even vertex")
    else:
        q = parts["hairpin"]
        x = q[-k - 1:-1]
        v = 2 * m.row[canon(x)] + (canon(x) != x)
        if not (rc(x) == q[-k:] and m.succ[v] == [v ^ 1] and not any(x + "G" in s or rc(x + "G") in s for s in got)):
            out.append("hairpin: x -> rc(x), never joined")
        a = [a for a in range(2 * len(g.segs)) if g.end(a) == v]
        if not (len(a) == 1 and g.links[a[0]] == [a[0] ^ 1]):
            out.append("hairpin: S+ -> S-")
    if len([s for s in got if len(s) >= 30 + k - 1]) != 1:
        out.append("the chain of 30 k-mers beside them: one unitig")
    return out


@functools.lru_cache(maxsize=None)
def situations(k):
    """the three palindrome situations of test_unitigs_host.hand_parts (even k) or its hairpin (odd k), each alone in the index beside one chain of
    30 k-mers.  Drawn again until they are isolated (at k = 10 two random 10-mers may touch)."""
    for attempt in range(50):
        rng = np.random.default_rng(31000 + 100 * k + 100000 * attempt)
        parts = {}
        if k % 2 == 0:
            for name, left, right in (("palindrome, one neighbour word", "G", "C"), ("palindrome between two neighbours", "G", "G")):
                half = _rand(rng, k // 2)
                parts[name] = left + half + rc(half) + right
            half = _rand(rng, k // 2)
            parts["palindromic successor"] = _rand(rng, 3) + "A" + half + rc(half)
        else:
            half = _rand(rng, (k - 1) // 2)
            parts["hairpin"] = _rand(rng, 4) + "C" + half + rc(half) + "G"
        parts["chain"] = _rand(rng, 30 + k - 1)
        names = list(parts)
        genomes = [[parts[n] for n in names[0::2]], [parts[n] for n in names[1::2]]]
        case = Case(H.Model(H.owners_of(genomes, k), k), parts=parts)
        if not situation_problems(case):
            return case
    raise AssertionError(("situations", k))


# ---- not canonical, decided late ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def late_noncanonical(k):
    """an index through insert_kmers: the smaller strands of every window of a few sequences, but of the k-mers decided at p = 32, k // 2 - 1 (late)
    and 0, 31 (early) the LARGER strand"""
    rng = np.random.default_rng(33000 + k)
    kmers, swapped = set(), []
    for p in (32, k // 2 - 1, 0, 31, 32, k // 2 - 1):
        x = deciding_kmer(rng, k, p, False)  # x > rc(x)
        q = _rand(rng, 40) + x + _rand(rng, 40)
        kmers |= {canon(w) for w in _windows(q, k)} - {rc(x)}
        kmers.add(x)
        swapped.append((x, p))
    kmers |= {canon(w) for w in _windows(_rand(rng, 200 + k), k)}
    return Case(H.Model({s: {0} for s in kmers}, k), swapped=swapped)


# ---- the ends of the table ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ends(k, table):
    """a small index (a chain of 60 k-mers, 20 loose ones, two genomes) with one k-mer added whose successor search meets the end of the table that
    ENDS_TABLES names; the counter of probe() proves it"""
    want = ENDS_TABLES[table]
    for attempt in range(200):
        rng = np.random.default_rng(32000 + 7919 * list(ENDS_TABLES).index(table) + 13 * k + 100000 * attempt)
        base = {canon(w) for w in _windows(_rand(rng, 60 + k - 1), k)} | {canon(_rand(rng, k)) for _ in range(20)}
        rows = H.rows_of(base, k)
        if table == "above":
            w = _rand(rng, 1) + "T" * 9 + _rand(rng, k - 10)  # its successor words' T-forms start with T's
        elif table == "empty bucket":
            w = _rand(rng, k - 8) + "A" * 8  # the reverse complements of its successor words: comp(N) then T's
        else:
            y = rows[-1] if table.startswith("last") else rows[0]
            w = _rand(rng, 1) + (y if table.endswith("interval") else rc(y))[:-1]
        owners = {s: ({0}, {1}, {0, 1})[int(rng.integers(0, 3))] for s in sorted(base | {canon(w)})}
        case = Case(H.Model(owners, k), added=canon(w))
        if case.slots == 2 and probe(case.m)[want] > 0:
            return case
    raise AssertionError(("ends", k, table))


# ---- dictionary ids of 1, 2 and 4 bytes -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def id_model(kind):
    """three genome slots at k = 27: the hand-made case of test_unitigs_host (its second genome's sequences also, every other one, in a third), or
    the first three related genomes of the key-width recipe"""
    k = ID_K
    if kind == "hand":
        genomes, _ = H.hand_case(k)
        circle, chain = genomes[0][:2]
        assert len(circle) == 150 + k - 1 and len(chain) > 3000
        genomes = [genomes[0], genomes[1] + [circle], [circle, chain] + genomes[1][0::2]]  # (the circle in all three, the chain and half of the situations in two)
    else:
        genomes = H.related_genomes(1000 + k, KEY_SHAPE_LENGTH)[:3]
    return H.Model(H.owners_of(genomes, k), k)


@functools.lru_cache(maxsize=None)
def id_width(kind, labels):
    return Case(id_model(kind), labels)


def id_bytes(labels):
    """bytes per dictionary id: by the largest genome id"""
    g = labels[-1] + 1
    return 1 if g <= 256 else 2 if g <= 65536 else 4


# ---- shared-set thresholds over 40 genomes --------------------------------------------------------------------------------------------------------
def shared_trace(a, b, t):
    """sp_shared (csrc/bft_succ.h) over two sorted id lists, restated: (answer, how it ended: "trivial" / "early" -- the got + min(...) < t exit --
    / "hit" / "end", tight: at some test got + min(...) was exactly t, so the answer hangs on every remaining id)"""
    if t == 0 or a == b:
        return True, "trivial", False
    i = j = got = 0
    tight = False
    while i < len(a) and j < len(b):
        rem = min(len(a) - i, len(b) - j)
        if got + rem < t:
            return False, "early", tight
        tight = tight or got + rem == t
        if a[i] == b[j]:
            got += 1
            if got >= t:
                return True, "hit", tight
            i += 1
            j += 1
        elif a[i] < b[j]:
            i += 1
        else:
            j += 1
    return got >= t, "end", tight


def _shared_sets(rng, o, kind, swap):
    """two sorted id lists over 0 .. 39 that share exactly o ids; None where the kind has none"""
    g = SHARED_G
    if kind == "nested":
        if o == 0:
            return None
        nb = g if not swap else int(rng.integers(o + 1, g + 1))
        b = sorted(rng.choice(g, nb, replace=False).tolist())
        a = sorted(rng.choice(b, o, replace=False).tolist())
    elif kind in ("disjoint then equal", "equal then disjoint"):
        ea, eb = int(rng.integers(1, (g - o) // 2 + 1)), int(rng.integers(1, (g - o) // 2 + 1))
        if kind == "equal then disjoint":
            ea = eb = 1  # (both lists end on an id of their own: the merge runs to the end)
        ids = list(range(g))
        if kind == "disjoint then equal":
            own, common = ids[:ea + eb], ids[g - o:] if o else []
        else:
            common, own = ids[:o], ids[g - ea - eb:]
        a = sorted(common + own[:ea])
        b = sorted(common + own[ea:ea + eb])
    else:
        ea, eb = int(rng.integers(1, (g - o) // 2 + 1)), int(rng.integers(1, (g - o) // 2 + 1))
        ids = sorted(rng.choice(g, o + ea + eb, replace=False).tolist())
        roles = ["c"] * o + ["a"] * ea + ["b"] * eb
        roles = [roles[i] for i in rng.permutation(len(roles))]
        a = [x for x, r in zip(ids, roles) if r in "ca"]
        b = [x for x, r in zip(ids, roles) if r in "cb"]
    if swap:
        a, b = b, a
    assert len(set(a) & set(b)) == o and a and b
    return a, b


@functools.lru_cache(maxsize=None)
def shared():
    """40 genomes at k = 27.  Per t of SHARED_TS, per overlap t - 1, t, t + 1, per kind and order of the two lists: a chain u -> v of two k-mers with
    those id lists, and the same two lists across a branching k-mer (u' with the first list, its successors v' with the second and v'' with the
    first: u' is a single-k-mer segment, and its link to v' is decided by the same merge in k_cg_links)"""
    rng = np.random.default_rng(34000)
    k = SHARED_K
    owners, pairs = {}, []
    for t in SHARED_TS:
        for o in (t - 1, t, t + 1):
            for kind in SHARED_KINDS:
                for swap in (0, 1):
                    ab = _shared_sets(rng, o, kind, swap)
                    if ab is None:
                        continue
                    a, b = ab
                    s, s2 = _rand(rng, k + 1), _rand(rng, k + 1)
                    alt = s2[1:k] + next(c for c in "ACGT" if c != s2[k])
                    for x, ids in ((s[:k], a), (s[1:], b), (s2[:k], a), (s2[1:], b), (alt, a)):
                        assert canon(x) not in owners
                        owners[canon(x)] = set(ids)
                    pairs.append({"t": t, "o": o, "kind": kind, "swap": swap, "a": a, "b": b, "chain": s, "branch": s2, "alt": alt})
    case = Case(H.Model(owners, k), pairs=pairs)
    case.thresholds = SHARED_TS
    return case


# ---- threshold cuts ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cut(k):
    """a cycle of 40 rows of genomes {0, 1}, but row CUT_GAP of genome 0 only (at t = 2 the cycle is a chain); a chain of 30 rows of {0, 1, 2}, but
    the rows CUT_RUN of {1, 2} (at t = 3 it splits)"""
    for attempt in range(50):
        rng = np.random.default_rng(35000 + k + 100000 * attempt)
        circ, line = _rand(rng, CUT_CYCLE), _rand(rng, CUT_CHAIN + k - 1)
        ring = (circ * (k // CUT_CYCLE + 2))[:CUT_CYCLE + k - 1]
        owners = {}
        for i, w in enumerate(_windows(ring, k)):
            owners[canon(w)] = {0} if i == CUT_GAP else {0, 1}
        for i, w in enumerate(_windows(line, k)):
            owners[canon(w)] = {1, 2} if CUT_RUN[0] <= i < CUT_RUN[1] else {0, 1, 2}
        m = H.Model(owners, k)
        if len(m.rows) == CUT_CYCLE + CUT_CHAIN and sorted(len(p) for p in m.paths(0)) == [CUT_CHAIN, CUT_CYCLE] and len(m.all_paths(0)[3]) == 2:
            return Case(m, ring=ring, line=line)
    raise AssertionError(("cut", k))


# ---- cycles beside chains -------------------------------------------------------------------------------------------------------------------------
def _strand_of(circle, s, p):
    """which strand of the circle the unitig s reads: "read", "mirror", None (no rotation of either) or "both" """
    read, mirror = s[:p] in circle * 2, s[:p] in rc(circle) * 2
    return "both" if read and mirror else "read" if read else "mirror" if mirror else None


@functools.lru_cache(maxsize=None)
def cycles(k, p):
    """two cycles of p rows (genome 0; genomes 0 and 1) and chains of CYCLE_CHAINS rows (genome 1; 0 and 1; 0) in one index.  A seed whose circle is
    its own reverse complement, or has a shorter period, is rejected (as test_unitigs_host.whole_case does): the rows and paths would not be these"""
    for attempt in range(200):
        rng = np.random.default_rng(36000 + 300 * k + p + 100000 * attempt)
        circles = [_rand(rng, p), _rand(rng, p)]
        lines = [_rand(rng, n + k - 1) for n in CYCLE_CHAINS]
        rings = [(q * (k // p + 2))[:p + k - 1] for q in circles]
        genomes = [[rings[0], rings[1], lines[1], lines[2]], [rings[1], lines[0], lines[1]]]
        m = H.Model(H.owners_of(genomes, k), k)
        _, _, chains, cyc = m.all_paths(0)
        if len(m.rows) != 2 * p + sum(CYCLE_CHAINS) or sorted(len(x) for x in m.paths(0)) != sorted((p, p) + CYCLE_CHAINS):
            continue
        if (len(chains), len(cyc)) != (6, 4) and p > 1:
            continue
        # the strand each kept cycle is reported on: the kept one starts at the even vertex of its smallest row
        strands = []
        for q in circles:
            mine = [_strand_of(q, s, p) for s in m.unitigs(0) if len(s) == p + k - 1 and _strand_of(q, s, p)]
            strands.append(mine[0] if len(mine) == 1 else "both")
        if "both" in strands:
            continue
        return Case(m, circles=circles, strands=strands)
    raise AssertionError(("cycles", k, p))


# ---- the dense link grid: a numpy restatement ---------------------------------------------------------------------------------------------------
def _digits(nat, k):
    """[n, k] nucleotide codes of k-mers given as integers with the first nucleotide most significant"""
    nat = np.asarray(nat, dtype=np.uint64)
    return np.stack([((nat >> np.uint64(2 * (k - 1 - j))) & np.uint64(3)).astype(np.uint8) for j in range(k)], axis=1)


def _from_digits(d):
    v = np.zeros(len(d), dtype=np.uint64)
    for j in range(d.shape[1]):
        v = (v << np.uint64(2)) | d[:, j].astype(np.uint64)
    return v


def vec_rc(nat, k):
    return _from_digits(3 - _digits(nat, k)[:, ::-1])


def vec_tkey(nat, k):
    return _from_digits(_digits(nat, k)[:, list(_order(k))])


class VectorTruth:
    """Canonical k-mers (k <= 31) as integers: rows in the order of the T-form key; vertex 2 * row + o with word s or rc(s); succ [2n, 4]: the
    vertex that represents the word with nucleotide c last (a stored y: its even vertex; a stored rc(y): its odd one), or -1"""

    def __init__(self, nat, k):
        nat = np.unique(np.asarray(nat, dtype=np.uint64))
        key = vec_tkey(nat, k)
        order = np.argsort(key)
        self.k, self.nat, self.keys, self.n = k, nat[order], key[order], len(nat)
        self.rcnat = vec_rc(self.nat, k)
        self.noncanonical = int((self.nat > self.rcnat).sum())
        self.palindromic = self.nat == self.rcnat
        words = np.empty(2 * self.n, dtype=np.uint64)
        words[0::2], words[1::2] = self.nat, self.rcnat
        mask = np.uint64((1 << (2 * k)) - 1)
        self.succ = np.full((2 * self.n, 4), -1, dtype=np.int64)
        for c in range(4):
            y = ((words << np.uint64(2)) & mask) | np.uint64(c)
            yr = vec_rc(y, k)
            for o, word in ((0, y), (1, yr)):  # (stored as itself first: a palindromic word is its even vertex)
                wk = vec_tkey(word, k)
                pos = np.minimum(np.searchsorted(self.keys, wk), self.n - 1)
                hit = (self.keys[pos] == wk) & (self.succ[:, c] < 0)
                self.succ[hit, c] = 2 * pos[hit] + o
        self.out = (self.succ >= 0).sum(axis=1)

    def strings(self):
        return [H.text(r) for r in _digits(self.nat, self.k)]

    def packed(self):
        return S.pack_codes(_digits(self.nat, self.k))

    def degrees(self):
        return (self.out[0::2] << 4 | self.out[1::2]).astype(np.uint8)

    def all_single(self):
        """no row is a node: every row is a single-k-mer segment, segment i is row i, the last vertex of oriented segment a is vertex a and the
        oriented segment that starts with vertex w is w"""
        return bool(((self.out[0::2] > 1) | (self.out[1::2] > 1)).all())

    def graph_arrays(self):
        """(seg_off, seqs, link_off, links, members, counts) of bft_gpu_unitig_graph where all_single() holds, at t = 0 or 1 over one genome"""
        assert self.all_single() and self.noncanonical == 0
        n, k = self.n, self.k
        tg = np.sort(np.where(self.succ >= 0, self.succ, np.iinfo(np.int64).max), axis=1)
        links = tg[tg != np.iinfo(np.int64).max].astype(np.uint32)
        link_off = np.concatenate([[0], np.cumsum(self.out)]).astype(np.uint64)
        seqs = GC._ASCII[_digits(self.nat, k)].reshape(-1)
        counts = [n, n * k, k, 0, int(self.out.sum()), n]
        return np.arange(n + 1, dtype=np.uint64) * np.uint64(k), seqs, link_off, links, np.arange(0, 2 * n, 2, dtype=np.uint32), counts


@functools.lru_cache(maxsize=None)
def dense():
    """every canonical 10-mer, one genome"""
    nat = np.arange(4 ** DENSE_K, dtype=np.uint64)
    return VectorTruth(nat[nat <= vec_rc(nat, DENSE_K)], DENSE_K)


# ---- tests: the restatements --------------------------------------------------------------------------------------------------------------------
def test_key_shapes_hit_every_shape():
    ks = sorted(set(KEY_SHAPES + DECIDE_KS + PAL_KS + HAIRPIN_KS + LATE_KS + ENDS_KS + CUT_KS + CYCLE_KS + (ID_K, SHARED_K, DENSE_K)))
    for k in ks:
        s = shape_of(k)
        assert s["W"] == -(-2 * k // 64) and 0 < s["tb"] <= 64 and s["tb"] + 64 * (s["W"] - 1) == 2 * k and 0 <= s["dn"] < 64 and s["dn"] == 64 - s["tb"]
        assert s["sb"] == min(2 * k, 20) and (s["branch"] == "direct") == (s["tb"] >= s["sb"]) and s["R"] == k % 9
        assert len(_order(k)) == k and sorted(_order(k)) == list(range(k))
    new = {k: shape_of(k) for k in KEY_SHAPES}
    assert {s["W"] for s in new.values()} == {1, 2, 3, 4}
    assert {(s["W"], s["branch"]) for s in new.values()} >= {(2, "spill"), (3, "spill"), (4, "spill"), (1, "direct"), (2, "direct"), (3, "direct")}
    assert [k for k in KEY_SHAPES if new[k]["dn"] == 0] == [32, 96]  # bft_x_revcomp takes its words as they are
    assert {(s["W"], s["R"] == 0) for s in new.values()} >= {(2, False), (3, True), (3, False), (4, True), (4, False)}
    # the mirrored model was run at nine values of k, none of them here but 72
    assert set(KEY_SHAPES) & set(H.KS) == {72}
    # the palindromes, the hairpins and the deciding nucleotides: every width, both tail layouts
    for ks in (PAL_KS, HAIRPIN_KS):
        assert {shape_of(k)["W"] for k in ks} == {1, 2, 3, 4} and {shape_of(k)["R"] == 0 for k in ks} == {True, False}
    assert all(k % 2 == 0 for k in PAL_KS) and all(k % 2 == 1 for k in HAIRPIN_KS) and 9 not in PAL_KS + HAIRPIN_KS
    assert {shape_of(k)["W"] for k in DECIDE_KS} == {2, 3, 4} and {shape_of(k)["W"] for k in LATE_KS} == {3, 4}


def test_the_key_and_the_bucket_are_the_row_models():
    rng = np.random.default_rng(5)
    for k in (10, 27, 42, 72, 126):
        codes = rng.integers(0, 4, (20, k), dtype=np.uint8)
        strings = [H.text(r) for r in codes]
        assert [tkey(s) for s in strings] == P.t_key_ints(codes, k)
        assert H.rows_of(strings, k) == sorted(strings, key=tkey)
        assert all(0 <= bucket(s) < 1 << shape_of(k)["sb"] for s in strings)
    assert bucket("ACGTACGTAC") == tkey("ACGTACGTAC")  # k = 10: sb = 2k, a bucket is one key


# ---- tests: the key shapes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KEY_SHAPES)
def test_key_shape_cases(k):
    case = key_shape(k)
    case.check()
    assert case.slots == H.N_GENOMES
    assert case.thresholds == (0, 1, 2, H.N_GENOMES, H.N_GENOMES + 1)
    assert case.m.unitigs(H.N_GENOMES + 1) == [] and 0 < len(case.m.unitigs(2)) != len(case.m.unitigs(0))  # (at k = 96 no window is in all four genomes)
    assert sum(1 for s in case.m.unitigs(0) if len(s) > k) >= 2
    c = probe(case.m)
    assert c["interval"] > 0 and c["lookup"] > 0  # successors stored as themselves and as their reverse complements
    g = case.graph(0)
    assert sum(g.is_single) > 0 and g.counts()[4] > 0 and len(g.segs) > sum(g.is_single)


# ---- tests: the deciding nucleotide -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", DECIDE_KS)
def test_deciding_nucleotide_cases(k):
    case = deciding(k)
    case.check()
    m = case.m
    assert [p for _, p, _ in case.pairs] == [p for p in decide_ps(k) for _ in (0, 1)] and all(p < k / 2 for p in decide_ps(k))
    late = collections.Counter()
    for x, p, smaller in case.pairs:
        assert first_difference(x) == p == first_difference(rc(x)) and (x < rc(x)) == smaller
        assert all(x[i] == rc(x)[i] for i in range(p)) and x[p] != rc(x)[p]
        row = m.row[canon(x)]
        assert m.degrees()[row] == 0x11 and first_difference(m.rows[row]) == p  # it has a neighbour on either side; the stored strand decides at p too
        assert any(x in s or rc(x) in s for s in m.unitigs(0) if len(s) > k)
        if p >= 32:
            late[smaller] += 1
            assert x[:32] == rc(x)[:32]  # word 0 alone calls it a palindrome
            assert p // 32 >= 1 and shape_of(k)["W"] >= 3
    if shape_of(k)["W"] >= 3:
        assert late[True] >= 2 and late[False] >= 2  # p = 32 and p = k // 2 - 1, both outcomes
        assert any(p // 32 == 1 for _, p, _ in case.pairs) and (k < 126 or any(p == 62 for _, p, _ in case.pairs))
    else:
        assert not late and max(decide_ps(k)) < 32


# ---- tests: palindromes and hairpins ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", PAL_KS + HAIRPIN_KS)
def test_palindrome_and_hairpin_situations(k):
    case = situations(k)
    case.check((0, 1, 2, 3))
    assert situation_problems(case) == []
    c = probe(case.m)
    if k % 2 == 0:
        pals = [s for s in case.m.rows if s == rc(s)]
        assert len(pals) == 3 and c["interval"] > 0
        # a palindromic successor is found by the interval; the lookup of its reverse complement would find it a second time
        q = case.parts["palindromic successor"]
        assert q[-k:] in case.m.row and rc(q[-k:]) in case.m.row


# ---- tests: not canonical, decided late -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", LATE_KS)
def test_late_noncanonical_cases(k):
    case = late_noncanonical(k)
    m = case.m
    above = [s for s in m.rows if s > rc(s)]
    assert m.noncanonical == len(above) == len(case.swapped) == 6 and sorted(above) == sorted(x for x, _ in case.swapped)
    late = [s for s in above if first_difference(s) >= 32]
    early = [s for s in above if first_difference(s) < 32]
    assert len(late) == 4 and len(early) == 2 and all(s[:32] == rc(s)[:32] for s in late)
    assert sum(1 for s in m.rows if s < rc(s)) > 200 and len(m.degrees()) == len(m.rows)
    assert all(m.degrees()[m.row[x]] == 0x11 for x, _ in case.swapped)
    probe(m)


# ---- tests: the ends of the table -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("table", list(ENDS_TABLES))
@pytest.mark.parametrize("k", ENDS_KS)
def test_ends_tables_show_their_situation(k, table):
    case = ends(k, table)
    case.check()
    m = case.m
    n, keys = len(m.rows), [tkey(s) for s in m.rows]
    c = probe(m)
    assert c[ENDS_TABLES[table]] > 0
    v = [2 * m.row[case.added], 2 * m.row[case.added] + 1]
    if table == "above":
        assert any(tkey(m.words[u][1:] + "A") > keys[-1] and m.succ[u] == [] for u in v)
    elif table == "empty bucket":
        last = bucket(m.rows[-1])
        assert any(bucket(rc(m.words[u][1:] + ch)) > last for u in v for ch in "ACGT")
    else:
        r = n - 1 if table.startswith("last") else 0
        o = 0 if table.endswith("interval") else 1
        assert any(m.succ[u] == [2 * r + o] for u in range(2 * n))  # (the added k-mer's vertex, unless it became that row itself)
    assert c["lookup in an empty bucket"] > 0  # (a few dozen rows in 2^20 buckets; at k = 10 in 4^10)


def test_ends_tables_together_reach_every_end():
    for k in ENDS_KS:
        total = collections.Counter()
        for table in ENDS_TABLES:
            total.update(probe(ends(k, table).m))
        for name in list(ENDS_TABLES.values()) + ["interval hits row 0", "interval hits the last row", "lookup hits row 0", "lookup hits the last row"]:
            assert total[name] > 0, (k, name)


# ---- tests: the id widths -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ID_KINDS)
def test_id_width_labellings_are_one_graph(kind):
    assert [id_bytes(x) for x in ID_LABELLINGS] == [1, 2, 4]
    cases = [id_width(kind, labels) for labels in ID_LABELLINGS]
    assert all(c.m is cases[0].m and c.slots == 3 for c in cases)  # the model works on slots: unitigs, degrees, links and members are one truth
    cases[0].check()
    m = cases[0].m
    sizes = collections.Counter(len(x) for x in m.owners.values())
    assert sizes[1] and sizes[2] and sizes[3]
    assert len({frozenset(x) for x in m.owners.values()}) >= 4
    for t in (0, 2):
        g = cases[0].graph(t)
        assert len(g.segs) > 3 and g.counts()[4] > 0
        if t:
            assert len(m.unitigs(t)) != len(m.unitigs(0)) or m.unitigs(t) != m.unitigs(0)  # the threshold (and so the merge of two id lists) decides
        for op in ("and", "or", "symdiff"):
            slot_rows, slot_counts = cases[0].colour_rows(t, op)
            assert slot_rows.shape[1] == 1
            for c in cases[1:]:
                rows, counts = c.colour_rows(t, op)
                assert rows.shape == (len(g.segs), (c.labels[-1] + 8) // 8) and (counts == slot_counts).all()
                bits = np.unpackbits(rows, axis=1, bitorder="little")
                moved = bits[:, list(c.labels)]
                assert (moved == np.unpackbits(slot_rows, axis=1, bitorder="little")[:, :3]).all()  # the slots' rows moved to the id bits
                assert bits.sum() == moved.sum()
    assert [gid for gid, _ in cases[2].inserts()] == list(ID_LABELLINGS[2])


# ---- tests: the merge of two id lists -------------------------------------------------------------------------------------------------------------
def test_shared_set_case():
    case = shared()
    m = case.m
    assert case.slots == SHARED_G and case.thresholds == SHARED_TS
    case.check()
    lengths = {len(x) for x in m.owners.values()}
    assert min(lengths) == 1 and max(lengths) == SHARED_G and len(lengths) >= 20
    seen, how = set(), collections.Counter()
    for pr in case.pairs:
        t, a, b = pr["t"], pr["a"], pr["b"]
        common = sorted(set(a) & set(b))
        assert len(common) == pr["o"] and pr["o"] in (t - 1, t, t + 1) and a == sorted(set(a)) and b == sorted(set(b))
        own = sorted(set(a) ^ set(b))
        if pr["kind"] == "nested":
            assert set(a) <= set(b) or set(b) <= set(a)
        elif pr["kind"] == "disjoint then equal":
            assert not common or common[0] > own[-1]
        elif pr["kind"] == "equal then disjoint":
            assert not common or common[-1] < own[0]
        seen.add((pr["o"] - t, pr["kind"], pr["swap"], t))
        # the structure: u -> v is u's only successor word; u' has two
        s, s2 = pr["chain"], pr["branch"]
        k_ = SHARED_K
        u, v = s[:k_], s[1:]
        vu = 2 * m.row[canon(u)] + (canon(u) != u)
        vv = 2 * m.row[canon(v)] + (canon(v) != v)
        assert m.succ[vu] == [vv] and m.succ[vv ^ 1] == [vu ^ 1]
        assert m.owners[canon(u)] == set(a) and m.owners[canon(v)] == set(b)
        vb = 2 * m.row[canon(s2[:k_])] + (canon(s2[:k_]) != s2[:k_])
        assert len(m.succ[vb]) == 2 and m.owners[canon(s2[:k_])] == set(a) and m.owners[canon(s2[1:])] == set(b)
        # the merge, restated, at the threshold the pair was made for: both rows are nodes there (the kernels merge only then)
        if len(a) >= t and len(b) >= t and a != b:
            for x, y in ((a, b), (b, a)):
                ans, end, tight = shared_trace(x, y, t)
                assert ans == (len(common) >= t)
                how[end] += 1
                how["tight and shared"] += tight and ans
                how["fails at the end"] += end == "end" and not ans
                how[f"{end}, {pr['kind']}"] += 1
            joined = any(s in q or rc(s) in q for q in m.unitigs(t))
            assert joined == (len(common) >= t)
            g = case.graph(t)
            i = g.seqs.index(canon(s2[:k_]))
            end_a = 2 * i + (canon(s2[:k_]) != s2[:k_])
            targets = [g.spelled(b_)[:k_] for b_ in g.links[end_a]]
            assert (s2[1:] in targets) == (len(common) >= t) and pr["alt"] in targets
    assert len(seen) == len(case.pairs) == sum(1 for t in SHARED_TS for o in (t - 1, t, t + 1) for kind in SHARED_KINDS for _ in (0, 1) if o or kind != "nested")
    # the got + min(...) < t exit is taken; it is not taken by a pair that then fails at the end; an answer hangs on every remaining id
    assert how["early"] > 0 and how["fails at the end"] > 0 and how["tight and shared"] > 0 and how["hit"] > 0
    assert how["early, disjoint then equal"] > 0 and how["end, equal then disjoint"] > 0


# ---- tests: threshold cuts ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", CUT_KS)
def test_cut_cases(k):
    case = cut(k)
    case.check()
    m = case.m
    assert case.slots == 3 and len(m.rows) == CUT_CYCLE + CUT_CHAIN
    lens = lambda t: sorted(len(s) - (k - 1) for s in m.unitigs(t))  # noqa: E731
    a, b = CUT_RUN
    assert lens(0) == lens(1) == [CUT_CHAIN, CUT_CYCLE]
    assert lens(2) == [CUT_CHAIN, CUT_CYCLE - 1]  # the cycle is a chain: it ends on either side of the row of genome 0 alone
    assert lens(3) == sorted([a, CUT_CHAIN - b])  # the chain splits at the run of {1, 2}; the cycle's rows have two genomes
    assert lens(4) == []
    gap = canon(_windows(case.ring, k)[CUT_GAP])
    opened = [s for s in m.unitigs(2) if len(s) == CUT_CYCLE - 1 + k - 1][0]
    assert not any(canon(w) == gap for w in _windows(opened, k))
    ends_ = {canon(opened[:k]), canon(opened[-k:])}
    assert ends_ == {canon(_windows(case.ring, k)[CUT_GAP - 1]), canon(_windows(case.ring, k)[CUT_GAP + 1])}
    _, _, chains, cyc = m.all_paths(2)
    assert len(cyc) == 0 and len(m.all_paths(0)[3]) == 2
    assert [len(case.graph(t).segs) for t in (0, 2, 3, 4)] == [2, 2, 2, 0]


# ---- tests: cycles beside chains ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", CYCLE_KS)
@pytest.mark.parametrize("p", CYCLE_PS)
def test_cycle_cases(p, k):
    case = cycles(k, p)
    case.check((0, 1, 2, 3))
    m = case.m
    assert len(m.rows) == 2 * p + sum(CYCLE_CHAINS)
    _, _, chains, cyc = m.all_paths(0)
    assert (len(chains), len(cyc)) == (6, 4) and sorted(len(x) for x in cyc) == [p] * 4
    assert sorted(len(s) - (k - 1) for s in m.unitigs(0)) == sorted((p, p) + CYCLE_CHAINS)
    assert sorted(len(s) - (k - 1) for s in m.unitigs(2)) == sorted((p, 18)) and m.unitigs(3) == []
    for q in case.circles:
        assert rc(q) not in q * 2  # no circle is its own reverse complement
    kept = [x for x in m.paths(0) if len(x) == p and m.all_paths(0)[1].get(x[-1]) == x[0]]
    assert len(kept) == 2 and all(x[0] & 1 == 0 and x[0] >> 1 == min(v >> 1 for v in x) for x in kept)  # from the even vertex of its smallest row
    g = case.graph(0)
    loops = [i for i in range(len(g.segs)) if g.links[2 * i] == [2 * i] and g.links[2 * i + 1] == [2 * i + 1]]
    assert len(loops) == 2 and all(len(g.segs[i]) == p for i in loops)
    assert set(case.strands) <= {"read", "mirror"}


def test_cycles_are_kept_on_the_read_strand_and_on_its_mirror():
    """the smallest row of a cycle is met, reading the circle as it was inserted, as its even vertex (the cycle is reported as read) or as its odd
    one (the kept path is the mirror: the reverse complement of the circle) -- both, over the cases"""
    seen = collections.Counter()
    for k in CYCLE_KS:
        for p in CYCLE_PS:
            seen.update((k, s) for s in cycles(k, p).strands)
    for k in CYCLE_KS:
        assert seen[(k, "read")] > 0 and seen[(k, "mirror")] > 0, seen


# ---- tests: the dense link grid -------------------------------------------------------------------------------------------------------------------
def test_dense_case():
    vt = dense()
    n = vt.n
    assert n == DENSE_ROWS == 524800 and vt.noncanonical == 0 and int(vt.palindromic.sum()) == 4 ** 5 == 1024
    assert vt.all_single()  # no row is a node
    assert 2 * n == 1049600 > GRID_CAP and 2 * n > 2 * GRID_CAP  # one lane per oriented end: a second grid pass, and a third begun
    assert (np.diff(vt.keys.astype(np.int64)) > 0).all()
    # every word is stored on one strand or the other: four successor words per vertex.  Two of them never share a canonical form: w[1:] + c' =
    # rc(w[1:] + c) forces c' = c, the one palindromic word, which the interval finds and the lookup must not find again.  So every end has four
    # targets on four segments -- none has fewer -- and a kernel that counted a word in both forms would show here as a fifth
    assert (vt.out == 4).all() and (vt.degrees() == 0x44).all()
    tg = np.sort(vt.succ, axis=1)
    assert (np.diff(tg, axis=1) > 0).all()  # four distinct targets on every end
    assert (np.diff(tg >> 1, axis=1) > 0).all()  # on four segments
    pal_target = vt.palindromic[vt.succ >> 1].any(axis=1)
    assert 0 < int(pal_target.sum()) < 2 * n and (vt.succ[vt.palindromic[vt.succ >> 1]] & 1 == 0).all()  # links into a palindrome name its +
    unsorted = (np.diff(vt.succ, axis=1) < 0).any(axis=1)
    assert int(unsorted.sum()) > n // 2  # the in-register sort has work on most ends
    seg_off, seqs, link_off, links, members, counts = vt.graph_arrays()
    assert counts == [n, n * DENSE_K, DENSE_K, 0, 8 * n, n] and len(links) == 8 * n and link_off[-1] == 8 * n
    assert min(2 * counts[0], 2 * n) == 2 * n > counts[0]  # a loop bounded by the segments, not by their ends, stops half way
    # the ends of the second pass have targets in the first and the other way round
    a = np.arange(2 * n)
    assert ((a >= GRID_CAP) & (tg[:, 0] < GRID_CAP)).any() and ((a < GRID_CAP) & (tg[:, 3] >= GRID_CAP)).any()


def test_dict_and_vector_truths_agree():
    """the numpy restatement against Model on 3000 canonical 10-mers: 2000 at random, and for some of them every successor word"""
    rng = np.random.default_rng(37000)
    k = DENSE_K
    full = dense()
    pick = rng.choice(full.n, 2000, replace=False)
    nat = full.nat[pick]
    words = np.concatenate([nat[:130], full.rcnat[pick[:130]]])
    mask = np.uint64((1 << (2 * k)) - 1)
    more = np.concatenate([((words << np.uint64(2)) & mask) | np.uint64(c) for c in range(4)])
    more = np.setdiff1d(np.minimum(more, vec_rc(more, k)), nat)
    nat = np.concatenate([nat, more[:1000]])
    assert len(nat) == 3000
    vt = VectorTruth(nat, k)
    m = H.Model({s: {0} for s in vt.strings()}, k)
    assert m.rows == vt.strings() and m.noncanonical == vt.noncanonical == 0
    assert [[int(x) for x in row if x >= 0] for row in vt.succ] == m.succ
    assert vt.degrees().tobytes() == m.degrees()
    assert int((vt.out > 0).sum()) > 500 and int(vt.palindromic.sum()) == sum(1 for s in m.rows if s == rc(s))
    assert collections.Counter(vt.out.tolist())[4] > 100
    probe(m)
    # and where every row branches, the graph arrays against Graph: every 6-mer's canonical form (2080 rows)
    k = 6
    nat = np.arange(4 ** k, dtype=np.uint64)
    vt = VectorTruth(nat[nat <= vec_rc(nat, k)], k)
    m = H.Model({s: {0} for s in vt.strings()}, k)
    g = G.Graph(m, 1)
    g.invariants()
    want = g.arrays()
    got = vt.graph_arrays()
    assert all((a == b).all() and len(a) == len(b) for a, b in zip(got[:5], want)) and got[5] == g.counts()
    assert m.unitigs(0) == [] and vt.all_single()
