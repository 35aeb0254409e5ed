"""The cases of the graph edge tests (tests/test_gpu_graph_edges.py runs them on the GPU), their ground truth, and -- here, without a GPU -- the
proof that each case reaches the regime it is named after.

Truth, in numpy and Python only (nothing of the library's).  The rows of an index are its distinct k-mers in the order of their T-form digits
(t_order / t_key_ints of test_prefix_cases_host, pinned here to bft_hosttest_roundtrip for every k used), a row's colour set is the set of genomes
that inserted it, and the graph is x -> x[1:] + N over the stored k-mers.  From that alone: the simple paths of include/bft_gpu.h (a node has
in <= 1, out <= 1 and |C| >= t; an edge needs both ends nodes, v != u and |C(u) & C(v)| >= t; a cycle is cut before its smallest row; paths in the
order of their head's row), the components numbered by smallest row, reach and boundary marks (test_marking_host.MarkModel over the same k-mers),
the pan-genome classes and the contents of a sub-graph.  The adjacency comes in two forms: by a dict of the k-mers' strings (every small case) and,
for k <= 32, by uint64 keys and searchsorted (the grid case, whose rows are never spelled one by one); test_dict_and_vector_truths_agree holds
them against each other.

What the kernels compute from k alone -- W, the bits of word 0 (tb), the bucket bits (sb), which branch of sp_top runs, R = k % 9 -- is restated
here from csrc/bft_succ.h and csrc/bft_paths.h (shape_of) and the key shapes are checked against it.

Sizes: no index but the grid's has more than about 5e3 rows; the grid has 2048 * 256 + 300."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_prefix_cases_host as P  # noqa: E402
from test_marking_host import MarkModel  # noqa: E402

from bloomfiltertrie_amd import _lib  # noqa: E402  (the host test library of the pin, nothing else)

KS = (9, 18, 27, 31, 36, 63, 64, 126)  # the recipe of test_gpu_simple_paths / _components / _pangenome / _subgraph
KEY_SHAPES = (10, 13, 32, 33, 41, 42, 65, 72, 74, 81, 90, 96, 97, 105, 117)
DENSE_KS = (9, 18, 27, 45, 72, 99, 126, 13, 31, 64, 80)
ENDS_KS = (9, 10, 27, 42, 72, 126)
ENDS_TABLES = ("above", "last", "lone", "homopolymer", "two")
CYCLE_PS = (2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 255, 256, 257)
CYCLE_KS = (27, 72)
CYCLE_CHAINS = (5, 18, 1)  # k-mers of the chains that share the index with the two cycles
WHOLE_NS = (1, 2, 3, 63, 64, 65, 1023, 1024, 1025)
WHOLE_KS = (27, 72)
CUT_KS = (13, 27, 72)
CUT_CYCLE, CUT_CHAIN, CUT_GAP, CUT_ODD = 40, 30, 7, 12  # k-mers of the cycle and the chain; the cycle's k-mer of genome 0 only; the chain's of {1, 2}
SHARED_TS = (1, 2, 7, 20)
SHARED_K, SHARED_G = 27, 40
ID_LABELLINGS = ((0, 1, 2), (0, 1, 300), (0, 300, 70000))  # dictionary ids of 1, 2 and 4 bytes
GRID_K, GRID_CAP, GRID_LOOSE = 27, 2048 * 256, 300  # (bft_grid_for: 2048 workgroups of 256 lanes)
GRID_LINEAR = GRID_CAP // 2
GRID_CIRCULAR = GRID_CAP - GRID_LINEAR
NONE = 0xFFFFFFFF
_ASCII = np.frombuffer(b"ACGT", dtype=np.uint8)


# ---- what the kernels derive from k (csrc/bft_succ.h, csrc/bft_paths.h) -----------------------------------------------------------------------------
def shape_of(k):
    """W words per key; tb bits in word 0; sb bucket bits (bft_sp_bucket_bits); sp_top's branch; R nucleotides behind the last whole block"""
    W = (2 * k + 63) // 64
    tb = 2 * k - 64 * (W - 1)
    sb = 2 * k if 2 * k < 20 else 20
    return {"W": W, "tb": tb, "sb": sb, "branch": "direct" if tb >= sb else "spill", "R": k % 9}


# ---- helpers ---------------------------------------------------------------------------------------------------------------------------------------
def pack(codes):
    """[n, k] nucleotide codes -> the packed k-mers every call takes: nucleotide j in bits 2 (j % 4) .. + 1 of byte j // 4"""
    codes = np.asarray(codes, dtype=np.uint8)
    n, k = codes.shape
    nb = (2 * k + 7) // 8
    pad = np.zeros((n, nb * 4), dtype=np.uint8)
    pad[:, :k] = codes
    q = pad.reshape(n, nb, 4)
    return np.ascontiguousarray(q[:, :, 0] | (q[:, :, 1] << 2) | (q[:, :, 2] << 4) | (q[:, :, 3] << 6)).astype(np.uint8)


def text(codes):
    return _ASCII[np.asarray(codes, dtype=np.uint8)].tobytes().decode()


def windows(seq, w):
    return np.lib.stride_tricks.sliding_window_view(np.asarray(seq, dtype=np.uint8), w)


def ring(period, w):
    """the len(period) windows of w nucleotides of the periodic sequence"""
    return windows(np.resize(np.asarray(period, dtype=np.uint8), len(period) + w - 1), w)


def _void(a):
    a = np.ascontiguousarray(a, dtype=np.uint8)
    return a.view(np.dtype((np.void, a.shape[1]))).ravel()


def all_distinct(rows):
    v = _void(rows)
    return len(np.unique(v)) == len(v)


def keys_u64(codes, order):
    key = np.zeros(len(codes), dtype=np.uint64)
    for j in order:
        key = (key << np.uint64(2)) | codes[:, j].astype(np.uint64)
    return key


def pack_flags(flags):
    """the flag array as bft_gpu_marks_read gives it: 4 rows per byte"""
    pad = np.zeros((len(flags) + 3) // 4 * 4, dtype=np.uint8)
    pad[:len(flags)] = flags
    q = pad.reshape(-1, 4)
    return q[:, 0] | (q[:, 1] << 2) | (q[:, 2] << 4) | (q[:, 3] << 6)


# ---- truth -----------------------------------------------------------------------------------------------------------------------------------------
class Truth:
    """parts: [(codes [m, k], slot)], the k-mers genome gids[slot] inserts (duplicates within and across parts collapse).  vector: the uint64 form."""

    def __init__(self, k, parts, gids, vector=False):
        assert not vector or k <= 32
        allc = np.concatenate([np.asarray(c, dtype=np.uint8).reshape(-1, k) for c, _ in parts])
        slot = np.concatenate([np.full(len(c), s, dtype=np.int64) for c, s in parts])
        if vector:
            key = keys_u64(allc, P.t_order(k).tolist())
            order = np.argsort(key, kind="stable")
            ks = key[order]
            new = np.concatenate([[True], ks[1:] != ks[:-1]])
        else:
            tc = allc[:, P.t_order(k)]
            order = np.lexsort(tc.T[::-1])
            ts = tc[order]
            new = np.concatenate([[True], (ts[1:] != ts[:-1]).any(axis=1)])
        row = np.cumsum(new) - 1
        self.k, self.vector, self.gids, self.N = k, vector, tuple(gids), int(row[-1]) + 1
        self.G = max(self.gids) + 1  # the library's genome count
        self.codes = np.ascontiguousarray(allc[order][new])
        self.member = np.zeros((self.N, len(self.gids)), dtype=bool)
        self.member[row, slot[order]] = True
        self.size = self.member.sum(axis=1)
        self.packed = pack(self.codes)
        self.eu, self.ev = self._edges_vector() if vector else self._edges_dict()
        self.outdeg = np.bincount(self.eu, minlength=self.N)
        self.indeg = np.bincount(self.ev, minlength=self.N)
        self._paths, self._comps = {}, {}

    # -- the two forms of the adjacency: every (u, v) with v a stored u[1:] + N, self-loops included, u ascending and v ascending within u
    @functools.cached_property
    def strings(self):
        return [text(r) for r in self.codes]

    @functools.cached_property
    def row_of(self):
        return {s: i for i, s in enumerate(self.strings)}

    def _edges_dict(self):
        eu, ev = [], []
        for u, x in enumerate(self.strings):
            for v in sorted(self.row_of[x[1:] + c] for c in "ACGT" if x[1:] + c in self.row_of):
                eu.append(u)
                ev.append(v)
        return np.array(eu, dtype=np.int64), np.array(ev, dtype=np.int64)

    def _edges_vector(self):
        k = self.k
        nat = keys_u64(self.codes, range(k))  # first nucleotide most significant
        order = np.argsort(nat)
        ns = nat[order]
        mask = np.uint64((1 << (2 * k)) - 1)
        eu, ev = [], []
        for c in range(4):
            y = ((nat << np.uint64(2)) & mask) | np.uint64(c)
            pos = np.minimum(np.searchsorted(ns, y), self.N - 1)
            hit = ns[pos] == y
            eu.append(np.flatnonzero(hit))
            ev.append(order[pos[hit]])
        eu, ev = np.concatenate(eu), np.concatenate(ev)
        o = np.lexsort((ev, eu))
        return eu[o].astype(np.int64), ev[o].astype(np.int64)

    # -- what to insert
    def inserts(self):
        """[(genome id, packed k-mers)]"""
        return [(g, np.ascontiguousarray(self.packed[self.member[:, s]])) for s, g in enumerate(self.gids) if self.member[:, s].any()]

    def sets(self):
        """per row the tuple of genome ids"""
        g = np.array(self.gids)
        return [tuple(g[m].tolist()) for m in self.member]

    # -- simple paths
    def path_rows(self, t):
        """the rows of every path, paths by the row of their head"""
        if t not in self._paths:
            node = (self.outdeg <= 1) & (self.indeg <= 1) & (self.size >= t)
            u, v = self.eu, self.ev
            ok = node[u] & node[v] & (u != v)
            if t:
                ok &= (self.member[u] & self.member[v]).sum(axis=1) >= t
            nxt, prv = np.full(self.N, -1, dtype=np.int64), np.full(self.N, -1, dtype=np.int64)
            nxt[u[ok]] = v[ok]
            prv[v[ok]] = u[ok]
            nl, seen, out = nxt.tolist(), bytearray(self.N), []
            # chains from their heads; what is left lies on cycles, and in ascending row the first k-mer met of a cycle is its smallest
            for h in np.flatnonzero(node & (prv < 0)).tolist() + np.flatnonzero(node & (prv >= 0)).tolist():
                if seen[h]:
                    continue
                p, x = [h], nl[h]
                seen[h] = 1
                while x >= 0 and not seen[x]:
                    p.append(x)
                    seen[x] = 1
                    x = nl[x]
                out.append(p)
            out.sort(key=lambda p: p[0])
            self._paths[t] = out
        return self._paths[t]

    def paths(self, t):
        last = self.codes[:, self.k - 1]
        return [text(self.codes[p[0]]) + text(last[p[1:]]) for p in self.path_rows(t)]

    def path_counts(self, t):
        """{paths, characters, longest} of the sizing call"""
        n = [len(p) + self.k - 1 for p in self.path_rows(t)]
        return [len(n), sum(n), max(n) if n else 0]

    # -- components
    def members(self, ids):
        if any(g not in self.gids for g in ids):
            return np.zeros(self.N, dtype=bool)
        return self.member[:, [self.gids.index(g) for g in ids]].all(axis=1)

    def components(self, ids=()):
        """(labels per row, sizes): the induced sub-graph of the rows that carry every id; components numbered by their smallest row"""
        ids = tuple(ids)
        if ids not in self._comps:
            mem = self.members(ids)
            ok = mem[self.eu] & mem[self.ev] & (self.eu != self.ev)
            parent = list(range(self.N))
            for a, b in zip(self.eu[ok].tolist(), self.ev[ok].tolist()):
                while parent[a] != a:
                    parent[a] = parent[parent[a]]
                    a = parent[a]
                while parent[b] != b:
                    parent[b] = parent[parent[b]]
                    b = parent[b]
                if a != b:
                    parent[max(a, b)] = min(a, b)  # (the root is the smallest row)
            root = np.array(parent, dtype=np.int64)
            while (root[root] != root).any():
                root = root[root]
            roots = np.unique(root[mem])
            labels = np.full(self.N, NONE, dtype=np.uint32)
            labels[mem] = np.searchsorted(roots, root[mem])
            sizes = np.bincount(labels[mem], minlength=len(roots)).astype(np.uint64)
            self._comps[ids] = (labels, sizes)
        return self._comps[ids]

    def component_counts(self, ids=()):
        labels, sizes = self.components(ids)
        return [len(sizes), int((labels != NONE).sum()), int(sizes.max()) if len(sizes) else 0]

    # -- marks, classes, sub-graphs
    def model(self):
        return MarkModel({s: set(c) for s, c in zip(self.strings, self.sets())})

    def by_count(self, lo, hi):
        return np.flatnonzero((self.size >= lo) & (self.size <= hi)).astype(np.uint32)

    def absent(self, n, seed):
        """n k-mers that are not stored, each one substitution away from a stored one"""
        rng = np.random.default_rng(seed)
        have = set(_void(self.codes).tolist())
        out = []
        while len(out) < n:
            x = self.codes[int(rng.integers(0, self.N))].copy()
            j = int(rng.integers(0, self.k))
            x[j] = (x[j] + int(rng.integers(1, 4))) & 3
            if _void(x[None])[0].item() not in have:
                out.append(x)
        return np.array(out, dtype=np.uint8)


def from_sets(k, codes, sets, gids, vector=False):
    """a truth from distinct k-mers and, per k-mer, the slots (positions in gids) that hold it"""
    codes = np.asarray(codes, dtype=np.uint8)
    parts = []
    for s in range(len(gids)):
        sel = [i for i, c in enumerate(sets) if s in c]
        if sel:
            parts.append((codes[sel], s))
    return Truth(k, parts, gids, vector)


# ---- case builders ---------------------------------------------------------------------------------------------------------------------------------
def _pieces(rng, k, cycles, chains):
    """periods of the given cycle lengths and sequences of the given chain lengths (in k-mers) that share no (k-1)-mer: the graph of their k-mers
    is exactly those cycles and chains.  Drawn again until it is so."""
    while True:
        per = [rng.integers(0, 4, p, dtype=np.uint8) for p in cycles]
        seq = [rng.integers(0, 4, m + k - 1, dtype=np.uint8) for m in chains]
        if all_distinct(np.concatenate([ring(x, k - 1) for x in per] + [windows(x, k - 1) for x in seq])):
            return per, seq


@functools.lru_cache(maxsize=None)
def key_shape(k):
    """an ancestor of 1500 bases with one internal repeat (branching at both of its ends) and two SNP mutants, genomes 0..2"""
    rng = np.random.default_rng(7000 + k)
    anc = rng.integers(0, 4, 1500, dtype=np.uint8)
    a, b = int(rng.integers(0, 400)), int(rng.integers(800, 1100))
    anc[b:b + 300] = anc[a:a + 300]
    parts = [(windows(anc, k), 0)]
    for g in (1, 2):
        m = anc.copy()
        hit = rng.random(len(m)) < 0.01
        m[hit] = (m[hit] + rng.integers(1, 4, int(hit.sum()), dtype=np.uint8)) & 3
        parts.append((windows(m, k), g))
    return Truth(k, parts, (0, 1, 2))


@functools.lru_cache(maxsize=None)
def dense(k):
    """a k-mer u with its four successors and four predecessors stored; at k % 9 == 0 every successor also with the three substitutions of its
    nucleotide k - 9 (the last digit of its T-form: they lie inside the 16-row interval of u's successors, and are no successors); 300 others"""
    rng = np.random.default_rng(8000 + k)
    u = rng.integers(0, 4, k, dtype=np.uint8)
    rows = [u]
    for c in range(4):
        rows += [np.concatenate([u[1:], [c]]), np.concatenate([[c], u[:-1]])]
        if k % 9 == 0:
            for s in (1, 2, 3):
                x = np.concatenate([u[1:], [c]]).astype(np.uint8)
                x[k - 9] = (x[k - 9] + s) & 3
                rows.append(x)
    rows = np.concatenate([np.array(rows, dtype=np.uint8), rng.integers(0, 4, (300, k), dtype=np.uint8)])
    rows = rows[np.sort(np.unique(_void(rows), return_index=True)[1])]
    sets = [((0,), (1,), (0, 1))[int(x)] for x in rng.integers(0, 3, len(rows))]
    tr = from_sets(k, rows, sets, (0, 1))
    tr.u = tr.row_of[text(u)]
    return tr


@functools.lru_cache(maxsize=None)
def ends(k, table):
    """the tables of the successor search's ends (test_ends_tables_show_their_situation derives each from the keys)"""
    rng = np.random.default_rng(9000 + 10 * k + ENDS_TABLES.index(table))
    key = lambda x: P.t_key_ints(np.asarray(x)[None], k)[0]
    if table == "lone":
        return from_sets(k, rng.integers(0, 4, (1, k), dtype=np.uint8), [(0,)], (0,))
    if table == "homopolymer":
        return from_sets(k, np.full((1, k), 2, dtype=np.uint8), [(0,)], (0,))
    if table == "two":
        x = _pieces(rng, k, (), (2,))[1][0]
        return from_sets(k, windows(x, k), [(0,), (0,)], (0,))
    rows = rng.integers(0, 4, (150, k), dtype=np.uint8)
    if table == "above":
        # x = N G T..T: the key its successors are searched from, that of G T..T A, starts with T's -- above x's own and above every other row kept
        x = np.full(k, 3, dtype=np.uint8)
        x[0], x[1] = rng.integers(0, 4), 2
        top = key(np.concatenate([x[1:], [0]]))
        rows = rows[[key(r) < top for r in rows]]
        a = np.zeros(k, dtype=np.uint8)  # all-A is row 0, and the successor of C A..A
        ca = a.copy()
        ca[0] = 1
        rows = np.concatenate([rows, x[None], a[None], ca[None]])
    else:
        # the last row gets a stored successor that sorts below it
        last = max(rows.tolist(), key=key)
        for c in range(4):
            s = np.array(last[1:] + [c], dtype=np.uint8)
            if key(s) < key(last):
                rows = np.concatenate([rows, s[None]])
                break
    rows = rows[np.sort(np.unique(_void(rows), return_index=True)[1])]
    sets = [((0,), (1,), (0, 1))[int(v)] for v in rng.integers(0, 3, len(rows))]
    return from_sets(k, rows, sets, (0, 1))


@functools.lru_cache(maxsize=None)
def cycles(k, p):
    """two cycles of p k-mers (genome 0; genomes 0 and 1) and chains of CYCLE_CHAINS k-mers (genome 1; 0 and 1; 0) in one index"""
    rng = np.random.default_rng(10000 + 300 * k + p)
    per, seq = _pieces(rng, k, (p, p), CYCLE_CHAINS)
    km = [ring(x, k) for x in per] + [windows(x, k) for x in seq]
    tr = Truth(k, [(np.concatenate([km[0], km[1], km[3], km[4]]), 0), (np.concatenate([km[1], km[2], km[3]]), 1)], (0, 1))
    tr.cycle_rows = [sorted(tr.row_of[text(x)] for x in c) for c in km[:2]]
    tr.periods = per
    return tr


@functools.lru_cache(maxsize=None)
def whole_table(n, kind, k):
    """the index is exactly one chain or one cycle of n k-mers, one genome"""
    rng = np.random.default_rng(11000 + 5000 * k + 2 * n + (kind == "cycle"))
    per, seq = _pieces(rng, k, (n,) if kind == "cycle" else (), (n,) if kind == "chain" else ())
    km = ring(per[0], k) if kind == "cycle" else windows(seq[0], k)
    return Truth(k, [(km, 0)], (0,))


@functools.lru_cache(maxsize=None)
def cut(k, gids=(0, 1, 2)):
    """a cycle of CUT_CYCLE and a chain of CUT_CHAIN k-mers held by the first two genomes; the cycle's k-mer CUT_GAP is held by the first genome
    only (at t = 2 the cycle is a chain headed behind the gap); the chain's k-mer CUT_ODD by the last two (a node at t = 2, both its edges cut)"""
    rng = np.random.default_rng(12000 + k)
    per, seq = _pieces(rng, k, (CUT_CYCLE,), (CUT_CHAIN,))
    cyc, chn = ring(per[0], k), windows(seq[0], k)
    sets = [(0,) if i == CUT_GAP else (0, 1) for i in range(CUT_CYCLE)] + [(1, 2) if i == CUT_ODD else (0, 1) for i in range(CUT_CHAIN)]
    tr = from_sets(k, np.concatenate([cyc, chn]), sets, gids)
    tr.cycle, tr.chain = [text(x) for x in cyc], [text(x) for x in chn]
    return tr


def id_widths():
    """the cut graph at k = 27 under three labellings of its genomes"""
    return [cut(27, g) for g in ID_LABELLINGS]


def _shared_lists(o, e, place):
    """(common, only a, only b): o common ids and e ids of either list's own, the common ones in front, at the back or interleaved"""
    ids = list(range(o + 2 * e)) if place != "back" else list(range(SHARED_G - o - 2 * e, SHARED_G))
    if place == "front":
        common, rest = ids[:o], ids[o:]
    elif place == "back":
        common, rest = ids[len(ids) - o:], ids[:len(ids) - o]
    else:
        step = max(1, len(ids) // max(o, 1))
        common = ids[1::step][:o] if o else []
        common += [x for x in ids if x not in common][:o - len(common)]
        rest = [x for x in ids if x not in common]
    return sorted(common), rest[0::2], rest[1::2]


@functools.lru_cache(maxsize=None)
def shared(t):
    """40 genomes; 18 pairs u -> v of neighbouring k-mers whose id lists of about 20 ids share exactly t - 1, t and t + 1, the common ids in
    front, at the back or interleaved, either list starting lower"""
    rng = np.random.default_rng(13000 + t)
    k = SHARED_K
    plan = [(o, place, swap) for o in (t - 1, t, t + 1) for place in ("front", "back", "inter") for swap in (0, 1)]
    _, seq = _pieces(rng, k, (), (2,) * len(plan))
    rows, sets, pairs = [], [], []
    for (o, place, swap), s in zip(plan, seq):
        e = max(20 - o, 3)
        assert o + 2 * e <= SHARED_G
        common, a, b = _shared_lists(o, e, place)
        if swap:
            a, b = b, a
        rows += [s[:k], s[1:]]
        sets += [tuple(sorted(common + a)), tuple(sorted(common + b))]
        pairs.append((text(s[:k]), text(s[1:]), o, place, swap))
    tr = from_sets(k, np.array(rows), sets, tuple(range(SHARED_G)))
    tr.pairs = pairs
    return tr


def grid_parts(n_lin, n_circ, n_loose, seed):
    """one linear genome of n_lin k-mers, one circular of n_circ, n_loose loose k-mers, all in genome 0; genome 1 holds all but a stretch of the
    linear genome.  ([(codes, slot)], (first, end) of the stretch among the linear k-mers)"""
    rng = np.random.default_rng(seed)
    k = GRID_K
    lin = windows(rng.integers(0, 4, n_lin + k - 1, dtype=np.uint8), k)
    circ = ring(rng.integers(0, 4, n_circ, dtype=np.uint8), k)
    loose = rng.integers(0, 4, (n_loose, k), dtype=np.uint8)
    # the stretch begins behind a linear k-mer among the last n_loose rows of the table: in the grid case the boundary row behind a reach over
    # genome 1 is found from a row of the second pass
    t_order = P.t_order(k).tolist()
    every = np.sort(np.concatenate([keys_u64(x, t_order) for x in (lin, circ, loose)]))
    high = np.flatnonzero(keys_u64(lin, t_order) >= every[len(every) - n_loose])
    a = int(high[high >= n_lin // 3][0]) + 1
    b = a + n_lin // 50
    return [(np.concatenate([lin, circ, loose]), 0), (np.concatenate([lin[:a], lin[b:], circ, loose]), 1)], (a, b), lin, circ


@functools.lru_cache(maxsize=None)
def grid():
    parts, stretch, lin, circ = grid_parts(GRID_LINEAR, GRID_CIRCULAR, GRID_LOOSE, 14000)
    tr = Truth(GRID_K, parts, (0, 1), vector=True)
    tr.stretch = stretch
    t_order = P.t_order(GRID_K).tolist()
    tkeys = keys_u64(tr.codes, t_order)
    row = lambda x: int(np.searchsorted(tkeys, keys_u64(np.asarray(x)[None], t_order)[0]))
    tr.seeds = {"linear": lin[5].copy(), "circular": circ[5].copy()}
    tr.seed_rows = {name: row(x) for name, x in tr.seeds.items()}
    tr.before_stretch = row(lin[stretch[0] - 1])
    return tr


# ---- tests: the order of the rows is the library's -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hostlib():
    subprocess.check_call(["make", "-C", _lib.CSRC, "all"], stdout=subprocess.DEVNULL)
    lib = C.CDLL(os.path.join(_lib.CSRC, "libbft_hosttest.so"))
    lib.bft_hosttest_roundtrip.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p]
    return lib


@pytest.mark.parametrize("k", sorted(set(KEY_SHAPES + DENSE_KS + ENDS_KS + CYCLE_KS + CUT_KS)))
def test_t_form_key_is_the_librarys(hostlib, k):
    tr = key_shape(k)
    pick = np.unique(np.concatenate([np.arange(0, tr.N, 53), [tr.N - 1]]))
    packed = np.ascontiguousarray(tr.packed[pick])
    W = shape_of(k)["W"]
    out, tf = np.zeros_like(packed), np.zeros(len(packed) * W, dtype=np.uint64)
    hostlib.bft_hosttest_roundtrip(packed.ctypes.data, len(packed), k, out.ctypes.data, tf.ctypes.data)
    assert (out == packed).all()
    got = [sum(int(w) << (64 * (W - 1 - j)) for j, w in enumerate(tf[i * W:(i + 1) * W])) for i in range(len(packed))]
    want = P.t_key_ints(tr.codes[pick], k)
    assert got == want
    assert all(a < b for a, b in zip(want, want[1:]))  # and the truth's rows are in the order of those keys


# ---- tests: the key shapes -------------------------------------------------------------------------------------------------------------------------
def test_key_shapes_with_the_recipe_hit_every_shape():
    shapes = {k: shape_of(k) for k in KS + KEY_SHAPES}
    new = {k: shape_of(k) for k in KEY_SHAPES}
    assert {s["W"] for s in shapes.values()} == {1, 2, 3, 4}
    assert {s["W"] for s in new.values()} == {1, 2, 3, 4} and 3 not in {shape_of(k)["W"] for k in KS}  # (the recipe has no three-word key)
    assert {(s["W"], s["R"] == 0) for s in shapes.values()} == {(W, z) for W in (1, 2, 3, 4) for z in (False, True)}
    # R != 0 on two words or more, other than k = 64
    assert {s["W"] for k, s in new.items() if s["R"] and s["W"] >= 2} == {2, 3, 4}
    branch = {(s["branch"], s["tb"]) for s in shapes.values()}
    assert {("spill", 2), ("spill", 18), ("direct", 20), ("direct", 64)} <= branch
    for tb, ks in ((2, (33, 65, 97)), (18, (41, 105)), (20, (10, 42, 74)), (64, (32, 96))):
        for k in ks:
            assert k in KEY_SHAPES and new[k]["tb"] == tb and new[k]["branch"] == ("direct" if tb >= 20 else "spill"), k
    assert all(new[k]["tb"] == new[k]["sb"] == 20 for k in (10, 42, 74))  # tb == sb on one, two and three words
    assert shape_of(10)["sb"] == 2 * 10 and shape_of(10)["R"] == 1  # every bucket is one key, with a remainder nucleotide
    assert shape_of(9)["sb"] == 18 and shape_of(9)["R"] == 0
    # spill on W = 2, 3, 4; none of those in the recipe except k = 36
    assert {s["W"] for s in new.values() if s["branch"] == "spill"} == {2, 3, 4}
    assert [k for k in KS if shape_of(k)["branch"] == "spill"] == [36]


@pytest.mark.parametrize("k", KEY_SHAPES)
def test_key_shape_indexes(k):
    tr = key_shape(k)
    assert 1400 <= tr.N <= 6500
    assert (tr.outdeg >= 2).any() and (tr.indeg >= 2).any()  # the repeat branches
    assert len(tr.path_rows(0)) > 3 and len(tr.path_rows(2)) > 3 and tr.path_rows(4) == []
    assert len({s for s in tr.sets()}) >= 4
    if k == 10:  # sb == 2k with R != 0: the four successors lie in four buckets, and some row has one beyond the first
        later = [(u, v) for u, v in zip(tr.eu.tolist(), tr.ev.tolist()) if tr.codes[v, k - 1] != 0]
        assert later


# ---- tests: dense, ends ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", DENSE_KS)
def test_dense_tables(k):
    tr = dense(k)
    u = tr.u
    succ = tr.ev[tr.eu == u]
    assert len(succ) == 4 and tr.indeg[u] == 4 and tr.outdeg[u] == 4
    between = set(range(int(succ.min()), int(succ.max()) + 1)) - set(succ.tolist())
    if k % 9 == 0:
        assert len(between) >= 1 and shape_of(k)["R"] == 0
        assert np.diff(succ).tolist() == [4, 4, 4]  # the whole 16-row interval is stored: three other rows between two successors
    else:
        assert not between
    assert u not in [p[0] for p in tr.path_rows(0)] and all(u not in p for p in tr.path_rows(0))  # u branches: in no path


@pytest.mark.parametrize("k", ENDS_KS)
def test_ends_tables_show_their_situation(k):
    sb = shape_of(k)["sb"]
    bucket = lambda key: key >> (2 * k - sb)
    target = lambda tr, u: P.t_key_ints(np.concatenate([tr.codes[u, 1:], [0]])[None], k)[0]  # the key the lower bound is taken from
    tr = ends(k, "above")
    keys = P.t_key_ints(tr.codes, k)
    assert keys == sorted(keys)
    occupied = {bucket(x) for x in keys}
    assert any(target(tr, u) > keys[-1] for u in range(tr.N))  # above every stored row
    assert any(bucket(target(tr, u)) not in occupied for u in range(tr.N))  # an empty bucket
    assert any(v == 0 and u != 0 for u, v in zip(tr.eu.tolist(), tr.ev.tolist()))  # a successor at row 0
    assert (tr.codes[0] == 0).all()
    tr = ends(k, "last")
    assert any(u == tr.N - 1 and v != u for u, v in zip(tr.eu.tolist(), tr.ev.tolist()))  # the last row has a stored successor
    for name, rows, paths in (("lone", 1, 1), ("homopolymer", 1, 1), ("two", 2, 1)):
        tr = ends(k, name)
        assert tr.N == rows and tr.path_counts(0) == [paths, rows + k - 1, rows + k - 1] and tr.component_counts() == [1, rows, rows]
    assert ends(k, "homopolymer").eu.tolist() == [0] and ends(k, "homopolymer").ev.tolist() == [0]  # its own successor: a lone node


# ---- tests: cycles, whole tables, cuts -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", CYCLE_KS)
@pytest.mark.parametrize("p", CYCLE_PS)
def test_cycle_indexes(p, k):
    tr = cycles(k, p)
    assert tr.N == 2 * p + sum(CYCLE_CHAINS)
    assert all_distinct(np.concatenate([ring(x, k - 1) for x in tr.periods]))
    assert (tr.outdeg <= 1).all() and (tr.indeg <= 1).all()
    assert tr.component_counts() == [5, tr.N, max(p, max(CYCLE_CHAINS))]
    assert sorted(tr.components()[1].tolist()) == sorted([p, p] + list(CYCLE_CHAINS))
    rows = tr.path_rows(0)
    assert len(rows) == 5 and [r[0] for r in rows] == sorted(r[0] for r in rows)
    for cyc in tr.cycle_rows:
        mine = [r for r in rows if r[0] == cyc[0]]  # the cycle is headed by its smallest row and holds all its rows once
        assert len(mine) == 1 and sorted(mine[0]) == cyc
    assert sorted(len(s) for s in tr.paths(0)) == sorted(m + k - 1 for m in (p, p) + CYCLE_CHAINS)
    assert tr.path_counts(2) == [2, p + 18 + 2 * (k - 1), max(p, 18) + k - 1] and tr.path_counts(3) == [0, 0, 0]


@pytest.mark.parametrize("k", WHOLE_KS)
@pytest.mark.parametrize("kind", ("chain", "cycle"))
@pytest.mark.parametrize("n", WHOLE_NS)
def test_whole_tables(n, kind, k):
    tr = whole_table(n, kind, k)
    assert tr.N == n and len(tr.eu) == (n if kind == "cycle" else n - 1)
    assert tr.path_counts(0) == [1, n + k - 1, n + k - 1] and tr.path_counts(1) == tr.path_counts(0) and tr.path_counts(2) == [0, 0, 0]
    assert tr.component_counts() == [1, n, n]
    assert tr.path_rows(0)[0][0] == (0 if kind == "cycle" else tr.path_rows(0)[0][0]) and sorted(tr.path_rows(0)[0]) == list(range(n))
    # the rounds of the jumps, ceil(log2(n + 1)), change between 2^r - 1 and 2^r
    rounds = lambda m: len(bin(m)) - 2
    assert [rounds(m) for m in (63, 64, 65, 1023, 1024, 1025)] == [6, 7, 7, 10, 11, 11]


@pytest.mark.parametrize("k", CUT_KS)
def test_cut_graphs(k):
    tr = cut(k)
    assert tr.N == CUT_CYCLE + CUT_CHAIN
    for t in (0, 1):
        assert sorted(len(s) for s in tr.paths(t)) == [CUT_CHAIN + k - 1, CUT_CYCLE + k - 1]
    two = tr.paths(2)
    assert sorted(len(s) for s in two) == sorted(m + k - 1 for m in (CUT_CYCLE - 1, CUT_ODD, 1, CUT_CHAIN - CUT_ODD - 1))
    opened = [s for s in two if len(s) == CUT_CYCLE - 1 + k - 1][0]
    assert opened[:k] == tr.cycle[CUT_GAP + 1] and opened[-k:] == tr.cycle[CUT_GAP - 1]  # headed behind the gap, not at the smallest row
    assert tr.chain[CUT_ODD] in two and tr.size[tr.row_of[tr.chain[CUT_ODD]]] == 2  # a node at t = 2, alone
    assert tr.paths(3) == []
    assert tr.component_counts() == [2, tr.N, CUT_CYCLE]
    assert tr.component_counts((tr.gids[1],)) == [2, tr.N - 1, CUT_CYCLE - 1]
    assert tr.component_counts((tr.gids[0], tr.gids[1])) == [3, tr.N - 2, CUT_CYCLE - 1]
    assert tr.component_counts((tr.gids[2] + 1,)) == [0, 0, 0]


def test_id_width_labellings_are_one_graph():
    a, b, c = id_widths()
    width = lambda tr: 1 if tr.G <= 256 else 2 if tr.G <= 65536 else 4  # (bytes per dictionary id: by the largest genome id)
    assert [width(x) for x in (a, b, c)] == [1, 2, 4]
    for x in (b, c):
        assert (x.codes == a.codes).all() and (x.member == a.member).all()
        for t in (0, 1, 2, 3):
            assert x.paths(t) == a.paths(t)
        for slots in ((), (0,), (1,), (0, 1), (1, 2)):
            la, lx = a.components([a.gids[s] for s in slots]), x.components([x.gids[s] for s in slots])
            assert (la[0] == lx[0]).all() and (la[1] == lx[1]).all()


# ---- tests: the merge of two id lists --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", SHARED_TS)
def test_shared_overlaps(t):
    tr = shared(t)
    assert tr.G == SHARED_G and len(tr.pairs) == 18
    sets = tr.sets()
    seen = set()
    for u, v, o, place, swap in tr.pairs:
        cu, cv = sets[tr.row_of[u]], sets[tr.row_of[v]]
        common = sorted(set(cu) & set(cv))
        own = sorted(set(cu) ^ set(cv))
        assert len(common) == o and o in (t - 1, t, t + 1)
        assert 20 <= len(cu) <= 24 and len(cu) == len(cv) and len(cu) >= t
        if common:
            if place == "front":
                assert common[-1] < own[0]
            elif place == "back":
                assert common[0] > own[-1]
            else:
                assert common[0] < own[-1] and common[-1] > own[0]
        assert (min(set(cu) - set(cv)) < min(set(cv) - set(cu))) == (swap == 0)  # either list starts lower
        assert tr.ev[tr.eu == tr.row_of[u]].tolist() == [tr.row_of[v]]
        seen.add((o - t, place, swap))
    assert len(seen) == 18
    # at the threshold: a pair that shares t - 1 is two paths, the others one
    assert tr.path_counts(t)[0] == 6 * 2 + 12 and tr.path_counts(0)[0] == 18 and tr.path_counts(t + 1)[0] == 12 * 2 + 6
    assert sorted(set(len(s) for s in tr.paths(t))) == [SHARED_K, SHARED_K + 1]


# ---- tests: the grid -------------------------------------------------------------------------------------------------------------------------------
def test_grid_case():
    tr = grid()
    k = GRID_K
    assert tr.N == GRID_CAP + GRID_LOOSE > GRID_CAP  # a one-row-per-lane kernel takes a second pass
    a, b = tr.stretch
    n0 = tr.path_counts(0)
    assert n0 == [2 + GRID_LOOSE, tr.N + (2 + GRID_LOOSE) * (k - 1), max(GRID_LINEAR, GRID_CIRCULAR) + k - 1]
    big = sorted(len(p) + k - 1 for p in tr.path_rows(0))[-2:]
    assert big == sorted([GRID_LINEAR + k - 1, GRID_CIRCULAR + k - 1]) and min(big) > GRID_CAP // 2  # both longer (in characters) than half the cap
    assert tr.path_counts(2) == [3 + GRID_LOOSE, tr.N - (b - a) + (3 + GRID_LOOSE) * (k - 1), GRID_CIRCULAR + k - 1]
    assert tr.component_counts() == [2 + GRID_LOOSE, tr.N, GRID_LINEAR]
    assert tr.component_counts((1,)) == [3 + GRID_LOOSE, tr.N - (b - a), GRID_CIRCULAR]
    assert tr.by_count(1, 1).shape == (b - a,) and len(tr.by_count(2, 2)) == tr.N - (b - a)
    # rows of both passes in both big paths, and edges that cross from one pass into the other
    for p in [p for p in tr.path_rows(0) if len(p) > 1]:
        r = np.array(p)
        assert (r < GRID_CAP).any() and (r >= GRID_CAP).any()
        assert ((r[:-1] < GRID_CAP) != (r[1:] < GRID_CAP)).any()
    assert tr.before_stretch >= GRID_CAP and a > 5 and tr.member[tr.before_stretch].all()  # the member that finds the boundary row: second pass
    labels = tr.components()[0]
    assert labels[tr.seed_rows["linear"]] != labels[tr.seed_rows["circular"]]
    assert {int(tr.components()[1][labels[r]]) for r in tr.seed_rows.values()} == {GRID_LINEAR, GRID_CIRCULAR}


def test_dict_and_vector_truths_agree():
    """the grid's recipe at 3e4 rows, by both forms"""
    parts, stretch, _, _ = grid_parts(14850, 14850, 300, 14001)
    d, v = Truth(GRID_K, parts, (0, 1)), Truth(GRID_K, parts, (0, 1), vector=True)
    assert d.N == v.N == 30000
    assert (d.codes == v.codes).all() and (d.member == v.member).all()
    assert (d.eu == v.eu).all() and (d.ev == v.ev).all()
    for t in (0, 1, 2, 3):
        assert d.path_rows(t) == v.path_rows(t) and d.paths(t) == v.paths(t)
    for ids in ((), (0,), (1,), (0, 1), (2,)):
        assert (d.components(ids)[0] == v.components(ids)[0]).all() and (d.components(ids)[1] == v.components(ids)[1]).all()
    assert d.path_counts(0)[0] == 302 and d.path_counts(2)[0] == 303
    # and the dict form against a definition written out once more, by strings alone
    owners = dict(zip(d.strings, d.sets()))
    succ = lambda x: [x[1:] + c for c in "ACGT" if x[1:] + c in owners]
    pred = lambda x: [c + x[:-1] for c in "ACGT" if c + x[:-1] in owners]
    node = {x for x in owners if len(succ(x)) <= 1 and len(pred(x)) <= 1 and len(owners[x]) >= 2}
    edges = sum(1 for x in node for y in succ(x) if y != x and y in node and len(set(owners[x]) & set(owners[y])) >= 2)
    assert sum(len(p) for p in d.path_rows(2)) == len(node)
    assert sum(len(p) - 1 for p in d.path_rows(2)) == edges - 1  # (the circular genome keeps all its edges: its path is cut at one of them)
