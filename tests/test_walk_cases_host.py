"""The cases of the walk edge tests (tests/test_gpu_walk_edges.py runs them on the GPU): query_body / branching_body of csrc/bft_kernels_query.h, the
container walk -- its per-wavefront queue of parked lanes, its 1024-k-mer chunks, the claim of the next chunk, the late OR -- and the root tables
that decide who parks.  Here, without a GPU: the indexes, their truth, and the proof that every case reaches the regime it is named after.

Built on test_assembly_cases_host (H): Table is the truth of the rows, model() the containers, codes_from_digits the way from T-form digits to
k-mers, hashpos the Bloom positions.

The walk index of a k (walk_index): about 10^4 rows in 3 genomes, made from T-form digits -- root prefixes that are child Nodes (one with 300 rows
under one second digit, so the parked walk descends two levels where L >= 3; a chain of 300 rows down to the last level), some hundred plain
root prefixes of 1 .. 255 rows, root UC rows, the root prefix 2^18 - 1 as a plain group (a group ends at the table's last row), and the
families of the branching cases.  L = 1 (k = 9, 13) has no child Nodes and no plain groups: every prefix a CC holds is special there.

special(r), rstart and rq (root_tables) come from the model alone, by the rule of bft_root_range_entry / bft_root_range_ok (csrc/bft_walk.h) read
as a specification; the count of plain prefixes is held against the host restatement's (bft_hosttest_root_plain), and the pools' truth
against its walk.

Layouts place the parked lanes of a batch exactly: a layout is a mask `parked` per batch position (and, for same_word, the answer too), filled from
the query pools.  Every layout is periodic in chunks of 1024, so it reaches its regime however the chunks are dealt: simulate() replays
query_body's queue and chunk bookkeeping for the static dealing and, with claim_seed, for a claimed dealing (the first chunk by wavefront
number, the others in a random order of arrival), and the tests below hold every (k, layout, dealing) the GPU file runs to a non-zero counter
of its regime.  The > 2^32-query guard on qbase (q0 + 64 - qbase > 0xFFFFFFFF) is unreachable at test size and has no case.

Not covered, and why.  (1) STAGED = false with CCs at the root: the walk stages a root of 1 .. 64 CCs, and `ncc_max`, the most CCs a node was ever
made to hold (test_assembly_cases_host.test_most_ccs_a_node_can_reach), has 20 -- so its root is staged, and the only unstaged root any test runs is the
one without a CC (`tiny`).  (2) Block reads of bft_group_count4 past the table's end: it reads aligned blocks of 8 one-word or 4 two-word rows (64
bytes) and only for W <= BFT_PROBE_MAX_W = 2; W = 3 and 4 search each successor on its own (bft_group_search) and read no block.  A block that
holds the table's last row reaches at most 56 (W = 1) or 48 (W = 2) bytes past it, inside the 256 bytes of slack every device block carries; the
"table end" families (k = 9 .. 64 with W <= 2; k = 72, 96, 126 through the per-successor search) run exactly that place."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_assembly_cases_host as H  # noqa: E402
import test_prefix_cases_host as P  # noqa: E402

from bloomfiltertrie_amd import synth as S  # noqa: E402

KS = (9, 13, 18, 31, 32, 36, 63, 64, 72, 96, 126)
FULL_KS = (18, 36)  # the k that run the full option set on the GPU
COUNTS = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 40, 255)
QCAP = {1: 64, 2: 32, 3: 16, 4: 16}  # query_body: entries per wavefront's queue
CHUNK, PASSES = 1024, 16
SPECIAL = 0x80000000
ABSENT = 0xFFFFFFFF
SUBSETS = ((), (0,), (3,), (0, 3), (1, 2), (0, 2, 3), (0, 1, 2, 3))  # stored successors / predecessors (0, 2, 3: so that a count of 3 occurs)
N_GENOMES = 3
N_LAYOUT = 49 * CHUNK + 3 * 64 + 7  # 50 chunks: 3 or 4 per wavefront of one workgroup (16) and 4 or 5 (12); a last chunk of 4 passes, a last word of 7 bits
POOLS = ("plain_present", "plain_absent", "empty", "node_present", "node_absent1", "node_absent_deep", "uc_present", "uc_absent")
PARKED_POOLS = ("node_present", "node_absent1", "node_absent_deep", "uc_present", "uc_absent")
DIRECT_POOLS = ("plain_present", "plain_absent", "empty")


def W_of(k):
    return (2 * k + 63) // 64


# ---- the walk index ------------------------------------------------------------------------------------------------------------------------------
class Rows:
    """rows of an index under construction, as T-form digits [n, L] and remainders [n]"""

    def __init__(self, k):
        self.k, self.L, self.R = k, k // 9, k % 9
        self.dig, self.rem = [], []

    def add(self, dig, rem=None):
        dig = np.asarray(dig, dtype=np.int64).reshape(-1, self.L)
        self.dig.append(dig)
        self.rem.append(np.zeros(len(dig), np.int64) if rem is None else np.asarray(rem, dtype=np.int64).reshape(-1) & ((1 << (2 * self.R)) - 1))

    def codes(self):
        return H.codes_from_digits(self.k, np.concatenate(self.dig), np.concatenate(self.rem) if self.R else None)


def _suffixes(k, rng, c, lo=4096, hi=(1 << 18) - 4096):
    """c distinct suffixes behind a root digit ([c, L - 1] digits, [c] remainders), second digits (or remainders, L = 1) ascending within [lo, hi)"""
    L, R = k // 9, k % 9
    if L == 1:
        c = min(c, 4 ** R - 8 if R else 1)
        return np.zeros((c, 0), np.int64), (8 + np.sort(rng.choice(4 ** R - 8, c, replace=False))) if R else np.zeros(c, np.int64)
    d1 = np.sort(rng.choice(hi - lo, c, replace=False)) + lo
    rest = rng.integers(0, 1 << 18, (c, L - 2))
    return np.concatenate([d1[:, None], rest], axis=1), rng.integers(0, 4 ** R, c) if R else np.zeros(c, np.int64)


def fam_suffix(k, depth, j, v):
    """The suffix behind `depth` fixed digits of sibling v of family j: (digits [L - depth], remainder).  The four siblings differ in the last
    nucleotide only -- the two lowest bits of the remainder, or bits 2..3 of the last digit (rb == 0) --, families sort by j, and no two families
    share more than their first k - 2 nucleotides' worth of path (j never sits in the last two nucleotides)."""
    L, R = k // 9, k % 9
    m = L - depth  # digits left
    const = 0x1A2B0
    if R:
        if m == 0:
            return [], (16 * j | v) & (4 ** R - 1)
        return [64 * j + 1] + [const] * (m - 1), (0x5550 & ~3 | v) & (4 ** R - 1)
    assert m >= 1
    if m == 1:
        return [64 * j + (v << 2) + 1], 0
    return [64 * j + 1] + [const] * (m - 2) + [const & ~12 | (v << 2)], 0


J_LAST = 4090  # the family behind every filler row of its group (64 j + 1 < 2^18); 15 where the family number sits in a remainder of 8 bits


class Family:
    """the sibling k-mers s[:-1] + N of one path; `stored`: the subset in the index; `kind`, `where`: the container and the placement it stands for"""

    def __init__(self, k, head, j, stored, kind, where="", dig=None, rem_base=None):
        self.kind, self.where, self.stored = kind, where, tuple(stored)
        if rem_base is not None:  # (every digit fixed: the siblings are four remainders)
            self.dig, self.rem = np.tile(np.asarray(head, dtype=np.int64), (4, 1)), rem_base + np.arange(4)
        elif dig is None:
            rows = [fam_suffix(k, len(head), j, v) for v in range(4)]
            self.dig = np.array([list(head) + r[0] for r in rows], dtype=np.int64).reshape(4, k // 9)
            self.rem = np.array([r[1] for r in rows], dtype=np.int64)
        else:  # (k = 9: the k-mer is its root digit)
            self.dig, self.rem = np.asarray(dig, dtype=np.int64).reshape(4, 1), np.zeros(4, np.int64)
        self.codes = H.codes_from_digits(k, self.dig, self.rem if k % 9 else None)  # [4, k]: sibling v ends in nucleotide v
        assert (self.codes[:, :-1] == self.codes[0, :-1]).all() and self.codes[:, -1].tolist() == [0, 1, 2, 3]


FULL = (0, 1, 2, 3)


class WalkIndex:
    """one k: codes as inserted, genome masks, Table, model, root tables, query pools, branching anchors"""

    def __init__(self, k, uc_key, n_tail):
        self.k, self.L, self.R, self.W = k, k // 9, k % 9, W_of(k)
        L, R = self.L, self.R
        rng = np.random.default_rng(5000 + k)
        rows = Rows(k)
        self.families = []
        keys = 29 * np.arange(545) + 7
        r_of = H._r_of(keys)
        h1, h2 = H.hashpos()
        last_key = 16383
        # two early keys whose Bloom positions cover those of the last key: the root's first CC claims it, so prefix 2^18 - 1 is a plain group
        ka = int(np.flatnonzero((h1 == h1[last_key]) | (h2 == h1[last_key]))[0])
        kb = int(np.flatnonzero((h1 == h2[last_key]) | (h2 == h2[last_key]))[0])
        assert max(ka, kb) < keys[200] and ka not in keys and kb not in keys
        groups = L > 1 or R  # a root prefix can hold several rows
        gkind = "group" if L > 1 else "remainder"
        j_last = J_LAST if L > 1 else 15
        MID = (64 * 100, (1 << 18) - 8192)  # where the filler rows' next digit lies: behind families 1..99, in front of family J_LAST

        def family(head, j, stored, kind, where=""):
            f = Family(k, head, j, stored, kind, where)
            self.families.append(f)
            if len(f.stored):
                rows.add(f.dig[list(f.stored)], f.rem[list(f.stored)])
            return f

        def plain(r, c):
            if not groups and c > 1:  # k = 9: a k-mer is its root digit, so a key's rows are its prefixes
                rows.add(((r >> 4) << 4 | np.sort(rng.choice(16, min(c, 12), replace=False)))[:, None])
                return
            sd, sr = _suffixes(k, rng, c)
            rows.add(np.concatenate([np.full((len(sd), 1), r), sd], axis=1), sr)

        def fill(head, c):
            """c filler rows under `head`, between the families of small j and family j_last"""
            m = L - len(head)
            if m == 0:  # remainders 16 x + 4 .. 16 x + 15, x = 1 .. 14: no family's (those are 16 j | v)
                cand = np.array([16 * x + y for x in range(1, 15) for y in range(4, 16)])
                assert c <= len(cand) and 4 ** R >= 256
                rows.add(np.tile(head, (c, 1)), np.sort(rng.choice(cand, c, replace=False)))
                return
            d = np.sort(rng.choice(MID[1] - MID[0], c, replace=False)) + MID[0]
            rows.add(np.concatenate([np.tile(head, (c, 1)), d[:, None], rng.integers(0, 1 << 18, (c, m - 1))], axis=1), rng.integers(0, 4 ** R, c) if R else None)

        def group(r, c, first=0, last=False, one=False):
            """root prefix r as a group of c rows: `first` full families at its first rows, a filler row behind each where there are several (so
            that their first rows take every residue mod 8), one family at its last rows"""
            used = 0
            if one:
                family([r], 0, (3,), gkind, "group of 1")
                used = 1
            for t in range(first):
                family([r], t, FULL, gkind, "first" if t == 0 else "ladder")
                used += 4
                if first > 1:
                    rows.add([[r, 64 * t + 40] + [7] * (L - 2)], [1] if R else None)
                    used += 1
            if last:
                family([r], j_last, FULL, gkind, "last")
                used += 4
            assert c >= used
            if c > used:
                fill([r], c - used)

        roles = {}
        if groups:
            roles = {30: "one", 40: "g4", 50: "g5", 60: "g8", 70: "g9", 90: "gsub", 100: "twin", 101: "half"}
            if L > 1:
                roles.update({20: "node256", 120: "node300", 220: "deep", 320: "chain", 80: "g255"})
        else:
            roles = {90: "gsub", 100: "twin", 101: "half"}
        ci = 0
        for i in range(len(keys)):
            r = int(r_of[i])
            what = roles.get(i)
            if what is None:
                c = COUNTS[ci % len(COUNTS)] if i < len(keys) - 70 else 1 + i % 3  # (the last keys stay small: what two CCs leave is the root's UC)
                ci += 1
                plain(r, c)
            elif what in ("node256", "node300"):
                plain(r, 256 if what == "node256" else 300)
            elif what == "deep":  # 400 rows of their own second digits and 300 (k = 32: + the 1024 remainders of one path) under one
                plain(r, 400)
                d1 = 77
                self.deep = (r, d1)
                if L >= 3:
                    fill([r, d1], 300)
                    for j, s in enumerate(SUBSETS):
                        family([r, d1], j + 1, s, "node2")
                    if k == 32:
                        self.rem1024 = [r, d1, 0x2AAA5]
                        rows.add(np.tile(self.rem1024, (1024, 1)), np.arange(1024))
                        for base, where in ((0, "rem1024 first"), (508, "rem1024 mid"), (512, "rem1024 mid"), (1020, "rem1024 last")):
                            self.families.append(Family(k, self.rem1024, 0, FULL, "remainder", where, rem_base=base))
                else:  # L = 2: the second digit is the last one
                    rows.add([[r, d1]], [5] if R else None)
            elif what == "chain":  # 300 rows and more that share every digit but the last: a Node at every depth down to the last level
                head = [r] + [0x0F0F0 + 16 * d for d in range(1, L - 1)]
                self.chain = head
                fill(head, 300)
                for j, s in enumerate(SUBSETS):
                    if R:  # a remainder group of the last level: the family's digits are all fixed
                        family(head + [64 * (j + 1) + 1], 0, s, "remainder")
                    else:
                        family(head, j + 1, s, "lastlevel")
            elif what == "one":
                group(r, 1, one=True)
            elif what == "g4":
                group(r, 4, first=1)
            elif what == "g5":
                group(r, 5, first=1)
            elif what == "g8":
                group(r, 8, first=1, last=True)
            elif what == "g9":
                group(r, 9, first=1, last=True)
            elif what == "g255":
                group(r, 255, first=8, last=True)
            elif what == "gsub":  # two families per stored subset (the anchors' first nucleotide y gives each four predecessor sets)
                if not groups:  # k = 9: the siblings are four prefixes of one key (keys 29 i + 9 + 4 j: none of the others', and no two share their first seven nucleotides)
                    for j in range(14):
                        f = Family(k, [], 0, SUBSETS[j % 7], "lastlevel", dig=[(int(keys[i]) + 2 + 4 * j) << 4 | (v << 2) | 1 for v in range(4)])
                        self.families.append(f)
                        if len(f.stored):
                            rows.add(f.dig[list(f.stored)])
                else:
                    for j in range(14):
                        family([r], j + 1, SUBSETS[j % 7], gkind)
                    if L > 1:
                        fill([r], 9)
            elif what == "twin":  # two prefixes of one key, both stored
                plain(r, 6 if groups else 1)
                plain(r ^ 1, 6 if groups else 1)
            elif what == "half":  # two prefixes of one key, one stored: the other is absent in a CC that claims its key
                plain(r, 6 if groups else 1)
                self.half_absent = r ^ 1
        for key in (ka, kb):
            plain(key << 4 | 3, 2)
        # the last root prefix: a plain group whose last rows are a family -- the table's last rows
        rl = (1 << 18) - 1
        if groups:
            group(rl, 7, last=True)
            self.families[-1].where = "table end"
        else:
            f = Family(k, [], 0, FULL, "lastlevel", "table end", dig=[last_key << 4 | (v << 2) | 3 for v in range(4)])
            self.families.append(f)
            rows.add(f.dig)
        # the root's UC: tail keys of two rows, and the families of the UC kind under uc_key
        self.uc_r = uc_key << 4 | 5
        for key in 15900 + 3 * np.arange(n_tail):
            plain(int(key) << 4 | 9, 2)
        if groups:
            for j, s in enumerate(SUBSETS):
                family([self.uc_r], j + 1, s, "uc")
        else:
            rows.add([[self.uc_r]])
        # the empty prefix: root prefixes nothing is stored under (no k-mer of their key either)
        self.empty_r = 16350 << 4 | 6
        for e in range(2):  # one whose key a CC claims (absent in the CC: plain), one no CC claims (the walk searches the root's UC)
            if groups:
                f = Family(k, [self.empty_r if e else self.half_absent], 9, (), "empty")
            else:
                f = Family(k, [], 0, (), "empty", dig=[(16350 if e else self.half_absent >> 4) << 4 | (v << 2) | ((self.half_absent & 3) ^ 2) for v in range(4)])
            self.families.append(f)
        # the anchors a = y + s[:-1] and their stored predecessors N + a[:-1]: the predecessor sets in turn per number of successors
        self.anchors = []  # (codes [k], successors stored, predecessors stored, family)
        turn = {}
        pred = []
        for f in self.families:
            # (the last root prefix is nine T: with y = T a predecessor of its anchor would be one of the family's own siblings)
            for y in (range(3) if f.where == "table end" else range(4) if f.kind in (gkind, "empty", "lastlevel") else range(2)):
                t = turn.get(len(f.stored), len(f.stored))
                turn[len(f.stored)] = t + 1
                ps = SUBSETS[t % len(SUBSETS)]
                a = np.concatenate([[y], f.codes[0, :-1]]).astype(np.uint8)
                self.anchors.append((a, f.stored, ps, f))
                for v in ps:
                    pred.append(np.concatenate([[v], a[:-1]]).astype(np.uint8))
        codes = np.concatenate([rows.codes(), np.array(pred, dtype=np.uint8).reshape(-1, k)])
        # a short k-mer's neighbour can be a row by chance (k = 9: one k-mer in 60 is stored): rows that would give an anchor a predecessor it was
        # not given leave the index, unless a family or another anchor put them there (the CPU tests would then fail: no such case)
        meant = {f.codes[v].tobytes() for f in self.families for v in f.stored} | {p.tobytes() for p in pred}
        unmeant = {np.concatenate([[v], a[:-1]]).astype(np.uint8).tobytes() for a, _, ps, _ in self.anchors for v in range(4) if v not in ps} - meant
        self.codes = codes[[c.tobytes() not in unmeant for c in codes]] if k < 16 else codes

    # ---- what follows is computed once the index stands
    @functools.cached_property
    def table(self):
        return H.Table(self.k, self.codes)

    @functools.cached_property
    def model(self):
        return H.model(self.table.dig, self.k)

    @functools.cached_property
    def packed(self):
        """the distinct k-mers, packed, in table order"""
        t = self.table
        rem = [v & ((1 << t.rb) - 1) for v in t.keys] if t.rb else None
        return S.pack_codes(H.codes_from_digits(self.k, t.dig, rem))

    @functools.cached_property
    def masks(self):
        """genome set of every row, as bits 0..2"""
        i = np.arange(self.table.n, dtype=np.int64)
        return (1 + (i * 2654435761 >> 7) % 7).astype(np.int64)

    @functools.cached_property
    def tables(self):
        return root_tables(self.table, self.model)

    @functools.cached_property
    def row_class(self):
        """per row: 0 plain group of the root, 1 under a child Node, 2 root UC, 3 held by a CC at L = 1"""
        root, n = self.model[0], self.table.n
        cls = np.full(n, -1, dtype=np.int64)
        cls[root["uc"]] = 2
        for c in root["ccs"]:
            for r, kind, first, cnt in c["pref"].tolist():
                cls[first:first + cnt] = 3 if self.L == 1 else (1 if kind == H.NODE else 0)
        assert (cls >= 0).all()
        return cls


def root_tables(table, nodes):
    """{"special": [2^18] bool, "rstart": [2^18 + 1] u32, "rq": [2^18] u32 or None}, or None for a root without CCs (nothing is derived then)"""
    root, L = nodes[0], table.L
    if not root["ccs"]:
        return None
    h1, h2 = H.hashpos()
    R = np.arange(1 << 18)
    key = R >> 4
    first = np.full(1 << 18, -1, dtype=np.int64)
    kind_of = np.full(1 << 18, -1, dtype=np.int64)
    cnt_of = np.zeros(1 << 18, dtype=np.int64)
    cc_of = np.full(1 << 18, -2, dtype=np.int64)
    for c in range(len(root["ccs"]) - 1, -1, -1):
        cc = root["ccs"][c]
        b = np.unpackbits(np.frombuffer(cc["bloom"], dtype=np.uint8))[:H.MODULO].astype(bool)
        first[b[h1[key]] & b[h2[key]]] = c
        p = cc["pref"]
        kind_of[p[:, 0]], cnt_of[p[:, 0]], cc_of[p[:, 0]] = p[:, 1], p[:, 3], c
    held = (first >= 0) & (cc_of == first)
    assert ((cc_of >= 0) <= held).all()  # (a prefix lives in the first CC that claims its key)
    special = np.where(first < 0, len(root["uc"]) > 0, held & ((kind_of == H.NODE) | (L == 1)))
    lb = np.searchsorted(table.dig[:, 0], np.arange((1 << 18) + 1), side="left").astype(np.int64)
    cnt = np.diff(lb)
    plain = ~special
    # (what bft_root_range_ok checks: a plain prefix owns exactly the rows its entry says -- none for one no CC holds)
    assert (cnt[plain & held] == cnt_of[plain & held]).all() and (cnt[plain & held] <= 255).all() and (cnt[plain & ~held] == 0).all()
    rstart = lb.astype(np.uint32)
    rstart[:-1] |= np.where(special, SPECIAL, 0).astype(np.uint32)
    rq = None
    if L >= 2:
        rq = np.zeros(1 << 18, dtype=np.uint32)
        two = table.dig[:, 1] >> 16  # the next two key bits behind the root digit
        for r in np.flatnonzero(plain & (cnt >= 1) & (cnt <= 255)):
            seg = two[lb[r]:lb[r + 1]]
            assert (np.diff(seg) >= 0).all()
            q = [int(np.searchsorted(seg, j, side="left")) for j in (1, 2, 3)]
            rq[r] = q[0] | q[1] << 8 | q[2] << 16
    return {"special": special, "rstart": rstart, "rq": rq, "rspec": np.packbits(special, bitorder="little").view(np.uint32)}


@functools.lru_cache(maxsize=None)
def walk_index(k):
    """the index of k: the first (UC key, tail keys) for which the root keeps UC rows -- the families of the UC kind among them -- and claims the last key"""
    h1, h2 = H.hashpos()
    for uc_key in (16300, 16311, 16322, 16333):
        for n_tail in range(0, 40):
            ix = WalkIndex(k, uc_key, n_tail)
            # the root's assignment needs the root digits alone
            keyints = P.t_key_ints(ix.codes, k) if 2 * k > 62 else H.vector_keys(ix.codes, k).tolist()
            d0 = np.sort(np.array([v >> (2 * k - 18) for v in set(keyints)], dtype=np.int64))
            kk, kc = np.unique(d0 >> 4, return_counts=True)
            cc, blooms, _ = H.assign(kk, kc, len(d0))
            uc_keys = kk[cc < 0]
            uc_rows = int(kc[cc < 0].sum())
            if len(blooms) >= 2 and uc_key in uc_keys and len(uc_keys) >= 3 and uc_rows >= 3 and cc[-1] >= 0 and kk[-1] == 16383:
                return ix
    raise AssertionError("no walk index for k = %d" % k)


# ---- the two small indexes reused from the assembly cases -------------------------------------------------------------------------------------------
class SmallIndex:
    """an assembly case as a walk index: one genome"""

    def __init__(self, name):
        c = H.CASES[name]
        self.name, self.k, self.L, self.R, self.W = name, c.k, c.k // 9, c.k % 9, W_of(c.k)
        self.codes, self.table, self.model, self.packed = c.codes, c.table, c.model, c.packed

    @functools.cached_property
    def masks(self):
        return np.ones(self.table.n, dtype=np.int64)

    @functools.cached_property
    def tables(self):
        return root_tables(self.table, self.model)


SMALL = {"tiny": "root_254", "ncc_max": "ncc_max"}  # fewer than 255 rows: no CC, no root tables, the root not staged; the most CCs a root is known to reach (staged: see the docstring)


@functools.lru_cache(maxsize=None)
def small_index(which):
    return SmallIndex(SMALL[which])


# ---- query pools -----------------------------------------------------------------------------------------------------------------------------------
class Queries:
    """base: [m, k] codes with truth (present, row, genome mask) and, per pool kind, the positions in base"""

    def __init__(self, ix, pools):
        self.ix = ix
        names = [p for p in pools if len(pools[p])]
        self.base = np.concatenate([pools[p] for p in names]).astype(np.uint8)
        at = np.cumsum([0] + [len(pools[p]) for p in names])
        self.pool = {p: np.arange(at[i], at[i + 1]) for i, p in enumerate(names)}
        self.present, self.row = ix.table.rows_of(self.base)
        self.mask = np.where(self.present, ix.masks[np.where(self.present, self.row, 0).astype(np.int64)], 0)
        self.packed = S.pack_codes(self.base)
        keys = P.t_key_ints(self.base, ix.k)
        self.root_digit = np.array([v >> (2 * ix.k - 18) for v in keys], dtype=np.int64)
        tb = ix.tables
        self.special = tb["special"][self.root_digit] if tb else np.zeros(len(self.base), dtype=bool)


def _vary_tail(ix, rng, dig, rem, depth):
    """the rows with everything behind `depth` digits drawn again (absent with all but no probability: the truth decides)"""
    dig, rem = dig.copy(), rem.copy()
    L, R = ix.L, ix.R
    if depth < L:
        dig[:, depth:] = rng.integers(0, 1 << 18, (len(dig), L - depth))
    if R:
        rem = (rem + 1 + rng.integers(0, 4 ** R - 1, len(rem))) % (4 ** R)
    return dig, rem


@functools.lru_cache(maxsize=None)
def queries(k):
    ix = walk_index(k)
    t, L, R = ix.table, ix.L, ix.R
    rng = np.random.default_rng(900 + k)
    rem_all = np.array([v & ((1 << t.rb) - 1) for v in t.keys], dtype=np.int64) if t.rb else np.zeros(t.n, np.int64)
    cls, sp = ix.row_class, ix.tables["special"]

    def codes(dig, rem):
        return H.codes_from_digits(k, dig, rem if R else None)

    def rows_of_class(c, m):
        rows = np.flatnonzero(cls == c)
        if not len(rows):
            return rows
        edge = np.flatnonzero(np.diff(t.dig[rows, 0]) != 0)
        pick = np.unique(np.concatenate([[0, len(rows) - 1], edge, edge + 1, rng.choice(len(rows), min(m, len(rows)), replace=False)]))  # groups' first and last rows
        return rows[pick]
    pools = {p: np.zeros((0, k), np.uint8) for p in POOLS}
    plain = rows_of_class(0, 700)
    if len(plain):
        plain = np.unique(np.concatenate([plain, [t.n - 1]]))  # the table's last row
        assert cls[t.n - 1] == 0
        pools["plain_present"] = codes(t.dig[plain], rem_all[plain])
        d, r = _vary_tail(ix, rng, t.dig[plain[:300]], rem_all[plain[:300]], L - 1 if (L > 2 or R) else 1)
        pools["plain_absent"] = codes(d, r)
    # empty prefixes: keys a CC claims without holding the prefix (absent in the CC), next to stored prefixes and at random
    stored = np.zeros(1 << 18, dtype=bool)
    stored[t.dig[:, 0]] = True
    empty = np.flatnonzero(~sp & ~stored)
    pe = np.unique(np.concatenate([[ix.half_absent], empty[rng.choice(len(empty), 250, replace=False)]]))
    assert not sp[ix.half_absent] and not stored[ix.half_absent]
    pools["empty"] = codes(np.concatenate([pe[:, None], rng.integers(0, 1 << 18, (len(pe), L - 1))], axis=1), rng.integers(0, 4 ** R, len(pe)) if R else None)
    node = rows_of_class(1, 500) if L > 1 else rows_of_class(3, 600)
    pools["node_present"] = codes(t.dig[node], rem_all[node])
    if L > 1:
        d, r = _vary_tail(ix, rng, t.dig[node[:200]], rem_all[node[:200]], 1)
        pools["node_absent1"] = codes(d, r)
        if L > 2 or R:
            deep = node[(t.dig[node, 0] == ix.deep[0]) & (t.dig[node, 1] == ix.deep[1])] if L > 2 else node[:0]
            chain = node[t.dig[node, 0] == ix.chain[0]]
            pick = np.concatenate([deep[:80], chain[:80], node[:80]])
            d, r = _vary_tail(ix, rng, t.dig[pick], rem_all[pick], max(2, L - 1) if L > 2 else 2)
            if L > 2 and not R:
                d[:len(deep[:80]), 2:] = rng.integers(0, 1 << 18, (len(deep[:80]), L - 2))  # under the deep path: absent at the third level
            pools["node_absent_deep"] = codes(d, r)
    elif R:
        d, r = _vary_tail(ix, rng, t.dig[node[:200]], rem_all[node[:200]], 1)
        pools["node_absent_deep"] = codes(d, r)
    uc = np.flatnonzero(cls == 2)
    pools["uc_present"] = codes(t.dig[uc], rem_all[uc])
    noc = np.flatnonzero(sp & ~stored)  # no CC claims the key, the root has UC rows: the walk searches them
    pu = noc[rng.choice(len(noc), 150, replace=False)]
    ua = codes(np.concatenate([pu[:, None], rng.integers(0, 1 << 18, (len(pu), L - 1))], axis=1), rng.integers(0, 4 ** R, len(pu)) if R else None)
    if L > 1 or R:
        d, r = _vary_tail(ix, rng, t.dig[uc], rem_all[uc], 1)
        ua = np.concatenate([ua, codes(d, r)])
    pools["uc_absent"] = ua
    q = Queries(ix, pools)
    # what lands in a pool is what the pool is named after: drop the few redrawn suffixes that happen to be stored
    for p, want in (("plain_absent", False), ("empty", False), ("node_absent1", False), ("node_absent_deep", False), ("uc_absent", False)):
        if p in q.pool:
            q.pool[p] = q.pool[p][q.present[q.pool[p]] == want]
    if "node_absent1" in q.pool:  # ... and the few redrawn second digits that a row under the same root prefix has
        two = {(a, b) for a, b in t.dig[:, :2].tolist()}
        keys = P.t_key_ints(q.base[q.pool["node_absent1"]], k)
        q.pool["node_absent1"] = q.pool["node_absent1"][[(v >> (2 * k - 18), (v >> (2 * k - 36)) & H.M18) not in two for v in keys]]
    return q


@functools.lru_cache(maxsize=None)
def small_queries(which):
    """members, their neighbours and random k-mers of a small index: one pool each (nothing parks by plan there)"""
    ix = small_index(which)
    rng = np.random.default_rng(len(which))
    t = ix.table
    codes = S.unpack_codes(ix.packed, ix.k)
    mem = codes[np.unique(np.concatenate([[0, t.n - 1], rng.choice(t.n, min(t.n, 1500), replace=False)]))]
    near = mem[:400].copy()
    at = rng.integers(0, ix.k, len(near))
    near[np.arange(len(near)), at] = (near[np.arange(len(near)), at] + 1 + rng.integers(0, 3, len(near))) & 3
    q = Queries(ix, {"plain_present": mem, "plain_absent": near, "empty": rng.integers(0, 4, (300, ix.k), dtype=np.uint8)})
    return q


# ---- layouts -----------------------------------------------------------------------------------------------------------------------------------
LAYOUTS = ("none", "all", "fill_exact", "over", "step", "pass15", "carry", "same_word")
TAILS = (1, 63, 64, 65, 1023, 1024, 1025, 2 * CHUNK + 3 * 64 + 1, 17 * CHUNK + 63, 13 * CHUNK + 64)


def layouts_of(W):
    return [n for n in LAYOUTS if n != "over" or W >= 2]


def chunk_pattern(name, W):
    """[16, 64] bool: the parked lanes of every chunk of the layout (the same chunk over and over: the patterns hold for 12 and 16 wavefronts per
    workgroup and for any dealing).  `step` departs from "one parked lane per pass": it parks QCAP / 16 a pass and leaves one pass out, 15 QCAP / 16
    a chunk, so that the queue runs over within the three or four chunks a wavefront of one workgroup takes (one lane a pass would need five chunks
    at W = 1) and at another pass in every chunk (sixteen a chunk would run over exactly at the chunk's edge where QCAP is 16)."""
    Q = QCAP[W]
    p = np.zeros((PASSES, 64), dtype=bool)
    lanes = (37 * np.arange(64) + 11) % 64  # a fixed scatter of the lanes
    if name == "all":
        p[:] = True
    elif name == "fill_exact":  # exactly QCAP in one pass, then one
        p[2, lanes[:Q]] = True
        p[3, 41] = True
    elif name == "over":  # QCAP + 1 in one pass while the queue holds five
        p[1, lanes[:5]] = True
        p[2, lanes[:Q + 1]] = True
    elif name == "step":  # QCAP / 16 a pass, one pass left out: the queue runs over in the middle of a chunk, elsewhere in each
        for ps in range(PASSES):
            if ps != 5:
                p[ps, lanes[(3 * ps) % 50:(3 * ps) % 50 + Q // 16]] = True
    elif name == "pass15":
        p[15, lanes[:Q // 2 + 1]] = True
        p[15, 63] = True
    elif name == "carry":  # a few parked late in a chunk; the wavefront's next chunk fills the queue in its first pass
        p[14, lanes[:3]] = True
        p[0, np.roll(lanes, -10)[:Q - 2]] = True
    elif name == "same_word":  # per word: parked present, parked absent, direct present, direct absent, interleaved
        p[:, np.arange(64) % 8 < 2] = True
    else:
        assert name == "none"
    return p


def layout_mask(name, W, n):
    pat = chunk_pattern(name, W).ravel()
    return np.tile(pat, (n + CHUNK - 1) // CHUNK)[:n]


def tail_mask(n):
    """the last query parked, and one lane in seven before it"""
    m = (np.arange(n) * 2654435761 >> 9) % 7 == 0
    m[n - 1] = True
    return m


def fill_batch(q, parked, want_present=None, seed=0):
    """positions in q.base for a batch whose lane i parks iff parked[i] (and is present iff want_present[i], where given): the pools in turn"""
    n = len(parked)
    idx = np.zeros(n, dtype=np.int64)
    sp, pr = q.special, q.present
    for park in (False, True):
        for pres in ((False, True) if want_present is not None else (None,)):
            sel = np.flatnonzero((parked == park) & ((want_present == pres) if pres is not None else True))
            if not len(sel):
                continue
            names = [p for p in (PARKED_POOLS if park else DIRECT_POOLS) if p in q.pool and len(q.pool[p])]
            cand = np.concatenate([q.pool[p] for p in names])
            cand = cand[sp[cand] == park]
            if pres is not None:
                cand = cand[pr[cand] == pres]
            assert len(cand), (park, pres)
            # the pools in turn, each walked through in order
            order = np.random.default_rng(seed + 2 * park + (pres or 0)).permutation(len(cand))
            idx[sel] = cand[order[np.arange(len(sel)) % len(cand)]]
    return idx


def has_direct_present(q):
    return bool(((~q.special) & q.present).any())


def batch(k, name, n=N_LAYOUT):
    """(positions in queries(k).base, parked mask) of a layout"""
    q = queries(k)
    W = W_of(k)
    if name == "tails":
        parked = tail_mask(n)
    else:
        parked = layout_mask(name, W, n)
    want = None
    if name == "same_word":
        want = np.tile(np.array([1, 0, 1, 0, 0, 1, 0, 1], dtype=bool), (n + 7) // 8)[:n]  # lanes 0, 1 park: present, absent; the others: present and absent in turn
        if not has_direct_present(q):  # L = 1: what a CC holds is special, so no lane that stays is present
            want = np.where(parked, want, False)
    idx = fill_batch(q, parked, want, seed=len(name))
    assert (q.special[idx] == parked).all()
    return idx, parked


# ---- the queue and chunk bookkeeping of query_body ----------------------------------------------------------------------------------------------
def simulate(special, W, waves_per_wg, n_wg, claim_seed=None):
    """Replay of query_body's control flow for the batch whose lane i parks iff special[i], on n_wg workgroups of waves_per_wg wavefronts: static
    dealing (chunk, chunk + n_waves, ...) or, with claim_seed, a claimed one (first chunk by number, the others in a random order of arrival)."""
    special = np.asarray(special, dtype=bool)
    n, Q = len(special), QCAP[W]
    n_chunks, n_waves = (n + CHUNK - 1) // CHUNK, waves_per_wg * n_wg
    deal = [[w] for w in range(min(n_waves, n_chunks))]
    if n_waves < n_chunks:
        if claim_seed is None:
            deal = [list(range(w, n_chunks, n_waves)) for w in range(n_waves)]
        else:
            rng = np.random.default_rng(claim_seed)
            for c in range(n_waves, n_chunks):
                deal[int(rng.integers(0, n_waves))].append(c)
    out = {"drains_open": 0, "drains_final": 0, "inline": 0, "max_queued": 0, "late_lds": 0, "late_bitmap_end": 0, "late_bitmap_earlier": 0,
           "max_chunks": max(len(d) for d in deal), "claimed": bool(n_waves < n_chunks and claim_seed is not None)}
    counts = np.zeros(n_chunks * PASSES, dtype=np.int64)
    full = special[:(n // 64) * 64].reshape(-1, 64).sum(axis=1)
    counts[:len(full)] = full
    if n % 64:
        counts[len(full)] = special[(n // 64) * 64:].sum()
    for chunks in deal:
        queue = []  # the chunk of every entry parked
        for chunk in chunks:
            for ps in range(PASSES):
                if chunk * CHUNK + ps * 64 >= n:
                    break
                np_ = int(counts[chunk * PASSES + ps])
                if not np_:
                    continue
                if len(queue) + np_ > Q and queue:  # drain(true) of a queue that holds entries (one of an empty queue walks nothing)
                    out["drains_open"] += 1
                    here = sum(1 for c in queue if c == chunk)
                    out["late_lds"] += here
                    out["late_bitmap_earlier"] += len(queue) - here
                    queue = []
                if np_ > Q:
                    out["inline"] += np_
                    out["late_lds"] += np_
                else:
                    queue += [chunk] * np_
                    out["max_queued"] = max(out["max_queued"], len(queue))
        if queue:
            out["drains_final"] += 1
            out["late_bitmap_end"] += len(queue)
    return out


DEALINGS = (("static", 16), ("static", 12), ("claimed", 16), ("claimed", 12))
REGIME = {"none": (), "all": ("late_lds",), "fill_exact": ("drains_open", "late_lds"), "over": ("inline", "drains_open"), "step": ("drains_open", "late_lds", "late_bitmap_earlier"),
          "pass15": ("drains_open", "late_bitmap_earlier", "late_bitmap_end"), "carry": ("late_bitmap_earlier", "late_lds", "drains_open"),
          "same_word": ("late_lds",)}


# ---- branching -----------------------------------------------------------------------------------------------------------------------------------
def branching_truth(ix, codes):
    """counts [m] = successors << 4 | predecessors, by set membership of the eight neighbours"""
    codes = np.asarray(codes, dtype=np.uint8).reshape(-1, ix.k)
    m = len(codes)
    cr, cl = np.zeros(m, np.int64), np.zeros(m, np.int64)
    for v in range(4):
        col = np.full((m, 1), v, dtype=np.uint8)
        cr += ix.table.rows_of(np.concatenate([codes[:, 1:], col], axis=1))[0]
        cl += ix.table.rows_of(np.concatenate([col, codes[:, :-1]], axis=1))[0]
    return (cr << 4 | cl).astype(np.uint8)


BRANCH_SIZES = (1, 63, 64, 65, 767, 768, 769, 1023, 1024, 1025)
BRANCH_GRID_N = 5003  # with "test_walk_grid" 2: three passes of the grid loop at 1024 threads, four at 768


@functools.lru_cache(maxsize=None)
def branching_base(k):
    """(codes [m, k], counts [m], number of anchors): the anchors of the families first, then the whole base of the query pools -- so that a layout's
    batch, positions in that base, is a branching batch too (layout_branching_idx) --, then successors' and predecessors' places of members"""
    ix = walk_index(k)
    q = queries(k)
    a = np.array([x[0] for x in ix.anchors], dtype=np.uint8)
    rng = np.random.default_rng(31 * k)
    mem = q.base[rng.choice(len(q.base), 500, replace=False)]
    nxt = np.concatenate([mem[:250, 1:], rng.integers(0, 4, (250, 1), dtype=np.uint8)], axis=1)  # a successor's place of a member
    prv = np.concatenate([rng.integers(0, 4, (250, 1), dtype=np.uint8), mem[250:, :-1]], axis=1)
    base = np.concatenate([a, q.base, nxt, prv])
    return base, branching_truth(ix, base), len(a)


def layout_branching_idx(k, name, n):
    """the layout's batch of n k-mers as positions in branching_base(k)"""
    return len(walk_index(k).anchors) + batch(k, name, n)[0]


@functools.lru_cache(maxsize=None)
def small_branching_base(which):
    q = small_queries(which)
    return q.base, branching_truth(q.ix, q.base), 0


def branching_batch(nbase, n_anchors, n, seed=0):
    """positions in the base: the anchors first (all of them where n allows), then the base over and over in a shuffled order"""
    rng = np.random.default_rng(1000 + n + seed)
    idx = rng.integers(0, nbase, n)
    m = min(n, n_anchors)
    idx[:m] = np.arange(m)
    return idx


# ---- CPU tests -----------------------------------------------------------------------------------------------------------------------------------
def test_the_k_set():
    """key widths 1..4, both remainder kinds, L = 1, last words that are exactly full"""
    assert {W_of(k) for k in KS} == {1, 2, 3, 4}
    assert {(W_of(k), k % 9 != 0) for k in KS} >= {(w, r) for w in (1, 2, 3) for r in (False, True)} | {(4, False)}
    assert [k for k in KS if k // 9 == 1] == [9, 13] and {2 * k % 64 for k in (32, 64, 96)} == {0}
    assert set(FULL_KS) <= set(KS) and {W_of(k) for k in FULL_KS} == {1, 2}


@pytest.mark.parametrize("k", KS)
def test_walk_index_has_every_container(k):
    ix = walk_index(k)
    t, nodes = ix.table, ix.model
    root = nodes[0]
    L, R = ix.L, ix.R
    assert (5000 if k > 9 else 3000) <= t.n <= 22000 and len(root["ccs"]) >= 2 and 3 <= len(root["uc"]) < 255
    pref = np.concatenate([c["pref"] for c in root["ccs"]])
    assert len(np.unique(t.dig[:, 0])) < (2000 if k > 9 else 6000)  # many empty root prefixes
    assert ((1 + (np.arange(t.n) * 2654435761 >> 7) % 7) == ix.masks).all() and set(np.unique(ix.masks)) == set(range(1, 8))
    last = pref[pref[:, 0] == (1 << 18) - 1]
    assert len(last) == 1 and last[0, 1] == H.GROUP and last[0, 2] + last[0, 3] == t.n  # a group ends at the table's last row
    if L > 1:
        groups = pref[pref[:, 1] == H.GROUP]
        assert len(groups) >= 400 and set(COUNTS) <= set(groups[:, 3].tolist())
        assert (pref[:, 1] == H.NODE).sum() >= 4
        depth = max(len(nd["path"]) for nd in nodes)
        assert depth == L - 1
        if L >= 3:
            two = [nd for nd in nodes if nd["path"] == tuple(ix.deep)]
            assert len(two) == 1 and two[0]["_rows"] >= 256  # the parked walk descends two levels
        if k == 32:
            nd = [nd for nd in nodes if nd["path"] == tuple(ix.rem1024[:2])][0]
            p = np.concatenate([c["pref"] for c in nd["ccs"]])
            assert p[p[:, 0] == ix.rem1024[2]][0, 3] == 1024
    else:
        assert len(nodes) == 1 and (pref[:, 1] == H.GROUP).all()
        assert (pref[:, 3].max() > 200) == (R != 0)


@pytest.mark.parametrize("k", KS)
def test_root_tables_follow_the_rule(k):
    """special(r) by the rule; the number of plain prefixes is the host restatement's; both kinds of prefix occur among the stored and the empty"""
    ix = walk_index(k)
    tb = ix.tables
    sp = tb["special"]
    lib = H.hostlib()
    lib.bft_hosttest_root_direct.argtypes = [C.c_void_p, C.c_int]
    lib.bft_hosttest_root_plain.restype = C.c_uint64
    lib.bft_hosttest_root_plain.argtypes = [C.c_void_p]
    lib.bft_hosttest_query.restype = C.c_uint64
    lib.bft_hosttest_query.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    km = np.ascontiguousarray(ix.packed)
    h = lib.bft_hosttest_build(km.ctypes.data, len(km), k, 0, 0)
    try:
        lib.bft_hosttest_root_direct(h, 3)
        assert lib.bft_hosttest_root_plain(h) == int((~sp).sum())
        q = queries(k)
        pq = np.ascontiguousarray(q.packed)
        bits, rows = np.zeros((len(pq) + 7) // 8, np.uint8), np.zeros(len(pq), np.uint32)
        lib.bft_hosttest_query(h, pq.ctypes.data, len(pq), bits.ctypes.data, rows.ctypes.data)
        assert (np.unpackbits(bits, bitorder="little")[:len(pq)].astype(bool) == q.present).all()
        assert (rows == q.row).all()
    finally:
        lib.bft_hosttest_free(h)
    stored = np.zeros(1 << 18, dtype=bool)
    stored[ix.table.dig[:, 0]] = True
    assert (sp & stored).any() and (sp & ~stored).any() and (~sp & ~stored).any()
    assert (~sp & stored).any() == (ix.L > 1)
    assert (tb["rstart"][:-1] & SPECIAL != 0).tolist() == sp.tolist() and tb["rstart"][-1] == ix.table.n
    assert (tb["rq"] is not None) == (ix.L > 1)
    if tb["rq"] is not None:
        nz = tb["rq"][tb["rq"] != 0]
        assert len(nz) > 300 and not tb["rq"][sp].any()
        assert len({(int(x) & 255 == 0, (int(x) >> 16) & 255 == 0) for x in nz}) >= 2  # empty first quarters and others


def test_small_indexes():
    tiny, big = small_index("tiny"), small_index("ncc_max")
    assert tiny.table.n < 255 and not tiny.model[0]["ccs"] and tiny.tables is None
    assert len(big.model[0]["ccs"]) == 20  # (test_most_ccs_a_node_can_reach: no node passes 32 CCs, so the root is staged wherever it has a CC)
    assert big.tables is not None and big.tables["rq"] is None
    for which in SMALL:
        q = small_queries(which)
        assert q.present.any() and not q.present.all()


@pytest.mark.parametrize("k", KS)
def test_pools_are_what_they_are_named_after(k):
    q = queries(k)
    ix = q.ix
    L, R = ix.L, ix.R
    want = {"empty", "node_present", "uc_present", "uc_absent"}
    if L > 1:
        want |= {"plain_present", "plain_absent", "node_absent1"}
    if L > 2 or R:
        want.add("node_absent_deep")
    assert {p for p in q.pool if len(q.pool[p]) >= 3} >= want, (sorted(q.pool), want)
    for p in q.pool:
        i = q.pool[p]
        assert (q.special[i] == (p in PARKED_POOLS)).all(), p
        assert (q.present[i] == p.endswith("present")).all(), p
    cls = ix.row_class
    assert (cls[q.row[q.pool["uc_present"]]] == 2).all() and (cls[q.row[q.pool["node_present"]]] == (1 if L > 1 else 3)).all()
    if L > 1:
        i = q.pool["node_absent1"]  # absent at level 1: no row shares the first two digits
        two = {(a, b) for a, b in ix.table.dig[:, :2].tolist()}
        keys = P.t_key_ints(q.base[i], k)
        sh = 2 * k - 36
        assert all(((v >> sh) >> 18, (v >> sh) & H.M18) not in two for v in keys)
    if "node_absent_deep" in q.pool and L > 2:
        i = q.pool["node_absent_deep"]
        two = {(a, b) for a, b in ix.table.dig[:, :2].tolist()}
        sh = 2 * k - 36
        assert all(((v >> sh) >> 18, (v >> sh) & H.M18) in two for v in P.t_key_ints(q.base[i], k))
    assert len({int(m) for m in q.mask[q.present]}) >= 5  # colour sets differ
    assert (q.row[q.present] != ABSENT).all() and (q.row[~q.present] == ABSENT).all()
    assert ix.table.n - 1 in q.row.tolist()  # the table's last row is asked for


@pytest.mark.parametrize("k", KS)
def test_every_layout_reaches_its_regime(k):
    """every (layout, dealing) the GPU file runs with "test_walk_grid" 1: the counters of its regime are not zero, every wavefront's chunks several"""
    W, Q = W_of(k), QCAP[W_of(k)]
    assert "over" in layouts_of(W) or W == 1
    for name in layouts_of(W):
        idx, parked = batch(k, name)
        q = queries(k)
        for how, wpw in DEALINGS:
            for seed in ((None,) if how == "static" else (1, 2, 3)):
                s = simulate(parked, W, wpw, 1, claim_seed=seed)
                assert s["max_chunks"] >= 3 and s["claimed"] == (how == "claimed"), (name, how, s)
                for ctr in REGIME[name]:
                    assert s[ctr] > 0, (name, how, wpw, ctr, s)
                if name == "none":
                    assert not any(s[c] for c in ("drains_open", "drains_final", "inline", "late_lds", "late_bitmap_end", "late_bitmap_earlier"))
                if name == "fill_exact":
                    assert s["max_queued"] == Q and s["inline"] == 0
                if name == "all":
                    assert (s["inline"] > 0) == (W >= 2) and (W >= 2 or s["max_queued"] == Q)
                if name in ("step", "pass15", "carry"):
                    assert s["inline"] == 0
        if name == "same_word":
            # every full word holds parked present, parked absent and direct absent lanes -- and direct present ones where the index has any
            n64 = len(idx) // 64 * 64
            pk, pr = parked[:n64].reshape(-1, 64), q.present[idx][:n64].reshape(-1, 64)
            assert (pk & pr).any(axis=1).all() and (pk & ~pr).any(axis=1).all() and (~pk & ~pr).any(axis=1).all()
            assert (~pk & pr).any(axis=1).all() == has_direct_present(q) == (k // 9 > 1)
        if name == "pass15":
            assert not parked.reshape(-1)[:len(parked) // CHUNK * CHUNK].reshape(-1, PASSES, 64)[:, :15].any()
    # uncapped, the grid covers the batch: every wavefront one chunk, no claim
    s = simulate(batch(k, "all")[1], W, 16, 512)
    assert s["max_chunks"] == 1


@pytest.mark.parametrize("k", KS)
def test_tails_park_the_last_query(k):
    W = W_of(k)
    assert {n % 64 for n in TAILS} >= {1, 63, 0} and any((n - 1) % CHUNK < 64 and n > CHUNK for n in TAILS)  # a last chunk of one pass
    for n in TAILS:
        idx, parked = batch(k, "tails", n)
        assert parked[-1] and queries(k).special[idx[-1]]
        s = simulate(parked, W, 16, 1)
        assert s["late_bitmap_end"] + s["late_lds"] + s["late_bitmap_earlier"] == parked.sum()
        assert s["late_bitmap_end"] > 0 or s["inline"] > 0


# per key width: (drains with the chunk open, late answers into an earlier chunk's bitmap, inline walks, most entries queued) of carry, over and
# fill_exact on one workgroup of 16 wavefronts, static dealing -- the figures the change log quotes
COUNTERS = {(1, "carry"): (83, 102, 0, 62), (1, "fill_exact"): (83, 34, 0, 64),
            (2, "carry"): (83, 102, 0, 30), (2, "over"): (50, 0, 1650, 5), (2, "fill_exact"): (83, 34, 0, 32),
            (3, "carry"): (83, 102, 0, 14), (3, "over"): (50, 0, 850, 5), (3, "fill_exact"): (83, 34, 0, 16),
            (4, "carry"): (83, 102, 0, 14), (4, "over"): (50, 0, 850, 5), (4, "fill_exact"): (83, 34, 0, 16)}


@pytest.mark.parametrize("k", (31, 36, 72, 126))
def test_counters_of_carry_over_and_fill_exact(k):
    W = W_of(k)
    for name in ("carry", "over", "fill_exact"):
        if name in layouts_of(W):
            s = simulate(batch(k, name)[1], W, 16, 1)
            assert (s["drains_open"], s["late_bitmap_earlier"], s["inline"], s["max_queued"]) == COUNTERS[(W, name)], (W, name, s)


def test_simulate_on_hand_made_batches():
    """the replay against cases counted by hand"""
    m = np.zeros(3 * CHUNK, dtype=bool)
    m[5] = True  # one lane parked in chunk 0
    s = simulate(m, 1, 1, 1)  # one wavefront: three chunks, the entry is drained at the end -- into the bitmap
    assert (s["max_chunks"], s["drains_final"], s["late_bitmap_end"], s["drains_open"], s["late_lds"]) == (3, 1, 1, 0, 0)
    m[CHUNK:CHUNK + 64] = True  # a full pass in chunk 1: 1 + 64 > 64 drains the carried entry into the bitmap while chunk 1 is open
    s = simulate(m, 1, 1, 1)
    assert (s["drains_open"], s["late_bitmap_earlier"], s["late_lds"], s["late_bitmap_end"], s["max_queued"]) == (1, 1, 0, 64, 64)
    s = simulate(m, 2, 1, 1)  # W = 2: 64 > 32 lanes walk inline, the queue keeps its entry until the end
    assert (s["inline"], s["late_lds"], s["drains_open"], s["late_bitmap_earlier"], s["late_bitmap_end"]) == (64, 64, 1, 1, 0)
    s = simulate(m, 1, 16, 1)  # sixteen wavefronts, three chunks: one each
    assert s["max_chunks"] == 1 and s["late_bitmap_end"] == 65 and s["late_bitmap_earlier"] == 0


@pytest.mark.parametrize("k", KS)
def test_branching_families(k):
    ix = walk_index(k)
    t, L, R = ix.table, ix.L, ix.R
    base, counts, na = branching_base(k)
    assert na == len(ix.anchors) >= 40
    # every anchor has exactly the successors and predecessors it was given
    for (a, succ, pred, f), c in zip(ix.anchors, counts[:na].tolist()):
        assert (c >> 4, c & 15) == (len(succ), len(pred)), (f.kind, f.where, succ, pred, c)
        ps, _ = t.rows_of(f.codes)
        assert tuple(np.flatnonzero(ps).tolist()) == tuple(succ)
    pairs = {(c >> 4, c & 15) for c in counts[:na].tolist()}
    assert pairs == {(a, b) for a in range(5) for b in range(5)}, sorted(set((a, b) for a in range(5) for b in range(5)) - pairs)
    kinds = {f.kind for f in ix.families}
    want = {"empty"} | ({"group", "uc"} if L > 1 else set()) | ({"node2"} if L >= 3 else set())
    want |= {"lastlevel"} if not R else {"remainder"}
    if L == 1 and R:
        want |= {"uc"}
    assert kinds >= want, (kinds, want)
    for kind in want - {"empty"}:
        assert {f.stored for f in ix.families if f.kind == kind} >= set(SUBSETS), kind
        assert {x[2] for x in ix.anchors if x[3].kind == kind} >= set(SUBSETS) or kind not in ("group",), kind
    assert {x[2] for x in ix.anchors} >= set(SUBSETS)
    # the containers the kinds are named after
    cls = ix.row_class
    for f in ix.families:
        rows = t.rows_of(f.codes[list(f.stored)])[1].astype(np.int64) if len(f.stored) else np.zeros(0, np.int64)
        if f.kind == "group":
            assert (cls[rows] == 0).all()
        elif f.kind == "uc":
            assert (cls[rows] == 2).all()
        elif f.kind == "node2":
            assert (cls[rows] == 1).all() and (t.dig[rows, :2] == np.array(ix.deep)).all()
        elif f.kind in ("lastlevel", "remainder") and L > 1 and not f.where.startswith("rem1024"):
            assert (cls[rows] == 1).all() and (t.dig[rows, :L - 1] == np.array(ix.chain)).all()
        elif f.kind == "empty":
            assert not len(rows) and not np.isin(f.dig[:, 0], t.dig[:, 0]).any()
    assert {bool(ix.tables["special"][f.dig[0, 0]]) for f in ix.families if f.kind == "empty"} == {False, True}
    # the placements
    if L > 1 or R:
        lb = np.searchsorted(t.dig[:, 0], np.arange((1 << 18) + 1))

        def span(f):
            rows = t.rows_of(f.codes)[1].astype(np.int64)
            assert (np.diff(rows) == 1).all()
            r0 = int(f.dig[0, 0])
            return int(rows[0]), int(lb[r0]), int(lb[r0 + 1])
        placed = {}
        for f in ix.families:
            if f.where in ("first", "last", "ladder", "table end"):
                placed.setdefault(f.where, []).append(span(f))
            if f.where == "group of 1":
                r0 = int(f.dig[0, 0])
                assert lb[r0 + 1] - lb[r0] == 1
                placed["one"] = True
        assert all(a == lo for a, lo, hi in placed["first"]) and all(a + 4 == hi for a, lo, hi in placed["last"])
        sizes_first = {hi - lo for a, lo, hi in placed["first"]}
        assert all(a + 4 == hi == t.n for a, lo, hi in placed["table end"])
        if L > 1:
            assert sizes_first >= {4, 5, 8, 9, 255} and {hi - lo for a, lo, hi in placed["last"]} >= {8, 9, 255} and placed["one"]
            starts = [a for a, lo, hi in placed["ladder"] + placed["first"]]
            assert {a % 8 for a in starts} == set(range(8))  # a family across a multiple of 8 rows, and of 4
            assert any(a // 8 != (a + 3) // 8 for a in starts) and any(a // 4 != (a + 3) // 4 and a // 8 == (a + 3) // 8 for a in starts)
        else:
            assert sizes_first >= {4, 5, 8, 9} and placed["one"]
    if k == 32:  # the remainder group of 1024 rows: families at its first rows, across its middle and at its last rows
        rows = np.flatnonzero((t.dig == np.array(ix.rem1024)).all(axis=1))
        assert len(rows) == 1024 and (np.diff(rows) == 1).all()
        got = {f.where: int(t.rows_of(f.codes)[1][0]) - int(rows[0]) for f in ix.families if f.where.startswith("rem1024")}
        assert got["rem1024 first"] == 0 and got["rem1024 last"] == 1020 and got["rem1024 mid"] in (508, 512)
        assert sum(f.where == "rem1024 mid" for f in ix.families) == 2


@pytest.mark.parametrize("k", KS)
def test_branching_batches_hold_every_anchor(k):
    base, counts, na = branching_base(k)
    for n in BRANCH_SIZES + (BRANCH_GRID_N,):
        idx = branching_batch(len(base), na, n)
        assert len(idx) == n and (n < na or (np.sort(idx[:na]) == np.arange(na)).all())
    assert (BRANCH_GRID_N + 1023) // 1024 > 2 * 2 and (BRANCH_GRID_N + 767) // 768 > 2 * 3  # several passes of the grid loop on two workgroups
    assert {n % 64 for n in BRANCH_SIZES} >= {0, 1, 63} and {767, 768, 769, 1023, 1024, 1025} <= set(BRANCH_SIZES)
    c = counts.astype(np.int64)
    assert ((c >> 4 > 1) | (c & 15 > 1)).any() and not ((c >> 4 > 1) | (c & 15 > 1)).all()
