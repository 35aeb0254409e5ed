"""CPU-side tests of the bubbles on the compacted coloured graph and of the k-mer -> segment table (no GPU).  The truth model of include/bft_gpu.h's
definition of bft_gpu_unitig_bubbles -- out(X), the predicate rule by rule, the reported mirror, the four counts -- written from that text alone over
the five arrays of test_cgraph_host.Graph.arrays(), and segment_of over its members.  The definition's invariants proved on every index the GPU tests
use: the mirror of a reported bubble satisfies the predicate and is the one not reported, no palindromic segment is a branch, at most one bubble per
source, segment_of inverts members.  A planted-variant case whose truth is known from construction: substitutions (one tri-allelic) and one insertion in
four genomes of one repeat-free ancestor.  The hand-made link tables, one per rule, and the table just past the capped grid that the GPU tests run.
The checker the GPU tests compare with, shown to report doctored results; the new names in the headers and SIGNATURES, the symbols exported; the
k_bb_* kernels without scratch memory, spills or LDS; NULL arguments refused before anything touches a device.  tests/test_gpu_bubbles.py runs the
cases of this file on the GPU."""
import ctypes as C
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_cgraph_host as G  # noqa: E402
import test_unitigs_host as H  # noqa: E402

from bloomfiltertrie_amd import _lib, synth as S  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = {"k_bb_find", "k_bb_emit", "k_bb_fill", "k_bb_segof"}
NAMES = ("bft_gpu_unitig_bubbles", "bft_gpu_unitig_bubbles_dev", "bft_gpu_unitig_segment_of", "bft_gpu_unitig_segment_of_dev")
NONE = 0xFFFFFFFF
PLANTED_KS = (27, 63)
GRID_LANES = 524288  # 2048 workgroups of 256: the capped grid of the launch kit


class Bubbles:
    """The definition, literally, over (seg_off, seqs, link_off, links) at k.  A list that is no list inside links (the device form's malformed input)
    makes "no bubble", as the definition's device form says."""

    def __init__(self, k, seg_off, seqs, link_off, links, max_branch_chars=0):
        self.k, self.max = k, int(max_branch_chars)
        self.so = [int(x) for x in seg_off]
        self.lo = [int(x) for x in link_off]
        self.lk = [int(x) for x in links]
        self.text = bytes(np.asarray(seqs, dtype=np.uint8)).decode()
        self.n2 = 2 * (len(self.so) - 1)

    def out(self, X):
        a, b = self.lo[X], self.lo[X + 1]
        return self.lk[a:b] if a <= b <= len(self.lk) else None

    def chars(self, i):
        return self.so[i + 1] - self.so[i]

    def palindromic(self, i):
        s = self.text[self.so[i]:self.so[i + 1]]
        return len(s) == self.k and s == H.rc(s)

    def predicate(self, A):
        """(Z, [B_1 .. B_m]) when A is the source of a bubble (whichever mirror), else None"""
        n2 = self.n2
        B = self.out(A)
        if B is None or not 2 <= len(B) <= 4 or any(b >= n2 for b in B):
            return None
        Z = None
        for b in B:
            o = self.out(b)
            if o is None or len(o) != 1 or (Z is not None and o[0] != Z):
                return None
            Z = o[0]
            if self.out(b ^ 1) != [A ^ 1]:
                return None
        if Z >= n2:
            return None
        zin = self.out(Z ^ 1)
        if zin is None or len(zin) != len(B) or any(t >= n2 or (t ^ 1) not in B for t in zin):
            return None
        segs = [A >> 1, Z >> 1] + [b >> 1 for b in B]
        if len(set(segs)) != len(segs):
            return None
        if self.palindromic(A >> 1) or self.palindromic(Z >> 1):
            return None
        if self.max and any(self.chars(b >> 1) > self.max for b in B):
            return None
        return Z, B

    @functools.lru_cache(maxsize=None)
    def reported(self):
        """(records [[A, Z, B_1 .. B_4], ...] in ascending A, counts [4])"""
        recs, branches, subst, longest = [], 0, 0, 0
        for A in range(self.n2):
            if self.lo[A + 1] - self.lo[A] < 2:
                continue
            hit = self.predicate(A)
            if hit is None or not A < (hit[0] ^ 1):
                continue
            Z, B = hit
            recs.append([A, Z] + B + [NONE] * (4 - len(B)))
            lens = [self.chars(b >> 1) for b in B]
            branches += len(B)
            subst += all(x == 2 * self.k - 1 for x in lens)
            longest = max(longest, max(lens))
        return recs, [len(recs), branches, subst, longest]


def segment_of(k, seg_off, members, n_rows):
    """(seg_of, pos) per row, from the members and the character offsets"""
    seg_of, pos = [NONE] * n_rows, [NONE] * n_rows
    for i in range(len(seg_off) - 1):
        a, b = int(seg_off[i]) - i * (k - 1), int(seg_off[i + 1]) - (i + 1) * (k - 1)
        for j in range(a, b):
            v = int(members[j])
            seg_of[v >> 1], pos[v >> 1] = 2 * i + (v & 1), j - a
    return seg_of, pos


def check(want, got):
    """problems of got = (records [n, 6], counts) as the truth want = Bubbles.reported(); empty when it is exactly that"""
    recs, counts = want
    have = [[int(x) for x in r] for r in got[0]]
    if have == recs and [int(x) for x in got[1]] == counts:
        return []
    out = []
    by_source = {r[0]: r for r in have}
    for r in recs:
        h = by_source.get(r[0])
        if h is None:
            mirror = by_source.get(r[1] ^ 1)
            out.append(f"bubble at source {r[0]} missing" + (": its mirror is reported" if mirror is not None and mirror[1] == r[0] ^ 1 else ""))
        elif h != r:
            out.append(f"bubble at source {r[0]}: " + ("branches out of order" if h[:2] == r[:2] and sorted(h[2:]) == sorted(r[2:]) else f"{h}, not {r}"))
    want_sources = {r[0] for r in recs}
    out += [f"source {r[0]} is none" for r in have if r[0] not in want_sources]
    if not out and have != recs:
        out.append("records: order or multiplicity differs")
    if [int(x) for x in got[1]] != counts:
        out.append(f"counts {[int(x) for x in got[1]]}, not {counts}")
    return out


def invariants(g, b):
    """g: a test_cgraph_host.Graph, b: the Bubbles over its arrays"""
    recs, counts = b.reported()
    assert [r[0] for r in recs] == sorted({r[0] for r in recs})  # ascending, at most one bubble per source
    for A, Z, *rest in recs:
        B = [x for x in rest if x != NONE]
        assert B == g.links[A] and A < (Z ^ 1)
        mirror = b.predicate(Z ^ 1)
        assert mirror is not None and mirror[0] == A ^ 1 and sorted(mirror[1]) == sorted(x ^ 1 for x in B)  # the mirror is a bubble ...
        assert not (Z ^ 1) < (mirror[0] ^ 1)  # ... and the one not reported
        assert not any(g.palindromic(x >> 1) for x in B + [A, Z])  # no palindromic segment is a branch (nor a flank)
        assert all(g.spelled(A)[-(g.k - 1):] == g.spelled(x)[:g.k - 1] and g.spelled(x)[-(g.k - 1):] == g.spelled(Z)[:g.k - 1] for x in B)
    sources = {r[0] for r in recs}
    for A in range(b.n2):  # every source of the other mirror is behind a reported one
        hit = b.predicate(A)
        if hit is not None and A not in sources:
            assert (hit[0] ^ 1) in sources
    assert counts[0] == len(recs) and counts[1] == sum(len(g.links[r[0]]) for r in recs)
    # segment_of is the inverse of members
    n = len(g.m.rows)
    seg_off, _, _, _, members = g.arrays()
    seg_of, pos = segment_of(g.k, seg_off, members, n)
    assert sum(x != NONE for x in seg_of) == len(members) == sum(g.eligible)
    for row in range(n):
        assert (seg_of[row] == NONE) == (pos[row] == NONE) == (not g.eligible[row])
        if seg_of[row] != NONE:
            assert g.segs[seg_of[row] >> 1][pos[row]] == 2 * row + (seg_of[row] & 1)
    return recs


@functools.lru_cache(maxsize=None)
def bubbles_of(case, *args):
    """Bubbles over the arrays of test_cgraph_host.graph(case, *args)"""
    g = G.graph(case, *args)
    return Bubbles(g.k, *g.arrays()[:4])


# ---- the planted-variant case ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def planted_case(k, length=2500):
    """(genomes, model, sites): four genomes of one random ancestor.  sites: [(kind, allele groups as a sorted list of sorted genome lists)] --
    substitutions at sites 2k apart or more (one of them tri-allelic) and one insertion of 5 bases in genome 1"""
    anc = H.text(S.random_genome(length, 4200 + k))
    assert len({H.canon(anc[i:i + k]) for i in range(length - k + 1)}) == length - k + 1  # no repeat, on either strand
    step = max(2 * k + 11, 300)
    at = [200 + j * step for j in range(4)]
    assert at[-1] + 2 * k < length
    other = lambda c, j: "ACGT"[("ACGT".index(c) + j) % 4]  # noqa: E731
    g = [list(anc) for _ in range(4)]
    sites = []
    for x in (2, 3):
        g[x][at[0]] = other(anc[at[0]], 1)
    sites.append(("sub", [[0, 1], [2, 3]]))
    for x in (1, 2, 3):
        g[x][at[1]] = other(anc[at[1]], 2)
    sites.append(("sub", [[0], [1, 2, 3]]))
    g[2][at[2]] = other(anc[at[2]], 1)
    g[3][at[2]] = other(anc[at[2]], 3)
    sites.append(("sub", [[0, 1], [2], [3]]))
    # (its first base is not the one behind it, its last not the one before it: the branches are cut exactly at the insertion)
    ins = other(anc[at[3]], 1) + "".join(other(anc[at[3]], 1 + j % 3) for j in range(3)) + other(anc[at[3] - 1], 1)
    g[1][at[3]:at[3]] = list(ins)  # (the sites before it keep their places)
    sites.append(("ins", [[0, 2, 3], [1]]))
    genomes = [["".join(x)] for x in g]
    return genomes, H.Model(H.owners_of(genomes, k), k), sites


@functools.lru_cache(maxsize=None)
def planted_graph(k):
    return G.Graph(planted_case(k)[1], 0)


def planted_truth(k):
    """per reported bubble of the planted case: (record, branch lengths, allele groups from the AND colour sets)"""
    g = planted_graph(k)
    b = Bubbles(k, *g.arrays()[:4])
    inter = g.colour_sets("and")
    out = []
    for rec in b.reported()[0]:
        B = [x for x in rec[2:] if x != NONE]
        out.append((rec, [len(g.seqs[x >> 1]) for x in B], sorted(sorted(inter[x >> 1]) for x in B)))
    return out


def expected_text(g, recs):
    """the file of extract_bubbles_to_disk (<bft/unitigs.h>) and of the command line's -bubbles for the records recs of the graph g"""
    inter = g.colour_sets("and")
    lines = []
    for i, (A, Z, *rest) in enumerate(recs):
        B = [x for x in rest if x != NONE]
        lines.append(f"B\t{i}\t{A >> 1}{'+-'[A & 1]}\t{Z >> 1}{'+-'[Z & 1]}\t{len(B)}")
        for x in B:
            ids = sorted(inter[x >> 1])
            lines.append(f"A\t{x >> 1}{'+-'[x & 1]}\t{g.spelled(x)}\t{len(ids)}\t{','.join(map(str, ids))}")
    return "".join(line + "\n" for line in lines)


def joins_to_gfa(text, gfa):
    """every A line of a bubble file names a segment of the GFA file, with that S line's sequence in the orientation given"""
    seqs = {f[1]: f[2] for f in (line.split("\t") for line in gfa.split("\n")) if f[0] == "S"}
    lines = [line.split("\t") for line in text.split("\n") if line.startswith("A\t")]
    return bool(lines) and all(f[1][:-1] in seqs and f[2] == (seqs[f[1][:-1]] if f[1][-1] == "+" else H.rc(seqs[f[1][:-1]])) for f in lines)


# ---- hand-made link tables ------------------------------------------------------------------------------------------------------------------------
def table(k, n_seg, edges, seed=0, seqs=None, lens=None):
    """(seg_off, seqs, link_off, links) of n_seg segments with the given links (a, b) between oriented segments, exactly as listed (mirror() adds the
    mirror forms); segment i spells seqs[i] when given, else lens[i] (default k .. 2k + 5) random nucleotides"""
    rng = np.random.default_rng(9000 + seed)
    strings = []
    for i in range(n_seg):
        s = (seqs or {}).get(i)
        if s is None:
            n = (lens or {}).get(i, int(rng.integers(k, 2 * k + 6)))
            s = "".join(rng.choice(list("ACGT"), n))
            while s == H.rc(s):
                s = "".join(rng.choice(list("ACGT"), n))
        strings.append(s)
    lists = [sorted(b for a, b in edges if a == x) for x in range(2 * n_seg)]
    seg_off = np.cumsum([0] + [len(s) for s in strings]).astype(np.uint64)
    link_off = np.cumsum([0] + [len(x) for x in lists]).astype(np.uint64)
    return seg_off, np.frombuffer("".join(strings).encode(), dtype=np.uint8), link_off, np.array([b for x in lists for b in x], dtype=np.uint32)


def mirror(edges):
    return sorted(set(edges) | {(b ^ 1, a ^ 1) for a, b in edges})


def motif(src, snk, branches):
    """the links of one bubble src+ -> branch+ -> snk+ (segments), both mirror forms"""
    return mirror([(2 * src, 2 * b) for b in branches] + [(2 * b, 2 * snk) for b in branches])


@functools.lru_cache(maxsize=None)
def hand_tables(k):
    """[(name, (seg_off, seqs, link_off, links), max_branch_chars, n_bubbles known by construction)]: one case per rule of the definition.  Segment 0
    is the source, 1 the sink, 2 .. the branches, 7 a bystander"""
    pal = None
    if k % 2 == 0:
        w = "".join(np.random.default_rng(k).choice(list("ACGT"), k // 2))
        pal = w + H.rc(w)
    cases = []
    for m in (2, 3, 4, 5):
        cases.append((f"m = {m}", table(k, 8, motif(0, 1, range(2, 2 + m)), m), 0, 1 if m <= 4 else 0))
    cases.append(("the mirror is the one reported", table(k, 8, motif(6, 0, (2, 3, 4)), 6), 0, 1))
    base = motif(0, 1, (2, 3))
    cases.append(("a sink with one extra in-link", table(k, 8, mirror(base + [(14, 2)]), 7), 0, 0))
    cases.append(("a branch with a second in-link", table(k, 8, mirror(base + [(14, 4)]), 8), 0, 0))
    cases.append(("a branch with two out-links", table(k, 8, mirror(base + [(4, 14)]), 9), 0, 0))
    cases.append(("branches to different sinks", table(k, 8, mirror([(0, 4), (0, 6), (4, 2), (6, 14)]), 10), 0, 0))
    cases.append(("the sink is the source: a cycle", table(k, 8, mirror([(0, 4), (0, 6), (4, 0), (6, 0)]), 11), 0, 0))
    cases.append(("a branch is the flip of the source", table(k, 8, mirror([(0, 1), (0, 4), (4, 2), (1, 2)]), 12), 0, 0))
    cases.append(("two branches are the two orientations of one segment", table(k, 8, [(0, 4), (0, 5), (4, 1), (5, 1)], 13), 0, 0))
    cases.append(("a self loop on the source", table(k, 8, mirror(base + [(0, 0)]), 14), 0, 0))
    # the in-links of the sink are evaluated literally: a table that is not mirror-symmetric, the sink's list names a bystander
    cases.append(("the sink's in-links name another segment", table(k, 8, [(0, 4), (0, 6), (4, 2), (6, 2), (5, 1), (7, 1), (3, 5), (3, 15)], 15), 0, 0))
    if pal:
        cases.append(("a palindromic source", table(k, 8, base, 16, seqs={0: pal}), 0, 0))
        cases.append(("a palindromic sink", table(k, 8, base, 17, seqs={1: pal}), 0, 0))
        cases.append(("a palindromic bystander", table(k, 8, base, 18, seqs={7: pal}), 0, 1))
        cases.append(("a flank of k characters that is no palindrome", table(k, 8, base, 19, lens={0: k, 1: k}), 0, 1))
    lens = {2: k + 3, 3: 2 * k + 4}
    cases.append(("max_branch_chars at the longest branch", table(k, 8, base, 20, lens=lens), 2 * k + 4, 1))
    cases.append(("max_branch_chars one below it", table(k, 8, base, 20, lens=lens), 2 * k + 3, 0))
    cases.append(("substitution shape", table(k, 8, motif(0, 1, (2, 3, 4)), 21, lens={2: 2 * k - 1, 3: 2 * k - 1, 4: 2 * k - 1}), 0, 1))
    return cases


@functools.lru_cache(maxsize=None)
def grid_table(k=27):
    """((seg_off, seqs, link_off, links), n_bubbles): bubble motifs of 2, 3 and 4 branches in a row, every other one numbered so that its mirror is
    the one reported, until 2S is just past the capped grid: the second grid-stride pass, a scan of more than one tile, the emission order"""
    edges, n_seg, n = [], 0, 0
    while 2 * n_seg <= GRID_LANES + 64:
        m = 2 + n % 3
        ids = list(range(n_seg, n_seg + 2 + m))
        src, snk = (ids[0], ids[-1]) if n % 2 == 0 else (ids[-1], ids[0])
        edges += [(2 * src, 2 * b) for b in ids[1:-1]] + [(2 * b, 2 * snk) for b in ids[1:-1]]
        n_seg += 2 + m
        n += 1
    e = np.array(edges, dtype=np.int64)
    e = np.concatenate([e, np.stack([e[:, 1] ^ 1, e[:, 0] ^ 1], axis=1)])
    e = e[np.lexsort((e[:, 1], e[:, 0]))]
    link_off = np.concatenate([[0], np.cumsum(np.bincount(e[:, 0], minlength=2 * n_seg))]).astype(np.uint64)
    seqs = np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(77).integers(0, 4, n_seg * k)]
    seg_off = (np.arange(n_seg + 1, dtype=np.uint64) * np.uint64(k)).astype(np.uint64)
    return (seg_off, seqs, link_off, e[:, 1].astype(np.uint32)), n


# ---- tests ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", H.KS)
def test_invariants_on_the_key_width_cases(k):
    total = 0
    for t in G.THRESHOLDS:
        recs = invariants(G.graph("width_case", k, t), bubbles_of("width_case", k, t))
        total += len(recs)
    assert bubbles_of("width_case", k, H.N_GENOMES + 1).reported() == ([], [0, 0, 0, 0])
    if k <= 36:
        assert total > 0 and bubbles_of("width_case", k, 0).reported()[1][2] > 0  # isolated SNPs: substitution shapes


@pytest.mark.parametrize("k", H.HAND_KS)
def test_invariants_on_the_hand_made_cases(k):
    for t in (0, 1, 2):
        invariants(G.graph("hand_case", k, t), bubbles_of("hand_case", k, t))


@pytest.mark.parametrize("k", PLANTED_KS)
def test_planted_variants_are_found_exactly(k):
    _, _, sites = planted_case(k)
    g = planted_graph(k)
    g.invariants()
    b = Bubbles(k, *g.arrays()[:4])
    invariants(g, b)
    truth = planted_truth(k)
    assert len(truth) == len(sites) == 4  # exactly one bubble per site
    by_groups = {tuple(map(tuple, groups)): (rec, lens) for rec, lens, groups in truth}
    assert len(by_groups) == 4
    for kind, groups in sites:
        rec, lens = by_groups[tuple(map(tuple, groups))]  # the AND colour sets of the branches are the construction's allele groups
        assert len(lens) == len(groups)
        if kind == "sub":
            assert lens == [2 * k - 1] * len(groups)
        else:
            assert len(lens) == 2 and abs(lens[0] - lens[1]) == 5
    assert b.reported()[1] == [4, 9, 3, max(max(lens) for _, lens, _ in truth)]
    assert Bubbles(k, *g.arrays()[:4], max_branch_chars=2 * k - 1).reported()[1] == [3, 7, 3, 2 * k - 1]  # the insertion's long branch is out


@pytest.mark.parametrize("k", (27, 36))
def test_hand_made_link_tables(k):
    seen = 0
    for name, arrays, max_chars, n in hand_tables(k):
        recs, counts = Bubbles(k, *arrays, max_branch_chars=max_chars).reported()
        assert len(recs) == counts[0] == n, name
        seen += n
        if name.startswith("m = ") and n:
            m = int(name[4:])
            assert recs == [[0, 2] + [4 + 2 * j for j in range(m)] + [NONE] * (4 - m)] and counts[1] == m, name
        if name == "the mirror is the one reported":
            assert recs == [[1, 13, 5, 7, 9, NONE]]
        if name == "substitution shape":
            assert counts == [1, 3, 1, 2 * k - 1]
    assert seen >= 6


def test_grid_table():
    arrays, n = grid_table()
    assert len(arrays[2]) - 1 > GRID_LANES
    recs, counts = Bubbles(27, *arrays).reported()
    assert counts[0] == n and counts[1] == sum(2 + i % 3 for i in range(n)) and counts[2] == 0 and counts[3] == 27
    assert [r[0] for r in recs] == sorted(r[0] for r in recs) and sum(r[0] & 1 for r in recs) == n // 2  # every other one through its mirror


def test_checker_reports_doctored_results():
    k = 27
    want = bubbles_of("width_case", k, 0).reported()
    recs, counts = want
    assert len(recs) >= 3 and check(want, (np.array(recs, dtype=np.uint32), np.array(counts, dtype=np.uint64))) == []
    # a dropped bubble
    assert any("missing" in p for p in check(want, (recs[:1] + recs[2:], counts)))
    # a swapped mirror
    A, Z, *B = recs[1]
    flipped = [Z ^ 1, A ^ 1] + [x ^ 1 if x != NONE else NONE for x in B]
    assert any("its mirror is reported" in p for p in check(want, (recs[:1] + [flipped] + recs[2:], counts)))
    # branches out of order
    r = list(recs[0])
    r[2], r[3] = r[3], r[2]
    assert any("branches out of order" in p for p in check(want, ([r] + recs[1:], counts)))
    # and anything else
    assert check(want, (recs[::-1], counts)) and check(want, (recs + [recs[0]], counts)) and check(want, (recs, counts[:3] + [counts[3] + 1]))
    assert any("is none" in p for p in check(want, (recs + [[NONE - 1, 0, 2, 4, NONE, NONE]], counts)))


def test_expected_text_of_the_planted_case():
    k = 27
    g = planted_graph(k)
    recs = Bubbles(k, *g.arrays()[:4]).reported()[0]
    text = expected_text(g, recs)
    lines = text.split("\n")
    assert lines[-1] == "" and sum(line.startswith("B\t") for line in lines) == 4 and sum(line.startswith("A\t") for line in lines) == 9
    groups = sorted(sorted([int(x) for x in line.split("\t")[4].split(",")] for line in lines[i + 1:i + 1 + int(lines[i].split("\t")[4])])
                    for i in range(len(lines)) if lines[i].startswith("B\t"))
    assert groups == sorted(site[1] for site in planted_case(k)[2])
    gfa = "".join(f"S\t{j}\t{q}\tLN:i:{len(q)}\n" for j, q in enumerate(g.seqs))
    used = next(line for line in lines if line.startswith("A\t")).split("\t")[1][:-1]
    assert joins_to_gfa(text, gfa) and not joins_to_gfa(text, gfa.replace(f"S\t{used}\t", "S\tx\t"))


def test_names_are_declared_exported_and_in_signatures():
    subprocess.check_call(["make", "-C", _lib.CSRC, "all"], stdout=subprocess.DEVNULL)
    hdr = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["bft_gpu_unitig_bubbles"][1]) == 11 and len(_lib.SIGNATURES["bft_gpu_unitig_bubbles_dev"][1]) == 12
    assert len(_lib.SIGNATURES["bft_gpu_unitig_segment_of"][1]) == 8 and len(_lib.SIGNATURES["bft_gpu_unitig_segment_of_dev"][1]) == 9
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert set(NAMES) <= set(re.findall(r" T (bft_gpu_[a-z_0-9]+)", out))
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(_lib.CSRC, "libbft.so")]).decode()
    assert re.search(r" T extract_bubbles_to_disk$", out, flags=re.M)
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bft", "unitigs.h")).read(), flags=re.S)
    assert re.search(r"\bvoid\s+extract_bubbles_to_disk\s*\(\s*BFT\s*\*\s*graph\s*,\s*int\s+min_shared\s*,\s*int\s+max_branch_length\s*,\s*char\s*\*\s*filename_output\s*\)\s*;", code)
    subprocess.run(["gcc", "-std=gnu99", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", "-I", os.path.join(ROOT, "include"), "-"],
                   input=b"#include <bft/unitigs.h>\nint main(void) { return 0; }\n", check=True)
    from bloomfiltertrie_amd import BFT
    assert all(hasattr(BFT, name) for name in ("unitig_bubbles", "unitig_bubbles_dev", "unitig_segment_of", "unitig_segment_of_dev", "bubbles"))
    usage = subprocess.run([os.path.join(_lib.CSRC, "bft_gpu")], capture_output=True, text=True)
    assert usage.returncode != 0 and "[-bubbles min_shared max_branch_chars output_file]" in usage.stderr


def test_bubble_kernels_use_no_scratch_no_spill_and_no_lds():
    """Every k_bb_* kernel: no scratch memory, no vector register spilled to it, no LDS, 128 VGPRs at the most"""
    subprocess.check_call(["make", "-C", _lib.CSRC, "all"], stdout=subprocess.DEVNULL)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "k_bb_"], capture_output=True, text=True).stdout
    seen = {}
    for line in out.splitlines()[1:]:
        if not line.strip():
            continue
        vgpr, sgpr, vspill, sspill, scratch, lds, maxwg, name = line.split(None, 7)
        kernel = re.search(r"(k_bb_[a-z]+)", name).group(1)
        seen[kernel] = seen.get(kernel, 0) + 1
        assert int(vspill) == 0 and int(scratch) == 0 and int(lds) == 0, line
        assert int(vgpr) <= 128, line  # (two workgroups of 256 threads per SIMD at least)
    assert set(seen) == KERNELS and all(v == 1 for v in seen.values()), seen


def test_null_arguments_are_refused_before_any_device_work():
    lib = _lib.load()
    cnt = (C.c_uint64 * 4)()
    one = C.c_void_p(1)
    assert lib.bft_gpu_unitig_bubbles(None, None, None, None, None, 0, 0, 0, None, 0, cnt) == -1  # BFT_GPU_E_ARG
    assert lib.bft_gpu_unitig_bubbles(one, None, None, None, None, 0, 0, 0, None, 0, None) == -1
    assert lib.bft_gpu_unitig_bubbles(one, None, one, one, one, 1, 0, 0, None, 0, cnt) == -1   # segments without offsets
    assert lib.bft_gpu_unitig_bubbles(one, one, None, one, one, 1, 0, 0, None, 0, cnt) == -1   # ... without characters
    assert lib.bft_gpu_unitig_bubbles(one, one, one, None, one, 1, 0, 0, None, 0, cnt) == -1   # ... without link offsets
    assert lib.bft_gpu_unitig_bubbles(one, one, one, one, None, 1, 1, 0, None, 0, cnt) == -1   # links without an array
    assert lib.bft_gpu_unitig_bubbles_dev(None, None, None, None, None, 0, 0, 0, None, 0, cnt, None) == -1
    assert lib.bft_gpu_unitig_bubbles_dev(one, None, None, None, None, 0, 0, 0, None, 0, None, None) == -1
    assert lib.bft_gpu_unitig_bubbles_dev(one, None, one, one, one, 1, 0, 0, None, 0, cnt, None) == -1
    assert lib.bft_gpu_unitig_bubbles_dev(one, one, one, one, None, 1, 1, 0, None, 0, cnt, None) == -1
    assert lib.bft_gpu_unitig_segment_of(None, None, 0, None, 0, None, None, 0) == -1
    assert lib.bft_gpu_unitig_segment_of(one, None, 0, None, 1, None, None, 0) == -1   # segments without offsets
    assert lib.bft_gpu_unitig_segment_of(one, None, 1, one, 1, None, None, 0) == -1    # members without an array
    assert lib.bft_gpu_unitig_segment_of_dev(None, None, 0, None, 0, None, None, 0, None) == -1
    assert lib.bft_gpu_unitig_segment_of_dev(one, None, 0, None, 1, None, None, 0, None) == -1
    assert "NULL" in lib.bft_gpu_last_error().decode()
    assert lib.bft_gpu_unitig_bubbles(one, one, one, one, one, 1 << 31, 0, 0, None, 0, cnt) == -3 and "2^31" in lib.bft_gpu_last_error().decode()  # BFT_GPU_E_LIMIT
