"""CPU-side tests of the compacted coloured graph (no GPU).  The truth model of include/bft_gpu.h's definition of bft_gpu_unitig_graph -- segments,
oriented segments, links, members, written from the definition over the model of tests/test_unitigs_host.py (vertices, successors, kept paths) --
with the definition's invariants proved on every index the GPU tests use: every kept successor is the first vertex of an oriented segment, every link
overlaps in k - 1 letters, the self links of cycles and homopolymers, the hairpin's S+ -> S-, a chain without a link, mirror symmetry up to the
palindromic single-k-mer segments, members that partition the eligible rows, link counts that are the out-degrees at t = 0, the unitigs inside the
segments, and no link that the unitig rule would have merged.  The checker the GPU tests compare with, shown to report doctored results; the new
names in the header and SIGNATURES, the symbols exported; the k_cg_* kernels without scratch memory, spills or LDS; NULL arguments refused before
anything touches a device.  tests/test_gpu_cgraph.py runs the cases of this file on the GPU."""
import ctypes as C
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_unitigs_host as H  # noqa: E402

from bloomfiltertrie_amd import _lib  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = {"k_cg_singles", "k_cg_members", "k_cg_links", "k_cg_emit", "k_cg_groups"}
NAMES = ("bft_gpu_unitig_graph", "bft_gpu_unitig_graph_dev", "bft_gpu_unitig_colors", "bft_gpu_unitig_colors_dev")
THRESHOLDS = (0, 1, 2, H.N_GENOMES, H.N_GENOMES + 1)


class Graph:
    """The definition, literally, over a test_unitigs_host.Model m at threshold t."""

    def __init__(self, m, t):
        self.m, self.t, self.k = m, t, m.k
        n = len(m.rows)
        own = [m.owners[s] for s in m.rows]
        node, _ = m.edges(t)
        self.eligible = [len(own[i]) >= t for i in range(n)]
        kept = m.paths(t)
        singles = [[2 * i] for i in range(n) if self.eligible[i] and not node[i]]
        self.segs = sorted([list(p) for p in kept] + singles, key=lambda p: p[0])
        self.is_single = [len(p) == 1 and not node[p[0] >> 1] for p in self.segs]
        self.seqs = [m.spell(p) for p in self.segs]
        self.first = {}  # first vertex -> oriented segment
        for i, p in enumerate(self.segs):
            assert p[0] not in self.first and (p[-1] ^ 1) not in self.first
            self.first[p[0]] = 2 * i
            self.first[p[-1] ^ 1] = 2 * i + 1
        self.links = []  # per oriented segment: its targets, ascending
        for a in range(2 * len(self.segs)):
            e = self.end(a)
            out = []
            for w in m.succ[e]:
                if self.eligible[w >> 1] and (t == 0 or len(own[e >> 1] & own[w >> 1]) >= t):
                    assert w in self.first, (a, e, w)  # every kept successor is the first vertex of an oriented segment, never an interior one
                    out.append(self.first[w])
            assert len(set(out)) == len(out)
            self.links.append(sorted(out))

    def end(self, a):
        """the last vertex of oriented segment a"""
        p = self.segs[a >> 1]
        return p[-1] if a & 1 == 0 else p[0] ^ 1

    def spelled(self, a):
        s = self.seqs[a >> 1]
        return s if a & 1 == 0 else H.rc(s)

    def palindromic(self, i):
        """segment i is one k-mer that is its own reverse complement"""
        p = self.segs[i]
        return len(p) == 1 and self.m.words[p[0]] == self.m.words[p[0] ^ 1]

    def arrays(self):
        """(seg_off, seqs, link_off, links, members) as bft_gpu_unitig_graph returns them"""
        seg_off = np.cumsum([0] + [len(s) for s in self.seqs]).astype(np.uint64)
        link_off = np.cumsum([0] + [len(x) for x in self.links]).astype(np.uint64)
        return (seg_off, np.frombuffer("".join(self.seqs).encode(), dtype=np.uint8), link_off,
                np.array([b for x in self.links for b in x], dtype=np.uint32), np.array([v for p in self.segs for v in p], dtype=np.uint32))

    def counts(self):
        return [len(self.segs), sum(map(len, self.seqs)), max(map(len, self.seqs), default=0), self.m.noncanonical, sum(map(len, self.links)),
                sum(self.is_single)]

    def colour_sets(self, op):
        """per segment: the set of genomes of op over the owners of its members"""
        out = []
        for p in self.segs:
            sets = [self.m.owners[self.m.rows[v >> 1]] for v in p]
            u, i = set().union(*sets), set.intersection(*map(set, sets))
            out.append({"or": u, "and": i, "symdiff": u - i if len(sets) > 1 else u}[op])
        return out

    def invariants(self):
        m, t, k = self.m, self.t, self.k
        n = len(m.rows)
        assert m.noncanonical == 0
        # the members partition the eligible rows
        rows = [v >> 1 for p in self.segs for v in p]
        assert sorted(rows) == [i for i in range(n) if self.eligible[i]]
        assert [p[0] for p in self.segs] == sorted(p[0] for p in self.segs)
        # the segments that are no singles are the unitigs
        assert [s for s, one in zip(self.seqs, self.is_single) if not one] == m.unitigs(t)
        assert all(len(s) == len(p) + k - 1 for s, p in zip(self.seqs, self.segs))
        # every link's two spellings overlap in k - 1 letters
        pairs = set()
        for a, out in enumerate(self.links):
            for b in out:
                assert self.spelled(a)[-(k - 1):] == self.spelled(b)[:k - 1]
                pairs.add((a, b))
        # mirror symmetry once the two orientations of a palindromic single-k-mer segment are identified; links into one always name its +
        ident = lambda a: a & ~1 if self.palindromic(a >> 1) else a  # noqa: E731
        folded = {(ident(a), ident(b)) for a, b in pairs}
        assert all((ident(b ^ 1), ident(a ^ 1)) in folded for a, b in pairs)
        literal = [(a, b) for a, b in pairs if (b ^ 1, a ^ 1) not in pairs]
        assert all(self.palindromic(a >> 1) or self.palindromic(b >> 1) for a, b in literal)
        assert all(b & 1 == 0 for _, b in pairs if self.palindromic(b >> 1))
        for i in range(len(self.segs)):
            if self.palindromic(i):
                assert self.links[2 * i] == self.links[2 * i + 1]
        if t == 0:
            deg = m.degrees()
            _, nxt = m.edges(0)
            for a, out in enumerate(self.links):
                e = self.end(a)
                assert len(out) == (deg[e >> 1] >> 4 if e & 1 == 0 else deg[e >> 1] & 15)  # the out nibble of that end
                for b in out:
                    w = next(v for v in m.succ[e] if self.first.get(v) == b)
                    assert nxt.get(e) != w or b == a  # no link joins two ends that the unitig rule would have merged (but a cycle's cut: its self link)
        return pairs


@functools.lru_cache(maxsize=None)
def graph(case, *args):
    """Graph of a case of test_unitigs_host (width_case, hand_case, grid_case, whole_case) at threshold args[-1]"""
    _, m = getattr(H, case)(*args[:-1])
    return Graph(m, args[-1])


def parse(k, seg_off, seqs, link_off, links, members):
    """the five arrays -> (strings, link lists per oriented segment, member lists per segment)"""
    strings = H.split(seg_off, seqs)
    ns = len(strings)
    lo = [int(x) for x in link_off]
    ll = [[int(b) for b in links[lo[a]:lo[a + 1]]] for a in range(2 * ns)]
    so = [int(x) for x in seg_off]
    mem = [[int(v) for v in members[so[i] - i * (k - 1):so[i + 1] - (i + 1) * (k - 1)]] for i in range(ns)]
    return strings, ll, mem


def check(g, got):
    """problems of `got` = (seg_off, seqs, link_off, links, members) as the graph g; empty when it is exactly the truth"""
    strings, ll, mem = parse(g.k, *got)
    if strings == g.seqs and ll == g.links and mem == g.segs and len(got[2]) == 2 * len(g.seqs) + 1 and len(got[4]) == sum(map(len, g.segs)):
        return []
    out = []
    if strings != g.seqs:
        have = set(strings)
        out += [f"single segment left out: {s}" for s, one in zip(g.seqs, g.is_single) if one and s not in have]
        out += [f"segment missing: {s[:40]}" for s, one in zip(g.seqs, g.is_single) if not one and s not in have]
        out += [f"not a segment: {s[:40]}" for s in strings if s not in set(g.seqs)]
        return out or ["segments: order or multiplicity differs"]
    for i, (a, b) in enumerate(zip(mem, g.segs)):
        if a != b:
            out.append(f"segment {i}: members in reverse order" if a == b[::-1] and len(b) > 1 else f"segment {i}: members differ")
    want = {(a, b) for a, x in enumerate(g.links) for b in x}
    have = {(a, b) for a, x in enumerate(ll) for b in x}
    for a, b in sorted(want - have):
        out.append(f"link {a} -> {b} missing" + (": its mirror is there" if (b ^ 1, a ^ 1) in have else ""))
    for a, b in sorted(have - want):
        out.append(f"link {a} -> {b} is none" + (": the target in the wrong orientation" if (a, b ^ 1) in want else ""))
    if not out and ll != g.links:
        out.append("links: order or multiplicity differs")
    return out or ["sizes differ"]


def check_gfa(g, text, colors):
    """problems of a GFA 1 file (extract_unitig_graph_to_disk of <bft/unitigs.h>, the command line's -gfa) as the graph g; empty when it is the truth:
    the header, one S line per segment in order (with colors: the union row, the intersection row, the genomes in the union), one L line per entry of
    the link lists in their order, nothing else"""
    lines = text.split("\n")
    if lines[-1] != "" or lines[0] != f"H\tVN:Z:1.0\tkl:i:{g.k}":
        return ["header or final newline"]
    lines = lines[1:-1]
    ns = len(g.seqs)
    out = []
    if len(lines) != ns + sum(map(len, g.links)):
        return [f"{len(lines)} lines, not {ns} segments + {sum(map(len, g.links))} links"]
    unions, inters = g.colour_sets("or"), g.colour_sets("and")

    def bits(tag, field):
        assert field.startswith(tag + ":H:") and len(field) % 2 == 1, field
        row = bytes.fromhex(field[5:])
        return {b for b in range(8 * len(row)) if row[b >> 3] >> (b & 7) & 1}, len(row)

    n_genomes = len({x for s in g.m.owners.values() for x in s})
    for i, line in enumerate(lines[:ns]):
        f = line.split("\t")
        if f[:4] != ["S", str(i), g.seqs[i], f"LN:i:{len(g.seqs[i])}"] or len(f) != (7 if colors else 4):
            out.append(f"S line {i}: {line[:60]}")
        elif colors:
            (cu, nu), (ci, ni) = bits("cu", f[4]), bits("ci", f[5])
            if cu != unions[i] or ci != inters[i] or f[6] != f"gc:i:{len(unions[i])}" or nu != ni or nu < (n_genomes + 7) // 8 or f[4][5:] != f[4][5:].upper():
                out.append(f"S line {i}: colours {f[4:]}, not {sorted(unions[i])} / {sorted(inters[i])}")
    want = [f"L\t{a >> 1}\t{'+-'[a & 1]}\t{b >> 1}\t{'+-'[b & 1]}\t{g.k - 1}M" for a, x in enumerate(g.links) for b in x]
    out += [f"L line {j}: {got}, not {w}" for j, (got, w) in enumerate(zip(lines[ns:], want)) if got != w]
    return out


# ---- tests ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", H.KS)
def test_invariants_on_the_key_width_cases(k):
    for t in THRESHOLDS:
        g = graph("width_case", k, t)
        g.invariants()
        assert (len(g.segs) == 0) == (t > H.N_GENOMES)
    g = graph("width_case", k, 0)
    assert sum(g.is_single) > 0 and g.counts()[4] > 0 and len(g.segs) > sum(g.is_single)


@pytest.mark.parametrize("k", H.HAND_KS)
def test_invariants_and_situations_of_the_hand_made_cases(k):
    _, m = H.hand_case(k)
    parts = H.hand_parts(k)
    for t in (0, 1, 2, 3):
        graph("hand_case", k, t).invariants()
    g = graph("hand_case", k, 0)
    if k == 9:
        return  # (a few hundred 9-mers touch each other by chance: the situations below are not isolated there, the invariants hold all the same)
    where = {s: i for i, s in enumerate(g.seqs)}
    i = where[H.canon(parts["lone"][0])]
    assert g.links[2 * i] == [] and g.links[2 * i + 1] == []  # a lone k-mer
    i = where["A" * k]
    assert g.links[2 * i] == [2 * i] and g.links[2 * i + 1] == [2 * i + 1]  # a homopolymer: a self loop
    circ = parts["circle"][0]
    ring2 = circ[:150] * 2
    i = next(j for j, s in enumerate(g.seqs) if len(s) == len(circ) and (s[:150] in ring2 or H.rc(s[:150]) in ring2))
    assert g.links[2 * i] == [2 * i] and g.links[2 * i + 1] == [2 * i + 1]  # a cycle: S+ -> S+ and S- -> S-
    if k % 2 == 0:
        pal2 = parts["palindrome between two neighbours"][0][1:-1]
        i = where[pal2]
        assert g.is_single[i] and g.palindromic(i) and len(g.links[2 * i]) == 2 and g.links[2 * i] == g.links[2 * i + 1]
        into = [(a, b) for a, x in enumerate(g.links) for b in x if b >> 1 == i]
        assert len(into) == 2 and all(b == 2 * i for _, b in into)  # links into a palindrome name its + orientation
        asym = [(a, b) for a, x in enumerate(g.links) for b in x if (a ^ 1) not in g.links[b ^ 1]]
        assert asym and all(g.palindromic(a >> 1) or g.palindromic(b >> 1) for a, b in asym)
        pal1 = parts["palindrome, one neighbour word"][0][1:-1]
        i = where[pal1]
        assert not g.is_single[i] and g.palindromic(i) and len(g.links[2 * i]) == 1
    else:
        q = parts["hairpin"][0]
        x = q[-k - 1:-1]
        v = 2 * m.row[H.canon(x)] + (H.canon(x) != x)
        a = next(a for a in range(2 * len(g.segs)) if g.end(a) == v)
        assert g.links[a] == [a ^ 1]  # a hairpin: S+ -> S-
    x = parts["two successors, two strands"][0][:k]
    i = where[H.canon(x)]
    assert g.is_single[i] and 2 in (len(g.links[2 * i]), len(g.links[2 * i + 1]))
    if "chain" in parts:
        assert max(map(len, g.segs)) >= 3000


def test_grid_case_invariants():
    g = graph("grid_case", 0)
    g.invariants()
    assert 2 * len(g.m.rows) > 524288


@pytest.mark.parametrize("k", H.WHOLE_KS)
@pytest.mark.parametrize("kind", ("chain", "cycle"))
@pytest.mark.parametrize("n", H.WHOLE_NS)
def test_whole_table_cases(n, kind, k):
    g = graph("whole_case", n, kind, k, 0)
    g.invariants()
    assert len(g.segs) == 1 and not g.is_single[0]
    if kind == "chain":
        assert g.links == [[], []]  # a chain alone has no link
    else:
        assert g.links == [[0], [1]]  # a cycle: S+ -> S+ and S- -> S- (a circle of one letter is a homopolymer: the same self loops)


def test_checker_reports_doctored_results():
    k = 36
    g = graph("hand_case", k, 0)
    seg_off, seqs, link_off, links, members = g.arrays()
    assert check(g, (seg_off, seqs, link_off, links, members)) == []

    def rebuilt(ll):
        return np.cumsum([0] + [len(x) for x in ll]).astype(np.uint64), np.array([b for x in ll for b in x], dtype=np.uint32)

    # a dropped mirror link
    a, b = next((a, b) for a, x in enumerate(g.links) for b in x if (b ^ 1) != a and (a ^ 1) in g.links[b ^ 1])
    ll = [list(x) for x in g.links]
    ll[b ^ 1].remove(a ^ 1)
    lo, lk = rebuilt(ll)
    assert any("its mirror is there" in p for p in check(g, (seg_off, seqs, lo, lk, members)))
    # a target given in the wrong orientation
    ll = [list(x) for x in g.links]
    ll[a] = sorted(x ^ 1 if x == b else x for x in ll[a])
    lo, lk = rebuilt(ll)
    assert any("wrong orientation" in p for p in check(g, (seg_off, seqs, lo, lk, members)))
    # a single segment left out
    i = g.is_single.index(True)
    strings = g.seqs[:i] + g.seqs[i + 1:]
    so = np.cumsum([0] + [len(s) for s in strings]).astype(np.uint64)
    assert any("single segment left out" in p for p in check(g, (so, np.frombuffer("".join(strings).encode(), dtype=np.uint8), link_off, links, members)))
    # members in reverse order
    i = max(range(len(g.segs)), key=lambda j: len(g.segs[j]))
    mem = [p[::-1] if j == i else p for j, p in enumerate(g.segs)]
    assert any("reverse order" in p for p in check(g, (seg_off, seqs, link_off, links, np.array([v for p in mem for v in p], dtype=np.uint32))))
    # the same through the GFA text
    gfa = f"H\tVN:Z:1.0\tkl:i:{k}\n" + "".join(f"S\t{j}\t{q}\tLN:i:{len(q)}\n" for j, q in enumerate(g.seqs))
    lines = [f"L\t{x >> 1}\t{'+-'[x & 1]}\t{y >> 1}\t{'+-'[y & 1]}\t{k - 1}M\n" for x, out in enumerate(g.links) for y in out]
    assert check_gfa(g, gfa + "".join(lines), False) == []
    assert check_gfa(g, gfa + "".join(lines[:-1]), False) and check_gfa(g, gfa + "".join(lines[1:] + lines[:1]), False)
    assert check_gfa(g, gfa.replace("LN:i:", "LN:i:1", 1) + "".join(lines), False) and check_gfa(g, gfa + "".join(lines), True)
    # and anything else
    assert check(g, (seg_off, seqs, link_off, links[:-1], members)) and check(g, (seg_off, seqs, link_off, links, members[:-1]))


def test_names_are_declared_exported_and_in_signatures():
    subprocess.check_call(["make", "-C", _lib.CSRC, "all"], stdout=subprocess.DEVNULL)
    hdr = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["bft_gpu_unitig_graph"][1]) == 12 and len(_lib.SIGNATURES["bft_gpu_unitig_graph_dev"][1]) == 13
    assert len(_lib.SIGNATURES["bft_gpu_unitig_colors"][1]) == 8 and len(_lib.SIGNATURES["bft_gpu_unitig_colors_dev"][1]) == 9
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert set(NAMES) <= set(re.findall(r" T (bft_gpu_[a-z_0-9]+)", out))
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(_lib.CSRC, "libbft.so")]).decode()
    assert re.search(r" T extract_unitig_graph_to_disk$", out, flags=re.M)
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bft", "unitigs.h")).read(), flags=re.S)
    assert re.search(r"\bvoid\s+extract_unitig_graph_to_disk\s*\(\s*BFT\s*\*\s*graph\s*,\s*int\s+min_shared\s*,\s*bool\s+colors\s*,\s*char\s*\*\s*filename_output\s*\)\s*;", code)
    subprocess.run(["gcc", "-std=gnu99", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", "-I", os.path.join(ROOT, "include"), "-"],
                   input=b"#include <bft/unitigs.h>\nint main(void) { return 0; }\n", check=True)


def test_graph_kernels_use_no_scratch_no_spill_and_no_lds():
    """Every k_cg_* kernel at every key width: no scratch memory, no vector register spilled to it, no LDS, 128 VGPRs at the most"""
    subprocess.check_call(["make", "-C", _lib.CSRC, "all"], stdout=subprocess.DEVNULL)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "k_cg_"], capture_output=True, text=True).stdout
    seen = {}
    for line in out.splitlines()[1:]:
        if not line.strip():
            continue
        vgpr, sgpr, vspill, sspill, scratch, lds, maxwg, name = line.split(None, 7)
        kernel = re.search(r"(k_cg_[a-z]+)", name).group(1)
        seen[kernel] = seen.get(kernel, 0) + 1
        assert int(vspill) == 0 and int(scratch) == 0 and int(lds) == 0, line
        assert int(vgpr) <= 128, line  # (two workgroups of 256 threads per SIMD at least)
    assert set(seen) == KERNELS, seen
    assert seen["k_cg_links"] == 4 and all(seen[name] == 1 for name in KERNELS - {"k_cg_links"}), seen  # the link search: one per key width


def test_null_arguments_are_refused_before_any_device_work():
    lib = _lib.load()
    cnt = (C.c_uint64 * 6)()
    one = C.c_void_p(1)
    assert lib.bft_gpu_unitig_graph(None, 0, None, None, None, None, None, 0, 0, 0, 0, cnt) == -1  # BFT_GPU_E_ARG
    assert lib.bft_gpu_unitig_graph(one, 0, None, None, None, None, None, 0, 0, 0, 0, None) == -1
    assert lib.bft_gpu_unitig_graph_dev(None, 0, None, None, None, None, None, 0, 0, 0, 0, cnt, None) == -1
    assert lib.bft_gpu_unitig_graph_dev(one, 0, None, None, None, None, None, 0, 0, 0, 0, None, None) == -1
    assert lib.bft_gpu_unitig_colors(None, None, 0, None, 0, 1, None, None) == -1
    assert lib.bft_gpu_unitig_colors(one, None, 0, None, 1, 1, None, None) == -1   # segments without offsets
    assert lib.bft_gpu_unitig_colors(one, None, 1, one, 1, 1, None, None) == -1    # members without an array
    assert lib.bft_gpu_unitig_colors_dev(None, None, 0, None, 0, 1, None, None, None) == -1
    assert lib.bft_gpu_unitig_colors_dev(one, None, 0, None, 1, 1, None, None, None) == -1
    assert "NULL" in lib.bft_gpu_last_error().decode()
    assert lib.bft_gpu_unitig_colors(one, None, 0, None, 0, 7, None, None) == -1 and "op must be" in lib.bft_gpu_last_error().decode()
