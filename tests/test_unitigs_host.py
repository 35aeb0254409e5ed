"""CPU-side tests of the canonical (bidirected) unitigs (no GPU).  The truth model of include/bft_gpu.h's definition -- dicts, sets and strings,
from nothing but {k-mer string: genome set} and the row order -- with the five invariants of the definition on every index the GPU tests use; the
checker the GPU tests compare with, shown to report doctored results (a path in its mirror orientation, a cycle started one vertex late, a palindrome
joined to a neighbour, a hairpin joined); the new names in the header and SIGNATURES, the symbols exported; the k_ug_* kernels and the mirrored
instantiations of the path engine's found, without scratch memory or LDS; NULL arguments refused before anything touches a device.  tests/test_gpu_unitigs.py runs the cases of this file on the GPU."""
import ctypes as C
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_prefix_cases_host as P  # noqa: E402  (t_order: the row order of the table, pinned to the library by test_graph_cases_host)

from bloomfiltertrie_amd import _lib, synth as S  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the family's own kernels, and the mirrored instantiations of the path engine's (csrc/bft_paths.hip: template <bool MIRRORED>) the unitigs run
KERNELS = {"k_ug_canon", "k_ug_degrees", "k_ug_links", "k_sp_ends<true>", "k_sp_offsets<true>", "k_sp_spell<true>"}
NAMES = ("bft_gpu_unitigs", "bft_gpu_unitigs_dev", "bft_gpu_bidirected_degrees", "bft_gpu_bidirected_degrees_dev")
KS = (9, 18, 27, 31, 36, 63, 64, 72, 126)  # W = 1..4, both tail layouts of the T-form (k % 9 == 0 and not)
HAND_KS = (9, 27, 36, 64)
N_GENOMES = 4
GRID_K, GRID_ROWS = 31, 262144  # 2n vertices just past the capped grid's 524 288 threads
# the whole table is one path: the sizes of tests/test_graph_cases_host.py's whole tables (a chain of 2^j k-mers needs the jumps' last round)
WHOLE_NS = (1, 2, 3, 63, 64, 65, 1023, 1024, 1025)
WHOLE_KS = (27, 72)

_COMP = str.maketrans("ACGT", "TGCA")


def rc(s):
    return s.translate(_COMP)[::-1]


def canon(s):
    r = rc(s)
    return s if s <= r else r


def text(codes):
    return "".join("ACGT"[c] for c in np.asarray(codes).tolist())


def rows_of(kmers, k):
    """the stored k-mers in row order (the bft_gpu_extract order: ascending T-form)"""
    order = P.t_order(k).tolist()
    return sorted(kmers, key=lambda s: "".join(s[i] for i in order))


def owners_of(genomes, k, canonical=True):
    """[[sequence, ...] per genome] -> {k-mer: set of genome ids}, every window (its smaller strand when canonical)"""
    owners = {}
    for gid, seqs in enumerate(genomes):
        for q in seqs:
            for i in range(len(q) - k + 1):
                w = q[i:i + k]
                owners.setdefault(canon(w) if canonical else w, set()).add(gid)
    return owners


class Model:
    """The definition, literally.  Vertex ids are 2 * row + o."""

    def __init__(self, owners, k, rows=None):
        self.k, self.owners = k, owners
        self.rows = rows if rows is not None else rows_of(owners, k)
        self.row = {s: i for i, s in enumerate(self.rows)}
        n = len(self.rows)
        self.words = [None] * (2 * n)
        for i, s in enumerate(self.rows):
            self.words[2 * i], self.words[2 * i + 1] = s, rc(s)
        self.noncanonical = sum(1 for i in range(n) if self.words[2 * i] > self.words[2 * i + 1])
        row, words = self.row, self.words
        self.succ = []
        for v in range(2 * n):
            w1, r1 = words[v][1:], words[v ^ 1][:-1]
            out = []
            for c, cc in zip("ACGT", "TGCA"):
                y = w1 + c
                if y in row:
                    out.append(2 * row[y])
                else:
                    y = cc + r1  # rc(y)
                    if y in row:
                        out.append(2 * row[y] + 1)
            self.succ.append(out)

    def degrees(self):
        return bytes(len(self.succ[2 * i]) << 4 | len(self.succ[2 * i + 1]) for i in range(len(self.rows)))

    @functools.lru_cache(maxsize=None)
    def edges(self, t):
        n, succ, own = len(self.rows), self.succ, [self.owners[s] for s in self.rows]
        node = [len(succ[2 * i]) <= 1 and len(succ[2 * i + 1]) <= 1 and len(own[i]) >= t for i in range(n)]
        pal = [self.words[2 * i] == self.words[2 * i + 1] for i in range(n)]
        nxt = {}
        for u in range(2 * n):
            if len(succ[u]) != 1:
                continue
            v = succ[u][0]
            ru, rv = u >> 1, v >> 1
            if succ[v ^ 1] == [u ^ 1] and node[ru] and node[rv] and ru != rv and not pal[ru] and not pal[rv] and len(own[ru] & own[rv]) >= t:
                nxt[u] = v
        return node, nxt

    @functools.lru_cache(maxsize=None)
    def all_paths(self, t):
        """every maximal chain and every cycle (each rotation class once per orientation) as vertex lists: P and its mirror both"""
        node, nxt = self.edges(t)
        prv = {v: u for u, v in nxt.items()}
        assert len(prv) == len(nxt)
        chains, cycles, seen = [], [], set()
        for v in range(2 * len(self.rows)):
            if node[v >> 1] and v not in prv:
                p = [v]
                while p[-1] in nxt:
                    p.append(nxt[p[-1]])
                chains.append(p)
                seen.update(p)
        for v in range(2 * len(self.rows)):
            if node[v >> 1] and v not in seen:
                p = [v]
                while nxt[p[-1]] != v:
                    p.append(nxt[p[-1]])
                seen.update(p)
                i = p.index(min(p, key=lambda x: x >> 1))
                cycles.append(p[i:] + p[:i])  # from the vertex of its smallest row
        return node, nxt, chains, cycles

    def paths(self, t):
        """the reported paths as vertex lists, in ascending id of their first vertex"""
        _, _, chains, cycles = self.all_paths(t)
        kept = [p for p in chains if p[0] < (p[-1] ^ 1)] + [p for p in cycles if p[0] & 1 == 0]
        return sorted(kept, key=lambda p: p[0])

    def spell(self, p):
        return self.words[p[0]] + "".join(self.words[v][-1] for v in p[1:])

    def unitigs(self, t=0):
        return [self.spell(p) for p in self.paths(t)]

    def invariants(self, t):
        """the five invariants of the definition, on a canonical index"""
        assert self.noncanonical == 0
        node, nxt, chains, cycles = self.all_paths(t)
        assert all((v ^ 1) in nxt and nxt[v ^ 1] == (u ^ 1) for u, v in nxt.items())  # the edge relation is mirror-symmetric
        every = chains + cycles
        for p in every:
            rows = [v >> 1 for v in p]
            assert len(set(rows)) == len(rows)  # no path holds both orientations of a row
        as_sets = {}
        for p in every:
            as_sets.setdefault(frozenset(p), []).append(p)
        for p in every:
            mirror = frozenset(v ^ 1 for v in p)
            assert mirror != frozenset(p) and mirror in as_sets  # no path is its own mirror
        kept = self.paths(t)
        count = {}
        for p in kept:
            for v in p:
                count[v >> 1] = count.get(v >> 1, 0) + 1
        assert all(count.get(i, 0) == 1 for i in range(len(self.rows)) if node[i]) and all(node[i] for i in count)  # every node row: one kept path
        for p in kept:
            s = self.spell(p)
            assert len(s) == len(p) + self.k - 1
            assert all(canon(s[i:i + self.k]) in self.row for i in range(len(p)))  # every window of every spelling is represented
        assert [p[0] for p in kept] == sorted(p[0] for p in kept)
        return kept


def split(offsets, seqs):
    """(offsets, seqs) of BFT.unitigs -> list of strings"""
    s = bytes(bytearray(seqs)).decode()
    return [s[int(offsets[i]):int(offsets[i + 1])] for i in range(len(offsets) - 1)]


def check(model, t, got):
    """problems of `got` (a list of strings) as the unitigs of the model's index at threshold t; empty when it is exactly the truth"""
    want = model.unitigs(t)
    if got == want:
        return []
    out = []
    k, ws, gs = model.k, set(want), set(got)
    for s in got:
        if s in ws:
            continue
        if rc(s) in ws:
            out.append(f"mirror orientation: {s[:40]}")
        elif len(s) >= k and any(len(s) == len(w) and s[:len(s) - k + 1] in (w[:len(w) - k + 1] * 2) for w in ws):
            out.append(f"cycle from another vertex: {s[:40]}")
        elif any(canon(s[i:i + k]) == s[i:i + k] == rc(s[i:i + k]) for i in range(len(s) - k + 1)) and len(s) > k:
            out.append(f"palindrome joined: {s[:40]}")
        elif any(s[i:i + k] == rc(s[i + 1:i + 1 + k]) for i in range(len(s) - k)):
            out.append(f"hairpin joined: {s[:40]}")
        else:
            out.append(f"not a unitig: {s[:40]}")
    out += [f"missing: {s[:40]}" for s in want if s not in gs]
    if not out:
        out.append("order or multiplicity differs")
    return out


# ---- the cases (shared with the GPU tests; each built once) -------------------------------------------------------------------------------------
def related_genomes(seed, length):
    """Four related genomes as tests/test_gpu_simple_paths.py builds them: an ancestor with a repeated stretch, and SNP mutants of it."""
    rng = np.random.default_rng(seed)
    anc = S.random_genome(length, seed + 1)
    a = int(rng.integers(0, length // 3))
    b = int(rng.integers(length // 2, length - 400))
    anc[b:b + 300] = anc[a:a + 300]
    return [[text(g)] for g in [anc] + [S.mutate(anc, 0.01, seed + 2 + g) for g in range(N_GENOMES - 1)]]


@functools.lru_cache(maxsize=None)
def width_case(k, length=2500):
    """(genomes, model) of the key-width index at k"""
    genomes = related_genomes(1000 + k, length)
    return genomes, Model(owners_of(genomes, k), k)


def _rand(rng, n):
    return "".join(rng.choice(list("ACGT"), n))


@functools.lru_cache(maxsize=None)
def hand_parts(k):
    """name -> sequences of the hand-made situations that exist at this k"""
    rng = np.random.default_rng(500 + k)
    parts = {"lone": [_rand(rng, k)], "homopolymer": ["A" * (k + 3)]}
    circ = _rand(rng, 150)
    parts["circle"] = [circ + circ[:k - 1]]
    if k % 2 == 0:
        half = _rand(rng, k // 2)
        pal = half + rc(half)
        parts["palindrome, one neighbour word"] = ["G" + pal + "C"]       # G+pal[:-1] -> pal -> pal[1:]+C = rc of the first: out(pal) = 1
        half = _rand(rng, k // 2)
        pal = half + rc(half)
        parts["palindrome between two neighbours"] = ["G" + pal + "G"]    # two neighbour words: out(pal) = 2
        half = _rand(rng, k // 2)
        pal = half + rc(half)
        parts["palindromic successor"] = [_rand(rng, 3) + "A" + pal]      # ... -> A+pal[:-1] -> pal: the word counts once
    else:
        half = _rand(rng, (k - 1) // 2)
        parts["hairpin"] = [_rand(rng, 4) + "C" + half + rc(half) + "G"]  # x = C+P, then x[1:]+G = rc(x)
    while True:  # x with two successor words: one stored as itself, one as its reverse complement
        x = _rand(rng, k)
        y1, y2 = x[1:] + "A", x[1:] + "C"
        if canon(y1) == y1 != rc(y1) and canon(y2) != y2:
            break
    parts["two successors, two strands"] = [x + "A", x + "C"]
    if k >= 27:
        parts["chain"] = [_rand(rng, 3000 + k + 40)]  # (random at k >= 27: no repeat; the stored strand flips at about every other k-mer)
    return parts


@functools.lru_cache(maxsize=None)
def hand_case(k):
    """(genomes, model): genome 0 holds the circle, the chain, the lone k-mer and the homopolymer; genome 1 the rest"""
    parts = hand_parts(k)
    first = ("circle", "chain", "lone", "homopolymer")
    genomes = [sum((parts[n] for n in first if n in parts), []), sum((v for n, v in parts.items() if n not in first), [])]
    return genomes, Model(owners_of(genomes, k), k)


@functools.lru_cache(maxsize=None)
def grid_case():
    """(genomes, model): one genome with just over GRID_ROWS distinct canonical k-mers"""
    genomes = [[text(S.random_genome(GRID_ROWS + GRID_K + 300, 77))]]
    m = Model(owners_of(genomes, GRID_K), GRID_K)
    assert GRID_ROWS < len(m.rows) < GRID_ROWS + 400
    return genomes, m


@functools.lru_cache(maxsize=None)
def whole_case(n, kind, k):
    """(genomes, model): the index is exactly one chain or one cycle of n canonical k-mers, one genome.  (A random line or circle: the first seed
    whose k-mers are n rows in one path -- a circle of two letters may be its own reverse complement.)"""
    for attempt in range(50):
        rng = np.random.default_rng(21000 + 5000 * k + 2 * n + (kind == "cycle") + 100000 * attempt)
        q = _rand(rng, n) if kind == "cycle" else _rand(rng, n + k - 1)
        genomes = [[(q * (k // n + 2))[:n + k - 1] if kind == "cycle" else q]]  # (the circle read once around and k - 1 letters on)
        m = Model(owners_of(genomes, k), k)
        if len(m.rows) == n and [len(p) for p in m.paths(0)] == [n]:
            return genomes, m
    raise AssertionError((n, kind, k))


def noncanonical_case(k):
    """(k-mers of both strands for insert_kmers, model of that index): every k-mer of a short genome and of its reverse complement"""
    g = text(S.random_genome(400, 4242 + k))
    kmers = sorted({g[i:i + k] for i in range(len(g) - k + 1)} | {rc(g)[i:i + k] for i in range(len(g) - k + 1)})
    return kmers, Model({s: {0} for s in kmers}, k)


# ---- tests ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
def test_invariants_on_the_key_width_cases(k):
    _, m = width_case(k)
    for t in (0, 1, 2, N_GENOMES, N_GENOMES + 1):
        kept = m.invariants(t)
        assert (len(kept) == 0) == (t > N_GENOMES)
    assert len(m.unitigs(0)) >= 2 and max(map(len, m.unitigs(0))) > k


@pytest.mark.parametrize("k", HAND_KS)
def test_invariants_and_situations_of_the_hand_made_cases(k):
    _, m = hand_case(k)
    parts = hand_parts(k)
    for t in (0, 1, 2, 3):
        m.invariants(t)
    got = m.unitigs(0)
    if k == 9:
        return  # (a few hundred 9-mers touch each other by chance: the situations below are not isolated there, the invariants hold all the same)
    assert canon(parts["lone"][0]) in got and "A" * k in got
    circ = parts["circle"][0]
    ring2 = circ[:150] * 2
    assert sum(1 for s in got if len(s) == len(circ) and (s[:150] in ring2 or rc(s[:150]) in ring2)) == 1  # one cycle, one orientation
    if k % 2 == 0:
        pal1, pal2 = parts["palindrome, one neighbour word"][0][1:-1], parts["palindrome between two neighbours"][0][1:-1]
        assert pal1 == rc(pal1) and pal1 in got        # a node: always a path of its own
        assert pal2 == rc(pal2) and not any(pal2 in s for s in got)  # two successor words: in no path, its neighbours end there
        one = m.row[parts["palindrome, one neighbour word"][0][1:-1]]
        two = m.row[parts["palindrome between two neighbours"][0][1:-1]]
        assert m.degrees()[one] == 0x11 and m.degrees()[two] == 0x22
        q = parts["palindromic successor"][0]
        x = q[-k - 1:-1]
        v = 2 * m.row[canon(x)] + (canon(x) != x)
        assert len(m.succ[v]) == 1 and m.words[m.succ[v][0]] == q[-k:]
    else:
        q = parts["hairpin"][0]
        x = q[-k - 1:-1]
        assert rc(x) == q[-k:] and not any(x + "G" in s for s in got)  # (x+G is its own reverse complement: either strand would show it)
    x = parts["two successors, two strands"][0][:k]
    v = 2 * m.row[canon(x)] + (canon(x) != x)
    assert len(m.succ[v]) == 2 and sorted(u & 1 for u in m.succ[v]) == [0, 1]
    if "chain" in parts:
        long = max(got, key=len)
        assert len(long) >= 3000 + k - 1
        flips = [canon(long[i:i + k]) != long[i:i + k] for i in range(len(long) - k + 1)]
        assert sum(a != b for a, b in zip(flips, flips[1:])) > 500  # the orientation flips many times
        assert int(np.ceil(np.log2(len(m.rows) + 1))) >= 12


def test_a_circle_read_from_its_other_strand_is_the_same_index():
    for k in HAND_KS:
        circ = hand_parts(k)["circle"][0]
        assert owners_of([[circ]], k) == owners_of([[rc(circ)]], k)


def test_grid_case_invariants():
    _, m = grid_case()
    m.invariants(0)
    assert 2 * len(m.rows) > 524288


@pytest.mark.parametrize("k", WHOLE_KS)
@pytest.mark.parametrize("kind", ("chain", "cycle"))
@pytest.mark.parametrize("n", WHOLE_NS)
def test_whole_table_cases(n, kind, k):
    _, m = whole_case(n, kind, k)
    kept = m.invariants(0)
    _, _, chains, cycles = m.all_paths(0)
    assert len(m.rows) == n and len(kept) == 1 and len(m.spell(kept[0])) == n + k - 1
    assert (len(chains), len(cycles)) == ((0, 2) if kind == "cycle" and n > 1 else (2, 0))  # the path and its mirror (a cycle of one row: a self-loop, no edge)


def test_noncanonical_model_counts():
    kmers, m = noncanonical_case(27)
    assert m.noncanonical == sum(1 for s in kmers if s > rc(s)) > 0
    assert len(m.degrees()) == len(kmers)


def test_checker_reports_doctored_results():
    k = 36
    _, m = hand_case(k)
    want = m.unitigs(0)
    assert check(m, 0, list(want)) == []
    parts = hand_parts(k)
    # a path given in the mirror orientation
    i = max(range(len(want)), key=lambda j: len(want[j]))
    bad = list(want)
    bad[i] = rc(bad[i])
    assert any("mirror" in p for p in check(m, 0, bad))
    # a cycle started one vertex late
    i = next(j for j, s in enumerate(want) if len(s) == 150 + k - 1)
    body = want[i][:150]
    bad = list(want)
    bad[i] = (body[1:] + body[:1]) + (body[1:] + body[:1])[:k - 1]
    assert any("cycle" in p for p in check(m, 0, bad))
    # a palindrome joined to a neighbour
    q = parts["palindrome, one neighbour word"][0]
    pal = q[1:-1]
    bad = [s for s in want if s != pal and s not in (q[:k], rc(q[:k]))] + [q[:k + 1]]
    assert any("palindrome joined" in p for p in check(m, 0, bad))
    # a hairpin joined (odd k)
    k = 27
    _, m = hand_case(k)
    want = m.unitigs(0)
    q = hand_parts(k)["hairpin"][0]
    x = q[-k - 1:-1]
    i = next(j for j, s in enumerate(want) if s.endswith(x) or s.startswith(rc(x)))
    bad = list(want)
    bad[i] = want[i] + "G" if want[i].endswith(x) else "C" + want[i]
    probs = check(m, 0, bad)
    assert any("hairpin joined" in p for p in probs), probs
    assert check(m, 0, want[::-1]) and check(m, 0, want + want[-1:]) and check(m, 0, want[:-1])


def test_names_are_declared_exported_and_in_signatures():
    subprocess.check_call(["make", "-C", _lib.CSRC, "all"], stdout=subprocess.DEVNULL)
    hdr = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["bft_gpu_unitigs"][1]) == 8 and len(_lib.SIGNATURES["bft_gpu_bidirected_degrees_dev"][1]) == 5
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert set(NAMES) <= set(re.findall(r" T (bft_gpu_[a-z_0-9]+)", out))
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(_lib.CSRC, "libbft.so")]).decode()
    assert re.search(r" T extract_unitigs_to_disk$", out, flags=re.M)
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bft", "unitigs.h")).read(), flags=re.S)
    assert re.search(r"\bvoid\s+extract_unitigs_to_disk\s*\(\s*BFT\s*\*\s*graph\s*,\s*int\s+min_shared\s*,\s*char\s*\*\s*filename_output\s*\)\s*;", code)
    subprocess.run(["gcc", "-std=gnu99", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", "-I", os.path.join(ROOT, "include"), "-"],
                   input=b"#include <bft/unitigs.h>\nint main(void) { return 0; }\n", check=True)


def test_unitig_kernels_use_no_scratch_and_no_lds():
    """Every kernel of the unitigs -- the k_ug_* and the MIRRORED instantiations of k_sp_ends, k_sp_offsets and k_sp_spell -- at every key width:
    no scratch memory, no vector register spilled to it, no LDS."""
    subprocess.check_call(["make", "-C", _lib.CSRC, "all"], stdout=subprocess.DEVNULL)
    seen = {}
    for pat in ("k_ug_", "k_sp_"):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), pat], capture_output=True, text=True).stdout
        for line in out.splitlines()[1:]:
            if not line.strip():
                continue
            vgpr, sgpr, vspill, sspill, scratch, lds, maxwg, name = line.split(None, 7)
            m = re.search(r"(k_ug_[a-z]+)", name) or re.search(r"(k_sp_[a-z]+)<(?:\d+, )?true>", name)
            if not m:
                continue
            kernel = m.group(1) + ("<true>" if m.group(1).startswith("k_sp_") else "")
            seen[kernel] = seen.get(kernel, 0) + 1
            assert int(vspill) == 0 and int(scratch) == 0 and int(lds) == 0, line
            assert int(vgpr) <= 128, line  # (two workgroups of 256 threads per SIMD at least)
    assert set(seen) == KERNELS, seen
    assert all(seen[name] == 4 for name in ("k_ug_canon", "k_ug_degrees", "k_sp_spell<true>")), seen  # one per key width


def test_null_arguments_are_refused_before_any_device_work():
    lib = _lib.load()
    n1, n2 = C.c_uint64(), C.c_uint64()
    cnt = (C.c_uint64 * 4)()
    assert lib.bft_gpu_unitigs(None, 0, None, None, 0, 0, C.byref(n1), C.byref(n2)) == -1  # BFT_GPU_E_ARG
    assert lib.bft_gpu_unitigs(C.c_void_p(1), 0, None, None, 0, 0, None, C.byref(n2)) == -1
    assert lib.bft_gpu_unitigs(C.c_void_p(1), 0, None, None, 0, 0, C.byref(n1), None) == -1
    assert lib.bft_gpu_unitigs_dev(None, 0, None, None, 0, 0, cnt, None) == -1
    assert lib.bft_gpu_unitigs_dev(C.c_void_p(1), 0, None, None, 0, 0, None, None) == -1
    assert lib.bft_gpu_bidirected_degrees(None, None, 0, C.byref(n1)) == -1
    assert lib.bft_gpu_bidirected_degrees(C.c_void_p(1), None, 0, None) == -1
    assert lib.bft_gpu_bidirected_degrees_dev(None, None, 0, cnt, None) == -1
    assert lib.bft_gpu_bidirected_degrees_dev(C.c_void_p(1), None, 0, None, None) == -1
    assert "NULL" in lib.bft_gpu_last_error().decode()
