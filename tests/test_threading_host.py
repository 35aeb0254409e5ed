"""CPU-side tests of sequence threading through the compacted coloured graph (no GPU).  The truth model of include/bft_gpu.h's definition of
bft_gpu_thread_sequences -- positions, validity, strand, located positions, the three transitions, walks, steps, the eight counts -- written from that
text alone over the arrays of test_cgraph_host.Graph.arrays(), test_bubbles_host.segment_of and the rows of test_unitigs_host.Model.  The definition's
three consequences proved on every case the GPU tests run: the steps spell the sequence, no break between located neighbours at t = 0, the walks of
the reverse complement are the mirrors (steps on a palindromic single-k-mer segment stay +).  The sequence sets of the cases, the planted-variant
case whose walks pass through the branch of each genome, thresholds that leave rows in no segment and breaks, the malformed arrays of the device
form, the batch shapes.  The checker the GPU tests compare with, shown to report doctored results; the expected GAF text; the new names in the
headers and SIGNATURES, the symbols exported, the usage line; the k_th_* kernels without scratch memory, spills or LDS; NULL and limit arguments
refused before anything touches a device.  tests/test_gpu_threading.py runs the cases of this file on the GPU."""
import ctypes as C
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_bubbles_host as B  # noqa: E402
import test_cgraph_host as G  # noqa: E402
import test_unitigs_host as H  # noqa: E402

from bloomfiltertrie_amd import _lib, synth as S  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = {"k_th_locate<1>", "k_th_locate<2>", "k_th_locate<3>", "k_th_locate<4>", "k_th_flags", "k_th_emit", "k_th_close"}
NAMES = ("bft_gpu_thread_sequences", "bft_gpu_thread_sequences_dev")
NONE = 0xFFFFFFFF
_NORM = str.maketrans("acgtuU", "ACGTTT")
_COMP = str.maketrans("ACGT", "TGCA")


def norm(s):
    """upper case, U reads as T"""
    return s.translate(_NORM)


def rc_any(s):
    """the reverse complement of a sequence with characters outside ACGT, which stay what they are"""
    return norm(s).translate(_COMP)[::-1]


class Threading:
    """The definition, literally, over the graph arrays, the segment table and the index's rows (row: k-mer string -> row).  A seg_of entry >= 2S or a
    pos >= m_i is "in no segment"; a link list of more than 4 entries, past the links or with decreasing offsets is the empty list."""

    def __init__(self, k, row, seg_off, link_off, links, seg_of, pos, noncanonical=0, n_links=None):
        self.k, self.row, self.noncanonical = k, row, noncanonical
        self.so = [int(x) for x in seg_off]
        self.lo = [int(x) for x in link_off]
        self.lk = [int(x) for x in links]
        self.nl = len(self.lk) if n_links is None else n_links
        self.seg_of, self.pos = [int(x) for x in seg_of], [int(x) for x in pos]
        self.n2 = 2 * (len(self.so) - 1)

    def members(self, i):
        return max(0, self.so[i + 1] - self.so[i] - (self.k - 1)) if self.so[i + 1] >= self.so[i] else 0

    def out(self, X):
        a, b = self.lo[X], self.lo[X + 1]
        return self.lk[a:b] if a <= b <= self.nl and b - a <= 4 else []

    def locate(self, w):
        """(X, q) of a window, or one of "invalid", "absent", "noseg" """
        u = norm(w)
        if any(c not in "ACGT" for c in u):
            return "invalid"
        c = H.canon(u)
        sigma = 0 if u == c else 1
        r = self.row.get(c)
        if r is None:
            return "absent"
        so = self.seg_of[r]
        if so >= self.n2:
            return "noseg"
        X = so ^ sigma
        m = self.members(X >> 1)
        if self.pos[r] >= m:
            return "noseg"
        return X, (self.pos[r] if X & 1 == 0 else m - 1 - self.pos[r])

    def transition(self, a, b):
        (X, q), (Y, r) = a, b
        if Y == X and r == q + 1:
            return "inside"
        if q == self.members(X >> 1) - 1 and r == 0 and Y in self.out(X):
            return "across"
        return "break"

    def run(self, seqs):
        """(walks [[s, p0, n_w, q0], ...], walk_off, steps, counts [8])"""
        k = self.k
        walks, walk_off, steps = [], [], []
        cnt = {"positions": 0, "invalid": 0, "absent": 0, "noseg": 0, "break": 0}
        for s, q in enumerate(seqs):
            prev = None
            for p in range(len(q) - k + 1):
                cnt["positions"] += 1
                at = self.locate(q[p:p + k])
                if isinstance(at, str):
                    cnt[at] += 1
                    prev = None
                    continue
                kind = self.transition(prev, at) if prev is not None else "start"
                if kind == "break":
                    cnt["break"] += 1
                if kind in ("start", "break"):
                    walks.append([s, p, 0, at[1]])
                    walk_off.append(len(steps))
                if kind != "inside":
                    steps.append(at[0])
                walks[-1][2] += 1
                prev = at
        walk_off.append(len(steps))
        return walks, walk_off, steps, [len(walks), len(steps), cnt["positions"], cnt["invalid"], cnt["absent"], cnt["noseg"], cnt["break"], self.noncanonical]


def threading_of(g, **kw):
    """Threading over a test_cgraph_host.Graph (its arrays, its segment table, its model's rows)"""
    seg_off, _, link_off, links, members = g.arrays()
    seg_of, pos = B.segment_of(g.k, seg_off, members, len(g.m.rows))
    return Threading(g.k, g.m.row, seg_off, link_off, links, seg_of, pos, g.m.noncanonical, **kw)


def paths_of(g, result):
    """per walk: (the path's string -- its steps spelled with k - 1 overlap --, its steps)"""
    walks, walk_off, steps, _ = result
    out = []
    for w in range(len(walks)):
        st = steps[walk_off[w]:walk_off[w + 1]]
        out.append((g.spelled(st[0]) + "".join(g.spelled(x)[g.k - 1:] for x in st[1:]), st))
    return out


def consequences(g, th, seqs, result):
    """the three consequences of the definition, on one run of the model over a Graph g (a canonical index)"""
    k = g.k
    walks, walk_off, steps, counts = result
    assert counts[0] == len(walks) and counts[1] == len(steps) == walk_off[-1] and counts[7] == 0
    assert counts[2] == sum(max(0, len(q) - k + 1) for q in seqs)
    assert [(w[0], w[1]) for w in walks] == sorted((w[0], w[1]) for w in walks)  # ascending (s, p), one walk per start
    paths = paths_of(g, result)
    # 1. the steps spell the sequence
    for (s, p0, nw, q0), (path, st) in zip(walks, paths):
        assert nw >= 1 and len(st) >= 1 and p0 + nw + k - 1 <= len(seqs[s])
        assert path[q0:q0 + nw + k - 1] == norm(seqs[s][p0:p0 + nw + k - 1]), (s, p0)
        assert q0 + nw + k - 1 <= len(path)
        assert q0 < th.members(st[0] >> 1) and q0 + nw + k - 1 > len(path) - th.members(st[-1] >> 1)  # no step is empty
    # 2. at t = 0 every break is an invalid or absent window
    if g.t == 0:
        assert counts[5] == 0 and counts[6] == 0
    # 3. the walks of rc(sequence) are the mirrors; steps on a palindromic single-k-mer segment stay +
    flip = lambda x: x if g.palindromic(x >> 1) else x ^ 1  # noqa: E731
    mirror = th.run([rc_any(q) for q in seqs])
    assert mirror[3] == counts
    by_seq, m_by_seq = {}, {}
    for (w, (path, st)) in zip(walks, paths):
        by_seq.setdefault(w[0], []).append((w, len(path), st))
    for (w, (path, st)) in zip(mirror[0], paths_of(g, mirror)):
        m_by_seq.setdefault(w[0], []).append((w, len(path), st))
    assert set(by_seq) == set(m_by_seq)
    for s, items in by_seq.items():
        want = [([s, len(seqs[s]) - (w[1] + w[2] + k - 1), w[2], plen - (w[3] + w[2] + k - 1)], plen, [flip(x) for x in reversed(st)]) for w, plen, st in reversed(items)]
        assert m_by_seq[s] == want, s
    return paths


def check(want, got):
    """problems of got = (walks [n, 4], walk_off, steps, counts) as the truth want = Threading.run(); empty when it is exactly that"""
    walks, walk_off, steps, counts = want
    g_walks = [[int(x) for x in w] for w in got[0]]
    g_off, g_steps, g_counts = [int(x) for x in got[1]], [int(x) for x in got[2]], [int(x) for x in got[3]]
    if (g_walks, g_off, g_steps, g_counts) == (walks, walk_off, steps, counts):
        return []
    out = []
    have = {(w[0], w[1]): i for i, w in enumerate(g_walks)}
    for i, w in enumerate(walks):
        j = have.get((w[0], w[1]))
        if j is None:
            out.append(f"walk of sequence {w[0]} at {w[1]} missing")
            continue
        if g_walks[j] != w:
            out.append(f"walk of sequence {w[0]} at {w[1]}: {g_walks[j]}, not {w}")
        if j + 1 < len(g_off) and g_steps[g_off[j]:g_off[j + 1]] != steps[walk_off[i]:walk_off[i + 1]]:
            mine, theirs = steps[walk_off[i]:walk_off[i + 1]], g_steps[g_off[j]:g_off[j + 1]]
            out.append(f"walk of sequence {w[0]} at {w[1]}: " + ("steps on the other strand" if theirs == [x ^ 1 for x in mine] else f"steps {theirs[:8]}, not {mine[:8]}"))
    starts = {(w[0], w[1]) for w in walks}
    out += [f"walk of sequence {w[0]} at {w[1]} is none" for w in g_walks if (w[0], w[1]) not in starts]
    if not out and g_walks != walks:
        out.append("walks: order or multiplicity differs")
    if len(g_off) != len(walk_off) or (not out and g_off != walk_off):
        out.append("walk offsets differ")
    if g_counts != counts:
        out.append(f"counts {g_counts}, not {counts}")
    if not out:
        out.append("steps differ")
    return out


def expected_gaf(g, names, seqs, result):
    """the file of thread_sequences_to_disk (<bft/unitigs.h>) and of the command line's -thread for the model's result over the graph g"""
    k = g.k
    walks, walk_off, steps, _ = result
    lines = []
    for w, (s, p0, nw, q0) in enumerate(walks):
        st = steps[walk_off[w]:walk_off[w + 1]]
        plen = sum(len(g.seqs[x >> 1]) for x in st) - (len(st) - 1) * (k - 1)
        span = nw + k - 1
        path = "".join(("<" if x & 1 else ">") + str(x >> 1) for x in st)
        lines.append(f"{names[s]}\t{len(seqs[s])}\t{p0}\t{p0 + span}\t+\t{path}\t{plen}\t{q0}\t{q0 + span}\t{span}\t{span}\t255\tcg:Z:{span}=")
    return "".join(line + "\n" for line in lines)


def joins_to_gfa(text, gfa, seqs_by_name):
    """every line of a GAF file names segments of the GFA file, and its path, spelled from the S lines, holds the sequence's stretch where it says"""
    S_ = {f[1]: f[2] for f in (line.split("\t") for line in gfa.split("\n")) if f[0] == "S"}
    k = int(re.search(r"kl:i:(\d+)", gfa).group(1))
    lines = [line.split("\t") for line in text.split("\n") if line]
    for f in lines:
        st = re.findall(r"([<>])([^<>]+)", f[5])
        if not st or any(i not in S_ for _, i in st):
            return False
        spelled = [S_[i] if o == ">" else H.rc(S_[i]) for o, i in st]
        path = spelled[0] + "".join(x[k - 1:] for x in spelled[1:])
        if len(path) != int(f[6]) or path[int(f[7]):int(f[8])] != norm(seqs_by_name[f[0]][int(f[2]):int(f[3])]):
            return False
    return bool(lines)


# ---- the sequence sets ----------------------------------------------------------------------------------------------------------------------------
def doctored(q, seed):
    """a copy with N, n, a lowercase stretch and U planted"""
    rng = np.random.default_rng(seed)
    c = list(q)
    n = len(c)
    if n < 40:
        return q
    a = int(rng.integers(0, n // 4))
    c[a:a + n // 5] = [x.lower() for x in c[a:a + n // 5]]
    for at, ch in ((n // 3, "N"), (n // 2, "n"), (2 * n // 3 + 1, "N")):
        c[at] = ch
    for at in range(n // 2 + 5, n, 17):
        if c[at] in "Tt":
            c[at] = "U" if c[at] == "T" else "u"
    return "".join(c)


def sequence_set(genomes, k, seed, extra=()):
    """the sequences a case is threaded with: every genome sequence, its reverse complement, a doctored copy, a random foreign sequence, sequences of
    length 0, k - 1, k and k + 1, and the case's extras"""
    src = [q for seqs in genomes for q in seqs]
    out = list(src) + [H.rc(q) for q in src] + [doctored(q, seed + j) for j, q in enumerate(src)]
    out.append(H.text(S.random_genome(300 + k, 90000 + seed)))
    long = max(src, key=len)
    out += ["", long[5:5 + k - 1], long[7:7 + k], long[9:9 + k + 1]]
    return out + list(extra)


@functools.lru_cache(maxsize=None)
def width_sequences(k):
    return sequence_set(H.width_case(k)[0], k, 3000 + k)


@functools.lru_cache(maxsize=None)
def hand_sequences(k):
    """the hand-made case's set, with the circle read 2.5 times round in front (sequence 0 of the extras)"""
    genomes, _ = H.hand_case(k)
    parts = H.hand_parts(k)
    circ = parts["circle"][0][:150]
    extra = [(circ * 3)[:375 + k - 1]]
    for name in ("hairpin", "palindrome, one neighbour word", "palindrome between two neighbours", "palindromic successor", "homopolymer", "two successors, two strands"):
        extra += parts.get(name, [])
    base = sequence_set(genomes, k, 4000 + k)
    return base + extra, len(base)


@functools.lru_cache(maxsize=None)
def planted_sequences(k):
    return sequence_set(B.planted_case(k)[0], k, 5000 + k)


@functools.lru_cache(maxsize=None)
def grid_sequences():
    q = H.grid_case()[0][0][0]
    return [q, H.rc(q)]


@functools.lru_cache(maxsize=None)
def batch_shapes(k=27):
    """several hundred short pieces of the key-width case's first genome whose lengths put the sequence boundaries one before, at and one behind
    every multiple of 64 positions (so of 256 too) up to 7680; empty sequences first, in the middle and last; an N at the first, the middle and the
    last character of a window"""
    src = H.width_case(k)[0][0][0]
    rng = np.random.default_rng(611)
    bounds = sorted({m + d for m in range(64, 64 * 121, 64) for d in (-1, 0, 1)})
    out, at = [""], 0
    for b in bounds:
        npos = b - at
        a = int(rng.integers(0, len(src) - (npos + k - 1)))
        out.append(src[a:a + npos + k - 1])
        at = b
        if b == 64 * 60:
            out += ["", "A" * (k - 1), ""]
    piece = src[100:100 + k + 5]
    for where in (0, k // 2, k - 1):
        out.append(piece[:where] + "N" + piece[where + 1:])
    out.append("")
    return out


def malformed(arrays, seg_of, pos, k):
    """[(name, (seg_off, link_off, links, n_links, seg_of, pos))]: the device form's bad input over a graph's arrays -- seg_of entries >= 2S, pos >= m_i, a
    five-entry link list, link offsets past n_links"""
    seg_off, _, link_off, links, _ = arrays
    ns = len(seg_off) - 1
    so, ps = np.array(seg_of, dtype=np.uint32), np.array(pos, dtype=np.uint32)
    rows = [r for r in range(len(so)) if so[r] != NONE]
    cases = []
    a = so.copy()
    a[rows[::7]] = 2 * ns
    a[rows[3::11]] = NONE - 1
    cases.append(("seg_of entries >= 2S", (seg_off, link_off, links, len(links), a, ps)))
    b = ps.copy()
    for r in rows[::5]:
        i = int(so[r]) >> 1
        b[r] = int(seg_off[i + 1]) - int(seg_off[i]) - (k - 1) + (r % 3)
    cases.append(("pos >= m_i", (seg_off, link_off, links, len(links), so, b)))
    # a five-entry list: the first list that is not empty gets entries until it has five (the lists behind it move on)
    A = next(x for x in range(2 * ns) if link_off[x + 1] > link_off[x])
    have = int(link_off[A + 1] - link_off[A])
    at = int(link_off[A + 1])
    lk5 = np.concatenate([links[:at], np.full(5 - have, links[at - 1], dtype=np.uint32), links[at:]])
    lo5 = link_off.copy()
    lo5[A + 1:] += np.uint64(5 - have)
    cases.append(("a five-entry link list", (seg_off, lo5, lk5, len(lk5), so, ps)))
    cases.append(("link offsets past n_links", (seg_off, link_off, links, len(links) // 2, so, ps)))
    return cases


# ---- tests ----------------------------------------------------------------------------------------------------------------------------------------
def _prove(g, seqs):
    th = threading_of(g)
    result = th.run(seqs)
    consequences(g, th, seqs, result)
    return th, result


@pytest.mark.parametrize("k", H.KS)
def test_consequences_on_the_key_width_cases(k):
    seqs = width_sequences(k)
    genomes, _ = H.width_case(k)
    for t in G.THRESHOLDS:
        _, (walks, _, _, counts) = _prove(G.graph("width_case", k, t), seqs)
        if t == 0:
            # a genome sequence and its reverse complement are one walk each; the doctored copies are cut at their three N
            assert [w[:3] for w in walks[:2 * len(genomes)]] == [[s, 0, len(seqs[s]) - k + 1] for s in range(2 * len(genomes))]
            assert counts[3] > 0 and counts[4] > 0
        if t == H.N_GENOMES + 1:
            assert counts[:2] == [0, 0] and counts[5] == counts[2] - counts[3] - counts[4] > 0


def test_thresholds_leave_rows_in_no_segment_and_breaks():
    """the two roads that t = 0 never takes are taken: positions present but in no segment, and breaks between two located neighbours"""
    noseg = breaks = 0
    for k in H.KS:
        for t in G.THRESHOLDS[1:]:
            counts = threading_of(G.graph("width_case", k, t)).run(width_sequences(k))[3]
            noseg += counts[5] > 0
            breaks += counts[6] > 0
    assert noseg > 0 and breaks > 0


@pytest.mark.parametrize("k", H.HAND_KS)
def test_consequences_and_situations_of_the_hand_made_cases(k):
    seqs, n_base = hand_sequences(k)
    parts = H.hand_parts(k)
    for t in (0, 1, 2):
        g = G.graph("hand_case", k, t)
        th, result = _prove(g, seqs)
        if t:
            continue
        walks, walk_off, steps, _ = result
        by_seq = {}
        for w, (s, p0, nw, q0) in enumerate(walks):
            by_seq.setdefault(s, []).append((p0, nw, q0, steps[walk_off[w]:walk_off[w + 1]]))
        # the circle read 2.5 times round: one walk, the one cyclic unitig again and again on one strand
        (p0, nw, q0, st), = by_seq[n_base]
        # (at k = 9 the circle shares k-mers with the other parts and is cut into a few segments: the same ones round after round)
        round_ = list(dict.fromkeys(st))
        assert p0 == 0 and nw == 375 and sum(th.members(x >> 1) for x in round_) == 150 and st == [round_[i % len(round_)] for i in range(len(st))]
        assert (len(round_) == 1 and len(st) in (3, 4)) or (k == 9 and len(st) > 2 * len(round_))
        # the homopolymer: one step per window
        s = seqs.index("A" * (k + 3), n_base)
        (p0, nw, q0, st), = by_seq[s]
        assert nw == 4 and len(st) == 4 and len(set(st)) == 1 and q0 == 0
        if "hairpin" in parts:
            s = seqs.index(parts["hairpin"][0], n_base)
            assert any(a ^ 1 == b for _, _, _, st in by_seq[s] for a, b in zip(st, st[1:]))  # S+ S-
        for name in ("palindrome, one neighbour word", "palindrome between two neighbours", "palindromic successor"):
            if name in parts:
                s = seqs.index(parts[name][0], n_base)
                pal = [x for _, _, _, st in by_seq[s] for x in st if g.palindromic(x >> 1)]
                assert pal and all(x & 1 == 0 for x in pal)  # a palindromic segment is always read as +
        for q in parts["two successors, two strands"]:
            s = seqs.index(q, n_base)
            assert sum(nw for _, nw, _, _ in by_seq[s]) == 2 and sum(len(st) for _, _, _, st in by_seq[s]) == 2  # two windows, two segments, one walk


@pytest.mark.parametrize("k", B.PLANTED_KS)
def test_planted_genomes_take_their_own_branches(k):
    genomes, _, sites = B.planted_case(k)
    g = B.planted_graph(k)
    seqs = planted_sequences(k)
    th, result = _prove(g, seqs)
    walks, walk_off, steps, counts = result
    inter = g.colour_sets("and")
    truth = B.planted_truth(k)
    assert len(truth) == 4
    for gid in range(4):
        (w,) = [i for i, x in enumerate(walks) if x[0] == gid]  # a genome is one walk, end to end
        assert walks[w][1:3] == [0, len(seqs[gid]) - k + 1]
        st = {x >> 1 for x in steps[walk_off[w]:walk_off[w + 1]]}
        for rec, _, _ in truth:
            taken = [x >> 1 for x in rec[2:] if x != NONE and x >> 1 in st]
            assert len(taken) == 1 and gid in inter[taken[0]]  # exactly the branch whose AND colour set holds the genome
            assert rec[0] >> 1 in st and rec[1] >> 1 in st


def test_grid_case():
    seqs = grid_sequences()
    g = G.graph("grid_case", 0)
    _, (walks, walk_off, steps, counts) = _prove(g, seqs)
    assert counts[2] > B.GRID_LANES and counts[2] == 2 * (len(seqs[0]) - H.GRID_K + 1)
    assert [w[:3] for w in walks] == [[0, 0, counts[2] // 2], [1, 0, counts[2] // 2]] and counts[3:7] == [0, 0, 0, 0]


def test_batch_shapes_and_malformed_arrays():
    k = 27
    seqs = batch_shapes(k)
    assert len(seqs) > 300 and seqs[0] == "" and seqs[-1] == "" and "" in seqs[100:250]
    npos = np.cumsum([max(0, len(q) - k + 1) for q in seqs])
    for m in (64, 256, 1024, 4096):
        assert {m - 1, m, m + 1} <= set(npos.tolist())
    g = G.graph("width_case", k, 0)
    th, result = _prove(g, seqs)
    assert result[3][3] == 1 + 6 + 6  # an N at the first character of a window spoils that one window, at the middle or the last one all six of its piece
    arrays = g.arrays()
    seg_of, pos = B.segment_of(k, arrays[0], arrays[4], len(g.m.rows))
    base = th.run(width_sequences(k))
    for name, (so, lo, lk, nl, sg, ps) in malformed(arrays, seg_of, pos, k):
        res = Threading(k, g.m.row, so, lo, lk, sg, ps, n_links=nl).run(width_sequences(k))
        assert res != base and res[3][2:5] == base[3][2:5], name
        assert (res[3][5] > 0) == ("seg_of" in name or "pos" in name) and (res[3][6] > 0) == ("link" in name), name


def test_noncanonical_model_counts():
    kmers, m = H.noncanonical_case(27)
    assert m.noncanonical > 0


def test_checker_reports_doctored_results():
    k = 27
    th = threading_of(G.graph("width_case", k, 2))
    want = th.run(width_sequences(k))
    walks, walk_off, steps, counts = want
    assert len(walks) >= 4 and len(steps) > len(walks)
    assert check(want, (np.array(walks, dtype=np.uint64), np.array(walk_off, dtype=np.uint64), np.array(steps, dtype=np.uint32), np.array(counts, dtype=np.uint64))) == []
    # a dropped walk
    assert any("missing" in p for p in check(want, (walks[:1] + walks[2:], walk_off[:1] + walk_off[2:], steps, counts)))
    # a walk on the other strand
    flipped = list(steps)
    for j in range(walk_off[1], walk_off[2]):
        flipped[j] ^= 1
    assert any("other strand" in p for p in check(want, (walks, walk_off, flipped, counts)))
    # a wrong length, a wrong index in the first step, an invented walk, a count
    w = [list(x) for x in walks]
    w[2][2] += 1
    assert any("not" in p for p in check(want, (w, walk_off, steps, counts)))
    w = [list(x) for x in walks]
    w[0][3] += 1
    assert check(want, (w, walk_off, steps, counts))
    assert any("is none" in p for p in check(want, (walks + [[10 ** 6, 0, 1, 0]], walk_off + [walk_off[-1]], steps, counts)))
    assert check(want, (walks, walk_off, steps, counts[:6] + [counts[6] + 1, 0])) and check(want, (walks, walk_off, steps[:-1] + [steps[-1] ^ 1], counts))
    assert check(want, (walks[::-1], walk_off, steps, counts))


def test_expected_gaf_of_the_planted_case():
    k = 27
    g = B.planted_graph(k)
    seqs = planted_sequences(k)
    names = [f"s{i}" for i in range(len(seqs))]
    text = expected_gaf(g, names, seqs, threading_of(g).run(seqs))
    lines = text.split("\n")
    assert lines[-1] == "" and len(lines) - 1 >= 8 + 4 * 4
    f = lines[0].split("\t")
    assert len(f) == 13 and f[0] == "s0" and f[4] == "+" and f[11] == "255" and f[12] == f"cg:Z:{f[9]}=" and f[9] == f[10]
    assert int(f[3]) - int(f[2]) == int(f[8]) - int(f[7]) == int(f[9]) == len(seqs[0]) and int(f[1]) == len(seqs[0])
    gfa = f"H\tVN:Z:1.0\tkl:i:{k}\n" + "".join(f"S\t{j}\t{q}\tLN:i:{len(q)}\n" for j, q in enumerate(g.seqs))
    by_name = dict(zip(names, seqs))
    used = re.findall(r"[<>](\d+)", f[5])[0]
    assert joins_to_gfa(text, gfa, by_name) and not joins_to_gfa(text, gfa.replace(f"S\t{used}\t", "S\tx\t"), by_name)


def test_names_are_declared_exported_and_in_signatures():
    subprocess.check_call(["make", "-C", _lib.CSRC, "all"], stdout=subprocess.DEVNULL)
    hdr = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["bft_gpu_thread_sequences"][1]) == 18 and len(_lib.SIGNATURES["bft_gpu_thread_sequences_dev"][1]) == 20
    for name, n in zip(NAMES, (18, 20)):
        decl = re.search(r"\b" + name + r"\s*\(([^;]*)\)\s*;", hdr).group(1)
        assert len(decl.split(",")) == n, name
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert set(NAMES) | {"bft_seqfile_read_named"} <= set(re.findall(r" T ([a-z_0-9]+)", out))
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(_lib.CSRC, "libbft.so")]).decode()
    assert re.search(r" T thread_sequences_to_disk$", out, flags=re.M)
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bft", "unitigs.h")).read(), flags=re.S)
    assert re.search(r"\bvoid\s+thread_sequences_to_disk\s*\(\s*BFT\s*\*\s*graph\s*,\s*int\s+min_shared\s*,\s*char\s*\*\s*filename_sequences\s*,\s*char\s*\*\s*filename_output\s*\)\s*;", code)
    from bloomfiltertrie_amd import BFT
    assert all(hasattr(BFT, name) for name in ("thread_sequences", "thread_sequences_dev", "thread"))
    usage = subprocess.run([os.path.join(_lib.CSRC, "bft_gpu")], capture_output=True, text=True)
    assert usage.returncode != 0 and "[-thread min_shared sequence_file output_file]" in usage.stderr


def test_headers_compile_as_c():
    for inc in ("bft_gpu.h", "bft/unitigs.h"):
        subprocess.run(["gcc", "-std=gnu99", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", "-I", os.path.join(ROOT, "include"), "-"],
                       input=f"#include <{inc}>\nint main(void) {{ return 0; }}\n".encode(), check=True)


def test_threading_kernels_use_no_scratch_no_spill_and_no_lds():
    """Every k_th_* kernel, once: no scratch memory, no vector register spilled to it, no LDS, 128 VGPRs at the most"""
    subprocess.check_call(["make", "-C", _lib.CSRC, "all"], stdout=subprocess.DEVNULL)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "k_th_"], capture_output=True, text=True).stdout
    seen = {}
    for line in out.splitlines()[1:]:
        if not line.strip():
            continue
        vgpr, sgpr, vspill, sspill, scratch, lds, maxwg, name = line.split(None, 7)
        kernel = re.search(r"(k_th_[a-z]+(<\d>)?)", name).group(1)
        seen[kernel] = seen.get(kernel, 0) + 1
        assert int(vspill) == 0 and int(scratch) == 0 and int(lds) == 0, line
        assert int(vgpr) <= 128, line
    assert set(seen) == KERNELS and all(v == 1 for v in seen.values()), seen


def test_null_and_limit_arguments_are_refused_before_any_device_work():
    lib = _lib.load()
    cnt = (C.c_uint64 * 8)()
    one = C.c_void_p(1)
    off = (C.c_uint64 * 2)(0, 10)
    offp = C.cast(off, C.c_void_p)
    host = lib.bft_gpu_thread_sequences
    dev = lib.bft_gpu_thread_sequences_dev
    assert host(None, None, None, 0, None, None, 0, None, 0, None, None, 0, None, None, 0, None, 0, cnt) == -1  # BFT_GPU_E_ARG
    assert host(one, None, None, 0, None, None, 0, None, 0, None, None, 0, None, None, 0, None, 0, None) == -1
    assert host(one, b"ACGT", None, 1, None, None, 0, None, 0, None, None, 0, None, None, 0, None, 0, cnt) == -1   # sequences without offsets
    assert host(one, None, offp, 1, None, None, 0, None, 0, None, None, 0, None, None, 0, None, 0, cnt) == -1      # ... without characters
    assert host(one, b"ACGT", offp, 1, None, one, 1, None, 0, None, None, 0, None, None, 0, None, 0, cnt) == -1   # rows without a segment table
    assert host(one, b"ACGT", offp, 1, one, None, 1, None, 0, None, None, 0, None, None, 0, None, 0, cnt) == -1
    assert host(one, b"ACGT", offp, 1, None, None, 0, None, 1, one, None, 0, None, None, 0, None, 0, cnt) == -1   # segments without offsets
    assert host(one, b"ACGT", offp, 1, None, None, 0, one, 1, None, None, 0, None, None, 0, None, 0, cnt) == -1   # ... without link offsets
    assert host(one, b"ACGT", offp, 1, None, None, 0, one, 1, one, None, 1, None, None, 0, None, 0, cnt) == -1    # links without an array
    assert dev(None, None, None, 0, 0, None, None, 0, None, 0, None, None, 0, None, None, 0, None, 0, cnt, None) == -1
    assert dev(one, None, None, 0, 0, None, None, 0, None, 0, None, None, 0, None, None, 0, None, 0, None, None) == -1
    assert dev(one, one, None, 1, 4, None, None, 0, None, 0, None, None, 0, None, None, 0, None, 0, cnt, None) == -1
    assert dev(one, None, one, 1, 4, None, None, 0, None, 0, None, None, 0, None, None, 0, None, 0, cnt, None) == -1
    assert dev(one, one, one, 1, 4, None, one, 1, None, 0, None, None, 0, None, None, 0, None, 0, cnt, None) == -1
    assert dev(one, one, one, 1, 4, None, None, 0, one, 1, None, None, 0, None, None, 0, None, 0, cnt, None) == -1
    assert dev(one, one, one, 1, 4, None, None, 0, one, 1, one, None, 1, None, None, 0, None, 0, cnt, None) == -1
    assert "NULL" in lib.bft_gpu_last_error().decode()
    down = (C.c_uint64 * 3)(0, 10, 9)
    assert host(one, b"ACGT", C.cast(down, C.c_void_p), 2, None, None, 0, None, 0, None, None, 0, None, None, 0, None, 0, cnt) == -1
    assert "decrease" in lib.bft_gpu_last_error().decode()
    big = (C.c_uint64 * 2)(0, 1 << 32)
    assert host(one, b"ACGT", C.cast(big, C.c_void_p), 1, None, None, 0, None, 0, None, None, 0, None, None, 0, None, 0, cnt) == -3  # BFT_GPU_E_LIMIT
    assert "2^32" in lib.bft_gpu_last_error().decode()
    assert dev(one, one, one, 1, 1 << 32, None, None, 0, None, 0, None, None, 0, None, None, 0, None, 0, cnt, None) == -3
    assert dev(one, one, one, 1 << 32, 4, None, None, 0, None, 0, None, None, 0, None, None, 0, None, 0, cnt, None) == -3
    assert dev(one, one, one, 1, 4, None, None, 0, one, 1 << 31, one, None, 0, None, None, 0, None, 0, cnt, None) == -3 and "2^31" in lib.bft_gpu_last_error().decode()


def test_named_sequence_file_reader(tmp_path):
    """bft_seqfile_read_named: the names are the headers up to the first blank, an empty name is the record's number; the sequences are those of
    bft_seqfile_read"""
    lib = C.CDLL(_lib.LIB_PATH)
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    fa = tmp_path / "r.fa"
    fa.write_text(">one first record\nACGT\nAC\n>\nGG\n>three\ttab\n\n> blank first\nT\r\n")
    fq = tmp_path / "r.fq"
    fq.write_text("@one first record\nACGTAC\n+\nIIIIII\n@\nGG\n+\nII\n@three\ttab\n\n+\n\n@ blank first\nT\n+\nI")
    for path in (fa, fq):
        blob, names = C.c_void_p(), C.c_void_p()
        off, noff = C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint64)()
        n = C.c_uint64()
        assert lib.bft_seqfile_read_named(os.fsencode(str(path)), C.byref(blob), C.byref(off), C.byref(names), C.byref(noff), C.byref(n)) == 0
        assert n.value == 4
        text = C.string_at(blob, off[4])
        assert [text[off[i]:off[i + 1]] for i in range(4)] == [b"ACGTAC", b"GG", b"", b"T"]
        raw = C.string_at(names, noff[4])
        assert [raw[noff[i]:noff[i + 1]] for i in range(4)] == [b"one\0", b"1\0", b"three\0", b"3\0"]
        blob2, off2, n2 = C.c_void_p(), C.POINTER(C.c_uint64)(), C.c_uint64()
        assert lib.bft_seqfile_read(os.fsencode(str(path)), C.byref(blob2), C.byref(off2), C.byref(n2)) == 0
        assert n2.value == 4 and [off2[i] for i in range(5)] == [off[i] for i in range(5)] and C.string_at(blob2, off2[4]) == text
        for p in (blob, names, blob2, C.cast(off, C.c_void_p), C.cast(noff, C.c_void_p), C.cast(off2, C.c_void_p)):
            libc.free(p)
    blob, names = C.c_void_p(), C.c_void_p()
    off, noff = C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint64)()
    n = C.c_uint64()
    args = (C.byref(blob), C.byref(off), C.byref(names), C.byref(noff), C.byref(n))
    assert lib.bft_seqfile_read_named(os.fsencode(str(tmp_path / "none.fa")), *args) == -1 and not blob.value and not names.value
    (tmp_path / "bad.txt").write_text("ACGT\n")
    assert lib.bft_seqfile_read_named(os.fsencode(str(tmp_path / "bad.txt")), *args) == -2 and not blob.value and not names.value
    (tmp_path / "cut.fq").write_text("@a\nACGT\n+\nII\n")
    assert lib.bft_seqfile_read_named(os.fsencode(str(tmp_path / "cut.fq")), *args) == -2 and not blob.value and not names.value
    (tmp_path / "empty.fa").write_text("\n \n")
    assert lib.bft_seqfile_read_named(os.fsencode(str(tmp_path / "empty.fa")), *args) == 0 and n.value == 0 and noff[0] == 0
    for p in (blob, names, C.cast(off, C.c_void_p), C.cast(noff, C.c_void_p)):
        libc.free(p)
