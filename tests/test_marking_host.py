"""Vertex marking, the part that needs no GPU: the ctypes binding declares every bft_gpu_marks_* symbol with the argument list of include/bft_gpu.h,
and the plain-Python ground truth the GPU tests compare against (MarkModel: a dict from k-mer to flag, the adjacency of the inserted k-mers, and a
literal model of the reference's BFS, DFS and BFS_subgraph loops, src/snippets.c:605-812) gives, on a five-vertex graph, the outcome written out
here by hand."""
import ctypes as C
import re

import numpy as np

from bloomfiltertrie_amd import _lib


class MarkModel:
    """flag[kmer] for every stored k-mer (ASCII); owners[kmer] = the set of genome ids that carry it.  The neighbours of x are the stored
    N + x[:-1] and x[1:] + N (get_neighbors: predecessors first, A C G T)."""

    def __init__(self, owners):
        self.owners = owners
        self.flag = {x: 0 for x in owners}

    def neighbors(self, x):
        return [y for y in [c + x[:-1] for c in "ACGT"] + [x[1:] + c for c in "ACGT"] if y in self.owners]

    def member(self, x, ids):
        """is_in_subgraph for strictly increasing ids; no ids (BFS / DFS): every k-mer."""
        return set(ids) <= self.owners[x]

    def bfs(self, kmer, through=0, to=1):
        """BFS (src/snippets.c:605-656) with V_NOT_VISITED = through, V_VISITED = to."""
        if self.flag[kmer] != through:
            return False
        self.flag[kmer] = to
        queue = [kmer]
        while queue:
            cur = queue.pop(0)
            for nb in self.neighbors(cur):
                if self.flag[nb] == through:
                    self.flag[nb] = to
                    queue.append(nb)
        return True

    def dfs(self, kmer, through=0, to=1):
        """DFS (src/snippets.c:743-762), with a stack of its own instead of the recursion."""
        if self.flag[kmer] != through:
            return False
        stack = [kmer]
        while stack:
            cur = stack.pop()
            if self.flag[cur] != through:
                continue
            self.flag[cur] = to
            stack.extend(reversed(self.neighbors(cur)))
        return True

    def bfs_subgraph(self, kmer, ids, through=0, to=1):
        """BFS_subgraph (src/snippets.c:667-735): every unvisited k-mer it looks at is marked, only the members are expanded."""
        if self.flag[kmer] != through:
            return False
        self.flag[kmer] = to
        if not self.member(kmer, ids):
            return False
        queue = [kmer]
        while queue:
            cur = queue.pop(0)
            for nb in self.neighbors(cur):
                if self.flag[nb] == through:
                    self.flag[nb] = to
                    if self.member(nb, ids):
                        queue.append(nb)
        return True

    def bfs_members(self, kmer, ids, through=0, to=1):
        """boundary = 0: the walk never leaves the eligible k-mers and marks nothing else."""
        if self.flag[kmer] != through or not self.member(kmer, ids):
            return False
        self.flag[kmer] = to
        queue = [kmer]
        while queue:
            cur = queue.pop(0)
            for nb in self.neighbors(cur):
                if self.flag[nb] == through and self.member(nb, ids):
                    self.flag[nb] = to
                    queue.append(nb)
        return True

    def reach(self, seeds, ids=(), through=0, to=1, boundary=False):
        """bft_gpu_marks_reach: the traversal called on the seeds in order.  (seed_new, [members painted, boundary painted, seeds absent])"""
        before = dict(self.flag)
        seed_new, absent = [], 0
        for s in seeds:
            if s not in self.flag:
                absent += 1
                seed_new.append(0)
            elif boundary:
                seed_new.append(int(self.bfs_subgraph(s, ids, through, to)))
            else:
                seed_new.append(int(self.bfs_members(s, ids, through, to)))
        changed = [x for x in self.flag if self.flag[x] != before[x]]
        members = sum(1 for x in changed if self.member(x, ids))
        return seed_new, [members, len(changed) - members, absent]

    def packed(self, row_of):
        """The flag array as bft_gpu_marks_read gives it: 4 rows per byte, row r in bits 2 (r % 4) .. + 1 of byte r // 4."""
        out = np.zeros((len(row_of) + 3) // 4, dtype=np.uint8)
        for x, r in row_of.items():
            out[r >> 2] |= self.flag[x] << (2 * (r & 3))
        return out


def test_lib_declares_every_marks_symbol_as_the_header_does():
    hdr = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER).read(), flags=re.S)
    ctype = {"bft_gpu*": C.c_void_p, "uint64_t": C.c_uint64, "uint32_t": C.c_uint32, "uint8_t": C.c_uint8, "int": C.c_int}
    want = ["begin", "end", "set", "set_dev", "get", "get_dev", "test_and_set", "test_and_set_dev", "fill", "fill_dev", "counts", "counts_dev", "select",
            "select_dev", "reach", "reach_dev", "read", "write"]
    seen = []
    for name, args in re.findall(r"\bint\s+bft_gpu_marks_([a-z_]+)\s*\(([^)]*)\)\s*;", hdr):
        seen.append(name)
        types = []
        for a in args.split(","):
            t = " ".join(a.replace("const", "").split()[:-1])  # (the last word is the argument's name)
            if t.endswith("*") and t != "bft_gpu*":
                # a pointer: void* in the binding, except the host counters passed by reference
                types.append((C.c_void_p, C.POINTER(C.c_uint64)) if t == "uint64_t*" else (C.c_void_p,))
            else:
                types.append((ctype[t],))
        res, argtypes = _lib.SIGNATURES["bft_gpu_marks_" + name]
        assert res is C.c_int, name
        assert len(argtypes) == len(types), (name, args)
        for got, ok in zip(argtypes, types):
            assert got in ok, (name, args, got)
    assert sorted(seen) == sorted(want)


def test_model_on_a_graph_worked_out_by_hand():
    """k = 3, five k-mers.  Edges: AAC - ACG, ACG - CGT, ACG - CGA (ACG branches); TTT has only itself as a neighbour.  Genome 0 carries all of
    them, genome 1 carries AAC, ACG and CGA."""
    owners = {"AAC": {0, 1}, "ACG": {0, 1}, "CGT": {0}, "CGA": {0, 1}, "TTT": {0}}
    m = MarkModel(owners)
    assert sorted(m.neighbors("ACG")) == ["AAC", "CGA", "CGT"]
    assert m.neighbors("TTT") == ["TTT", "TTT"]  # (a homopolymer is its own predecessor and successor)
    # the whole graph: two components
    assert [m.bfs(x) for x in ("CGT", "AAC", "TTT", "TTT")] == [True, False, True, False]
    assert m.flag == {x: 1 for x in owners}
    d = MarkModel(owners)
    assert [d.dfs(x) for x in ("CGT", "AAC", "TTT", "TTT")] == [True, False, True, False] and d.flag == m.flag
    # the sub-graph of genome 1 from AAC: AAC, ACG, CGA are members; CGT is looked at from ACG and marked, not expanded; TTT is never seen
    m = MarkModel(owners)
    assert m.bfs_subgraph("AAC", (1,)) is True
    assert m.flag == {"AAC": 1, "ACG": 1, "CGT": 1, "CGA": 1, "TTT": 0}
    # TTT is not a member: marked visited, no new component; a second call finds it visited
    assert m.bfs_subgraph("TTT", (1,)) is False and m.flag["TTT"] == 1
    assert m.bfs_subgraph("TTT", (1,)) is False
    # a barrier: ACG holds 2, so the walk from AAC stops there and the far side stays 0
    m = MarkModel(owners)
    m.flag["ACG"] = 2
    assert m.reach(["AAC"]) == ([1], [1, 0, 0])
    assert m.flag == {"AAC": 1, "ACG": 2, "CGT": 0, "CGA": 0, "TTT": 0}
    # reach: seeds in order, an absent one, other flag values, boundary on and off
    m = MarkModel(owners)
    assert m.reach(["CGA", "GGG", "AAC", "TTT"], ids=(1,), boundary=True) == ([1, 0, 0, 0], [3, 2, 1])
    assert m.flag == {x: 1 for x in owners}
    m = MarkModel(owners)
    assert m.reach(["CGA", "TTT"], ids=(1,), boundary=False) == ([1, 0], [3, 0, 0])
    assert m.flag == {"AAC": 1, "ACG": 1, "CGT": 0, "CGA": 1, "TTT": 0}
    assert m.reach(["ACG"], ids=(), through=1, to=3) == ([1], [3, 0, 0])
    assert m.flag == {"AAC": 3, "ACG": 3, "CGT": 0, "CGA": 3, "TTT": 0}
    row_of = {"AAC": 0, "ACG": 1, "CGA": 2, "CGT": 3, "TTT": 4}
    assert m.packed(row_of).tolist() == [3 | 3 << 2 | 3 << 4 | 0 << 6, 0]
