"""set_marking / unset_marking / set_flag_kmer / get_flag_kmer of the reference's bft.h and the traversal snippets that need them (BFS, DFS,
BFS_subgraph through iterate_over_kmers and nb_connected_components, cdbg_traversal; src/bft.c:686-765, src/snippets.c:605-930):
tests/c/ref_marking_program.c, compiled with -Werror against the headers as a position-independent and as a fixed-address executable, marks and
traverses an index of three genomes; flags and counts are checked against ground truth computed in Python from the inserted k-mers
(test_marking_host.MarkModel), and the three error paths against the reference's messages."""
import os
import subprocess

import pytest

from bloomfiltertrie_amd import BFT, _lib, synth as S

from test_gpu_components import _owners_of, _row_of, _truth
from test_marking_host import MarkModel

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "ref_marking_program.c")
K = 27


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    subprocess.check_call(["make", "-C", _lib.CSRC, "all"], stdout=subprocess.DEVNULL)
    d = tmp_path_factory.mktemp("marking")
    exes = {}
    for form, flags in (("pie", []), ("nopie", ["-no-pie"])):
        exe = str(d / f"ref_marking_program_{form}")
        subprocess.check_call(["gcc", "-O2", "-std=gnu99", "-Wall", "-Werror"] + flags + ["-I", os.path.join(ROOT, "include"), "-o", exe, SRC, "-L",
                              _lib.CSRC, "-lbft", f"-Wl,-rpath,{_lib.CSRC}", f"-Wl,-rpath-link,{_lib.CSRC}", "-Wl,-rpath-link,/opt/rocm/lib"])
        exes[form] = exe
    # three genomes: an ancestor, a mutant, and two pieces of the ancestor (an inner deletion) followed by an unrelated stretch
    anc = S.random_genome(3000, 51)
    mut = S.mutate(anc, 0.02, 52)
    third = S.random_genome(1500, 53)
    third[:500] = anc[1000:1500]
    third[500:900] = anc[1600:2000]
    files, lists = [], []
    for gid, g in enumerate((anc, mut, third)):
        asc = S.packed_to_ascii(S.distinct(S.kmers_of(g, K)), K)
        path = str(d / f"genome{gid}.txt")
        with open(path, "w") as f:
            f.write("\n".join(asc) + "\n")
        files.append(path)
        lists.append((asc, gid))
    owners = _owners_of(lists)
    t = BFT(K, device=0)  # (the rows that order the truth: the product's extract, nothing else)
    for asc, gid in lists:
        t.insert_kmers(S.ascii_to_packed(asc, K)[0], gid)
    row_of = _row_of(t)
    t.close()
    return exes, files, owners, row_of


def _run(program, form, mode):
    exes, files, _, _ = program
    return subprocess.run([exes[form], str(K), mode] + files, capture_output=True, text=True, timeout=300)


def test_flags_set_and_read_back_per_kmer(program):
    _, _, owners, row_of = program
    r = _run(program, "pie", "flags")
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    order = sorted(row_of, key=row_of.get)
    assert len(lines) == len(order) + 1
    for i, (line, x) in enumerate(zip(lines, order)):
        assert line == f"{x} {1 + (i // 3) % 3 if i % 3 == 0 else 0}", i
    assert lines[-1] == "again 0"


@pytest.mark.parametrize("form", ["pie", "nopie"])
def test_traversals_through_iterate_over_kmers(program, form):
    _, _, owners, row_of = program
    order = sorted(row_of, key=row_of.get)
    n_all = len(_truth(owners, (), row_of)[1])
    model = MarkModel(owners)
    n_sub = sum(model.bfs_subgraph(x, (0, 1)) for x in order)
    assert n_sub == len(_truth(owners, (0, 1), row_of)[1]) and n_sub >= 2
    # (called on every k-mer, BFS_subgraph leaves none unvisited: a k-mer outside the sub-graph is marked and starts no component)
    assert set(model.flag.values()) == {1}
    r = _run(program, form, "traverse")
    assert r.returncode == 0, r.stderr
    assert r.stdout.splitlines() == [f"BFS {n_all}", "direct 0", f"count {n_all}", f"DFS {n_all}", f"BFS_subgraph {n_sub}",
                                     "flags " + "".join(str(model.flag[x]) for x in order)]


def test_cdbg_traversal_leaves_the_graph_unmarked(program):
    _, _, owners, row_of = program
    r = _run(program, "pie", "cdbg")
    assert r.returncode == 0, r.stderr
    assert r.stdout.splitlines() == ["marked 0", f"cdbg {len(_truth(owners, (), row_of)[1])}", "marked 0"]


@pytest.mark.parametrize("mode, message", [("flag4", "set_flag_kmer(): a flag can only have as value 0, 1, 2 or 3.\n"),
                                           ("unmarked", "set_flag_kmer(): the graph is not initialized for marking.\n"),
                                           ("absent", "set_flag_kmer(): k-mer is not present in the graph.\n")], ids=["flag4", "unmarked", "absent"])
def test_error_paths_take_the_reference_messages(program, mode, message):
    r = _run(program, "pie", mode)
    assert r.returncode == 1
    assert r.stderr == message
