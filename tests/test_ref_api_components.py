"""get_nb_connected_component with BFS, DFS, BFS_subgraph and DFS_subgraph, and is_in_subgraph, of the reference's snippets (<bft/snippets.h>, -lbft;
src/snippets.c:605-960): tests/c/ref_components_program.c, compiled with -Werror against the headers as a position-independent and as a fixed-address
executable (the traversals are told apart by their addresses across the library boundary), counts the components of an index of three genomes;
the counts are checked against ground truth computed in Python from the inserted k-mers, the accumulation into *nb, the ids that add nothing,
is_in_subgraph per k-mer, and the error for any other function."""
import os
import subprocess

import pytest

from bloomfiltertrie_amd import BFT, _lib, synth as S

from test_gpu_components import _owners_of, _row_of, _truth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "ref_components_program.c")
K = 27


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    subprocess.check_call(["make", "-C", _lib.CSRC, "all"], stdout=subprocess.DEVNULL)
    d = tmp_path_factory.mktemp("components")
    exes = {}
    for form, flags in (("pie", []), ("nopie", ["-no-pie"])):
        exe = str(d / f"ref_components_program_{form}")
        subprocess.check_call(["gcc", "-O2", "-std=gnu99", "-Wall", "-Werror"] + flags + ["-I", os.path.join(ROOT, "include"), "-o", exe, SRC, "-L",
                              _lib.CSRC, "-lbft", f"-Wl,-rpath,{_lib.CSRC}", f"-Wl,-rpath-link,{_lib.CSRC}", "-Wl,-rpath-link,/opt/rocm/lib"])
        exes[form] = exe
    # three genomes: an ancestor, a mutant, and two pieces of the ancestor (an inner deletion) followed by an unrelated stretch
    anc = S.random_genome(6000, 51)
    mut = S.mutate(anc, 0.02, 52)
    third = S.random_genome(3000, 53)
    third[:1000] = anc[2000:3000]
    third[1000:1800] = anc[3200:4000]
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


@pytest.mark.parametrize("form", ["pie", "nopie"])
def test_counts_match_ground_truth(program, form):
    _, _, owners, row_of = program
    n = {ids: len(_truth(owners, ids, row_of)[1]) for ids in ((), (0,), (0, 1), (1, 2))}
    assert n[(0, 1)] >= 2  # (SNPs of the mutant split the k-mers it shares with the ancestor)
    r = _run(program, form, "count")
    assert r.returncode == 0, r.stderr
    want = [f"BFS {n[()]}", f"DFS {n[()]}", f"BFS_subgraph {n[(0,)]}", f"DFS_subgraph {n[(0, 1)]}", f"BFS_subgraph {n[(1, 2)]}",
            f"acc {1000 + 2 * n[()] + n[(0,)]}", "zero 5"]
    assert r.stdout.splitlines() == want


def test_is_in_subgraph(program):
    _, _, owners, _ = program
    r = _run(program, "pie", "member")
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == len(owners)
    for line in lines[::7]:
        kmer, bits = line.split()
        o = owners[kmer]
        want = [0 in o, {0, 1} <= o, {1, 2} <= o, False, False]
        assert [c == "1" for c in bits] == want, (kmer, bits, o)


@pytest.mark.parametrize("form", ["pie", "nopie"])
def test_other_function_is_an_error(program, form):
    r = _run(program, form, "bad")
    assert r.returncode == 1
    assert "get_nb_connected_component()" in r.stderr


def test_traversals_called_directly_are_an_error(program):
    r = _run(program, "pie", "direct")
    assert r.returncode == 1
    assert r.stderr.startswith("BFS()") and "get_nb_connected_component()" in r.stderr
