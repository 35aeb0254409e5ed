"""create_cdbg_from_bft_kmers and add_id_genomes of the reference's public API (<bft/bft.h>, -lbft; include/bft.h:179-180,
src/bft.c:1353-1684): tests/c/ref_subgraph_program.c, compiled with -Werror against the header, builds sub-graphs with and without colours
(checked against ground truth through get_annotation / get_list_id_genomes), widens a k-mer's colour set and exits on a genome id that was
never inserted."""
import os
import subprocess

import numpy as np
import pytest

from bloomfiltertrie_amd import _lib, synth as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "ref_subgraph_program.c")
K = 27


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    subprocess.check_call(["make", "-C", _lib.CSRC, "all"], stdout=subprocess.DEVNULL)
    d = tmp_path_factory.mktemp("subgraph")
    exe = str(d / "ref_subgraph_program")
    subprocess.check_call(["gcc", "-O2", "-std=gnu99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, SRC, "-L", _lib.CSRC, "-lbft",
                           f"-Wl,-rpath,{_lib.CSRC}", f"-Wl,-rpath-link,{_lib.CSRC}", "-Wl,-rpath-link,/opt/rocm/lib"])
    anc = S.random_genome(6000, 31)
    genomes = [anc, S.mutate(anc, 0.03, 32), S.mutate(anc, 0.03, 33)]
    files, truth = [], {}
    for gid, g in enumerate(genomes):
        asc = S.packed_to_ascii(S.distinct(S.kmers_of(g, K)), K)
        path = str(d / f"genome{gid}.txt")
        with open(path, "w") as f:
            f.write("\n".join(asc) + "\n")
        files.append(path)
        for s in asc:
            truth.setdefault(s, []).append(gid)
    rng = np.random.default_rng(3)
    stored = sorted(truth)
    pick = [stored[i] for i in rng.choice(len(stored), 800, replace=False)]
    absent = ["".join(rng.choice(list("ACGT"), K)) for _ in range(50)]
    absent = [a for a in absent if a not in truth]
    query = pick + pick[:100] + absent
    rng.shuffle(query)
    qpath = str(d / "query.txt")
    with open(qpath, "w") as f:
        f.write("\n".join(query) + "\n")
    return exe, files, truth, qpath, pick, absent


def _run(program, mode):
    exe, files, _, qpath, _, _ = program
    return subprocess.run([exe, str(K), mode, qpath] + files, capture_output=True, text=True, timeout=300)


def _lines(r):
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().split("\n")
    return lines[0].split(" "), dict(tuple(l.split(" ")) for l in lines[1:])


def test_subgraph_with_colours(program):
    _, files, truth, _, pick, _ = program
    head, got = _lines(_run(program, "colors"))
    assert head[:2] == ["genomes", "3"] and os.path.basename(files[0]) in head[2]
    assert got == {s: ",".join(map(str, truth[s])) for s in pick}


def test_subgraph_without_colours_takes_every_kmer(program):
    _, files, _, _, pick, absent = program
    head, got = _lines(_run(program, "plain"))
    assert head[:2] == ["genomes", "1"] and os.path.basename(files[0]) in head[2]
    assert got == {s: "0" for s in pick + absent}  # (as the reference: stored in the source or not)


def test_add_id_genomes_widens_the_set(program):
    exe, files, truth, qpath, _, _ = program
    first = next(l for l in open(qpath).read().split("\n") if l)
    r = _run(program, "add")
    assert r.returncode == 0, r.stderr
    want = ",".join(map(str, sorted(set(truth.get(first, [])) | {0, 2})))
    assert r.stdout.strip().split("\n") == [f"{first} {want}", f"{first} {want}"]


def test_add_id_genomes_rejects_an_unknown_genome(program):
    r = _run(program, "addbad")
    assert r.returncode == 1
    assert "add_id_genomes(): An attempt to update a k-mer with a genome id that has not been inserted in the BFT yet has been made." in r.stderr
