"""extract_simple_paths_to_disk and extract_simple_core_paths_to_disk of the reference's snippets (<bft/snippets.h>, -lbft; src/snippets.c:306-603):
tests/c/ref_simple_paths_program.c, compiled with -Werror against the headers, writes the paths of an index of three related genomes; the file
and the stdout line are checked against ground truth computed in Python from the inserted k-mers, and a file that cannot be created exits
through the reference's error."""
import os
import subprocess

import pytest

from bloomfiltertrie_amd import BFT, _lib, synth as S

from test_gpu_simple_paths import _owners_of, _row_of, _truth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "ref_simple_paths_program.c")
K = 27


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    subprocess.check_call(["make", "-C", _lib.CSRC, "all"], stdout=subprocess.DEVNULL)
    d = tmp_path_factory.mktemp("simple_paths")
    exe = str(d / "ref_simple_paths_program")
    subprocess.check_call(["gcc", "-O2", "-std=gnu99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, SRC, "-L", _lib.CSRC, "-lbft",
                           f"-Wl,-rpath,{_lib.CSRC}", f"-Wl,-rpath-link,{_lib.CSRC}", "-Wl,-rpath-link,/opt/rocm/lib"])
    anc = S.random_genome(6000, 41)
    anc[4000:4200] = anc[1000:1200]  # (a repeat: branching k-mers at its ends)
    genomes = [anc, S.mutate(anc, 0.02, 42), S.mutate(anc, 0.02, 43)]
    files, lists = [], []
    for gid, g in enumerate(genomes):
        km = S.distinct(S.kmers_of(g, K))
        asc = S.packed_to_ascii(km, K)
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
    return exe, files, owners, row_of, d


def _run(program, mode, ratio, out):
    exe, files, _, _, _ = program
    return subprocess.run([exe, str(K), mode, str(ratio), out] + files, capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize("mode,ratio,thr", [("plain", 0, 0), ("core", 0.7, 2), ("core", 1.0, 3), ("core", 0.2, 0)])
def test_paths_file_and_longest_line(program, mode, ratio, thr):
    _, _, owners, row_of, d = program
    out = str(d / f"{mode}_{ratio}.txt")
    r = _run(program, mode, ratio, out)
    assert r.returncode == 0, r.stderr
    want = _truth(owners, K, thr, row_of)
    assert open(out).read() == "".join(p + "\n" for p in want)
    longest = max(map(len, want), default=0)
    what = "simple path" if mode == "plain" else "simple core path"
    assert r.stdout == f"Longest {what} has {longest} nuc.\n"


@pytest.mark.parametrize("mode", ["plain", "core"])
def test_unwritable_file_exits_through_error(program, mode):
    _, _, _, _, d = program
    r = _run(program, mode, 0.5, str(d / "no_such_dir" / "out.txt"))
    assert r.returncode == 1
    msg = ("extract_simple_paths_to_disk(): failed to create output file.\n" if mode == "plain"
           else "extract_simple_core_paths_to_disk(): failed to create/open output file.\n")
    assert r.stderr == msg
