"""extract_unitigs_to_disk (<bft/unitigs.h>, -lbft): tests/c/ref_unitigs_program.c, compiled with -Werror against the headers, ingests FASTA files
canonically and writes the unitigs; the file and the stdout line are checked against the model of tests/test_unitigs_host.py; an index that is not
canonical and a file that cannot be created exit through the library's errors."""
import os
import subprocess
import sys

import pytest

from bloomfiltertrie_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_unitigs_host as H  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "ref_unitigs_program.c")
K = 27


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    subprocess.check_call(["make", "-C", _lib.CSRC, "all"], stdout=subprocess.DEVNULL)
    d = tmp_path_factory.mktemp("unitigs")
    exe = str(d / "ref_unitigs_program")
    subprocess.check_call(["gcc", "-O2", "-std=gnu99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, SRC, "-L", _lib.CSRC, "-lbft",
                           f"-Wl,-rpath,{_lib.CSRC}", f"-Wl,-rpath-link,{_lib.CSRC}", "-Wl,-rpath-link,/opt/rocm/lib"])
    genomes, model = H.width_case(K)
    files = []
    for gid, seqs in enumerate(genomes):
        path = str(d / f"genome{gid}.fa")
        with open(path, "w") as f:
            f.write("".join(f">s{i}\n{s}\n" for i, s in enumerate(seqs)))
        files.append(path)
    return exe, files, model, d


def _run(program, word, t, out):
    exe, files, _, _ = program
    return subprocess.run([exe, str(K), word, str(t), out] + files, capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize("t", [0, 2, H.N_GENOMES, -1])
def test_unitigs_file_and_longest_line(program, t):
    _, _, model, d = program
    out = str(d / f"unitigs_{t}.txt")
    r = _run(program, "sequences_canonical", t, out)
    assert r.returncode == 0, r.stderr
    want = model.unitigs(max(t, 0))
    assert H.check(model, max(t, 0), open(out).read().split("\n")[:-1]) == []
    assert open(out).read() == "".join(p + "\n" for p in want)
    assert r.stdout.endswith(f"Longest unitig has {max(map(len, want), default=0)} nuc.\n")


def test_noncanonical_index_and_unwritable_file_exit_through_errors(program):
    _, _, _, d = program
    r = _run(program, "sequences", 0, str(d / "nc.txt"))
    assert r.returncode == 1 and "not canonical" in r.stderr
    r = _run(program, "sequences_canonical", 0, str(d / "no_such_dir" / "out.txt"))
    assert r.returncode == 1 and r.stderr == "extract_unitigs_to_disk(): failed to create output file.\n"
