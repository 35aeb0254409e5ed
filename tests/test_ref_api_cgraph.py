"""extract_unitig_graph_to_disk (<bft/unitigs.h>, -lbft): tests/c/ref_cgraph_program.c, compiled with -Werror against the headers, ingests FASTA
files canonically and writes the compacted coloured graph as GFA 1; the file is parsed back and compared with the model of tests/test_cgraph_host.py,
with and without colours (the hexadecimal rows against the same sets); an index that is not canonical and a file that cannot be created exit through
the library's errors."""
import os
import subprocess
import sys

import pytest

from bloomfiltertrie_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_cgraph_host as G  # noqa: E402
import test_unitigs_host as H  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "ref_cgraph_program.c")
K = 27


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    subprocess.check_call(["make", "-C", _lib.CSRC, "all"], stdout=subprocess.DEVNULL)
    d = tmp_path_factory.mktemp("cgraph")
    exe = str(d / "ref_cgraph_program")
    subprocess.check_call(["gcc", "-O2", "-std=gnu99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, SRC, "-L", _lib.CSRC, "-lbft",
                           f"-Wl,-rpath,{_lib.CSRC}", f"-Wl,-rpath-link,{_lib.CSRC}", "-Wl,-rpath-link,/opt/rocm/lib"])
    genomes, _ = H.width_case(K)
    files = []
    for gid, seqs in enumerate(genomes):
        path = str(d / f"genome{gid}.fa")
        with open(path, "w") as f:
            f.write("".join(f">s{i}\n{s}\n" for i, s in enumerate(seqs)))
        files.append(path)
    return exe, files, d


def _run(program, word, t, colors, out):
    exe, files, _ = program
    return subprocess.run([exe, str(K), word, str(t), str(colors), out] + files, capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize("t,colors", [(0, 0), (0, 1), (2, 1), (H.N_GENOMES + 1, 1), (-1, 0)])
def test_gfa_file_is_the_model(program, t, colors):
    _, _, d = program
    out = str(d / f"graph_{t}_{colors}.gfa")
    r = _run(program, "sequences_canonical", t, colors, out)
    assert r.returncode == 0, r.stderr
    assert G.check_gfa(G.graph("width_case", K, max(t, 0)), open(out).read(), bool(colors)) == []


def test_noncanonical_index_and_unwritable_file_exit_through_errors(program):
    _, _, d = program
    r = _run(program, "sequences", 0, 1, str(d / "nc.gfa"))
    assert r.returncode == 1 and "not canonical" in r.stderr
    r = _run(program, "sequences_canonical", 0, 0, str(d / "no_such_dir" / "out.gfa"))
    assert r.returncode == 1 and r.stderr == "extract_unitig_graph_to_disk(): failed to create output file.\n"
