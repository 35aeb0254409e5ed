"""extract_bubbles_to_disk (<bft/unitigs.h>, -lbft): tests/c/ref_bubbles_program.c, compiled with -Werror against the headers, ingests the FASTA files
of the planted-variant genomes canonically and writes their bubbles; the file is byte for byte the text of the model of tests/test_bubbles_host.py
(bubbles, allele strings, genome ids) and the file the command line's -bubbles writes; its segment ids are those of extract_unitig_graph_to_disk at the
same min_shared; an index that is not canonical and a file that cannot be created exit through the library's errors."""
import os
import subprocess
import sys

import pytest

from bloomfiltertrie_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_bubbles_host as B  # noqa: E402
import test_cgraph_host as G  # noqa: E402
import test_gpu_cli_bubbles as CB  # noqa: E402  (the set-up: FASTA files of the planted-variant genomes and their list)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "ref_bubbles_program.c")
K = CB.K


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    subprocess.check_call(["make", "-C", _lib.CSRC, "all"], stdout=subprocess.DEVNULL)
    d = tmp_path_factory.mktemp("bubbles")
    exe = str(d / "ref_bubbles_program")
    subprocess.check_call(["gcc", "-O2", "-std=gnu99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, SRC, "-L", _lib.CSRC, "-lbft",
                           f"-Wl,-rpath,{_lib.CSRC}", f"-Wl,-rpath-link,{_lib.CSRC}", "-Wl,-rpath-link,/opt/rocm/lib"])
    return exe, CB.setup_files(str(d)), d


def _run(program, word, t, limit, out, gfa="-"):
    exe, files, _ = program
    return subprocess.run([exe, str(K), word, str(t), str(limit), out, gfa] + files, capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize("limit", (0, -1, 2 * K - 1))
def test_bubble_file_is_the_model_and_joins_to_the_gfa(program, limit):
    _, _, d = program
    out, gfa = str(d / f"bubbles_{limit}.txt"), str(d / f"graph_{limit}.gfa")
    r = _run(program, "sequences_canonical", 0, limit, out, gfa)
    assert r.returncode == 0, r.stderr
    text = open(out).read()
    assert text == CB.want_text(max(limit, 0)) and text.count("B\t") == (3 if limit > 0 else 4)
    gfa_text = open(gfa).read()
    assert G.check_gfa(B.planted_graph(K), gfa_text, False) == [] and B.joins_to_gfa(text, gfa_text)


def test_the_command_line_writes_the_same_file(program):
    _, _, d = program
    out = str(d / "lib.txt")
    assert _run(program, "sequences_canonical", 0, 0, out).returncode == 0
    subprocess.run([CB.CLI, "build", str(K), "sequences_canonical", "list.txt", "c.bft"], cwd=str(d), check=True, capture_output=True, timeout=300)
    r = subprocess.run([CB.CLI, "load", "c.bft", "-bubbles", "0", "0", "cli.txt"], cwd=str(d), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert open(out).read() == open(str(d / "cli.txt")).read() != ""


def test_noncanonical_index_and_unwritable_file_exit_through_errors(program):
    _, _, d = program
    r = _run(program, "sequences", 0, 0, str(d / "nc.txt"))
    assert r.returncode == 1 and "not canonical" in r.stderr
    r = _run(program, "sequences_canonical", 0, 0, str(d / "no_such_dir" / "out.txt"))
    assert r.returncode == 1 and r.stderr == "extract_bubbles_to_disk(): failed to create output file.\n"
