"""thread_sequences_to_disk (<bft/unitigs.h>, -lbft): tests/c/ref_threading_program.c, compiled with -Werror against the headers, ingests the FASTA files
of the planted-variant genomes canonically and threads a sequence file through their compacted graph; the GAF file is byte for byte the text of the
model of tests/test_threading_host.py and the file the command line's -thread writes, from a FASTA and from a FASTQ input; its segment ids are those of
extract_unitig_graph_to_disk at the same min_shared; a missing input file, an index that is not canonical and a file that cannot be created exit
through the library's errors."""
import os
import subprocess
import sys

import pytest

from bloomfiltertrie_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_bubbles_host as B  # noqa: E402
import test_cgraph_host as G  # noqa: E402
import test_gpu_cli_bubbles as CB  # noqa: E402  (the set-up: FASTA files of the planted-variant genomes and their list)
import test_gpu_cli_threading as CT  # noqa: E402  (the sequence files and the expected text)
import test_threading_host as T  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "ref_threading_program.c")
K = CB.K


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    subprocess.check_call(["make", "-C", _lib.CSRC, "all"], stdout=subprocess.DEVNULL)
    d = tmp_path_factory.mktemp("threading")
    exe = str(d / "ref_threading_program")
    subprocess.check_call(["gcc", "-O2", "-std=gnu99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, SRC, "-L", _lib.CSRC, "-lbft",
                           f"-Wl,-rpath,{_lib.CSRC}", f"-Wl,-rpath-link,{_lib.CSRC}", "-Wl,-rpath-link,/opt/rocm/lib"])
    names, seqs = CT.sequence_files(str(d))
    return exe, CB.setup_files(str(d)), d, names, seqs


def _run(program, word, t, reads, out, gfa="-"):
    exe, files, d = program[:3]
    return subprocess.run([exe, str(K), word, str(t), reads, out, gfa] + files, capture_output=True, text=True, timeout=300, cwd=str(d))


@pytest.mark.parametrize("reads,t", (("reads.fa", 0), ("reads.fq", 0), ("reads.fa", 2), ("reads.fa", -1)))
def test_gaf_file_is_the_model_and_joins_to_the_gfa(program, reads, t):
    _, _, d, names, seqs = program
    out, gfa = str(d / f"walks_{reads}_{t}.gaf"), str(d / f"graph_{reads}_{t}.gfa")
    r = _run(program, "sequences_canonical", t, reads, out, gfa)
    assert r.returncode == 0, r.stderr
    text = open(out).read()
    thr = max(t, 0)
    assert text == CT.want_text(names, seqs, thr) != ""
    g = B.planted_graph(K) if thr == 0 else G.Graph(B.planted_case(K)[1], thr)
    gfa_text = open(gfa).read()
    assert G.check_gfa(g, gfa_text, False) == [] and T.joins_to_gfa(text, gfa_text, dict(zip(names, seqs)))


def test_the_command_line_writes_the_same_file(program):
    d = program[2]
    out = str(d / "lib.gaf")
    assert _run(program, "sequences_canonical", 0, "reads.fa", out).returncode == 0
    subprocess.run([CB.CLI, "build", str(K), "sequences_canonical", "list.txt", "c.bft"], cwd=str(d), check=True, capture_output=True, timeout=300)
    r = subprocess.run([CB.CLI, "load", "c.bft", "-thread", "0", "reads.fa", "cli.gaf"], cwd=str(d), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert open(out).read() == open(str(d / "cli.gaf")).read() != ""


def test_missing_input_noncanonical_index_and_unwritable_file_exit_through_errors(program):
    d = program[2]
    r = _run(program, "sequences", 0, "reads.fa", str(d / "nc.gaf"))
    assert r.returncode == 1 and "not canonical" in r.stderr
    r = _run(program, "sequences_canonical", 0, "no_such_file.fa", str(d / "missing.gaf"))
    assert r.returncode == 1 and r.stderr == "thread_sequences_to_disk(): failed to read the sequence file.\n" and not os.path.exists(str(d / "missing.gaf"))
    r = _run(program, "sequences_canonical", 0, "reads.fa", str(d / "no_such_dir" / "out.gaf"))
    assert r.returncode == 1 and r.stderr == "thread_sequences_to_disk(): failed to create output file.\n"
