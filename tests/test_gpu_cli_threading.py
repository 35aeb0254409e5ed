"""The CLI's -thread min_shared sequence_file output_file (csrc/bft_gpu_cli.c): the GAF file of the planted-variant case's sequence set, threaded
through the index built with `sequences_canonical`, is byte for byte the text of the model of tests/test_threading_host.py; its segment ids are those of
-gfa at the same min_shared; FASTA and FASTQ inputs, record names up to the first blank, an empty name as the record's number; a missing input file,
an index that is not canonical and bad arguments are refused."""
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_bubbles_host as B  # noqa: E402
import test_cgraph_host as G  # noqa: E402
import test_gpu_cli_bubbles as CB  # noqa: E402  (the set-up: FASTA files of the planted-variant genomes and their list)
import test_threading_host as T  # noqa: E402

pytestmark = pytest.mark.gpu
CLI = CB.CLI
K = CB.K


def sequence_files(d):
    """the planted case's sequence set as a FASTA file (lines of 70 characters, headers with a comment, one empty name) and as a FASTQ file in directory
    d; returns (the names as the reader gives them, the sequences)"""
    seqs = T.planted_sequences(K)
    names = [str(i) if i == 2 else f"read{i}" for i in range(len(seqs))]
    with open(os.path.join(d, "reads.fa"), "w") as f:
        for i, q in enumerate(seqs):
            f.write(">" + ("" if i == 2 else f"read{i}") + f" number {i}\tof the set\n" + "".join(q[a:a + 70] + "\n" for a in range(0, len(q), 70)))
    with open(os.path.join(d, "reads.fq"), "w") as f:
        for i, q in enumerate(seqs):
            f.write("@" + ("" if i == 2 else f"read{i}") + f" number {i}\n{q}\n+\n{'I' * len(q)}\n")
    return names, seqs


def want_text(names, seqs, t=0):
    g = B.planted_graph(K) if t == 0 else G.Graph(B.planted_case(K)[1], t)
    return T.expected_gaf(g, names, seqs, T.threading_of(g).run(seqs))


def test_gaf_files_equal_the_model_and_join_to_the_gfa(tmp_path):
    d = str(tmp_path)
    CB.setup_files(d)
    names, seqs = sequence_files(d)
    subprocess.run([CLI, "build", str(K), "sequences_canonical", "list.txt", "c.bft"], cwd=d, check=True, capture_output=True, timeout=300)
    out = subprocess.run([CLI, "load", "c.bft", "-thread", "0", "reads.fa", "w0.gaf", "-gfa", "0", "0", "g0.gfa", "-thread", "0", "reads.fq", "w1.gaf", "-thread", "2",
                          "reads.fa", "w2.gaf"], cwd=d, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    text = open(os.path.join(d, "w0.gaf")).read()
    assert text == want_text(names, seqs) and text.startswith("read0\t")
    assert open(os.path.join(d, "w1.gaf")).read() == text  # (the option that follows a -gfa is read where it starts; FASTQ gives the same file)
    assert open(os.path.join(d, "w2.gaf")).read() == want_text(names, seqs, 2) != text
    gfa = open(os.path.join(d, "g0.gfa")).read()
    assert G.check_gfa(B.planted_graph(K), gfa, False) == [] and T.joins_to_gfa(text, gfa, dict(zip(names, seqs)))


def test_missing_input_noncanonical_index_and_bad_arguments_are_refused(tmp_path):
    d = str(tmp_path)
    CB.setup_files(d)
    sequence_files(d)
    subprocess.run([CLI, "build", str(K), "sequences", "list.txt", "n.bft"], cwd=d, check=True, capture_output=True, timeout=300)
    out = subprocess.run([CLI, "load", "n.bft", "-thread", "0", "reads.fa", "w.gaf"], cwd=d, capture_output=True, text=True, timeout=300)
    assert out.returncode != 0 and "not canonical" in out.stderr and not os.path.exists(os.path.join(d, "w.gaf"))
    out = subprocess.run([CLI, "load", "n.bft", "-thread", "0", "no_such_file.fa", "w.gaf"], cwd=d, capture_output=True, text=True, timeout=300)
    assert out.returncode != 0 and "cannot read no_such_file.fa" in out.stderr and not os.path.exists(os.path.join(d, "w.gaf"))
    with open(os.path.join(d, "plain.txt"), "w") as f:
        f.write("ACGT\n")
    out = subprocess.run([CLI, "load", "n.bft", "-thread", "0", "plain.txt", "w.gaf"], cwd=d, capture_output=True, text=True, timeout=300)
    assert out.returncode != 0 and "neither FASTA nor FASTQ" in out.stderr and not os.path.exists(os.path.join(d, "w.gaf"))
    out = subprocess.run([CLI, "load", "n.bft", "-thread", "two", "reads.fa", "w.gaf"], cwd=d, capture_output=True, text=True, timeout=300)
    assert out.returncode != 0 and "min_shared" in out.stderr
    out = subprocess.run([CLI, "load", "n.bft", "-thread", "0", "reads.fa"], cwd=d, capture_output=True, text=True, timeout=300)
    assert out.returncode != 0 and "-thread min_shared sequence_file output_file" in out.stderr and not os.path.exists(os.path.join(d, "w.gaf"))
