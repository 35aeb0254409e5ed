"""The CLI's -bubbles min_shared max_branch_chars output_file (csrc/bft_gpu_cli.c): the bubble file of the planted-variant genomes, built with
`sequences_canonical`, is byte for byte the text of the model of tests/test_bubbles_host.py -- bubbles, allele strings, genome ids --, with and
without a limit on the branches; its segment ids are those of -gfa at the same min_shared; an index that is not canonical and bad arguments are
refused."""
import os
import subprocess
import sys

import pytest

from bloomfiltertrie_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_bubbles_host as B  # noqa: E402
import test_cgraph_host as G  # noqa: E402

pytestmark = pytest.mark.gpu
CLI = os.path.join(_lib.CSRC, "bft_gpu")
K = 27


def setup_files(d):
    """the planted-variant genomes as FASTA files in directory d, and their list; returns the paths"""
    genomes, _, _ = B.planted_case(K)
    files = []
    with open(os.path.join(d, "list.txt"), "w") as lst:
        for gid, seqs in enumerate(genomes):
            path = os.path.join(d, f"genome{gid}.fa")
            with open(path, "w") as f:
                f.write("".join(f">s{i}\n{s}\n" for i, s in enumerate(seqs)))
            lst.write(path + "\n")
            files.append(path)
    return files


def want_text(limit=0):
    g = B.planted_graph(K)
    return B.expected_text(g, B.Bubbles(K, *g.arrays()[:4], max_branch_chars=limit).reported()[0])


def test_bubble_files_equal_the_model_and_join_to_the_gfa(tmp_path):
    d = str(tmp_path)
    setup_files(d)
    subprocess.run([CLI, "build", str(K), "sequences_canonical", "list.txt", "c.bft"], cwd=d, check=True, capture_output=True, timeout=300)
    out = subprocess.run([CLI, "load", "c.bft", "-bubbles", "0", "0", "b0.txt", "-gfa", "0", "0", "g0.gfa", "-bubbles", "0", str(2 * K - 1), "b1.txt"], cwd=d,
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    text = open(os.path.join(d, "b0.txt")).read()
    assert text == want_text() and text.count("B\t") == 4
    assert open(os.path.join(d, "b1.txt")).read() == want_text(2 * K - 1) != text  # (the option that follows a -gfa is read where it starts)
    gfa = open(os.path.join(d, "g0.gfa")).read()
    assert G.check_gfa(B.planted_graph(K), gfa, False) == [] and B.joins_to_gfa(text, gfa)


def test_noncanonical_index_and_bad_arguments_are_refused(tmp_path):
    d = str(tmp_path)
    setup_files(d)
    subprocess.run([CLI, "build", str(K), "sequences", "list.txt", "n.bft"], cwd=d, check=True, capture_output=True, timeout=300)
    out = subprocess.run([CLI, "load", "n.bft", "-bubbles", "0", "0", "b.txt"], cwd=d, capture_output=True, text=True, timeout=300)
    assert out.returncode != 0 and "not canonical" in out.stderr and not os.path.exists(os.path.join(d, "b.txt"))
    out = subprocess.run([CLI, "load", "n.bft", "-bubbles", "two", "0", "b.txt"], cwd=d, capture_output=True, text=True, timeout=300)
    assert out.returncode != 0 and "min_shared" in out.stderr
    out = subprocess.run([CLI, "load", "n.bft", "-bubbles", "0", "-3", "b.txt"], cwd=d, capture_output=True, text=True, timeout=300)
    assert out.returncode != 0 and "max_branch_chars" in out.stderr
    out = subprocess.run([CLI, "load", "n.bft", "-bubbles", "0", "0"], cwd=d, capture_output=True, text=True, timeout=300)
    assert out.returncode != 0 and "-bubbles min_shared max_branch_chars output_file" in out.stderr and not os.path.exists(os.path.join(d, "b.txt"))
