"""The CLI's -gfa min_shared colors output_file (csrc/bft_gpu_cli.c): the GFA 1 file of an index built with `sequences_canonical`, parsed back and
compared with the model of tests/test_cgraph_host.py, with and without colours; an index that is not canonical and bad arguments are refused."""
import os
import subprocess
import sys

import pytest

from bloomfiltertrie_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_cgraph_host as G  # noqa: E402
import test_gpu_cli_unitigs as CU  # noqa: E402  (the set-up: FASTA files of the key-width case and their list)

pytestmark = pytest.mark.gpu
CLI = CU.CLI
K = CU.K


def test_gfa_files_equal_the_model(tmp_path):
    d, _ = CU._setup(tmp_path)
    subprocess.run([CLI, "build", str(K), "sequences_canonical", "list.txt", "c.bft"], cwd=d, check=True, capture_output=True, timeout=300)
    out = subprocess.run([CLI, "load", "c.bft", "-gfa", "0", "0", "g0.gfa", "-gfa", "2", "1", "g2.gfa", "-unitigs", "0", "u0.fa", "-gfa", "0", "1", "g0c.gfa"], cwd=d,
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    for thr, colors, name in ((0, False, "g0.gfa"), (2, True, "g2.gfa"), (0, True, "g0c.gfa")):
        assert G.check_gfa(G.graph("width_case", K, thr), open(os.path.join(d, name)).read(), colors) == []
    assert os.path.exists(os.path.join(d, "u0.fa"))  # (the option that follows a -gfa is read where it starts)


def test_noncanonical_index_and_bad_arguments_are_refused(tmp_path):
    d, _ = CU._setup(tmp_path)
    subprocess.run([CLI, "build", str(K), "sequences", "list.txt", "n.bft"], cwd=d, check=True, capture_output=True, timeout=300)
    out = subprocess.run([CLI, "load", "n.bft", "-gfa", "0", "1", "g.gfa"], cwd=d, capture_output=True, text=True, timeout=300)
    assert out.returncode != 0 and "not canonical" in out.stderr and not os.path.exists(os.path.join(d, "g.gfa"))
    out = subprocess.run([CLI, "load", "n.bft", "-gfa", "two", "1", "g.gfa"], cwd=d, capture_output=True, text=True, timeout=300)
    assert out.returncode != 0 and "min_shared" in out.stderr
    out = subprocess.run([CLI, "load", "n.bft", "-gfa", "0", "yes", "g.gfa"], cwd=d, capture_output=True, text=True, timeout=300)
    assert out.returncode != 0 and "colors" in out.stderr
