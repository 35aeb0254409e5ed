"""The CLI's -unitigs min_shared output_file (csrc/bft_gpu_cli.c): the FASTA records `>unitig_<i> length=<L>` of an index built with
`sequences_canonical` equal BFT.unitigs of the loaded file and the model of tests/test_unitigs_host.py; an index that is not canonical is refused."""
import os
import subprocess
import sys

import pytest

from bloomfiltertrie_amd import BFT, _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_unitigs_host as H  # noqa: E402

pytestmark = pytest.mark.gpu
CLI = os.path.join(_lib.CSRC, "bft_gpu")
K = 27


def _setup(tmp_path):
    genomes, model = H.width_case(K)
    d = str(tmp_path)
    with open(os.path.join(d, "list.txt"), "w") as lst:
        for gid, seqs in enumerate(genomes):
            path = os.path.join(d, f"genome{gid}.fa")
            with open(path, "w") as f:
                f.write("".join(f">s{i}\n{s}\n" for i, s in enumerate(seqs)))
            lst.write(path + "\n")
    return d, model


def _records(path):
    lines = open(path).read().split("\n")
    assert lines[-1] == ""
    heads, seqs = lines[:-1:2], lines[1:-1:2]
    assert heads == [f">unitig_{i} length={len(s)}" for i, s in enumerate(seqs)]
    return seqs


def test_unitigs_records_equal_the_library_and_the_model(tmp_path):
    d, model = _setup(tmp_path)
    subprocess.run([CLI, "build", str(K), "sequences_canonical", "list.txt", "c.bft"], cwd=d, check=True, capture_output=True, timeout=300)
    out = subprocess.run([CLI, "load", "c.bft", "-unitigs", "0", "u0.fa", "-unitigs", "2", "u2.fa"], cwd=d, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    t = BFT.load_bft(os.path.join(d, "c.bft"))
    for thr, name in ((0, "u0.fa"), (2, "u2.fa")):
        got = _records(os.path.join(d, name))
        assert got == H.split(*t.unitigs(thr))
        assert H.check(model, thr, got) == []
    t.close()


def test_noncanonical_index_and_bad_threshold_are_refused(tmp_path):
    d, _ = _setup(tmp_path)
    subprocess.run([CLI, "build", str(K), "sequences", "list.txt", "n.bft"], cwd=d, check=True, capture_output=True, timeout=300)
    out = subprocess.run([CLI, "load", "n.bft", "-unitigs", "0", "u.fa"], cwd=d, capture_output=True, text=True, timeout=300)
    assert out.returncode != 0 and "not canonical" in out.stderr and not os.path.exists(os.path.join(d, "u.fa"))
    out = subprocess.run([CLI, "load", "n.bft", "-unitigs", "two", "u.fa"], cwd=d, capture_output=True, text=True, timeout=300)
    assert out.returncode != 0 and "min_shared" in out.stderr
