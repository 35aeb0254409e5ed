"""insert_genomes_from_sequence_files (<bft/ingest.h>, -lbft: an extension, the reference has no counterpart): tests/c/ref_ingest_program.c, written
against <bft/bft.h> and <bft/ingest.h> only and compiled with -Werror, ingests two small FASTA files and prints the genome ids of a fixed list of
k-mers; the same program built from k-mer files of the truth's k-mers (tests/test_ingest_cases_host.py) through the reference's own
insert_genomes_from_files must print the same, and both are held against the truth.  The declaration, the export and the link need no GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

from bloomfiltertrie_amd import _lib, synth as S
from test_ingest_cases_host import Truth, rand_text, revcomp, with_bad

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "ref_ingest_program.c")
K = 27


def _compile(d):
    subprocess.check_call(["make", "-C", _lib.CSRC, "all"], stdout=subprocess.DEVNULL)
    exe = str(d / "ref_ingest_program")
    subprocess.check_call(["gcc", "-O2", "-std=gnu99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, SRC, "-L", _lib.CSRC, "-lbft",
                           f"-Wl,-rpath,{_lib.CSRC}", f"-Wl,-rpath-link,{_lib.CSRC}", "-Wl,-rpath-link,/opt/rocm/lib"])
    return exe


def test_ingest_header_declares_it_and_a_program_links(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "bft", "ingest.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bvoid\s+insert_genomes_from_sequence_files\s*\(\s*int\s+nb_files\s*,\s*char\s*\*\*\s*paths\s*,\s*int\s+canonical\s*,\s*uint32_t\s+min_abundance\s*,"
                     r"\s*BFT_Root\s*\*\s*root\s*\)\s*;", code)
    assert "EXTENSION" in hdr and "no counterpart" in hdr  # (the header says that the reference does not have it)
    exe = _compile(tmp_path)
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(_lib.CSRC, "libbft.so")]).decode()
    assert re.search(r" T insert_genomes_from_sequence_files$", out, flags=re.M)
    und = subprocess.check_output(["nm", "-D", "--undefined-only", exe]).decode()
    assert re.search(r" U insert_genomes_from_sequence_files$", und, flags=re.M)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stderr


def _fasta(path, seqs):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "wb") as f:
        for i, s in enumerate(seqs):
            f.write(b">contig%d\n" % i + b"".join(s[j:j + 70] + b"\n" for j in range(0, len(s), 70)))
    return path


@pytest.mark.gpu
@pytest.mark.parametrize("mode,min_abundance", [("sequences", 0), ("sequences_canonical", 0), ("sequences_canonical", 2)])
def test_sequence_files_against_kmer_files_of_the_truth(tmp_path, mode, min_abundance):
    exe = _compile(tmp_path)
    rng = np.random.default_rng(17)
    a = rand_text(1500, rng)
    # (both genomes repeat a stretch they share, on either strand: -min_abundance 2 keeps k-mers of both)
    genomes = [[a, a[100:800], with_bad(rand_text(400, rng), [100, 101, 300]), b"acgtu" * 20],
               [a[200:900], revcomp(a[:700].decode()).encode(), rand_text(K - 1, rng), rand_text(600, rng)]]
    canonical = mode.endswith("canonical")
    truths = [Truth(g, K, canonical, min_abundance) for g in genomes]
    fa = [_fasta(str(tmp_path / "fa" / f"g{i}.fa"), g) for i, g in enumerate(genomes)]
    km = []
    for i, t in enumerate(truths):
        p = str(tmp_path / "km" / f"g{i}.fa")  # (the same base name: genomes are named by it)
        os.makedirs(os.path.dirname(p), exist_ok=True)
        with open(p, "w") as f:
            f.write("".join(x + "\n" for x in t.kmers))
        km.append(p)
    truth = {}
    for g, t in enumerate(truths):
        for x in t.kmers:
            truth.setdefault(x, set()).add(g)
    stored = sorted(truth)
    assert sum(len(v) == 2 for v in truth.values()) > 100 and any(len(v) == 1 for v in truth.values()) and len(stored) > 500
    mutants = S.packed_to_ascii(S.snp_mutants(S.ascii_to_packed(stored[:200], K)[0], K, 9), K)
    absent = [s for s in mutants if s not in truth][:50]
    query = [stored[i] for i in rng.choice(len(stored), 400, replace=False)] + absent
    qfile = str(tmp_path / "query.txt")
    with open(qfile, "w") as f:
        f.write("\n".join(query) + "\n")
    r1 = subprocess.run([exe, str(K), mode, str(min_abundance), qfile] + fa, capture_output=True, text=True, timeout=300)
    r2 = subprocess.run([exe, str(K), "kmers", "0", qfile] + km, capture_output=True, text=True, timeout=300)
    assert r1.returncode == 0, r1.stderr
    assert r2.returncode == 0, r2.stderr
    assert r1.stdout == r2.stdout
    lines = r1.stdout.splitlines()
    assert lines[:3] == ["genomes 2", "name 0 g0.fa", "name 1 g1.fa"]
    body = lines[3:]
    assert len(body) == len(query) and len(absent) >= 20
    for q, line in zip(query, body):
        kmer, ids = line.split()
        assert kmer == q and ids == (",".join(str(g) for g in sorted(truth[q])) if q in truth else "-"), q
