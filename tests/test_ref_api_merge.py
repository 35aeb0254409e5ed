"""merging_BFT of the reference's API (<bft/merge.h>, -lbft; include/merge.h:14): tests/c/ref_merge_program.c, written against the reference's
names only and compiled with -Werror, writes two .bft files, merges them and loads the result, once with disjoint genome names (the second graph's
genomes are appended) and once with the first graph's last name equal to the second's first (are_genomes_ids_overlapping, include/Node.h:147-155:
they start one earlier and the shared genome's two halves unite).  Per k-mer of a fixed list it prints the genome ids, and the genome names; the
Python side holds that against the truth over the k-mers the files hold.  The declaration, the export and the link need no GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

from bloomfiltertrie_amd import _lib, synth as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "ref_merge_program.c")
K = 27


def _compile(d):
    subprocess.check_call(["make", "-C", _lib.CSRC, "all"], stdout=subprocess.DEVNULL)
    exe = str(d / "ref_merge_program")
    subprocess.check_call(["gcc", "-O2", "-std=gnu99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, SRC, "-L", _lib.CSRC, "-lbft",
                           f"-Wl,-rpath,{_lib.CSRC}", f"-Wl,-rpath-link,{_lib.CSRC}", "-Wl,-rpath-link,/opt/rocm/lib"])
    return exe


def test_merge_header_declares_it_and_a_program_links(tmp_path):
    """no GPU: the reference's signature in <bft/merge.h>, the export of libbft.so, and a program written against the header compiles and links"""
    hdr = open(os.path.join(ROOT, "include", "bft", "merge.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bvoid\s+merging_BFT\s*\(\s*char\s*\*\s*prefix_bft1\s*,\s*char\s*\*\s*prefix_bft2\s*,\s*char\s*\*\s*output_prefix\s*,\s*int\s+cut_lvl\s*,"
                     r"\s*bool\s+packed_in_subtries\s*\)\s*;", code)
    assert "cut_lvl" in hdr and "ignored" in hdr  # (the header says what becomes of the two arguments of the split on-disk form)
    exe = _compile(tmp_path)
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(_lib.CSRC, "libbft.so")]).decode()
    assert re.search(r" T merging_BFT$", out, flags=re.M)
    und = subprocess.check_output(["nm", "-D", "--undefined-only", exe]).decode()
    assert re.search(r" U merging_BFT$", und, flags=re.M)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stderr


def _write(path, asc):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(asc) + "\n")
    return path


@pytest.mark.gpu
@pytest.mark.parametrize("overlap", [False, True])
def test_merging_bft_against_ground_truth(tmp_path, overlap):
    exe = _compile(tmp_path)
    anc = S.random_genome(2500, 61)
    per = [S.packed_to_ascii(S.distinct(S.kmers_of(g, K)), K) for g in [anc] + [S.mutate(anc, 0.02, 62 + i) for i in range(4)]]
    # graph 1: genomes 0, 1, 2; graph 2: three more -- or, overlapping, the other half of genome 2 under the same file name, then two more
    half = len(per[2]) // 2
    d1, d2 = str(tmp_path / "one"), str(tmp_path / "two")
    files1 = [_write(os.path.join(d1, "g0.txt"), per[0]), _write(os.path.join(d1, "g1.txt"), per[1]),
              _write(os.path.join(d1, "g2.txt"), per[2][:half] if overlap else per[2])]
    if overlap:
        files2 = [_write(os.path.join(d2, "g2.txt"), per[2][half - 30:]), _write(os.path.join(d2, "g3.txt"), per[3]), _write(os.path.join(d2, "g4.txt"), per[4])]
        lists = [(per[0], 0), (per[1], 1), (per[2], 2), (per[3], 3), (per[4], 4)]
        names = ["g0.txt", "g1.txt", "g2.txt", "g3.txt", "g4.txt"]
    else:
        files2 = [_write(os.path.join(d2, "h0.txt"), per[3]), _write(os.path.join(d2, "h1.txt"), per[4]), _write(os.path.join(d2, "h2.txt"), per[0][::2])]
        lists = [(per[0], 0), (per[1], 1), (per[2], 2), (per[3], 3), (per[4], 4), (per[0][::2], 5)]
        names = ["g0.txt", "g1.txt", "g2.txt", "h0.txt", "h1.txt", "h2.txt"]
    truth = {}
    for asc, g in lists:
        for s in asc:
            truth.setdefault(s, set()).add(g)
    stored = sorted(truth)
    rng = np.random.default_rng(5 + overlap)
    mutants = S.packed_to_ascii(S.snp_mutants(S.ascii_to_packed(stored[:200], K)[0], K, 9), K)
    absent = [s for s in mutants if s not in truth][:50]
    query = [stored[i] for i in rng.choice(len(stored), 400, replace=False)] + absent
    if overlap:
        query += per[2][half - 30:half + 30]  # around the seam of the shared genome's two halves
    qfile = _write(str(tmp_path / "query.txt"), query)
    r = subprocess.run([exe, str(K), qfile, str(tmp_path / "merged"), "3"] + files1 + files2, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert lines[0] == f"genomes {len(names)}"
    assert lines[1:1 + len(names)] == [f"name {i} {nm}" for i, nm in enumerate(names)]
    body = lines[1 + len(names):]
    assert len(body) == len(query) and len(absent) >= 20
    for q, line in zip(query, body):
        kmer, ids = line.split()
        assert kmer == q
        assert ids == (",".join(str(g) for g in sorted(truth[q])) if q in truth else "-"), q
    for suffix in (".1", ".2", ".m"):
        assert os.path.getsize(str(tmp_path / "merged") + suffix) > 0
