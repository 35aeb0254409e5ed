"""`bft_gpu load index.bft -genome_matrix {shared|jaccard|mash} out.tsv` (csrc/bft_gpu_cli.c) on a 5-genome index: the three tables parsed back and
compared with the truth computed from the inserted k-mers' genome sets -- the counts exactly, the distances to the six printed decimals; an unknown
word and a file that cannot be created exit non-zero with a message."""
import math
import os
import subprocess

import numpy as np
import pytest

from bloomfiltertrie_amd import BFT, _lib, synth as S

pytestmark = pytest.mark.gpu
CLI = os.path.join(_lib.CSRC, "bft_gpu")
K, G = 27, 5
NAMES = ["anc", "mut_one", "m2", "far", "empty"]


def _parse(path):
    lines = open(path).read().split("\n")
    assert lines[-1] == "" and len(lines) == G + 2
    assert lines[0].split("\t") == [""] + NAMES
    cells = [ln.split("\t") for ln in lines[1:-1]]
    assert [c[0] for c in cells] == NAMES and all(len(c) == G + 1 for c in cells)
    return [c[1:] for c in cells]


def test_the_three_tables(tmp_path):
    anc = S.random_genome(3000, 21)
    genomes = [anc, S.mutate(anc, 0.01, 22), S.mutate(anc, 0.03, 23), S.random_genome(1500, 24)]
    kms = [S.distinct(S.kmers_of(g, K)) for g in genomes]
    pool = S.distinct(np.concatenate(kms))
    Bm = np.stack([S.member(pool, km) for km in kms] + [np.zeros(len(pool), dtype=bool)], axis=1)
    want = Bm.T.astype(np.int64) @ Bm
    assert want[0, 1] > want[0, 2] > 0 and want[0, 3] == 0 and want[4, 4] == 0
    t = BFT(K, device=0)
    for g, name in enumerate(NAMES):
        assert t.add_genome(name) == g
        if g < 4:
            t.insert_kmers(kms[g], g)
    path = str(tmp_path / "i.bft")
    t.write_bft(path)
    t.close()
    out = subprocess.run([CLI, "load", path, "-genome_matrix", "shared", str(tmp_path / "s.tsv"), "-genome_matrix", "jaccard", str(tmp_path / "j.tsv"),
                          "-genome_matrix", "mash", str(tmp_path / "m.tsv")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    shared = _parse(tmp_path / "s.tsv")
    assert [[int(x) for x in row] for row in shared] == want.tolist()
    assert all(x.isdigit() for row in shared for x in row)
    n = np.diag(want)
    jac = _parse(tmp_path / "j.tsv")
    mash = _parse(tmp_path / "m.tsv")
    for i in range(G):
        for j in range(G):
            union = int(n[i] + n[j] - want[i, j])
            J = want[i, j] / union if union else 0.0
            D = min(1.0, -math.log(2 * J / (1 + J)) / K) + 0.0 if J > 0 else 1.0
            assert jac[i][j] == "%.6f" % J, (i, j)
            assert mash[i][j] == "%.6f" % D, (i, j)
    assert jac[0][0] == "1.000000" and jac[4][4] == "0.000000" and mash[0][0] == "0.000000" and mash[0][3] == "1.000000" and mash[4][4] == "1.000000"
    # an unknown word; a file that cannot be created
    bad = subprocess.run([CLI, "load", path, "-genome_matrix", "hamming", str(tmp_path / "x.tsv")], capture_output=True, text=True, timeout=120)
    assert bad.returncode != 0 and "hamming" in bad.stderr and not (tmp_path / "x.tsv").exists()
    bad = subprocess.run([CLI, "load", path, "-genome_matrix", "shared", str(tmp_path / "no_such_dir" / "x.tsv")], capture_output=True, text=True, timeout=120)
    assert bad.returncode != 0 and "Cannot create" in bad.stderr
