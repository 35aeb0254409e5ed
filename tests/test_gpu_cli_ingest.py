"""The CLI's file-type words `sequences` / `sequences_canonical` and the trailing `-min_abundance N` of `build` and `-add_genomes`
(csrc/bft_gpu_cli.c): an index built from FASTA / FASTQ files against an index built with `kmers` from k-mer files of the truth's k-mers
(tests/test_ingest_cases_host.py) under the same file names -- byte-identical -query_kmers CSV and -extract_kmers output."""
import os
import subprocess

import numpy as np
import pytest

from bloomfiltertrie_amd import _lib, synth as S
from test_ingest_cases_host import Truth, rand_text, revcomp, with_bad

pytestmark = pytest.mark.gpu
CLI = os.path.join(_lib.CSRC, "bft_gpu")
K = 27


def _genomes():
    rng = np.random.default_rng(23)
    a = rand_text(2000, rng)
    g0 = [a, a[300:800], with_bad(rand_text(500, rng), [250, 251]), b"acgtu" * 30]  # (every genome repeats some of its k-mers: -min_abundance 2 keeps those)
    g1 = [a[100:1200], revcomp(a[:400].decode()).encode(), rand_text(K - 1, rng), b"", rand_text(700, rng)]
    g2 = [a[1000:], a[1000:1500], rand_text(300, rng)]
    g3 = [revcomp(a[500:1500].decode()).encode(), a[600:900], rand_text(200, rng)]
    return [g0, g1, g2, g3]


def _write_seq(path, seqs, fastq):
    with open(path, "wb") as f:
        for i, s in enumerate(seqs):
            if fastq:
                f.write(b"@r%d\n%s\n+\n%s\n" % (i, s, b"I" * len(s)))
            else:
                f.write(b">s%d\n" % i + b"".join(s[j:j + 80] + b"\n" for j in range(0, len(s), 80)) + (b"" if s else b"\n"))


def _run(cwd, *args):
    out = subprocess.run([CLI, *args], capture_output=True, text=True, cwd=cwd, timeout=300)
    assert out.returncode == 0, out.stderr
    return out.stdout


def _outputs(cwd, bft):
    """(CSV of -query_kmers, -extract_kmers output) of an index, over the same query list"""
    _run(cwd, "load", bft, "-query_kmers", "kmers", "qlist.txt", "-extract_kmers", "kmers", "extracted.txt")
    return open(os.path.join(cwd, "queries.csv"), "rb").read(), open(os.path.join(cwd, "extracted.txt"), "rb").read()


def _dirs(tmp_path, genomes, canonical, min_abundance):
    """two working directories with the same file names: sequence files in one, the truth's k-mer files in the other, and one query list"""
    ds, dk = str(tmp_path / "seq"), str(tmp_path / "kmers")
    truths = [Truth(g, K, canonical, min_abundance) for g in genomes]
    allk = sorted({x for t in truths for x in t.kmers})
    rng = np.random.default_rng(1)
    mutants = S.packed_to_ascii(S.snp_mutants(S.ascii_to_packed(allk[:300], K)[0], K, 5), K)
    query = [allk[i] for i in rng.choice(len(allk), 500, replace=False)] + mutants[:100] + ["ACGTNNNNACGTACGTACGTACGTACG", "ACGT"]
    for d in (ds, dk):
        os.makedirs(d)
        with open(os.path.join(d, "queries.txt"), "w") as f:
            f.write("\n".join(query) + "\n")
        with open(os.path.join(d, "qlist.txt"), "w") as f:
            f.write(os.path.join(d, "queries.txt") + "\n")
    for i, (g, t) in enumerate(zip(genomes, truths)):
        name = f"genome{i}.{'fq' if i % 2 else 'fa'}"
        _write_seq(os.path.join(ds, name), g, fastq=bool(i % 2))
        with open(os.path.join(dk, name), "w") as f:
            f.write("".join(x + "\n" for x in t.kmers))
    for d in (ds, dk):
        for lst, ids in (("l01.txt", (0, 1)), ("l23.txt", (2, 3)), ("lall.txt", (0, 1, 2, 3))):
            with open(os.path.join(d, lst), "w") as f:
                f.write("".join(os.path.join(d, f"genome{i}.{'fq' if i % 2 else 'fa'}") + "\n" for i in ids))
    return ds, dk, truths


@pytest.mark.parametrize("word,extra", [("sequences", ()), ("sequences_canonical", ()), ("sequences_canonical", ("-min_abundance", "2")),
                                        ("sequences", ("-min_abundance", "1"))])
def test_build_and_add_genomes_from_sequence_files(tmp_path, word, extra):
    canonical, min_abundance = word.endswith("canonical"), int(extra[1]) if extra else 0
    ds, dk, truths = _dirs(tmp_path, _genomes(), canonical, min_abundance)
    assert all(t.appended > 0 for t in truths) and (not min_abundance or any(t.appended < t.distinct for t in truths) or min_abundance == 1)
    # build
    so = _run(ds, "build", str(K), word, "lall.txt", "all.bft", *extra)
    ko = _run(dk, "build", str(K), "kmers", "lall.txt", "all.bft")
    assert so.replace(ds, dk) == ko  # the same "File <id>: <path>" lines
    want = _outputs(dk, "all.bft")
    assert _outputs(ds, "all.bft") == want
    assert want[0].startswith(b"genome0.fa,genome1.fq,genome2.fa,genome3.fq\n") and want[1].count(b"\n") == len({x for t in truths for x in t.kmers})
    # -add_genomes on top of a build of the first two
    _run(ds, "build", str(K), word, "l01.txt", "a.bft", *extra)
    _run(ds, "load", "a.bft", "-add_genomes", word, "l23.txt", "b.bft", *extra)
    _run(dk, "build", str(K), "kmers", "l01.txt", "a.bft")
    _run(dk, "load", "a.bft", "-add_genomes", "kmers", "l23.txt", "b.bft")
    assert _outputs(ds, "b.bft") == _outputs(dk, "b.bft") == want
    # options still follow the optional -min_abundance
    out = _run(ds, "load", "a.bft", "-add_genomes", word, "l23.txt", "c.bft", *extra, "-extract_kmers", "kmers", "x.txt")
    assert open(os.path.join(ds, "x.txt"), "rb").read() == want[1] and "File 2:" in out


def test_min_abundance_is_refused_for_kmer_files(tmp_path):
    ds, dk, _ = _dirs(tmp_path, _genomes(), False, 0)
    out = subprocess.run([CLI, "build", str(K), "kmers", "lall.txt", "x.bft", "-min_abundance", "2"], capture_output=True, text=True, cwd=dk)
    assert out.returncode != 0 and "-min_abundance" in out.stderr
    out = subprocess.run([CLI, "build", str(K), "sequences", "lall.txt", "x.bft", "-min_abundance", "two"], capture_output=True, text=True, cwd=ds)
    assert out.returncode != 0 and "-min_abundance" in out.stderr
