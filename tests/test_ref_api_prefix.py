"""prefix_matching of the reference's public API (<bft/bft.h>, -lbft; include/bft.h:135, src/bft.c:1087-1147): tests/c/ref_prefix_program.c,
compiled with -Werror against the header, lists the matches of a prefix with their genome ids (get_annotation inside the callback) equal to
ground truth, stops when the callback returns 0, returns false when nothing matches and exits on a bad prefix."""
import os
import subprocess

import numpy as np
import pytest

from bloomfiltertrie_amd import _lib, synth as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "ref_prefix_program.c")
K = 27


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    subprocess.check_call(["make", "-C", _lib.CSRC, "all"], stdout=subprocess.DEVNULL)
    d = tmp_path_factory.mktemp("prefix")
    exe = str(d / "ref_prefix_program")
    subprocess.check_call(["gcc", "-O2", "-std=gnu99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, SRC, "-L", _lib.CSRC, "-lbft",
                           f"-Wl,-rpath,{_lib.CSRC}", f"-Wl,-rpath-link,{_lib.CSRC}", "-Wl,-rpath-link,/opt/rocm/lib"])
    anc = S.random_genome(6000, 21)
    genomes = [anc, S.mutate(anc, 0.03, 22), S.mutate(anc, 0.03, 23)]
    files, truth = [], {}
    for gid, g in enumerate(genomes):
        asc = S.packed_to_ascii(S.distinct(S.kmers_of(g, K)), K)
        path = str(d / f"genome{gid}.txt")
        with open(path, "w") as f:
            f.write("\n".join(asc) + "\n")
        files.append(path)
        for s in asc:
            truth.setdefault(s, []).append(gid)
    return exe, files, truth


def _run(program, mode, prefix):
    exe, files, _ = program
    return subprocess.run([exe, str(K), mode, prefix] + files, capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize("prefix_len", [4, 9, 10, 17, 26, 27])
def test_lists_matches_with_genome_ids(program, prefix_len):
    truth = program[2]
    prefix = sorted(truth)[len(truth) // 3][:prefix_len].lower()  # (either case, as parseKmerCount)
    r = _run(program, "list", prefix)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().split("\n")
    want = sorted((s, ",".join(map(str, ids))) for s, ids in truth.items() if s.startswith(prefix.upper()))
    got = [tuple(l.split(" ")) for l in lines[:-1]]
    assert sorted(got) == want and len(got) == len(want) > 0
    assert lines[-1] == f"matched 1 calls {len(want)}"


def test_stops_when_the_callback_returns_zero(program):
    r = _run(program, "stop3", "A")
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == "matched 1 calls 3"


def test_no_match_returns_false(program):
    truth = program[2]
    prefix = next(p for p in ("".join(np.random.default_rng(i).choice(list("ACGT"), 12)) for i in range(1000))
                  if not any(s.startswith(p) for s in truth))
    r = _run(program, "list", prefix)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == "matched 0 calls 0"


@pytest.mark.parametrize("prefix", ["", "A" * (K + 1), "ACGNA"])
def test_bad_prefix_exits(program, prefix):
    r = _run(program, "list", prefix)
    assert r.returncode == 1 and "prefix_matching()" in r.stderr
