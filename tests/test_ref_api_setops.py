"""intersection_annotations / union_annotations / sym_difference_annotations and the three byte helpers of the reference's API (<bft/bft.h>, -lbft;
include/bft.h:100-114, src/bft.c:421-613): tests/c/ref_setops_program.c, written against the reference's names only and compiled with -Werror, takes
get_annotation of k-mer pairs and triples of a 5-genome k = 27 and a 70-genome k = 18 index (multi-byte ids; annotations in modes 0, 1 and 2) and prints
each operation with 1, 2 and 3 arguments and results nested as arguments.  Every printed result is compared with Python sets and, byte for byte, with
the mode-0 image cmp_annots returns (src/annotation.c:2358-2551).  nb_annotations == 0 and a NULL argument exit with the reference's messages."""
import os
import subprocess

import numpy as np
import pytest

from bloomfiltertrie_amd import _lib, synth as S

from test_gpu_components import _owners_of

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "ref_setops_program.c")
NAMES = {"i": "intersection_annotations", "u": "union_annotations", "s": "sym_difference_annotations"}


def _image(ids, genomes):
    out = bytearray(max((genomes + 2 + 7) // 8, 1))
    for g in ids:
        out[(g + 2) >> 3] |= 1 << ((g + 2) & 7)
    return bytes(out)


def _five(d):
    """5 genomes, k = 27: an ancestor and SNP mutants"""
    anc = S.random_genome(3000, 81)
    lists = [(S.packed_to_ascii(S.distinct(S.kmers_of(g, 27)), 27), gid)
             for gid, g in enumerate([anc] + [S.mutate(anc, 0.02, 82 + i) for i in range(4)])]
    return 27, lists


def _seventy(d):
    """70 genomes, k = 18, 300 k-mers: a third held by a run of consecutive genomes (ranges), a third by two or three (id lists, ids of one and of two
    bytes), a third by a random half (bitmaps)"""
    rng = np.random.default_rng(7)
    asc = S.packed_to_ascii(S.distinct(S.pack_codes(rng.integers(0, 4, (320, 18), dtype=np.uint8)))[:300], 18)
    own = np.zeros((300, 70), dtype=bool)
    for i in range(300):
        if i % 3 == 0:
            a = int(rng.integers(0, 40))
            own[i, a:a + int(rng.integers(12, 30))] = True
        elif i % 3 == 1:
            own[i, rng.choice(70, int(rng.integers(2, 4)), replace=False)] = True
        else:
            own[i] = rng.random(70) < 0.5
            own[i, 0] = True
    return 18, [([asc[i] for i in np.nonzero(own[:, g])[0]], g) for g in range(70)]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    subprocess.check_call(["make", "-C", _lib.CSRC, "all"], stdout=subprocess.DEVNULL)
    d = tmp_path_factory.mktemp("setops")
    exe = str(d / "ref_setops_program")
    subprocess.check_call(["gcc", "-O2", "-std=gnu99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, SRC, "-L", _lib.CSRC, "-lbft",
                           f"-Wl,-rpath,{_lib.CSRC}", f"-Wl,-rpath-link,{_lib.CSRC}", "-Wl,-rpath-link,/opt/rocm/lib"])
    cases = {}
    for name, make in (("five", _five), ("seventy", _seventy)):
        k, lists = make(d)
        files = []
        for asc, gid in lists:
            path = str(d / f"{name}_{gid}.txt")
            with open(path, "w") as f:
                f.write("\n".join(asc) + "\n")
            files.append(path)
        owners = _owners_of(lists)
        rng = np.random.default_rng(len(files))
        stored = sorted(owners)
        groups = [[stored[j] for j in rng.choice(len(stored), 1 + i % 3, replace=False)] for i in range(90)]
        gfile = str(d / f"{name}_groups.txt")
        with open(gfile, "w") as f:
            f.write("".join(" ".join(g) + "\n" for g in groups))
        cases[name] = (k, files, owners, groups, gfile)
    return exe, cases


def _run(exe, case, mode):
    k, files, _, _, gfile = case
    return subprocess.run([exe, str(k), mode, gfile] + files, capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize("name", ["five", "seventy"])
def test_operations_match_sets_and_the_byte_image(program, name):
    exe, cases = program
    k, files, owners, groups, _ = cases[name]
    genomes = len(files)
    r = _run(exe, cases[name], "ops")
    assert r.returncode == 0, r.stderr
    lines = iter(r.stdout.splitlines())
    modes, differ = set(), 0
    for grp in groups:
        sets = [owners[x] for x in grp]
        want = []
        for s in sets:
            want.append(("in", s))
        for op in ("and", "or", "sym"):
            for m in range(1, len(sets) + 1):
                part = sets[:m]
                inter, union = set.intersection(*part), set.union(*part)
                # (one argument: its set under every operation -- the reference's intersection returns the empty set there)
                want.append((f"{op}{m}", inter if op == "and" else union if op == "or" or m == 1 else union - inter))
        if len(sets) == 3:
            a, b, c = sets
            r1 = (a | b) & c
            tri = [a & b, b | c, a]
            want += [("nest1", r1), ("nest2", set.union(*tri) - set.intersection(*tri)), ("nest3", r1)]
            differ += (a & b & c) != (a | b | c)
        for tag, ids in want:
            got = next(lines).split()
            assert got[0] == tag, (got, tag)
            size, data, n, listed = int(got[1]), bytes.fromhex(got[2]), int(got[3]), [int(x) for x in got[4:]]
            assert size == len(data) and n == len(listed) and listed == sorted(ids), (tag, grp)
            if tag == "in":
                modes.add(data[0] & 3)
            else:
                assert data == _image(ids, genomes), (tag, grp)
        assert next(lines) == "end"
    assert next(lines, None) is None
    assert differ >= 10
    assert modes == ({0, 1, 2} if name == "seventy" else modes) and modes  # (the 70-genome index hands out ranges and id lists too)


def test_helpers(program):
    exe, cases = program
    r = _run(exe, cases["five"], "helpers")
    assert r.returncode == 0 and r.stdout.split() == ["48", "252", "204"]


@pytest.mark.parametrize("which", ["i", "u", "s"])
def test_no_annotation_and_a_null_annotation_exit_like_the_reference(program, which):
    exe, cases = program
    r = _run(exe, cases["five"], f"zero-{which}")
    assert r.returncode == 1 and r.stdout == ""
    assert r.stderr.endswith(f"{NAMES[which]}(): no annotations given as parameters.\n")
    r = _run(exe, cases["five"], f"null-{which}")
    assert r.returncode == 1 and r.stdout == ""
    assert r.stderr.endswith(f"usage of a null pointer in function {NAMES[which]}()\n \n")  # (ASSERT_NULL_PTR, include/useful_macros.h:38-43)
