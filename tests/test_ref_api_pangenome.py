"""extract_pangenome_kmers_to_disk with extract_core_kmers, extract_dispensable_kmers, extract_singleton_kmers and a callback of the caller's, of the
reference's snippets (<bft/snippets.h>, -lbft; src/snippets.c:10-106): tests/c/ref_pangenome_program.c, compiled with -Werror against the header as a
position-independent and as a fixed-address executable (the callbacks are told apart by their addresses across the library boundary), writes the classes
of an index of three genomes through the GPU route and through iterate_over_kmers; the files are checked against ground truth computed in Python from
the inserted k-mers, the two routes byte for byte against each other, the printed counts, and the error for an output file that cannot be created."""
import os
import subprocess

import pytest

from bloomfiltertrie_amd import _lib, synth as S

from test_gpu_components import _owners_of

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "ref_pangenome_program.c")
K = 27
CLASSES = {"core": (3, 3), "dispensable": (0, 2), "singleton": (1, 1)}


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    subprocess.check_call(["make", "-C", _lib.CSRC, "all"], stdout=subprocess.DEVNULL)
    d = tmp_path_factory.mktemp("pangenome")
    exes = {}
    for form, flags in (("pie", ["-fPIE", "-pie"]), ("nopie", ["-no-pie"])):
        exe = str(d / f"ref_pangenome_program_{form}")
        subprocess.check_call(["gcc", "-O2", "-std=gnu99", "-Wall", "-Werror"] + flags + ["-I", os.path.join(ROOT, "include"), "-o", exe, SRC, "-L",
                              _lib.CSRC, "-lbft", f"-Wl,-rpath,{_lib.CSRC}", f"-Wl,-rpath-link,{_lib.CSRC}", "-Wl,-rpath-link,/opt/rocm/lib"])
        exes[form] = exe
    anc = S.random_genome(6000, 71)
    files, lists = [], []
    for gid, g in enumerate((anc, S.mutate(anc, 0.01, 72), S.mutate(anc, 0.01, 73))):
        asc = S.packed_to_ascii(S.distinct(S.kmers_of(g, K)), K)
        path = str(d / f"genome{gid}.txt")
        with open(path, "w") as f:
            f.write("\n".join(asc) + "\n")
        files.append(path)
        lists.append((asc, gid))
    return exes, files, _owners_of(lists), d


def _run(program, form, mode, prefix):
    exes, files, _, _ = program
    return subprocess.run([exes[form], str(K), mode, prefix] + files, capture_output=True, text=True, timeout=300)


def _entries(path):
    data = open(path, "rb").read()
    assert len(data) % (K + 1) == 0 and (not data or data[-1] == 0)
    parts = data.split(b"\0")[:-1] if data else []
    assert all(len(p) == K for p in parts)
    return [p.decode() for p in parts]


def _want(owners, lo, hi):
    return {x for x, o in owners.items() if lo <= len(o) <= hi}


@pytest.mark.parametrize("form", ["pie", "nopie"])
def test_classes_on_disk_match_ground_truth_and_the_callback_route(program, form):
    _, _, owners, d = program
    gpu, cb = str(d / f"gpu_{form}"), str(d / f"cb_{form}")
    r = _run(program, form, "disk", gpu)
    assert r.returncode == 0, r.stderr
    want = {c: _want(owners, *CLASSES[c]) for c in CLASSES}
    assert all(len(w) >= 200 for w in want.values())
    assert r.stdout.splitlines() == [f"Number of extracted k-mers is {len(want[c])}." for c in ("core", "dispensable", "singleton")]
    r2 = _run(program, form, "iterate", cb)
    assert r2.returncode == 0, r2.stderr
    assert r2.stdout.splitlines() == [f"{c} {len(want[c])}" for c in ("core", "dispensable", "singleton")]
    for c in CLASSES:
        got = _entries(f"{gpu}.{c}")
        assert len(got) == len(want[c]) and set(got) == want[c], c
        assert open(f"{gpu}.{c}", "rb").read() == open(f"{cb}.{c}", "rb").read(), c  # (both routes visit the k-mers in row order)


@pytest.mark.parametrize("form", ["pie", "nopie"])
def test_a_callback_of_the_callers_is_served(program, form):
    _, _, owners, d = program
    prefix = str(d / f"own_{form}")
    r = _run(program, form, "own", prefix)
    assert r.returncode == 0, r.stderr
    want = _want(owners, 2, 2)
    assert len(want) > 0
    got = _entries(prefix + ".two")
    assert len(got) == len(want) and set(got) == want
    assert r.stdout.splitlines() == [f"Number of extracted k-mers is {len(want)}."]


def test_an_uncreatable_output_file_is_an_error(program):
    _, _, _, d = program
    r = _run(program, "pie", "unwritable", str(d / "no_such_directory" / "out"))
    assert r.returncode != 0
    assert "extract_pangenome_kmers_to_disk()" in r.stderr
