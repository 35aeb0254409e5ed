"""CPU-side tests of the k-mer hash's geometry (no GPU): which (key width W, slots per line S) bft_kh_geometry (csrc/bft_walk.h) can
pick, that KH_DISPATCH (csrc/bft_kh_dev.h) has a kernel for each of them, and that the cases of tests/test_gpu_kh_geometries.py --
one per reachable (W, S) -- still land on the geometry they are meant to run.  When the geometry changes, this file fails until a GPU
case covers the new (W, S) again."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from bloomfiltertrie_amd import _lib, synth as S

# (W, S) -> the indexes that run it: (k, colour sets, kmer_hash_load), N_KMERS distinct k-mers each.  "Body full": the slot body's
# bits are used to the last one (cb + db + kb - f == 8 wb); a colour-set count of 2^c - 1 puts the top id at all ones in c value bits.
N_KMERS = 200000
CASES = {
    (1, 10): [(18, 3, 55)],
    (1, 9): [(27, 7, 55)],
    (1, 8): [(31, 4095, 55)],            # 12 value bits, top id all ones
    (1, 7): [(32, 4096, 55)],            # body full; k = 32 fills the word
    (1, 6): [(31, 131071, 55)],          # 17 value bits
    (2, 9): [(33, 1, 10)],               # body full; the first two-word k
    (2, 8): [(34, 1, 55)],
    (2, 7): [(37, 7, 55)],               # body full
    (2, 6): [(48, 1, 55)],               # body full
    (2, 5): [(50, 255, 55)],             # body full
    (2, 4): [(62, 32767, 55)],           # body full
    (2, 3): [(64, 32767, 55)],           # k = 64
    (3, 4): [(65, 1, 55), (69, 1, 55)],  # the first three-word k; 69: body full
    (3, 3): [(85, 1, 55)],               # body full
    (3, 2): [(96, 7, 55)],               # k = 96
    (4, 2): [(97, 7, 55), (109, 131071, 55)],  # the first four-word k; 109: body full
    (4, 1): [(126, 131071, 55), (126, 131071, 80)],  # 80: an overflow list
}
# ten slots of two-word keys need more k-mers than a small case holds: the large case of the GPU file
LARGE = {(2, 10): (33, 1, 10, 125_000_000)}
PALINDROMES = 8  # reverse-complement palindromes among the stored k-mers at even k
HOT_FAMILIES = 24  # families of 16 k-mers (every first and last nucleotide: one home line) gathered into a few neighbouring home lines


def words(k):
    return (2 * k + 63) // 64


def hot_run(lib, k, n, n_sets, load, rng):
    """HOT_FAMILIES x 16 k-mers whose home lines, under the geometry of n k-mers with n_sets colour sets at `load`, lie within
    nl / 4096 lines of each other: more than the slots up to the largest displacement hold at any S, so a run of full lines that
    ends in the overflow list"""
    g = geometry_of(lib, k, n, n_sets, load)
    width = max(1, g["nl"] // 4096)
    seeds = rng.integers(0, 4, (HOT_FAMILIES * 4096, k), dtype=np.uint8)
    packed = np.ascontiguousarray(S.pack_codes(seeds))
    homes = np.zeros(len(seeds), np.uint64)
    lib.bft_hosttest_kh_homes_of(packed.ctypes.data, len(packed), k, n, n_sets, load, homes.ctypes.data)
    order = np.argsort(homes, kind="stable")
    hs = homes[order].astype(np.int64)
    cnt = np.searchsorted(hs, hs + width) - np.arange(len(hs))  # seeds in [home, home + width)
    a = int(np.argmax(cnt))
    pick = seeds[order[a:a + min(int(cnt[a]), HOT_FAMILIES)]]
    assert len(pick) >= HOT_FAMILIES // 2, (k, n_sets, load, int(cnt[a]))
    fam = np.repeat(pick, 16, axis=0)
    fam[:, 0] = np.tile(np.repeat(np.arange(4, dtype=np.uint8), 4), len(pick))
    fam[:, -1] = np.tile(np.arange(4, dtype=np.uint8), 4 * len(pick))
    return S.pack_codes(fam)


def case_data(lib, k, n, n_sets, load, seed):
    """n distinct k-mers and a colour-set index in [0, n_sets) per k-mer, every index used: a few reverse-complement palindromes at
    even k, a hot run (hot_run) under the case's geometry and one under its geometry at 80 %, then the distinct k-mers of a random
    genome in order of first occurrence, truncated.  Genome g holds the k-mers whose index + 1 has bit g set, so there are exactly
    n_sets distinct colour sets.  Returns (packed [n, B], set index [n], genome codes)."""
    rng = np.random.default_rng(seed)
    parts = []
    if k % 2 == 0:
        half = rng.integers(0, 4, (PALINDROMES, k // 2), dtype=np.uint8)
        parts.append(S.pack_codes(np.concatenate([half, 3 - half[:, ::-1]], axis=1)))
    parts += [hot_run(lib, k, n, n_sets, load, rng), hot_run(lib, k, n, n_sets, 80, rng)]
    genome = rng.integers(0, 4, n + n // 50 + k + 1000, dtype=np.uint8)
    parts.append(S.kmers_of(genome, k))
    km = S.distinct(np.concatenate(parts))[:n]
    assert len(km) == n
    sets = (rng.permutation(n) % n_sets).astype(np.uint32)
    return np.ascontiguousarray(km), sets, genome


def n_genomes(n_sets):
    return int(n_sets).bit_length()


@pytest.fixture(scope="module")
def hostlib():
    subprocess.check_call(["make", "-C", _lib.CSRC, "libbft_hosttest.so"], stdout=subprocess.DEVNULL)
    return load_hostlib()


def load_hostlib():
    lib = C.CDLL(os.path.join(_lib.CSRC, "libbft_hosttest.so"))
    lib.bft_hosttest_kh_geometry_of.argtypes = [C.c_int, C.c_uint64, C.c_uint64, C.c_uint32, C.c_void_p]
    lib.bft_hosttest_kh_reachable.restype = C.c_int64
    lib.bft_hosttest_kh_reachable.argtypes = [C.c_void_p, C.c_uint32]
    lib.bft_hosttest_kh_build.restype = C.c_uint64
    lib.bft_hosttest_kh_build.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.bft_hosttest_kh_verify.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                                           C.c_uint32]
    lib.bft_hosttest_roundtrip.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p]
    lib.bft_hosttest_kh_homes_of.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_uint64, C.c_uint64, C.c_uint32, C.c_void_p]
    return lib


def geometry_of(lib, k, n, n_values, load):
    """bft_kh_geometry: dict of the fields of bft_hosttest_kh_geometry"""
    g = np.zeros(14, np.uint32)
    lib.bft_hosttest_kh_geometry_of(k, n, n_values, load, g.ctypes.data)
    names = ["S", "f", "wb", "cb", "kb", "qb", "hb", "restb", "t", "m", "nl", "maxd", "db", "novf"]
    return dict(zip(names, [int(x) for x in g]))


def reachable(lib):
    """{(W, S): (k, n, n_values, load)} of the host scan"""
    out = np.zeros(64 * 6, np.uint64)
    rows = lib.bft_hosttest_kh_reachable(out.ctypes.data, 64)
    assert 0 < rows <= 64, rows  # (negative: the scan disagreed with bft_kh_geometry)
    return {(int(r[0]), int(r[1])): tuple(int(x) for x in r[2:]) for r in out.reshape(-1, 6)[:rows]}


def dispatch_entries():
    src = open(os.path.join(_lib.CSRC, "bft_kh_dev.h")).read()
    body = src[src.index("#define KH_DISPATCH"):]
    body = body[:body.index("default:")]
    return {(int(w), int(s)) for w, s in re.findall(r"case (\d+) \* 16 \+ (\d+):", body)}


def sorted_tform(lib, km, k):
    """the sorted table of the index: T-form rows (W words, most significant first), in T order, and the permutation that sorts"""
    W = words(k)
    tf = np.zeros(len(km) * W, np.uint64)
    back = np.zeros_like(km)
    lib.bft_hosttest_roundtrip(km.ctypes.data, len(km), k, back.ctypes.data, tf.ctypes.data)
    tf = tf.reshape(-1, W)
    order = np.lexsort(tuple(tf[:, w] for w in range(W - 1, -1, -1)))
    return np.ascontiguousarray(tf[order]), order


def test_every_reachable_geometry_has_a_kernel_and_a_gpu_case(hostlib):
    reach = reachable(hostlib)
    disp = dispatch_entries()
    assert len(disp) == 20
    assert set(reach) <= disp, sorted(set(reach) - disp)
    assert set(reach) == set(CASES) | set(LARGE), (sorted(set(reach) - set(CASES) - set(LARGE)), sorted(set(CASES) | set(LARGE) - set(reach)))
    assert disp - set(reach) == {(1, 4), (1, 5)}
    for (W, S), (k, n, nv, load) in reach.items():  # (the examples themselves: their k has W words and the geometry picks S there)
        assert words(k) == W and 1 <= nv <= n < 2 ** 31 and 10 <= load <= 80
        assert geometry_of(hostlib, k, n, nv, load)["S"] == S


@pytest.mark.parametrize("ws", sorted(CASES) + sorted(LARGE), ids=lambda ws: f"W{ws[0]}-S{ws[1]}")
def test_gpu_cases_land_on_their_geometry(hostlib, ws):
    W, S_ = ws
    subs = [(k, ns, load, N_KMERS) for k, ns, load in CASES[ws]] if ws in CASES else [LARGE[ws]]
    for k, n_sets, load, n in subs:
        g = geometry_of(hostlib, k, n, n_sets, load)
        assert words(k) == W and g["S"] == S_, (k, n_sets, load, g)
        assert g["cb"] == max(1, int(n_sets).bit_length()) and g["nl"] + 256 < 2 ** 32
        if S_ > 1:
            assert g["cb"] + g["db"] + g["kb"] - g["f"] <= 8 * g["wb"]
    # the edges the cases are there for
    full = lambda k, ns, load: (lambda g: g["cb"] + g["db"] + g["kb"] - g["f"] == 8 * g["wb"])(geometry_of(hostlib, k, N_KMERS, ns, load))
    for ws_, k, ns, load in [((1, 7), 32, 4096, 55), ((2, 9), 33, 1, 10), ((2, 7), 37, 7, 55), ((2, 6), 48, 1, 55), ((2, 5), 50, 255, 55),
                             ((2, 4), 62, 32767, 55), ((3, 4), 69, 1, 55), ((3, 3), 85, 1, 55), ((4, 2), 109, 131071, 55)]:
        if ws_ == ws:
            assert full(k, ns, load), (k, ns, load)


@pytest.mark.parametrize("ws", sorted(CASES), ids=lambda ws: f"W{ws[0]}-S{ws[1]}")
def test_host_restatement_of_the_cases_at_load_80(hostlib, ws):
    """The sequential build (bft_kh_host.h) of each small case's k-mers at 80 %: the table verifies, and the hot run of the case at
    80 % runs beyond the displacement bits into the overflow list, whatever the slots per line."""
    k, n_sets, load = CASES[ws][0]
    km, sets, _ = case_data(hostlib, k, N_KMERS, n_sets, load, seed=k)
    tk, order = sorted_tform(hostlib, km, k)
    vals = np.ascontiguousarray(sets[order])
    g = geometry_of(hostlib, k, len(tk), n_sets, 80)
    words_cap = (g["nl"] + 256) * 8
    lines = np.zeros(words_cap, np.uint64)
    geo = np.zeros(14, np.uint32)
    W = words(k)
    ovk, ovv = np.zeros(4096 * W, np.uint64), np.zeros(4096, np.uint32)
    nw = hostlib.bft_hosttest_kh_build(tk.ctypes.data, vals.ctypes.data, len(tk), k, n_sets, 80, lines.ctypes.data, words_cap, geo.ctypes.data, ovk.ctypes.data,
                                       ovv.ctypes.data)
    assert nw == words_cap, (nw, words_cap)
    novf = int(geo[13])
    rc = hostlib.bft_hosttest_kh_verify(tk.ctypes.data, vals.ctypes.data, len(tk), k, n_sets, 80, int(geo[11]), lines.ctypes.data, g["nl"] + 256, ovk.ctypes.data,
                                        ovv.ctypes.data, novf)
    assert rc == 1, rc
    assert novf > 0, (ws, g)
