"""CPU-side tests (no GPU) of merging two indexes (csrc/bft_union.hip, bft_gpu_merge): the case sets tests/test_gpu_union.py runs -- how the rows
of one sorted pool are dealt to the two sources so that the co-ranked placement meets every tile edge, the sizes and positions of a small side,
the genome-id layouts that change the dictionary's id width -- with a restatement of the split rule that checks the cases reach what they claim
to reach; the tile constant; the new kernels' resources; the new symbols; NULL arguments.  When the tile or the split rule changes, this file fails
until the cases cover every edge again."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from bloomfiltertrie_amd import _lib, synth as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 1024  # BFT_UNION_TILE (csrc/bft_union.h): keys of the merged diagonal per workgroup
EDGE_KS = (27, 63, 99, 126)  # W = 1 .. 4


def test_tile_constant_is_the_headers():
    txt = open(os.path.join(_lib.CSRC, "bft_union.h")).read()
    m = re.search(r"^#define\s+BFT_UNION_TILE\s+(\d+)\s*$", txt, flags=re.M)
    assert m and int(m.group(1)) == TILE
    assert TILE % 64 == 0


# ---- one sorted pool --------------------------------------------------------------------------------------------------------------------------
def table_order(km, k):
    """the packed k-mers in the order of the sorted table: ascending T-form, word 0 first (the host restatement's T-form, libbft_hosttest.so)"""
    subprocess.check_call(["make", "-C", _lib.CSRC, "libbft_hosttest.so"], stdout=subprocess.DEVNULL)
    lib = C.CDLL(os.path.join(_lib.CSRC, "libbft_hosttest.so"))
    lib.bft_hosttest_roundtrip.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p]
    lib.bft_hosttest_roundtrip.restype = None
    km = np.ascontiguousarray(km)
    W = (2 * k + 63) // 64
    back = np.zeros_like(km)
    t = np.zeros((len(km), W), dtype=np.uint64)
    lib.bft_hosttest_roundtrip(km.ctypes.data, len(km), k, back.ctypes.data, t.ctypes.data)
    assert (back == km).all()
    order = np.lexsort(tuple(t[:, w] for w in range(W - 1, -1, -1)))
    return np.ascontiguousarray(km[order])


def pool(k, n, seed):
    """n distinct packed k-mers of a random genome, in table order"""
    km = S.distinct(S.kmers_of(S.random_genome(n + k + 63, seed), k))
    assert len(km) >= n
    return table_order(km[:n], k)


def test_table_order_is_strict_and_total():
    for k in EDGE_KS:
        km = pool(k, 300, k)
        assert len(S.distinct(km)) == 300
        again = table_order(km[np.random.default_rng(k).permutation(300)], k)
        assert (again == km).all()


# ---- the split rule, restated -----------------------------------------------------------------------------------------------------------------
def split(ia, ib, d):
    """(i, j, parted): rows of a and of b in front of diagonal d of the stable merge (a's row first among equals), j one more when the boundary
    would part a pair of equal keys (parted).  ia, ib: the two sides as ascending row numbers of the pool -- the row number is the key."""
    n_a, n_b = len(ia), len(ib)
    lo, hi = max(0, d - n_b), min(n_a, d)
    while lo < hi:
        mid = (lo + hi) // 2
        if ia[mid] <= ib[d - 1 - mid]:
            lo = mid + 1
        else:
            hi = mid
    j = d - lo
    parted = lo > 0 and j < n_b and ia[lo - 1] == ib[j]
    return lo, j + (1 if parted else 0), parted


def tiles_of(ia, ib, tile=TILE):
    """[(i0, i1, j0, j1, parted at its start)] of every tile"""
    n = len(ia) + len(ib)
    cuts = [split(ia, ib, min(t * tile, n)) for t in range((n + tile - 1) // tile + 1)]
    return [(cuts[t][0], cuts[t + 1][0], cuts[t][1], cuts[t + 1][1], cuts[t][2]) for t in range(len(cuts) - 1)]


def tiles_are_sound(ia, ib, tile=TILE):
    """what k_un_count / k_un_emit rely on: the tiles partition both sides in order, none stages more than tile + 1 rows, and no key is in two tiles"""
    tl = tiles_of(ia, ib, tile)
    assert tl[0][0] == 0 and tl[0][2] == 0 and tl[-1][1] == len(ia) and tl[-1][3] == len(ib)
    n_out = 0
    for t, (i0, i1, j0, j1, _) in enumerate(tl):
        assert i0 <= i1 and j0 <= j1 and (i1 - i0) + (j1 - j0) <= tile + 1 and i1 - i0 <= tile
        if t:
            assert tl[t - 1][1] == i0 and tl[t - 1][3] == j0
        keys = np.union1d(ia[i0:i1], ib[j0:j1])
        if t + 1 < len(tl) and len(keys):
            rest = np.concatenate([ia[i1:], ib[j1:]])
            assert len(rest) == 0 or keys[-1] < rest.min()
        n_out += len(keys)
    assert n_out == len(np.union1d(ia, ib))
    return tl


# ---- 1. placement edges: stretches of one pool ----------------------------------------------------------------------------------------------------
# (kind, rows): only_a / only_b: one side holds the stretch; both: every key in both; alt: a, b, both in turn
EDGE_STRETCHES = (("only_a", 2 * TILE + 37), ("both", 2 * TILE + 1), ("only_b", 2 * TILE + 41), ("both", 2 * TILE + 2), ("alt", 2 * TILE + 5),
                  ("only_b", TILE), ("only_a", TILE - 1), ("only_b", TILE + 1), ("only_a", TILE), ("both", 2 * TILE + 3), ("only_b", 9), ("alt", 2 * TILE + 7))
EDGE_ROWS = sum(n for _, n in EDGE_STRETCHES)


def edge_split():
    """(ia, ib, kind of every pool row)"""
    ia, ib, kinds, at = [], [], [], 0
    for kind, n in EDGE_STRETCHES:
        rows = np.arange(at, at + n)
        at += n
        if kind == "only_a":
            ia.append(rows)
        elif kind == "only_b":
            ib.append(rows)
        elif kind == "both":
            ia.append(rows)
            ib.append(rows)
        else:
            ia.append(rows[rows % 3 != 1])
            ib.append(rows[rows % 3 != 0])
        kinds += [kind] * n
    return np.concatenate(ia), np.concatenate(ib), kinds


def test_edge_stretches_reach_every_tile_edge():
    ia, ib, kinds = edge_split()
    assert len(kinds) == EDGE_ROWS and EDGE_ROWS > 6 * TILE
    for kind, n in EDGE_STRETCHES[:5]:
        assert n > 2 * TILE
    assert {n for _, n in EDGE_STRETCHES} >= {TILE - 1, TILE, TILE + 1}
    tl = tiles_are_sound(ia, ib)
    # a boundary inside a stretch of pairs: some part a pair (the earlier tile takes the second half), some fall between two pairs
    parted = [t for t, x in enumerate(tl) if x[4]]
    between = [t for t, x in enumerate(tl) if t and not x[4] and x[0] < len(ia) and x[2] < len(ib) and kinds[ia[x[0]]] == "both" and ia[x[0]] == ib[x[2]]
               and kinds[ia[x[0] - 1]] == "both"]
    assert len(parted) >= 2 and len(between) >= 2, (parted, between)
    # boundaries inside the alternating stretches: one that parts a pair, one that does not
    assert any(kinds[ia[tl[t][0] - 1]] == "alt" and kinds[ia[tl[t][0]]] == "alt" for t in parted)
    assert any(t and not x[4] and x[0] < len(ia) and kinds[ia[x[0] - 1]] == "alt" and kinds[ia[x[0]]] == "alt" for t, x in enumerate(tl))
    # every shape of a tile between parted boundaries: parted at its start and at its end (tile rows, one row late), at its end only (tile + 1
    # rows staged), at its start only (tile - 1 rows)
    ends = [t + 1 < len(tl) and bool(tl[t + 1][4]) for t in range(len(tl))]
    rows = [(x[1] - x[0]) + (x[3] - x[2]) for x in tl]
    assert any(x[4] and ends[t] and rows[t] == TILE for t, x in enumerate(tl))
    assert any(not x[4] and ends[t] and rows[t] == TILE + 1 for t, x in enumerate(tl))
    assert any(x[4] and not ends[t] and t + 1 < len(tl) and rows[t] == TILE - 1 for t, x in enumerate(tl))
    # tiles of one side only, and tiles of both
    assert any(x[1] - x[0] == TILE and x[3] == x[2] for x in tl) and any(x[3] - x[2] == TILE and x[1] == x[0] for x in tl)
    assert any(x[1] > x[0] and x[3] > x[2] for x in tl)
    assert max((x[1] - x[0]) + (x[3] - x[2]) for x in tl) == TILE + 1  # the + 1 row of LDS is used


# ---- 2. sizes and positions of a small side ----------------------------------------------------------------------------------------------------------
SMALL_SIZES = (1, TILE - 1, TILE, TILE + 1)
BIG_ROWS = 3 * TILE + 17
SIZE_CASES = [(side, n) for side in ("a", "b") for n in SMALL_SIZES] + [("below", 0), ("above", 0)]


def size_split(side, n_small, seed=0):
    """(ia, ib, pool rows): the small side's rows spread at random among the big side's (a third of them also in the big side); below / above:
    b (TILE + 9 rows) wholly below / above a (2 TILE + 3 rows)"""
    rng = np.random.default_rng(1000 * n_small + seed + (side == "a"))
    if side in ("below", "above"):
        nb, na = TILE + 9, 2 * TILE + 3
        every = np.arange(na + nb)
        return (every[nb:], every[:nb], na + nb) if side == "below" else (every[:na], every[na:], na + nb)
    shared = n_small // 3
    n = BIG_ROWS + n_small - shared
    small = np.sort(rng.choice(n, n_small, replace=False))
    drop = rng.choice(n_small, n_small - shared, replace=False)  # small rows the big side does not hold
    big = np.setdiff1d(np.arange(n), small[drop])
    assert len(big) == BIG_ROWS
    return (small, big, n) if side == "a" else (big, small, n)


@pytest.mark.parametrize("side,n_small", SIZE_CASES)
def test_size_cases_are_what_their_names_say(side, n_small):
    ia, ib, n = size_split(side, n_small)
    assert len(np.union1d(ia, ib)) == n and (np.diff(ia) > 0).all() and (np.diff(ib) > 0).all()
    tl = tiles_are_sound(ia, ib)
    if side == "below":
        assert ib[-1] < ia[0] and tl[0][1] == 0 and tl[-1][3] == tl[-1][2]
    elif side == "above":
        assert ia[-1] < ib[0] and tl[0][3] == 0 and tl[-1][1] == tl[-1][0]
    else:
        small = ia if side == "a" else ib
        assert len(small) == n_small and len(ia if side == "b" else ib) == BIG_ROWS > 3 * TILE
        assert len(np.intersect1d(ia, ib)) == n_small // 3


# ---- 3. genome-id layouts: the dictionary's id width on each side and in the result -------------------------------------------------------------
# name -> (ids a's rows draw from, ids (local to b) b's rows draw from, id_base, bytes per id of a, of b, of the result)
def width_layout(name):
    rng = np.random.default_rng(len(name) + 7)
    if name == "b_crosses_255":      # a: one byte; b: one byte, its ids land on 200 .. 299
        return np.concatenate([np.sort(rng.choice(199, 20, replace=False)), [199]]), np.concatenate([[0, 55, 56], np.sort(rng.choice(np.arange(57, 100), 20, replace=False))]), 200, 1, 1, 2
    if name == "b_crosses_65535":    # a: two bytes up to 65535; b: one byte, its ids land on 65500 .. 65600 (wide4 of test_merge_cases_host.py)
        return np.concatenate([np.sort(rng.choice(65535, 20, replace=False)), [65535]]), np.concatenate([[0, 35, 36], np.sort(rng.choice(np.arange(37, 101), 20, replace=False))]), 65500, 2, 1, 4
    if name == "a_wide_b_narrow":    # the reverse: a's ids take four bytes, b's stay below 256 in the result
        return np.concatenate([np.sort(rng.choice(60000, 20, replace=False)), [70000]]), np.sort(rng.choice(250, 24, replace=False)), 0, 4, 1, 4
    assert name == "a_two_b_one"     # a's take two, b's one, and the result two
    return np.concatenate([np.sort(rng.choice(255, 12, replace=False)), [255, 256, 40000]]), np.sort(rng.choice(256, 24, replace=False)), 0, 2, 1, 2


WIDTH_LAYOUTS = ("b_crosses_255", "b_crosses_65535", "a_wide_b_narrow", "a_two_b_one")
WIDTH_ROWS = 2 * TILE + 100


def width_sets(name, seed=3):
    """(ia, ib, x_of, y_of, id_base): thirds of the pool in a only, in both, in b only; per row one to three ids of its side's pool"""
    ids_a, ids_b, id_base, _, _, _ = width_layout(name)
    rng = np.random.default_rng(seed)
    n = WIDTH_ROWS
    side = rng.integers(0, 3, n)  # 0: a, 1: both, 2: b
    ia, ib = np.flatnonzero(side <= 1), np.flatnonzero(side >= 1)
    x_of, y_of = [()] * n, [()] * n
    for r in ia:
        x_of[r] = tuple(int(v) for v in np.sort(rng.choice(ids_a, int(rng.integers(1, 4)), replace=False)))
    for r in ib:
        y_of[r] = tuple(int(v) for v in np.sort(rng.choice(ids_b, int(rng.integers(1, 4)), replace=False)))
    # every id of both pools is used, so that the widths are what the layout says
    for i, g in enumerate(ids_a):
        x_of[ia[i]] = (int(g),)
    for i, g in enumerate(ids_b):
        y_of[ib[-1 - i]] = (int(g),)
    return ia, ib, x_of, y_of, id_base


def id_bytes(max_id):
    return 1 if max_id < 256 else (2 if max_id < 65536 else 4)


@pytest.mark.parametrize("name", WIDTH_LAYOUTS)
def test_width_layouts_change_the_width_they_say(name):
    ids_a, ids_b, id_base, wa, wb, wo = width_layout(name)
    ia, ib, x_of, y_of, _ = width_sets(name)
    used_a = {g for x in x_of for g in x}
    used_b = {g for y in y_of for g in y}
    assert used_a == set(ids_a.tolist()) and used_b == set(ids_b.tolist())
    assert id_bytes(max(used_a)) == wa and id_bytes(max(used_b)) == wb
    assert id_base <= max(used_a) + 1  # (at most a's genome count)
    shifted = {id_base + g for g in used_b}
    assert id_bytes(max(used_a | shifted)) == wo
    if name == "b_crosses_255":
        assert {255, 256} <= shifted and max(used_a) < 256
    if name == "b_crosses_65535":
        assert {65535, 65536} <= shifted and 65535 in used_a and max(used_a) < 65536
    if name == "a_wide_b_narrow":
        assert max(shifted) < 256 <= 65536 <= max(used_a)
    assert len(np.intersect1d(ia, ib)) > 500 and len(ia) > TILE and len(ib) > TILE
    assert len(used_a) + len(used_b) <= 50  # (one insert call per id)


# ---- the kernels, the symbols, the argument checks ------------------------------------------------------------------------------------------------
def test_union_kernels_use_no_scratch():
    """Every k_un_* kernel (every key width / id width): no scratch memory, no vector register spilled to it; and they are exactly the expected ones."""
    subprocess.check_call(["make", "-C", _lib.CSRC, "all"], stdout=subprocess.DEVNULL)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "k_un_"], capture_output=True, text=True).stdout
    seen = {}
    for line in out.splitlines()[1:]:
        if not line.strip():
            continue
        vgpr, sgpr, vspill, sspill, scratch, lds, maxwg, name = line.split(None, 7)
        m = re.search(r"(k_un_[a-z]+)", name)
        if not m:
            continue
        seen[m.group(1)] = seen.get(m.group(1), 0) + 1
        assert int(vspill) == 0 and int(scratch) == 0, line
    assert seen == {"k_un_split": 4, "k_un_count": 4, "k_un_emit": 4, "k_un_shift": 3}, seen


def test_merge_symbols_are_declared_and_exported():
    subprocess.check_call(["make", "-C", _lib.CSRC, "all"], stdout=subprocess.DEVNULL)
    hdr = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+bft_gpu_merge\s*\(\s*bft_gpu\s*\*\s*a\s*,\s*bft_gpu\s*\*\s*b\s*,\s*uint32_t\s+id_base\s*,\s*bft_gpu\s*\*\*\s*out\s*\)\s*;", hdr)
    assert "bft_gpu_merge" in _lib.SIGNATURES
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert "bft_gpu_merge" in set(re.findall(r" T (bft_gpu_[a-z_0-9]+)", out))
    compat = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bft", "merge.h")).read(), flags=re.S)
    assert re.search(r"\bvoid\s+merging_BFT\s*\(\s*char\s*\*\s*prefix_bft1\s*,\s*char\s*\*\s*prefix_bft2\s*,\s*char\s*\*\s*output_prefix\s*,\s*int\s+cut_lvl\s*,"
                     r"\s*bool\s+packed_in_subtries\s*\)\s*;", compat)
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(_lib.CSRC, "libbft.so")]).decode()
    assert re.search(r" T merging_BFT$", out, flags=re.M)


def test_append_constant_is_the_headers():
    m = re.search(r"^#define\s+BFT_GPU_MERGE_APPEND\s+(0x[0-9A-Fa-f]+)u?\s*$", open(_lib.HEADER).read(), flags=re.M)
    assert m and int(m.group(1), 16) == _lib.MERGE_APPEND == 0xFFFFFFFF


def test_null_arguments_are_refused_before_any_device_work():
    lib = _lib.load()
    out = C.c_void_p()
    one = C.c_void_p(1)
    assert lib.bft_gpu_merge(None, one, 0, C.byref(out)) == -1  # BFT_GPU_E_ARG
    assert lib.bft_gpu_merge(one, None, 0, C.byref(out)) == -1
    assert lib.bft_gpu_merge(one, one, 0, None) == -1
    assert lib.bft_gpu_merge(None, None, 0, None) == -1
    assert "NULL" in lib.bft_gpu_last_error().decode()
    assert not out.value
