"""Merging two indexes on the GPU (bft_gpu_merge, BFT.merge; csrc/bft_union.hip) against ground truth.  The truth is plain Python everywhere:
{packed k-mer bytes: sorted tuple of genome ids} over the (k-mer, genome) pairs that were inserted, b's ids shifted by id_base; the library is read
through extract(), colorset(), info() and the query calls.  The case sets -- which rows of a sorted pool go to which source, the sizes and positions
of a small side, the id layouts -- and the conditions they must hold are in tests/test_union_cases_host.py, which checks them without a GPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_union_cases_host as H  # noqa: E402

from bloomfiltertrie_amd import BFT, _lib, synth as S  # noqa: E402
from bloomfiltertrie_amd._lib import BFTError  # noqa: E402

pytestmark = pytest.mark.gpu

# (restated from tests/test_gpu_build.py: the container image of an index)
ARRAYS = ["tk", "nodes", "bfT", "ccs", "f2w", "clus", "child", "uck", "ucrow", "ccx", "f18", "fent"]
IMAGE_KS = (9, 18, 27, 31, 36, 63, 64, 126)
SETS_A = [(0,), (1,), (2,), (0, 1), (0, 2), (1, 2), (0, 1, 2)]
SETS_B = [(0,), (1,), (0, 1)]
_POOLS = {}


def _pool(k, n, seed):
    """the first n rows of one sorted pool per (k, seed) (computed once, never changed)"""
    key = (k, seed)
    if key not in _POOLS or len(_POOLS[key]) < n:
        _POOLS[key] = H.pool(k, n, seed)
        _POOLS[key].setflags(write=False)
    return _POOLS[key][:n]


def _colour_map(t):
    """{packed k-mer bytes: tuple of genome ids} of everything the handle stores, and the number of sets in use"""
    km, cs = t.extract()
    sets = {c: tuple(int(x) for x in t.colorset(c)) for c in np.unique(cs).tolist()}
    return {km[i].tobytes(): sets[int(cs[i])] for i in range(len(km))}, len(sets)


def _arrays(t):
    return {name: t.debug_array(name) for name in ARRAYS}


def _fill(t, km, id_lists):
    """insert calls genome by genome, ascending"""
    rows = {}
    for r, ids in enumerate(id_lists):
        for g in ids:
            rows.setdefault(g, []).append(r)
    for g in sorted(rows):
        t.insert_kmers(np.ascontiguousarray(km[np.array(rows[g])]), g)


def _truth(km, x_of, y_of, id_base):
    out = {}
    for r in range(len(km)):
        ids = set(x_of[r]) | {id_base + g for g in y_of[r]}
        if ids:
            out[km[r].tobytes()] = tuple(sorted(ids))
    return out


def _mismatch(got, truth):
    bad = [(kk.hex()[:16], truth.get(kk), got.get(kk)) for kk in list(truth) + [x for x in got if x not in truth] if got.get(kk) != truth.get(kk)]
    return f"{len(bad)} k-mers differ; first: {bad[:4]}"


def _check_against_truth(out, truth, genomes):
    got, n_sets = _colour_map(out)
    assert got == truth, _mismatch(got, truth)
    info = out.info()
    assert info["kmers"] == len(truth)
    assert info["pairs"] == sum(len(v) for v in truth.values())
    assert info["colorsets"] == len(set(truth.values())) == n_sets
    assert info["genomes"] == genomes
    assert info["pending_pairs"] == 0
    lists = [tuple(out.colorset(c)) for c in range(info["colorsets"])]
    assert len(set(lists)) == len(lists) and all(all(a < b for a, b in zip(ids, ids[1:])) for ids in lists)  # no list twice, every list ascending


def _same_image(x, y):
    ax, ay = _arrays(x), _arrays(y)
    for name in ARRAYS:
        assert ax[name].shape == ay[name].shape and (ax[name] == ay[name]).all(), name
    kx, cx = x.extract()
    ky, cy = y.extract()
    assert (kx == ky).all() and (cx == cy).all()
    assert x.info()["colorsets"] == y.info()["colorsets"]
    assert [x.colorset(c) for c in range(x.info()["colorsets"])] == [y.colorset(c) for c in range(y.info()["colorsets"])]


def _merge_both_ways(a, b, id_base=None):
    """(co-ranked, search): the two placements of the same merge"""
    outs = []
    for place in (1, 0):
        a.set_option("merge_place", place)
        outs.append(a.merge(b, id_base))
    a.set_option("merge_place", 1)
    return outs


def _sets_for(rng, ia, ib, n):
    x_of, y_of = [()] * n, [()] * n
    for r in ia:
        x_of[r] = SETS_A[int(rng.integers(len(SETS_A)))]
    for r in ib:
        y_of[r] = SETS_B[int(rng.integers(len(SETS_B)))]
    x_of[ia[0]] = (0, 1, 2)  # (a's genome count is 3 whatever was drawn)
    return x_of, y_of


def _run_split(k, km, ia, ib, seed):
    """a holds rows ia of the sorted pool km, b rows ib; appended: b's genomes 0, 1 become 3, 4"""
    n = len(km)
    x_of, y_of = _sets_for(np.random.default_rng(seed), ia, ib, n)
    truth = _truth(km, x_of, y_of, 3)
    a, b = BFT(k), BFT(k)
    _fill(a, km, x_of)
    _fill(b, km, y_of)
    a.build()
    b.build()
    assert a.info()["kmers"] == len(ia) and b.info()["kmers"] == len(ib) and a.info()["genomes"] == 3
    co, se = _merge_both_ways(a, b)
    for out in (co, se):
        _check_against_truth(out, truth, 3 + max(g for y in y_of for g in y) + 1)
        ek, _ = out.extract()
        assert (ek == km).all()  # the merged table's rows are the pool's, in its order
    _same_image(co, se)
    for t in (a, b, co, se):
        t.close()


# ---- 1. placement edges ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", H.EDGE_KS)
def test_placement_edges_against_ground_truth(k):
    """Stretches of one sorted pool held by a only, by b only, by both (pairs of equal keys across tile boundaries, parted and not), by a / b / both
    in turn, and stretches of one tile, one less and one more: rows, colour sets and counts are the truth's, and both placements give one image."""
    ia, ib, kinds = H.edge_split()
    _run_split(k, _pool(k, H.EDGE_ROWS, 500 + k), ia, ib, k)


@pytest.mark.parametrize("side,n_small", H.SIZE_CASES)
@pytest.mark.parametrize("k", H.EDGE_KS)
def test_small_sides_and_disjoint_ranges_against_ground_truth(k, side, n_small):
    """One side of 1, tile - 1, tile, tile + 1 k-mers against a large other side; b wholly below and wholly above a."""
    ia, ib, n = H.size_split(side, n_small)
    _run_split(k, _pool(k, H.EDGE_ROWS, 500 + k)[:n], ia, ib, 7 * k + n_small)


# ---- 2. the same image as one build ----------------------------------------------------------------------------------------------------------------
def _genomes(seed, length, n):
    """n related genomes (as tests/test_gpu_components.py draws four): an ancestor with a repeated stretch, and SNP mutants of it"""
    rng = np.random.default_rng(seed)
    anc = S.random_genome(length, seed + 1)
    a = int(rng.integers(0, length // 3))
    b = int(rng.integers(length // 2, length - 400))
    anc[b:b + 300] = anc[a:a + 300]
    return [anc] + [S.mutate(anc, 0.01, seed + 2 + g) for g in range(n - 1)]


def _kh_is_canonical(t, k):
    hostlib = C.CDLL(os.path.join(_lib.CSRC, "libbft_hosttest.so"))
    hostlib.bft_hosttest_kh_verify.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p,
                                               C.c_void_p, C.c_uint32]
    W = (2 * k + 63) // 64
    t.set_option("compact_table", 0)
    kh = np.ascontiguousarray(t.debug_array("kh", np.uint64))
    tk = np.ascontiguousarray(t.debug_array("tk", np.uint64).reshape(-1, W))
    tcol = np.ascontiguousarray(t.debug_array("tcol", np.uint32))
    ovk = np.ascontiguousarray(t.debug_array("kh_ovf_k", np.uint64))
    ovv = np.ascontiguousarray(t.debug_array("kh_ovf_v", np.uint32))
    bt = t.build_time()
    assert int(bt["kmer_hash_lines"]) > 0
    rc = hostlib.bft_hosttest_kh_verify(tk.ctypes.data, tcol.ctypes.data, len(tk), k, t.info()["colorsets"], 55, int(bt["kmer_hash_maxd"]), kh.ctypes.data,
                                        len(kh) // 8, ovk.ctypes.data, ovv.ctypes.data, int(bt["kmer_hash_overflow"]))
    assert rc == 1, rc


@pytest.mark.parametrize("k", IMAGE_KS)
def test_merge_is_the_single_build_of_all_genomes(k):
    """4 + 4 related genomes: a.merge(b) against one handle with all 8 inserted -- every array of the image bit-identical, the k-mer hash as its host
    restatement lays it out, presence / colours / branching identical over stored k-mers and SNP mutants."""
    per = [S.distinct(S.kmers_of(g, k)) for g in _genomes(40 + k, 6000, 8)]
    a, b, whole = BFT(k), BFT(k), BFT(k)
    truth = {}
    for g, km in enumerate(per):
        (a if g < 4 else b).insert_kmers(km, g % 4)
        whole.insert_kmers(km, g)
        for row in km:
            truth.setdefault(row.tobytes(), []).append(g)
    truth = {kk: tuple(v) for kk, v in truth.items()}
    whole.build()
    co, se = _merge_both_ways(a, b)
    for out in (co, se):
        _check_against_truth(out, truth, 8)
        _same_image(out, whole)
    allk = S.distinct(np.concatenate(per))
    mix = np.ascontiguousarray(np.concatenate([allk, S.snp_mutants(allk[:3000], k, k)]))
    for out in (co, se):
        assert (out.query_presence(mix) == whole.query_presence(mix)).all()
        for x, y in zip(out.query_colors(mix), whole.query_colors(mix)):
            assert (x == y).all()
        for x, y in zip(out.query_branching(mix, with_counts=True), whole.query_branching(mix, with_counts=True)):
            assert (x == y).all()
    _kh_is_canonical(co, k)
    _kh_is_canonical(se, k)
    for t in (a, b, whole, co, se):
        t.close()


# ---- 3. id_base regimes --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (27, 63))
def test_id_base_regimes(k):
    per = [S.distinct(S.kmers_of(g, k)) for g in _genomes(90 + k, 4000, 7)]
    rng = np.random.default_rng(k)

    def pairs_truth(pairs):
        t = {}
        for km, g in pairs:
            for row in km:
                t.setdefault(row.tobytes(), set()).add(g)
        return {kk: tuple(sorted(v)) for kk, v in t.items()}

    # append (None) and overlap by one: a's genome 3 and b's genome 0 are halves of one genome
    half = len(per[3]) // 2
    a, b = BFT(k), BFT(k)
    for g in range(3):
        a.insert_kmers(per[g], g)
    a.insert_kmers(per[3][:half], 3)
    b.insert_kmers(per[3][half - 50:], 0)  # (50 k-mers in both halves)
    for g in range(1, 4):
        b.insert_kmers(per[3 + g], g)
    pa = [(per[g], g) for g in range(3)] + [(per[3][:half], 3)]
    pb = [(per[3][half - 50:], 0)] + [(per[3 + g], g) for g in range(1, 4)]
    for id_base, genomes in ((None, 8), (4, 8), (3, 7)):
        base = 4 if id_base is None else id_base
        truth = pairs_truth(pa + [(km, base + g) for km, g in pb])
        co, se = _merge_both_ways(a, b, id_base)
        _check_against_truth(co, truth, genomes)
        _same_image(co, se)
        if id_base == 3:  # the shared genome's halves united: one build of the seven whole genomes
            whole = BFT(k)
            for g in range(7):
                whole.insert_kmers(per[g], g)
            whole.build()
            _same_image(co, whole)
            whole.close()
        co.close()
        se.close()
    # refused: id_base beyond a's genomes, another k
    with pytest.raises(BFTError, match="id_base"):
        a.merge(b, 5)
    other = BFT(36)
    other.insert_kmers(S.distinct(S.kmers_of(S.random_genome(500, 1), 36)), 0)
    with pytest.raises(BFTError, match="differ in k"):
        a.merge(other, 0)
    other.close()
    # a with itself: id_base 0 is a's own image; appended, every genome twice
    own, _ = _colour_map(a)
    assert own == pairs_truth(pa)
    same = a.merge(a, 0)
    _same_image(same, a)
    assert same.info()["genomes"] == 4
    twice = a.merge(a)
    _check_against_truth(twice, {kk: v + tuple(4 + g for g in v) for kk, v in own.items()}, 8)
    for t in (same, twice, a, b):
        t.close()
    # id_base 0: the pairs of every genome dealt at random to the two handles (a tenth to both); the result is the unsplit build
    a, b, whole = BFT(k), BFT(k), BFT(k)
    for g in range(4):
        where = rng.random(len(per[g]))
        a.insert_kmers(np.ascontiguousarray(per[g][where < 0.55]), g)
        b.insert_kmers(np.ascontiguousarray(per[g][where >= 0.45]), g)
        whole.insert_kmers(per[g], g)
    whole.build()
    co, se = _merge_both_ways(a, b, 0)
    _check_against_truth(co, pairs_truth([(per[g], g) for g in range(4)]), 4)
    _same_image(co, whole)
    _same_image(se, whole)
    for t in (a, b, whole, co, se):
        t.close()


# ---- 4. id widths --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", H.WIDTH_LAYOUTS)
@pytest.mark.parametrize("k", (27, 63))
def test_id_widths_against_ground_truth(k, name):
    """b's ids carried across 255 -> 256 and 65535 -> 65536 by the shift while a's stay narrow, and wide ids of a beside narrow ones of b: the resident
    dictionaries have the widths the layout says, before and after, and every list is the truth's id by id."""
    _, _, _, wa, wb, wo = H.width_layout(name)
    ia, ib, x_of, y_of, id_base = H.width_sets(name)
    km = _pool(k, H.EDGE_ROWS, 500 + k)[:H.WIDTH_ROWS]
    a, b = BFT(k), BFT(k)
    _fill(a, km, x_of)
    _fill(b, km, y_of)
    a.build()
    b.build()

    def width(t, lists):
        n_ids = sum(len(v) for v in set(lists))
        return (t.footprint()["colorset_dictionary"] - 4 * (t.info()["colorsets"] + 1)) // n_ids

    assert width(a, [x for x in x_of if x]) == wa and width(b, [y for y in y_of if y]) == wb
    truth = _truth(km, x_of, y_of, id_base)
    co, se = _merge_both_ways(a, b, id_base)
    g_a, g_b = max(g for x in x_of for g in x) + 1, max(g for y in y_of for g in y) + 1
    _check_against_truth(co, truth, max(g_a, id_base + g_b))
    _same_image(co, se)
    assert width(co, list(truth.values())) == wo
    assert width(a, [x for x in x_of if x]) == wa and width(b, [y for y in y_of if y]) == wb  # the sources keep theirs
    pick = km[::7]
    bits, off, ids = co.query_colors(pick)  # (the committed, narrowed dictionary through a query)
    assert S.from_bits(bits, len(pick)).all()
    for i in range(len(pick)):
        assert tuple(ids[int(off[i]):int(off[i + 1])].tolist()) == truth[pick[i].tobytes()], i
    for t in (a, b, co, se):
        t.close()


# ---- 5. empty sides ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("empty", ("a", "b", "both"))
def test_empty_sides(empty):
    k = 27
    km = _pool(k, H.EDGE_ROWS, 500 + k)[:1500]
    rng = np.random.default_rng(3)
    rows = np.arange(len(km))
    x_of, y_of = _sets_for(rng, rows, rows, len(km))
    a, b = BFT(k), BFT(k)
    if empty == "b":
        _fill(a, km, x_of)
    if empty == "a":
        _fill(b, km, y_of)
        for g in range(3):
            a.add_genome(f"a{g}")  # (an empty index of three named genomes: b's ids are shifted by 3)
    co, se = _merge_both_ways(a, b)
    truth = _truth(km, x_of if empty == "b" else [()] * len(km), y_of if empty == "a" else [()] * len(km), 3)
    genomes = {"a": 3 + max(g for y in y_of for g in y) + 1, "b": 3, "both": 0}[empty]
    for out in (co, se):
        _check_against_truth(out, truth, genomes)
        assert (S.from_bits(out.query_presence(km), len(km)) == (empty != "both")).all()
    _same_image(co, se)
    if empty == "a":
        assert [co.genome_name(g) for g in range(3)] == ["a0", "a1", "a2"]
    co.insert_kmers(km[:10], 0)  # an empty result is a full handle too
    co.build()
    assert S.from_bits(co.query_presence(km[:10]), 10).all()
    for t in (a, b, co, se):
        t.close()


# ---- 6. the sources stay as they are; the result stands alone ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("state", ["compact0", "kmer_hash0", "pending", "merges", "file"])
def test_sources_unchanged_and_result_independent(state, tmp_path):
    k = 36  # (a multiple of 9: the .bft format; two key words)
    per = [S.distinct(S.kmers_of(g, k)) for g in _genomes(17, 5000, 6)]
    opts = {"compact0": [("compact_table", 0)], "kmer_hash0": [("kmer_hash", 0)]}.get(state, [])
    srcs = []
    for side in range(2):
        t = BFT(k)
        for name, v in opts:
            t.set_option(name, v)
        for g in range(3):
            t.add_genome(f"s{side}g{g}")
            t.insert_kmers(per[3 * side + g], g)
            if state == "merges":
                t.build()
        t.build()
        if state == "file":
            path = str(tmp_path / f"s{side}.bft")
            t.write_bft(path)
            t.close()
            t = BFT.load_bft(path)
        srcs.append(t)
    a, b = srcs
    allk = S.distinct(np.concatenate(per))
    mix = np.ascontiguousarray(np.concatenate([allk[::3], S.snp_mutants(allk[:1500], k, 5)]))
    pairs_a = [(per[g], g) for g in range(3)]
    if state == "pending":
        extra = S.distinct(S.kmers_of(S.random_genome(900, 99), k))
        a.insert_kmers(extra, 1)
        assert a.info()["pending_pairs"] > 0
        pairs_a.append((extra, 1))
        mix = np.ascontiguousarray(np.concatenate([mix, extra]))
        ref = BFT(k)  # what a's own build of the pending pairs answers
        for km, g in pairs_a:
            ref.insert_kmers(km, g)
        before = [(ref.query_presence(mix), ref.query_colors(mix), ref.query_branching(mix, with_counts=True)), None]
        ref.close()
    else:
        before = [(a.query_presence(mix), a.query_colors(mix), a.query_branching(mix, with_counts=True)), None]
    before[1] = (b.query_presence(mix), b.query_colors(mix), b.query_branching(mix, with_counts=True))
    compact = state not in ("compact0", "kmer_hash0")
    if compact and state != "pending":
        assert a.footprint()["kmer_table"] == 0 and b.footprint()["kmer_table"] == 0  # ("compact_table": away before the call)
    out = a.merge(b)
    assert a.info()["pending_pairs"] == 0
    for t, (p, c, br) in zip((a, b), before):
        assert (t.query_presence(mix) == p).all()
        for x, y in zip(t.query_colors(mix), c):
            assert (x == y).all()
        for x, y in zip(t.query_branching(mix, with_counts=True), br):
            assert (x == y).all()
        fp = t.footprint()
        if compact:  # the sorted table came back for the call and is away again
            assert fp["kmer_table"] == 0 and fp["colorset_per_kmer"] == 0
        else:
            assert fp["kmer_table"] > 0
    truth = {}
    for km, g in pairs_a + [(per[3 + g], 3 + g) for g in range(3)]:
        for row in km:
            truth.setdefault(row.tobytes(), set()).add(g)
    truth = {kk: tuple(sorted(v)) for kk, v in truth.items()}
    a.close()
    b.close()  # (the result shares nothing with its sources)
    _check_against_truth(out, truth, 6)
    assert [out.genome_name(g) for g in range(7)] == ["s0g0", "s0g1", "s0g2", "s1g0", "s1g1", "s1g2", "genome_6"]
    more = S.distinct(S.kmers_of(S.random_genome(700, 5), k))
    out.insert_kmers(more, 6)
    out.build()
    for row in more:
        truth[row.tobytes()] = tuple(sorted(set(truth.get(row.tobytes(), ())) | {6}))
    _check_against_truth(out, truth, 7)
    path = str(tmp_path / "out.bft")
    out.write_bft(path)
    back = BFT.load_bft(path)
    _check_against_truth(back, truth, 7)
    import torch
    blob = torch.empty(out.image_size(), dtype=torch.uint8, device="cuda")
    out.image_pack(blob.data_ptr(), blob.numel())
    torch.cuda.synchronize()
    replica = BFT.from_image(blob.data_ptr(), blob.numel())
    _check_against_truth(replica, truth, 7)
    for t in (out, back, replica):
        t.close()


# ---- 7. names, timing, stages ----------------------------------------------------------------------------------------------------------------------------
def test_genome_names_in_the_append_and_overlap_cases():
    k = 27
    km = _pool(k, H.EDGE_ROWS, 500 + k)[:600]
    a, b = BFT(k), BFT(k)
    for g, name in enumerate(("x", "y", "shared")):
        a.add_genome(name)
        a.insert_kmers(km[100 * g:100 * g + 150], g)
    a.insert_kmers(km[:20], 3)  # (a fourth genome nobody named)
    for g, name in enumerate(("shared", "z")):
        b.add_genome(name)
        b.insert_kmers(km[300 + 100 * g:300 + 100 * g + 150], g)
    b.insert_kmers(km[580:], 2)  # (b's third: unnamed)
    out = a.merge(b)  # appended behind a's four
    assert out.info()["genomes"] == 7
    assert [out.genome_name(g) for g in range(8)] == ["x", "y", "shared", "genome_3", "shared", "z", "genome_6", "genome_7"]
    out.close()
    out = a.merge(b, 3)  # b's first genome is a's fourth: a's (missing) name stays, b's follow
    assert out.info()["genomes"] == 6
    assert [out.genome_name(g) for g in range(7)] == ["x", "y", "shared", "genome_3", "z", "genome_5", "genome_6"]
    out.close()
    out = a.merge(b, 2)  # b's first genome is a's "shared": every id below a's count keeps what a calls it
    assert out.info()["genomes"] == 5
    assert [out.genome_name(g) for g in range(6)] == ["x", "y", "shared", "genome_3", "genome_4", "genome_5"]
    got, _ = _colour_map(out)
    assert got[km[310].tobytes()] == (2,) and got[km[590].tobytes()] == (4,) and got[km[5].tobytes()] == (0, 3)
    for t in (out, a, b):
        t.close()


def test_kernel_timing_and_stages_follow_the_first_source():
    k = 31
    per = [S.distinct(S.kmers_of(g, k)) for g in _genomes(3, 5000, 2)]
    a, b = BFT(k), BFT(k)
    a.insert_kmers(per[0], 0)
    b.insert_kmers(per[1], 0)
    a.build()
    b.build()
    a.kernel_time(reset=True)
    a.kernel_time(reset=True)
    out = a.merge(b)
    ms, n = a.kernel_time(reset=True)
    assert n >= 5 and ms > 0  # shift, split, count, scan, emit
    assert out.build_stages() == []
    a.set_option("build_stages", 1)
    for place, word in ((1, "co-ranked"), (0, "search")):
        a.set_option("merge_place", place)
        out = a.merge(b)
        stages = out.build_stages()
        names = [st[0] for st in stages]
        placed = [st for st in stages if st[0].startswith("merge: k-mers placed")]
        assert len(placed) == 1 and word in placed[0][0] and placed[0][2] > 0, names
        assert any(nm.startswith("merge: colour sets") for nm in names) and any(nm.startswith("containers") for nm in names), names
        out.close()
    with pytest.raises(BFTError):
        a.set_option("merge_place", 2)
    a.close()
    b.close()
