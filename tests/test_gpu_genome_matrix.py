"""The genome-by-genome shared k-mer matrix on the GPU (bft_gpu_genome_matrix / _dev, bft_gpu_genome_matrix_colorsets / _dev, BFT.genome_matrix*,
BFT.genome_distances), exactly, against ground truth computed in Python from the inserted k-mers and their genome sets: a boolean N x G membership
matrix Bm and Bm.T.astype(int64) @ Bm, never from the product's own calls (extract() only tells which colour-set id a k-mer's set was given, and the
row order).

Both roads are reached by the public calls: forced ("test_genome_matrix_road" 1 sparse / 2 dense) in nearly every test, and by the cost model (0),
which takes the DENSE road on the 300 genomes of test_300_genomes_nested_and_overlapping_sets and the SPARSE road on the 1100 nearly disjoint
genomes of test_more_than_1024_genomes (both asserted through the hook bft_gpu_test_genome_matrix_state).

Tile edges: 16 (the dense road's tile; 32 = two tiles) and 127 (BFT_GM_LDS_GENOMES: the sparse road's LDS triangle), one below, at and one above
each.  The hook bft_gpu_test_genome_matrix runs a road with caller-given 32-bit weights: every 7-bit digit edge up to 2^31 - 1, mixed inside one
64-set step, whole steps of zeros (the skipped steps and digits), the accumulators flushed at every step and never."""
import ctypes as C

import numpy as np
import pytest

from bloomfiltertrie_amd import BFT, _lib, synth as S

from test_gpu_components import _owners_of

pytestmark = pytest.mark.gpu

U32 = 0xFFFFFFFF
NOSPACE, E_ARG = -6, -1
SPARSE, DENSE = 1, 2
ROADS = (0, SPARSE, DENSE)


def _pool(k, n, seed):
    km = S.distinct(S.kmers_of(S.random_genome(n + k + 64, seed), k))[:n]
    assert len(km) == n
    return km


def _from_membership(k, Bm, seed, named=True, build_each=False, options=()):
    """An index whose k-mer i (of a random pool) belongs to the genomes of row i of the boolean matrix Bm: (BFT, packed pool)"""
    km = _pool(k, Bm.shape[0], seed)
    t = BFT(k, device=0)
    for name, v in options:
        t.set_option(name, v)
    for g in range(Bm.shape[1]):
        if named:
            assert t.add_genome(f"g{g}") == g
        if Bm[:, g].any():
            t.insert_kmers(km[Bm[:, g]], g)
        if build_each:
            t.build()
    return t, km


def _truth(Bm, lo=0, hi=U32):
    """Bm.T.astype(int64) @ Bm over the k-mers carried by lo .. hi genomes.  numpy multiplies int64 matrices without BLAS (12 s at 1340 x 1040), so
    beyond 512 genomes the same product is taken in float64 and converted: every entry and every partial sum is an integer below 2^53, so it is exact."""
    cnt = Bm.sum(axis=1)
    B = Bm[(cnt >= lo) & (cnt <= hi)]
    if Bm.shape[1] > 512:
        assert len(B) < 2**53
        B = B.astype(np.float64)
        return (B.T @ B).astype(np.int64)
    return B.T.astype(np.int64) @ B.astype(np.int64)


def _state(t, canary=0):
    out = (C.c_uint32 * 2)()
    _lib.check(_lib.load().bft_gpu_test_genome_matrix_state(t._h, canary, out))
    return int(out[0]), int(out[1])


def _check(t, Bm, roads=ROADS, ranges=((0, None),)):
    """the matrix of every range on every road; returns the road the cost model took for the last range"""
    auto = None
    wants = {(lo, hi): _truth(Bm, lo, U32 if hi is None else hi) for lo, hi in ranges}
    for road in roads:
        t.set_option("test_genome_matrix_road", road)
        for lo, hi in ranges:
            got = t.genome_matrix(lo, hi)
            want = wants[(lo, hi)]
            assert got.dtype == np.uint64 and got.shape == want.shape, (road, lo, hi)
            assert np.array_equal(got.astype(np.int64), want), (road, lo, hi, np.argwhere(got.astype(np.int64) != want)[:5])
        taken = _state(t)[0]
        if road:
            assert taken == road
        else:
            auto = taken
    t.set_option("test_genome_matrix_road", 0)
    return auto


def _random_membership(n, g, p, seed):
    return np.random.default_rng(seed).random((n, g)) < p


# ---- four related genomes ---------------------------------------------------------------------------------------------------------------
def _related(k, seed, length=4000):
    rate = 0.01 if k < 63 else 0.002
    anc = S.random_genome(length, seed + 1)
    genomes = [anc] + [S.mutate(anc, rate, seed + 2 + g) for g in range(3)]
    lists = [(S.packed_to_ascii(S.distinct(S.kmers_of(g, k)), k), gid) for gid, g in enumerate(genomes)]
    owners = _owners_of(lists)
    keys = sorted(owners)
    Bm = np.zeros((len(keys), 4), dtype=bool)
    for i, x in enumerate(keys):
        Bm[i, sorted(owners[x])] = True
    t = BFT(k, device=0)
    for gid, g in enumerate(genomes):
        t.add_genome(f"g{gid}")
        t.insert_kmers(S.distinct(S.kmers_of(g, k)), gid)
    return t, Bm


@pytest.mark.parametrize("k", (27, 63))
def test_four_related_genomes_on_every_road(k):
    G = 4
    t, Bm = _related(k, seed=k)
    ranges = ((0, None), (0, G - 1), (1, 1), (G + 1, G + 5), (3, 2), (G, G), (2, 3))
    _check(t, Bm, ranges=ranges)
    spectrum, total, private = t.pangenome_stats()
    for road in ROADS:
        t.set_option("test_genome_matrix_road", road)
        m = t.genome_matrix()
        assert np.array_equal(np.diag(m), total) and np.array_equal(m, m.T)
        assert m[0, 1] > 200 and len({int(m[i, j]) for i in range(G) for j in range(i + 1, G)}) >= 4  # (no comparison is vacuous: the pairs differ)
        single = t.genome_matrix(1, 1)
        assert np.array_equal(np.diag(single), private) and not (single - np.diag(np.diag(single))).any()
        assert not t.genome_matrix(G + 1, G + 5).any() and not t.genome_matrix(3, 2).any()
        core = t.genome_matrix(G, G)
        assert (core == spectrum[G]).all()
        assert np.array_equal(t.genome_matrix(0, G - 1) + core, m)
    # the distances are numpy over that matrix
    m = t.genome_matrix().astype(np.float64)
    n = np.diag(m)
    jac = t.genome_distances("jaccard")
    assert np.allclose(jac, m / (n[:, None] + n[None, :] - m), rtol=1e-15)
    assert np.allclose(t.genome_distances("containment"), m / n[:, None], rtol=1e-15)
    mash = t.genome_distances("mash")
    assert np.allclose(mash, np.minimum(1.0, -np.log(2 * jac / (1 + jac)) / k), atol=1e-15) and (np.diag(mash) == 0).all()
    acc = t.genome_distances("jaccard", 0, G - 1)
    assert (acc[~np.eye(G, dtype=bool)] < jac[~np.eye(G, dtype=bool)]).all()  # without the core the genomes are further apart
    t.close()


# ---- hand-made indexes ------------------------------------------------------------------------------------------------------------------
def test_one_genome():
    Bm = np.ones((500, 1), dtype=bool)
    t, _ = _from_membership(27, Bm, 1)
    _check(t, Bm, ranges=((0, None), (1, 1), (0, 0)))
    assert t.genome_matrix().tolist() == [[500]]
    t.close()


def test_disjoint_genomes():
    Bm = np.zeros((900, 3), dtype=bool)
    Bm[:200, 0] = Bm[200:500, 1] = Bm[500:, 2] = True
    t, _ = _from_membership(27, Bm, 2)
    _check(t, Bm, ranges=((0, None), (1, 1), (2, 3)))
    assert t.genome_matrix().tolist() == [[200, 0, 0], [0, 300, 0], [0, 0, 400]]
    t.close()


@pytest.mark.parametrize("named_after_build", [False, True])
def test_a_genome_without_kmers_has_its_zero_row_and_column(named_after_build):
    Bm = _random_membership(600, 3, 0.5, 3)
    Bm[:, 2] = False
    t, _ = _from_membership(27, Bm[:, :2] if named_after_build else Bm, 3)
    if named_after_build:
        t.build()
        assert t.add_genome("empty") == 2
    _check(t, Bm, ranges=((0, None), (0, 2), (3, 3)))
    m = t.genome_matrix()
    assert m.shape == (3, 3) and not m[2].any() and not m[:, 2].any() and m[0, 1] > 0
    t.close()


def test_ids_inserted_without_a_name_count():
    Bm = _random_membership(300, 5, 0.4, 4)
    t, _ = _from_membership(27, Bm, 4, named=False)
    _check(t, Bm)
    t.close()


def test_empty_index():
    lib = _lib.load()
    e = BFT(27, device=0)
    g = C.c_uint32(9)
    assert lib.bft_gpu_genome_matrix(e._h, 0, U32, None, 0, C.byref(g)) == 0 and g.value == 0
    assert e.genome_matrix().shape == (0, 0) and e.genome_matrix_colorsets([]).shape == (0, 0)
    e.add_genome("named")
    for road in ROADS:
        e.set_option("test_genome_matrix_road", road)
        assert e.genome_matrix().tolist() == [[0]] and e.genome_matrix_colorsets([U32]).tolist() == [[0]]
    assert e.genome_distances("jaccard").tolist() == [[0.0]] and e.genome_distances("mash").tolist() == [[1.0]]
    e.close()


# ---- tile edges -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", (15, 16, 17, 31, 32, 33, 126, 127, 128))
def test_genome_counts_around_every_tile_edge(G):
    """16: the dense road's tile (32: two of them, 128: eight); 127: the last count whose upper triangle the sparse road keeps in LDS.  Random
    membership, so every pair of genomes has a count of its own; the last genome is in the first k-mers only, the first one in the last."""
    Bm = _random_membership(700, G, 0.3, 100 + G)
    Bm[:20, G - 1] = True
    Bm[-30:, 0] = True
    t, _ = _from_membership(27, Bm, 100 + G)
    _check(t, Bm, ranges=((0, None), (0, G // 3)))
    want = _truth(Bm)
    assert len(np.unique(want[np.triu_indices(G, 1)])) > min(40, G)  # (a transposed or shifted tile cannot go unseen)
    t.close()


def test_300_genomes_nested_and_overlapping_sets():
    """2-byte dictionary ids.  Interval sets [a, b) and nested prefix sets [0, c): the count of the pair (i, j) depends on i and on j - i, so the
    matrix is far from symmetric inside an off-diagonal tile -- a tile written transposed, or with rows and columns of the fragment swapped, fails."""
    G, N = 300, 1500
    rng = np.random.default_rng(300)
    a = rng.integers(0, G, N)
    b = np.minimum(G, a + 1 + rng.integers(0, 120, N))
    a[::3] = 0  # the nested ones
    cols = np.arange(G)[None, :]
    Bm = (cols >= a[:, None]) & (cols < b[:, None])
    t, _ = _from_membership(27, Bm, 300)
    want = _truth(Bm)
    tile = want[16:32, 64:80]
    assert not np.array_equal(tile, tile.T) and len(np.unique(want[np.triu_indices(G, 1)])) > 200
    auto = _check(t, Bm, roads=(DENSE, 0, SPARSE), ranges=((0, 100), (0, None)))
    assert auto == DENSE  # (1500 sets of 60 genomes on average: millions of pair updates against 24 digit steps over 19 x 19 tiles)
    assert np.array_equal(np.diag(t.genome_matrix()), t.pangenome_stats()[1])
    t.close()


def test_more_than_1024_genomes():
    """1100 genomes with two private k-mers each and 300 k-mers shared by two to five genomes: the sparse road's case (global 64-bit atomics, the
    cost model takes it), the dense road over 69 x 69 tiles."""
    G = 1100
    rng = np.random.default_rng(1100)
    Bm = np.zeros((2 * G + 300, G), dtype=bool)
    Bm[np.arange(2 * G), np.arange(2 * G) // 2] = True
    for i in range(300):
        Bm[2 * G + i, rng.choice(G, size=2 + i % 4, replace=False)] = True
    t, _ = _from_membership(27, Bm, 1100)
    auto = _check(t, Bm, ranges=((0, None), (2, 5)))
    assert auto == SPARSE
    t.close()


# ---- states -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("state", ["compact1", "compact0", "merges"])
def test_index_states(state):
    Bm = _random_membership(800, 6, 0.4, 7)
    opts = {"compact1": [("compact_table", 1)], "compact0": [("compact_table", 0)]}.get(state, [])
    t, km = _from_membership(27, Bm, 7, options=opts, build_each=state == "merges")
    t.build()
    if state == "compact1":
        assert S.from_bits(t.query_presence(km[Bm.any(axis=1)][:100]), 100).all()  # (answered by the k-mer hash: the table may be away when the matrix is asked for)
    _check(t, Bm, ranges=((0, None), (0, 5)))
    t.close()


def test_after_a_merge_of_two_indexes():
    Bm = _random_membership(900, 9, 0.35, 8)
    km = _pool(27, 900, 8)
    a, b = BFT(27, device=0), BFT(27, device=0)
    for g in range(9):
        t, col = (a, g) if g < 5 else (b, g - 5)
        assert t.add_genome(f"g{g}") == col
        t.insert_kmers(km[Bm[:, g]], col)
    m = a.merge(b)
    _check(m, Bm)
    _check(a, Bm[:, :5], roads=(DENSE,))
    for t in (a, b, m):
        t.close()


def test_caps():
    import torch
    lib = _lib.load()
    G = 5
    Bm = _random_membership(400, G, 0.5, 9)
    t, _ = _from_membership(27, Bm, 9)
    want = _truth(Bm)
    g = C.c_uint32(77)
    assert lib.bft_gpu_genome_matrix(t._h, 0, U32, None, 0, C.byref(g)) == 0 and g.value == G  # the size only
    buf = np.full(G * G + 3, 0xAAAAAAAAAAAAAAAA, dtype=np.uint64)
    g = C.c_uint32(77)
    assert lib.bft_gpu_genome_matrix(t._h, 0, U32, buf.ctypes.data, G * G - 1, C.byref(g)) == NOSPACE and g.value == G
    assert (buf == 0xAAAAAAAAAAAAAAAA).all()  # nothing written
    cs = np.zeros(4, dtype=np.uint32)
    g = C.c_uint32(77)
    assert lib.bft_gpu_genome_matrix_colorsets(t._h, cs.ctypes.data, 4, buf.ctypes.data, G * G - 1, C.byref(g)) == NOSPACE and g.value == G
    assert (buf == 0xAAAAAAAAAAAAAAAA).all()
    assert lib.bft_gpu_genome_matrix(t._h, 0, U32, buf.ctypes.data, G * G, C.byref(g)) == 0
    assert np.array_equal(buf[:G * G].reshape(G, G).astype(np.int64), want) and (buf[G * G:] == 0xAAAAAAAAAAAAAAAA).all()
    d = torch.full((G * G + 3,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    with pytest.raises(_lib.BFTError):
        t.genome_matrix_dev(d.data_ptr(), G * G - 1)
    with pytest.raises(_lib.BFTError):
        t.genome_matrix_colorsets_dev(d.data_ptr(), 0, d.data_ptr(), G * G - 1)
    torch.cuda.synchronize()
    assert (d.cpu().numpy() == 0x5A5A5A5A5A5A5A5A).all()
    t.genome_matrix_dev(d.data_ptr(), G * G)
    torch.cuda.synchronize()
    h = d.cpu().numpy()
    assert np.array_equal(h[:G * G].reshape(G, G), want) and (h[G * G:] == 0x5A5A5A5A5A5A5A5A).all()
    t.close()


def test_dev_form_on_a_user_stream_interleaved_with_other_queries():
    import torch
    G = 20
    Bm = _random_membership(1500, G, 0.3, 10)
    t, km = _from_membership(27, Bm, 10)
    want, acc = _truth(Bm), _truth(Bm, 0, G - 1)
    spectrum, total, private = t.pangenome_stats()
    _, cs = t.extract()
    q = np.concatenate([km[:300], S.snp_mutants(km[:100], 27, 5)])
    pres_h = t.query_presence(q)
    s = torch.cuda.Stream()
    out = []
    with torch.cuda.stream(s):
        st = s.cuda_stream
        dq = torch.from_numpy(q.reshape(-1).copy()).cuda()
        dcs = torch.from_numpy(cs.view(np.int32).copy()).cuda()
        dpres = [torch.zeros((len(q) + 63) // 64, dtype=torch.int64, device="cuda") for _ in range(2)]
        sp = [torch.full((G + 1,), 7, dtype=torch.int64, device="cuda") for _ in range(2)]
        to = torch.full((G,), 7, dtype=torch.int64, device="cuda")
        for i, road in enumerate((SPARSE, DENSE, 0)):
            t.set_option("test_genome_matrix_road", road)
            m1 = torch.full((G * G,), 7, dtype=torch.int64, device="cuda")
            m2 = torch.full((G * G,), 7, dtype=torch.int64, device="cuda")
            m3 = torch.full((G * G,), 7, dtype=torch.int64, device="cuda")
            t.genome_matrix_dev(m1.data_ptr(), G * G, stream=st)
            t.query_presence_dev(dq.data_ptr(), len(q), dpres[i % 2].data_ptr(), st)
            t.genome_matrix_dev(m2.data_ptr(), G * G, 0, G - 1, stream=st)
            t.pangenome_stats_dev(sp[i % 2].data_ptr(), to.data_ptr(), 0, G + 1, stream=st)
            t.genome_matrix_colorsets_dev(dcs.data_ptr(), len(cs), m3.data_ptr(), G * G, stream=st)
            out.append((m1, m2, m3))
    s.synchronize()
    for m1, m2, m3 in out:
        assert np.array_equal(m1.cpu().numpy().reshape(G, G), want)
        assert np.array_equal(m2.cpu().numpy().reshape(G, G), acc)
        assert np.array_equal(m3.cpu().numpy().reshape(G, G), want)
    for i in range(2):
        assert (dpres[i].cpu().numpy().view(np.uint8)[:len(pres_h)] == pres_h).all()
        assert sp[i].cpu().numpy().tolist() == spectrum.tolist()
    assert to.cpu().numpy().tolist() == total.tolist()
    # the host forms afterwards, on the handle's stream
    _check(t, Bm)
    t.close()


def test_kernel_time_and_stages():
    Bm = _random_membership(300, 6, 0.4, 11)
    t, _ = _from_membership(27, Bm, 11)
    t.build()
    t.kernel_time(reset=True)
    t.genome_matrix()
    ms, launches = t.kernel_time(reset=True)
    assert launches >= 4 and ms > 0
    t.set_option("build_stages", 1)
    t.genome_matrix()
    names = [nm for nm, _, _ in t.build_stages()]
    for part in ("rows per colour set", "weights", "sparse road", "dense road"):
        assert any(part in nm for nm in names), (part, names)
    t.close()


# ---- the colour-set form ----------------------------------------------------------------------------------------------------------------
def test_colour_set_batches():
    import torch
    lib = _lib.load()
    G, k = 12, 27
    Bm = _random_membership(1200, G, 0.3, 12)
    Bm[Bm.sum(axis=1) == 0, 0] = True
    t, km = _from_membership(k, Bm, 12)
    want = _truth(Bm)
    ekm, cs = t.extract()
    n_sets = int(cs.max()) + 1
    asc = S.packed_to_ascii(km, k)
    for road in ROADS:
        t.set_option("test_genome_matrix_road", road)
        # extract()'s ids: the whole index; duplicates count with their multiplicity; absent entries are skipped; n = 0
        assert np.array_equal(t.genome_matrix_colorsets(cs).astype(np.int64), want)
        assert np.array_equal(t.genome_matrix_colorsets(np.repeat(cs, 3)).astype(np.int64), 3 * want)
        mixed = np.concatenate([cs[:500], np.full(70, U32, dtype=np.uint32), cs[:500], np.full(1, U32, dtype=np.uint32)])
        sub = Bm[np.isin(S.row_keys(km), S.row_keys(ekm[:500]))]
        assert np.array_equal(t.genome_matrix_colorsets(mixed).astype(np.int64), 2 * _truth(sub))
        assert not t.genome_matrix_colorsets([]).any() and not t.genome_matrix_colorsets([U32, U32]).any()
        # the ids of a prefix query: the truth over the matching k-mers (two prefixes, the second twice)
        prefixes = ["AC", "GT", "GT"]
        _, _, _, pcs = t.query_prefixes(prefixes)
        match = np.array([[x.startswith(p) for x in asc] for p in prefixes])
        assert match.sum() > 100
        assert np.array_equal(t.genome_matrix_colorsets(pcs).astype(np.int64), sum(_truth(Bm[mk]) for mk in match))
    # an id past the dictionary: E_ARG on the host, nothing written; skipped by the device form, which writes nothing behind usage's logical end
    bad = np.concatenate([cs[:300], np.array([n_sets, U32 - 1, n_sets + 5], dtype=np.uint32), cs[300:]])
    buf = np.full(G * G, 0xAAAAAAAAAAAAAAAA, dtype=np.uint64)
    g = C.c_uint32()
    assert lib.bft_gpu_genome_matrix_colorsets(t._h, bad.ctypes.data, len(bad), buf.ctypes.data, G * G, C.byref(g)) == E_ARG
    assert (buf == 0xAAAAAAAAAAAAAAAA).all() and "past the dictionary" in lib.bft_gpu_last_error().decode()
    dbad = torch.from_numpy(bad.view(np.int32).copy()).cuda()
    for road in (SPARSE, DENSE):
        t.set_option("test_genome_matrix_road", road)
        assert _state(t, canary=0xC0FFEE11)[1] == 0xC0FFEE11
        d = torch.zeros(G * G, dtype=torch.int64, device="cuda")
        t.genome_matrix_colorsets_dev(dbad.data_ptr(), len(bad), d.data_ptr(), G * G)
        torch.cuda.synchronize()
        assert np.array_equal(d.cpu().numpy().reshape(G, G), want)
        assert _state(t) == (road, 0xC0FFEE11)
    t.close()


# ---- the roads with given weights (the hook) ----------------------------------------------------------------------------------------------
EDGES = (1, 127, 128, 16383, 16384, 2**21 - 1, 2**21, 2**28 - 1, 2**28, 2**31 - 1)


def _weight_patterns(n_sets):
    rng = np.random.default_rng(5)
    mixed = np.array([EDGES[i % len(EDGES)] for i in range(n_sets)], dtype=np.uint32)  # every edge inside every 64-set step
    holes = mixed.copy()
    holes[64:128] = 0   # a whole step of zeros: skipped
    holes[192:256] = 5  # a step whose upper four digits are all zero
    holes[256:320] = np.uint32(1 << 14)  # ... and one with the third digit alone
    random = rng.integers(0, 2**31, n_sets, dtype=np.int64).astype(np.uint32)
    random[rng.random(n_sets) < 0.3] = 0
    top = np.full(n_sets, 2**31 - 1, dtype=np.uint32)  # every digit at its largest in every set
    return {"mixed": mixed, "holes": holes, "random": random, "top": top}


def test_given_weights_at_every_digit_edge_and_flush_interval():
    import torch
    lib = _lib.load()
    G, k = 40, 27
    Bm = _random_membership(420, G, 0.25, 13)
    Bm[Bm.sum(axis=1) == 0, 3] = True
    t, km = _from_membership(k, Bm, 13)
    ekm, cs = t.extract()
    n_sets = int(cs.max()) + 1
    assert n_sets >= 330  # (five steps of 64 sets and a part of a sixth)
    # membership of every colour set, from Bm: the set id of a k-mer is all that is taken from the product
    row_of_key = {key: i for i, key in enumerate(S.row_keys(km).tolist())}
    Bs = np.zeros((n_sets, G), dtype=object)
    for key, c in zip(S.row_keys(ekm).tolist(), cs.tolist()):
        Bs[c] = Bm[row_of_key[key]].astype(int)
    for name, w in _weight_patterns(n_sets).items():
        want = (Bs.T * np.array([int(x) for x in w], dtype=object)).dot(Bs)  # Python integers
        assert max(int(x) for x in want.reshape(-1)) < 2**63
        dw = torch.from_numpy(w.view(np.int32).copy()).cuda()
        for road in (SPARSE, DENSE):
            for flush in ((0,) if road == SPARSE else (64, n_sets + 64, 128, 0)):
                d = torch.full((G * G + 1,), 0x5A5A5A5A, dtype=torch.int64, device="cuda")
                _lib.check(lib.bft_gpu_test_genome_matrix(t._h, dw.data_ptr(), road, flush, d.data_ptr(), G * G, None))
                torch.cuda.synchronize()
                got = d.cpu().numpy()
                assert got[G * G] == 0x5A5A5A5A
                assert [int(x) for x in got[:G * G]] == [int(x) for x in want.reshape(-1)], (name, road, flush)
                assert _state(t)[0] == road
    t.close()
