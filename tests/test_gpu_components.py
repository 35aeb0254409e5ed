"""Connected components on the GPU (bft_gpu_components / _dev, BFT.components): against ground truth computed in Python from the inserted k-mer
strings and their genome sets -- a dict and a union-find for small indexes, scipy.sparse.csgraph for large ones; the product's extract only gives
the rows that number the components.  Key widths W = 1, 2 and 4 (KS has no three-word key, k = 65..96; tests/test_gpu_graph_edges.py runs W = 3 and the other key shapes); the whole graph and sub-graphs of one, two and all ids and of an id past the last
genome; hand-made graphs (a lone k-mer, a homopolymer self-loop, a circular genome, two unrelated genomes, a bridge, an inner deletion that splits
the induced sub-graph); a 2 Mbp genome (one chain) and a dense random index; index states; argument handling and caps; the device form on a user
stream interleaved with other queries on one handle; the largest component fed back through bft_gpu_subgraph."""
import ctypes as C

import numpy as np
import pytest

from bloomfiltertrie_amd import BFT, _lib, synth as S

pytestmark = pytest.mark.gpu

KS = (9, 18, 27, 31, 36, 63, 64, 126)
N_GENOMES = 4
NONE = 0xFFFFFFFF


def _genomes(seed, length):
    """Four related genomes: an ancestor with a repeated stretch, and SNP mutants of it."""
    rng = np.random.default_rng(seed)
    anc = S.random_genome(length, seed + 1)
    a = int(rng.integers(0, length // 3))
    b = int(rng.integers(length // 2, length - 400))
    anc[b:b + 300] = anc[a:a + 300]
    return [anc] + [S.mutate(anc, 0.01, seed + 2 + g) for g in range(N_GENOMES - 1)]


def _owners_of(kmer_lists):
    owners = {}
    for asc, gid in kmer_lists:
        for s in asc:
            owners.setdefault(s, set()).add(gid)
    return owners


def _row_of(t):
    km, _ = t.extract()
    return {s: i for i, s in enumerate(S.packed_to_ascii(km, t.k))}


def _truth(owners, ids, row_of):
    """(labels per row, sizes) of include/bft_gpu.h's definition: members carry every id; edges x - x[1:]+N between members; components numbered
    by their smallest row."""
    want = set(ids)
    members = [x for x in owners if want <= owners[x]]
    parent = {x: x for x in members}

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for x in members:
        for c in "ACGT":
            y = x[1:] + c
            if y != x and y in parent:
                a, b = find(x), find(y)
                if a != b:
                    parent[a] = b
    first = {}
    for x in members:
        r = find(x)
        first[r] = min(first.get(r, len(row_of)), row_of[x])
    order = {r: i for i, r in enumerate(sorted(first, key=first.get))}
    labels = np.full(len(row_of), NONE, dtype=np.uint32)
    sizes = np.zeros(len(order), dtype=np.uint64)
    for x in members:
        c = order[find(x)]
        labels[row_of[x]] = c
        sizes[c] += 1
    return labels, sizes


def _index(k, seed=0, length=6000, options=(), merges=False):
    t = BFT(k, device=0)
    for name, v in options:
        t.set_option(name, v)
    lists = []
    for gid, g in enumerate(_genomes(seed, length)):
        assert t.add_genome(f"g{gid}") == gid
        km = S.distinct(S.kmers_of(g, k))
        t.insert_kmers(km, gid)
        if merges:
            t.build()
        lists.append((S.packed_to_ascii(km, k), gid))
    return t, _owners_of(lists)


def _counts(t, ids=()):
    ids = np.ascontiguousarray(ids, dtype=np.uint32)
    cnt = np.zeros(3, dtype=np.uint64)
    rc = _lib.load().bft_gpu_components(t._h, ids.ctypes.data if len(ids) else None, len(ids), None, 0, None, 0, cnt.ctypes.data)
    return rc, [int(v) for v in cnt]


def _check(t, ids, want):
    labels, sizes = t.components(ids)
    wl, ws = want
    assert (labels == wl).all(), (ids, int((labels != wl).sum()))
    assert sizes.tolist() == ws.tolist(), ids
    rc, cnt = _counts(t, ids)
    assert rc == 0 and cnt == [len(ws), int((wl != NONE).sum()), int(ws.max()) if len(ws) else 0], (ids, cnt)


@pytest.mark.parametrize("k", KS)
def test_components_match_ground_truth(k):
    t, owners = _index(k, seed=k)
    row_of = _row_of(t)
    for ids in ((), (0,), (1, 3), tuple(range(N_GENOMES)), (N_GENOMES,), (2, N_GENOMES + 5)):
        _check(t, ids, _truth(owners, ids, row_of))
    assert _counts(t, (N_GENOMES,))[1] == [0, 0, 0]
    t.close()


def test_more_ids_than_one_membership_launch():
    """More requested ids than one k_cc_sets launch carries (64): the launches AND their answers.  150 close variants of one ancestor, so that
    many k-mers carry 100 ids or more; an id missing from the first, the second or the third launch's share changes the answer."""
    k = 27
    anc = S.random_genome(3000, 61)
    t = BFT(k, device=0)
    lists = []
    for gid in range(150):
        km = S.distinct(S.kmers_of(S.mutate(anc, 0.001, 700 + gid), k))
        t.insert_kmers(km, gid)
        lists.append((S.packed_to_ascii(km, k), gid))
    owners = _owners_of(lists)
    row_of = _row_of(t)
    for ids in (tuple(range(64)), tuple(range(65)), tuple(range(100)), tuple(range(150)), tuple(range(0, 150, 2)),
                tuple(range(63)) + (149,), tuple(range(129)) + (150,)):
        want = _truth(owners, ids, row_of)
        _check(t, ids, want)
    assert _counts(t, tuple(range(129)) + (150,))[1] == [0, 0, 0]
    assert _counts(t, tuple(range(100)))[1][1] > 0
    t.close()


def _ascii_index(k, genomes):
    """genomes: lists of ASCII k-mers, one per genome id"""
    t = BFT(k, device=0)
    for gid, kms in enumerate(genomes):
        t.add_genome(f"g{gid}")
        t.insert_kmers(S.ascii_to_packed(sorted(set(kms)), k)[0], gid)
    return t, _owners_of([(kms, gid) for gid, kms in enumerate(genomes)])


def _kmers(seq, k):
    return [seq[i:i + k] for i in range(len(seq) - k + 1)]


@pytest.mark.parametrize("k", (9, 27, 36, 63))
def test_hand_made_graphs(k):
    rng = np.random.default_rng(200 + k)
    rnd = lambda n: "".join(rng.choice(list("ACGT"), n))
    lone = rnd(k)
    t, owners = _ascii_index(k, [[lone]])
    assert t.components()[1].tolist() == [1] and _counts(t)[1] == [1, 1, 1]
    t.close()
    homo = "A" * k  # (its own successor and predecessor: a self-loop, one vertex)
    t, owners = _ascii_index(k, [[homo]])
    assert t.components()[1].tolist() == [1]
    t.close()
    circ = rnd(200)
    ring = _kmers(circ + circ[:k - 1], k)
    t, owners = _ascii_index(k, [ring])
    m = len(set(ring))
    assert _counts(t)[1] == [1, m, m]
    t.close()
    # two unrelated genomes: two components; a third genome that overlaps the end of the first and the start of the second: one
    a, b = rnd(300), rnd(300)
    bridge = a[-(k + 20):] + b[:k + 20]
    t, owners = _ascii_index(k, [_kmers(a, k), _kmers(b, k)])
    row_of = _row_of(t)
    _check(t, (), _truth(owners, (), row_of))
    if k >= 27:  # (at k = 9, two random genomes may share a k-mer)
        assert _counts(t)[1][0] == 2
    t.close()
    t, owners = _ascii_index(k, [_kmers(a, k), _kmers(b, k), _kmers(bridge, k)])
    row_of = _row_of(t)
    _check(t, (), _truth(owners, (), row_of))
    assert _counts(t)[1][0] == 1
    _check(t, (2,), _truth(owners, (2,), row_of))
    t.close()
    # a genome and a copy with an inner deletion: the whole graph is one piece, the induced sub-graph {0, 1} two
    g = rnd(600)
    cut = g[:250] + g[350:]
    t, owners = _ascii_index(k, [_kmers(g, k), _kmers(cut, k)])
    row_of = _row_of(t)
    assert _counts(t)[1][0] == 1
    if k >= 27:
        assert _counts(t, (0, 1))[1][0] == 2
    for ids in ((), (0,), (1,), (0, 1)):
        _check(t, ids, _truth(owners, ids, row_of))
    t.close()


def _codes(packed, k):
    """k-mers (k <= 31) as integers, first nucleotide most significant"""
    c = S.unpack_codes(packed, k).astype(np.uint64)
    v = np.zeros(len(c), dtype=np.uint64)
    for j in range(k):
        v = (v << np.uint64(2)) | c[:, j]
    return v


def _scipy_truth(t, member=None):
    """labels and sizes from scipy over the extract's rows (member: bool per row, None = all)"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    k = t.k
    km, _ = t.extract()
    v = _codes(km, k)
    n = len(v)
    order = np.argsort(v)
    sv = v[order]
    mask = np.uint64((1 << (2 * k)) - 1)
    us, ws = [], []
    for c in range(4):
        y = ((v << np.uint64(2)) & mask) | np.uint64(c)
        pos = np.searchsorted(sv, y)
        pos[pos == n] = 0
        hit = (sv[pos] == y)
        u = np.nonzero(hit)[0]
        w = order[pos[hit]]
        keep = u != w
        us.append(u[keep])
        ws.append(w[keep])
    u, w = np.concatenate(us), np.concatenate(ws)
    if member is not None:
        keep = member[u] & member[w]
        u, w = u[keep], w[keep]
    g = coo_matrix((np.ones(len(u), dtype=np.int8), (u, w)), shape=(n, n))
    _, lab = connected_components(g, directed=True, connection="weak")
    rows = np.arange(n) if member is None else np.nonzero(member)[0]
    first = np.full(lab.max() + 1, n, dtype=np.int64)
    np.minimum.at(first, lab[rows], rows)
    used = np.unique(lab[rows])
    rank = np.full(lab.max() + 1, NONE, dtype=np.int64)
    rank[used[np.argsort(first[used])]] = np.arange(len(used))
    labels = np.full(n, NONE, dtype=np.uint32)
    labels[rows] = rank[lab[rows]]
    sizes = np.bincount(labels[rows], minlength=len(used)).astype(np.uint64)
    return labels, sizes


def test_one_long_chain():
    """One 2 Mbp genome: about 2x10^6 k-mers in one chain whose rows are scattered (depth of the trees, termination)."""
    k = 31
    g = S.random_genome(2_000_000, 71)
    t = BFT(k, device=0)
    t.insert_kmers(S.distinct(S.kmers_of(g, k)), 0)
    labels, sizes = t.components()
    wl, ws = _scipy_truth(t)
    assert (labels == wl).all() and sizes.tolist() == ws.tolist()
    assert sizes[0] > 1_900_000
    labels2, sizes2 = t.components()
    assert (labels2 == labels).all() and (sizes2 == sizes).all()
    t.close()


def test_dense_random_index():
    """Three million random 11-mers (most of the 4^11): one giant component, many small ones; genome 0 holds a random half."""
    k = 11
    rng = np.random.default_rng(5)
    km = S.distinct(S.pack_codes(rng.integers(0, 4, (3_000_000, k), dtype=np.uint8)))
    half = km[rng.random(len(km)) < 0.5]
    t = BFT(k, device=0)
    t.insert_kmers(half, 0)
    t.insert_kmers(km, 1)
    labels, sizes = t.components()
    wl, ws = _scipy_truth(t)
    assert (labels == wl).all() and sizes.tolist() == ws.tolist()
    km_rows, _ = t.extract()
    member = S.member(km_rows, half)
    labels, sizes = t.components((0,))
    wl, ws = _scipy_truth(t, member)
    assert (labels == wl).all() and sizes.tolist() == ws.tolist()
    t.close()


@pytest.mark.parametrize("state", ["compact0", "kmer_hash0", "pending", "merges", "file"])
@pytest.mark.parametrize("k", (27, 63))
def test_index_states_give_the_same_components(state, k, tmp_path):
    ref, owners = _index(k, seed=7)
    row_of = _row_of(ref)
    want = {ids: _truth(owners, ids, row_of) for ids in ((), (0, 2))}
    opts = {"compact0": [("compact_table", 0)], "kmer_hash0": [("kmer_hash", 0)]}.get(state, [])
    if state == "file":
        path = str(tmp_path / "i.bft")
        ref.write_bft(path)
        t = BFT.load_bft(path)
    elif state == "pending":
        t, _ = _index(k, seed=7)
        t.components()
        extra = S.distinct(S.kmers_of(S.random_genome(800, 99), k))
        t.insert_kmers(extra, 0)  # (pending: built by the next call)
        owners2 = {key: set(v) for key, v in owners.items()}
        for s in S.packed_to_ascii(extra, k):
            owners2.setdefault(s, set()).add(0)
        _check(t, (), _truth(owners2, (), _row_of(t)))
        t.close()
        ref.close()
        return
    else:
        t, _ = _index(k, seed=7, options=opts, merges=state == "merges")
    for ids, w in want.items():
        _check(t, ids, w)
        a = t.components(ids)
        b = t.components(ids)
        assert (a[0] == b[0]).all() and (a[1] == b[1]).all()
    t.close()
    ref.close()


def test_arguments_caps_and_empty_index():
    k = 27
    t, owners = _index(k, seed=11)
    lib = _lib.load()
    rc, (nc, nm, big) = _counts(t)  # (builds the pending insertions)
    n = int(t.info()["kmers"])
    assert rc == 0 and nm == n
    for bad in ((1, 1), (2, 1), (3, 0, 1)):
        ids = np.array(bad, dtype=np.uint32)
        cnt = np.zeros(3, dtype=np.uint64)
        assert lib.bft_gpu_components(t._h, ids.ctypes.data, len(ids), None, 0, None, 0, cnt.ctypes.data) == -1
        assert lib.bft_gpu_components_dev(t._h, ids.ctypes.data, len(ids), None, None, 0, cnt.ctypes.data, None) == -1
    lab = np.full(n, 7, dtype=np.uint32)
    sz = np.full(nc, 7, dtype=np.uint64)
    cnt = np.zeros(3, dtype=np.uint64)
    assert lib.bft_gpu_components(t._h, None, 0, lab.ctypes.data, n - 1, sz.ctypes.data, nc, cnt.ctypes.data) == -6  # BFT_GPU_E_NOSPACE
    assert cnt.tolist() == [nc, nm, big] and (lab == 7).all() and (sz == 7).all()
    assert lib.bft_gpu_components(t._h, None, 0, lab.ctypes.data, n, sz.ctypes.data, nc - 1, cnt.ctypes.data) == -6
    assert (lab == 7).all() and (sz == 7).all()
    assert lib.bft_gpu_components(t._h, None, 0, lab.ctypes.data, n, None, 0, cnt.ctypes.data) == 0
    wl, ws = _truth(owners, (), _row_of(t))
    assert (lab == wl).all()
    assert lib.bft_gpu_components(t._h, None, 0, None, 0, sz.ctypes.data, nc, cnt.ctypes.data) == 0
    assert sz.tolist() == ws.tolist()
    e = BFT(27, device=0)
    assert _counts(e) == (0, [0, 0, 0])
    assert _counts(e, (0, 1)) == (0, [0, 0, 0])
    labels, sizes = e.components()
    assert len(labels) == 0 and len(sizes) == 0
    e.close()
    t.close()


def test_dev_form_on_a_user_stream_interleaved_with_queries():
    import torch
    k = 36
    t, owners = _index(k, seed=5)
    row_of = _row_of(t)
    n = len(row_of)
    w_all = _truth(owners, (), row_of)
    w_sub = _truth(owners, (1, 2), row_of)
    paths = t.simple_paths()
    asc = sorted(owners)[::5]
    q, _ = S.ascii_to_packed(asc, k)
    bits_h, off_h, ids_h = t.query_colors(q)
    pref = q[:64].copy()
    po, _, _, _ = t.query_prefixes(pref, np.full(64, 20, dtype=np.uint8))
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        dq = torch.from_numpy(q.reshape(-1).copy()).cuda()
        dbits = torch.zeros((len(q) + 63) // 64, dtype=torch.int64, device="cuda")
        doffc = torch.zeros(len(q) + 1, dtype=torch.int64, device="cuda")
        dids = torch.zeros(len(ids_h) + 1, dtype=torch.int32, device="cuda")
        dp = torch.from_numpy(pref.reshape(-1).copy()).cuda()
        dl = torch.full((64,), 20, dtype=torch.uint8, device="cuda")
        dpo = torch.zeros(65, dtype=torch.int64, device="cuda")
        lab = torch.full((n,), 7, dtype=torch.int32, device="cuda")
        lab2 = torch.full((n,), 7, dtype=torch.int32, device="cuda")
        nc = len(w_all[1])
        sz = torch.full((nc,), 7, dtype=torch.int64, device="cuda")
        sz_half = torch.full((nc,), 7, dtype=torch.int64, device="cuda")
        c1 = torch.full((3,), 7, dtype=torch.int64, device="cuda")
        c2 = torch.full((3,), 7, dtype=torch.int64, device="cuda")
        c3 = torch.full((3,), 7, dtype=torch.int64, device="cuda")
        pc = torch.zeros(3, dtype=torch.int64, device="cuda")
        t.components_dev(lab.data_ptr(), sz.data_ptr(), nc, c1.data_ptr(), stream=s.cuda_stream)
        t.query_colors_dev(dq.data_ptr(), len(q), dbits.data_ptr(), doffc.data_ptr(), dids.data_ptr(), len(ids_h) + 1, stream=s.cuda_stream)
        t.simple_paths_dev(0, 0, 0, 0, pc.data_ptr(), stream=s.cuda_stream)
        t.components_dev(lab2.data_ptr(), 0, 0, c2.data_ptr(), genome_ids=(1, 2), stream=s.cuda_stream)
        t.query_prefixes_dev(dp.data_ptr(), dl.data_ptr(), 64, dpo.data_ptr(), 0, 0, 0, 0, 0, stream=s.cuda_stream)
        t.components_dev(0, sz_half.data_ptr(), nc // 2, c3.data_ptr(), stream=s.cuda_stream)
    s.synchronize()
    wl, ws = w_all
    assert (lab.cpu().numpy().view(np.uint32) == wl).all()
    assert sz.cpu().numpy().astype(np.uint64).tolist() == ws.tolist()
    assert c1.cpu().tolist() == [nc, n, int(ws.max())]
    assert c3.cpu().tolist() == [nc, n, int(ws.max())]
    h = sz_half.cpu().numpy()
    assert h[:nc // 2].tolist() == ws[:nc // 2].tolist() and (h[nc // 2:] == 7).all()
    sl, ss = w_sub
    assert (lab2.cpu().numpy().view(np.uint32) == sl).all()
    assert c2.cpu().tolist() == [len(ss), int((sl != NONE).sum()), int(ss.max())]
    assert pc.cpu().tolist()[0] == len(paths)
    assert (dbits.cpu().numpy().view(np.uint8)[:len(bits_h)] == bits_h).all()
    assert (doffc.cpu().numpy().astype(np.uint64) == off_h).all()
    assert (dids.cpu().numpy()[:len(ids_h)].astype(np.uint32) == ids_h).all()
    assert (dpo.cpu().numpy().astype(np.uint64) == po).all()
    assert t.query_colors(q)[0].tobytes() == bits_h.tobytes()
    assert t.simple_paths() == paths
    t.close()


def test_largest_component_through_subgraph():
    k = 27
    a, b = S.random_genome(5000, 901), S.random_genome(2000, 902)
    t = BFT(k, device=0)
    t.insert_kmers(S.distinct(S.kmers_of(a, k)), 0)
    t.insert_kmers(S.distinct(S.kmers_of(b, k)), 1)
    labels, sizes = t.components()
    assert len(sizes) == 2
    big = int(np.argmax(sizes))
    km, _ = t.extract()
    sub, absent = t.subgraph(km[labels == big])
    assert absent == 0
    l2, s2 = sub.components()
    assert s2.tolist() == [int(sizes[big])] and (l2 == 0).all()
    sub.close()
    t.close()


def test_kernel_time_counts_the_launches():
    t, _ = _index(27, seed=2)
    t.kernel_time(reset=True)
    t.components()
    ms, launches = t.kernel_time(reset=True)
    assert launches >= 8 and ms > 0
    t.close()
