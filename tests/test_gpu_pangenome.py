"""Pan-genome k-mer classes on the GPU (bft_gpu_kmers_by_count / _dev, bft_gpu_pangenome_stats / _dev, BFT.kmers_by_count, BFT.pangenome_stats): against
ground truth computed in Python from the inserted k-mer strings and their genome sets; the product's extract() only gives the row order.  Every
comparison is over all k-mers of the index.  Key widths W = 1, 2 and 4 (KS has no three-word key, k = 65..96; tests/test_gpu_graph_edges.py runs W = 3 and the other key shapes); the classes core, dispensable, singleton and other ranges, empty ones included; packed
k-mers, ASCII with its NULs and stride, rows; the statistics; hand-made indexes (one genome, disjoint genomes, a genome without k-mers, 300 genomes
with 2-byte dictionary ids, more genomes than the dictionary pass keeps counters for in LDS, one colour set owning over 90 % of a few million rows,
the empty index); index states; caps; the device forms on a user stream interleaved with other queries on one handle; a class fed back through
bft_gpu_subgraph."""
import ctypes as C

import numpy as np
import pytest

from bloomfiltertrie_amd import BFT, _lib, synth as S

from test_gpu_components import _owners_of, _row_of

pytestmark = pytest.mark.gpu

KS = (9, 18, 27, 31, 36, 63, 64, 126)
G = 4
U32 = 0xFFFFFFFF
NOSPACE = -6


def _genomes(k, seed, length=6000):
    """Four related genomes: an ancestor and SNP mutants of it.  With 1 % SNPs a 126-mer survives in all three mutants with probability 0.02, so the
    rate falls for long k-mers: (1 - 0.002)^(3 * 126) = 0.47 of the ancestor's k-mers stay core."""
    rate = 0.01 if k < 63 else 0.002
    anc = S.random_genome(length, seed + 1)
    return [anc] + [S.mutate(anc, rate, seed + 2 + g) for g in range(G - 1)]


def _index(k, seed=0, options=(), merges=False):
    t = BFT(k, device=0)
    for name, v in options:
        t.set_option(name, v)
    lists = []
    for gid, g in enumerate(_genomes(k, seed)):
        assert t.add_genome(f"g{gid}") == gid
        km = S.distinct(S.kmers_of(g, k))
        t.insert_kmers(km, gid)
        if merges:
            t.build()
        lists.append((S.packed_to_ascii(km, k), gid))
    return t, _owners_of(lists)


def _class(owners, row_of, lo, hi):
    """the k-mers carried by lo .. hi genomes, in row order: (strings, rows)"""
    sel = sorted((row_of[x], x) for x, o in owners.items() if lo <= len(o) <= hi)
    return [x for _, x in sel], np.array([r for r, _ in sel], dtype=np.uint32)


def _stats(owners, genomes):
    spectrum = np.zeros(genomes + 1, dtype=np.uint64)
    total = np.zeros(genomes, dtype=np.uint64)
    private = np.zeros(genomes, dtype=np.uint64)
    for o in owners.values():
        spectrum[len(o)] += 1
        for g in o:
            total[g] += 1
        if len(o) == 1:
            private[next(iter(o))] += 1
    return spectrum, total, private


def _raw(t, lo, hi, cap=None):
    """bft_gpu_kmers_by_count with all three outputs over canaries: (rc, n, packed, ascii bytes [cap, k + 1], rows)"""
    lib = _lib.load()
    n = C.c_uint64()
    assert lib.bft_gpu_kmers_by_count(t._h, lo, hi, None, None, None, 0, C.byref(n)) == 0
    m = int(n.value) if cap is None else cap
    km = np.full((m, t.nb), 0xAA, dtype=np.uint8)
    asc = np.full((m, t.k + 1), 0xAA, dtype=np.uint8)
    rows = np.full(m, 0xAAAAAAAA, dtype=np.uint32)
    rc = lib.bft_gpu_kmers_by_count(t._h, lo, hi, km.ctypes.data, asc.ctypes.data, rows.ctypes.data, m, C.byref(n))
    return rc, int(n.value), km, asc, rows


def _check_class(t, owners, row_of, lo, hi):
    want, wrows = _class(owners, row_of, lo, hi)
    rc, n, km, asc, rows = _raw(t, lo, hi)
    assert rc == 0 and n == len(want), (lo, hi, n, len(want))
    assert rows.tolist() == wrows.tolist(), (lo, hi)
    assert S.packed_to_ascii(km, t.k) == want, (lo, hi)
    # k characters and the NUL per k-mer, nothing between two k-mers
    assert (asc[:, t.k] == 0).all()
    assert [r.tobytes().decode() for r in asc[:, :t.k]] == want, (lo, hi)
    packed, prow = t.kmers_by_count(lo, hi)
    assert packed.tobytes() == km.tobytes() and prow.tolist() == wrows.tolist()
    strs, _ = t.kmers_by_count(lo, hi, ascii=True)
    assert strs == want
    return len(want)


def _check_stats(t, owners, genomes):
    spectrum, total, private = t.pangenome_stats()
    ws, wt, wp = _stats(owners, genomes)
    assert spectrum.tolist() == ws.tolist()
    assert total.tolist() == wt.tolist()
    assert private.tolist() == wp.tolist()
    assert int(spectrum.sum()) == int(t.info()["kmers"]) == len(owners)
    assert int(spectrum[1]) == int(private.sum())
    assert spectrum[0] == 0


@pytest.mark.parametrize("k", KS)
def test_classes_and_statistics_match_ground_truth(k):
    t, owners = _index(k, seed=k)
    row_of = _row_of(t)
    n_core = _check_class(t, owners, row_of, G, G)
    n_disp = _check_class(t, owners, row_of, 0, G - 1)
    n_single = _check_class(t, owners, row_of, 1, 1)
    assert n_core >= 200 and n_disp >= 200 and n_single >= 200, (n_core, n_disp, n_single)  # (no comparison is vacuous)
    assert n_core + n_disp == len(owners)
    assert _check_class(t, owners, row_of, 2, 3) > 0
    assert _check_class(t, owners, row_of, 0, U32) == len(owners)
    assert _check_class(t, owners, row_of, 3, 2) == 0
    assert _check_class(t, owners, row_of, G + 1, G + 5) == 0
    _check_stats(t, owners, G)
    lists = _genomes(k, k)
    _, total, _ = t.pangenome_stats()
    assert total.tolist() == [len(S.distinct(S.kmers_of(g, k))) for g in lists]
    t.close()


def _ascii_index(k, genomes, names=None):
    """genomes: lists of ASCII k-mers, one per genome id (an empty list: the genome is only named)"""
    t = BFT(k, device=0)
    for gid, kms in enumerate(genomes):
        t.add_genome(f"g{gid}")
        if kms:
            t.insert_kmers(S.ascii_to_packed(sorted(set(kms)), k)[0], gid)
    return t, _owners_of([(kms, gid) for gid, kms in enumerate(genomes)])


def _kmers(genome, k):
    return S.packed_to_ascii(S.distinct(S.kmers_of(genome, k)), k)


def test_one_genome():
    k = 27
    t, owners = _ascii_index(k, [_kmers(S.random_genome(3000, 1), k)])
    row_of = _row_of(t)
    n = len(owners)
    assert _check_class(t, owners, row_of, 1, 1) == n  # core = singleton = everything
    assert _check_class(t, owners, row_of, 0, 0) == 0  # dispensable
    _check_stats(t, owners, 1)
    t.close()


def test_two_disjoint_genomes_have_no_core():
    k = 31
    t, owners = _ascii_index(k, [_kmers(S.random_genome(3000, 2), k), _kmers(S.random_genome(2000, 3), k)])
    row_of = _row_of(t)
    assert _check_class(t, owners, row_of, 2, 2) == 0
    assert _check_class(t, owners, row_of, 0, 1) == len(owners)
    assert _check_class(t, owners, row_of, 1, 1) == len(owners)
    _check_stats(t, owners, 2)
    t.close()


@pytest.mark.parametrize("named_after_build", [False, True])
def test_a_genome_without_kmers_counts(named_after_build):
    """Three genomes added, the last one without k-mers (named before or after the index was built): nothing is core, the two-genome k-mers are
    dispensable, genome_total of the empty genome is 0."""
    k = 27
    anc = S.random_genome(3000, 4)
    lists = [_kmers(anc, k), _kmers(S.mutate(anc, 0.01, 5), k)]
    t, owners = _ascii_index(k, lists if named_after_build else lists + [[]])
    if named_after_build:
        t.build()
        assert t.add_genome("empty") == 2
    row_of = _row_of(t)
    assert _check_class(t, owners, row_of, 3, 3) == 0
    assert _check_class(t, owners, row_of, 0, 2) == len(owners)
    assert _check_class(t, owners, row_of, 2, 2) > 0
    _check_stats(t, owners, 3)
    assert t.pangenome_stats()[1][2] == 0
    t.close()


def _variants(k, n_genomes, length, rate, seed):
    anc = S.random_genome(length, seed)
    t = BFT(k, device=0)
    lists = []
    for gid in range(n_genomes):
        km = S.distinct(S.kmers_of(S.mutate(anc, rate, seed + 1 + gid), k))
        t.insert_kmers(km, gid)
        lists.append((S.packed_to_ascii(km, k), gid))
    return t, _owners_of(lists)


def test_300_genomes_two_byte_ids():
    """Genome ids beyond 255: the dictionary stores 2-byte ids where the other indexes of this file store 1-byte ones."""
    k, n_g = 27, 300
    t, owners = _variants(k, n_g, 2000, 0.0001, 800)
    row_of = _row_of(t)
    assert _check_class(t, owners, row_of, n_g, n_g) > 0
    assert _check_class(t, owners, row_of, 0, n_g - 1) > 0
    assert _check_class(t, owners, row_of, 1, 1) > 0
    assert _check_class(t, owners, row_of, 256, 299) > 0
    _check_stats(t, owners, n_g)
    t.close()


def test_more_genomes_than_lds_counters():
    """4200 genomes: beyond the 4095 whose counters the dictionary pass keeps in LDS (the form with atomics straight to memory)."""
    k, n_g = 27, 4200
    t, owners = _variants(k, n_g, 300, 0.004, 900)
    row_of = _row_of(t)
    assert _check_class(t, owners, row_of, 1, 1) > 0
    assert _check_class(t, owners, row_of, 3500, n_g) > 0
    _check_stats(t, owners, n_g)
    t.close()


def test_one_hot_colour_set_over_millions_of_rows():
    """Over 90 % of 3 million rows share one colour set (the core set of two genomes): the usage counters' hot case.  Truth from the inserted
    arrays (numpy set membership), the extract only ordering it."""
    k = 27
    base = S.distinct(S.kmers_of(S.random_genome(3_000_000, 31), k))
    only0 = S.distinct(S.kmers_of(S.random_genome(100_000, 32), k))
    only1 = S.distinct(S.kmers_of(S.random_genome(150_000, 33), k))
    t = BFT(k, device=0)
    t.add_genome("a")
    t.add_genome("b")
    t.insert_kmers(np.concatenate([base, only0]), 0)
    t.insert_kmers(np.concatenate([base, only1]), 1)
    km, _ = t.extract()
    in0 = S.member(km, np.concatenate([base, only0]))
    in1 = S.member(km, np.concatenate([base, only1]))
    count = in0.astype(np.int64) + in1
    assert (count >= 1).all() and (count == 2).mean() >= 0.9 and len(km) >= 3_000_000
    for lo, hi in ((2, 2), (0, 1), (1, 1)):
        mask = (count >= lo) & (count <= hi)
        packed, rows = t.kmers_by_count(lo, hi)
        assert rows.tolist() == np.flatnonzero(mask).tolist()
        assert packed.tobytes() == km[mask].tobytes()
    spectrum, total, private = t.pangenome_stats()
    assert spectrum.tolist() == [0, int((count == 1).sum()), int((count == 2).sum())]
    assert total.tolist() == [int(in0.sum()), int(in1.sum())]
    assert private.tolist() == [int((in0 & ~in1).sum()), int((in1 & ~in0).sum())]
    t.close()


def test_empty_index():
    lib = _lib.load()
    e = BFT(27, device=0)
    n = C.c_uint64(5)
    assert lib.bft_gpu_kmers_by_count(e._h, 0, U32, None, None, None, 0, C.byref(n)) == 0 and n.value == 0
    packed, rows = e.kmers_by_count(1, 1)
    assert packed.shape == (0, e.nb) and len(rows) == 0
    spectrum, total, private = e.pangenome_stats()
    assert spectrum.tolist() == [0] and len(total) == 0 and len(private) == 0
    e.add_genome("named")
    spectrum, total, private = e.pangenome_stats()
    assert spectrum.tolist() == [0, 0] and total.tolist() == [0] and private.tolist() == [0]
    e.close()


@pytest.mark.parametrize("state", ["merges", "compact1", "file", "image", "kmer_hash0"])
@pytest.mark.parametrize("k", (27, 63))
def test_index_states_give_the_same_classes(state, k, tmp_path):
    import torch
    ref, owners = _index(k, seed=7)
    opts = {"compact1": [("compact_table", 1)], "kmer_hash0": [("kmer_hash", 0)]}.get(state, [])
    if state == "file":
        path = str(tmp_path / "i.bft")
        ref.write_bft(path)
        t = BFT.load_bft(path)
    elif state == "image":
        nbytes = ref.image_size()
        blob = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        ref.image_pack(blob.data_ptr(), nbytes)
        t = BFT.from_image(blob.data_ptr(), nbytes, device=0)
    else:
        t, _ = _index(k, seed=7, options=opts, merges=state == "merges")
    if state == "compact1":
        t.build()
        q = S.ascii_to_packed(sorted(owners)[:100], k)[0]
        assert S.from_bits(t.query_presence(q), 100).all()  # (answered by the k-mer hash: the table may be away when the class is asked for)
    row_of = _row_of(t) if state != "compact1" else _row_of(ref)
    for lo, hi in ((G, G), (0, G - 1), (1, 1)):
        assert _check_class(t, owners, row_of, lo, hi) > 0
    _check_stats(t, owners, G)
    t.close()
    ref.close()


def test_pending_insertions_are_merged_first():
    k = 27
    t, owners = _index(k, seed=9)
    t.kmers_by_count(1, 1)
    extra = S.distinct(S.kmers_of(S.random_genome(800, 99), k))
    t.insert_kmers(extra, 2)  # (pending: built by the next call)
    owners2 = {key: set(v) for key, v in owners.items()}
    for s in S.packed_to_ascii(extra, k):
        owners2.setdefault(s, set()).add(2)
    rc, n, _, _, _ = _raw(t, 1, 1)
    assert rc == 0 and n == sum(1 for o in owners2.values() if len(o) == 1)
    _check_class(t, owners2, _row_of(t), 1, 1)
    _check_stats(t, owners2, G)
    t.close()


def test_caps_host_and_device_forms():
    import torch
    k = 31
    t, owners = _index(k, seed=11)
    lib = _lib.load()
    row_of = _row_of(t)
    want, wrows = _class(owners, row_of, 0, G - 1)
    n = len(want)
    cnt = C.c_uint64()
    assert lib.bft_gpu_kmers_by_count(t._h, 0, G - 1, None, None, None, 0, C.byref(cnt)) == 0 and cnt.value == n  # count only
    rc, got, km, asc, rows = _raw(t, 0, G - 1, cap=n - 1)
    assert rc == NOSPACE and got == n
    assert (km == 0xAA).all() and (asc == 0xAA).all() and (rows == 0xAAAAAAAA).all()  # nothing written
    spectrum = np.full(G, 7, dtype=np.uint64)
    assert lib.bft_gpu_pangenome_stats(t._h, spectrum.ctypes.data, None, None, G) == NOSPACE and (spectrum == 7).all()
    assert lib.bft_gpu_pangenome_stats(t._h, None, None, None, 0) == 0
    # the device form with a small cap: exactly the first `cap` in row order, the bytes behind them untouched, the total reported
    cap = 100
    assert n > 2 * cap
    dk = torch.full((2 * cap, t.nb), 0xAA, dtype=torch.uint8, device="cuda")
    da = torch.full((2 * cap, k + 1), 0xAA, dtype=torch.uint8, device="cuda")
    dr = torch.full((2 * cap,), 0x7A7A7A7A, dtype=torch.int32, device="cuda")
    dc = torch.zeros(1, dtype=torch.int64, device="cuda")
    t.kmers_by_count_dev(0, G - 1, dk.data_ptr(), da.data_ptr(), dr.data_ptr(), cap, dc.data_ptr())
    torch.cuda.synchronize()
    assert int(dc.cpu()[0]) == n
    hk, ha, hr = dk.cpu().numpy(), da.cpu().numpy(), dr.cpu().numpy()
    assert S.packed_to_ascii(hk[:cap], k) == want[:cap] and (hk[cap:] == 0xAA).all()
    assert [r.tobytes().decode() for r in ha[:cap, :k]] == want[:cap] and (ha[:cap, k] == 0).all() and (ha[cap:] == 0xAA).all()
    assert hr[:cap].astype(np.uint32).tolist() == wrows[:cap].tolist() and (hr[cap:] == 0x7A7A7A7A).all()
    # sizing call: NULL outputs, cap 0; an inverted range gives zero
    dc.fill_(7)
    t.kmers_by_count_dev(G, G, 0, 0, 0, 0, dc.data_ptr())
    torch.cuda.synchronize()
    assert int(dc.cpu()[0]) == len(_class(owners, row_of, G, G)[0])
    t.kmers_by_count_dev(3, 2, 0, 0, 0, 0, dc.data_ptr())
    torch.cuda.synchronize()
    assert int(dc.cpu()[0]) == 0
    ds = torch.full((G + 1,), 7, dtype=torch.int64, device="cuda")
    with pytest.raises(_lib.BFTError):
        t.pangenome_stats_dev(ds.data_ptr(), 0, 0, G)
    t.close()


def test_dev_forms_on_a_user_stream_interleaved_with_queries():
    import torch
    k = 36
    t, owners = _index(k, seed=5)
    row_of = _row_of(t)
    n = len(row_of)
    core, core_rows = _class(owners, row_of, G, G)
    single, single_rows = _class(owners, row_of, 1, 1)
    ws, wt, wp = _stats(owners, G)
    paths = t.simple_paths()
    labels, sizes = t.components()
    asc = sorted(owners)[::5]
    q, _ = S.ascii_to_packed(asc, k)
    bits_h, off_h, ids_h = t.query_colors(q)
    pres_h = t.query_presence(q)
    pref = q[:64].copy()
    po, _, _, _ = t.query_prefixes(pref, np.full(64, 20, dtype=np.uint8))
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        dq = torch.from_numpy(q.reshape(-1).copy()).cuda()
        dbits = torch.zeros((len(q) + 63) // 64, dtype=torch.int64, device="cuda")
        dpres = torch.zeros((len(q) + 63) // 64, dtype=torch.int64, device="cuda")
        doffc = torch.zeros(len(q) + 1, dtype=torch.int64, device="cuda")
        dids = torch.zeros(len(ids_h) + 1, dtype=torch.int32, device="cuda")
        dp = torch.from_numpy(pref.reshape(-1).copy()).cuda()
        dl = torch.full((64,), 20, dtype=torch.uint8, device="cuda")
        dpo = torch.zeros(65, dtype=torch.int64, device="cuda")
        pc = torch.zeros(3, dtype=torch.int64, device="cuda")
        cc = torch.zeros(3, dtype=torch.int64, device="cuda")
        lab = torch.full((n,), 7, dtype=torch.int32, device="cuda")
        k1 = torch.zeros((len(core), t.nb), dtype=torch.uint8, device="cuda")
        r1 = torch.zeros(len(core), dtype=torch.int32, device="cuda")
        a2 = torch.zeros((len(single), k + 1), dtype=torch.uint8, device="cuda")
        r2 = torch.zeros(len(single), dtype=torch.int32, device="cuda")
        c1 = torch.full((1,), 7, dtype=torch.int64, device="cuda")
        c2 = torch.full((1,), 7, dtype=torch.int64, device="cuda")
        c3 = torch.full((1,), 7, dtype=torch.int64, device="cuda")
        sp1 = torch.full((G + 1,), 7, dtype=torch.int64, device="cuda")
        to1 = torch.full((G,), 7, dtype=torch.int64, device="cuda")
        pr1 = torch.full((G,), 7, dtype=torch.int64, device="cuda")
        sp2 = torch.full((G + 1,), 7, dtype=torch.int64, device="cuda")
        st = s.cuda_stream
        t.kmers_by_count_dev(G, G, k1.data_ptr(), 0, r1.data_ptr(), len(core), c1.data_ptr(), stream=st)
        t.query_presence_dev(dq.data_ptr(), len(q), dpres.data_ptr(), st)
        t.pangenome_stats_dev(sp1.data_ptr(), to1.data_ptr(), pr1.data_ptr(), G + 1, stream=st)
        t.query_colors_dev(dq.data_ptr(), len(q), dbits.data_ptr(), doffc.data_ptr(), dids.data_ptr(), len(ids_h) + 1, stream=st)
        t.simple_paths_dev(0, 0, 0, 0, pc.data_ptr(), stream=st)
        t.kmers_by_count_dev(1, 1, 0, a2.data_ptr(), r2.data_ptr(), len(single), c2.data_ptr(), stream=st)
        t.components_dev(lab.data_ptr(), 0, 0, cc.data_ptr(), stream=st)
        t.query_prefixes_dev(dp.data_ptr(), dl.data_ptr(), 64, dpo.data_ptr(), 0, 0, 0, 0, 0, stream=st)
        t.pangenome_stats_dev(sp2.data_ptr(), 0, 0, G + 1, stream=st)
        t.kmers_by_count_dev(0, G - 1, 0, 0, 0, 0, c3.data_ptr(), stream=st)
    s.synchronize()
    assert int(c1.cpu()[0]) == len(core) and int(c2.cpu()[0]) == len(single) and int(c3.cpu()[0]) == n - len(core)
    assert S.packed_to_ascii(k1.cpu().numpy(), k) == core and r1.cpu().numpy().astype(np.uint32).tolist() == core_rows.tolist()
    ha = a2.cpu().numpy()
    assert [r.tobytes().decode() for r in ha[:, :k]] == single and (ha[:, k] == 0).all()
    assert r2.cpu().numpy().astype(np.uint32).tolist() == single_rows.tolist()
    assert sp1.cpu().tolist() == ws.tolist() == sp2.cpu().tolist()
    assert to1.cpu().tolist() == wt.tolist() and pr1.cpu().tolist() == wp.tolist()
    assert pc.cpu().tolist()[0] == len(paths)
    assert cc.cpu().tolist()[0] == len(sizes) and (lab.cpu().numpy().view(np.uint32) == labels).all()
    assert (dpres.cpu().numpy().view(np.uint8)[:len(pres_h)] == pres_h).all() and S.from_bits(pres_h, len(q)).all()
    assert (dbits.cpu().numpy().view(np.uint8)[:len(bits_h)] == bits_h).all()
    assert (doffc.cpu().numpy().astype(np.uint64) == off_h).all()
    assert (dids.cpu().numpy()[:len(ids_h)].astype(np.uint32) == ids_h).all()
    want_ids = np.concatenate([np.array(sorted(owners[x]), dtype=np.uint32) for x in asc])
    assert ids_h.tolist() == want_ids.tolist()
    assert (dpo.cpu().numpy().astype(np.uint64) == po).all()
    # the host forms afterwards, on the handle's stream
    _check_class(t, owners, row_of, G, G)
    _check_stats(t, owners, G)
    assert t.simple_paths() == paths
    t.close()


def test_a_class_through_subgraph():
    k = 27
    t, owners = _index(k, seed=13)
    row_of = _row_of(t)
    for lo, hi in ((G, G), (1, 1)):
        want, _ = _class(owners, row_of, lo, hi)
        packed, _ = t.kmers_by_count(lo, hi)
        sub, absent = t.subgraph(packed)
        assert absent == 0
        km, _ = sub.extract()
        assert sorted(S.packed_to_ascii(km, k)) == sorted(want)
        sub_owners = {x: owners[x] for x in want}
        _check_stats(sub, sub_owners, G)
        sub.close()
    t.close()


def test_kernel_time_and_stages():
    t, _ = _index(27, seed=2)
    t.build()
    t.kernel_time(reset=True)
    t.kmers_by_count(1, 1)
    ms, launches = t.kernel_time(reset=True)
    assert launches >= 2 and ms > 0
    t.set_option("build_stages", 1)
    t.pangenome_stats()
    names = [nm for nm, _, _ in t.build_stages()]
    assert any("rows per colour set" in nm for nm in names) and any("dictionary" in nm for nm in names)
    t.close()
