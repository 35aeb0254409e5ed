"""Batched prefix matching on the GPU (bft_gpu_query_prefixes / _dev, BFT.query_prefixes): every prefix's matches against ground truth -- a
numpy filter over the inserted k-mers, not the product's own extract -- at key widths W = 1..4, with and without remaining nucleotides
(k % 9), for prefixes of every length; host and device calls agree; capacity, "compact_table", merges, .bft round trips, bad lengths and
kernel timing."""
import numpy as np
import pytest

from bloomfiltertrie_amd import BFT, _lib, synth as S

pytestmark = pytest.mark.gpu

KS = (9, 18, 27, 31, 36, 63, 64, 90, 126)
N_GENOMES = 4


def _index(k, seed=0, length=20000, compact=None):
    """An index of N_GENOMES related genomes (shared and private k-mers: real colour sets) and the ground truth: distinct k-mer codes with
    the sorted genome ids of each."""
    anc = S.random_genome(length, seed + 1)
    genomes = [anc] + [S.mutate(anc, 0.02, seed + 2 + g) for g in range(N_GENOMES - 1)]
    t = BFT(k, device=0)
    if compact is not None:
        t.set_option("compact_table", compact)
    owners = {}
    for gid, g in enumerate(genomes):
        km = S.distinct(S.kmers_of(g, k))
        t.insert_kmers(km, gid)
        for key in S.row_keys(km).tolist():
            owners.setdefault(key, []).append(gid)
    allk = np.concatenate([S.distinct(S.kmers_of(g, k)) for g in genomes])
    allk = S.distinct(allk)
    return t, allk, owners


def _lengths_for(k, rng, n, short=True):
    """Every length with extra weight on 9f, 9f + 1, 9f + 8 and the lengths that reach into the k % 9 remaining nucleotides."""
    L, R = divmod(k, 9)
    special = [ln for f in range(L + 1) for ln in (9 * f, 9 * f + 1, 9 * f + 8) if 1 <= ln <= k] + list(range(9 * L + 1, k + 1))
    pool = np.array(list(range(1, k + 1)) + special * 3)
    if not short:
        pool = pool[pool >= min(k, 8)]
    return rng.choice(pool, n).astype(np.uint8)


def _prefixes(allk, k, n, rng, short=True):
    """n prefixes: from stored k-mers, random, duplicated; nucleotides past the length (and the padding bits of the last byte) are garbage."""
    nb = S.kmer_bytes(k)
    if n == 0:
        return np.zeros((0, nb), np.uint8), np.zeros(0, np.uint8)
    lens = _lengths_for(k, rng, n, short)
    src = rng.integers(0, 3, n)
    codes = rng.integers(0, 4, (n, k), dtype=np.uint8)
    stored = S.unpack_codes(allk[rng.integers(0, len(allk), n)], k)
    codes[src == 0] = stored[src == 0]
    dup = np.nonzero(src == 2)[0]
    if len(dup) > 1:
        codes[dup[1::2]] = codes[dup[::2]][:len(dup[1::2])]
        lens[dup[1::2]] = lens[dup[::2]][:len(dup[1::2])]
    garbage = rng.integers(0, 4, (n, k), dtype=np.uint8)
    keep = np.arange(k)[None, :] < lens[:, None]
    pref = S.pack_codes(np.where(keep, codes, garbage))
    if (2 * k) % 8:
        pref[:, -1] |= (rng.integers(0, 256, n).astype(np.uint8) & np.uint8((0xFF << ((2 * k) % 8)) & 0xFF))
    return pref, lens


def _truth_counts(allk_codes, k, pref, lens):
    """Matches per prefix by sorted prefix keys of the inserted k-mers (numpy only)."""
    pc = S.unpack_codes(pref, k)
    counts = np.zeros(len(pref), dtype=np.int64)
    for ln in np.unique(lens):
        sel = np.nonzero(lens == ln)[0]
        kv = np.sort(np.ascontiguousarray(allk_codes[:, :ln]).view(np.dtype((np.void, int(ln)))).ravel())
        qv = np.ascontiguousarray(pc[sel, :ln]).view(np.dtype((np.void, int(ln)))).ravel()
        counts[sel] = np.searchsorted(kv, qv, side="right") - np.searchsorted(kv, qv, side="left")
    return counts


def _check(t, k, allk, owners, pref, lens, res, ext=None):
    offsets, kmers, rows, sets = res
    n = len(pref)
    assert offsets.shape == (n + 1,) and offsets[0] == 0
    cnt = np.diff(offsets.astype(np.int64))
    allk_codes = S.unpack_codes(allk, k)
    assert (cnt == _truth_counts(allk_codes, k, pref, lens)).all()
    m = int(offsets[-1])
    assert len(kmers) == m and len(rows) == m and len(sets) == m
    if m == 0:
        return
    owner = np.repeat(np.arange(n), cnt)
    # every returned k-mer starts with its prefix and is stored; rows ascend strictly inside a prefix
    got = S.unpack_codes(kmers, k)
    pc = S.unpack_codes(pref, k)
    ln = lens[owner].astype(np.int64)
    head = np.arange(k)[None, :] < ln[:, None]
    assert ((got == pc[owner]) | ~head).all()
    assert S.member(kmers, allk).all()
    same = owner[1:] == owner[:-1]
    assert (rows[1:][same] > rows[:-1][same]).all()
    # rows are positions in extract(); colour sets are query_rows' for those k-mers and hold the inserted genomes
    if ext is None:
        ext = t.extract()
    assert (ext[0][rows] == kmers).all()
    _, qrows, qsets = t.query_rows(kmers)
    assert (qrows == rows).all() and (qsets == sets).all()
    pick = np.unique(np.linspace(0, m - 1, min(m, 200)).astype(np.int64))
    keys = S.row_keys(kmers[pick]).tolist()
    for key, cs in zip(keys, sets[pick]):
        assert t.colorset(int(cs)) == owners[key]


def _dev_query(t, pref, lens, cap=None, stream=None):
    import torch
    n = len(pref)
    nb = t.nb
    dp = torch.from_numpy(np.ascontiguousarray(pref).reshape(-1).copy()).cuda() if n else torch.zeros(1, dtype=torch.uint8, device="cuda")
    dl = torch.from_numpy(lens.copy()).cuda() if n else torch.zeros(1, dtype=torch.uint8, device="cuda")
    doff = torch.full((n + 1,), 7, dtype=torch.int64, device="cuda")
    dneed = torch.full((1,), 7, dtype=torch.int64, device="cuda")
    t.query_prefixes_dev(dp.data_ptr(), dl.data_ptr(), n, doff.data_ptr(), 0, 0, 0, 0, dneed.data_ptr(), stream)
    torch.cuda.synchronize()
    need = int(dneed.item())
    c = need if cap is None else cap
    size = max(c, 1) + 16
    dk = torch.full((size * nb,), 0xAB, dtype=torch.uint8, device="cuda")
    dr = torch.full((size,), -1, dtype=torch.int32, device="cuda")
    dc = torch.full((size,), -1, dtype=torch.int32, device="cuda")
    dneed.fill_(7)
    t.query_prefixes_dev(dp.data_ptr(), dl.data_ptr(), n, doff.data_ptr(), dk.data_ptr(), dr.data_ptr(), dc.data_ptr(), c, dneed.data_ptr(), stream)
    torch.cuda.synchronize()
    return (doff.cpu().numpy().view(np.uint64), dk.cpu().numpy().reshape(size, nb), dr.cpu().numpy().view(np.uint32), dc.cpu().numpy().view(np.uint32),
            int(dneed.item()), c)


@pytest.mark.parametrize("k", KS)
def test_prefixes_match_ground_truth(k):
    t, allk, owners = _index(k)
    ext = t.extract()
    rng = np.random.default_rng(k)
    for n in (0, 1, 65, 100000):
        pref, lens = _prefixes(allk, k, n, rng, short=n <= 65)
        res = t.query_prefixes(pref, lens)
        _check(t, k, allk, owners, pref, lens, res, ext)
        if n in (0, 65, 100000):  # the device call gives the same answer
            doff, dk, dr, dc, need, c = _dev_query(t, pref, lens)
            m = int(res[0][-1])
            assert need == m and (doff == res[0]).all()
            assert (dk[:m] == res[1]).all() and (dr[:m] == res[2]).all() and (dc[:m] == res[3]).all()
            assert (dk[m:] == 0xAB).all() and (dr[m:] == 0xFFFFFFFF).all()
    t.close()


def test_ascii_prefixes_and_every_length():
    k = 27
    t, allk, owners = _index(k, seed=3)
    asc = S.packed_to_ascii(allk[:40], k)
    rng = np.random.default_rng(1)
    strs = [s[:int(ln)] for s, ln in zip(asc, rng.integers(1, k + 1, 40))] + [asc[0][:ln] for ln in range(1, k + 1)] + ["acgU", "TTTTTTTTTTTT"]
    res = t.query_prefixes(strs)
    pref, _ = S.ascii_to_packed([s.upper().replace("U", "T") + "A" * (k - len(s)) for s in strs], k)
    lens = np.array([len(s) for s in strs], dtype=np.uint8)
    _check(t, k, allk, owners, pref, lens, res)
    for bad in ([""], ["A" * (k + 1)], ["ACGN"]):
        with pytest.raises(ValueError):
            t.query_prefixes(bad)
    t.close()


def test_capacity_host_and_device():
    import ctypes as C
    k = 27
    t, allk, owners = _index(k, seed=5)
    rng = np.random.default_rng(2)
    pref, lens = _prefixes(allk, k, 65, rng)
    full = t.query_prefixes(pref, lens)
    m = int(full[0][-1])
    assert m > 10
    lib = _lib.load()
    for cap in (0, 1, m - 1):
        offs = np.full(66, 5, dtype=np.uint64)
        km = np.full((m, t.nb), 9, dtype=np.uint8)
        rows = np.full(m, 9, dtype=np.uint32)
        sets = np.full(m, 9, dtype=np.uint32)
        need = C.c_uint64(0)
        rc = lib.bft_gpu_query_prefixes(t._h, pref.ctypes.data, lens.ctypes.data, 65, offs.ctypes.data, km.ctypes.data, rows.ctypes.data,
                                        sets.ctypes.data, cap, C.byref(need))
        assert rc == -6 and need.value == m
        assert (offs == 5).all() and (km == 9).all() and (rows == 9).all() and (sets == 9).all()  # nothing written
    # every output NULL: the call only counts
    offs = np.zeros(66, dtype=np.uint64)
    need = C.c_uint64(0)
    assert lib.bft_gpu_query_prefixes(t._h, pref.ctypes.data, lens.ctypes.data, 65, offs.ctypes.data, None, None, None, 0, C.byref(need)) == 0
    assert need.value == m and (offs == full[0]).all()
    # the device call writes the first cap entries, never one beyond, and the exact total
    for cap in (1, m // 3, m - 1, m, m + 5):
        doff, dk, dr, dc, need, c = _dev_query(t, pref, lens, cap=cap)
        w = min(cap, m)
        assert need == m and (doff == full[0]).all()
        assert (dk[:w] == full[1][:w]).all() and (dr[:w] == full[2][:w]).all() and (dc[:w] == full[3][:w]).all()
        assert (dk[w:] == 0xAB).all() and (dr[w:] == 0xFFFFFFFF).all() and (dc[w:] == 0xFFFFFFFF).all()
    t.close()


def test_compact_table_on_and_off_agree():
    k = 31
    out = []
    for compact in (1, 0):
        t, allk, owners = _index(k, seed=7, compact=compact)
        pref, lens = _prefixes(allk, k, 2000, np.random.default_rng(4))
        # the device call first: under "compact_table" 1 it brings the sorted table back itself
        doff, dk, dr, dc, need, c = _dev_query(t, pref, lens)
        res = t.query_prefixes(pref, lens)
        _check(t, k, allk, owners, pref, lens, res)
        assert (doff == res[0]).all() and (dr[:need] == res[2]).all()
        out.append(res)
        t.close()
    for a, b in zip(*out):
        assert (a == b).all()


def test_after_merge_and_bft_file_round_trip(tmp_path):
    k = 27
    t, allk, owners = _index(k, seed=9)
    rng = np.random.default_rng(6)
    pref, lens = _prefixes(allk, k, 3000, rng)
    _check(t, k, allk, owners, pref, lens, t.query_prefixes(pref, lens))
    # insert (a new genome and more of an old one), build, query
    extra = S.distinct(S.kmers_of(S.random_genome(8000, 99), k))
    t.insert_kmers(extra, N_GENOMES)
    t.insert_kmers(extra[:100], 0)
    for i, key in enumerate(S.row_keys(extra).tolist()):
        ids = owners.setdefault(key, [])
        for g in ([0, N_GENOMES] if i < 100 else [N_GENOMES]):
            if g not in ids:
                ids.append(g)
                ids.sort()
    allk2 = S.distinct(np.concatenate([allk, extra]))
    pref2, lens2 = _prefixes(allk2, k, 3000, rng)
    _check(t, k, allk2, owners, pref2, lens2, t.query_prefixes(pref2, lens2))
    # .bft round trip
    path = str(tmp_path / "p.bft")
    t.write_bft(path)
    u = BFT.load_bft(path)
    ru, rt = u.query_prefixes(pref2, lens2), t.query_prefixes(pref2, lens2)
    _check(u, k, allk2, owners, pref2, lens2, ru)
    for a, b in zip(ru, rt):
        assert (a == b).all()
    u.close()
    t.close()


def test_presence_and_colours_unchanged_around_a_prefix_call():
    k = 36
    t, allk, owners = _index(k, seed=11)
    rng = np.random.default_rng(8)
    q = np.concatenate([allk[::3], S.snp_mutants(allk[::5], k, 3)])
    before = (t.query_presence(q), t.query_colors(q), t.query_rows(q))
    pref, lens = _prefixes(allk, k, 5000, rng)
    t.query_prefixes(pref, lens)
    _dev_query(t, pref, lens)
    after = (t.query_presence(q), t.query_colors(q), t.query_rows(q))
    assert (before[0] == after[0]).all()
    for a, b in zip(before[1], after[1]):
        assert (a == b).all()
    for a, b in zip(before[2], after[2]):
        assert (a == b).all()
    t.close()


def test_bad_length_and_empty_index():
    import ctypes as C
    k = 18
    t, allk, owners = _index(k, seed=13, length=5000)
    lib = _lib.load()
    pref = allk[:3].copy()
    offs = np.zeros(4, dtype=np.uint64)
    need = C.c_uint64(0)
    for bad in (0, k + 1):
        lens = np.array([3, bad, 5], dtype=np.uint8)
        assert lib.bft_gpu_query_prefixes(t._h, pref.ctypes.data, lens.ctypes.data, 3, offs.ctypes.data, None, None, None, 0, C.byref(need)) == -1
        # the device call gives that prefix an empty list
        doff, dk, dr, dc, m, c = _dev_query(t, pref, lens)
        ok = t.query_prefixes(pref[[0, 2]], lens[[0, 2]])
        assert doff[2] == doff[1] and m == int(ok[0][-1])
        assert (dr[:m] == ok[2]).all()
    t.close()
    e = BFT(27, device=0)  # nothing inserted
    offs, km, rows, sets = e.query_prefixes(["ACG", "T"])
    assert (offs == 0).all() and len(rows) == 0
    e.close()


def test_kernel_time_counts_prefix_launches():
    k = 27
    t, allk, owners = _index(k, seed=15, length=5000)
    pref, lens = _prefixes(allk, k, 500, np.random.default_rng(3))
    t.query_prefixes(pref, lens)  # (warm: builds, brings the table back)
    t.kernel_time(reset=True)
    t.query_prefixes(pref, lens)
    ms, launches = t.kernel_time(reset=True)
    assert launches >= 6 and ms > 0
    _dev_query(t, pref, lens)
    ms, launches = t.kernel_time(reset=True)
    assert launches >= 11 and ms > 0
    t.close()
