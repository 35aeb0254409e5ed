"""Every k-mer hash instantiation the geometry can pick, against ground truth: one case per reachable (key width W, slots per line S) of
bft_kh_geometry (the cases and the scan that proves them complete: tests/test_kh_geometry_host.py).  Each case builds an index of
exactly N_KMERS distinct k-mers with exactly the case's number of colour sets, asserts that the table was built with the case's S (a
table that fails to build leaves the queries to the container walk, which would pass without running the hash), checks the table
against the host restatement, and runs every query entry point -- host and device forms, at batch sizes that leave partial quads
and wavefronts -- against the membership matrix the index was built from."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_kh_geometry_host import CASES, LARGE, N_KMERS, case_data, geometry_of, load_hostlib, n_genomes, words  # noqa: E402

from bloomfiltertrie_amd import synth as S  # noqa: E402

pytestmark = pytest.mark.gpu
BATCHES = (1, 2, 3, 5, 63, 65, 257, 4097)
RAGGED = 30011
COMP = str.maketrans("ACGTN", "TGCAN")


@pytest.fixture(scope="module")
def hostlib():
    return load_hostlib()


def _guards(t, S_):
    bt, fp = t.build_time(), t.footprint()
    assert bt["kmer_hash_lines"] > 0 and int(bt["kmer_hash_slots"]) == S_ and fp["kmer_hash"] > 0, (bt["kmer_hash_lines"], bt["kmer_hash_slots"], fp["kmer_hash"])


def _table_check(t, hostlib, k, load):
    """the GPU table against bft_hosttest_kh_verify and, byte for byte, the sequential build (test_kmer_hash_table_invariants' check)"""
    W = words(k)
    kh = np.ascontiguousarray(t.debug_array("kh", np.uint64))
    tk = np.ascontiguousarray(t.debug_array("tk", np.uint64).reshape(-1, W))
    tcol = np.ascontiguousarray(t.debug_array("tcol", np.uint32))
    ovk = np.ascontiguousarray(t.debug_array("kh_ovf_k", np.uint64))
    ovv = np.ascontiguousarray(t.debug_array("kh_ovf_v", np.uint32))
    n_sets = t.info()["colorsets"]
    bt = t.build_time()
    home_lines, db, maxd, novf = int(bt["kmer_hash_lines"]), int(bt["kmer_hash_dbits"]), int(bt["kmer_hash_maxd"]), int(bt["kmer_hash_overflow"])
    assert home_lines > 0 and len(kh) == (home_lines + 256) * 8 and len(ovv) == novf and len(ovk) == novf * W
    assert novf > 0  # (the case's hot runs: tests/test_kh_geometry_host.py)
    rc = hostlib.bft_hosttest_kh_verify(tk.ctypes.data, tcol.ctypes.data, len(tk), k, n_sets, load, maxd, kh.ctypes.data, len(kh) // 8, ovk.ctypes.data, ovv.ctypes.data, novf)
    assert rc == 1, (rc, load)
    lines = np.zeros(len(kh) + 4096, np.uint64)
    geo = np.zeros(14, np.uint32)
    hk, hv = np.zeros(4096 * W, np.uint64), np.zeros(4096, np.uint32)
    nw = hostlib.bft_hosttest_kh_build(tk.ctypes.data, tcol.ctypes.data, len(tk), k, n_sets, load, lines.ctypes.data, len(lines), geo.ctypes.data, hk.ctypes.data, hv.ctypes.data)
    assert nw == len(kh) and int(geo[10]) == home_lines and int(geo[12]) == db and int(geo[13]) == novf and int(geo[11]) == maxd, (nw, len(kh), geo)
    assert (kh == lines[:nw]).all() and (ovk == hk[: novf * W]).all() and (ovv == hv[:novf]).all()


def _mutate_at(codes, col, rng):
    c = codes.copy()
    c[:, col] = (c[:, col] + rng.integers(1, 4, len(c), dtype=np.uint8)) & 3
    return c


def _neighbours(q, k, stored_keys):
    """successors / predecessors of every query among the stored k-mers"""
    codes = S.unpack_codes(q, k)
    succ = np.zeros(len(q), np.int64)
    pred = np.zeros(len(q), np.int64)
    for c in range(4):
        col = np.full((len(q), 1), c, np.uint8)
        succ += np.isin(S.row_keys(S.pack_codes(np.concatenate([codes[:, 1:], col], axis=1))), stored_keys)
        pred += np.isin(S.row_keys(S.pack_codes(np.concatenate([col, codes[:, :-1]], axis=1))), stored_keys)
    return succ, pred


class Truth:
    def __init__(self, km, sets, M, k):
        self.km, self.sets, self.M, self.k = km, sets, M, k
        self.keys = S.row_keys(km)
        self.pos = dict(zip(self.keys.tolist(), range(len(km))))
        self.str_pos = dict(zip(S.packed_to_ascii(km, k), range(len(km))))

    def idx(self, q):
        return np.array([self.pos.get(x, -1) for x in S.row_keys(q).tolist()], np.int64)

    def rows(self, qidx):
        out = np.zeros((len(qidx), self.M.shape[1]), np.uint8)
        out[qidx >= 0] = self.M[self.sets[qidx[qidx >= 0]]]
        return out

    def sequence(self, r, canonical, thr):
        k = self.k
        nb = max(0, len(r) - k + 1)
        cnt = np.zeros(self.M.shape[1], np.int64)
        for i in range(nb):
            x = r[i:i + k]
            if "N" in x:
                continue
            if canonical:
                x = min(x, x[::-1].translate(COMP))
            j = self.str_pos.get(x, -1)
            if j >= 0:
                cnt += self.M[self.sets[j]]
        return np.flatnonzero((cnt > 0) & (cnt >= math.ceil(nb * thr))).tolist()


def _dev_colors(t, dq, b, cap, G, dev, st):
    import torch
    dbits = torch.zeros(((b + 63) // 64) * 8, dtype=torch.uint8, device=dev)
    doff = torch.zeros(b + 1, dtype=torch.int64, device=dev)
    dids = torch.full((cap + 256,), -1, dtype=torch.int32, device=dev)
    dneed = torch.zeros(1, dtype=torch.int64, device=dev)
    t.query_colors_dev(dq.data_ptr(), b, dbits.data_ptr(), doff.data_ptr(), dids.data_ptr(), cap, dneed.data_ptr(), st)
    torch.cuda.synchronize()
    return dbits.cpu().numpy(), doff.cpu().numpy().view(np.uint64), dids.cpu().numpy().view(np.uint32), int(dneed.item())


def _check_colors(t, q, exp_rows, dev, st, dq=None, hashed=True):
    """id lists, host and device calls; hashed: the k-mer hash answers (k_colors_kh), which writes the first ids_cap ids of a list that
    does not fit, where the container walk writes none (include/bft_gpu.h)"""
    import torch
    b = len(q)
    pres = exp_rows.any(axis=1) if exp_rows.shape[1] else np.zeros(b, bool)
    bits, off, ids = t.query_colors(q)
    exp_off = np.zeros(b + 1, np.uint64)
    exp_off[1:] = np.cumsum(exp_rows.sum(axis=1))
    exp_ids = np.nonzero(exp_rows)[1].astype(np.uint32)
    total = len(exp_ids)
    assert (S.from_bits(bits, b) == pres).all() and (off == exp_off).all() and (ids == exp_ids).all()
    dq = torch.from_numpy(q).to(dev) if dq is None else dq
    db, do, di, need = _dev_colors(t, dq, b, total, exp_rows.shape[1], dev, st)
    assert need == total and (S.from_bits(db, b) == pres).all() and (do == exp_off).all() and (di[:total] == exp_ids).all() and (di[total:] == 0xFFFFFFFF).all()
    if total:  # one id short: the needed count, and nothing written beyond the capacity
        db, do, di, need = _dev_colors(t, dq, b, total - 1, exp_rows.shape[1], dev, st)
        assert need == total and (di[total - 1:] == 0xFFFFFFFF).all() and (do == exp_off).all()
        assert (di[:total - 1] == exp_ids[:total - 1]).all() if hashed else (di == 0xFFFFFFFF).all()


def _check_batch(t, q, qidx, tr, succ, pred, dev, st):
    import torch
    b = len(q)
    G = tr.M.shape[1]
    pres = qidx >= 0
    exp_rows = tr.rows(qidx)
    dq = torch.from_numpy(np.ascontiguousarray(q)).to(dev)
    nbw = ((b + 63) // 64) * 8
    # presence
    assert (S.from_bits(t.query_presence(q), b) == pres).all()
    dbits = torch.zeros(nbw, dtype=torch.uint8, device=dev)
    t.query_presence_dev(dq.data_ptr(), b, dbits.data_ptr(), st)
    torch.cuda.synchronize()
    assert (S.from_bits(dbits.cpu().numpy(), b) == pres).all()
    # colour rows
    bits, rows = t.query_color_rows(q)
    assert (S.from_bits(bits, b) == pres).all() and (np.unpackbits(rows, axis=1, bitorder="little")[:, :G] == exp_rows).all()
    dbits.zero_()
    drows = torch.full((b, (G + 7) // 8), 0xAA, dtype=torch.uint8, device=dev)
    dscr = torch.zeros(b, dtype=torch.int32, device=dev)
    t.query_color_rows_dev(dq.data_ptr(), b, dbits.data_ptr(), drows.data_ptr(), dscr.data_ptr(), st)
    torch.cuda.synchronize()
    assert (S.from_bits(dbits.cpu().numpy(), b) == pres).all()
    assert (np.unpackbits(drows.cpu().numpy(), axis=1, bitorder="little")[:, :G] == exp_rows).all()
    # id lists
    _check_colors(t, q, exp_rows, dev, st, dq)
    # branching: (successors << 4) | predecessors among the stored k-mers
    exp_cnt = ((succ << 4) | pred).astype(np.uint8)
    exp_bits = (succ > 1) | (pred > 1)
    bb, cnt = t.query_branching(q, with_counts=True)
    assert (cnt == exp_cnt).all() and (S.from_bits(bb, b) == exp_bits).all()
    dbits.zero_()
    dcnt = torch.zeros(b, dtype=torch.uint8, device=dev)
    t.query_branching_dev(dq.data_ptr(), b, dbits.data_ptr(), dcnt.data_ptr(), st)
    torch.cuda.synchronize()
    assert (dcnt.cpu().numpy() == exp_cnt).all() and (S.from_bits(dbits.cpu().numpy(), b) == exp_bits).all()


def _reads(tr, genome, k, rng):
    s = "".join("ACGT"[c] for c in genome[:150000])
    reads = []
    for ln in [k - 1, k, k + 1, 300] * 10 + [int(x) for x in rng.integers(k, 400, 12)]:
        a = int(rng.integers(0, len(s) - ln))
        r = s[a:a + ln]
        if rng.random() < 0.4:
            r = r[::-1].translate(COMP)
        if rng.random() < 0.25:
            p = int(rng.integers(0, len(r)))
            r = r[:p] + "N" + r[p + 1:]
        reads.append(r)
    reads.append("".join("ACGT"[c] for c in rng.integers(0, 4, 200)))  # (absent)
    if k % 2 == 0:  # the stored palindromes, alone and inside a read, and one not stored
        pal = S.packed_to_ascii(tr.km[:8], k)
        assert all(p == p[::-1].translate(COMP) for p in pal)
        reads += pal + [s[:40] + pal[0] + s[40:90]]
        h = "".join("ACGT"[c] for c in rng.integers(0, 4, k // 2))
        reads.append(h + h[::-1].translate(COMP))
    return reads


def _check_sequences(t, tr, reads, dev, st):
    import torch
    G = tr.M.shape[1]
    enc = [r.encode() for r in reads]
    off = np.zeros(len(enc) + 1, np.int64)
    off[1:] = np.cumsum([len(e) for e in enc])
    d_blob = torch.from_numpy(np.frombuffer(b"".join(enc), dtype=np.uint8).copy()).to(dev)
    d_off = torch.from_numpy(off).to(dev)
    for canonical in (False, True):
        for thr in (0.1, 1.0):
            exp = [tr.sequence(r, canonical, thr) for r in reads]
            got = t.query_sequences(reads, thr, canonical)
            assert got == exp, (canonical, thr, [i for i in range(len(exp)) if got[i] != exp[i]][:5])
            d_rows = torch.full((len(enc), (G + 7) // 8), 0x55, dtype=torch.uint8, device=dev)
            t.query_sequences_dev(d_blob.data_ptr(), d_off.data_ptr(), len(enc), int(off[-1]), thr, d_rows.data_ptr(), canonical, st)
            torch.cuda.synchronize()
            unp = np.unpackbits(d_rows.cpu().numpy(), axis=1, bitorder="little")[:, :G]
            assert [np.flatnonzero(x).tolist() for x in unp] == exp, (canonical, thr)


def _run_case(hostlib, W, S_, k, n_sets, load):
    import torch
    from bloomfiltertrie_amd import BFT
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    km, sets, genome = case_data(hostlib, k, N_KMERS, n_sets, load, seed=k)
    G = n_genomes(n_sets)
    M = (((np.arange(n_sets)[:, None] + 1) >> np.arange(G)[None, :]) & 1).astype(np.uint8)
    assert geometry_of(hostlib, k, N_KMERS, n_sets, load)["S"] == S_
    t = BFT(k)
    try:
        t.set_option("kmer_hash_load", load)
        t.set_option("compact_table", 0)
        for g in range(G):
            t.insert_kmers(np.ascontiguousarray(km[M[sets, g] == 1]), g)
        t.build()
        info = t.info()
        assert info["kmers"] == N_KMERS and info["colorsets"] == n_sets and info["genomes"] == G
        _guards(t, S_)
        # the table, at the case's load and at 80 %
        _table_check(t, hostlib, k, load)
        if load != 80:
            t.set_option("kmer_hash_load", 80)
            _guards(t, geometry_of(hostlib, k, N_KMERS, n_sets, 80)["S"])
            _table_check(t, hostlib, k, 80)
            t.set_option("kmer_hash_load", load)
            _guards(t, S_)
        # the sorted table dropped and restored from the table's slots (k_kh_dump)
        t.set_option("compact_table", 1)
        _guards(t, S_)
        ek, ecs = t.extract()
        tr = Truth(km, sets, M, k)
        eidx = tr.idx(ek)
        assert len(ek) == N_KMERS and (eidx >= 0).all() and len(np.unique(eidx)) == N_KMERS
        lib_cs = np.full(n_sets, -1, np.int64)  # our colour-set index -> the library's id: one-to-one
        lib_cs[sets[eidx]] = ecs
        assert (lib_cs[sets[eidx]] == ecs).all() and len(np.unique(lib_cs)) == n_sets
        rng = np.random.default_rng(k * 7 + load)
        for s in rng.choice(n_sets, min(n_sets, 300), replace=False):
            assert t.colorset(int(lib_cs[s])) == np.flatnonzero(M[s]).tolist()
        # queries: stored k-mers (the palindromes and hot runs among them), stored k-mers with their first, last or middle nucleotide
        # changed (the first two share the stored k-mer's home line), random k-mers
        head = km[:2 * 16 * 24 + 8]
        samp = km[rng.choice(N_KMERS, 9000, replace=False)]
        codes = S.unpack_codes(km[rng.choice(N_KMERS, 15000, replace=False)], k)
        q = np.concatenate([head, samp, S.pack_codes(_mutate_at(codes[:5000], 0, rng)), S.pack_codes(_mutate_at(codes[5000:10000], k - 1, rng)),
                            S.pack_codes(_mutate_at(codes[10000:], k // 2, rng))])
        q = np.concatenate([q, S.pack_codes(rng.integers(0, 4, (RAGGED - len(q), k), dtype=np.uint8))])
        q = np.ascontiguousarray(q[rng.permutation(len(q))])
        qidx = tr.idx(q)
        assert 0.25 < (qidx >= 0).mean() < 0.75
        succ, pred = _neighbours(q, k, tr.keys)
        for b in BATCHES + (RAGGED,):
            _check_batch(t, q[:b], qidx[:b], tr, succ[:b], pred[:b], dev, st)
        # rows: the row of the sorted table and the colour-set id
        pres = qidx >= 0
        bits, rows, csid = t.query_rows(q)
        assert (S.from_bits(bits, len(q)) == pres).all() and (rows[~pres] == 0xFFFFFFFF).all()
        assert (ek[rows[pres]] == q[pres]).all() and (csid[pres] == lib_cs[sets[qidx[pres]]]).all()
        reads = _reads(tr, genome, k, rng)
        _check_sequences(t, tr, reads, dev, st)
        # the container walk with plain root groups looked up in the table (k_query6h)
        t.set_option("walk_hash", 1)
        assert (S.from_bits(t.query_presence(q), len(q)) == pres).all()
        bits, crow = t.query_color_rows(q)
        assert (np.unpackbits(crow, axis=1, bitorder="little")[:, :G] == tr.rows(qidx)).all()
        t.set_option("walk_hash", 0)
        _guards(t, S_)
        if W >= 3:  # the walk's sequence and id-list kernels beyond k = 63
            t.set_option("kmer_hash", 0)
            assert t.build_time()["kmer_hash_lines"] == 0
            _check_sequences(t, tr, reads, dev, st)
            _check_colors(t, q, tr.rows(qidx), dev, st, hashed=False)
    finally:
        t.close()


@pytest.mark.parametrize("ws", sorted(CASES), ids=lambda ws: f"W{ws[0]}-S{ws[1]}")
def test_kmer_hash_instantiation_against_ground_truth(hostlib, ws):
    for k, n_sets, load in CASES[ws]:
        _run_case(hostlib, ws[0], ws[1], k, n_sets, load)


def _member_k33(uk, qk):
    """membership of 33-mer keys (high word: the last nucleotide alone) in the sorted keys uk, one high word at a time
    (workloads.member assumes few keys per high word)"""
    import torch
    out = torch.zeros(qk.shape[0], dtype=torch.bool, device=qk.device)
    for h in range(4):
        grp = uk[uk[:, 0] == h, 1].contiguous()
        sel = torch.nonzero(qk[:, 0] == h).flatten()
        if grp.numel() and sel.numel():
            x = qk[sel, 1].contiguous()
            out[sel] = grp[torch.searchsorted(grp, x).clamp(max=grp.numel() - 1)] == x
    return out


@pytest.mark.parametrize("ws", sorted(LARGE), ids=lambda ws: f"W{ws[0]}-S{ws[1]}")
def test_kmer_hash_large_instantiation_against_ground_truth(hostlib, ws):
    """Ten slots of two-word keys: 1.25x10^8 distinct 33-mers at 10 %, one genome; presence, colour rows and id lists of 2x10^7
    stored k-mers and 2x10^7 single-SNP mutants."""
    import torch
    from bloomfiltertrie_amd import BFT, workloads as WL
    k, n_sets, load, n_target = LARGE[ws]
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device=dev)
    g.manual_seed(33)
    # distinct by construction: nucleotides 0..31 are i times an odd constant (a bijection of 64-bit words), nucleotide 32 is random
    n = n_target
    lo = torch.arange(n, device=dev, dtype=torch.int64) * -7046029254386353131  # (0x9E3779B97F4A7C15 as a signed word)
    hi = torch.randint(0, 4, (n,), generator=g, device=dev, dtype=torch.int64)
    assert geometry_of(hostlib, k, n, n_sets, load)["S"] == ws[1], n
    packed = torch.cat([lo.view(torch.uint8).reshape(n, 8), hi.to(torch.uint8)[:, None]], dim=1).contiguous()
    order = torch.sort(lo, stable=True)[1]
    order = order[torch.sort(hi[order], stable=True)[1]]
    uk = torch.stack([hi[order], lo[order]], dim=1).contiguous()  # the keys of workloads.keys_of, sorted: high word first
    del lo, hi, order
    t = BFT(k)
    try:
        t.set_option("kmer_hash_load", load)
        t.insert_kmers_dev(packed.data_ptr(), n, 0)
        t.build()
        assert t.info()["kmers"] == n
        _guards(t, ws[1])
        nq = 20_000_000
        q = packed[torch.randint(0, n, (2 * nq,), generator=g, device=dev)]
        q[nq:] = WL.snp_mutate_packed(q[nq:], k, 1.0, g)
        del packed
        truth = _member_k33(uk, WL.keys_of(q))
        m = 2 * nq
        dbits = torch.zeros(((m + 63) // 64) * 8, dtype=torch.uint8, device=dev)
        t.query_presence_dev(q.data_ptr(), m, dbits.data_ptr(), st)
        torch.cuda.synchronize()
        assert torch.equal(WL.bits_to_bool(dbits, m), truth)
        assert bool(truth[:nq].all()) and int(truth[nq:].sum()) < nq // 100
        dbits.zero_()
        drows = torch.full((m, 1), 0xAA, dtype=torch.uint8, device=dev)
        dscr = torch.zeros(m, dtype=torch.int32, device=dev)
        t.query_color_rows_dev(q.data_ptr(), m, dbits.data_ptr(), drows.data_ptr(), dscr.data_ptr(), st)
        torch.cuda.synchronize()
        assert torch.equal(WL.bits_to_bool(dbits, m), truth) and torch.equal(drows[:, 0], truth.to(torch.uint8))
        del drows, dscr
        total = int(truth.sum())
        dbits.zero_()
        doff = torch.zeros(m + 1, dtype=torch.int64, device=dev)
        dids = torch.full((total + 64,), -1, dtype=torch.int32, device=dev)
        dneed = torch.zeros(1, dtype=torch.int64, device=dev)
        t.query_colors_dev(q.data_ptr(), m, dbits.data_ptr(), doff.data_ptr(), dids.data_ptr(), total, dneed.data_ptr(), st)
        torch.cuda.synchronize()
        assert int(dneed.item()) == total and torch.equal(WL.bits_to_bool(dbits, m), truth)
        assert torch.equal(doff[1:] - doff[:-1], truth.to(torch.int64)) and int(doff[0].item()) == 0
        assert bool((dids[:total] == 0).all()) and bool((dids[total:] == -1).all())
    finally:
        t.close()
        torch.cuda.empty_cache()
