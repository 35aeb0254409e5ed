"""One handle serving a mix of calls (run on the MI355X box with -m gpu): host and device-resident forms, the k-mer hash and the container walk,
the handle's stream and callers' streams, large and small batches in any order.  Every query family keeps scratch on the handle that only grows
(qc_*, sq_*, pm_*), and the library's scan carries state from one launch to the next in its scratch block (bft_scan.h) -- so the order of
the calls matters to the code, and must not matter to the answers.  Every answer is checked against ground truth: numpy tables built from
the inserted (k-mer, genome) pairs, never one GPU path against another.  Also: graphs replayed between eager calls, and kernel timing
counting every query entry point."""
import ctypes as C
import functools

import numpy as np
import pytest

from bloomfiltertrie_amd import BFT, _lib, synth as S

pytestmark = pytest.mark.gpu

GENOME_LEN = 40000
# the scan's single-tile limit (n + 1 <= 4096), k_colors_kh's tile (1024), multi-tile batches, query_dynamic_min (65536), a large batch
SIZES_2A = (70000, 20000, 4097, 4096, 4095, 1025, 1024, 1023)
SIZES_2B = (1, 63, 64, 1023, 1024, 1025, 4095, 4096, 4097, 20000, 65535, 65536, 200000)
INDEXES = [(27, 130), (63, 20)]  # (130 genomes: 17-byte colour rows, the one-launch row kernel of the k-mer hash)


def _genome_kmers(k, ngen, seed):
    """ngen genomes: a 40 kb ancestor and SNP mutants of it, each keeping a random part of its k-mers (real, varied colour sets)."""
    anc = S.random_genome(GENOME_LEN, seed)
    rng = np.random.default_rng(seed + 1)
    out = []
    for g in range(ngen):
        km = S.distinct(S.kmers_of(S.mutate(anc, 0.002, seed + 10 + g) if g else anc, k))
        out.append(np.ascontiguousarray(km[rng.random(len(km)) < (0.9 if g % 7 == 0 else 0.2)]))
    return anc, out


class Truth:
    """Ground truth from the inserted (k-mer, genome) pairs: the sorted distinct keys and a genome-membership matrix."""

    def __init__(self, k):
        self.k = k
        self.pairs = []  # (packed k-mers, genome)
        self._keys = None

    def add(self, km, g):
        self.pairs.append((km, g))
        self._keys = None

    def _make(self):
        if self._keys is not None:
            return
        allk = np.concatenate([km for km, _ in self.pairs])
        gids = np.concatenate([np.full(len(km), g, np.int64) for km, g in self.pairs])
        keys, first, inv = np.unique(S.row_keys(allk), return_index=True, return_inverse=True)
        self._keys = keys
        self.kmers = allk[first]  # (distinct, in key order)
        self.G = int(gids.max()) + 1
        self.member = np.zeros((len(keys), self.G), dtype=bool)
        self.member[inv.reshape(-1), gids] = True

    @property
    def genomes(self):
        self._make()
        return self.G

    def lookup(self, packed):
        """index of every k-mer in the distinct table, -1 when absent"""
        self._make()
        q = S.row_keys(np.ascontiguousarray(packed))
        if len(q) == 0:
            return np.zeros(0, np.int64)
        pos = np.minimum(np.searchsorted(self._keys, q), len(self._keys) - 1)
        return np.where(self._keys[pos] == q, pos, -1)

    def members(self, idx):
        """[n, G] bool: the genomes of every k-mer (none for an absent one)"""
        m = self.member[np.maximum(idx, 0)].copy()
        m[idx < 0] = False
        return m

    def colors(self, packed):
        """(presence bits, offsets [n + 1], ids) as get_annotation + get_list_id_genomes give them: ascending ids per k-mer"""
        idx = self.lookup(packed)
        m = self.members(idx)
        off = np.zeros(len(idx) + 1, np.uint64)
        off[1:] = np.cumsum(m.sum(axis=1))
        return S.to_bits(idx >= 0), off, np.nonzero(m)[1].astype(np.uint32)

    def rows(self, packed, rowbytes):
        m = self.members(self.lookup(packed))
        out = np.zeros((len(m), rowbytes), np.uint8)
        if len(m):
            pk = np.packbits(m, axis=1, bitorder="little")
            out[:, :pk.shape[1]] = pk
        return out

    def branching(self, packed):
        """counts (successors << 4 | predecessors) and the branching bit of every k-mer, present or not (src/branchingNode.c)"""
        k, n = self.k, len(packed)
        codes = S.unpack_codes(packed, k)
        cr, cl = np.zeros(n, np.int64), np.zeros(n, np.int64)
        for x in range(4):
            col = np.full((n, 1), x, np.uint8)
            cr += self.lookup(S.pack_codes(np.concatenate([codes[:, 1:], col], axis=1))) >= 0
            cl += self.lookup(S.pack_codes(np.concatenate([col, codes[:, :-1]], axis=1))) >= 0
        return ((cr << 4) | cl).astype(np.uint8), S.to_bits((cr > 1) | (cl > 1))

    def sequences(self, reads, thr):
        """genome lists of query_sequence: genomes holding at least ceil(m * thr) (and at least one) of a read's m k-mer positions"""
        k = self.k
        wins = [np.lib.stride_tricks.sliding_window_view(r, k) for r in reads]
        m = np.array([len(w) for w in wins])
        mem = self.members(self.lookup(S.pack_codes(np.concatenate(wins)))).view(np.uint8)  # (at most 40 positions per read: no overflow)
        cnt = np.add.reduceat(mem, np.concatenate([[0], np.cumsum(m)[:-1]]), axis=0)
        need = np.ceil(m * thr)
        ok = (cnt >= need[:, None]) & (cnt > 0)
        return [np.flatnonzero(r).tolist() for r in ok]


@functools.lru_cache(maxsize=None)
def _inputs(k, ngen):
    anc, per = _genome_kmers(k, ngen, 1000 + k)
    extra = S.distinct(S.kmers_of(S.mutate(anc, 0.01, 77), k))  # the incremental insertion: a new genome and more k-mers for genome 3
    return anc, per, extra


def _index(k, ngen):
    anc, per, _ = _inputs(k, ngen)
    t, gt = BFT(k), Truth(k)
    for g, km in enumerate(per):
        t.insert_kmers(km, g)
        gt.add(km, g)
    t.build()
    return t, gt, anc


def _queries(gt, n, seed):
    """n k-mers: stored ones, SNP mutants of stored ones (mostly absent, near misses) and random ones, shuffled"""
    gt._make()
    rng = np.random.default_rng(seed)
    a = gt.kmers[rng.integers(0, len(gt.kmers), n)]
    b = S.snp_mutants(gt.kmers[rng.integers(0, len(gt.kmers), n)], gt.k, seed + 1)
    c = S.pack_codes(rng.integers(0, 4, (n, gt.k), dtype=np.uint8))
    src = rng.choice(3, n, p=[0.55, 0.35, 0.1])
    return np.ascontiguousarray(np.where(src[:, None] == 0, a, np.where(src[:, None] == 1, b, c)))


def _host_colors(t, q, cap):
    """bft_gpu_query_colors with the capacity given (BFT.query_colors retries on a count it learns: one C call here)"""
    n = len(q)
    bits = np.zeros((n + 7) // 8, np.uint8)
    off = np.zeros(n + 1, np.uint64)
    ids = np.zeros(max(cap, 1), np.uint32)
    need = C.c_uint64()
    _lib.check(t._lib.bft_gpu_query_colors(t._h, q.ctypes.data, n, bits.ctypes.data, off.ctypes.data, ids.ctypes.data, cap, C.byref(need)))
    return bits, off, ids[:int(need.value)]


def _sync():
    import torch
    torch.cuda.synchronize()


# ---- 2a: host and device id-list calls alternating on one handle --------------------------------------------------------------------
@pytest.mark.parametrize("k,ngen", INDEXES)
def test_id_lists_alternating_host_and_device(k, ngen):
    """query_colors (three launches, a library scan on qc_tmp) and query_colors_dev (one launch through the k-mer hash, k_colors_kh with scratch
    of its own; or the walk and the scan) in the orders H D H D H and D H D H D, then device calls through the walk (walk_hash 1 / 0, kmer_hash
    0 / 1).  Sizes around the scan's single tile (n + 1 <= 4096) and k_colors_kh's tile (1024), largest first: every later call reuses the
    blocks the earlier ones grew.  Every call: presence, offsets[n + 1] and ids against ground truth; device calls also d_needed and a capacity
    that is too small (through the k-mer hash the first ids and not one more, through the walk nothing)."""
    import torch
    t, gt, _ = _index(k, ngen)
    big = _queries(gt, SIZES_2A[0], 5)
    log = []

    def host(q, eb, eoff, eids):
        log.append(("H", len(q)))
        b, off, ids = _host_colors(t, q, len(eids) + 8)
        assert (b == eb).all(), log
        assert (off == eoff).all(), log
        assert (ids == eids).all(), log

    def dev(q, eb, eoff, eids, kh):
        n = len(q)
        log.append(("D", n, "kh" if kh else "walk"))
        dq = torch.from_numpy(q).cuda()
        bits = torch.zeros(((n + 63) // 64) * 8, dtype=torch.uint8, device="cuda")
        off = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
        need = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        small = torch.full((24,), -1, dtype=torch.int32, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        t.query_colors_dev(dq.data_ptr(), n, bits.data_ptr(), off.data_ptr(), small.data_ptr(), 16, need.data_ptr(), stream)
        _sync()
        assert int(need.item()) == len(eids), log
        assert (off.cpu().numpy().view(np.uint64) == eoff).all(), log
        sm = small.cpu().numpy().view(np.uint32)
        if len(eids) > 16:
            assert (sm[:16] == eids[:16]).all() if kh else bool((small[:16] == -1).all()), log
        assert bool((small[16:] == -1).all()), log  # never past the capacity
        ids = torch.full((len(eids) + 8,), -1, dtype=torch.int32, device="cuda")
        off.fill_(-1)
        need.fill_(-1)
        bits.fill_(0xFF)
        t.query_colors_dev(dq.data_ptr(), n, bits.data_ptr(), off.data_ptr(), ids.data_ptr(), len(eids) + 8, need.data_ptr(), stream)
        _sync()
        assert (bits.cpu().numpy()[: len(eb)] == eb).all(), log
        assert (off.cpu().numpy().view(np.uint64) == eoff).all(), log
        assert int(need.item()) == len(eids), log
        got = ids.cpu().numpy().view(np.uint32)
        assert (got[: len(eids)] == eids).all() and (got[len(eids):] == 0xFFFFFFFF).all(), log

    for n in SIZES_2A:
        q = np.ascontiguousarray(big[:n])
        exp = gt.colors(q)
        for order in ("HDHDH", "DHDHD"):
            for c in order:
                host(q, *exp) if c == "H" else dev(q, *exp, kh=True)
        t.set_option("walk_hash", 1)  # the walk, which looks plain root groups up in the k-mer hash
        dev(q, *exp, kh=False)
        host(q, *exp)
        dev(q, *exp, kh=False)
        t.set_option("walk_hash", 0)
        dev(q, *exp, kh=True)
        t.set_option("kmer_hash", 0)  # the walk alone
        dev(q, *exp, kh=False)
        host(q, *exp)
        t.set_option("kmer_hash", 1)
        dev(q, *exp, kh=True)
        host(q, *exp)
    t.close()


# ---- 2b: a seeded schedule over every query entry point ----------------------------------------------------------------------------
ENTRIES = ("presence", "presence_dev", "colors", "colors_dev", "color_rows", "color_rows_dev", "rows", "branching", "branching_dev",
           "sequences", "sequences_dev", "prefixes", "prefixes_dev", "subgraph")
CAP = {"branching": 70000, "branching_dev": 70000, "sequences": 20000, "sequences_dev": 20000, "prefixes": 70000, "prefixes_dev": 70000, "subgraph": 20000}


class _Extract:
    """extract() of the handle and what the checks derive from it (refreshed after every build)"""

    def __init__(self, t, gt):
        gt._make()
        self.kmers, self.cs = t.extract()
        keys = S.row_keys(self.kmers)
        assert sorted(keys.tolist()) == sorted(S.row_keys(gt.kmers).tolist())  # the handle stores exactly the inserted k-mers
        self.order = np.argsort(keys)
        self.keys_sorted = keys[self.order]
        self.codes = S.unpack_codes(self.kmers, gt.k)
        self.sets = {}  # colour-set id -> packed row of its genomes
        self.by_len = {}

    def rows_of(self, packed):
        """row of every k-mer in extract() order, -1 when absent"""
        q = S.row_keys(np.ascontiguousarray(packed))
        if len(q) == 0:
            return np.zeros(0, np.int64)
        pos = np.minimum(np.searchsorted(self.keys_sorted, q), len(self.keys_sorted) - 1)
        return np.where(self.keys_sorted[pos] == q, self.order[pos], -1)

    def set_rows(self, t, ids, rowbytes):
        for c in np.unique(ids).tolist():
            if c not in self.sets:
                r = np.zeros(rowbytes * 8, bool)
                r[t.colorset(c)] = True
                self.sets[c] = np.packbits(r, bitorder="little")
        return np.stack([self.sets[c] for c in ids.tolist()]) if len(ids) else np.zeros((0, rowbytes), np.uint8)

    def prefixes(self, pcodes, lens):
        """brute force over the extracted k-mers: (offsets [n + 1], rows in extract() order)"""
        n = len(lens)
        lo, cnt = np.zeros(n, np.int64), np.zeros(n, np.int64)
        for L in np.unique(lens).tolist():
            if L not in self.by_len:
                key = (self.codes[:, :L].astype(np.uint64) << (2 * np.arange(L, dtype=np.uint64))).sum(axis=1, dtype=np.uint64)
                o = np.argsort(key, kind="stable")  # (equal prefixes: ascending rows)
                self.by_len[L] = (key[o], o)
            ks, _ = self.by_len[L]
            sel = np.flatnonzero(lens == L)
            pk = (pcodes[sel, :L].astype(np.uint64) << (2 * np.arange(L, dtype=np.uint64))).sum(axis=1, dtype=np.uint64)
            a, b = np.searchsorted(ks, pk, "left"), np.searchsorted(ks, pk, "right")
            lo[sel], cnt[sel] = a, b - a
        off = np.zeros(n + 1, np.uint64)
        off[1:] = np.cumsum(cnt)
        rows = np.zeros(int(off[-1]), np.int64)
        for L in np.unique(lens).tolist():
            sel = np.flatnonzero(lens == L)
            _, o = self.by_len[L]
            for i in sel[cnt[sel] > 0]:
                rows[int(off[i]):int(off[i + 1])] = o[lo[i]:lo[i] + cnt[i]]
        return off, rows


@pytest.mark.parametrize("k,ngen,seed,ncalls", [(27, 130, 11, 80), (63, 20, 12, 40)])
def test_seeded_schedule_over_every_entry_point(k, ngen, seed, ncalls):
    """A fixed-seed schedule of calls over every query entry point of one handle: on the handle's stream or on one of two caller streams,
    after random kmer_hash / walk_hash / query_dynamic toggles, batch sizes around every threshold of the kernels (scan tile, k_colors_kh tile,
    query_dynamic_min) from 1 to ~2e5 in any order -- large after small too -- and one incremental insert + build half-way (which resets the
    derived colour-row dictionary and the table).  Every answer against ground truth; a failure names the seed, the call and the calls so far."""
    import torch
    t, gt, anc = _index(k, ngen)
    _, _, extra = _inputs(k, ngen)
    rng = np.random.default_rng(seed)
    streams = [None, torch.cuda.Stream(), torch.cuda.Stream()]
    opts = {"kmer_hash": 1, "walk_hash": 0, "query_dynamic": 1}
    ex = _Extract(t, gt)
    log = []
    genomes = [S.mutate(anc, 0.002, 1000 + k + 10 + g) if g else anc for g in range(4)]

    def where():
        return f"seed {seed}, call {len(log) - 1}: {log[-1]}; calls so far: {log[:-1]}"

    def call_dev(st, fn):
        """a device call on stream st (None: the handle's own); everything before it and after it is drained (no test of ordering here)"""
        _sync()
        if st is None:
            fn(None)
        else:
            with torch.cuda.stream(st):
                fn(st.cuda_stream)
        _sync()

    def dq_of(q):
        return torch.from_numpy(q).cuda()

    for i in range(ncalls):
        if i == ncalls // 2:  # incremental insertion: a new genome, more k-mers for genome 3
            g_new = gt.genomes
            t.insert_kmers(extra, g_new)
            t.insert_kmers(extra[::3], 3)
            gt.add(extra, g_new)
            gt.add(extra[::3], 3)
            t.build()
            ex = _Extract(t, gt)
            log.append(("insert+build", g_new))
        for name in opts:
            if rng.random() < 0.3:
                opts[name] ^= 1
                t.set_option(name, opts[name])
        entry = ENTRIES[int(rng.integers(len(ENTRIES)))]
        n = int(SIZES_2B[int(rng.integers(len(SIZES_2B)))])
        n = min(n, CAP.get(entry, n))
        si = int(rng.integers(3))
        st = streams[si]
        log.append((entry, n, "handle stream" if si == 0 else f"stream {si}", dict(opts)))
        G = gt.genomes
        rb = (G + 7) // 8
        if entry in ("sequences", "sequences_dev"):
            starts = rng.integers(0, GENOME_LEN - 200, n)
            lens = rng.integers(k, k + 40, n)
            src = rng.integers(0, 4, n)
            reads = [genomes[s][a:a + m] for s, a, m in zip(src, starts, lens)]
            thr = float(rng.choice([0.3, 0.5, 0.8, 1.0]))
            want = gt.sequences(reads, thr)
            asc = [bytes(S._ASCII[r]).decode() for r in reads]
            if entry == "sequences":
                assert t.query_sequences(asc, thr) == want, where()
            else:
                enc = [r.encode() for r in asc]
                off = np.zeros(n + 1, np.int64)
                off[1:] = np.cumsum([len(e) for e in enc])
                d_blob = torch.from_numpy(np.frombuffer(b"".join(enc), dtype=np.uint8).copy()).cuda()
                d_off = torch.from_numpy(off).cuda()
                d_rows = torch.full((n, rb), 0xAB, dtype=torch.uint8, device="cuda")
                call_dev(st, lambda s: t.query_sequences_dev(d_blob.data_ptr(), d_off.data_ptr(), n, int(off[-1]), thr, d_rows.data_ptr(), False, s))
                unp = np.unpackbits(d_rows.cpu().numpy(), axis=1, bitorder="little")
                assert not unp[:, G:].any(), where()
                assert [np.flatnonzero(r).tolist() for r in unp[:, :G]] == want, where()
            continue
        if entry in ("prefixes", "prefixes_dev"):
            pq = _queries(gt, n, int(rng.integers(1 << 30)))
            plen = rng.integers(min(k, 10), min(k, 31) + 1, n).astype(np.uint8)
            eoff, erows = ex.prefixes(S.unpack_codes(pq, k), plen)
            if entry == "prefixes":
                off, km, rows, sets = t.query_prefixes(pq, plen)
            else:
                m = int(eoff[-1])
                d_p, d_l = dq_of(pq), torch.from_numpy(plen).cuda()
                d_off = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
                d_k = torch.zeros((m + 1, pq.shape[1]), dtype=torch.uint8, device="cuda")
                d_r = torch.full((m + 1,), -1, dtype=torch.int32, device="cuda")
                d_c = torch.full((m + 1,), -1, dtype=torch.int32, device="cuda")
                d_n = torch.full((1,), -1, dtype=torch.int64, device="cuda")
                call_dev(st, lambda s: t.query_prefixes_dev(d_p.data_ptr(), d_l.data_ptr(), n, d_off.data_ptr(), d_k.data_ptr(), d_r.data_ptr(), d_c.data_ptr(),
                                                            m + 1, d_n.data_ptr(), s))
                assert int(d_n.item()) == m, where()
                off = d_off.cpu().numpy().view(np.uint64)
                km, rows, sets = d_k.cpu().numpy()[:m], d_r.cpu().numpy().view(np.uint32)[:m], d_c.cpu().numpy().view(np.uint32)[:m]
            assert (off == eoff).all(), where()
            assert (rows.astype(np.int64) == erows).all(), where()
            assert (km == ex.kmers[erows]).all() and (sets == ex.cs[erows]).all(), where()
            continue
        q = _queries(gt, n, int(rng.integers(1 << 30)))
        idx = gt.lookup(q)
        ebits = S.to_bits(idx >= 0)
        nbits = (n + 7) // 8
        if entry == "presence":
            assert (t.query_presence(q) == ebits).all(), where()
        elif entry == "presence_dev":
            dq, d_b = dq_of(q), torch.full((((n + 63) // 64) * 8,), 0xAB, dtype=torch.uint8, device="cuda")
            call_dev(st, lambda s: t.query_presence_dev(dq.data_ptr(), n, d_b.data_ptr(), s))
            assert (d_b.cpu().numpy()[:nbits] == ebits).all(), where()
        elif entry == "colors":
            eb, eoff, eids = gt.colors(q)
            b, off, ids = t.query_colors(q)
            assert (b == eb).all() and (off == eoff).all() and (ids == eids).all(), where()
        elif entry == "colors_dev":
            eb, eoff, eids = gt.colors(q)
            dq = dq_of(q)
            d_b = torch.full((((n + 63) // 64) * 8,), 0xAB, dtype=torch.uint8, device="cuda")
            d_off = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
            d_ids = torch.full((len(eids) + 4,), -1, dtype=torch.int32, device="cuda")
            d_n = torch.full((1,), -1, dtype=torch.int64, device="cuda")
            call_dev(st, lambda s: t.query_colors_dev(dq.data_ptr(), n, d_b.data_ptr(), d_off.data_ptr(), d_ids.data_ptr(), len(eids) + 4, d_n.data_ptr(), s))
            assert (d_b.cpu().numpy()[:nbits] == eb).all(), where()
            assert (d_off.cpu().numpy().view(np.uint64) == eoff).all() and int(d_n.item()) == len(eids), where()
            got = d_ids.cpu().numpy().view(np.uint32)
            assert (got[:len(eids)] == eids).all() and (got[len(eids):] == 0xFFFFFFFF).all(), where()
        elif entry == "color_rows":
            b, rows = t.query_color_rows(q)
            assert (b == ebits).all() and (rows == gt.rows(q, rb)).all(), where()
        elif entry == "color_rows_dev":
            dq = dq_of(q)
            d_b = torch.full((((n + 63) // 64) * 8,), 0xAB, dtype=torch.uint8, device="cuda")
            d_rows = torch.full((n, rb), 0xAB, dtype=torch.uint8, device="cuda")
            d_scr = torch.zeros(max(n, 1), dtype=torch.int32, device="cuda")
            call_dev(st, lambda s: t.query_color_rows_dev(dq.data_ptr(), n, d_b.data_ptr(), d_rows.data_ptr(), d_scr.data_ptr(), s))
            assert (d_b.cpu().numpy()[:nbits] == ebits).all(), where()
            assert (d_rows.cpu().numpy() == gt.rows(q, rb)).all(), where()
        elif entry == "rows":
            b, rows, sets = t.query_rows(q)
            assert (b == ebits).all(), where()
            present = idx >= 0
            assert (rows[~present] == 0xFFFFFFFF).all(), where()
            assert (rows[present].astype(np.int64) == ex.rows_of(q[present])).all(), where()  # the row of the k-mer in extract() order
            # the colour set, as the ids it stands for
            assert (ex.set_rows(t, sets[present], rb) == gt.rows(q[present], rb)).all(), where()
        elif entry in ("branching", "branching_dev"):
            ecnt, ebr = gt.branching(q)
            if entry == "branching":
                b, cnt = t.query_branching(q, with_counts=True)
            else:
                dq = dq_of(q)
                d_b = torch.full((((n + 63) // 64) * 8,), 0xAB, dtype=torch.uint8, device="cuda")
                d_c = torch.full((max(n, 1),), 0xAB, dtype=torch.uint8, device="cuda")
                call_dev(st, lambda s: t.query_branching_dev(dq.data_ptr(), n, d_b.data_ptr(), d_c.data_ptr(), s))
                b, cnt = d_b.cpu().numpy()[:nbits], d_c.cpu().numpy()[:n]
            assert (cnt == ecnt).all() and (b == ebr).all(), where()
        elif entry == "subgraph":
            sub, absent = t.subgraph(q)
            try:
                assert absent == int((idx < 0).sum()), where()
                # one query on the new handle: the stored part of the batch and its mutants, with the colour sets of the source
                keep = np.unique(idx[idx >= 0])
                sq = np.ascontiguousarray(np.concatenate([q[:200], S.snp_mutants(q[:200], k, i)]))
                in_sub = np.isin(gt.lookup(sq), keep)
                b, off, ids = sub.query_colors(sq)
                m = gt.members(gt.lookup(sq)) & in_sub[:, None]
                assert (b == S.to_bits(in_sub)).all(), where()
                assert (np.diff(off.astype(np.int64)) == m.sum(axis=1)).all() and (ids == np.nonzero(m)[1]).all(), where()
            finally:
                sub.close()
    t.close()


# ---- 2c: graph replays next to eager calls on the two colour blocks ----------------------------------------------------------------
def test_captured_kh_id_lists_replay_between_host_and_walk_calls():
    """query_colors_dev through the k-mer hash (k_colors_kh, block qc_kh) captured into a graph and replayed between eager calls at the same n:
    host query_colors (the scan, on qc_tmp) and device calls through the walk (walk_hash 1: the scan again).  Every replay and every eager
    call against ground truth.  No call between two replays may grow the captured block (none does: the eager calls use the scan's blocks)."""
    import torch
    k, ngen, n = 27, 130, 20000
    t, gt, _ = _index(k, ngen)
    batches = [_queries(gt, n, 40 + i) for i in range(3)]
    expect = [gt.colors(q) for q in batches]
    cap = max(len(e[2]) for e in expect) + 16
    dev = torch.device("cuda", 0)
    dq = torch.from_numpy(batches[0]).to(dev)
    bits = torch.zeros((n + 63) // 64 * 8, dtype=torch.uint8, device=dev)
    offs = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    ids = torch.zeros(cap, dtype=torch.int32, device=dev)
    need = torch.zeros(1, dtype=torch.int64, device=dev)
    s, s2 = torch.cuda.Stream(), torch.cuda.Stream()

    def check(b, off, idl, nd, e, what):
        eb, eoff, eids = e
        assert (b[: len(eb)] == eb).all(), what
        assert (off == eoff).all(), what
        assert nd == len(eids) and (idl[: len(eids)] == eids).all(), what

    def read():
        return (bits.cpu().numpy(), offs.cpu().numpy().view(np.uint64), ids.cpu().numpy().view(np.uint32), int(need.item()))

    def direct():
        with torch.cuda.stream(s):
            t.query_colors_dev(dq.data_ptr(), n, bits.data_ptr(), offs.data_ptr(), ids.data_ptr(), cap, need.data_ptr(), s.cuda_stream)
        s.synchronize()

    direct()  # scratch sized by a direct call: nothing allocates while the stream is captured
    check(*read(), expect[0], "direct")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        t.query_colors_dev(dq.data_ptr(), n, bits.data_ptr(), offs.data_ptr(), ids.data_ptr(), cap, need.data_ptr(), torch.cuda.current_stream().cuda_stream)
    direct()  # (an eager call behind the capture: the handle's event of the scratch is an eager one again)
    check(*read(), expect[0], "direct after capture")
    for rep in range(6):
        i = rep % 3
        dq.copy_(torch.from_numpy(batches[i]))
        offs.zero_(); ids.zero_(); bits.zero_(); need.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        check(*read(), expect[i], f"replay {rep}")
        if rep % 2 == 0:  # the host entry point: the scan on qc_tmp, at the same n
            check(*_host_colors(t, batches[i], cap), len(expect[i][2]), expect[i], f"host call after replay {rep}")
        else:  # a device call through the walk, on another stream, with buffers of its own
            t.set_option("walk_hash", 1)
            wq = torch.from_numpy(batches[i]).to(dev)
            wb = torch.zeros_like(bits); wo = torch.zeros_like(offs); wi = torch.zeros_like(ids); wn = torch.zeros_like(need)
            torch.cuda.synchronize()
            with torch.cuda.stream(s2):
                t.query_colors_dev(wq.data_ptr(), n, wb.data_ptr(), wo.data_ptr(), wi.data_ptr(), cap, wn.data_ptr(), s2.cuda_stream)
            torch.cuda.synchronize()
            check(wb.cpu().numpy(), wo.cpu().numpy().view(np.uint64), wi.cpu().numpy().view(np.uint32), int(wn.item()), expect[i], f"walk call after replay {rep}")
            t.set_option("walk_hash", 0)
    del g
    t.close()


# ---- 2d: kernel_time counts every query entry point --------------------------------------------------------------------------------
FORMS = {"kmer_hash": {"kmer_hash": 1, "walk_hash": 0}, "walk_hash": {"kmer_hash": 1, "walk_hash": 1}, "walk": {"kmer_hash": 0, "walk_hash": 0}}


@pytest.mark.parametrize("form", list(FORMS))
def test_kernel_time_counts_every_query_entry_point(form):
    """With timing on, one call of every host and device query entry point adds timed launches (kernel_time: launches >= 1, ms > 0) -- the
    one-launch colour rows of the k-mer hash, the row kernels, the sequence path and the id-list fill included.  Where a call makes several
    timed launches (query, then rows or ids; the sequence path's encode, plan, lookups and tally) the count says so."""
    import torch
    k, ngen, n = 27, 130, 5000
    t, gt, anc = _index(k, ngen)
    for name, v in FORMS[form].items():
        t.set_option(name, v)
    q = _queries(gt, n, 90)
    _, _, eids = gt.colors(q)
    rb = (gt.genomes + 7) // 8
    dq = torch.from_numpy(q).cuda()
    d_b = torch.zeros(((n + 63) // 64) * 8, dtype=torch.uint8, device="cuda")
    d_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    d_ids = torch.zeros(len(eids) + 4, dtype=torch.int32, device="cuda")
    d_n = torch.zeros(1, dtype=torch.int64, device="cuda")
    d_rows = torch.zeros((n, rb), dtype=torch.uint8, device="cuda")
    d_scr = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_cnt = torch.zeros(n, dtype=torch.uint8, device="cuda")
    asc = [bytes(S._ASCII[anc[a:a + 60]]).decode() for a in range(0, 30000, 300)]
    enc = b"".join(x.encode() for x in asc)
    soff = np.arange(len(asc) + 1, dtype=np.int64) * 60
    d_blob = torch.from_numpy(np.frombuffer(enc, dtype=np.uint8).copy()).cuda()
    d_soff = torch.from_numpy(soff).cuda()
    d_srows = torch.zeros((len(asc), rb), dtype=torch.uint8, device="cuda")
    plen = np.full(n, 12, np.uint8)
    d_pl = torch.from_numpy(plen).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    kh = form == "kmer_hash"
    calls = {  # entry point -> (call, the timed launches it makes at least)
        "presence": (lambda: t.query_presence(q), 1),
        "presence_dev": (lambda: t.query_presence_dev(dq.data_ptr(), n, d_b.data_ptr(), stream), 1),
        "colors": (lambda: _host_colors(t, q, len(eids)), 2),  # lookups, id fill
        "colors_dev": (lambda: t.query_colors_dev(dq.data_ptr(), n, d_b.data_ptr(), d_off.data_ptr(), d_ids.data_ptr(), len(eids) + 4, d_n.data_ptr(), stream),
                       1 if kh else 2),  # one launch through the k-mer hash; lookups and id fill through the walk
        "color_rows": (lambda: t.query_color_rows(q), 2),  # lookups, rows
        "color_rows_dev": (lambda: t.query_color_rows_dev(dq.data_ptr(), n, d_b.data_ptr(), d_rows.data_ptr(), d_scr.data_ptr(), stream), 1 if kh else 2),
        "rows": (lambda: t.query_rows(q), 1),
        "branching": (lambda: t.query_branching(q, with_counts=True), 1),
        "branching_dev": (lambda: t.query_branching_dev(dq.data_ptr(), n, d_b.data_ptr(), d_cnt.data_ptr(), stream), 1),
        "sequences": (lambda: t.query_sequences(asc, 0.5), 4),  # encode, plan, lookups, tally
        "sequences_dev": (lambda: t.query_sequences_dev(d_blob.data_ptr(), d_soff.data_ptr(), len(asc), len(enc), 0.5, d_srows.data_ptr(), False, stream), 4),
        "prefixes": (lambda: t.query_prefixes(q, plen), 1),
        "prefixes_dev": (lambda: t.query_prefixes_dev(dq.data_ptr(), d_pl.data_ptr(), n, d_off.data_ptr(), 0, 0, 0, 0, d_n.data_ptr(), stream), 1),
        "subgraph": (lambda: t.subgraph(q[:2000])[0].close(), 1),
    }
    for name, (fn, at_least) in calls.items():
        fn()  # (warm: the first call may derive what the entry point needs -- colour-row dictionary, table -- outside the count)
        _sync()
        t.kernel_time(reset=True)
        fn()
        _sync()
        ms, launches = t.kernel_time(reset=True)
        assert launches >= at_least and ms > 0, (form, name, launches, ms)
    t.close()


# ---- 2e: the scratch owner's policy (HandleScratch, bft_handle.h) ------------------------------------------------------------------------
def _hip_runtime():
    """the HIP runtime this process already has loaded (torch's): raw streams, which can be destroyed"""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return C.CDLL(line.split()[-1])
    raise RuntimeError("no libamdhip64 mapped")


def test_sequence_queries_after_their_last_stream_is_destroyed():
    """Sequence queries on a stream made with hipStreamCreate, used once, synchronised and DESTROYED; then on another stream and on the handle's own.
    The scratch's last user is gone by the second call: the handle waits on an event of its own, never on that stream.  Every call returns
    BFT_GPU_OK (the wrapper raises otherwise) and every answer equals ground truth."""
    import torch
    hip = _hip_runtime()
    k, ngen, n, thr = 27, 130, 3000, 0.5
    t, gt, anc = _index(k, ngen)
    genomes = [S.mutate(anc, 0.002, 1000 + k + 10 + g) if g else anc for g in range(4)]
    rb = (gt.genomes + 7) // 8

    def ask(stream, seed):
        rng = np.random.default_rng(seed)
        reads = [genomes[s][a:a + m] for s, a, m in zip(rng.integers(0, 4, n), rng.integers(0, GENOME_LEN - 200, n), rng.integers(k, k + 40, n))]
        enc = [bytes(S._ASCII[r]) for r in reads]
        off = np.zeros(n + 1, np.int64)
        off[1:] = np.cumsum([len(e) for e in enc])
        d_blob = torch.from_numpy(np.frombuffer(b"".join(enc), dtype=np.uint8).copy()).cuda()
        d_off = torch.from_numpy(off).cuda()
        d_rows = torch.full((n, rb), 0xAB, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        t.query_sequences_dev(d_blob.data_ptr(), d_off.data_ptr(), n, int(off[-1]), thr, d_rows.data_ptr(), False, stream)
        return reads, d_rows

    def check(reads, d_rows, what):
        unp = np.unpackbits(d_rows.cpu().numpy(), axis=1, bitorder="little")
        assert not unp[:, gt.genomes:].any(), what
        assert [np.flatnonzero(r).tolist() for r in unp[:, :gt.genomes]] == gt.sequences(reads, thr), what

    st = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(st)) == 0
    reads, d_rows = ask(st.value, 1)
    assert hip.hipStreamSynchronize(st) == 0
    assert hip.hipStreamDestroy(st) == 0
    check(reads, d_rows, "on the stream that was destroyed afterwards")
    s2 = torch.cuda.Stream()
    with torch.cuda.stream(s2):
        reads, d_rows = ask(s2.cuda_stream, 2)
    s2.synchronize()
    check(reads, d_rows, "on a second stream")
    reads, d_rows = ask(None, 3)
    _sync()
    check(reads, d_rows, "on the handle's stream")
    t.close()


def _replay_between_streams(call, read, want):
    """call(stream) direct on stream A, captured on A, replayed twice, eager on stream B, replayed again: read() after each of the four equals
    want (checked for the direct call too).  A recorded call leaves no event of the handle's inside the graph, so the eager call on B neither
    fails nor waits on one."""
    import torch
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(sa):
        call(sa.cuda_stream)
    sa.synchronize()
    want(read(), "direct")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=sa):
        call(torch.cuda.current_stream().cuda_stream)
    for what in ("replay 1", "replay 2", "eager on another stream", "replay 3"):
        read(clear=True)
        torch.cuda.synchronize()
        if what.startswith("replay"):
            g.replay()
        else:
            with torch.cuda.stream(sb):
                call(sb.cuda_stream)
        torch.cuda.synchronize()
        want(read(), what)
    del g


def test_recorded_id_lists_and_prefixes_between_eager_calls_on_another_stream():
    """An id-list call recorded on stream A after one direct call of that size, replayed twice, the same call eager on stream B, a replay again;
    the same for the prefix call.  All against ground truth (id lists) / brute force over extract() (prefixes)."""
    import torch
    k, ngen, n = 27, 130, 20000
    t, gt, _ = _index(k, ngen)
    q = _queries(gt, n, 61)
    eb, eoff, eids = gt.colors(q)
    cap = len(eids) + 16
    dq = torch.from_numpy(q).cuda()
    bits = torch.zeros((n + 63) // 64 * 8, dtype=torch.uint8, device="cuda")
    offs = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    ids = torch.zeros(cap, dtype=torch.int32, device="cuda")
    need = torch.zeros(1, dtype=torch.int64, device="cuda")

    def read(clear=False):
        if clear:
            bits.zero_(); offs.zero_(); ids.zero_(); need.zero_()
            return None
        return bits.cpu().numpy(), offs.cpu().numpy().view(np.uint64), ids.cpu().numpy().view(np.uint32), int(need.item())

    def want(got, what):
        b, off, idl, nd = got
        assert (b[: len(eb)] == eb).all() and (off == eoff).all(), what
        assert nd == len(eids) and (idl[: len(eids)] == eids).all(), what

    _replay_between_streams(lambda s: t.query_colors_dev(dq.data_ptr(), n, bits.data_ptr(), offs.data_ptr(), ids.data_ptr(), cap, need.data_ptr(), s), read, want)

    ex = _Extract(t, gt)
    plen = np.random.default_rng(62).integers(10, 28, n).astype(np.uint8)
    poff, prow = ex.prefixes(S.unpack_codes(q, k), plen)
    m = int(poff[-1])
    d_l = torch.from_numpy(plen).cuda()
    d_k = torch.zeros((m + 1, q.shape[1]), dtype=torch.uint8, device="cuda")
    d_r = torch.zeros(m + 1, dtype=torch.int32, device="cuda")
    d_c = torch.zeros(m + 1, dtype=torch.int32, device="cuda")

    def pread(clear=False):
        if clear:
            offs.zero_(); d_k.zero_(); d_r.zero_(); d_c.zero_(); need.zero_()
            return None
        return offs.cpu().numpy().view(np.uint64), d_k.cpu().numpy()[:m], d_r.cpu().numpy().view(np.uint32)[:m], d_c.cpu().numpy().view(np.uint32)[:m], int(need.item())

    def pwant(got, what):
        off, km, rows, sets, nd = got
        assert nd == m and (off == poff).all() and (rows.astype(np.int64) == prow).all(), what
        assert (km == ex.kmers[prow]).all() and (sets == ex.cs[prow]).all(), what

    _replay_between_streams(lambda s: t.query_prefixes_dev(dq.data_ptr(), d_l.data_ptr(), n, offs.data_ptr(), d_k.data_ptr(), d_r.data_ptr(), d_c.data_ptr(),
                                                           m + 1, need.data_ptr(), s), pread, pwant)
    t.close()


def test_recorded_id_list_call_that_would_grow_the_scratch_is_refused():
    """An id-list call LARGER than any direct call before it, made while its stream is being captured, returns BFT_GPU_E_ARG (nothing may allocate in
    a capture) and records nothing; the test ends the capture itself and replays nothing from it.  A direct call of that size is then answered
    correctly."""
    import torch
    k, ngen, n_small, n_big = 27, 130, 5000, 60000
    t, gt, _ = _index(k, ngen)
    q = _queries(gt, n_big, 63)
    eb, eoff, eids = gt.colors(q)
    cap = len(eids) + 16
    dq = torch.from_numpy(q).cuda()
    bits = torch.zeros((n_big + 63) // 64 * 8, dtype=torch.uint8, device="cuda")
    offs = torch.zeros(n_big + 1, dtype=torch.int64, device="cuda")
    ids = torch.zeros(cap, dtype=torch.int32, device="cuda")
    need = torch.zeros(1, dtype=torch.int64, device="cuda")
    s = torch.cuda.Stream()

    def raw(n, stream):
        return t._lib.bft_gpu_query_colors_dev(t._h, C.c_void_p(dq.data_ptr()), n, C.c_void_p(bits.data_ptr()), C.c_void_p(offs.data_ptr()),
                                               C.c_void_p(ids.data_ptr()), cap, C.c_void_p(need.data_ptr()), C.c_void_p(stream))

    with torch.cuda.stream(s):
        assert raw(n_small, s.cuda_stream) == 0
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        need.zero_()  # (the recorded graph is not empty)
        rc = raw(n_big, torch.cuda.current_stream().cuda_stream)
        msg = t._lib.bft_gpu_last_error()
    del g  # (never replayed)
    assert rc == -1, rc  # BFT_GPU_E_ARG
    assert b"make one direct call of this size first" in msg, msg
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        assert raw(n_big, s.cuda_stream) == 0
    s.synchronize()
    assert (bits.cpu().numpy()[: len(eb)] == eb).all() and (offs.cpu().numpy().view(np.uint64) == eoff).all()
    assert int(need.item()) == len(eids) and (ids.cpu().numpy().view(np.uint32)[: len(eids)] == eids).all()
    t.close()


# ---- 2f: the tuner gives back what it borrows ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [27, 63])
def test_tune_leaves_the_handle_as_it_found_it(k):
    """set_option("tune", 1) measures candidate launch shapes of the container walk on the image (an index of at least 2^16 k-mers: below that
    the tuner returns before it measures).  It does not time itself (kernel_time's launch count stands still over the tune), it leaves timing on
    (a query after it is counted as one before it was), it respects the options the caller fixed (query_wgs_per_cu, query_probe), and the
    answers of presence, rows, branching and sequence queries are the same before and after -- through the walk and, at the end, through the
    k-mer hash with walk_hash."""
    g = S.random_genome(75000, 300 + k)
    km = S.distinct(S.kmers_of(g, k))
    t = BFT(k)
    t.insert_kmers(km, 0)
    t.insert_kmers(km[::2], 1)
    t.insert_kmers(km[::3], 2)
    t.build()
    assert t.info()["kmers"] >= 65536
    t.set_option("kmer_hash", 0)  # the walk answers
    t.set_option("timing", 1)
    q = np.ascontiguousarray(np.concatenate([km[:5000], S.snp_mutants(km[5000:10000], k, 7)]))
    reads = [bytes(S._ASCII[g[a:a + 200]]).decode() for a in range(1000, 71000, 7000)]
    assert len(reads) == 10

    def answers():
        bits, rows, sets = t.query_rows(q)
        br, cnt = t.query_branching(q[:2000], with_counts=True)
        return t.query_presence(q), bits, rows, sets, br, cnt, t.query_sequences(reads, 0.5)

    def same(a, b, what):
        for i, (x, y) in enumerate(zip(a[:-1], b[:-1])):
            assert (x == y).all(), (what, i)
        assert a[-1] == b[-1], what

    ref = answers()
    assert S.from_bits(ref[0], len(q))[:5000].all() and (ref[0] == ref[1]).all()
    _, l0 = t.kernel_time(reset=False)
    t.query_presence(q)
    _, l1 = t.kernel_time(reset=False)
    per_call = l1 - l0
    assert per_call >= 1
    t.set_option("query_wgs_per_cu", 1)
    if k == 27:
        t.set_option("query_probe", 8)
    t.set_option("tune", 1)
    _, l2 = t.kernel_time(reset=False)
    assert l2 == l1  # the tuner does not time itself
    bt = t.build_time()
    assert bt["query_wgs_per_cu"] == 1.0
    if k == 27:
        assert bt["query_probe_rows"] == 8.0
    t.query_presence(q)
    _, l3 = t.kernel_time(reset=False)
    assert l3 - l2 == per_call  # timing is still on
    same(answers(), ref, "after a tune with the shape fixed by options")
    t.set_option("query_wgs_per_cu", 0)
    t.set_option("query_probe", 0)
    t.set_option("tune", 1)
    assert t.build_time()["query_wgs_per_cu"] in (1.0, 2.0, 3.0)
    same(answers(), ref, "after a free tune")
    t.set_option("kmer_hash", 1)
    t.set_option("walk_hash", 1)
    same(answers(), ref, "through the k-mer hash and walk_hash")
    t.close()
