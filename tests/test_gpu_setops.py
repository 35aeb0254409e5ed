"""Colour-set algebra over groups of k-mers on the GPU (bft_gpu_combine_colors / _dev, bft_gpu_combine_colorsets / _dev, BFT.combine_colors,
BFT.combine_colorsets) against ground truth: the genome set of every k-mer of a batch comes from the inserted (k-mer string -> genome set) map, and the
AND / OR / SYMDIFF of a group is set algebra over those sets (as counts per genome: a genome is in the AND when every member that counts holds it, in the
OR when one does).  The product is never its own reference.  Every case is checked over all groups of its batch, every output lies between 0xAA canaries,
and the three outputs are also asked for one at a time."""
import ctypes as C

import numpy as np
import pytest

from bloomfiltertrie_amd import BFT, _lib, synth as S

from test_gpu_components import _owners_of

pytestmark = pytest.mark.gpu

AND, OR, SYMDIFF = 0, 1, 2
OPS = {AND: "and", OR: "or", SYMDIFF: "symdiff"}
E_ARG = -1
ABSENT = 0xFFFFFFFF
PAD = 64  # canary bytes on either side of an output


class Pool:
    """An index, and a pool of k-mers to draw batches from: packed [P, B], M [P, G] = the genomes of each (all False: the index does not store it)."""

    def __init__(self, t, owners, packed):
        self.t, self.owners, self.packed = t, owners, np.ascontiguousarray(packed)
        t.build()  # (the genome count is the image's)
        self.G = int(t.info()["genomes"])
        self.M = np.zeros((len(packed), self.G), dtype=bool)
        for i, s in enumerate(S.packed_to_ascii(self.packed, t.k)):
            for g in owners.get(s, ()):
                self.M[i, g] = True
        self.present = self.M.any(axis=1)

    def truth(self, idx, off, op, skip):
        """(rows bool [ng, G], counts, found) for the batch pool[idx] grouped by off"""
        off = np.asarray(off, dtype=np.int64)
        m = self.M[idx].astype(np.int32)
        cs = np.concatenate([np.zeros((1, self.G), np.int32), np.cumsum(m, axis=0, dtype=np.int32)])
        cp = np.concatenate([[0], np.cumsum(self.present[idx])])
        a, e = off[:-1], off[1:]
        cnt = cs[e] - cs[a]
        found = cp[e] - cp[a]
        neff = (found if skip else e - a)[:, None]
        all_, any_ = (cnt == neff) & (neff > 0), cnt > 0
        rows = all_ if op == AND else any_ if op == OR else np.where(neff == 1, any_, any_ & ~all_)
        return rows, rows.sum(axis=1), found


def _pack(rows):
    return np.packbits(rows, axis=1, bitorder="little") if rows.shape[1] else np.zeros((len(rows), 0), np.uint8)


def _canary(nbytes):
    return np.full(nbytes + 2 * PAD, 0xAA, dtype=np.uint8)


def _intact(buf, nbytes):
    return bool((buf[:PAD] == 0xAA).all() and (buf[PAD + nbytes:] == 0xAA).all())


def _raw(t, kmers, off, op, skip, want=(True, True, True), colorsets=None):
    """one host call; returns (rc, rows bytes or None, counts or None, found or None); the canaries around every output are checked here"""
    lib = _lib.load()
    off = np.ascontiguousarray(off, dtype=np.uint64)
    ng = len(off) - 1
    rb = (int(t.info()["genomes"]) + 7) // 8
    sizes = (ng * rb, ng * 4, ng * 4)
    bufs = [_canary(sz) for sz in sizes]
    ptrs = [b.ctypes.data + PAD if w else None for b, w in zip(bufs, want)]
    if colorsets is None:
        kmers = np.ascontiguousarray(kmers, dtype=np.uint8)
        rc = lib.bft_gpu_combine_colors(t._h, kmers.ctypes.data, len(kmers), off.ctypes.data, ng, op, skip, ptrs[0], ptrs[1], ptrs[2])
    else:
        cs = np.ascontiguousarray(colorsets, dtype=np.uint32)
        rc = lib.bft_gpu_combine_colorsets(t._h, cs.ctypes.data, len(cs), off.ctypes.data, ng, op, ptrs[0], ptrs[1])
    out = []
    for b, sz, w in zip(bufs, sizes, want):
        assert _intact(b, sz)
        if not w or rc != 0:
            assert (b == 0xAA).all()  # an output that was not asked for, or a refused call: nothing written
            out.append(None)
        else:
            out.append(b[PAD:PAD + sz].copy())
    rows = out[0].reshape(ng, rb) if out[0] is not None else None
    return rc, rows, None if out[1] is None else out[1].view(np.uint32), None if out[2] is None else out[2].view(np.uint32)


def _check(p, idx, off, ops=(AND, OR, SYMDIFF), skips=(0, 1), singly=False):
    idx = np.asarray(idx, dtype=np.int64)
    kmers = p.packed[idx] if len(idx) else np.zeros((0, p.t.nb), np.uint8)
    for op in ops:
        for skip in skips:
            wr, wc, wf = p.truth(idx, off, op, skip)
            rc, rows, counts, found = _raw(p.t, kmers, off, op, skip)
            assert rc == 0, _lib.load().bft_gpu_last_error()
            bad = np.nonzero((rows != _pack(wr)).any(axis=1))[0]
            assert len(bad) == 0, (OPS[op], skip, "first wrong groups", bad[:5], "of", len(wr))
            assert (counts == wc).all(), (OPS[op], skip)
            assert (found == wf).all(), (OPS[op], skip)
            if p.G % 8 and len(rows):  # the bits at and past G
                assert not (rows[:, -1] >> (p.G % 8)).any()
            if singly:
                for j in range(3):
                    one = _raw(p.t, kmers, off, op, skip, want=tuple(i == j for i in range(3)))
                    assert one[0] == 0 and (one[1 + j] == (rows, counts, found)[j]).all()


# ---- the 4-genome SNP family at every key width ------------------------------------------------------------------------------------------

def _snp_pool(k, seed, options=(), merges=False, genomes=4):
    rate = 0.01 if k < 63 else 0.002
    anc = S.random_genome(5000, seed + 1)
    gs = [anc] + [S.mutate(anc, rate, seed + 2 + g) for g in range(genomes - 1)]
    t = BFT(k, device=0)
    for name, v in options:
        t.set_option(name, v)
    lists, stored = [], []
    for gid, g in enumerate(gs):
        assert t.add_genome(f"g{gid}") == gid
        km = S.distinct(S.kmers_of(g, k))
        t.insert_kmers(km, gid)
        if merges:
            t.build()
        lists.append((S.packed_to_ascii(km, k), gid))
        stored.append(km)
    stored = S.distinct(np.concatenate(stored))
    rng = np.random.default_rng(seed)
    packed = np.concatenate([stored, S.snp_mutants(stored[::4], k, seed + 9), S.pack_codes(rng.integers(0, 4, (1000, k), dtype=np.uint8))])
    return t, _owners_of(lists), packed, len(stored)


_POOLS = {}


def _shared(k):
    """one index per key width, shared by the tests that only query it"""
    if k not in _POOLS:
        t, owners, packed, ns = _snp_pool(k, seed=k)
        _POOLS[k] = (Pool(t, owners, packed), ns)
    return _POOLS[k]


def _sized_batch(p, n_stored, seed):
    """groups of 0, 1, 2, 3, 63, 64, 65, 257, 5 000 and 70 000 members; empty groups at the start, in the middle and at the end; the 70 000 are the
    pool's stored k-mers repeated, the others mix stored k-mers, absent ones with a stored prefix and random ones"""
    rng = np.random.default_rng(seed)
    sizes = [0, 1, 2, 3, 0, 63, 64, 65, 257, 0, 5000, 70000, 1, 0]
    idx, off = [], [0]
    for s in sizes:
        if s == 70000:
            part = np.resize(np.arange(n_stored), s)
        elif s >= 63:
            part = np.where(rng.random(s) < 0.9, rng.integers(0, n_stored, s), rng.integers(0, len(p.packed), s))
        else:
            part = rng.integers(0, len(p.packed), s)
        idx.append(part)
        off.append(off[-1] + s)
    return np.concatenate(idx), off


@pytest.mark.parametrize("k", (9, 27, 31, 63, 126))
def test_every_group_size_op_and_absence_rule(k):
    p, ns = _shared(k)
    assert p.present[:ns].all() and (~p.present[ns:]).sum() >= 1000  # stored k-mers, and absent ones (near misses and random)
    idx, off = _sized_batch(p, ns, k)
    _check(p, idx, off, singly=(k == 27))
    # all-stored groups of every size, so that no AND is empty because of an absent member
    rng = np.random.default_rng(k + 1)
    idx2, off2 = [], [0]
    for s in (1, 2, 3, 17, 63, 64, 65, 257, 5000):
        start = int(rng.integers(0, ns - 40))
        idx2.append(start + rng.integers(0, 40 if s < 5000 else 8, s))  # neighbours in the genome: sets that overlap
        off2.append(off2[-1] + s)
    idx2 = np.concatenate(idx2)
    assert p.truth(idx2, off2, AND, 0)[1].max() > 0
    _check(p, idx2, off2)


def test_pairs_gaps_and_empty_batches():
    p, ns = _shared(27)
    rng = np.random.default_rng(5)
    n = 100000
    idx = np.where(rng.random(2 * n) < 0.8, rng.integers(0, ns, 2 * n), rng.integers(0, len(p.packed), 2 * n))
    _check(p, idx, np.arange(0, 2 * n + 1, 2))
    # groups that leave k-mers between them uncovered (and in front of the first, behind the last)
    idx = rng.integers(0, len(p.packed), 3000)
    starts = np.arange(5, 2900, 29)
    off = np.stack([starts, starts + rng.integers(0, 20, len(starts))], axis=1).reshape(-1)  # every other "group" is a gap
    wr = [p.truth(idx, off, op, 0) for op in (AND, OR, SYMDIFF)]
    for op in (AND, OR, SYMDIFF):
        rc, rows, counts, found = _raw(p.t, p.packed[idx], off, op, 0)
        assert rc == 0 and (rows == _pack(wr[op][0])).all() and (counts == wr[op][1]).all() and (found == wr[op][2]).all()
    # no group; groups over no k-mer
    assert _raw(p.t, p.packed[:7], [0], AND, 0)[0] == 0
    _check(p, [], [0, 0, 0], singly=True)
    lib = _lib.load()
    z = np.zeros(1, dtype=np.uint64)
    assert lib.bft_gpu_combine_colors(p.t._h, None, 0, z.ctypes.data, 0, OR, 0, None, None, None) == 0


def test_runs_of_one_colour_set():
    p, ns = _shared(27)
    sets = {}
    for i in range(ns):
        sets.setdefault(p.M[i].tobytes(), []).append(i)
    by_size = sorted(sets.values(), key=len, reverse=True)
    a, b = np.array(by_size[0]), np.array(by_size[1])
    assert len(a) >= 100 and len(b) >= 20 and (p.M[a[0]] != p.M[b[0]]).any()
    absent = np.nonzero(~p.present)[0]
    single = next(np.array(v) for v in by_size if p.M[v[0]].sum() == 1)
    other = next(np.array(v) for v in by_size if p.M[v[0]].sum() == 1 and (p.M[v[0]] != p.M[single[0]]).any())
    groups = [np.resize(a, 300),                                            # one colour set throughout
              np.stack([np.resize(a, 150), np.resize(b, 150)], 1).reshape(-1),  # two sets alternating
              np.concatenate([single[:1], other[:1], np.resize(absent, 40), np.resize(a, 40)]),  # the AND is empty at the second member
              np.concatenate([single[:1], other[:1], np.resize(absent, 8)])]
    off = np.concatenate([[0], np.cumsum([len(g) for g in groups])])
    idx = np.concatenate(groups)
    assert p.truth(idx, off, AND, 1)[1][2] == 0 and p.truth(idx, off, AND, 1)[2][2] == 42
    _check(p, idx, off)


# ---- row widths: hand-made indexes ---------------------------------------------------------------------------------------------------------

def _wide_pool(G, no_bitmaps=False, k=27):
    """G genomes over 600 k-mers: every third genome holds all of them (no AND is empty), the others each hold about half; half of the k-mers share
    one of 12 sets (runs), the others have a set of their own"""
    rng = np.random.default_rng(G)
    P = 600
    packed = S.distinct(S.pack_codes(rng.integers(0, 4, (P + 50, k), dtype=np.uint8)))[:P]
    classes = rng.random((12, G)) < 0.5
    own = rng.random((P, G)) < 0.5
    own[::2] = classes[(np.arange(P)[::2] // 2) % 12]
    own[:, ::3] = True
    own[-40:] = False  # k-mers no genome holds: absent
    t = BFT(k, device=0)
    if no_bitmaps:
        t.set_option("test_no_cs_bitmaps", 1)
    asc = S.packed_to_ascii(packed, k)
    lists = []
    for g in range(G):
        assert t.add_genome(f"g{g}") == g
        sel = np.nonzero(own[:, g])[0]
        t.insert_kmers(packed[sel], g)
        lists.append(([asc[i] for i in sel], g))
    t.build()
    p = Pool(t, _owners_of(lists), packed)
    assert p.G == G and (p.M == own).all()
    return p


def _wide_batch(p, seed):
    rng = np.random.default_rng(seed)
    sizes = [2, 3, 1, 0, 16, 17, 64, 65, 130, 700, 2, 2, 5]
    idx = [rng.integers(0, 560, s) for s in sizes]                # stored k-mers only
    idx += [rng.integers(0, 600, s) for s in (2, 9, 40, 300)]      # with absent ones
    ev = rng.integers(0, 280, 200)
    idx += [ev[np.argsort(ev % 12, kind="stable")] * 2]            # the k-mers that share one of the 12 sets, set by set: runs
    off = np.concatenate([[0], np.cumsum([len(g) for g in idx])])
    return np.concatenate(idx), off


@pytest.mark.parametrize("G", (1, 8, 9, 32, 33, 64, 65, 100, 128, 300, 2100))
def test_row_widths(G):
    p = _wide_pool(G)
    idx, off = _wide_batch(p, G)
    a, o, s = (p.truth(idx, off, op, 0)[1] for op in (AND, OR, SYMDIFF))
    assert a[:3].min() > 0 and (o >= a).all()  # no AND over stored k-mers is empty,
    if G > 1:
        assert (o[:3] > a[:3]).any() and s.max() > 0 and (s != o).any()  # and the three ops differ
    _check(p, idx, off, singly=(G == 100))
    if G in (9, 100, 300, 2100):  # the same bytes from the id lists
        with_bm = [_raw(p.t, p.packed[idx], off, op, skip) for op in (AND, OR, SYMDIFF) for skip in (0, 1)]
        assert p.t.footprint()["dictionary_bitmaps"] > 0
        q = _wide_pool(G, no_bitmaps=True)
        assert (q.packed == p.packed).all()
        lists = [_raw(q.t, q.packed[idx], off, op, skip) for op in (AND, OR, SYMDIFF) for skip in (0, 1)]
        assert q.t.footprint()["dictionary_bitmaps"] <= 8
        for x, y in zip(with_bm, lists):
            assert x[0] == y[0] == 0 and all((u == v).all() for u, v in zip(x[1:], y[1:]))
        _check(q, idx, off, ops=(SYMDIFF,))
        q.t.close()
    p.t.close()


# ---- colour-set ids as members -----------------------------------------------------------------------------------------------------------

def test_colorsets_from_rows_and_prefixes():
    p, ns = _shared(27)
    t = p.t
    idx, off = _sized_batch(p, ns, 77)
    kmers = p.packed[idx]
    _, _, sets = t.query_rows(kmers)
    assert (sets == ABSENT).any() and (sets != ABSENT).any()
    for op in (AND, OR, SYMDIFF):
        rc, rows, counts, _ = _raw(t, kmers, off, op, 0)
        rc2, rows2, counts2, _ = _raw(t, None, off, op, 0, want=(True, True, False), colorsets=sets)
        assert rc == rc2 == 0 and (rows == rows2).all() and (counts == counts2).all()
        wr, wc, _ = p.truth(idx, off, op, 0)
        assert (rows2 == _pack(wr)).all() and (counts2 == wc).all()
        prow, pcnt = t.combine_colorsets(sets, off, OPS[op])
        assert prow.tobytes() == rows2.tobytes() and (pcnt == counts2).all()
    # the matches of a batch of prefixes: `offsets` already is a group array
    prefixes = ["A", "CG", "TTT", "ACGTAC", "GGGGGGGGGGGG"] + S.packed_to_ascii(p.packed[:40], 27)
    poff, pk, _, pcs = t.query_prefixes([s[:6] if len(s) == 27 else s for s in prefixes])
    assert len(pk) > 1000
    owners = [p.owners[s] for s in S.packed_to_ascii(pk, 27)]
    for op in (AND, OR, SYMDIFF):
        rc, rows, counts, _ = _raw(t, None, poff, op, 0, want=(True, True, False), colorsets=pcs)
        rc2, rows2, counts2, found2 = _raw(t, pk, poff, op, 0)
        assert rc == rc2 == 0 and (rows == rows2).all() and (counts == counts2).all()
        assert (found2 == np.diff(poff.astype(np.int64))).all()
        for g in range(len(poff) - 1):
            grp = owners[int(poff[g]):int(poff[g + 1])]
            if not grp:
                want = set()
            elif op == AND:
                want = set.intersection(*grp)
            elif op == OR or len(grp) == 1:
                want = set.union(*grp)
            else:
                want = set.union(*grp) - set.intersection(*grp)
            assert {i for i in range(p.G) if rows[g, i // 8] >> (i % 8) & 1} == want, (op, g)
    # an id outside the dictionary
    bad = sets.copy()
    bad[3] = int(t.info()["colorsets"])
    rc, *_ = _raw(t, None, off, AND, 0, want=(True, True, False), colorsets=bad)
    assert rc == E_ARG and b"colour-set id" in _lib.load().bft_gpu_last_error()


# ---- index states ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("state", ("pending", "merged", "kmer_hash0", "walk_hash1", "compact"))
def test_index_states(state):
    opts = {"kmer_hash0": [("kmer_hash", 0)], "walk_hash1": [("walk_hash", 1)]}.get(state, [])
    t, owners, packed, ns = _snp_pool(31, seed=3, options=opts, merges=(state == "merged"))
    rng = np.random.default_rng(1)
    idx = rng.integers(0, len(packed), 4000)
    off = np.concatenate([[0], np.sort(rng.integers(0, 4000, 150)), [4000]])
    if state == "pending":  # the first call builds what was inserted
        assert t.info()["pending_pairs"] > 0
        lib = _lib.load()
        o = np.ascontiguousarray(off, dtype=np.uint64)
        cnt = np.zeros(len(off) - 1, dtype=np.uint32)
        k = np.ascontiguousarray(packed[idx])
        assert lib.bft_gpu_combine_colors(t._h, k.ctypes.data, len(k), o.ctypes.data, len(cnt), OR, 0, None, cnt.ctypes.data, None) == 0
        assert t.info()["pending_pairs"] == 0 and cnt.max() > 0
    p = Pool(t, owners, packed)
    _check(p, idx, off)
    if state == "compact":  # the default: the call does not bring the sorted table back
        assert t.footprint()["kmer_table"] <= 8
    if state == "merged":  # one more genome: the rows widen
        for gid in range(4, 9):
            extra = S.distinct(S.kmers_of(S.mutate(S.random_genome(5000, 4), 0.02, 50 + gid), 31))
            assert t.add_genome(f"g{gid}") == gid
            t.insert_kmers(extra, gid)
            for s in S.packed_to_ascii(extra, 31):
                owners.setdefault(s, set()).add(gid)
        p = Pool(t, owners, packed)
        assert p.G == 9
        _check(p, idx, off)
    t.close()


# ---- errors ------------------------------------------------------------------------------------------------------------------------------

def test_bad_arguments_write_nothing():
    p, ns = _shared(27)
    kmers = p.packed[:100]
    lib = _lib.load()
    for off, op, word in (([0, 10, 20], 3, b"op"), ([0, 10, 20], -1, b"op"), ([0, 30, 20, 40], AND, b"decrease"), ([0, 50, 101], OR, b"behind")):
        rc, rows, counts, found = _raw(p.t, kmers, off, op, 0)  # (_raw asserts that every buffer is still all canary)
        assert rc == E_ARG and rows is None and word in lib.bft_gpu_last_error()
    cs = np.zeros(100, dtype=np.uint32)
    assert _raw(p.t, None, [0, 30, 20], AND, 0, want=(True, True, False), colorsets=cs)[0] == E_ARG
    assert _raw(p.t, None, [0, 101], AND, 0, want=(True, True, False), colorsets=cs)[0] == E_ARG
    assert _raw(p.t, None, [0, 100], 7, 0, want=(True, True, False), colorsets=cs)[0] == E_ARG


# ---- device forms ------------------------------------------------------------------------------------------------------------------------

def _dev_outputs(torch, ng, rb, mis):
    """rows at byte offset `mis` of their tensor, counts, found; all between canaries"""
    r = torch.full((ng * rb + 2 * PAD,), 0xAA, dtype=torch.uint8, device="cuda")
    c = torch.full((ng + 2 * PAD,), -1431655766, dtype=torch.int32, device="cuda")
    f = torch.full((ng + 2 * PAD,), -1431655766, dtype=torch.int32, device="cuda")
    return r, c, f, r.data_ptr() + PAD + mis - (PAD % 4), c.data_ptr() + 4 * PAD, f.data_ptr() + 4 * PAD


def _dev_read(r, c, f, ng, rb, mis):
    start = PAD + mis - (PAD % 4)
    rh, ch, fh = r.cpu().numpy(), c.cpu().numpy().view(np.uint32), f.cpu().numpy().view(np.uint32)
    assert (rh[:start] == 0xAA).all() and (rh[start + ng * rb:] == 0xAA).all()
    for x in (ch, fh):
        assert (x[:PAD] == 0xAAAAAAAA).all() and (x[PAD + ng:] == 0xAAAAAAAA).all()
    return rh[start:start + ng * rb].reshape(ng, rb), ch[PAD:PAD + ng], fh[PAD:PAD + ng]


def test_device_form_clamps_bad_offsets():
    import torch
    p = _wide_pool(100)  # 13-byte rows: output rows at every alignment
    rng = np.random.default_rng(2)
    idx = rng.integers(0, 600, 3000)
    n = len(idx)
    good = np.concatenate([[0], np.sort(rng.integers(0, n, 60)), [n]]).astype(np.uint64)
    bad = good.copy()
    bad[10] = bad[12] + 5          # group 9 ends behind the start of group 10, whose end lies before its start
    bad[30] = n + 1000             # group 29 ends past the batch; group 30 starts there
    bad[-1] = 2 ** 63              # the last group too
    ng = len(good) - 1
    dk = torch.from_numpy(p.packed[idx].reshape(-1).copy()).cuda()
    s = torch.cuda.Stream()
    for mis in range(4):
        for off, op, skip in ((good, AND, 0), (good, SYMDIFF, 1), (bad, OR, 0), (bad, AND, 1)):
            doff = torch.from_numpy(off.view(np.int64).copy()).cuda()
            r, c, f, pr, pc, pf = _dev_outputs(torch, ng, 13, mis)
            torch.cuda.synchronize()
            p.t.combine_colors_dev(dk.data_ptr(), n, doff.data_ptr(), ng, OPS[op], skip, pr, pc, pf, stream=s.cuda_stream)
            s.synchronize()
            rows, counts, found = _dev_read(r, c, f, ng, 13, mis)
            # the truth: a group whose end lies before its start or past the batch is empty
            a, e = off[:-1].astype(np.int64, copy=True), off[1:].astype(np.int64, copy=True)
            empty = (off[1:] < off[:-1]) | (off[1:] > n)
            a[empty] = e[empty] = 0
            wr, wc, wf = p.truth(idx, np.stack([a, e], 1).reshape(-1), op, skip)
            assert (rows == _pack(wr[::2])).all() and (counts == wc[::2]).all() and (found == wf[::2]).all(), (mis, op, skip)
            if off is bad:
                assert empty.sum() >= 4 and not rows[empty].any() and not counts[empty].any()
    # counts alone: no row is written anywhere
    r, c, f, pr, pc, pf = _dev_outputs(torch, ng, 13, 1)
    doff = torch.from_numpy(good.view(np.int64).copy()).cuda()
    torch.cuda.synchronize()
    p.t.combine_colors_dev(dk.data_ptr(), n, doff.data_ptr(), ng, "or", 0, 0, pc, 0, stream=s.cuda_stream)
    s.synchronize()
    assert bool((r == 0xAA).all()) and bool((f == -1431655766).all())
    assert (c.cpu().numpy().view(np.uint32)[PAD:PAD + ng] == p.truth(idx, good, OR, 0)[1]).all()
    p.t.close()


def test_device_forms_interleave_with_other_queries_on_one_handle():
    import torch
    t, owners, packed, ns = _snp_pool(27, seed=11)
    p = Pool(t, owners, packed)
    rng = np.random.default_rng(3)
    idx = rng.integers(0, len(packed), 20000)
    n = len(idx)
    off = np.concatenate([[0], np.sort(rng.integers(0, n, 500)), [n]]).astype(np.uint64)
    ng = len(off) - 1
    q = np.ascontiguousarray(packed[idx])
    want_bits = np.packbits(p.present[idx], bitorder="little")
    t.set_marking()
    t.set_flags(packed[:ns:2], 2)
    core, _ = t.kmers_by_count(4, 4)
    s = torch.cuda.Stream()
    st = s.cuda_stream
    with torch.cuda.stream(s):
        dq = torch.from_numpy(q.reshape(-1).copy()).cuda()
        doff = torch.from_numpy(off.view(np.int64).copy()).cuda()
        outs = [_dev_outputs(torch, ng, 1, m) for m in (0, 1, 3)]
        bits = torch.zeros((n + 63) // 64, dtype=torch.int64, device="cuda")
        bits2 = torch.zeros((n + 63) // 64, dtype=torch.int64, device="cuda")
        crow = torch.zeros(n, dtype=torch.uint8, device="cuda")
        scr = torch.zeros(n, dtype=torch.int32, device="cuda")
        cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
        flags = torch.zeros(n, dtype=torch.uint8, device="cuda")
        sets = torch.from_numpy(t.query_rows(q)[2].view(np.int32).copy()).cuda()
        cs_out = _dev_outputs(torch, ng, 1, 2)
    s.synchronize()
    t.combine_colors_dev(dq.data_ptr(), n, doff.data_ptr(), ng, "and", 0, *outs[0][3:], stream=st)
    t.query_presence_dev(dq.data_ptr(), n, bits.data_ptr(), stream=st)
    t.combine_colors_dev(dq.data_ptr(), n, doff.data_ptr(), ng, "symdiff", 1, *outs[1][3:], stream=st)
    t.query_color_rows_dev(dq.data_ptr(), n, bits2.data_ptr(), crow.data_ptr(), scr.data_ptr(), stream=st)
    t.kmers_by_count_dev(4, 4, 0, 0, 0, 0, cnt.data_ptr(), stream=st)
    t.combine_colorsets_dev(sets.data_ptr(), n, doff.data_ptr(), ng, "or", cs_out[3], cs_out[4], stream=st)
    t.get_flags_dev(dq.data_ptr(), n, flags.data_ptr(), stream=st)
    t.combine_colors_dev(dq.data_ptr(), n, doff.data_ptr(), ng, "or", 0, *outs[2][3:])  # (the handle's own stream: the scratch changes streams)
    s.synchronize()
    torch.cuda.synchronize()
    for (r, c, f, *_), mis, (op, skip) in zip(outs, (0, 1, 3), ((AND, 0), (SYMDIFF, 1), (OR, 0))):
        rows, counts, found = _dev_read(r, c, f, ng, 1, mis)
        wr, wc, wf = p.truth(idx, off, op, skip)
        assert (rows == _pack(wr)).all() and (counts == wc).all() and (found == wf).all(), OPS[op]
    rows, counts, _ = _dev_read(cs_out[0], cs_out[1], cs_out[2], ng, 1, 2)
    wr, wc, _ = p.truth(idx, off, OR, 0)
    assert (rows == _pack(wr)).all() and (counts == wc).all()
    assert bool((cs_out[2] == -1431655766).all())  # (the colour-set form has no `found`)
    got_bits = bits.cpu().numpy().view(np.uint8)[:(n + 7) // 8]
    assert (got_bits == want_bits[:len(got_bits)]).all()
    assert (crow.cpu().numpy() == _pack(p.M[idx]).reshape(-1)).all()
    assert int(cnt.item()) == len(core) == int(p.M[:ns].all(axis=1).sum())
    fl = flags.cpu().numpy()
    # (a near miss of the pool may be a k-mer another genome stores: the flag follows the k-mer string, as the genome sets do)
    asc = S.packed_to_ascii(packed, 27)
    flagged = set(asc[:ns:2])
    wantf = np.array([0xFF if not p.present[i] else 2 if asc[i] in flagged else 0 for i in range(len(packed))], dtype=np.uint8)
    assert (wantf[ns:] != 0xFF).any() and (wantf == 2).sum() >= ns // 2
    assert (fl == wantf[idx]).all()
    t.unset_marking()
    t.close()


# ---- Python wrappers ---------------------------------------------------------------------------------------------------------------------

def test_python_wrappers_give_the_raw_calls_bytes():
    p, ns = _shared(31)
    idx, off = _sized_batch(p, ns, 8)
    kmers = p.packed[idx]
    for op in (AND, OR, SYMDIFF):
        for skip in (0, 1):
            rc, rows, counts, found = _raw(p.t, kmers, off, op, skip)
            prow, pcnt, pfnd = p.t.combine_colors(kmers, off, OPS[op], skip_absent=bool(skip))
            assert rc == 0 and prow.tobytes() == rows.tobytes() and (pcnt == counts).all() and (pfnd == found).all()
            assert prow.dtype == np.uint8 and pcnt.dtype == np.uint32 and pfnd.dtype == np.uint32
    with pytest.raises(ValueError):
        p.t.combine_colors(kmers, off, "xor")
    with pytest.raises(ValueError):
        p.t.combine_colors(kmers, [0, 5, 3])


def test_launches_are_counted_and_staged():
    p, ns = _shared(27)
    idx, off = _sized_batch(p, ns, 4)
    p.t.kernel_time(reset=True)
    _raw(p.t, p.packed[idx], off, AND, 0)
    ms, launches = p.t.kernel_time(reset=True)
    assert launches >= 6 and ms > 0
    p.t.set_option("build_stages", 1)
    _raw(p.t, p.packed[idx], off, SYMDIFF, 0)
    names = [s[0] if isinstance(s, tuple) else s["name"] for s in p.t.build_stages()]
    p.t.set_option("build_stages", 0)
    assert [x for x in names if x.startswith("set operations")] == ["set operations: colour set per k-mer", "set operations: segmented reduction",
                                                                     "set operations: rows and counts"]
