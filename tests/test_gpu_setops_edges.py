"""The colour-set algebra (csrc/bft_setops.hip: bft_gpu_combine_colors / _colorsets and their _dev forms) at every group class, row width and split
edge.  The cases, the truth and the proof that each case reaches its regime are in tests/test_setops_cases_host.py (no GPU); this file builds the five
hand-made indexes, each with the dictionary as bitmaps and as id lists ("test_no_cs_bitmaps"), and runs the cases.  Every comparison is exact, on rows,
counts and found, over all groups and all three ops; every output lies between canaries; the two dictionary forms must give the same bytes, and both the
truth's.  The product only names the colour-set ids (extract()): an index is accepted once every id stands for one ownership row and no row for two ids."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_setops_cases_host as H  # noqa: E402

from bloomfiltertrie_amd import BFT, _lib  # noqa: E402

pytestmark = pytest.mark.gpu

AND, OR, SYMDIFF, OPS = H.AND, H.OR, H.SYMDIFF, H.OPS
E_ARG = -1
PAD = 64  # canary bytes (device counts / found: entries) on either side of an output
CANARY32 = 0xAAAAAAAA


class Handle:
    """what a call needs: the index and the bytes of its rows"""

    def __init__(self, t, rb):
        self.t, self.rb = t, rb


class Index(Handle):
    def __init__(self, G, lists):
        fam = self.fam = H.family(G)
        t = self.t = BFT(H.K, device=0)
        if lists:
            t.set_option("test_no_cs_bitmaps", 1)
        for g, part in fam.inserts():
            t.insert_kmers(part, g)
        t.build()
        info = t.info()
        assert info["genomes"] == max(fam.ids) + 1 == G and info["kmers"] == fam.per * len(fam.sets)
        km, cs = t.extract()
        want = fam.set_of_kmer()
        sets_of_id = {}
        for kmer, c in zip(km, cs.tolist()):
            sets_of_id.setdefault(c, set()).add(want[kmer.tobytes()])
        assert len(km) == len(want) and all(len(v) == 1 for v in sets_of_id.values())  # all k-mers with one id have one ownership row
        id_of = {next(iter(v)): c for c, v in sets_of_id.items()}
        assert len(id_of) == len(sets_of_id) == len(fam.sets) == info["colorsets"]      # distinct ids have distinct rows
        self.id_of_set = np.array([id_of[s] for s in range(len(fam.sets))], dtype=np.uint32)
        self.n_sets, self.lists, self.rb = int(info["colorsets"]), lists, fam.rb

    def check_form(self):
        bm = self.t.footprint()["dictionary_bitmaps"]
        assert bm <= 8 if self.lists else bm > 0


_INDEXES = {}


def _index(G, lists):
    if (G, lists) not in _INDEXES:
        _INDEXES[G, lists] = Index(G, lists)
    return _INDEXES[G, lists]


def _canary(nbytes):
    return np.full(nbytes + 2 * PAD, 0xAA, dtype=np.uint8)


def _host(ix, batch, op, skip, kmers=None, colorsets=None):
    """one host call, every output between canaries: (rc, rows [ng, rb], counts, found or None)"""
    lib = _lib.load()
    off = np.ascontiguousarray(batch.off, dtype=np.uint64)
    ng, rb = batch.ng, ix.rb
    sizes = (ng * rb, ng * 4, ng * 4)
    bufs = [_canary(sz) for sz in sizes]
    ptrs = [b.ctypes.data + PAD for b in bufs]
    if colorsets is None:
        rc = lib.bft_gpu_combine_colors(ix.t._h, kmers.ctypes.data, len(kmers), off.ctypes.data, ng, op, skip, *ptrs)
    else:
        rc = lib.bft_gpu_combine_colorsets(ix.t._h, colorsets.ctypes.data, len(colorsets), off.ctypes.data, ng, op, ptrs[0], ptrs[1])
    for b, sz in zip(bufs, sizes):
        assert (b[:PAD] == 0xAA).all() and (b[PAD + sz:] == 0xAA).all()
    if rc != 0 or colorsets is not None:
        assert (bufs[2] == 0xAA).all()  # (the colour-set form has no `found`)
    if rc != 0:
        assert all((b == 0xAA).all() for b in bufs)
        return rc, None, None, None
    out = [b[PAD:PAD + sz].copy() for b, sz in zip(bufs, sizes)]
    return rc, out[0].reshape(ng, rb), out[1].view(np.uint32), None if colorsets is not None else out[2].view(np.uint32)


def _same(got, want, batch, what):
    rows, counts, found = got
    wr, wc, wf = want
    bad = np.nonzero((rows != wr).any(axis=1))[0]
    assert len(bad) == 0, (what, "rows: first wrong groups", bad[:5].tolist(), "of sizes", batch.sizes[bad[:5]].tolist(), "of", batch.ng)
    bad = np.nonzero(counts != wc)[0]
    assert len(bad) == 0, (what, "counts: first wrong groups", bad[:5].tolist(), counts[bad[:5]].tolist(), wc[bad[:5]].tolist())
    if found is not None:
        bad = np.nonzero(found != wf)[0]
        assert len(bad) == 0, (what, "found: first wrong groups", bad[:5].tolist(), found[bad[:5]].tolist(), wf[bad[:5]].tolist())


def _check(G, name, batch, forms=("kmers", "colorsets")):
    """the batch through the host calls on both dictionary forms, against the truth and against each other"""
    fam = H.family(G)
    want = {(op, skip): H.truth(fam, batch, op, skip) for op in OPS for skip in (0, 1)}
    kmers = np.ascontiguousarray(fam.packed[batch.kmer_rows(fam)]) if "kmers" in forms else None
    got = {}
    for lists in (False, True):
        ix = _index(G, lists)
        cs = np.ascontiguousarray(batch.colorsets(ix.id_of_set, ix.n_sets)) if "colorsets" in forms else None
        for op in OPS:
            for skip in (0, 1) if kmers is not None else ():
                rc, *out = _host(ix, batch, op, skip, kmers=kmers)
                assert rc == 0, _lib.load().bft_gpu_last_error()
                _same(out, want[op, skip], batch, (G, name, OPS[op], "skip" if skip else "count", "lists" if lists else "bitmaps", "k-mers"))
                got[lists, op, skip] = out
            if cs is not None:
                rc, *out = _host(ix, batch, op, 0, colorsets=cs)
                assert rc == 0, _lib.load().bft_gpu_last_error()
                _same(out, want[op, 0], batch, (G, name, OPS[op], "lists" if lists else "bitmaps", "colour sets"))
                got[lists, op, "cs"] = out
        ix.check_form()
    for (lists, op, skip), out in got.items():
        if lists:
            assert all(x is None or x.tobytes() == y.tobytes() for x, y in zip(out, got[False, op, skip])), (G, name, OPS[op], skip)
    return want


# ---- the cases of every width ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", H.WIDTHS)
def test_every_group_size(G):
    """0, 1, 2, SMALL - 1 | SMALL | SMALL + 1, 63 | 64 | 65, 128, CHUNK - 1 | CHUNK | CHUNK + 1, WAVE_MAX - 1 | WAVE_MAX | WAVE_MAX + 1, whole steps and a
    last step of one member; empty groups first, last and between two split groups; on the widest rows enough split groups for a second pass of
    k_so_finish"""
    P = H.plan()
    batch = H.sizes_batch(H.family(G), P)
    want = _check(G, "sizes", batch)
    big = batch.sizes > P.small
    a, o, s = (want[op, 0][1] for op in (AND, OR, SYMDIFF))
    assert (a[big] > 0).all() and (o[big] > a[big]).all() and (s[big] > 0).all() and (s[big] < o[big]).all()  # no result is trivial


@pytest.mark.parametrize("G", H.WIDTHS)
def test_lone_dissenter(G):
    """every member is C but one D at 0, SMALL - 1, 63, 64, CHUNK - 1, CHUNK, the last place -- in small, wave and split groups; D first and last
    in groups of whole loads"""
    P = H.plan()
    fam = H.family(G)
    cases = H.lone_groups(fam, P, "D")
    want = _check(G, "dissent", H.Batch([g for g, _, _ in cases]))
    assert (want[SYMDIFF, 0][1] == 2).all() and (want[AND, 0][1] == len(fam.core)).all() and (want[OR, 0][1] == len(fam.core) + 2).all()


@pytest.mark.parametrize("G", H.WIDTHS)
def test_lone_absent_member(G):
    """the same places, an absent member: the AND is empty unless it is skipped, SYMDIFF differs between the two, found = members - 1; and split
    groups absent in one whole step, absent throughout, with one found member"""
    P = H.plan()
    fam = H.family(G)
    cases = H.lone_groups(fam, P, H.ABS)
    batch = H.Batch([g for g, _, _ in cases] + H.absent_extra(fam, P))
    want = _check(G, "absent", batch)
    n = len(cases)
    assert (want[AND, 1][1][:n] > 0).all() and not want[AND, 0][1][:n].any() and (want[SYMDIFF, 0][1][:n] != want[SYMDIFF, 1][1][:n]).all()
    lone = np.array([sum(m for s, m in g if s < 0) == 1 for g, _, _ in cases])
    assert (want[AND, 0][2][:n][lone] == batch.sizes[:n][lone] - 1).all() and lone.sum() >= 20


@pytest.mark.parametrize("G", H.WIDTHS)
def test_runs(G):
    """two sets alternating (every member a head), one set throughout at whole loads, a short run across a load and a step boundary, an absent member
    at lane 63 followed by the set before it"""
    _check(G, "runs", H.Batch(list(H.runs_groups(H.family(G), H.plan()).values())))


# ---- device forms ----------------------------------------------------------------------------------------------------------------------------
def _dev(ix, batch, op, skip, mis, kmers=None, colorsets=None):
    """one device call on a stream of its own; rows at byte misalignment `mis`; (rows, counts, found or None) after the canaries are checked"""
    import torch
    ng, rb = batch.ng, ix.rb
    r = torch.full((ng * rb + 2 * PAD,), 0xAA, dtype=torch.uint8, device="cuda")
    c = torch.full((ng + 2 * PAD,), -1431655766, dtype=torch.int32, device="cuda")
    f = torch.full((ng + 2 * PAD,), -1431655766, dtype=torch.int32, device="cuda")
    doff = torch.from_numpy(np.ascontiguousarray(batch.off).view(np.int64).copy()).cuda()
    start = PAD + mis
    assert (r.data_ptr() + start) % 4 == mis
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    if colorsets is None:
        din = torch.from_numpy(kmers.reshape(-1).copy()).cuda()
        ix.t.combine_colors_dev(din.data_ptr(), len(kmers), doff.data_ptr(), ng, OPS[op], skip, r.data_ptr() + start, c.data_ptr() + 4 * PAD, f.data_ptr() + 4 * PAD,
                                stream=s.cuda_stream)
    else:
        din = torch.from_numpy(colorsets.view(np.int32).copy()).cuda()
        ix.t.combine_colorsets_dev(din.data_ptr(), len(colorsets), doff.data_ptr(), ng, OPS[op], r.data_ptr() + start, c.data_ptr() + 4 * PAD, stream=s.cuda_stream)
    s.synchronize()
    rh, ch, fh = r.cpu().numpy(), c.cpu().numpy().view(np.uint32), f.cpu().numpy().view(np.uint32)
    assert (rh[:start] == 0xAA).all() and (rh[start + ng * rb:] == 0xAA).all()
    assert (ch[:PAD] == CANARY32).all() and (ch[PAD + ng:] == CANARY32).all() and (fh[:PAD] == CANARY32).all() and (fh[PAD + ng:] == CANARY32).all()
    if colorsets is not None:
        assert (fh == CANARY32).all()
    return rh[start:start + ng * rb].reshape(ng, rb), ch[PAD:PAD + ng], None if colorsets is not None else fh[PAD:PAD + ng]


@pytest.mark.parametrize("G", H.WIDTHS)
def test_device_rows_at_every_byte_alignment(G):
    """rows of 1, 5, 9, 257 and 8751 bytes at misalignment 0 .. 3, between canaries: the k-mer form and the colour-set form"""
    fam = H.family(G)
    P = H.plan()
    groups = [g for g, _, _ in H.lone_groups(fam, P, "D") + H.lone_groups(fam, P, H.ABS) if H.size_of(g) <= P.chunk + 2]
    batch = H.Batch([()] + groups + list(H.bad_id_groups(fam, P))[-1:] + [()])
    kmers = np.ascontiguousarray(fam.packed[batch.kmer_rows(fam)])
    for mis, (op, skip) in enumerate(((AND, 0), (SYMDIFF, 1), (OR, 0), (AND, 1))):
        ix = _index(G, lists=bool(mis & 1))
        _same(_dev(ix, batch, op, skip, mis, kmers=kmers), H.truth(fam, batch, op, skip), batch, (G, "k-mers", mis, OPS[op], skip))
        cs = np.ascontiguousarray(batch.colorsets(ix.id_of_set, ix.n_sets))
        _same(_dev(ix, batch, SYMDIFF - op, 0, 3 - mis, colorsets=cs), H.truth(fam, batch, SYMDIFF - op, 0), batch, (G, "colour sets", 3 - mis, OPS[SYMDIFF - op]))


@pytest.mark.parametrize("G", H.WIDTHS)
def test_ids_outside_the_dictionary(G):
    """0xFFFFFFFE and n_sets beside valid ids in a small, a wave and a split group: the empty set in the device form, BFT_GPU_E_ARG in the host form"""
    fam = H.family(G)
    batch = H.Batch(H.bad_id_groups(fam, H.plan()))
    for lists in (False, True):
        ix = _index(G, lists)
        cs = np.ascontiguousarray(batch.colorsets(ix.id_of_set, ix.n_sets))
        assert (cs == ix.n_sets).sum() >= 4 and (cs == 0xFFFFFFFE).sum() >= 4
        for op in OPS:
            _same(_dev(ix, batch, op, 0, op + 1, colorsets=cs), H.truth(fam, batch, op, 0), batch, (G, lists, OPS[op]))
            rc, *_ = _host(ix, batch, op, 0, colorsets=cs)  # (_host asserts that nothing was written)
            assert rc == E_ARG and b"colour-set id" in _lib.load().bft_gpu_last_error()
        for bad in (ix.n_sets, 0xFFFFFFFE):  # each alone, too
            one = np.where((cs == ix.n_sets) | (cs == 0xFFFFFFFE), np.uint32(bad), cs)
            assert _host(ix, batch, AND, 0, colorsets=one)[0] == E_ARG


# ---- batches that make a grid-stride loop take a second pass --------------------------------------------------------------------------------
def test_second_pass_of_wave_count_and_emit():
    """more groups of SMALL + 1 members than k_so_wave has wavefronts, k_so_count groups of 64 lanes and k_so_emit lanes per output dword"""
    fam = H.family(H.GRID_G)
    _check(H.GRID_G, "grid_wave", H.grid_wave_batch(fam, H.plan()))


def test_second_pass_of_small():
    fam = H.family(H.GRID_G)
    _check(H.GRID_G, "grid_small", H.grid_small_batch(fam, H.plan()))


def test_split_steps_beyond_the_grid():
    """one group of (wavefronts of k_so_split's grid) x CHUNK + 1 colour-set ids: the last step, the only one with another set, is a second pass"""
    G = H.WIDTHS[0]
    want = _check(G, "split_stride", H.split_stride_batch(H.family(G), H.plan()), forms=("colorsets",))
    assert want[SYMDIFF, 0][1][0] == 2 and want[AND, 0][1][0] > 0


def test_more_groups_than_the_plan_has_lanes():
    """mostly empty and one-member groups, a split group in k_so_plan's first pass and two in its second"""
    G = H.WIDTHS[0]
    _check(G, "plan_cap", H.plan_cap_batch(H.family(G), H.plan()), forms=("colorsets",))


# ---- empty indexes ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("genomes", (0, 9))
def test_index_without_a_kmer(genomes):
    """a fresh handle, and one with nine genomes and no k-mer: zero counts, zero found, zero rows (none at all without a genome), canaries intact"""
    fam = H.family(40)
    t = BFT(H.K, device=0)
    for g in range(genomes):
        assert t.add_genome(f"g{g}") == g
    t.build()
    assert t.info()["genomes"] == genomes and t.info()["kmers"] == 0
    rb = (genomes + 7) // 8
    ix = Handle(t, rb)
    batch = H.Batch([(), H.runs((0, 2), (H.ABS, 1)), (), H.runs((1, 70)), H.runs((H.ABS, 1))])
    kmers = np.ascontiguousarray(fam.packed[batch.kmer_rows(fam)])
    zero = (np.zeros((batch.ng, rb), np.uint8), np.zeros(batch.ng, np.uint32), np.zeros(batch.ng, np.uint32))
    absent = np.full(batch.n, 0xFFFFFFFF, dtype=np.uint32)
    outside = absent.copy()
    outside[::3] = np.array([0, 5, genomes])[np.arange(len(outside[::3])) % 3]
    for op in OPS:
        for skip in (0, 1):
            rc, *out = _host(ix, batch, op, skip, kmers=kmers)
            assert rc == 0, _lib.load().bft_gpu_last_error()
            _same(out, zero, batch, (genomes, "host k-mers", op, skip))
            _same(_dev(ix, batch, op, skip, 1 + skip, kmers=kmers), zero, batch, (genomes, "device k-mers", op, skip))
        rc, *out = _host(ix, batch, op, 0, colorsets=absent)
        assert rc == 0, _lib.load().bft_gpu_last_error()
        _same(out, zero, batch, (genomes, "host colour sets", op))
        assert _host(ix, batch, op, 0, colorsets=outside)[0] == E_ARG  # (no id is inside a dictionary without a set)
        _same(_dev(ix, batch, op, 0, 3, colorsets=outside), zero, batch, (genomes, "device colour sets", op))
    t.close()
