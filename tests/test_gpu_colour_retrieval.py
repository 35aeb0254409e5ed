"""Colour retrieval (bft_gpu_query_color_rows / _dev, bft_gpu_query_colors / _dev: k_row_colorsets, k_color_rows_bm<false>, <true>,
k_color_rows_bm16 / cr16_stream_tile, k_color_rows_kh, k_color_rows, k_cs_bitmaps, k_color_fill_cs, k_colors_kh) against ground truth at every
row width, output alignment, straddle and tile edge.  The cases and the truth come from tests/test_colour_cases_host.py, which checks on the
CPU that every case holds what it is there for.  Every comparison is bit-exact over every byte.  Device outputs are written into tensors with
64 guard bytes in front and behind, once over a fill of 0x55 and once over 0xFF, and the guards must come back untouched.  Each test asserts
the regime it means to reach with what the handle reports: footprint()["dictionary_bitmaps"], build_time()["kmer_hash_lines"], and the launch
count of kernel_time() (lookup and rows in one launch: 1; lookup, then rows: 2; lookup, scan, fill: 2 timed launches, the scan is not timed)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_colour_cases_host as H  # noqa: E402

from bloomfiltertrie_amd import BFT  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 64
FILLS = (0x55, 0xFF)


def _dev():
    import torch
    return torch.device("cuda", 0)


# ---- indexes: built once per genome count, shared by the tests of this module -------------------------------------------------------------------------
_INDEXES = {}


def _index(G):
    """(handle, pool) for the pool over G genomes; the handle is handed out with the k-mer hash on and the bitmap dictionary allowed"""
    if G not in _INDEXES:
        p = H.Pool(G)
        t = BFT(H.K)
        p.insert_into(t)
        t.build()
        info = t.info()
        assert info["genomes"] == G and info["kmers"] == int(p.member.any(axis=1).sum())
        t.kernel_time()  # (turns the launch count on)
        _INDEXES[G] = (t, p)
    return _INDEXES[G]


@pytest.fixture(scope="module", autouse=True)
def _close_indexes():
    yield
    for t, _ in _INDEXES.values():
        t.close()
    _INDEXES.clear()


def _hash(t, on):
    t.set_option("kmer_hash", 1 if on else 0)
    lines = t.build_time()["kmer_hash_lines"]
    assert (lines > 0) if on else (lines == 0), (on, lines)


def _launches(t):
    return t.kernel_time()[1]


# ---- guarded device outputs ---------------------------------------------------------------------------------------------------------------------------
class Guarded:
    """a device byte buffer whose payload of `nbytes` starts `shift` bytes behind a 16-byte boundary, GUARD bytes in front and behind, all filled"""

    def __init__(self, nbytes, fill, shift=0):
        import torch
        self.nbytes, self.fill = nbytes, fill
        self.buf = torch.full((nbytes + 2 * GUARD + 32,), fill, dtype=torch.uint8, device=_dev())
        self.at = (-self.buf.data_ptr()) % 16 + GUARD + shift
        self.ptr = self.buf.data_ptr() + self.at
        assert self.ptr % 16 == shift % 16 and self.at >= GUARD and self.at + nbytes + GUARD <= len(self.buf)

    def check(self, want, what):
        """the payload equals `want` (numpy uint8, any shape) byte for byte and nothing else changed"""
        import torch
        torch.cuda.synchronize()
        exp = torch.full_like(self.buf, self.fill)
        flat = np.ascontiguousarray(want, dtype=np.uint8).reshape(-1)
        assert len(flat) == self.nbytes
        if len(flat):
            exp[self.at:self.at + self.nbytes] = torch.from_numpy(flat).to(_dev())
        if torch.equal(self.buf, exp):
            return
        got = self.buf.cpu().numpy()
        bad = np.flatnonzero(got != exp.cpu().numpy()) - self.at
        raise AssertionError((what, "first wrong bytes (payload offsets; < 0 or >= %d: a guard)" % self.nbytes, bad[:8].tolist(),
                              [(int(got[self.at + b]), int(flat[b]) if 0 <= b < self.nbytes else self.fill) for b in bad[:8]], len(bad)))

    def payload(self):
        return self.buf[self.at:self.at + self.nbytes]


def _dev_rows(t, dq, n, rowbytes, fill, shift):
    """(guarded rows, presence bits as numpy) of the device call on the first n k-mers of dq"""
    import torch
    rows = Guarded(n * rowbytes, fill, shift)
    bits = Guarded(((n + 63) // 64) * 8, fill)
    scratch = torch.zeros(max(n, 1), dtype=torch.int32, device=_dev())
    t.query_color_rows_dev(dq.data_ptr(), n, bits.ptr, rows.ptr, scratch.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rows, bits


def _check_bits(bits, present, what):
    """the presence bits of the n k-mers (what the last word holds behind them is not specified), guards untouched"""
    n = len(present)
    got = bits.payload().cpu().numpy()
    assert (H.S.from_bits(got, n).astype(bool) == present).all(), (what, "presence bits")
    bits.check(got, (what, "presence bits: guards"))


def _rows_all_forms(t, p, idx, what, offsets=H.DEVICE_OFFSETS, bitmaps=True):
    """Forms 1 to 4 of the colour rows on the batch p.kmers[idx] (bitmaps=False: form 5, the same calls on a handle without the bitmap
    dictionary), every one against the truth, with the regime of each asserted."""
    import torch
    n, rb = len(idx), p.rowbytes
    q = np.ascontiguousarray(p.kmers[idx])
    want, present = p.rows(idx), p.present(idx)
    dq = torch.from_numpy(q).to(_dev())
    has_bm = lambda: t.footprint()["dictionary_bitmaps"]
    # 1. the host call: row numbers (the container walk), k_row_colorsets, k_color_rows_bm<false> / <true> / _bm16 (k_color_rows without bitmaps)
    _hash(t, True)
    _launches(t)
    hbits, hrows = t.query_color_rows(q)
    assert _launches(t) == 2, what
    assert hrows.shape == (n, rb)
    bad = np.flatnonzero((hrows != want).any(axis=1))
    assert not len(bad), (what, "host call", bad[:5].tolist(), hrows[bad[:2]].tolist(), want[bad[:2]].tolist())
    assert (hbits == H.bits_of(present)).all(), (what, "host call: presence bits")
    assert (has_bm() > 0) if bitmaps else (has_bm() == 0), what
    for fill in FILLS:
        # 2. the device call, d_rows 16-byte aligned, through the k-mer hash: k_color_rows_kh from 16 bytes (one launch), below it the lookup that
        #    hands out colour sets and the dword kernels (two); without bitmaps: the walk for row numbers, then k_color_rows
        # 3. d_rows 1, 4, 8, 15 bytes past a 16-byte boundary: k_color_rows_bm<true> at every width from 4 up, <false> below
        for shift in (0,) + tuple(offsets):
            _launches(t)
            rows, bits = _dev_rows(t, dq, n, rb, fill, shift)
            assert _launches(t) == (1 if bitmaps and rb >= 16 and shift == 0 else 2), (what, shift)
            rows.check(want, (what, "device call, k-mer hash", "fill %#x" % fill, "d_rows at +%d" % shift))
            _check_bits(bits, present, (what, shift))
    if bitmaps:
        # 4. the device call without the k-mer hash: the container walk, then _bm16 (aligned, 16 bytes and up) or the dword kernels
        _hash(t, False)
        for fill in FILLS:
            for shift in (0, offsets[0]):
                _launches(t)
                rows, bits = _dev_rows(t, dq, n, rb, fill, shift)
                assert _launches(t) == 2, (what, shift)
                rows.check(want, (what, "device call, container walk", "fill %#x" % fill, "d_rows at +%d" % shift))
                _check_bits(bits, present, (what, "walk", shift))
        _hash(t, True)
    assert (has_bm() > 0) if bitmaps else (has_bm() == 0), what


# =====================================================================================================================================================
@pytest.mark.parametrize("rowbytes,G", H.WIDTH_CASES)
def test_rows_every_width(rowbytes, G):
    """Every row width: 4 to 15 bytes (k_color_rows_bm<true> below the 16-byte kernel), powers of two (division by shifts), one byte (no
    division), widths around the 16-byte chunk and the dword, 250 and 1125 bytes.  The batch holds every ordered pair of colour-set classes --
    all genomes, single genomes, single bytes, 0x55 / 0xAA, a random half, sets of their own, absent -- with the second row starting at every
    phase (mod 16) the width has, so a byte that leaks across a straddle is a set bit where a zero belongs or the other way round; the
    dictionary's first and last set stand next to an all-genomes row and next to an absent k-mer, where the loads reach into the slack."""
    t, p = _index(G)
    assert p.rowbytes == rowbytes
    # the k-mers that hold the dictionary's first and last set (the loads around those reach the zero slack in front of and behind the dictionary)
    # stand between all-genomes rows and between absent k-mers at every phase, whichever sets the build's order put there
    n_sets = t.info()["colorsets"]
    assert n_sets == len({r.tobytes() for r in p.row_table() if r.any()})
    _, _, pool_sets = t.query_rows(p.kmers)
    idx = np.concatenate([p.pick(H.pair_order())] + [H.edge_set_block(int(np.flatnonzero(pool_sets == e)[0]), int(p.of_class[H.ALL][0]), int(p.of_class[H.ABSENT][0]))
                                                     for e in (0, n_sets - 1)])
    sets, cl = pool_sets[idx], p.cls[idx]
    for edge in (0, n_sets - 1):
        at = np.flatnonzero(sets == edge)
        at = at[(at > 0) & (at + 1 < len(idx))]
        for company in (H.ALL, H.ABSENT):
            mine = at[(cl[at - 1] == company) & (cl[at + 1] == company)]
            assert sorted({int(i * rowbytes) % 16 for i in mine}) == H.phases(rowbytes), (edge, company)
    assert (sets[cl == H.ABSENT] == 0xFFFFFFFF).all() and (sets[cl != H.ABSENT] < n_sets).all()
    what = "rowbytes %d, %d genomes" % (rowbytes, G)
    # 5. first, on the handle as built: no bitmap dictionary is ever derived -- k_color_rows fills the rows from the id lists
    t.set_option("test_no_cs_bitmaps", 1)
    try:
        assert t.footprint()["dictionary_bitmaps"] == 0
        _rows_all_forms(t, p, idx, what + ", id lists", offsets=H.DEVICE_OFFSETS[:1], bitmaps=False)
    finally:
        t.set_option("test_no_cs_bitmaps", 0)
    _rows_all_forms(t, p, idx, what)


@pytest.mark.parametrize("rowbytes", H.EDGE_WIDTHS)
def test_rows_tile_edges(rowbytes):
    """Batches of 1 .. 65 k-mers and of T - 1, T, T + 1, 2T - 1, 2T + 1 and 4T + 1 (one workgroup's wavefronts and one more) for the tile T of
    every kernel form that serves the width -- read from the library, not restated.  The last k-mer of every tile is an all-genomes row and the
    first of the next one absent, then the other way round: the sentinel behind a tile's colour sets and the first row of the next tile."""
    t, p = _index(8 * rowbytes)
    tiles = sorted({H.plan(rowbytes, f)[0] for f in H.plan_forms(rowbytes)})
    for n in H.edge_sizes(tiles):
        for swap in (False, True):
            idx = p.pick(H.edge_batch(n, tiles, swap))
            _rows_all_forms(t, p, idx, "rowbytes %d, tiles %s, %d k-mers%s" % (rowbytes, tiles, n, ", swapped" if swap else ""))


@pytest.mark.parametrize("rowbytes,form", [(16, H.FORM_16), (16, H.FORM_KH), (1, H.FORM_DWORD), (4, H.FORM_DWORD)])
def test_rows_more_tiles_than_the_grid(rowbytes, form):
    """More tiles than workgroups can be resident, so the tile loop of every kernel takes a second turn: a CU holds at most eight workgroups of
    256 threads and a workgroup of the wavefront-tiled kernels four tiles at a time (8 x CUs x 4 + 5 tiles); the dword kernels' grid ends at
    2048 workgroups (2048 + 5 tiles).  Expected rows: a gather on the device from the table of the pool's rows."""
    import torch
    t, p = _index(8 * rowbytes)
    T = H.plan(rowbytes, form)[0]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    tiles = (8 * cus * 4 + 5) if form != H.FORM_DWORD else (2048 + 5)
    n = tiles * T - 3
    idx = np.take(p.pick(H.pair_order()), np.arange(n) % len(H.pair_order()))
    dq = torch.from_numpy(np.take(p.kmers, idx, axis=0)).to(_dev())
    d_idx = torch.from_numpy(idx).to(_dev())
    want = torch.index_select(torch.from_numpy(p.row_table()).to(_dev()), 0, d_idx).reshape(-1)
    present = p.member.any(axis=1)[idx]
    _hash(t, form != H.FORM_16)  # (the 16-byte kernel behind the container walk; the others behind the k-mer hash)
    try:
        for fill in FILLS:
            _launches(t)
            rows, bits = _dev_rows(t, dq, n, rowbytes, fill, 0)
            assert _launches(t) == (1 if form == H.FORM_KH else 2)
            assert t.footprint()["dictionary_bitmaps"] > 0
            assert torch.equal(rows.payload(), want), (rowbytes, form, fill)
            front, behind = rows.buf[:rows.at], rows.buf[rows.at + rows.nbytes:]
            assert bool((front == fill).all()) and bool((behind == fill).all()), "guard bytes"
            _check_bits(bits, present, (rowbytes, form))
    finally:
        _hash(t, True)


# ---- id lists -------------------------------------------------------------------------------------------------------------------------------------------
_LIST_INDEXES = {}


def _list_index(layout):
    if layout not in _LIST_INDEXES:
        lc = H.ListCase(layout)
        t = BFT(H.K)
        lc.insert_into(t)
        t.build()
        assert t.info()["genomes"] == lc.G
        # the dictionary holds its offsets (4 bytes per set, and one) and its ids in 1, 2 or 4 bytes: not a byte more
        lists = {tuple(np.flatnonzero(m).tolist()) for m in lc.member if m.any()}
        assert t.info()["colorsets"] == len(lists)
        assert t.footprint()["colorset_dictionary"] == 4 * (len(lists) + 1) + H.id_bytes(lc.G - 1) * sum(len(s) for s in lists)
        t.kernel_time()
        _LIST_INDEXES[layout] = (t, lc)
    return _LIST_INDEXES[layout]


@pytest.fixture(scope="module", autouse=True)
def _close_list_indexes():
    yield
    for t, _ in _LIST_INDEXES.values():
        t.close()
    _LIST_INDEXES.clear()


def _dev_lists(t, dq, n, ids_cap, fill, null_ids=False, room=None):
    """the device call: (offsets, ids, bits, needed) as guarded buffers; ids has room for `room` ids (default ids_cap), all beyond ids_cap a guard"""
    import torch
    room = ids_cap if room is None else room
    off = Guarded((n + 1) * 8, fill)
    ids = Guarded(room * 4, fill)
    bits = Guarded(((n + 63) // 64) * 8, fill)
    need = Guarded(8, fill)
    t.query_colors_dev(dq.data_ptr(), n, bits.ptr, off.ptr, 0 if null_ids else ids.ptr, ids_cap, need.ptr, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return off, ids, bits, need


def _one_launch(t, lc):
    """k_colors_kh answers (one launch) where the k-mer hash exists and the genome count fits the kernel's 16-bit lengths"""
    return t.build_time()["kmer_hash_lines"] > 0 and lc.G < 65536


@pytest.mark.parametrize("layout", list(H.LIST_LAYOUTS))
def test_id_lists_wavefront_shapes(layout):
    """Lists of 0, 1, 2, 63 ... 257 and all ids in groups of 64 k-mers -- all absent; one list at lane 0, 31, 63; all of length 1; one list of
    several rounds of 64 followed by 63 empty ones; a list of all ids at the last lane of a group and the first of the next -- at batch sizes
    around the wavefront, the workgroup and the tile of k_colors_kh (BFT_KH_CT x 256), with one-, two- and four-byte dictionary ids: the host
    call (k_color_fill_cs), the device call behind the container walk (k_color_fill_cs) and behind the k-mer hash (k_colors_kh; with four-byte
    ids the genome count passes 65535, so that call takes the three launches too, which is asserted)."""
    import torch
    t, lc = _list_index(layout)
    for n in H.LIST_BATCHES:
        idx = lc.batch(n)
        q = np.ascontiguousarray(lc.kmers[idx])
        off, ids = lc.lists(idx)
        present = lc.present(idx)
        total = len(ids)
        _hash(t, True)
        hb, hoff, hids = t.query_colors(q)
        assert (hb == H.bits_of(present)).all() and (hoff == off).all() and len(hids) == total and (hids == ids).all(), (layout, n, "host call")
        dq = torch.from_numpy(q).to(_dev())
        for hashed in (True, False):
            _hash(t, hashed)
            for fill in FILLS:
                _launches(t)
                d_off, d_ids, d_bits, d_need = _dev_lists(t, dq, n, total, fill)
                one = hashed and _one_launch(t, lc)
                assert _launches(t) == (1 if one else 2), (layout, n, hashed)
                what = (layout, n, "k-mer hash" if hashed else "container walk", "fill %#x" % fill)
                d_off.check(off.view(np.uint8), (what, "offsets"))
                d_ids.check(ids.view(np.uint8), (what, "ids"))
                d_need.check(np.array([total], np.uint64).view(np.uint8), (what, "needed"))
                _check_bits(d_bits, present, what)
    _hash(t, True)


@pytest.mark.parametrize("layout", ["ids2"])
def test_id_lists_capacity_rule(layout):
    """bft_gpu.h's rule for a buffer that is too small: through the k-mer hash (one launch, which knows the total at its end) the first ids_cap
    ids and never a byte beyond; on the three launches nothing at all; offsets, presence bits and *needed complete either way.  d_ids NULL: only
    the sizes.  The ids' buffer has room for all ids, and everything behind ids_cap is a guard."""
    import torch
    t, lc = _list_index(layout)
    n = 1025
    idx = lc.batch(n)
    q = np.ascontiguousarray(lc.kmers[idx])
    off, ids = lc.lists(idx)
    present, total = lc.present(idx), len(ids)
    assert total > 2000
    dq = torch.from_numpy(q).to(_dev())
    for hashed in (True, False):
        _hash(t, hashed)
        assert _one_launch(t, lc) == hashed
        for fill in FILLS:
            for cap, null_ids in ((total, False), (total - 1, False), (1, False), (0, False), (total, True)):
                _launches(t)
                d_off, d_ids, d_bits, d_need = _dev_lists(t, dq, n, cap, fill, null_ids, room=total + 16)
                assert _launches(t) == (1 if hashed else 2)
                what = (layout, "k-mer hash" if hashed else "container walk", "fill %#x" % fill, "ids_cap %d" % cap, "NULL" if null_ids else "")
                written = 0 if null_ids else (cap if hashed or cap >= total else 0)
                want = np.full(total + 16, fill * 0x01010101, dtype=np.uint32)
                want[:written] = ids[:written]
                d_ids.check(want.view(np.uint8), (what, "ids"))
                d_off.check(off.view(np.uint8), (what, "offsets"))
                d_need.check(np.array([total], np.uint64).view(np.uint8), (what, "needed"))
                _check_bits(d_bits, present, what)
    _hash(t, True)


_WIDE = {}


@pytest.fixture(scope="module")
def wide_indexes():
    """G = 65535 and G = 65536: one k-mer held by every genome, one by genome 0 alone, one by the last genome alone, one by none"""
    km = H.S.distinct(H.S.kmers_of(H.S.random_genome(200, 79), H.K))[:4]
    out = {}
    for G in (65535, 65536):
        t = BFT(H.K)
        member = np.zeros((4, G), dtype=bool)
        member[0, :] = True
        member[1, 0] = True
        member[2, G - 1] = True
        for g in range(G):
            t.insert_kmers(np.ascontiguousarray(km[member[:, g]]), g)
        t.build()
        assert t.info()["genomes"] == G
        t.kernel_time()
        out[G] = (t, np.ascontiguousarray(km), member)
    yield out
    for t, _, _ in out.values():
        t.close()


@pytest.mark.parametrize("G", [65535, 65536])
def test_id_lists_sixteen_bit_lengths(wide_indexes, G):
    """k_colors_kh keeps a list's length in 16 bits; colors_core sends indexes of 65536 genomes and more the three-launch way.  65535 genomes:
    through the k-mer hash (one launch), a list of 65535 ids.  65536 genomes: three launches, a list of 65536 ids, which 16 bits would call
    empty.  The rows too: 8192 bytes, the widest in the suite."""
    import torch
    t, km, member = wide_indexes[G]
    order = np.array([3, 0, 3, 1, 0, 0, 2, 3, 0, 1, 2, 0, 3], dtype=np.int64)
    q = np.ascontiguousarray(km[order])
    off, ids = H.lists_of(member, order)
    present, total, n = member[order].any(axis=1), len(ids), len(order)
    assert total == 5 * G + 4 and int(off[2] - off[1]) == G
    _hash(t, True)
    hb, hoff, hids = t.query_colors(q)
    assert (hb == H.bits_of(present)).all() and (hoff == off).all() and len(hids) == total and (hids == ids).all()
    dq = torch.from_numpy(q).to(_dev())
    for fill in FILLS:
        _launches(t)
        d_off, d_ids, d_bits, d_need = _dev_lists(t, dq, n, total, fill)
        assert t.build_time()["kmer_hash_lines"] > 0
        assert _launches(t) == (1 if G < 65536 else 2), G
        d_off.check(off.view(np.uint8), (G, "offsets"))
        d_ids.check(ids.view(np.uint8), (G, "ids"))
        d_need.check(np.array([total], np.uint64).view(np.uint8), (G, "needed"))
        _check_bits(d_bits, present, G)
    # the rows: 8192 bytes each (k_color_rows_kh, k_color_rows_bm<true> at an odd address, the host call's k_color_rows_bm16)
    rows = np.packbits(member[order], axis=1, bitorder="little")
    assert rows.shape == (n, 8192)
    hbits, hrows = t.query_color_rows(q)
    assert (hrows == rows).all() and (hbits == H.bits_of(present)).all()
    for fill in FILLS:
        for shift in (0, 1):
            _launches(t)
            d_rows, d_bits = _dev_rows(t, dq, n, 8192, fill, shift)
            assert _launches(t) == (1 if shift == 0 else 2)
            d_rows.check(rows, (G, "rows", shift))
            _check_bits(d_bits, present, (G, "rows"))
