"""Prefix matching (bft_gpu_query_prefixes / _dev: k_pm_bounds, k_pm_count, k_pm_emit at W = 1..4) against ground truth at every chunk, tile,
filter and write-back edge.  The batches, the indexes and the truth come from tests/test_prefix_cases_host.py, which proves on the CPU that
every batch reaches the regime it is named after.  Every output byte is compared: offsets, k-mers, rows, colour sets (each distinct id resolved
once with colorset(), then every match compared), *needed.  The host call and the device call; on the device every output lies between 64 guard
bytes, over a fill of 0x55 and of 0xFF, and d_kmers_out stands 0, 1, 2 and 3 bytes past a 4-byte boundary."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_prefix_cases_host as H  # noqa: E402

from bloomfiltertrie_amd import BFT  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 64
PLACEMENTS = ((0, 0x55), (1, 0xFF), (2, 0x55), (3, 0xFF))  # (bytes past a 4-byte boundary, fill)
SMALL = 100000  # batches of fewer candidates also run with the fills swapped


def _dev():
    import torch
    return torch.device("cuda", 0)


# ---- indexes: built once per (index, k), shared by the tests of this module ---------------------------------------------------------------------
_INDEXES = {}


def _index(name, k):
    """the handle of H.index(name, k); extract() is in the truth's order, so that "row" means the same on both sides"""
    if (name, k) not in _INDEXES:
        tr = H.index(name, k)
        t = BFT(k, device=0)
        tr.insert_into(t)
        km, cs = t.extract()
        assert km.shape == tr.packed.shape and (km == tr.packed).all()
        ids = {int(c): sum(1 << g for g in t.colorset(int(c))) for c in np.unique(cs)}
        assert (np.array([ids[int(c)] for c in cs]) == tr.setmask).all()
        _INDEXES[(name, k)] = t
    return _INDEXES[(name, k)]


@pytest.fixture(scope="module", autouse=True)
def _close_indexes():
    yield
    for t in _INDEXES.values():
        t.close()
    _INDEXES.clear()
    H.case.cache_clear()


class Guarded:
    """a device byte buffer whose payload of `nbytes` starts `shift` bytes behind a 16-byte boundary, GUARD bytes in front and behind, all filled"""

    def __init__(self, nbytes, fill, shift=0):
        import torch
        self.nbytes, self.fill = nbytes, fill
        self.buf = torch.full((nbytes + 2 * GUARD + 32,), fill, dtype=torch.uint8, device=_dev())
        self.at = (-self.buf.data_ptr()) % 16 + GUARD + shift
        self.ptr = self.buf.data_ptr() + self.at
        assert self.ptr % 16 == shift and self.at >= GUARD and self.at + nbytes + GUARD <= len(self.buf)

    def check(self, want, what):
        """the payload starts with `want` (numpy, any shape and type: its bytes) and nothing else changed, behind it and in the guards"""
        import torch
        torch.cuda.synchronize()
        exp = torch.full_like(self.buf, self.fill)
        flat = np.ascontiguousarray(want).reshape(-1).view(np.uint8)
        assert len(flat) <= self.nbytes
        if len(flat):
            exp[self.at:self.at + len(flat)] = torch.from_numpy(flat.copy()).to(_dev())
        if torch.equal(self.buf, exp):
            return
        got = self.buf.cpu().numpy()
        bad = np.flatnonzero(got != exp.cpu().numpy())
        raise AssertionError((what, "first wrong bytes (payload offsets; < 0 or >= %d: untouched space)" % len(flat), (bad[:8] - self.at).tolist(),
                              [(int(got[b]), int(exp[b])) for b in bad[:8]], len(bad)))


class Expected:
    """what the calls must return for a case: from the truth, the colour-set ids from the host call once they are checked against it"""

    def __init__(self, c, t):
        self.c, self.t, ans = c, t, c.ans
        self.offsets = ans.offsets
        self.rows = ans.rows
        self.kmers = np.ascontiguousarray(c.tr.packed[ans.rows])
        self.total = ans.total
        self.sets = None


def _host(c, t, e):
    off, km, rows, sets = t.query_prefixes(c.pref, c.lens)
    assert off.dtype == np.uint64 and (off == e.offsets).all(), (c.name, "offsets", np.flatnonzero(off != e.offsets)[:5])
    assert len(rows) == e.total and (rows == e.rows).all(), (c.name, "rows", np.flatnonzero(rows != e.rows)[:5])
    assert km.shape == e.kmers.shape and (km == e.kmers).all(), (c.name, "k-mers", np.flatnonzero((km != e.kmers).any(axis=1))[:5])
    ids, inv = np.unique(sets, return_inverse=True)
    masks = np.array([sum(1 << g for g in t.colorset(int(i))) for i in ids], dtype=np.int64)
    if e.total:
        assert (masks[inv] == c.tr.setmask[e.rows]).all(), (c.name, "colour sets")
    e.sets = np.ascontiguousarray(sets, dtype=np.uint32)


class DevBatch:
    def __init__(self, c):
        import torch
        n = len(c.pref)
        self.n = n
        self.dp = torch.from_numpy(np.ascontiguousarray(c.pref).reshape(-1).copy()).to(_dev()) if n else torch.zeros(1, dtype=torch.uint8, device=_dev())
        self.dl = torch.from_numpy(np.ascontiguousarray(c.lens).copy()).to(_dev()) if n else torch.zeros(1, dtype=torch.uint8, device=_dev())


def _device(c, t, e, db, shift, fill, cap=None, want=("kmers", "rows", "sets"), room=None):
    """one device call with capacity `cap` (default: the total) into outputs with room for `room` matches (default: cap), all compared"""
    nb = t.nb
    cap = e.total if cap is None else cap
    room = max(cap, 1) if room is None else room
    off = Guarded((db.n + 1) * 8, fill)
    need = Guarded(8, fill)
    out = {"kmers": Guarded(room * nb, fill, shift) if "kmers" in want else None,
           "rows": Guarded(room * 4, fill) if "rows" in want else None, "sets": Guarded(room * 4, fill) if "sets" in want else None}
    ptr = lambda g: g.ptr if g is not None else 0
    import torch
    t.query_prefixes_dev(db.dp.data_ptr(), db.dl.data_ptr(), db.n, off.ptr, ptr(out["kmers"]), ptr(out["rows"]), ptr(out["sets"]), cap, need.ptr,
                         torch.cuda.current_stream().cuda_stream)
    what = (c.name, "shift", shift, "fill", fill, "cap", cap, want)
    w = min(cap, e.total)
    off.check(e.offsets, what + ("offsets",))
    need.check(np.array([e.total], dtype=np.uint64), what + ("needed",))
    for key, exp in (("kmers", e.kmers), ("rows", e.rows), ("sets", e.sets)):
        if out[key] is not None:
            out[key].check(exp[:w], what + (key,))


def _run_case(name):
    c = H.case(name)
    t = _index(c.index, c.k)
    e = Expected(c, t)
    _host(c, t, e)
    db = DevBatch(c)
    for shift, fill in PLACEMENTS:
        _device(c, t, e, db, shift, fill)
    if c.ans.C < SMALL:
        for shift, fill in PLACEMENTS:
            _device(c, t, e, db, shift, fill ^ 0xAA)
    return c, t, e, db


@pytest.mark.parametrize("name", H.names("geometry"))
def test_chunk_geometry(name):
    _run_case(name)


@pytest.mark.parametrize("name", H.names("all_kept") + H.names("quarter_kept") + ["none_kept", "one_kept"])
def test_kept_density_over_multi_tile_chunks(name):
    _run_case(name)


@pytest.mark.parametrize("name", H.names("runs"))
def test_run_shapes(name):
    _run_case(name)


@pytest.mark.parametrize("name", H.names("bounds"))
def test_bounds(name):
    _run_case(name)


@pytest.mark.parametrize("name", H.names("every_length"))
def test_every_length(name):
    _run_case(name)


def test_capacity_on_the_device_form_at_multi_tile_size():
    """cap = 0 with outputs given, 1, the matches of exactly the first tile, a chunk's first output slot (from the truth) and one to either side,
    total - 1, total, total + 5: the first cap entries complete, everything behind them and the guards untouched, offsets and *needed exact"""
    c = H.case("quarter_kept-27")
    t = _index(c.index, c.k)
    e = Expected(c, t)
    _host(c, t, e)
    db = DevBatch(c)
    cs, begins, ends, tiles = H.tiles_of(c.ans)
    assert cs >= 3 * H.TILE
    ck = np.concatenate([[0], np.cumsum(c.ans.keep)])
    first_tile = int(ck[H.TILE])
    g = next(g for g in range(1000, H.CHUNKS) if 0 < ck[begins[g] + H.TILE] - ck[begins[g]] < H.TILE)  # a chunk whose first tile keeps some
    chunk_off = int(ck[begins[g]])  # what the emit reads as chunk_off[g]
    mid_tile = int(ck[begins[g] + H.TILE])  # the end of that chunk's first tile: the next tile starts at base == cap
    assert 0 < first_tile < chunk_off < mid_tile < e.total and ends[g] - begins[g] == cs
    caps = (0, 1, first_tile, chunk_off - 1, chunk_off, chunk_off + 1, mid_tile, e.total - 1, e.total, e.total + 5)
    for i, cap in enumerate(caps):
        shift, fill = PLACEMENTS[i % 4]
        _device(c, t, e, db, shift, fill, cap=cap, room=e.total + 5)


@pytest.mark.parametrize("name", ("quarter_kept-27", "every_length-90", "runs-heads-27"))
def test_each_output_alone(name):
    c = H.case(name)
    t = _index(c.index, c.k)
    e = Expected(c, t)
    _host(c, t, e)
    db = DevBatch(c)
    for i, want in enumerate((("kmers",), ("rows",), ("sets",), ())):
        for shift, fill in (PLACEMENTS[i], PLACEMENTS[(i + 1) % 4]):
            _device(c, t, e, db, shift, fill, want=want)  # (no output at all, cap > 0: offsets and *needed)
