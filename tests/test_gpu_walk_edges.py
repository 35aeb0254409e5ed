"""The walk kernels (csrc/bft_kernels_query.h: query_body as k_query / k_query8 / k_query6 and, from bft_walkh.hip, k_query6h; branching_body as
k_branching*) at every queue, chunk, claim and grid edge, and the root tables that decide who parks (k_root_ranges + k_root_ranges_check,
k_root_quartiles, k_rspec), read out by name.

The indexes, the query pools, the layouts that place the parked lanes, the branching families and all truth are tests/test_walk_cases_host.py's
(no GPU: it proves that every (k, layout, dealing) run here reaches the regime it is named after, by a replay of query_body's queue and chunk
bookkeeping).  Every comparison here is exact and against that truth -- set membership and rank in the T-form order, the genome set of the row, the
eight neighbours' membership --, never against another kernel: where two dealings "give the same bits", both equal the truth.

"test_walk_grid" caps the walk's launches at one or two workgroups, so that a batch of 5 * 10^4 k-mers gives every wavefront several chunks, dealt
by number ("query_dynamic" 0) or claimed ("query_dynamic" 1 with "query_dynamic_min" 1024): the loop's second turn, the claim path, and queue
entries carried from one chunk into the next.  The > 2^32-query guard on qbase is unreachable at test size and has no case here."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_walk_cases_host as C  # noqa: E402

from bloomfiltertrie_amd import BFT  # noqa: E402

pytestmark = pytest.mark.gpu

CANARY = -0x5555555555555556  # 0xAAAA... as a signed word
DEFAULTS = (("test_walk_grid", 0), ("query_dynamic", 1), ("query_dynamic_min", 1 << 16), ("query_grid_mult", 1), ("query_wgs_per_cu", 0), ("query_probe", 0),
            ("walk_hash", 0), ("kmer_hash", 1), ("root_direct", 3), ("root_quartiles", 1), ("node_hash", 1), ("flat_min", 3584))
_HANDLES = {}


def _index(name):
    return C.small_index(name) if name in C.SMALL else C.walk_index(name)


def _build(name):
    """the index built on the device: the rows of each genome inserted in shuffled order"""
    ix = _index(name)
    t = BFT(ix.k)
    rng = np.random.default_rng(ix.table.n)
    for g in range(C.N_GENOMES):
        rows = np.flatnonzero((ix.masks >> g) & 1)
        if len(rows):
            t.insert_kmers(np.ascontiguousarray(ix.packed[rng.permutation(rows)]), g)
    t.build()
    assert t.info()["kmers"] == ix.table.n
    return t


def _handle(name):
    """... once per module"""
    if name not in _HANDLES:
        _HANDLES[name] = _build(name)
    return _HANDLES[name]


@pytest.fixture
def bft(request):
    t = _handle(request.param)
    t.set_option("root_direct", 2)  # the range table, so the queue, whatever the default's rule ("root_direct" 3) makes of the index
    yield request.param, t
    for nm, v in DEFAULTS:
        t.set_option(nm, v)


def teardown_module(module):
    for t in _HANDLES.values():
        t.close()
    _HANDLES.clear()


def _deal(t, how, cap=1):
    t.set_option("test_walk_grid", cap)
    t.set_option("query_dynamic", 0 if how == "static" else 1)
    t.set_option("query_dynamic_min", 1024 if how == "claimed" else 1 << 16)


class Truth:
    """a batch base[idx] with its truth, and the colour sets of the handle resolved once"""

    def __init__(self, q, idx):
        self.n = len(idx)
        self.packed = np.ascontiguousarray(q.packed[idx])
        self.present, self.row, self.mask = q.present[idx], q.row[idx], q.mask[idx]
        self.bits = np.packbits(self.present, bitorder="little")
        self.words = np.zeros(((self.n + 63) // 64) * 8, dtype=np.uint8)  # (the padding bits of the last word: zero)
        self.words[:len(self.bits)] = self.bits


_SETS = {}


def _mask_of_sets(name, t, sets):
    cache = _SETS.setdefault(name, {})
    for c in np.unique(sets).tolist():
        if c not in cache:
            cache[c] = sum(1 << g for g in t.colorset(c))
    return np.array([cache[c] for c in sets.tolist()], dtype=np.int64)


def check_rows(name, t, tr, what):
    bits, rows, sets = t.query_rows(tr.packed)
    assert (bits == tr.bits).all(), (what, "presence", int(np.flatnonzero(np.unpackbits(bits ^ tr.bits, bitorder="little"))[0]))
    assert (rows == tr.row).all(), (what, "rows", int(np.flatnonzero(rows != tr.row)[0]))
    p = tr.present
    assert (_mask_of_sets(name, t, sets[p]) == tr.mask[p]).all(), (what, "colour sets")


def presence_dev(t, dq, n):
    import torch
    nw = (n + 63) // 64
    out = torch.full((nw + 8,), CANARY, dtype=torch.int64, device="cuda")
    t.query_presence_dev(dq.data_ptr(), n, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out


def check_presence_dev(t, tr, what, dq=None):
    import torch
    dq = torch.from_numpy(tr.packed).cuda() if dq is None else dq
    out = presence_dev(t, dq, tr.n).cpu().numpy()
    nw = (tr.n + 63) // 64
    assert (out[nw:] == CANARY).all(), (what, "canaries")
    assert (out[:nw].view(np.uint8) == tr.words).all(), (what, "presence words")


def _batch(name, layout, n=C.N_LAYOUT):
    if name in C.SMALL:
        q = C.small_queries(name)
        return Truth(q, np.random.default_rng(n).integers(0, len(q.base), n))
    q = C.queries(name)
    return Truth(q, C.batch(name, layout, n)[0])


def _layouts(name):
    return ("none",) if name in C.SMALL else C.layouts_of(C.W_of(name))


ALL = list(C.KS) + list(C.SMALL)


# ---- 1. the root tables ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bft", ALL, indirect=True)
def test_root_tables(bft):
    """the read-outs against the model's words: on a handle of its own as the build left it, then on the module's after each option's round trip"""
    name, t = bft
    tb = _index(name).tables

    def check(what, rq=True, t=t):
        rs, q, sp = t.debug_array("rstart", np.uint32), t.debug_array("rq", np.uint32), t.debug_array("rspec", np.uint32)
        if tb is None:  # a root without CCs: nothing is derived
            assert len(rs) == len(q) == len(sp) == 0, what
            return
        assert len(rs) == (1 << 18) + 2 and (rs[:(1 << 18) + 1] == tb["rstart"]).all(), what  # (the last word pads the array)
        if tb["rq"] is not None and rq:
            assert len(q) == 1 << 18 and (q == tb["rq"]).all(), what
        else:
            assert len(q) == 0, what
        assert len(sp) == (1 << 18) // 32 and (sp == tb["rspec"]).all(), what
    fresh = _build(name)
    try:
        check("after the build", t=fresh)
    finally:
        fresh.close()
    for v in (0, 1):
        t.set_option("root_direct", v)
        assert all(len(t.debug_array(a)) == 0 for a in ("rstart", "rq", "rspec")), v
    t.set_option("root_direct", 2)
    check("root_direct 2 -> 0 -> 1 -> 2")
    t.set_option("root_quartiles", 0)
    check("root_quartiles 0", rq=False)
    t.set_option("root_quartiles", 1)
    check("root_quartiles 0 -> 1")
    t.set_option("kmer_hash", 0)  # the bit table belongs to the walk that looks plain groups up in the k-mer hash
    assert len(t.debug_array("rspec")) == 0 and (tb is None or len(t.debug_array("rstart", np.uint32)) == (1 << 18) + 2)
    t.set_option("kmer_hash", 1)
    check("kmer_hash 0 -> 1")


# ---- 2. presence and rows at every layout -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["static", "claimed"])
@pytest.mark.parametrize("bft", ALL, indirect=True)
def test_layouts_capped(bft, how):
    """every layout on one workgroup: rows, colour sets, and -- without the k-mer hash, so that presence walks too -- the device form's words"""
    name, t = bft
    _deal(t, how)
    for layout in _layouts(name):
        tr = _batch(name, layout)
        check_rows(name, t, tr, (layout, how))
        t.set_option("kmer_hash", 0)
        check_presence_dev(t, tr, (layout, how, "no k-mer hash"))
        t.set_option("kmer_hash", 1)


@pytest.mark.parametrize("bft", ALL, indirect=True)
def test_tails_and_uncapped(bft):
    name, t = bft
    for layout in ("none", "all") if name not in C.SMALL else ("none",):
        tr = _batch(name, layout)
        check_rows(name, t, tr, (layout, "no cap"))
    t.set_option("kmer_hash", 0)
    for n in C.TAILS:
        tr = _batch(name, "tails", n)
        for how in ("no cap", "static", "claimed"):
            if how == "no cap":
                t.set_option("test_walk_grid", 0)
            else:
                _deal(t, how)
            check_rows(name, t, tr, ("tails", n, how))
            check_presence_dev(t, tr, ("tails", n, how))


OPTIONS = ([("query_wgs_per_cu", v) for v in (1, 2, 3)] + [("query_probe", v) for v in (4, 8)] + [("root_quartiles", v) for v in (0, 1)] +
           [("root_direct", v) for v in (0, 1, 2)] + [("node_hash", v) for v in (0, 1)] + [("flat_min", 1)])


@pytest.mark.parametrize("bft", ALL, indirect=True)
def test_layouts_under_every_option(bft):
    """residency, probe width, root tables on / off (root_direct 0: the staged root, no queue; 1: no queue), node prefix hash, every CC flat: every
    value on every k, with every layout on k = 18 and 36 and the queue's three carrying layouts elsewhere; static and claimed in turn"""
    name, t = bft
    W = _index(name).W
    full = name in C.FULL_KS
    todo = _layouts(name) if full else [x for x in ("carry", "over", "same_word") if x in _layouts(name)] or ["none"]
    batches = [(x, _batch(name, x)) for x in todo]
    import torch
    dqs = [torch.from_numpy(tr.packed).cuda() for _, tr in batches]
    for i, (opt, v) in enumerate(OPTIONS):
        if opt == "query_probe" and v == 8 and W > 2:
            continue
        t.set_option(opt, v)
        how = ("static", "claimed")[i % 2]
        _deal(t, how)
        for layout, tr in batches:
            check_rows(name, t, tr, (opt, v, layout, how))
        if full or opt in ("query_wgs_per_cu", "root_direct"):
            t.set_option("kmer_hash", 0)
            for (layout, tr), dq in zip(batches, dqs):
                check_presence_dev(t, tr, (opt, v, layout, how, "no k-mer hash"), dq)
            t.set_option("kmer_hash", 1)
        t.set_option(opt, dict(DEFAULTS)[opt] if opt != "root_direct" else 2)


def _ids_truth(tr):
    counts = np.array([bin(int(m)).count("1") for m in tr.mask], dtype=np.uint64)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    ids = np.array([g for m in tr.mask.tolist() for g in range(C.N_GENOMES) if (m >> g) & 1], dtype=np.uint32)
    return off, ids


@pytest.mark.parametrize("bft", ALL, indirect=True)
def test_walk_hash_and_kmer_hash(bft):
    """every layout and every tail through k_query6h ("walk_hash" 1: plain root groups looked up in the k-mer hash, special prefixes parked),
    capped and not, and through the k-mer hash itself (a cross-check of the cases): presence, id lists, colour rows"""
    name, t = bft
    for layout, n in [(x, C.N_LAYOUT) for x in _layouts(name)] + [("tails", n) for n in C.TAILS]:
        tr = _batch(name, layout, n)
        off, ids = _ids_truth(tr)
        rows = ((tr.mask[:, None] >> np.arange(8)[None, :]) & 1).astype(np.uint8)
        rows = np.packbits(rows, axis=1, bitorder="little")[:, :(C.N_GENOMES + 7) // 8]
        for wh, how in ((1, "static"), (1, "claimed"), (1, "no cap"), (0, "no cap")):
            t.set_option("walk_hash", wh)
            if how == "no cap":
                t.set_option("test_walk_grid", 0)
            else:
                _deal(t, how)
            what = (layout, n, "walk_hash", wh, how)
            check_presence_dev(t, tr, what)
            b, o, i = t.query_colors(tr.packed)
            assert (b == tr.bits).all() and (o == off).all() and (i == ids).all(), what
            b, r = t.query_color_rows(tr.packed)
            assert (b == tr.bits).all() and (r == rows).all(), what


# ---- 3. dealing does not change bits ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bft", ALL, indirect=True)
def test_dealing_does_not_change_bits(bft):
    """static and claimed; caps 1, 2, 3 and none; grid multipliers; two streams at once, each capped and claimed; after stale claim counters"""
    import torch
    name, t = bft
    trs = [_batch(name, x) for x in ([x for x in ("carry", "step") if x in _layouts(name)] or ["none"])]
    dqs = [torch.from_numpy(tr.packed).cuda() for tr in trs]
    t.set_option("kmer_hash", 0)
    for how in ("static", "claimed"):
        for cap in (1, 2, 3, 0):
            for mult in (1, 3):
                _deal(t, how, cap)
                t.set_option("query_grid_mult", mult)
                for tr, dq in zip(trs, dqs):
                    check_presence_dev(t, tr, (how, cap, mult), dq)
                    if mult == 1:
                        check_rows(name, t, tr, (how, cap, mult))
    t.set_option("query_grid_mult", 1)
    _deal(t, "claimed", 1)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    for rep in range(3):
        outs = [torch.full(((tr.n + 63) // 64 + 8,), CANARY, dtype=torch.int64, device="cuda") for tr in (trs * 2)[:2]]
        torch.cuda.synchronize()  # (the canaries stand before either stream starts)
        for tr, dq, s, out in zip((trs * 2)[:2], (dqs * 2)[:2], (s1, s2), outs):
            t.query_presence_dev(dq.data_ptr(), tr.n, out.data_ptr(), s.cuda_stream)
        torch.cuda.synchronize()
        for tr, out in zip((trs * 2)[:2], outs):
            out = out.cpu().numpy()
            nw = (tr.n + 63) // 64
            assert (out[nw:] == CANARY).all() and (out[:nw].view(np.uint8) == tr.words).all(), ("two streams", rep)
    for mode in (1, 2, 3):
        check_presence_dev(t, trs[0], ("before stale claims", mode), dqs[0])  # (the stream's slot exists and has moved on)
        t.set_option("test_stale_claims", mode)
        for rep in range(2):
            check_presence_dev(t, trs[0], ("stale claims", mode, rep), dqs[0])
        check_rows(name, t, trs[0], ("stale claims", mode, "rows"))


# ---- 4. branching through the walk ---------------------------------------------------------------------------------------------------------------
def _branching(name):
    return C.small_branching_base(name) if name in C.SMALL else C.branching_base(name)


def check_branching(t, packed, counts, what, dq=None):
    import torch
    n = len(packed)
    want_bits = np.packbits((counts >> 4 > 1) | (counts & 15 > 1), bitorder="little")
    b, c = t.query_branching(packed, with_counts=True)
    assert (c == counts).all(), (what, "counts", int(np.flatnonzero(c != counts)[0]), int(c[c != counts][0]), int(counts[c != counts][0]))
    assert (b == want_bits).all(), (what, "bits")
    assert (t.query_branching(packed) == want_bits).all(), (what, "bits, early exit")
    # the device form: canaries behind the words and behind the counts
    dq = torch.from_numpy(packed).cuda() if dq is None else dq
    nw = (n + 63) // 64
    words = np.zeros(nw * 8, dtype=np.uint8)
    words[:len(want_bits)] = want_bits
    stream = torch.cuda.current_stream().cuda_stream
    for with_counts in (True, False):
        out = torch.full((nw + 8,), CANARY, dtype=torch.int64, device="cuda")
        cnt = torch.full((n + 64,), 0xAA, dtype=torch.uint8, device="cuda")
        t.query_branching_dev(dq.data_ptr(), n, out.data_ptr(), cnt.data_ptr() if with_counts else None, stream)
        torch.cuda.synchronize()
        out, cnt = out.cpu().numpy(), cnt.cpu().numpy()
        assert (out[nw:] == CANARY).all() and (out[:nw].view(np.uint8) == words).all(), (what, "device words", with_counts)
        assert (cnt[n:] == 0xAA).all() and (cnt[:n] == (counts if with_counts else 0xAA)).all(), (what, "device counts", with_counts)


@pytest.mark.parametrize("bft", ALL, indirect=True)
def test_branching(bft):
    """the families and members of the index through k_branching* ("kmer_hash" 0) at every size edge and residency, and every layout's batch at a
    size that gives the grid loop several passes on two workgroups -- then the same batches through the k-mer hash"""
    name, t = bft
    base, counts, na = _branching(name)
    ix = _index(name)
    packed = C.S.pack_codes(base)
    for kh in (0, 1):
        t.set_option("kmer_hash", kh)
        for res in (1, 2, 3) if kh == 0 else (0,):
            t.set_option("query_wgs_per_cu", res)
            for n in C.BRANCH_SIZES + (max(na, 1),):
                idx = C.branching_batch(len(base), na, n)
                check_branching(t, np.ascontiguousarray(packed[idx]), counts[idx], (name, "kmer_hash", kh, "residency", res, n))
            t.set_option("test_walk_grid", 2)
            idx = C.branching_batch(len(base), na, C.BRANCH_GRID_N)
            check_branching(t, np.ascontiguousarray(packed[idx]), counts[idx], (name, "kmer_hash", kh, "residency", res, "two workgroups"))
            for layout in _layouts(name) if name not in C.SMALL else ():
                idx = C.layout_branching_idx(name, layout, C.BRANCH_GRID_N)
                check_branching(t, np.ascontiguousarray(packed[idx]), counts[idx], (name, "kmer_hash", kh, "residency", res, "two workgroups", layout))
            t.set_option("test_walk_grid", 0)
    assert ix.k == t.info()["k"]
