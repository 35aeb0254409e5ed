"""CPU-side tests (no GPU) of colour retrieval (csrc/bft_kernels_color.h, bft_rows16.h, k_color_rows_kh and k_colors_kh of bft_kh.hip): the
cases tests/test_gpu_colour_retrieval.py runs, their truth, and assertions that each case reaches what it is there for.

The truth is plain numpy over what was inserted: a boolean matrix k-mer x genome; packed rows are np.packbits(..., bitorder="little") of it,
id lists np.flatnonzero; an absent k-mer has a zero row and an empty list.  Nothing comes from the library under test; where the CPU oracle
can answer (k = 27 = 9 x 3, the small cases) the truth is compared with it.

The tile and the division constants are read from the library (bft_gpu_debug_color_rows_plan, csrc/bft_color_plan.h: no device needed), never
restated here: the division is checked over every output offset a tile can hold, for every row width from 1 to 8192 bytes and around every
power of two up to 2^24, and the tile against the sizes of the kernels' LDS arrays."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from bloomfiltertrie_amd import _lib, synth as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 27

# every row width of test_rows_every_width; G = 8 x rowbytes fills the last byte, ONE_BIT_WIDTHS also run with one bit in it (G = 8 x rowbytes - 7)
WIDTHS = (1, 2, 3, 4, 5, 7, 8, 9, 12, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 250, 255, 256, 257, 1024, 1125)
ONE_BIT_WIDTHS = (1, 3, 4, 15, 16, 17, 250)
WIDTH_CASES = [(rb, 8 * rb) for rb in WIDTHS] + [(rb, 8 * rb - 7) for rb in ONE_BIT_WIDTHS]
EDGE_WIDTHS = (1, 3, 4, 9, 16, 17, 250, 1125)
DEVICE_OFFSETS = (1, 4, 8, 15)  # bytes past a 16-byte boundary at which the device call is handed d_rows (besides 0)

FORM_DWORD, FORM_16, FORM_KH = 0, 1, 2  # bft_gpu_debug_color_rows_plan's `form`


# ---- the plan, from the library -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def built():
    subprocess.check_call(["make", "-C", _lib.CSRC, "all"], stdout=subprocess.DEVNULL)
    return True


def plan(rowbytes, form):
    """(tile_rows, div_m, div_l) the library launches the colour-row kernels of `form` with"""
    out = (C.c_uint32 * 3)()
    _lib.check(_lib.load().bft_gpu_debug_color_rows_plan(rowbytes, form, out))
    return int(out[0]), int(out[1]), int(out[2])


def plan_forms(rowbytes):
    """the forms of the plan that serve rows of this width"""
    return (FORM_DWORD, FORM_16, FORM_KH) if rowbytes >= 16 else (FORM_DWORD,)


def header_constant(name):
    txt = open(os.path.join(_lib.CSRC, "bft_color_plan.h")).read()
    m = re.search(r"^#define\s+%s\s+(\d+)u?\s*$" % name, txt, flags=re.M)
    assert m, name
    return int(m.group(1))


# ---- the pool: colour-set classes over G genomes --------------------------------------------------------------------------------------------------
CLASSES = ("all", "g0", "glast", "byte0", "bytelast", "alt", "half", "own", "absent")
ALL, ABSENT = CLASSES.index("all"), CLASSES.index("absent")
PER_CLASS, N_OWN, N_ABSENT = 30, 60, 30  # 7 x 30 + 60 + 30 = 300 distinct 27-mers


def _nonempty(v, rng):
    if not v.any():
        v[rng.integers(len(v))] = True
    return v


class Pool:
    """300 distinct 27-mers: PER_CLASS of each shared class (all genomes; genome 0 only; genome G - 1 only; exactly the genomes of the first byte;
    of the last byte; bytes alternating 0x55 / 0xAA; a random half), N_OWN with a random set of their own, N_ABSENT that are never inserted.
    member[i, g]: k-mer i was inserted for genome g.  cls[i]: index into CLASSES."""

    def __init__(self, G, seed=None):
        self.G, self.rowbytes = G, (G + 7) // 8
        rng = np.random.default_rng(1000 + G if seed is None else seed)
        km = S.distinct(S.kmers_of(S.random_genome(400 + K, 77), K))
        n = 7 * PER_CLASS + N_OWN + N_ABSENT
        assert len(km) >= n
        self.kmers = np.ascontiguousarray(km[rng.permutation(len(km))[:n]])
        g = np.arange(G)
        shared = [np.ones(G, bool), g == 0, g == G - 1, g < 8, g >= 8 * (self.rowbytes - 1), ((g >> 3) & 1) == (g & 1),
                  _nonempty(rng.random(G) < 0.5, rng)]
        self.member = np.zeros((n, G), dtype=bool)
        self.cls = np.zeros(n, dtype=np.int64)
        at = 0
        for c, v in enumerate(shared):
            self.member[at:at + PER_CLASS] = v
            self.cls[at:at + PER_CLASS] = c
            at += PER_CLASS
        for j in range(N_OWN):
            self.member[at] = _nonempty(rng.random(G) < (0.1, 0.5, 0.9)[j % 3], rng)
            self.cls[at] = CLASSES.index("own")
            at += 1
        self.cls[at:] = ABSENT
        self.of_class = [np.flatnonzero(self.cls == c) for c in range(len(CLASSES))]

    def insert_into(self, t):
        """one insert call per genome, ascending"""
        for g in range(self.G):
            sel = self.member[:, g]
            if sel.any():
                t.insert_kmers(np.ascontiguousarray(self.kmers[sel]), g)

    def pick(self, classes):
        """pool indices for a sequence of class indices: the k-mers of a class take turns, so sets repeat and k-mers repeat"""
        classes = np.asarray(classes, dtype=np.int64)
        out = np.zeros(len(classes), dtype=np.int64)
        for c in range(len(CLASSES)):
            at = np.flatnonzero(classes == c)
            out[at] = self.of_class[c][np.arange(len(at)) % len(self.of_class[c])]
        return out

    # -- the truth ----------------------------------------------------------------------------------------------------------------------------------
    def present(self, idx):
        return self.member[idx].any(axis=1)

    def rows(self, idx):
        """[len(idx), rowbytes] uint8: genome g -> bit g % 8 of byte g // 8; the padding bits of the last byte are zero"""
        return np.packbits(self.member[idx], axis=1, bitorder="little")

    def row_table(self):
        """the rows of all pool k-mers (absent ones: zero)"""
        return self.rows(np.arange(len(self.kmers)))

    def lists(self, idx):
        """(offsets[n + 1] uint64, ids uint32)"""
        return lists_of(self.member, idx)


def lists_of(member, idx):
    per = [np.flatnonzero(member[i]).astype(np.uint32) for i in idx]
    off = np.zeros(len(idx) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(p) for p in per])
    return off, (np.concatenate(per) if per else np.zeros(0, np.uint32)).astype(np.uint32)


def bits_of(flags):
    return np.packbits(np.asarray(flags, dtype=bool), bitorder="little")


# ---- the query order: every ordered pair of classes at every phase of the row start -----------------------------------------------------------
def pair_cycle(c):
    """a cyclic sequence over range(c) of length c * c in which every ordered pair (a, b), a == b included, is adjacent exactly once
    (an Euler circuit of the complete digraph with loops)"""
    nxt = [list(range(c)) for _ in range(c)]
    stack, out = [0], []
    while stack:
        v = stack[-1]
        if nxt[v]:
            stack.append(nxt[v].pop())
        else:
            out.append(stack.pop())
    out = out[::-1][:-1]
    assert len(out) == c * c
    return out


def pair_order():
    """Class indices: the pair cycle 16 times, each turn one position later (mod 16) than the one before, so that every ordered pair of classes
    occurs with its second k-mer at every position mod 16 -- whatever the row width, its row then starts at every phase (mod 16) that width has."""
    cyc = pair_cycle(len(CLASSES))
    pad = (1 - len(cyc)) % 16  # block length = 1 (mod 16)
    block = [cyc[0]] * pad + cyc
    assert len(block) % 16 == 1
    return np.array(block * 16 + [cyc[0]], dtype=np.int64)


def phases(rowbytes):
    """the values (row start mod 16) takes when the first row starts 16-byte aligned"""
    return sorted({(i * rowbytes) % 16 for i in range(16)})


def pairs_at_phases(classes, rowbytes):
    """{(a, b, phase of b's row start)} over the adjacent pairs of a class sequence"""
    i = np.arange(1, len(classes))
    return set(zip(classes[:-1].tolist(), classes[1:].tolist(), ((i * rowbytes) % 16).tolist()))


def edge_set_block(x, all_k, absent_k):
    """Pool indices: k-mer x between two all-genomes rows and between two absent k-mers, 16 times, each turn 7 positions later -- x at every
    position mod 16 in either company.  For the k-mers that hold the dictionary's first and its last set, whatever the build's set order made them."""
    return np.array([all_k, x, all_k, absent_k, x, absent_k, absent_k] * 16, dtype=np.int64)


def edge_batch(n, tiles, swap):
    """Class indices of a batch of n k-mers for the tile-edge test: the pair order repeated, and for every tile size T in `tiles` and every
    multiple m * T < n the k-mer in front of the tile boundary an all-genomes row and the first of the next tile absent (swap: the other way)."""
    cl = np.resize(pair_order(), n).copy()
    first, second = (ABSENT, ALL) if swap else (ALL, ABSENT)
    for T in tiles:
        at = np.arange(T, n, T)
        cl[at - 1] = first
        cl[at] = second
    return cl


def edge_sizes(tiles):
    s = {1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65}
    for T in tiles:
        s |= {T - 1, T, T + 1, 2 * T - 1, 2 * T + 1, 4 * T + 1}
    return sorted(s)


# ---- id lists: wavefront shapes ---------------------------------------------------------------------------------------------------------------------
LIST_SIZES = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257)
LIST_BATCHES = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097)
# name -> the genome ids in use (the largest decides the dictionary's id width: 1, 2 or 4 bytes)
LIST_LAYOUTS = {"ids1": np.arange(256), "ids2": np.arange(300),
                "ids4": np.concatenate([np.arange(0, 290), [65535, 65536, 70001]])}


def id_bytes(max_id):
    return 1 if max_id < 256 else (2 if max_id < 65536 else 4)


class ListCase:
    """k-mers whose lists have 1, 2, 63 ... 257 and all ids in use (sizes beyond the ids in use are left out: a one-byte dictionary has at most
    256), two k-mers per size with different sets, and 64 absent k-mers; batches laid out in groups of 64 k-mers = the wavefronts of
    k_color_fill_cs and k_colors_kh."""

    def __init__(self, layout):
        self.used = LIST_LAYOUTS[layout].astype(np.int64)
        self.G = int(self.used.max()) + 1
        rng = np.random.default_rng(len(self.used))
        self.sizes = sorted({s for s in LIST_SIZES if s < len(self.used)} | {len(self.used)})
        km = S.distinct(S.kmers_of(S.random_genome(400 + K, 78), K))
        n = 2 * len(self.sizes) + 64
        self.kmers = np.ascontiguousarray(km[:n])
        self.member = np.zeros((n, self.G), dtype=bool)
        self.by_size = {}
        for j, s in enumerate(self.sizes):
            for r in range(2):
                self.member[2 * j + r, rng.choice(self.used, size=s, replace=False)] = True
            self.by_size[s] = (2 * j, 2 * j + 1)
        self.absent = np.arange(2 * len(self.sizes), n)
        self.full = len(self.used)
        self.long = max(s for s in self.sizes if s <= 257)  # 257, or all 256 ids of a one-byte dictionary

    def insert_into(self, t):
        for g in self.used.tolist():
            sel = self.member[:, g]
            if sel.any():
                t.insert_kmers(np.ascontiguousarray(self.kmers[sel]), g)

    def groups(self):
        """[(name, 64 pool indices)]"""
        A = self.absent

        def one(lane, size, r=0):
            g = A.copy()
            g[lane] = self.by_size[size][r]
            return g
        ones = np.array([self.by_size[1][i & 1] for i in range(64)])
        mixed = np.array([self.by_size[self.sizes[i % len(self.sizes)]][(i // len(self.sizes)) & 1] if i % 3 else A[i] for i in range(64)])
        return [("all absent", A.copy()), ("lane 0", one(0, 65)), ("lane 31", one(31, 65, 1)), ("lane 63", one(63, 65)), ("all of length 1", ones),
                ("long list, then 63 absent", one(0, self.long)), ("all ids at the last lane", one(63, self.full)),
                ("all ids at the first lane", one(0, self.full, 1)), ("mixed", mixed)]

    def batch(self, n):
        """pool indices of the batch of n k-mers: the groups in order, starting one group later for every batch size, repeated to length n"""
        base = np.concatenate([g for _, g in self.groups()])
        return np.resize(np.roll(base, -64 * LIST_BATCHES.index(n)), n)

    def lists(self, idx):
        return lists_of(self.member, idx)

    def present(self, idx):
        return self.member[idx].any(axis=1)


# =====================================================================================================================================================
# the tests
# =====================================================================================================================================================
def test_pool_classes_are_what_they_say():
    for rb, G in WIDTH_CASES:
        p = Pool(G)
        assert p.rowbytes == rb and len(p.kmers) == 300 and len(S.distinct(p.kmers)) == 300
        rows = p.row_table()
        assert rows.shape == (300, rb)
        r = {CLASSES[c]: rows[p.of_class[c][0]] for c in range(len(CLASSES))}
        last = (1 << (G - 8 * (rb - 1))) - 1  # the genomes of the last byte
        assert (r["all"][:-1] == 0xFF).all() and r["all"][-1] == last
        assert r["g0"][0] == 1 and not r["g0"][1:].any()
        assert r["glast"][-1] == (last + 1) >> 1 and not r["glast"][:-1].any()  # (the highest genome of the last byte)
        assert r["byte0"][0] == (0xFF if G >= 8 else last) and not r["byte0"][1:].any()
        assert r["bytelast"][-1] == last and not r["bytelast"][:-1].any()
        want = np.array([0x55 if b % 2 == 0 else 0xAA for b in range(rb)], dtype=np.uint8)
        want[-1] &= last
        assert (r["alt"] == want).all()
        assert not r["absent"].any()
        # the shared classes repeat their set; the k-mers of "own" have sets of their own (as far as G allows different ones)
        for c in range(7):
            assert (rows[p.of_class[c]] == rows[p.of_class[c][0]]).all() and rows[p.of_class[c][0]].any()
        own = rows[p.of_class[CLASSES.index("own")]]
        assert own.any(axis=1).all()
        if G >= 64:
            assert len({x.tobytes() for x in own}) == N_OWN
        assert not rows[p.of_class[ABSENT]].any() and len(p.of_class[ABSENT]) == N_ABSENT
        # padding bits of the last byte are zero in the truth
        assert not (rows[:, -1] & ~np.uint8(last)).any()


def test_pair_order_has_every_ordered_pair_at_every_phase():
    order = pair_order()
    c = len(CLASSES)
    assert len(order) < 1500
    for rb in sorted(set(WIDTHS) | set(EDGE_WIDTHS) | {8192}):
        got = pairs_at_phases(order, rb)
        ph = phases(rb)
        assert len(ph) == 16 // math.gcd(rb, 16)
        assert got == {(a, b, f) for a in range(c) for b in range(c) for f in ph}, rb
    # through the pool: every k-mer of the pool is queried, and the adjacent pairs are pairs of classes
    p = Pool(24)
    idx = p.pick(order)
    assert (p.cls[idx] == order).all() and set(idx.tolist()) == set(range(300))


def test_edge_set_block_has_both_companies_at_every_phase():
    blk = edge_set_block(7, 1, 2)
    for rb in sorted(set(WIDTHS) | {8192}):
        at = np.flatnonzero(blk == 7)
        for company in (1, 2):
            mine = at[(blk[at - 1] == company) & (blk[at + 1] == company)]
            assert sorted({int(i * rb) % 16 for i in mine}) == phases(rb), (rb, company)


def test_pool_truth_matches_the_oracle(oracle_mod):
    for G in (1, 17, 24, 121):
        p = Pool(G)
        o = oracle_mod.OracleBFT(K)
        p.insert_into(o)
        idx = p.pick(pair_order())
        q = np.ascontiguousarray(p.kmers[idx])
        obits, ooff, oids = o.query_colors(q)
        off, ids = p.lists(idx)
        assert (obits == bits_of(p.present(idx))).all()
        assert (ooff == off).all() and (oids == ids).all()
        # the rows are the lists as bitmaps
        rows = p.rows(idx)
        unp = np.unpackbits(rows, axis=1, bitorder="little")
        for i in (0, 1, len(idx) // 2, len(idx) - 1):
            assert (np.flatnonzero(unp[i]) == oids[int(ooff[i]):int(ooff[i + 1])]).all()
        o.close()


def test_edge_batches_put_all_and_absent_on_either_side_of_every_tile(built):
    for rb in EDGE_WIDTHS:
        tiles = sorted({plan(rb, f)[0] for f in plan_forms(rb)})
        sizes = edge_sizes(tiles)
        for T in tiles:
            assert {T - 1, T, T + 1, 2 * T - 1, 2 * T + 1, 4 * T + 1} <= set(sizes)
        assert {1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65} <= set(sizes)
        for n in sizes:
            for swap in (False, True):
                cl = edge_batch(n, tiles, swap)
                assert len(cl) == n
                for T in tiles:
                    for b in range(T, n, T):
                        assert (cl[b - 1], cl[b]) == ((ABSENT, ALL) if swap else (ALL, ABSENT)), (rb, n, T, b)
        # (no boundary of one tile size is the last k-mer of another's tile: the two overrides never meet)
        assert all(T % 4 == 0 for T in tiles)


def test_list_cases_hold_the_shapes_they_name():
    for name in LIST_LAYOUTS:
        lc = ListCase(name)
        assert id_bytes(lc.G - 1) == {"ids1": 1, "ids2": 2, "ids4": 4}[name]
        sizes = lc.member.sum(axis=1)
        assert set(sizes[sizes > 0].tolist()) == set(lc.sizes) and lc.full in lc.sizes
        assert set(LIST_SIZES) <= set(lc.sizes) | {s for s in LIST_SIZES if s >= lc.full}
        if name != "ids1":
            assert lc.long == 257 and set(LIST_SIZES) <= set(lc.sizes)
        assert set(np.flatnonzero(lc.member.any(axis=0)).tolist()) == set(lc.used.tolist())  # every id in use is inserted: the width is as named
        g = dict(lc.groups())
        n_of = lambda ix: lc.member[ix].sum(axis=1)
        assert not n_of(g["all absent"]).any()
        for nm, lane in (("lane 0", 0), ("lane 31", 31), ("lane 63", 63)):
            v = n_of(g[nm])
            assert v[lane] == 65 and v.sum() == 65
        assert (n_of(g["all of length 1"]) == 1).all()
        v = n_of(g["long list, then 63 absent"])
        assert v[0] == lc.long and v.sum() == lc.long and lc.long > 4 * 64 - 1  # several rounds of 64
        assert n_of(g["all ids at the last lane"])[63] == lc.full and n_of(g["all ids at the first lane"])[0] == lc.full
        names = [nm for nm, _ in lc.groups()]
        assert names.index("all ids at the first lane") == names.index("all ids at the last lane") + 1
        assert all(len(ix) == 64 for ix in g.values())
        seen = set()
        for n in LIST_BATCHES:
            b = lc.batch(n)
            assert len(b) == n
            seen |= {names[(j + LIST_BATCHES.index(n)) % len(names)] for j in range((n + 63) // 64)}
        assert seen == set(names)
        assert (lc.batch(4097)[:64] == lc.groups()[LIST_BATCHES.index(4097) % len(names)][1]).all()


# ---- the division and the tile -------------------------------------------------------------------------------------------------------------------------
def division_widths():
    w = set(range(1, 8193))
    for j in range(0, 25):
        w |= {(1 << j) - 1, 1 << j, (1 << j) + 1}
    w.discard(0)
    return sorted(x for x in w if x <= (1 << 24) + 1)


def check_division(rowbytes, form, bufs):
    """the kernels' quotient == byte // rowbytes at every offset a lane can start at: multiples of 4 (16: the 16-byte kernel) below tile_rows * rowbytes"""
    tile_rows, m, l = plan(rowbytes, form)
    step = 16 if form == FORM_16 else 4
    mult, cap = {FORM_DWORD: (4, header_constant("CR_MAX_TILE_ROWS")), FORM_16: (16, header_constant("CR16_WAVE_ROWS")),
                 FORM_KH: (64, header_constant("BFT_KH_ROWS_TILE"))}[form]
    assert tile_rows >= mult and tile_rows % mult == 0 and tile_rows <= cap, (rowbytes, form, tile_rows)
    limit = tile_rows * rowbytes
    assert limit < 1 << 32, (rowbytes, form)
    if l == 0:
        assert rowbytes == 1  # q = byte
        return limit
    assert m < 1 << 32 and 1 <= l <= 32 and (1 << l) >= rowbytes > (1 << (l - 1))
    rb, (base, byte, t, s) = np.uint64(rowbytes), bufs  # (in place, in blocks that stay in the cache: 2.5 x 10^9 offsets in all)
    for a in range(0, limit, len(base) * step):
        cnt = (min(limit, a + len(base) * step) - a + step - 1) // step
        byte, t, s = byte[:cnt], t[:cnt], s[:cnt]
        np.multiply(base[:cnt], np.uint64(step), out=byte)
        byte += np.uint64(a)
        np.multiply(byte, np.uint64(m), out=t)
        t >>= np.uint64(32)  # mulhi(byte, div_m)
        np.subtract(byte, t, out=s)
        s >>= np.uint64(1)
        s += t  # (32-bit arithmetic on the device: t <= byte, so no step passes 2^32)
        top = int(s.max())
        s >>= np.uint64(l - 1)  # the quotient
        s *= rb
        np.subtract(byte, s, out=s)  # the remainder (wraps to a huge value where the quotient is too large)
        if int(s.max()) >= rowbytes or top >= 1 << 32:
            i = int(np.flatnonzero(s >= rb)[0]) if int(s.max()) >= rowbytes else -1
            raise AssertionError((rowbytes, form, m, l, int(byte[i]), int(byte[i]) // rowbytes, top))
        byte, t, s = bufs[1:]
    return limit


def test_division_is_exact_over_every_tile(built):
    bufs = (np.arange(1 << 15, dtype=np.uint64),) + tuple(np.empty(1 << 15, dtype=np.uint64) for _ in range(3))
    for rowbytes in division_widths():
        for form in plan_forms(rowbytes):
            check_division(rowbytes, form, bufs)


def test_plan_constants_the_kernels_special_case(built):
    """a power of two divides by shifts alone (multiplier 1), one-byte rows are not divided at all, and the LDS arrays hold a tile and its sentinel"""
    assert plan(1, FORM_DWORD)[1:] == (0, 0)
    for j in range(1, 25):
        for form in plan_forms(1 << j):
            assert plan(1 << j, form)[1:] == (1, j)
    assert header_constant("CR_MAX_TILE_ROWS") == 2048 and header_constant("CR16_WAVE_ROWS") == 1024 and header_constant("BFT_KH_ROWS_TILE") == 256
    src = open(os.path.join(_lib.CSRC, "bft_kernels_color.h")).read()
    assert "s_cs[CR_MAX_TILE_ROWS + 1]" in src and "s_cs_all[4][CR16_WAVE_ROWS + 1]" in src
    assert "s_cs_all[4][BFT_KH_ROWS_TILE + 1]" in open(os.path.join(_lib.CSRC, "bft_kh.hip")).read()
    # the rule lives in one place
    for f in ("bft_gpu.hip", "bft_kh.hip"):
        txt = open(os.path.join(_lib.CSRC, f)).read()
        assert "bft_color_rows_plan(" in txt and "1ull << div_l" not in txt


def test_dead_list_kernels_are_gone():
    for dp, _, fs in os.walk(_lib.CSRC):
        for f in fs:
            if f.endswith((".h", ".hip", ".cpp", ".c")):
                assert not re.search(r"\bk_color_(counts|fill)\b", open(os.path.join(dp, f), errors="ignore").read()), f


# ---- the symbol, the argument checks -----------------------------------------------------------------------------------------------------------------
def test_plan_symbol_is_declared_and_exported(built):
    hdr = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+bft_gpu_debug_color_rows_plan\s*\(\s*uint32_t\s+rowbytes\s*,\s*int\s+form\s*,\s*uint32_t\s+out\s*\[\s*3\s*\]\s*\)\s*;", hdr)
    assert "bft_gpu_debug_color_rows_plan" in _lib.SIGNATURES
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert "bft_gpu_debug_color_rows_plan" in set(re.findall(r" T (bft_gpu_[a-z_0-9]+)", out))


def test_plan_refuses_null_and_what_no_kernel_serves(built):
    lib = _lib.load()
    out = (C.c_uint32 * 3)(7, 7, 7)
    assert lib.bft_gpu_debug_color_rows_plan(16, 0, None) == -1  # BFT_GPU_E_ARG
    assert "NULL" in lib.bft_gpu_last_error().decode()
    for rb, form in ((0, 0), (15, 1), (15, 2), (1, 1), (16, 3), (16, -1)):
        assert lib.bft_gpu_debug_color_rows_plan(rb, form, out) == -1, (rb, form)
    assert list(out) == [7, 7, 7]
    assert lib.bft_gpu_debug_color_rows_plan(16, 1, out) == 0 and out[0] % 16 == 0 and out[0] > 0


def test_header_states_the_alignment_rule_of_d_rows():
    txt = open(_lib.HEADER).read()
    at = txt.index("int bft_gpu_query_color_rows_dev(")
    doc = txt[txt.rindex("/*", 0, at):at]
    assert "d_rows may have any alignment" in doc and "16-byte aligned" in doc
