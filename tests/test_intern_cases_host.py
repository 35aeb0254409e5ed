"""CPU-side tests (no GPU) of the colour-set interning (csrc/bft_intern.hip: bft_intern_colors_gpu and its k_cs_* kernels): the cases that
tests/test_gpu_intern_edges.py runs through the hook bft_gpu_test_intern, the truth they are held to, and a proof that each case reaches the
regime it is named for.  When a constant of the interning changes, this file fails until the cases cover every edge again.

Truth is plain numpy / Python; nothing of the library's is used:
  * the distinct lists (the bytes of their ids: `Truth.sets`, in numbering order) and, per k-mer, the list it holds (`Truth.which`);
  * the signature, restated from the text of csrc/bft_cs_sig.h in numpy.uint64 arithmetic (mix64, term, finish, and the weak form);
  * the numbering: the sets in the order of (signature, second key, first k-mer that holds the set).  Without the weak hook no two sets of a
    case share a signature, and that is the rank of the signature among the distinct lists' signatures -- the documented numbering of an image.
    Under weak hook 1 the signature is the length and the second key the real signature; under weak hook 2 both are the length.
From it follow tcol, cs_off and cs_ids exactly.

bft_cs_sig.h is device code: the restatement has NO host-side pin.  It is pinned on the GPU, by agreement with the library on every case.

Two assertions are kept apart (check_sets, check_numbering), so that a failure says which one broke.

Not constructible, and therefore without a case: a signature of 0 (cs_key's substitute), and a genuine collision of two 64-bit signatures
(or of both keys of the exact pass) -- the weak hooks stand in for the latter.  "More than 2048 distinct signatures in one workgroup's 256
lookups" cannot exist either (256 lookups carry at most 256 signatures, and a workgroup's ninth pass needs 4.7 x 10^6 lists): `alias_wg` fills a
workgroup's 256 lookups with 256 signatures of which every one shares its cache entry with another, and `grid` brings a workgroup back to a
cache that its first pass filled."""
import os
import re

import numpy as np
import pytest

from bloomfiltertrie_amd import _lib

U64 = np.uint64
ABLK = 256          # lists per workgroup and pass
WAVE = 64           # lists per wavefront; ids per step of the streamed kernels
GRID_CAP = 2048     # bft_grid_for: workgroups per launch
CS_CACHE = 2048     # k_cs_hash_insert: remembered slots per workgroup
PROBES = 64         # k_cs_hash_insert: slots tried before a lookup gives up
MIN_SLOTS = 1 << 16  # smallest hash table; accepted while the distinct signatures fill at most half of it


def test_constants_are_the_sources():
    asm = open(os.path.join(_lib.CSRC, "bft_intern.hip")).read()
    dev = open(os.path.join(_lib.CSRC, "bft_dev.h")).read()
    assert re.search(r"^#define ABLK (\d+)$", asm, flags=re.M).group(1) == str(ABLK)
    assert re.search(r"^#define CS_CACHE (\d+)u$", asm, flags=re.M).group(1) == str(CS_CACHE)
    assert "const uint32_t ch = (uint32_t)(key >> 40) & (CS_CACHE - 1u);" in asm
    assert "for (int probe = 0; probe < %d; probe++)" % PROBES in asm
    assert "uint64_t n_slots = 1ull << 16;" in asm and MIN_SLOTS == 1 << 16
    assert "while (n_slots < nk / 8 || n_slots < 3 * distinct_hint) n_slots <<= 1;" in asm
    assert "while (n_slots < 2 * nk) n_slots <<= 1;" in asm
    assert "if (scan.get(1) == 0 && scan.get(0) * 2 <= n_slots) done = true;" in asm
    assert "const uint64_t cap = 256ull * 8ull;" in dev and GRID_CAP == 256 * 8
    assert "for (uint32_t e0 = base; e0 < end; e0 += 64)" in asm and "uint32_t lo = 0, hi = 63;" in asm and WAVE == 64
    sig = open(os.path.join(_lib.CSRC, "bft_cs_sig.h")).read()
    for text in ("x ^= x >> 33; x *= 0xff51afd7ed558ccdULL; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ULL; x ^= x >> 33;",
                 "return bft_mix64((uint64_t)id + 0x632BE59BD9B4E019ULL);",
                 "return weak ? (uint64_t)len : bft_mix64(sum ^ ((uint64_t)len * 0x9E3779B97F4A7C15ULL));"):
        assert text in sig


# ---- the signature, restated (csrc/bft_cs_sig.h) ------------------------------------------------------------------------------------------------
def mix64(x):
    x = np.array(x, dtype=U64)
    with np.errstate(over="ignore"):
        x ^= x >> U64(33)
        x *= U64(0xff51afd7ed558ccd)
        x ^= x >> U64(33)
        x *= U64(0xc4ceb9fe1a85ec53)
        x ^= x >> U64(33)
    return x


def term(ids):
    with np.errstate(over="ignore"):
        return mix64(np.asarray(ids).astype(U64) + U64(0x632BE59BD9B4E019))


def finish(sums, lens, weak):
    lens = np.asarray(lens).astype(U64)
    if weak:
        return lens
    with np.errstate(over="ignore"):
        return mix64(np.asarray(sums, dtype=U64) ^ (lens * U64(0x9E3779B97F4A7C15)))


def signatures(seg_off, ids, weak=0):
    """the signature of every list (every list holds at least one id, as every k-mer of an index does)"""
    seg_off = np.asarray(seg_off, dtype=np.int64)
    assert (np.diff(seg_off) > 0).all()
    with np.errstate(over="ignore"):
        sums = np.add.reduceat(term(ids), seg_off[:-1])
    return finish(sums, np.diff(seg_off), weak)


def test_restated_signature_on_hand_computed_values():
    """(no pin against the device code is possible here: these only hold the restatement to itself)"""
    m = mix64([0, 1])
    assert int(m[0]) == 0 and int(m[1]) == 0xb456bcfc34c2cb2c  # (MurmurHash3's fmix64: 0 is its fixed point, fmix64(1) is a published value)
    s = signatures([0, 1, 3], [7, 7, 9])
    assert int(s[0]) == int(finish(term([7]), [1], 0)[0])
    with np.errstate(over="ignore"):
        assert int(s[1]) == int(finish(term([7]) + term([9]), [2], 0)[0])
    assert signatures([0, 1, 3], [7, 7, 9], weak=1).tolist() == [1, 2]
    assert len(set(signatures(np.arange(5001), np.arange(5000)).tolist())) == 5000 and (signatures(np.arange(5001), np.arange(5000)) != 0).all()


# ---- truth ---------------------------------------------------------------------------------------------------------------------------------------
class Truth:
    """which[i]: the first k-mer that holds k-mer i's list; sets: the distinct lists (bytes of their u32 ids) in numbering order; tcol, cs_off, cs_ids"""

    def __init__(self, seg_off, ids, weak):
        seg_off = np.asarray(seg_off, dtype=np.int64)
        nk = len(seg_off) - 1
        raw, first = ids.astype("<u4").tobytes(), {}
        self.which = np.empty(nk, dtype=np.int64)
        for i in range(nk):
            self.which[i] = first.setdefault(raw[4 * seg_off[i]:4 * seg_off[i + 1]], i)
        f = np.fromiter(first.values(), dtype=np.int64, count=len(first))
        lens = np.diff(seg_off).astype(U64)
        real = signatures(seg_off, ids, 0)
        sig = lens if weak else real
        key2 = real if weak == 1 else lens if weak == 2 else np.zeros(nk, dtype=U64)  # (weak 0: no two sets of a case share a signature)
        self.sig_distinct = len(set(sig[f].tolist()))
        if not weak:
            assert self.sig_distinct == len(f), "two lists of a case share a real signature"
        f = f[np.lexsort((f, key2[f], sig[f]))]
        rank = np.empty(nk, dtype=np.int64)
        rank[f] = np.arange(len(f))
        self.tcol = rank[self.which].astype(np.uint32)
        self.n_sets = len(f)
        pos = {int(i): key for key, i in first.items()}
        self.sets = [pos[int(i)] for i in f]
        self.cs_off = np.concatenate([[0], np.cumsum(np.diff(seg_off)[f])]).astype(np.uint32)
        self.cs_ids = np.frombuffer(b"".join(self.sets), dtype="<u4").astype(np.uint32)
        self.n_ids = len(self.cs_ids)
        self.collides = weak != 0 and self.sig_distinct < self.n_sets  # two different lists with one signature: the verification must object


def check_sets(seg_off, ids, truth, tcol, cs_off, cs_ids):
    """(a) every k-mer's entry equals its list; the dictionary holds each distinct list exactly once; cs_off is contiguous and ends at n_ids; ids
    ascend inside an entry.  Nothing here looks at the numbering."""
    seg_off = np.asarray(seg_off, dtype=np.int64)
    nk, lens = len(seg_off) - 1, np.diff(seg_off)
    n_sets = len(cs_off) - 1
    off = cs_off.astype(np.int64)
    assert off[0] == 0 and (np.diff(off) > 0).all() and off[-1] == len(cs_ids), "cs_off is not contiguous"
    assert len(tcol) == nk and (tcol < n_sets).all(), "a k-mer's set is outside the dictionary"
    t = tcol.astype(np.int64)
    assert ((off[t + 1] - off[t]) == lens).all(), "a k-mer's entry has another length than its list"
    at = np.repeat(off[t], lens) + (np.arange(len(ids)) - np.repeat(seg_off[:-1], lens))
    assert (cs_ids[at] == ids).all(), "a k-mer's entry differs from its list"
    inner = np.ones(len(cs_ids), dtype=bool)
    inner[off[:-1]] = False
    assert (np.diff(cs_ids.astype(np.int64), prepend=-1)[inner] > 0).all(), "ids do not ascend inside an entry"
    assert len(np.unique(t)) == n_sets, "a dictionary entry that no k-mer holds"
    assert n_sets == truth.n_sets, "%d dictionary entries for %d distinct lists" % (n_sets, truth.n_sets)
    assert len(cs_ids) == truth.n_ids


def check_numbering(truth, tcol, cs_off, cs_ids):
    """(b) the numbering: tcol is the restated rank, and with it the dictionary is the truth's byte for byte"""
    assert np.array_equal(tcol, truth.tcol), "tcol is not the rank of the signature"
    assert np.array_equal(cs_off, truth.cs_off) and np.array_equal(cs_ids, truth.cs_ids)


# ---- cases ---------------------------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, lists=None, seg_off=None, ids=None, weak=0, hint=0, narrow_w=4, about=""):
        if lists is not None:
            lens = np.fromiter((len(x) for x in lists), dtype=np.int64, count=len(lists))
            seg_off = np.concatenate([[0], np.cumsum(lens)])
            ids = np.concatenate([np.asarray(x, dtype=np.uint32) for x in lists])
        self.seg_off = np.ascontiguousarray(seg_off, dtype=np.uint32)
        self.ids = np.ascontiguousarray(ids, dtype=np.uint32)
        self.nk, self.np = len(self.seg_off) - 1, len(self.ids)
        self.weak, self.hint, self.narrow_w, self.about = weak, hint, narrow_w, about
        self._truth = None

    @property
    def truth(self):  # (computed once, shared by every test of the case, never written)
        if self._truth is None:
            self._truth = Truth(self.seg_off, self.ids, self.weak)
        return self._truth

    def first_table(self):
        n = MIN_SLOTS
        while n < self.nk // 8 or n < 3 * self.hint:
            n <<= 1
        return n

    def attempts(self):
        """hash tables a call on the hash path tries: the first one stands when the distinct signatures fill at most half of it"""
        return 1 if 2 * self.truth.sig_distinct <= self.first_table() else 2


def long_list(n, salt=0):
    return (np.arange(n, dtype=np.uint32) * 3 + 1 + salt).astype(np.uint32)


def _one(i):
    return np.array([i % 7 + 10], dtype=np.uint32)


BUILDERS = {}
LENGTHS = (1, 2, 63, 64, 65, 127, 128, 129, 4096, 70000)
NK_EDGES = (1, 63, 64, 65, 255, 256, 257)
LANES = (0, 31, 63)
TAIL_NK = WAVE + 37  # one whole wavefront and a partial one


def _register():
    B = BUILDERS
    for n in NK_EDGES:
        B["nk%d_equal" % n] = lambda n=n: Case([np.array([3, 7], np.uint32)] * n)
        B["nk%d_distinct" % n] = lambda n=n: Case([np.array([i] if i % 2 else [i, i + 5000], np.uint32) for i in range(n)])
        B["nk%d_mixed" % n] = lambda n=n: Case([[np.array([1], np.uint32), np.array([1, 2], np.uint32), np.array([2], np.uint32), long_list(5)][(i * 7 + i // 3) % 4] for i in range(n)])
    for L in LENGTHS:
        for lane in LANES:
            B["len%d_lane%d" % (L, lane)] = lambda L=L, lane=lane: Case([long_list(L) if i == WAVE + lane else _one(i) for i in range(3 * WAVE)])
        B["len%d_tail" % L] = lambda L=L: Case([long_list(L) if i == TAIL_NK - 1 else _one(i) for i in range(TAIL_NK)])
    # the second wavefront's lists total exactly 63 (a partial wavefront of 63 lists), 64, 65 and 128 ids
    B["step63"] = lambda: Case([_one(i) for i in range(WAVE + 63)])
    B["step64"] = lambda: Case([_one(i) for i in range(2 * WAVE)])
    B["step65"] = lambda: Case([np.array([4, 9], np.uint32) if i == 2 * WAVE - 1 else _one(i) for i in range(2 * WAVE)])
    B["step128"] = lambda: Case([np.array([i % 5, 100 + i % 3], np.uint32) if i >= WAVE else _one(i) for i in range(2 * WAVE)])
    B["side_by_side"] = lambda: Case([long_list(100) if i == WAVE + 10 else long_list(90, 1) if i == WAVE + 11 else _one(i) for i in range(3 * WAVE)])

    def near_equal():
        a, a2, p = long_list(70), long_list(70), long_list(40)
        a2[-1] += 1
        put = {5: a, 6: a2, 7: p, 70: a, 71: p, 300: a2, 301: a, 599: p, 598: a}  # other lanes, wavefronts, workgroups
        return Case([put.get(i, _one(i)) for i in range(600)])
    B["near_equal"] = near_equal

    def idvals(vals, w):
        vals = np.array(vals, dtype=np.uint32)
        subsets = [vals[[bool(m >> b & 1) for b in range(len(vals))]] for m in range(1, 1 << len(vals))]
        return Case([subsets[(i * 5) % len(subsets)] for i in range(300)], narrow_w=w)
    B["idvals_w1"] = lambda: idvals([0, 1, 254, 255], 1)
    B["idvals_w2"] = lambda: idvals([0, 255, 256, 65535], 2)
    B["idvals_w4"] = lambda: idvals([0, 255, 256, 65535, 65536, 2 ** 31 - 1], 4)
    B["one_hot"] = lambda: Case(seg_off=np.arange(200001) * 2, ids=np.tile(np.array([3, 9], np.uint32), 200000))
    B["per_genome"] = lambda: Case(seg_off=np.arange(200001), ids=np.random.default_rng(1).integers(0, 100, 200000))
    B["half_32768"] = lambda: Case(seg_off=np.arange(32769), ids=np.arange(32768) + 1000)
    B["half_32769"] = lambda: Case(seg_off=np.arange(32770), ids=np.arange(32769) + 1000)
    B["hint_below"] = lambda: Case(seg_off=np.arange(40001), ids=np.arange(40000) + 7, hint=21845)
    B["hint_above"] = lambda: Case(seg_off=np.arange(40001), ids=np.arange(40000) + 7, hint=21846)

    def alias_pairs(n_pairs):
        """ids whose one-id lists pair up on one cache entry ((sig >> 40) & 2047), by search over the restated signature"""
        ids = np.arange(1, 60001)
        ch = ((signatures(np.arange(len(ids) + 1), ids) >> U64(40)) & U64(CS_CACHE - 1)).astype(np.int64)
        order = np.argsort(ch, kind="stable")
        out, j = [], 0
        while len(out) < n_pairs:
            if ch[order[j]] == ch[order[j + 1]]:
                out.append((int(ids[order[j]]), int(ids[order[j + 1]])))
                j += 2 * 30  # (the next pair from another entry)
            else:
                j += 1
        return out

    def alias_wave():
        (x, y), = alias_pairs(1)
        return Case([np.array([x if (i % WAVE) in (3, 40, 41) else y if (i % WAVE) in (4, 39, 63) else 100000 + i % 9], np.uint32) for i in range(2 * ABLK)])
    B["alias_wave"] = alias_wave
    B["alias_wg"] = lambda: Case([np.array([v], np.uint32) for _ in range(2) for pair in alias_pairs(ABLK // 2) for v in pair])

    def grid():
        rng = np.random.default_rng(7)
        n_pool, nk = 5000, GRID_CAP * ABLK + 300
        plen = rng.integers(1, 4, n_pool + 1)
        pids = np.sort(rng.choice(30000, (n_pool + 1, 3), replace=True) * 3 + np.arange(3), axis=1).astype(np.uint32)  # (three distinct ids, ascending)
        pick = rng.integers(0, n_pool, nk)
        edge = GRID_CAP * ABLK
        pick[edge:edge + 300] = pick[edge - 300:edge]  # equal lists on both sides of the pass boundary (and lists seen only there)
        pick[edge + 7] = n_pool  # (a list that no k-mer of the first pass holds)
        lens = plen[pick]
        keep = np.arange(3)[None, :] < lens[:, None]
        return Case(seg_off=np.concatenate([[0], np.cumsum(lens)]), ids=pids[pick][keep])
    B["grid"] = grid

    def weak_dense(weak, nk):
        sets = [np.array(p, np.uint32) for p in ((1, 2), (1, 3), (2, 3), (0, 9), (5, 6))]

        def at(i):  # A B A B inside a wavefront, across wavefronts (i // 64) and across workgroups (i // 256)
            return sets[(i + i // WAVE + i // ABLK) % 2] if i % 5 else sets[2 + (i // 5) % 3]
        return Case([at(i) for i in range(nk)], weak=weak)
    B["weak1_dense"] = lambda: weak_dense(1, 3000)
    B["weak2_dense"] = lambda: weak_dense(2, 1500)

    def weak_sparse(weak):
        uniq = [long_list(L, L) for L in range(1, 41)]
        twins = {5: long_list(5, 77), 9: long_list(9, 78), 17: long_list(17, 79)}
        lists = []
        for r in range(4):
            for L in range(1, 41):
                lists.append(uniq[L - 1])
                if L in twins and r != 2:
                    lists.append(twins[L])
        return Case(lists, weak=weak)
    B["weak1_sparse"] = lambda: weak_sparse(1)
    B["weak2_sparse"] = lambda: weak_sparse(2)
    B["weak1_long"] = lambda: Case([long_list(200, i % 3) if i % 2 else _one(i) for i in range(130)], weak=1)


_register()
NAMES = list(BUILDERS)
_CASES = {}


def case(name):
    if name not in _CASES:
        _CASES[name] = BUILDERS[name]()
    return _CASES[name]


# ---- each case is in its regime ----------------------------------------------------------------------------------------------------------------------
def wave_steps(c, w):
    """(64-id steps of wavefront w, ids in its last step)"""
    a, b = int(c.seg_off[w * WAVE]), int(c.seg_off[min(c.nk, (w + 1) * WAVE)])
    return (b - a + WAVE - 1) // WAVE, (b - a - 1) % WAVE + 1


def longest_occupied_run(homes, n_slots):
    """linear probing: the occupied slots do not depend on the order of insertion; the longest run of them bounds every probe sequence"""
    occ = np.zeros(n_slots, dtype=bool)
    nxt = over = 0
    for h in np.sort(np.asarray(homes, dtype=np.int64)).tolist():  # in the order of their homes every key takes the first slot behind the last one
        p = max(h, nxt)
        if p >= n_slots:
            over += 1
            continue
        occ[p] = True
        nxt = p + 1
    occ[np.flatnonzero(~occ)[:over]] = True  # (inserted last, what ran off the end takes the first free slots from 0 on)
    free = np.flatnonzero(~np.concatenate([occ, occ]))  # (twice: a run may go round the end)
    return int((np.diff(free) - 1).max()) if len(free) > 1 else n_slots


@pytest.mark.parametrize("name", NAMES)
def test_case_reaches_its_regime(name):
    c = case(name)
    t = c.truth
    lens = np.diff(c.seg_off.astype(np.int64))
    assert c.nk >= 1 and (lens >= 1).all() and c.np == int(c.seg_off[-1]) < 2 ** 32
    for i in np.flatnonzero(lens > 1)[:2000]:
        assert (np.diff(c.ids[c.seg_off[i]:c.seg_off[i + 1]].astype(np.int64)) > 0).all()  # ids ascend inside a list
    if c.weak == 0:
        assert not t.collides and (signatures(c.seg_off, c.ids) != 0).all()
    m = re.match(r"nk(\d+)_(\w+)", name)
    if m:
        assert c.nk == int(m.group(1)) and c.nk in NK_EDGES
        assert {"equal": t.n_sets == 1, "distinct": t.n_sets == c.nk, "mixed": t.n_sets == min(c.nk, 4)}[m.group(2)]
    m = re.match(r"len(\d+)_(lane(\d+)|tail)", name)
    if m:
        L = int(m.group(1))
        at = TAIL_NK - 1 if m.group(2) == "tail" else WAVE + int(m.group(3))
        assert L in LENGTHS and lens[at] == L and (np.delete(lens, at) == 1).all()
        if m.group(2) == "tail":
            assert c.nk % WAVE and at // WAVE == c.nk // WAVE and at == c.nk - 1  # in the last, partial wavefront: its last list
        else:
            assert at % WAVE in LANES and at // WAVE == 1 and c.nk == 3 * WAVE
        steps, _ = wave_steps(c, at // WAVE)
        assert steps == (L + (c.nk - WAVE if m.group(2) == "tail" else WAVE) - 1 + WAVE - 1) // WAVE
        assert L < 70000 or L > 65536  # (a list longer than a u16 counts)
    if name.startswith("step"):
        total = int(name[4:])
        w_lists = c.nk - WAVE
        assert int(c.seg_off[c.nk] - c.seg_off[WAVE]) == total and w_lists == min(total, WAVE)
        assert wave_steps(c, 1) == {63: (1, 63), 64: (1, 64), 65: (2, 1), 128: (2, 64)}[total]
    if name == "side_by_side":
        a, b = WAVE + 10, WAVE + 11
        assert lens[a] > WAVE and lens[b] > WAVE
        assert (int(c.seg_off[b]) - int(c.seg_off[WAVE])) % WAVE not in (0, WAVE - 1)  # the boundary between them falls inside a step
    if name == "near_equal":
        sets = [np.frombuffer(s, dtype="<u4") for s in t.sets if len(s) > 4]
        by_len = sorted(sets, key=len)
        assert [len(s) for s in by_len] == [40, 70, 70]
        assert (by_len[1][:-1] == by_len[2][:-1]).all() and by_len[1][-1] != by_len[2][-1]  # equal but for the last id
        assert (by_len[0] == by_len[1][:40]).all()                                           # a prefix of another
        where = np.flatnonzero(t.which == 5)
        assert len({int(i) // WAVE for i in where}) >= 3 and len({int(i) // ABLK for i in where}) >= 2
    if name.startswith("idvals"):
        need = {1: {0, 255}, 2: {0, 255, 256, 65535}, 4: {0, 255, 256, 65535, 65536, 2 ** 31 - 1}}[c.narrow_w]
        assert need <= set(c.ids.tolist()) and int(c.ids.max()) < 1 << (8 * c.narrow_w) and (c.narrow_w == 4 or int(c.ids.max()) == (1 << 8 * c.narrow_w) - 1)
    if name == "one_hot":
        assert c.nk == 200000 and t.n_sets == 1
    if name == "per_genome":
        assert c.nk == 200000 and t.n_sets == 100 and (lens == 1).all()
    if name.startswith("half"):
        assert t.n_sets == c.nk == int(name[5:]) and c.first_table() == MIN_SLOTS
        assert c.attempts() == (1 if c.nk * 2 <= MIN_SLOTS else 2) == {32768: 1, 32769: 2}[c.nk]
        n_slots = MIN_SLOTS if c.attempts() == 1 else 4 * MIN_SLOTS // 2
        assert n_slots >= (1 if c.attempts() == 1 else 2) * c.nk
        homes = (signatures(c.seg_off, c.ids) & U64(n_slots - 1)).astype(np.int64)
        assert longest_occupied_run(homes, n_slots) < PROBES  # no lookup of the table that stands can give up
    if name.startswith("hint"):
        assert t.n_sets == 40000
        assert (3 * c.hint < MIN_SLOTS, c.first_table(), c.attempts()) == {"hint_below": (True, MIN_SLOTS, 2), "hint_above": (False, 2 * MIN_SLOTS, 1)}[name]
        n_slots = 2 * MIN_SLOTS
        assert longest_occupied_run((signatures(c.seg_off, c.ids) & U64(n_slots - 1)).astype(np.int64), n_slots) < PROBES
    if name.startswith("alias"):
        sig = signatures(c.seg_off, c.ids)
        ch = ((sig >> U64(40)) & U64(CS_CACHE - 1)).astype(np.int64)
        if name == "alias_wave":
            for w in range(c.nk // WAVE):
                s, h = sig[w * WAVE:(w + 1) * WAVE], ch[w * WAVE:(w + 1) * WAVE]
                assert s[3] != s[4] and h[3] == h[4] and s[40] == s[41] == s[3] and s[39] == s[63] == s[4]
        else:
            for g in range(c.nk // ABLK):
                s, h = sig[g * ABLK:(g + 1) * ABLK], ch[g * ABLK:(g + 1) * ABLK]
                assert len(set(s.tolist())) == ABLK and len(set(h.tolist())) == ABLK // 2  # 256 signatures, every one sharing its entry with another
    if name == "grid":
        edge = GRID_CAP * ABLK
        assert c.nk == edge + 300 and set(lens.tolist()) == {1, 2, 3} and 4500 <= t.n_sets <= 5000
        assert (t.which[edge:] < edge - 300).sum() > 100          # equal lists on both sides of the pass boundary
        assert (t.which[edge:] >= edge).sum() >= 1                # and a list that only the second pass sees
        assert c.attempts() == 1
    if name.startswith("weak"):
        assert c.weak == int(name[4]) and t.collides and c.attempts() == 1
    if name.endswith("_dense"):
        assert len(set(lens.tolist())) == 1 and c.nk > 2 * ABLK and t.n_sets == 5
        alt = t.which[np.arange(c.nk) % 5 != 0]
        assert (alt[:-1] != alt[1:]).mean() > 0.7  # A B A B: under a key that cannot tell them apart, nearly every list differs from its predecessor
        i = np.arange(c.nk)
        keep = (i % 5 != 0) & ((i + WAVE) % 5 != 0) & (i + WAVE < c.nk)
        assert (t.which[i[keep]] != t.which[(i + WAVE)[keep]]).any() and (t.which[i[keep]] == t.which[(i + WAVE)[keep]]).any()
    if name.endswith("_sparse"):
        cnt = np.bincount(np.array([len(s) // 4 for s in t.sets]))
        assert (cnt == 2).sum() == 3 and (cnt == 1).sum() == 37 and t.n_sets == 43  # most lengths unique, three colliding pairs


def test_every_row_of_the_plan_has_its_cases():
    want = ["nk%d_%s" % (n, kind) for n in NK_EDGES for kind in ("equal", "distinct", "mixed")]
    want += ["len%d_%s" % (L, p) for L in LENGTHS for p in ("lane0", "lane31", "lane63", "tail")]
    want += ["step63", "step64", "step65", "step128", "side_by_side", "near_equal", "idvals_w1", "idvals_w2", "idvals_w4", "one_hot", "per_genome",
             "half_32768", "half_32769", "hint_below", "hint_above", "alias_wave", "alias_wg", "grid", "weak1_dense", "weak2_dense", "weak1_sparse",
             "weak2_sparse", "weak1_long"]
    assert sorted(want) == sorted(NAMES)


# ---- the checks themselves ---------------------------------------------------------------------------------------------------------------------------
def simulate_predecessor_only(c):
    """the exact pass as it was before this file existed: a stable sort on the signature, a new set wherever a list differs from its predecessor"""
    t = c.truth
    sig = signatures(c.seg_off, c.ids, c.weak)
    order = np.argsort(sig & U64((1 << 48) - 1), kind="stable")
    w = t.which[order]
    return 1 + int((w[1:] != w[:-1]).sum())


def test_the_checks_tell_a_sound_dictionary_from_an_unsound_one():
    c = case("weak1_dense")
    t = c.truth
    check_sets(c.seg_off, c.ids, t, t.tcol, t.cs_off, t.cs_ids)
    check_numbering(t, t.tcol, t.cs_off, t.cs_ids)
    assert simulate_predecessor_only(c) > 2000 and t.n_sets == 5  # what the dense case is there to catch
    # a dictionary with one list twice: every k-mer's entry equals its list, and check_sets still objects
    dup_off = np.concatenate([t.cs_off, [t.cs_off[-1] + 2]]).astype(np.uint32)
    dup_ids = np.concatenate([t.cs_ids, t.cs_ids[:2]]).astype(np.uint32)
    dup_tcol = t.tcol.copy()
    dup_tcol[np.flatnonzero(t.tcol == 0)[0]] = t.n_sets
    with pytest.raises(AssertionError, match="6 dictionary entries for 5"):
        check_sets(c.seg_off, c.ids, t, dup_tcol, dup_off, dup_ids)
    # the same sets under another numbering: check_sets passes, check_numbering objects
    perm = np.arange(t.n_sets)[::-1]
    lens = np.diff(t.cs_off.astype(np.int64))
    sets = [t.sets[i] for i in perm]
    p_off = np.concatenate([[0], np.cumsum(lens[perm])]).astype(np.uint32)
    p_ids = np.frombuffer(b"".join(sets), dtype="<u4").astype(np.uint32)
    inv = np.empty(t.n_sets, dtype=np.uint32)
    inv[perm] = np.arange(t.n_sets)
    check_sets(c.seg_off, c.ids, t, inv[t.tcol], p_off, p_ids)
    with pytest.raises(AssertionError, match="rank"):
        check_numbering(t, inv[t.tcol], p_off, p_ids)
    wrong = t.cs_ids.copy()
    wrong[0] += 1
    with pytest.raises(AssertionError):
        check_sets(c.seg_off, c.ids, t, t.tcol, t.cs_off, wrong)
    # k_cs_hash_tcol reading a slot's `rep` for its `id`: every k-mer gets the number of a k-mer that holds its list (a mutant that is not run on
    # a device: k_cs_verify would read cs_off at that number).  Both checks object.
    as_rep = t.which.astype(np.uint32)
    with pytest.raises(AssertionError, match="outside the dictionary"):
        check_sets(c.seg_off, c.ids, t, as_rep, t.cs_off, t.cs_ids)
    with pytest.raises(AssertionError, match="rank"):
        check_numbering(t, as_rep, t.cs_off, t.cs_ids)


def test_hook_is_declared_exported_and_refuses_null():
    lib = _lib.load()
    assert "bft_gpu_test_intern" in _lib.TEST_HOOKS and "bft_gpu_test_intern" not in _lib.SIGNATURES
    assert "bft_gpu_test_intern" not in open(_lib.HEADER).read()
    import ctypes as C
    counts = (C.c_uint64 * 5)()
    assert lib.bft_gpu_test_intern(None, None, 1, 1, 0, 4, 0, None, None, 0, None, 0, None, counts, None) == -1  # BFT_GPU_E_ARG
    assert "NULL" in lib.bft_gpu_last_error().decode()
