"""The library's own radix sort (csrc/bft_sort.h) and scan (csrc/bft_scan.h) at everything the build uses them for, against numpy references
computed in uint64 (a digit that ends at bit 64 of a key with its top bit set included).

Sort: every (key, value, input) the library instantiates -- u64 keys (plain and through BftCompose), u64 + u32, u32 + u32, u32 + u64, u64 +
u8 / u16 through BftPairIn, u64 + the packed 12-byte BftSplit2Val through BftSplit2In, u32 + the packed KhRec<W> records (W = 1..4) -- in the
shapes the product sorts them in plus BIG, at the one-tile / ranged boundary of each (its tile size from the library), at the ranged / chained
boundary 2^23, at bit ranges that end at the key's top bit, and over distributions that leave chains empty or put every key in one.  Every
case also checks which regime ran (bft_gpu_test_sort_last) and, where the sort made one, the digit-start table the build reads back
(last_dbase).  Payloads are random and compared byte for byte.

Scan: wrap-around, totals at the 2^62 state limit, the tail slot left alone, the look-back window and grid boundaries, the flag functors the
build scans, long sequences of different sizes on one scratch block, and a sort writing a scan's scratch block in between."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BIG, LIGHT, BACK = 0, 1, 2
CHAIN_MIN = 1 << 23  # the sort chains its later passes from 2^23 entries on (bft_sort.h: BFT_RS_CHAIN_MIN)
RUN_COPY, RUN_TILE, RUN_RANGED, RUN_CHAINED, RUN_NONE = 0, 1, 2, 3, 255
U64 = np.uint64
M64 = (1 << 64) - 1

# kind -> (key bytes, value bytes as stored in the output, what the build sorts it for)
KINDS = {0: (8, 0), 1: (8, 4), 2: (4, 4), 3: (4, 8), 4: (8, 0), 5: (8, 1), 6: (8, 2), 7: (8, 12), 8: (4, 12), 9: (4, 20), 10: (4, 28), 11: (4, 36)}


@pytest.fixture(scope="module")
def lib():
    from bloomfiltertrie_amd import _lib
    L = _lib.load()
    L.bft_gpu_test_sort_ex.restype = C.c_int
    L.bft_gpu_test_sort_ex.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint, C.c_uint, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    L.bft_gpu_test_sort_tile.restype = C.c_uint32
    L.bft_gpu_test_sort_tile.argtypes = [C.c_int, C.c_int]
    L.bft_gpu_test_sort_last.restype = C.c_int
    L.bft_gpu_test_sort_last.argtypes = [C.c_void_p, C.c_int]
    L.bft_gpu_test_scan_ex.restype = C.c_int
    L.bft_gpu_test_scan_ex.argtypes = [C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_int, C.c_uint64, C.c_void_p]
    L.bft_gpu_test_scan_seq.restype = C.c_int
    L.bft_gpu_test_scan_seq.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
    L.bft_gpu_test_scan_sort_scan.restype = C.c_int
    L.bft_gpu_test_scan_sort_scan.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.bft_gpu_last_error.restype = C.c_char_p
    return L


def _combos():
    # (kind, shape) pairs the hook is built for; kept in step with bft_gpu_test_sort_tile by test_every_kind_has_a_tile
    out = [(0, BIG), (1, BIG), (1, LIGHT), (1, BACK), (2, BIG), (2, LIGHT), (2, BACK), (3, BIG), (4, BIG), (5, BIG), (6, BIG), (7, BIG)]
    out += [(k, s) for k in (8, 9, 10, 11) for s in (BACK, BIG)]
    return out


COMBOS = _combos()


def _dev():
    import torch
    return torch.device("cuda", 0)


def _last(lib):
    w = np.zeros(40, dtype=np.uint64)
    assert lib.bft_gpu_test_sort_last(w.ctypes.data, 40) == 40
    rec = {"regime": int(w[0]), "P": int(w[1]), "tiles": int(w[2]), "ranges": int(w[3]), "tpr": int(w[4]), "tile": int(w[5])}
    rec["passes"] = [tuple(int(x) for x in w[8 + 4 * p: 12 + 4 * p]) for p in range(rec["P"])]  # (bit, nbits, chains, look-back groups)
    return rec


def _rand64(rng, n):
    return rng.integers(0, 1 << 64, size=n, dtype=np.uint64, endpoint=False)


class Case:
    """One sort: the hook's inputs (host arrays), the key the sort orders by and the payload bytes that must travel with it."""

    def __init__(self, kind, keys, raw_vals=None, param=0):
        self.kind, self.param = kind, param
        self.kbytes, self.vbytes = KINDS[kind]
        self.keys = keys  # what the hook reads as keys (u64 or u32)
        self.raw_vals = raw_vals  # what the hook reads as values (bytes / ids / word 1 + ids), or None
        n = len(keys)
        k64 = keys.astype(np.uint64)
        if kind == 4 and raw_vals is not None:  # BftCompose: (key << gb) | id
            self.sort_key = (k64 << U64(param)) | raw_vals.astype(np.uint64)
        elif kind == 7 and param not in (0, 64):  # BftSplit2In: the top 64 bits of the two words
            w1 = raw_vals[: 8 * n].view(np.uint64)
            self.sort_key = (k64 << U64(64 - param)) | (w1 >> U64(param))
        else:
            self.sort_key = k64
        if self.vbytes == 0:
            self.payload = None
        elif kind in (5, 6):  # ids narrowed to u8 / u16
            self.payload = raw_vals.view(np.uint8).reshape(n, 4)[:, : self.vbytes]
        elif kind == 7:  # {lo, id}, packed
            w1 = raw_vals[: 8 * n].view(np.uint64)
            lo = w1 if param in (0, 64) else w1 & U64((1 << param) - 1)
            ids = raw_vals[8 * n:].view(np.uint32)
            self.payload = np.concatenate([lo.view(np.uint8).reshape(n, 8), ids.view(np.uint8).reshape(n, 4)], axis=1)
        else:
            self.payload = raw_vals.view(np.uint8).reshape(n, self.vbytes)


def make_case(kind, keys, rng, gb=7, sh=64):
    """Random payloads for `keys` (u64 for 8-byte-key kinds, u32 else); the sort key is `keys` itself except for BftSplit2In at sh < 64."""
    n = len(keys)
    if kind in (0,):
        return Case(kind, keys)
    if kind == 4:
        if gb == 0:
            return Case(kind, keys)
        return Case(kind, keys >> U64(gb), (keys & U64((1 << gb) - 1)).astype(np.uint32), gb)  # (k-mer, id) whose composite is `keys`
    if kind in (1, 2, 5, 6):
        return Case(kind, keys, rng.integers(0, 1 << 32, size=n, dtype=np.uint32))
    if kind == 3:
        return Case(kind, keys, _rand64(rng, n))
    if kind == 7:
        raw = np.concatenate([_rand64(rng, n).view(np.uint8), rng.integers(0, 1 << 32, size=n, dtype=np.uint32).view(np.uint8)])
        return Case(kind, keys, raw, 0 if sh == 64 else sh)
    return Case(kind, keys, rng.integers(0, 256, size=n * KINDS[kind][1], dtype=np.uint8))


def digits(key_u64, b0, b1):
    mask = U64(((1 << (b1 - b0)) - 1) & M64)
    return (key_u64 >> U64(b0)) & mask if b1 > b0 else np.zeros(len(key_u64), dtype=np.uint64)


def ref_order(dig):
    """The stable order of uint64 digits: numpy, or -- for the largest arrays -- two stable torch sorts on the GPU over the non-negative
    32-bit halves of the digit (low half first)."""
    n = len(dig)
    if n < (1 << 22):
        return np.argsort(dig, kind="stable")
    import torch
    dev = _dev()
    lo = torch.from_numpy((dig & U64(0xFFFFFFFF)).astype(np.int64)).to(dev)
    hi = torch.from_numpy((dig >> U64(32)).astype(np.int64)).to(dev)
    o = torch.sort(lo, stable=True).indices
    o = o[torch.sort(hi[o], stable=True).indices]
    return o.cpu().numpy()


def run_sort(lib, case, shape, b0, b1, want_dbase=True):
    """Runs the hook; returns (out keys, out payload bytes (n, vbytes) or None, dbase or None) on the host."""
    import torch
    dev = _dev()
    n = len(case.keys)
    kt = torch.from_numpy(case.keys.view(np.uint8).copy()).to(dev)
    vt = torch.from_numpy(case.raw_vals.view(np.uint8).copy()).to(dev) if case.raw_vals is not None else None
    ok = torch.full((max(n, 1) * case.kbytes,), 0xA5, dtype=torch.uint8, device=dev)
    ov = torch.full((max(n, 1) * case.vbytes,), 0xA5, dtype=torch.uint8, device=dev) if case.vbytes else None
    db = np.full(512, 0xFFFFFFFF, dtype=np.uint32)
    rc = lib.bft_gpu_test_sort_ex(case.kind, shape, kt.data_ptr(), vt.data_ptr() if vt is not None else None, n, b0, b1, ok.data_ptr(),
                                  ov.data_ptr() if ov is not None else None, case.param, db.ctypes.data if want_dbase else None, None)
    assert rc == 0, (case.kind, shape, n, b0, b1, rc, lib.bft_gpu_last_error())
    torch.cuda.synchronize()
    out_k = ok.cpu().numpy().view(np.uint64 if case.kbytes == 8 else np.uint32)
    out_v = ov.cpu().numpy().reshape(-1, case.vbytes) if ov is not None else None
    del kt, vt, ok, ov
    return out_k, out_v, (db if want_dbase and int(db[0]) != 0xFFFFFFFF else None)


def expected_regime(n, b0, b1, tile):
    if n == 0:
        return RUN_NONE
    if b0 == b1:
        return RUN_COPY
    if n <= tile:
        return RUN_TILE
    if n < CHAIN_MIN or b1 - b0 <= 9:  # (one pass: ranged at any size)
        return RUN_RANGED
    return RUN_CHAINED


def check_sort(lib, case, shape, b0, b1, tile, identity=False, label=""):
    """Sorts `case` on [b0, b1) and checks keys, payload bytes, the regime and the digit-start table; returns the run record."""
    n = len(case.keys)
    out_k, out_v, db = run_sort(lib, case, shape, b0, b1)
    rec = _last(lib)
    what = (case.kind, shape, n, (b0, b1), label)
    assert rec["regime"] == expected_regime(n, b0, b1, tile), (what, rec)
    if n == 0:
        assert (out_k.view(np.uint8) == 0xA5).all() and (out_v is None or (out_v == 0xA5).all()), what
        return rec
    if rec["regime"] != RUN_COPY:
        assert rec["tile"] == tile and rec["tiles"] == (n + tile - 1) // tile, (what, rec)
    order = ref_order(digits(case.sort_key, b0, b1))
    if identity:
        assert (order == np.arange(n)).all()
    want_k = case.sort_key[order]
    if case.kbytes == 4:
        want_k = want_k.astype(np.uint32)
    bad = np.flatnonzero(out_k[:n] != want_k)
    assert bad.size == 0, (what, "keys differ from", int(bad[0]), "of", bad.size, rec)
    if case.payload is not None:
        badv = np.flatnonzero((out_v[:n] != case.payload[order]).any(axis=1))
        assert badv.size == 0, (what, "payload bytes differ from", int(badv[0]), "of", badv.size, rec)
    if rec["regime"] in (RUN_RANGED, RUN_CHAINED):
        assert db is not None, what
        bit, nb, _, _ = rec["passes"][-1]
        assert bit + nb == b1, (what, rec)
        ld = digits(want_k.astype(np.uint64), bit, bit + nb)
        cnt = np.bincount(ld.astype(np.int64), minlength=512)
        want_db = np.concatenate([[0], np.cumsum(cnt)])[:512]
        assert (db.astype(np.int64) == want_db).all(), (what, "last_dbase", np.flatnonzero(db != want_db)[:4])
    else:
        assert db is None, what
    return rec


def key_bits(kind):
    return 8 * KINDS[kind][0]


def ranges_for(kind):
    if key_bits(kind) == 64:
        # copy; 1, 9, 10, 18, 19 bits; every range that ends at the top bit; k = 31 / 32 ([0, 62), [0, 64)) and the top word at k = 63 ([0, 62))
        return [(5, 5), (63, 64), (0, 1), (55, 64), (54, 64), (46, 64), (45, 64), (0, 64), (0, 62), (3, 21), (40, 59)]
    return [(7, 7), (31, 32), (0, 1), (23, 32), (22, 32), (14, 32), (13, 32), (0, 32), (3, 21), (0, 9)]


def random_keys(kind, rng, n):
    k = _rand64(rng, n)
    return k if key_bits(kind) == 64 else (k >> U64(32)).astype(np.uint32)


def dist_keys(kind, dist, rng, n, b0, b1, plan=None):
    """Keys of distribution `dist` for the range [b0, b1) (full-width random outside what the distribution fixes)."""
    kb = key_bits(kind)
    k = random_keys(kind, rng, n).astype(np.uint64)
    rmask = U64((((1 << (b1 - b0)) - 1) << b0) & M64)
    if dist == "random":
        pass
    elif dist == "equal":
        k[:] = k[0]
    elif dist == "equal_in_range":  # only bits outside the range differ: the stable order is the identity
        k = (k & ~rmask) | (k[0] & rmask)
    elif dist == "one_digit":  # pass 0's digit takes a single value: every key of pass 1 is in one chain, the other chains are empty
        bit, nb = plan[0][:2]
        m = U64(((1 << nb) - 1) << bit)
        k = (k & ~m) | (k[0] & m)
    elif dist == "two":
        k = np.where(rng.integers(0, 2, size=n).astype(bool), k[0], k[1 % n])
    elif dist in ("sorted", "reverse"):
        k = k[np.argsort(digits(k, b0, b1), kind="stable")]
        if dist == "reverse":
            k = k[::-1].copy()
    elif dist == "runs":
        reps = rng.integers(1, 200, size=n)
        k = np.repeat(k, reps)[:n].copy()
    else:
        raise ValueError(dist)
    return k if kb == 64 else k.astype(np.uint32)


DISTS = ["random", "equal", "equal_in_range", "one_digit", "two", "sorted", "reverse", "runs"]


def plan_of(lib, kind, shape, b0, b1):
    """The passes of [b0, b1) as the library plans them (a two-entry sort records its plan)."""
    rng = np.random.default_rng(0)
    run_sort(lib, make_case(kind, random_keys(kind, rng, 2), rng), shape, b0, b1, want_dbase=False)
    return _last(lib)["passes"]


def test_every_kind_has_a_tile(lib):
    """The hook builds exactly the (kind, shape) pairs listed here; tiles are THREADS x IPT by entry size."""
    built = [(k, s) for k in KINDS for s in (BIG, LIGHT, BACK) if lib.bft_gpu_test_sort_tile(k, s)]
    assert built == sorted(COMBOS), built
    assert lib.bft_gpu_test_sort_tile(1, BIG) == 1024 * 8 and lib.bft_gpu_test_sort_tile(1, LIGHT) == 256 * 8 and lib.bft_gpu_test_sort_tile(11, BACK) == 1024


@pytest.mark.parametrize("kind,shape", COMBOS)
def test_sort_small_sizes_every_range(lib, kind, shape):
    """0, 1, 2, TILE - 1, TILE, TILE + 1 and 2 TILE + 1 entries on every bit range (one tile in LDS, then the ranged passes)."""
    tile = lib.bft_gpu_test_sort_tile(kind, shape)
    rng = np.random.default_rng(1000 + 10 * kind + shape)
    for b0, b1 in ranges_for(kind):
        for n in (0, 1, 2, tile - 1, tile, tile + 1, 2 * tile + 1):
            check_sort(lib, make_case(kind, random_keys(kind, rng, n), rng), shape, b0, b1, tile)


@pytest.mark.parametrize("kind,shape", COMBOS)
def test_sort_distributions(lib, kind, shape):
    """Every distribution, in one tile and in the ranged regime, with random payloads."""
    tile = lib.bft_gpu_test_sort_tile(kind, shape)
    rng = np.random.default_rng(2000 + 10 * kind + shape)
    kb = key_bits(kind)
    for b0, b1 in ((0, kb), (kb - 19, kb), (3, 21)):
        plan = plan_of(lib, kind, shape, b0, b1)
        for n in (tile - 3, 2 * tile + 1, 100_003):
            for dist in DISTS:
                case = make_case(kind, dist_keys(kind, dist, rng, n, b0, b1, plan), rng)
                check_sort(lib, case, shape, b0, b1, tile, identity=dist in ("equal", "equal_in_range"), label=dist)


def big_sizes(kind):
    kb = key_bits(kind)
    wide = KINDS[kind][0] + KINDS[kind][1] > 12
    return [(CHAIN_MIN - 1, (0, kb)), (CHAIN_MIN, (kb - 18, kb)), (CHAIN_MIN + 1, (0, kb - 2)), (10_000_019 if wide else 30_000_001, (0, kb))]


@pytest.mark.parametrize("kind,shape", COMBOS)
def test_sort_regime_boundaries(lib, kind, shape):
    """2^23 - 1 (ranged, more tiles than workgroups: several tiles per range), 2^23 and 2^23 + 1 (chained), and one large chained sort, on
    ranges that end at the key's top bit, full-width random keys."""
    tile = lib.bft_gpu_test_sort_tile(kind, shape)
    rng = np.random.default_rng(3000 + 10 * kind + shape)
    for n, (b0, b1) in big_sizes(kind):
        case = make_case(kind, random_keys(kind, rng, n), rng)
        rec = check_sort(lib, case, shape, b0, b1, tile)
        if rec["regime"] == RUN_RANGED:
            assert rec["tpr"] > 1 and rec["ranges"] * rec["tpr"] >= rec["tiles"], rec
        if rec["regime"] == RUN_CHAINED:
            assert all(p[2] >= 1 and p[3] >= 1 for p in rec["passes"][1:]) and rec["passes"][0][2:] == (0, 0), rec
        del case


@pytest.mark.parametrize("kind,shape", [(0, BIG), (1, BIG), (1, LIGHT), (2, BIG), (7, BIG), (8, BACK), (11, BACK)])
def test_sort_distributions_chained(lib, kind, shape):
    """The distributions that leave chains empty or crowd them, in the chained regime."""
    tile = lib.bft_gpu_test_sort_tile(kind, shape)
    rng = np.random.default_rng(4000 + 10 * kind + shape)
    kb = key_bits(kind)
    b0, b1 = (kb - 19, kb)
    plan = plan_of(lib, kind, shape, b0, b1)
    for dist in ("equal", "equal_in_range", "one_digit", "two", "reverse", "runs"):
        case = make_case(kind, dist_keys(kind, dist, rng, CHAIN_MIN + 1, b0, b1, plan), rng)
        rec = check_sort(lib, case, shape, b0, b1, tile, identity=dist in ("equal", "equal_in_range"), label=dist)
        assert rec["regime"] == RUN_CHAINED
        del case


def test_sort_compose_and_split_inputs(lib):
    """BftCompose reading plain keys (no ids) and BftSplit2In taking the top 64 bits of two words (sh < 64), as the split at k = 47 does."""
    rng = np.random.default_rng(5)
    tile4, tile7 = lib.bft_gpu_test_sort_tile(4, BIG), lib.bft_gpu_test_sort_tile(7, BIG)
    for n in (tile4 + 1, 100_003, CHAIN_MIN + 1):
        check_sort(lib, make_case(4, _rand64(rng, n), rng, gb=0), BIG, 0, 64, tile4)
        check_sort(lib, make_case(4, _rand64(rng, n), rng, gb=9), BIG, 9, 64, tile4)
    for n in (tile7, 100_003, CHAIN_MIN + 1):
        check_sort(lib, make_case(7, _rand64(rng, n), rng, sh=30), BIG, 46, 64, tile7)


def test_chained_passes_reach_both_look_back_forms(lib):
    """Between them, chained sorts launch the one-group and the all-groups look-back form (both are checked for their output)."""
    rng = np.random.default_rng(6)
    seen = set()
    for kind, shape, (b0, b1) in ((1, BIG, (46, 64)), (1, BIG, (0, 64)), (8, BACK, (14, 32)), (0, BIG, (0, 64))):
        tile = lib.bft_gpu_test_sort_tile(kind, shape)
        rec = check_sort(lib, make_case(kind, random_keys(kind, rng, CHAIN_MIN + 1), rng), shape, b0, b1, tile)
        assert rec["regime"] == RUN_CHAINED
        seen |= {p[3] for p in rec["passes"][1:]}
    assert 1 in seen and any(g > 1 for g in seen), seen


def test_sort_with_ballot_ranks_every_entry_size(lib):
    """"sort_ballots" 1 over every entry-size class (8, 9, 12, 16, 20, 40 bytes) in one tile, ranged and chained."""
    from bloomfiltertrie_amd import BFT
    w = BFT(27)
    try:
        w.set_option("sort_ballots", 1)
        rng = np.random.default_rng(7)
        seen = set()
        for kind, shape in ((0, BIG), (5, BIG), (1, LIGHT), (8, BACK), (7, BIG), (11, BIG)):
            tile = lib.bft_gpu_test_sort_tile(kind, shape)
            kb = key_bits(kind)
            for n, (b0, b1) in ((tile, (0, kb)), (3 * tile + 7, (kb - 19, kb)), (CHAIN_MIN + 1, (0, kb))):
                rec = check_sort(lib, make_case(kind, random_keys(kind, rng, n), rng), shape, b0, b1, tile, label="ballots")
                seen.add(rec["regime"])
        assert seen == {RUN_TILE, RUN_RANGED, RUN_CHAINED}
    finally:
        w.set_option("sort_ballots", 0)
        w.close()


# ---- scan ------------------------------------------------------------------------------------------------------------------------------

def run_scan(lib, kind, x, tail=True, param=0, sentinel=0x5A5A5A5A5A5A5A5A):
    import torch
    dev = _dev()
    n = len(x)
    xt = torch.from_numpy(x.view(np.uint8).copy()).to(dev)
    w = 4 if kind in (0, 4) else 8
    out = torch.from_numpy(np.full(n + 1, sentinel & ((1 << (8 * w)) - 1), dtype=np.uint32 if w == 4 else np.uint64).view(np.uint8).copy()).to(dev)
    tot = torch.zeros(1, dtype=torch.int64, device=dev)
    rc = lib.bft_gpu_test_scan_ex(kind, xt.data_ptr(), n, out.data_ptr(), tot.data_ptr(), 1 if tail else 0, param, None)
    assert rc == 0, (kind, n, rc, lib.bft_gpu_last_error())
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint32 if w == 4 else np.uint64), int(tot.cpu().numpy().view(np.uint64)[0])


def excl(x, dtype):
    c = np.cumsum(x.astype(np.uint64), dtype=np.uint64)  # (wraps modulo 2^64; masked below for u32)
    e = np.concatenate([np.zeros(1, dtype=np.uint64), c])
    return e.astype(dtype) if dtype == np.uint64 else (e & U64(0xFFFFFFFF)).astype(np.uint32)


SCAN_SIZES = [1, 4095, 4096, 4097, 64 * 4096, 64 * 4096 + 1, 65 * 4096 + 1, 2048 * 4096 + 1]


@pytest.mark.parametrize("n", SCAN_SIZES)
def test_scan_u32_wraps_and_u64_reaches_the_state_limit(lib, n):
    """u32 sums whose total wraps 2^32 (modulo 2^32), u64 sums whose total is 2^62 - 1, and all zeros: at one tile, at the 64-tile look-back window
    (64, 65 tiles and one past), and past the 2048-workgroup grid."""
    rng = np.random.default_rng(n)
    x = rng.integers(0, 1 << 32, size=n, dtype=np.uint32)
    out, tot = run_scan(lib, 0, x)
    want = excl(x, np.uint32)
    assert (out == want).all(), (n, np.flatnonzero(out != want)[:4])
    assert tot == int(want[-1])
    lim = (1 << 62) - 1
    y = rng.integers(0, max(1, lim // n), size=n, dtype=np.uint64)
    y[-1] += U64(lim - int(y.sum(dtype=np.uint64)))
    out, tot = run_scan(lib, 1, y)
    want = excl(y, np.uint64)
    assert int(want[-1]) == lim and (out == want).all() and tot == lim, (n, np.flatnonzero(out != want)[:4])
    z = np.zeros(n, dtype=np.uint64)
    out, tot = run_scan(lib, 1, z)
    assert (out == 0).all() and tot == 0


@pytest.mark.parametrize("n", [1, 4097, 65 * 4096 + 1, 2048 * 4096 + 1])
def test_scan_max_edges(lib, n):
    """Inclusive max: every value below init, a decreasing input, the maximum as the last element."""
    rng = np.random.default_rng(10 + n)
    init = 1 << 40
    x = rng.integers(0, init, size=n, dtype=np.uint64)
    out, tot = run_scan(lib, 2, x, tail=False, param=init)
    assert (out[:n] == init).all() and tot == init
    d = np.sort(rng.integers(0, 1 << 50, size=n, dtype=np.uint64))[::-1].copy()
    out, tot = run_scan(lib, 2, d, tail=False, param=3)
    assert (out[:n] == max(int(d[0]), 3)).all() and tot == max(int(d[0]), 3)
    x[-1] = U64(1 << 41)
    out, tot = run_scan(lib, 2, x, tail=True, param=5)
    want = np.maximum.accumulate(np.maximum(x, U64(5)))
    assert (out[:n] == want).all() and int(out[n]) == 1 << 41 and tot == 1 << 41


@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("n", [1, 4096, 4097, 65 * 4096 + 1, 2048 * 4096 + 1])
def test_scan_without_tail_leaves_the_slot_behind(lib, kind, n):
    rng = np.random.default_rng(20 + n + kind)
    x = rng.integers(0, 1000, size=n, dtype=np.uint32 if kind == 0 else np.uint64)
    out, tot = run_scan(lib, kind, x, tail=False, param=7)
    sentinel = 0x5A5A5A5A if kind == 0 else 0x5A5A5A5A5A5A5A5A
    assert int(out[n]) == sentinel, (kind, n)
    want = excl(x, np.uint32 if kind == 0 else np.uint64) if kind < 2 else np.concatenate([np.maximum.accumulate(np.maximum(x, U64(7))), np.zeros(1, dtype=np.uint64)])
    assert (out[:n] == want[:n]).all() and tot == int(want[n] if kind < 2 else want[n - 1]), (kind, n)


@pytest.mark.parametrize("n", [1, 4097, 65 * 4096 + 1, 3_000_017])
def test_scan_flag_functors(lib, n):
    """The exclusive sums the build takes over flags computed on the fly: BftPairFlags over sorted composites ((first of its k-mer) << 32 |
    (first of its (k-mer, genome))), and BftSpHead over (head, distance) pairs."""
    rng = np.random.default_rng(30 + n)
    gb = 5
    c = np.sort(rng.integers(0, max(2, n // 3), size=n, dtype=np.uint64) << U64(gb) | rng.integers(0, 3, size=n, dtype=np.uint64))
    prev = np.concatenate([~c[:1], c[:-1]])
    f = (((c >> U64(gb)) != (prev >> U64(gb))).astype(np.uint64) << U64(32)) | (c != prev).astype(np.uint64)
    out, tot = run_scan(lib, 3, c, tail=True, param=gb)
    want = excl(f, np.uint64)
    assert (out == want).all() and tot == int(want[-1]), np.flatnonzero(out != want)[:4]
    hx = np.where(rng.integers(0, 4, size=n) == 0, np.arange(n), rng.integers(0, n, size=n)).astype(np.uint32)
    hd = hx.astype(np.uint64) | (rng.integers(0, 1 << 32, size=n, dtype=np.uint64) << U64(32))  # uint2 {head, distance}, one 8-byte element each
    out, tot = run_scan(lib, 4, hd, tail=False)
    heads = (hx == np.arange(n, dtype=np.uint32)).astype(np.uint32)
    want = excl(heads, np.uint32)
    assert (out[:n] == want[:n]).all() and tot == int(want[n]) and int(out[n]) == 0x5A5A5A5A


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_scans_of_different_sizes_share_one_block(lib, kind):
    """30 x 10^6, 1, 5000, 65 x 4096 + 1, 30 x 10^6 on ONE scratch block, as the library's long-lived blocks are used: every launch zeroes what
    the one before it left, whatever its size."""
    import torch
    dev = _dev()
    sizes = [30_000_000, 1, 5000, 65 * 4096 + 1, 30_000_000, 4097]
    rng = np.random.default_rng(40 + kind)
    dt = np.uint32 if kind == 0 else np.uint64
    x = rng.integers(0, 1 << 32 if kind == 0 else 1 << 34, size=max(sizes), dtype=dt)
    xt = torch.from_numpy(x.view(np.uint8).copy()).to(dev)
    outs = [torch.full((n + 1,), -1, dtype=torch.int32 if kind == 0 else torch.int64, device=dev) for n in sizes]
    ptrs = (C.c_void_p * len(sizes))(*[o.data_ptr() for o in outs])  # (kept alive until the call returns)
    sz = np.array(sizes, dtype=np.uint64)
    tots = torch.zeros(len(sizes), dtype=torch.int64, device=dev)
    assert lib.bft_gpu_test_scan_seq(kind, xt.data_ptr(), sz.ctypes.data, len(sizes), C.cast(ptrs, C.c_void_p), tots.data_ptr(), 9, None) == 0, lib.bft_gpu_last_error()
    torch.cuda.synchronize()
    tots = tots.cpu().numpy().view(np.uint64)
    full = excl(x, dt) if kind < 2 else np.maximum.accumulate(np.maximum(x, U64(9)))
    for i, n in enumerate(sizes):
        o = outs[i].cpu().numpy().view(dt)
        if kind < 2:
            assert (o == full[: n + 1]).all() and int(tots[i]) == int(full[n]), (kind, i, n, np.flatnonzero(o != full[: n + 1])[:4])
        else:
            assert (o[:n] == full[:n]).all() and int(o[n]) == int(full[n - 1]) == int(tots[i]), (kind, i, n)


def test_a_sort_on_a_scans_block_hands_it_back_zeroed(lib):
    """scan (2^25) -> sort (a ranged sort of 50 000 keys, whose scratch fits the scan's block) -> scan, one block: the sort must leave the block's
    tag at 0, or the second scan would claim tiles from the sort's words (the hook refuses to launch it then)."""
    import torch
    dev = _dev()
    rng = np.random.default_rng(50)
    n, m = 1 << 25, 50_000
    x = torch.from_numpy(rng.integers(0, 1000, size=n, dtype=np.uint32)).to(dev)
    keys = _rand64(rng, m)
    kt = torch.from_numpy(keys.view(np.int64).copy()).to(dev)
    o1 = torch.full((n + 1,), -1, dtype=torch.int32, device=dev)
    o2 = torch.full((n + 1,), -1, dtype=torch.int32, device=dev)
    sk = torch.empty(m, dtype=torch.int64, device=dev)
    info = np.zeros(3, dtype=np.uint64)
    rc = lib.bft_gpu_test_scan_sort_scan(x.data_ptr(), n, kt.data_ptr(), m, o1.data_ptr(), o2.data_ptr(), sk.data_ptr(), info.ctypes.data, None)
    torch.cuda.synchronize()
    assert int(info[1]) == int(info[2]) and int(info[1]) > 0, info  # (the sort did use the scan's block as it was)
    assert rc == 0 and int(info[0]) == 0, (rc, info, lib.bft_gpu_last_error())
    want = excl(x.cpu().numpy(), np.uint32)
    assert (o1.cpu().numpy().view(np.uint32) == want).all() and (o2.cpu().numpy().view(np.uint32) == want).all()
    assert (sk.cpu().numpy().view(np.uint64) == np.sort(keys)).all()
