"""The colour-set interning (csrc/bft_intern.hip: bft_intern_colors_gpu, the k_cs_* kernels) at every list, wavefront and table edge.

The cases, their truth and the proof that each reaches its regime are tests/test_intern_cases_host.py's (no GPU).  Here every case goes through
the hook bft_gpu_test_intern in its three modes -- 0: the hash path on the caller's stream; 1: the tail deferred to a side stream, its verdict
collected and the exact call made on collisions, as a fresh build does; 2: the exact pass at once -- on the default stream and on a stream of
the test's own, and exactly:
  (a) sets: every k-mer's entry equals its list, the dictionary holds each distinct list once, cs_off is contiguous, ids ascend;
  (b) numbering: tcol, cs_off and cs_ids are the truth's, i.e. the sets are numbered by (signature, second key, first k-mer) -- the rank of the
      signature wherever no two sets share one.  This is also what pins the host file's restatement of csrc/bft_cs_sig.h;
  * every output sits between canaries, and nothing behind the reported sizes is written;
  * counts: exact passes taken, hash tables tried, whether the deferred tail reported collisions;
  * mode 1: the ids the tail narrowed to 1 / 2 bytes, byte for byte.
Through the product: a fresh build and the same index grown in three merges, ordinary and under the weak-signature hook, against ground truth
from the inserted genomes; the colours after the collision recovery through the default query path and through the containers; and an ordinary
build after the hook is restored.  The largest inputs are `grid` (0.5 M lists, 1 M ids) and the 70 000-id lists."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_intern_cases_host as H  # noqa: E402

from bloomfiltertrie_amd import BFT, _lib, synth as S  # noqa: E402

pytestmark = pytest.mark.gpu

PAD = 256      # canary bytes on either side of an output
CANARY = 0xA5
E_NOSPACE = -6  # BFT_GPU_E_NOSPACE (include/bft_gpu.h)


class Guarded:
    """`nbytes` of device memory between two canary stretches, all of it filled with the canary byte"""

    def __init__(self, nbytes):
        self.nbytes = int(nbytes)
        self.t = torch.full((2 * PAD + self.nbytes + (-self.nbytes) % 16,), CANARY, dtype=torch.uint8, device="cuda:0")
        self.ptr = self.t.data_ptr() + PAD

    def read(self, used, dtype):
        """the first `used` bytes; everything else must still be the canary"""
        host = self.t.cpu().numpy()
        assert used <= self.nbytes
        assert (host[:PAD] == CANARY).all() and (host[PAD + used:] == CANARY).all(), "written outside the reported size"
        return host[PAD:PAD + used].copy().view(dtype)


@pytest.fixture(scope="module")
def ctl():
    """a handle for the process-wide weak-signature hook; restored to 0 whatever happens"""
    t = BFT(27)
    yield t
    t.set_option("test_weak_signature", 0)
    t.close()


@pytest.fixture(scope="module")
def side_stream():
    return torch.cuda.Stream(device="cuda:0")


_DEV = {}  # case name -> (seg_off, ids) on the device, uploaded once


def _device_lists(name):
    if name not in _DEV:
        c = H.case(name)
        _DEV[name] = (torch.from_numpy(c.seg_off.view(np.int32)).to("cuda:0"), torch.from_numpy(c.ids.view(np.int32)).to("cuda:0"))
    return _DEV[name]


def intern(name, mode, stream=None, narrow_w=None, cs_off_cap=None, cs_ids_cap=None):
    """one call of the hook: (rc, counts, tcol, cs_off, cs_ids, narrowed bytes or None)"""
    c = H.case(name)
    lib = _lib.load()
    d_off, d_ids = _device_lists(name)
    w = narrow_w or c.narrow_w
    cs_off_cap = c.nk + 1 if cs_off_cap is None else cs_off_cap  # (at most one set per list, one id per id)
    cs_ids_cap = c.np if cs_ids_cap is None else cs_ids_cap
    tcol, cs_off, cs_ids, narrow = Guarded(4 * c.nk), Guarded(4 * cs_off_cap), Guarded(4 * cs_ids_cap), Guarded(w * cs_ids_cap)
    counts = (C.c_uint64 * 5)()
    torch.cuda.synchronize()
    rc = lib.bft_gpu_test_intern(d_off.data_ptr(), d_ids.data_ptr(), c.nk, c.np, mode, w, c.hint, tcol.ptr, cs_off.ptr, cs_off_cap, cs_ids.ptr, cs_ids_cap,
                                 narrow.ptr, counts, stream.cuda_stream if stream is not None else None)
    counts = [int(x) for x in counts]
    if rc != 0:
        for g in (tcol, cs_off, cs_ids, narrow):
            g.read(0, np.uint8)  # nothing copied
        return rc, counts, None, None, None, None
    n_sets, n_ids = counts[0], counts[1]
    narrowed = mode == 1 and w < 4 and counts[3] == 0
    return (rc, counts, tcol.read(4 * c.nk, np.uint32), cs_off.read(4 * (n_sets + 1), np.uint32), cs_ids.read(4 * n_ids, np.uint32),
            narrow.read(w * n_ids if narrowed else 0, np.uint8))


def expected_counts(c, mode, counts):
    t = c.truth
    assert counts[0] == t.n_sets and counts[1] == t.n_ids, "%d dictionary entries (%d ids) for %d distinct lists (%d ids)" % (counts[0], counts[1], t.n_sets, t.n_ids)
    if mode == 2:
        assert counts[2:] == [1, 0, 0], counts
    else:
        assert counts[2] == (1 if t.collides else 0), "exact passes: %r" % (counts,)
        assert counts[4] == c.attempts(), "hash tables tried: %r" % (counts,)
        assert (counts[3] > 0) == (mode == 1 and t.collides), "collisions the tail reported: %r" % (counts,)


@pytest.mark.parametrize("mode", (0, 1, 2))
@pytest.mark.parametrize("name", H.NAMES)
def test_intern_case(name, mode, ctl, side_stream):
    c = H.case(name)
    t = c.truth
    ctl.set_option("test_weak_signature", c.weak)
    try:
        for stream in (None, side_stream):
            rc, counts, tcol, cs_off, cs_ids, narrow = intern(name, mode, stream)
            assert rc == 0, _lib.load().bft_gpu_last_error()
            print(name, mode, "default" if stream is None else "own stream", "counts", counts, "truth", t.n_sets, t.n_ids)
            assert counts[0] + 1 == len(cs_off) and counts[1] == len(cs_ids)
            H.check_sets(c.seg_off, c.ids, t, tcol, cs_off, cs_ids)   # (a)
            H.check_numbering(t, tcol, cs_off, cs_ids)                # (b)
            expected_counts(c, mode, counts)
            if mode == 1 and c.narrow_w < 4 and not t.collides:
                want = t.cs_ids.astype({1: np.uint8, 2: np.dtype("<u2")}[c.narrow_w]).view(np.uint8)
                assert (t.cs_ids < 1 << (8 * c.narrow_w)).all() and np.array_equal(narrow, want), "narrowed ids"
    finally:
        ctl.set_option("test_weak_signature", 0)


@pytest.mark.parametrize("w", (1, 2))
def test_deferred_tail_narrows_a_long_list(w, ctl):
    """the tail's narrowing over more ids than one pass of its grid-stride loop covers in a workgroup: the 70 000-id list, ids reduced to the width"""
    name = "len70000_lane31"
    c = H.case(name)
    assert c.weak == 0
    rc, counts, tcol, cs_off, cs_ids, narrow = intern(name, 1, None, narrow_w=w)
    assert rc == 0 and counts[3] == 0
    H.check_numbering(c.truth, tcol, cs_off, cs_ids)
    # (ids beyond the width: the product never asks for that; the kernel's cast is what is held here)
    assert np.array_equal(narrow, c.truth.cs_ids.astype({1: np.uint8, 2: np.dtype("<u2")}[w]).view(np.uint8))


@pytest.mark.parametrize("mode", (0, 1, 2))
def test_too_small_a_capacity_copies_nothing(mode, ctl):
    c = H.case("near_equal")
    t = c.truth
    for caps in ({"cs_off_cap": t.n_sets}, {"cs_ids_cap": t.n_ids - 1}):
        rc, counts, *_ = intern("near_equal", mode, None, **caps)  # (intern() checks that every output is still all canary)
        assert rc == E_NOSPACE and counts[0] == t.n_sets and counts[1] == t.n_ids
    rc, counts, tcol, cs_off, cs_ids, _ = intern("near_equal", mode, None, cs_off_cap=t.n_sets + 1, cs_ids_cap=t.n_ids)
    assert rc == 0
    H.check_numbering(t, tcol, cs_off, cs_ids)


# ---- through the product -------------------------------------------------------------------------------------------------------------------------
K = 27
GIDS = (0, 1, 2, 300, 301)  # (the dictionary's ids take two bytes)


@pytest.fixture(scope="module")
def genomes():
    anc = S.random_genome(3000, 3)
    return {g: S.distinct(S.kmers_of(S.mutate(anc, 0.03, 40 + i), K)) for i, g in enumerate(GIDS)}


@pytest.fixture(scope="module")
def ground(genomes):
    """{packed k-mer bytes: ascending genome ids}"""
    truth = {}
    for g in GIDS:
        for row in genomes[g]:
            truth.setdefault(row.tobytes(), []).append(g)
    assert 10 < len({tuple(v) for v in truth.values()}) <= 31
    return truth


def _build(genomes, groups):
    t = BFT(K)
    for grp in groups:
        for g in grp:
            t.insert_kmers(genomes[g], g)
        t.build()
    return t


def _holds_the_truth(t, ground, weak, numbering=True):
    """tcol, every colorset, the number of sets and the dictionary's id width of a handle, against the truth of its k-mers in table order"""
    km, cs = t.extract()
    assert len(km) == len(ground)
    lists = [np.array(ground[row.tobytes()], dtype=np.uint32) for row in km]
    c = H.Case(lists, weak=weak)
    tr = c.truth
    info, fp = t.info(), t.footprint()
    assert info["colorsets"] == tr.n_sets, "%d colour sets for %d distinct sets" % (info["colorsets"], tr.n_sets)
    sets = [np.array(t.colorset(s), dtype=np.uint32) for s in range(info["colorsets"])]
    cs_off = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.uint32)
    cs_ids = np.concatenate(sets).astype(np.uint32)
    assert np.array_equal(t.debug_array("tcol", np.uint32), cs)
    H.check_sets(c.seg_off, c.ids, tr, cs, cs_off, cs_ids)
    if numbering:
        H.check_numbering(tr, cs, cs_off, cs_ids)
    assert fp["colorset_dictionary"] == 4 * (tr.n_sets + 1) + 2 * tr.n_ids  # ids up to 301: two bytes each
    return tr


FRESH = (GIDS,)
MERGED = ((0, 1), (2,), (300,), (301,))  # a first build and three merges


@pytest.mark.parametrize("groups", (FRESH, MERGED), ids=("fresh", "three_merges"))
def test_product_dictionary_is_the_truths(genomes, ground, groups):
    t = _build(genomes, groups)
    before = t.build_time()["intern_exact_passes"]
    tr = _holds_the_truth(t, ground, 0)
    assert not tr.collides and t.build_time()["intern_exact_passes"] == before
    t.close()


@pytest.mark.parametrize("groups", (FRESH, MERGED), ids=("fresh", "three_merges"))
def test_product_dictionary_under_the_weak_hook(genomes, ground, groups, ctl):
    """(under hook 1 the numbering is (length, real signature): a function of the lists alone, so a merge numbers like a fresh build)"""
    before = ctl.build_time()["intern_exact_passes"]
    ctl.set_option("test_weak_signature", 1)
    try:
        t = _build(genomes, groups)
    finally:
        ctl.set_option("test_weak_signature", 0)
    assert t.build_time()["intern_exact_passes"] >= before + len(groups)  # every build and every merge took the exact pass
    tr = _holds_the_truth(t, ground, 1)
    assert tr.collides
    t.close()


def test_product_under_weak_hook_2_holds_the_sets(genomes, ground, ctl):
    """neither key tells two lists of one length apart: the exact pass finds equal lists among the earlier ones of the tie (the merge's lists come
    in another order than a build's, so only the sets are held here, not their numbers)"""
    ctl.set_option("test_weak_signature", 2)
    try:
        fresh, merged = _build(genomes, FRESH), _build(genomes, MERGED)
    finally:
        ctl.set_option("test_weak_signature", 0)
    _holds_the_truth(fresh, ground, 2)
    _holds_the_truth(merged, ground, 2, numbering=False)
    fresh.close()
    merged.close()


def test_colours_after_the_collision_recovery(genomes, ground, ctl):
    """a fresh build whose deferred tail reports collisions interns again, exactly, and derives the k-mer hash from the committed table: colours
    through the default query path, and through the containers ("kmer_hash" 0)"""
    ctl.set_option("test_weak_signature", 1)
    try:
        t = _build(genomes, FRESH)
    finally:
        ctl.set_option("test_weak_signature", 0)
    q = np.ascontiguousarray(np.concatenate([genomes[g] for g in GIDS]))
    for how in ("default", "containers"):
        bits, off, ids = t.query_colors(q)
        assert S.from_bits(bits, len(q)).all(), how
        off = off.astype(np.int64)
        for i in range(len(q)):
            assert ids[off[i]:off[i + 1]].tolist() == ground[q[i].tobytes()], (how, i)
        t.set_option("kmer_hash", 0)
    t.close()


def test_an_ordinary_build_after_the_hook_is_restored(genomes, ground, ctl):
    """(last in the file: every test above switches the hook off in a `finally`)"""
    before = ctl.build_time()["intern_exact_passes"]
    t = _build(genomes, MERGED)
    assert t.build_time()["intern_exact_passes"] == before
    _holds_the_truth(t, ground, 0)
    t.close()
