"""The build's front end behind the root-prefix split (csrc/bft_front.hip: k_bucket_sort_wave, k_bucket_sort, k_bucket2_tiny, k_bucket2_sort_wave,
k_bucket2_sort, the two emit kernels) against ground truth at every size class, key width, id width and fallback.  The cases and their truth come
from tests/test_front_cases_host.py, which proves on the CPU -- with the library's own selection rules, bft_gpu_debug_front_plan -- that every case
runs the kernel it is named after; here every case is built with "build_msd" 2 (the split at any size) and compared exactly: the extracted k-mers
in the order of their T-form keys, the colour set of every k-mer, the numbers of distinct k-mers and pairs (where a lost stability shows: duplicate
pairs stop being neighbours), presence of every stored k-mer and absence of one-base mutants.  The counters are asserted, so that no case passes
by another road: "sort_max_bucket" is the truth's largest bucket -- also where the front end declines and the device-wide sort builds the index --,
"sort_redone_buckets" is 0 as shipped and, under "test_front_rank_mode" 1 and 2, the number of buckets the plan gives to a radix kernel, and the
kernel that sorted the largest bucket (bft_gpu_debug_front_last, written where the kernels are launched) is the one the rules, as DESIGN.md states
them, name for that size; the road of the build, its id bits and id width (bft_gpu_debug_run_road) are those the case's road is named after."""
import contextlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_front_cases_host as H  # noqa: E402

from bloomfiltertrie_amd import BFT  # noqa: E402

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def front_options(mode=0, wave_cap=0):
    """the two process-wide test hooks, back at their defaults afterwards"""
    w = BFT(9)
    try:
        w.set_option("test_front_rank_mode", mode)
        w.set_option("test_front_wave_cap", wave_cap)
        yield
    finally:
        w.set_option("test_front_rank_mode", 0)
        w.set_option("test_front_wave_cap", 0)
        w.close()


def _handle(c, msd=2, composite=1):
    t = BFT(c.k)
    t.set_option("build_msd", msd)
    if c.words == 1:
        t.set_option("composite_log", c.comp_log)
    t.set_option("build_composite", composite)
    return t


def _insert(t, calls):
    for gid, km in calls:
        t.insert_kmers(km, gid)
    t.build()
    return t.build_time()


def _check(t, tr, seed=0):
    km, cs = t.extract()
    assert km.shape == tr.packed.shape and (km == tr.packed).all(), (km.shape, tr.packed.shape)
    sets = {c: tuple(t.colorset(c)) for c in np.unique(cs).tolist()}
    got, want = [sets[c] for c in cs.tolist()], [tr.sets[x] for x in tr.order]
    assert got == want, [i for i, (a, b) in enumerate(zip(got, want)) if a != b][:5]
    info = t.info()
    assert (info["kmers"], info["pairs"]) == (tr.kmers, tr.pairs)
    present = np.unpackbits(t.query_presence(tr.packed), bitorder="little")[:tr.kmers]
    assert present.all()
    absent = tr.absent(64, seed)
    assert len(absent) and not np.unpackbits(t.query_presence(absent), bitorder="little")[:len(absent)].any()


def _run(c, mode=0, wave_cap=0):
    with front_options(mode, wave_cap):
        t = _handle(c)
        try:
            bt = _insert(t, c.inserts())
            ran = H.last_kernel()
            assert H.run_road(t) == H.want_road(c.road)  # composites or pairs, the id bits and the id width the road is named after
            _check(t, c.truth)
        finally:
            t.close()
    assert int(bt["sort_max_bucket"]) == c.truth.max_bucket  # the split ran, and counted what was inserted
    # the kernel that sorted the largest bucket is the one the case is named after (the rules as stated, not as the library has them)
    assert ran == (H.want_kernel(c.road, c.truth.max_bucket, wave_cap), c.truth.max_bucket), ran
    return int(bt["sort_redone_buckets"])


@pytest.mark.parametrize("road,size,wave_cap", H.CASES, ids=lambda x: str(x))
def test_case_against_truth(road, size, wave_cap):
    """every road at every size class, as shipped: no bucket fails its order check"""
    assert _run(H.case(road, size, wave_cap), 0, wave_cap) == 0


@pytest.mark.parametrize("mode", (1, 2))
@pytest.mark.parametrize("road,size,wave_cap", H.MODE_CASES, ids=lambda x: str(x))
def test_rank_modes_against_truth(road, size, wave_cap, mode):
    """ballot ranks only (1) and an order check that always fails (2): the fallback launch sorts exactly the buckets the radix kernels own"""
    c = H.case(road, size, wave_cap)
    assert _run(c, mode, wave_cap) == c.redone()


@pytest.mark.parametrize("road,size,wave_cap", H.CAP_CASES, ids=lambda x: str(x))
def test_forced_wave_cap_against_truth(road, size, wave_cap):
    """the rule's cases with the wavefront kernel's share forced: 1024 runs k_bucket_sort_wave<16> and hands k_bucket_sort the buckets beyond 1024"""
    assert _run(H.case(road, size), 0, wave_cap) == 0


@pytest.mark.parametrize("road", H.TWO_STEP_ROADS)
def test_second_build_merges_into_the_first(road):
    """the front end's output is a run the merge consumes: a second insert goes through the front end again and is merged into the index"""
    a, calls, second, tr = H.two_step(road)
    t = _handle(a)
    try:
        bt = _insert(t, a.inserts())
        assert int(bt["sort_max_bucket"]) == a.truth.max_bucket and int(bt["sort_redone_buckets"]) == 0
        _check(t, a.truth)
        bt = _insert(t, calls)
        assert int(bt["sort_max_bucket"]) == second.max_bucket and int(bt["sort_redone_buckets"]) == 0
        _check(t, tr, 1)
    finally:
        t.close()


@pytest.mark.parametrize("road,why", [("k37", "order"), ("k63_big", "order"), ("k37", "composite"), ("k64", "composite"), ("k27_gb9", "composite"), ("k31_b2", "composite"),
                                      ("k27_gb9", "order"), ("k31_b2", "order")])
def test_the_split_is_not_taken(road, why):
    """genome ids that do not ascend, or "build_composite" 0: the general sort builds the same index and no bucket is counted"""
    c = H.case(road, 513)
    calls = c.inserts()
    if why == "order":
        calls = calls[1:] + calls[:1]
        assert [g for g, _ in calls] != sorted(g for g, _ in calls)
    t = _handle(c, composite=0 if why == "composite" else 1)
    H.last_raw()  # (reading clears the record)
    try:
        bt = _insert(t, calls)
        assert int(bt["sort_max_bucket"]) == 0 and int(bt["sort_redone_buckets"]) == 0 and H.last_raw() == [0] * 8  # the front end was not called
        assert H.run_road(t) == [2, H.bits_for(max(c.gids)), 4, 0]  # the general road, the split not tried
        _check(t, c.truth)
    finally:
        t.close()
