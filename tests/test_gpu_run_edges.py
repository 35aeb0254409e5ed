"""The device-wide roads of the build's run stage (csrc/bft_run.hip: composite_sort, pairs_sort -> sort_dedupe_w1_narrow -> dedupe_w1, general_sort ->
bft_sort_pairs, with k_gather_pairs, k_flags, k_scatter, k_scatter_c, k_scatter_2 and the log's own k_log_decompose) against ground truth at every edge.
The cases and their truth come from tests/test_run_cases_host.py, which proves on the CPU -- with the library's own road rules, bft_gpu_debug_run_plan,
and a counted table of conditions -- that every case is what it is named after; here every case is built on one handle with its options and compared
exactly (test_run_cases_host.compare): the extracted k-mers in the order of their T-form keys, the colour set of every k-mer as colorset() returns it
(not re-sorted), info()'s numbers of distinct k-mers and pairs, presence of every stored k-mer and absence of 64 one-base mutants.  The road of the
build (bft_gpu_debug_run_road) is the one written by hand beside the case, and where that road does not try the root-prefix split no bucket is counted
and the front end is not called (bft_gpu_debug_front_last reads all zero).  An insert call of no k-mers goes to the library through _lib with n = 0."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_front_cases_host as H  # noqa: E402  (last_raw, run_road)
import test_run_cases_host as R  # noqa: E402

from bloomfiltertrie_amd import BFT, _lib  # noqa: E402

pytestmark = pytest.mark.gpu


def _handle(c):
    t = BFT(c.k)
    for name, value in c.options.items():
        if name != "composite_log" or c.W == 1:
            t.set_option(name, value)
    return t


def _insert(t, calls):
    for gid, km in calls:
        if len(km) == 0:
            _lib.check(_lib.load().bft_gpu_insert_kmers(t._h, None, 0, gid))  # (BFT.insert_kmers would hand it on as well: the library returns first)
        else:
            t.insert_kmers(km, gid)


def _insert_resident(t, c):
    """the calls of a table case out of one resident array of packed k-mers"""
    import torch
    base, calls = c.dev
    packed = R.G.pack(base)
    d = torch.from_numpy(packed).cuda()
    torch.cuda.synchronize()
    ptr, nb = d.data_ptr(), packed.shape[1]
    fn, h = _lib.load().bft_gpu_insert_kmers_dev, t._h
    for gid, first, n in calls:
        rc = fn(h, ptr + first * nb, n, gid)
        if rc:
            _lib.check(rc)
    return d


def _build(t, road):
    H.last_raw()  # (reading clears the record)
    t.build()
    bt = t.build_time()
    assert H.run_road(t) == road
    front = H.last_raw()
    if road[3] == 0:  # the split is not tried: no bucket is counted, the front end is not called
        assert int(bt["sort_max_bucket"]) == 0 and int(bt["sort_redone_buckets"]) == 0 and front == [0] * 8
    else:
        assert int(bt["sort_max_bucket"]) > 0 and int(bt["sort_redone_buckets"]) == 0 and front[0] == 1


def _check(t, tr, seed=0):
    km, cs = t.extract()
    sets = {c: t.colorset(c) for c in np.unique(cs).tolist()}
    info = t.info()
    assert R.compare(tr, km, cs, sets, info["kmers"], info["pairs"]) == []
    present = np.unpackbits(t.query_presence(tr.packed), bitorder="little")[:tr.kmers]
    assert present.all()
    absent = tr.absent(64, seed)
    assert len(absent) and not np.unpackbits(t.query_presence(absent), bitorder="little")[:len(absent)].any()


def _run(c):
    t = _handle(c)
    try:
        if c.first is not None:
            _insert(t, c.inserts(c.first))
            _build(t, c.first_road)
            _check(t, c.truth_first, 1)
        keep = _insert_resident(t, c) if c.dev else _insert(t, c.inserts())
        _build(t, c.road)
        del keep
        _check(t, c.truth)
    finally:
        t.close()


@pytest.mark.parametrize("name", R.QUICK)
def test_case_against_truth(name):
    """every road family at every ending, size, key shape, id width and call-table shape; the two-step cases are checked after each build"""
    _run(R.case(name))


@pytest.mark.parametrize("name", list(R.MEDIUM))
def test_table_and_log_cases_against_truth(name):
    """65 536 | 65 537 entries in the table of insert calls; a log of composites taken apart at an id without room and grown behind it"""
    _run(R.case(name))


@pytest.mark.parametrize("name", list(R.LARGE))
def test_large_cases_against_truth(name):
    """a second grid pass of every kernel of the composite and of the W = 3 road; 2^20 - 1 | 2^20 pairs under "build_msd" 1"""
    _run(R.case(name))
