"""The mirrored model -- canonical unitigs and degrees (bft_unitigs.hip), the MIRRORED instantiations of the path engine (bft_paths.hip) and the
compacted coloured graph (bft_cgraph.hip) -- against ground truth at every strand decision, key shape, table end, id width, threshold, cycle shape
and over link lists that take a second grid pass.  The cases and their truth come from tests/test_bidirected_cases_host.py, which proves on the CPU
that every case reaches the regime it is named after.  Every index is first checked to extract in the model's row order; then, exactly: the degree
bytes and the count of rows that are not canonical; the unitigs of both forms with the four counts of the sizing call; the five arrays and six counts
of the graph in both forms; and, on the id-width and the 40-genome cases, a colour row per segment under AND, OR and SYMDIFF."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_bidirected_cases_host as B  # noqa: E402
import test_cgraph_host as G  # noqa: E402
import test_unitigs_host as H  # noqa: E402

from bloomfiltertrie_amd import BFT, _lib, synth as S  # noqa: E402

pytestmark = pytest.mark.gpu


def _build(case):
    """the handle of a case; extract() must be in the model's order, so that "row" means the same on both sides"""
    t = BFT(case.k, device=0)
    for gid, km in case.inserts():
        t.insert_kmers(km, gid)
    km, _ = t.extract()
    assert S.packed_to_ascii(km, case.k) == case.m.rows
    return t


def _dev(n, dtype):
    import torch
    return torch.full((n,), 7, dtype=dtype, device=torch.device("cuda", 0))


def _degrees(t, m):
    deg, bad = t.bidirected_degrees()
    assert bad == m.noncanonical and deg.tobytes() == m.degrees(), (m.k, bad, [i for i, (a, b) in enumerate(zip(deg.tobytes(), m.degrees())) if a != b][:5])


def _unitigs(t, m, thr):
    """both forms, and the sizing call with no buffers: {paths, chars, longest, noncanonical}"""
    import torch
    want = m.unitigs(thr)
    problems = H.check(m, thr, H.split(*t.unitigs(thr)))
    assert problems == [], (m.k, thr, problems[:5])
    n_paths, n_chars = len(want), sum(map(len, want))
    counts = [n_paths, n_chars, max(map(len, want), default=0), 0]
    cnt = _dev(4, torch.int64)
    t.unitigs_dev(0, 0, 0, 0, cnt.data_ptr(), min_shared=thr)
    torch.cuda.synchronize()
    assert cnt.cpu().tolist() == counts, (m.k, thr)
    off, seq, cnt = _dev(n_paths + 1, torch.int64), _dev(n_chars, torch.uint8), _dev(4, torch.int64)
    t.unitigs_dev(off.data_ptr(), seq.data_ptr(), n_paths, n_chars, cnt.data_ptr(), min_shared=thr)
    torch.cuda.synchronize()
    assert cnt.cpu().tolist() == counts
    assert H.check(m, thr, H.split(off.cpu().numpy().astype(np.uint64), seq.cpu().numpy())) == [], (m.k, thr)


def _host_counts(t, thr):
    cnt = (C.c_uint64 * 6)()
    _lib.check(_lib.load().bft_gpu_unitig_graph(t._h, thr, None, None, None, None, None, 0, 0, 0, 0, cnt))
    return list(cnt)


def _graph_dev(t, k, thr, counts):
    """the device form with buffers of exactly the counted sizes: the five arrays and the six counts"""
    import torch
    ns, nc, _, _, nl, _ = counts
    nm = nc - ns * (k - 1)
    so, sq, lo = _dev(ns + 1, torch.int64), _dev(nc, torch.uint8), _dev(2 * ns + 1, torch.int64)
    lk, mem, cnt = _dev(nl, torch.int32), _dev(nm, torch.int32), _dev(6, torch.int64)
    t.unitig_graph_dev(so.data_ptr(), sq.data_ptr(), lo.data_ptr(), lk.data_ptr(), mem.data_ptr(), ns, nc, nl, nm, cnt.data_ptr(), min_shared=thr)
    torch.cuda.synchronize()
    assert cnt.cpu().tolist() == counts, (k, thr)
    return (so.cpu().numpy().astype(np.uint64), sq.cpu().numpy(), lo.cpu().numpy().astype(np.uint64), lk.cpu().numpy().view(np.uint32),
            mem.cpu().numpy().view(np.uint32))


def _same(got, want):
    return all(len(a) == len(b) and (np.asarray(a) == np.asarray(b)).all() for a, b in zip(got, want))


def _graph(t, case, thr):
    g = case.graph(thr)
    problems = G.check(g, t.unitig_graph(thr))
    assert problems == [], (case.k, thr, problems[:5])
    assert _host_counts(t, thr) == g.counts(), (case.k, thr)
    assert _same(_graph_dev(t, case.k, thr, g.counts()), g.arrays()), (case.k, thr)


def _colours(t, case, thr):
    seg_off, _, _, _, members = t.unitig_graph(thr)
    for op in ("and", "or", "symdiff"):
        rows, counts = t.unitig_colors(members, seg_off, op)
        want_rows, want_counts = case.colour_rows(thr, op)
        assert rows.shape == want_rows.shape and (rows == want_rows).all(), (case.k, thr, op)
        assert counts.tolist() == want_counts.tolist(), (case.k, thr, op)


def _run(case, thresholds=None, colours=False):
    """every call of the mirrored model on one case"""
    t = _build(case)
    _degrees(t, case.m)
    for thr in thresholds if thresholds is not None else case.thresholds:
        _unitigs(t, case.m, thr)
        _graph(t, case, thr)
        if colours:
            _colours(t, case, thr)
    return t


@pytest.mark.parametrize("k", B.KEY_SHAPES)
def test_key_shapes(k):
    _run(B.key_shape(k)).close()


@pytest.mark.parametrize("k", B.DECIDE_KS)
def test_the_deciding_nucleotide_in_every_word(k):
    """s <=> rc(s) decided at nucleotide 0, 31, 32 and k // 2 - 1, by either outcome of the read strand: beyond word 0 where the key has three words"""
    _run(B.deciding(k)).close()


@pytest.mark.parametrize("k", B.PAL_KS + B.HAIRPIN_KS)
def test_palindromes_and_hairpins_at_every_width(k):
    _run(B.situations(k), (0, 1, 2, 3)).close()


@pytest.mark.parametrize("k", B.LATE_KS)
def test_not_canonical_decided_late(k):
    """larger strands whose comparison is decided in word 1: the degrees and the count on any index; the host forms refuse and fill nothing; the device
    forms report the count"""
    import torch
    case = B.late_noncanonical(k)
    m = case.m
    t = _build(case)
    _degrees(t, m)
    assert m.noncanonical == 6
    lib = _lib.load()
    n_paths, n_chars = C.c_uint64(5), C.c_uint64(5)
    off, seq = np.full(4096, 7, dtype=np.uint64), np.full(1 << 17, 7, dtype=np.uint8)
    assert lib.bft_gpu_unitigs(t._h, 0, None, None, 0, 0, C.byref(n_paths), C.byref(n_chars)) == -4  # BFT_GPU_E_STATE
    assert lib.bft_gpu_unitigs(t._h, 0, off.ctypes.data, seq.ctypes.data, len(off) - 1, len(seq), C.byref(n_paths), C.byref(n_chars)) == -4
    assert "not canonical (6 k-mers" in lib.bft_gpu_last_error().decode() and (off == 7).all() and (seq == 7).all()
    cnt = (C.c_uint64 * 6)()
    bufs = [np.full(1 << 12, 7, dtype=np.uint64), np.full(1 << 17, 7, dtype=np.uint8), np.full(1 << 13, 7, dtype=np.uint64), np.full(1 << 14, 7, dtype=np.uint32),
            np.full(1 << 14, 7, dtype=np.uint32)]
    assert lib.bft_gpu_unitig_graph(t._h, 0, None, None, None, None, None, 0, 0, 0, 0, cnt) == -4 and cnt[3] == 6
    cnt[3] = 0
    assert lib.bft_gpu_unitig_graph(t._h, 0, *[b.ctypes.data for b in bufs], (1 << 12) - 1, 1 << 17, 1 << 14, 1 << 14, cnt) == -4
    assert "not canonical (6 k-mers" in lib.bft_gpu_last_error().decode() and cnt[3] == 6 and all((b == 7).all() for b in bufs)
    ucnt, gcnt, bad = _dev(4, torch.int64), _dev(6, torch.int64), _dev(1, torch.int64)
    t.unitigs_dev(0, 0, 0, 0, ucnt.data_ptr())
    t.unitig_graph_dev(0, 0, 0, 0, 0, 0, 0, 0, 0, gcnt.data_ptr())
    t.bidirected_degrees_dev(0, 0, bad.data_ptr())
    torch.cuda.synchronize()
    assert ucnt.cpu().tolist()[3] == gcnt.cpu().tolist()[3] == bad.cpu().tolist()[0] == m.noncanonical
    t.close()


@pytest.mark.parametrize("k", B.ENDS_KS)
def test_table_ends_of_both_searches(k):
    for table in B.ENDS_TABLES:
        _run(B.ends(k, table)).close()


@pytest.mark.parametrize("kind", B.ID_KINDS)
def test_id_widths_give_the_same_answers(kind):
    """dictionary ids of one, two and four bytes under ug_edge and k_cg_links (no call reports the width: the labellings put the largest id below
    2^8, 2^16 and above): one truth for unitigs, degrees, links and members; the colour rows at the ids' bits"""
    answers = []
    for labels in B.ID_LABELLINGS:
        case = B.id_width(kind, labels)
        t = _run(case, colours=True)
        answers.append([(thr, [x.tobytes() for x in t.unitig_graph(thr)], [x.tobytes() for x in t.unitigs(thr)]) for thr in case.thresholds])
        t.close()
    assert answers[0] == answers[1] == answers[2]


def test_shared_sets_at_the_threshold():
    case = B.shared()
    assert case.thresholds == B.SHARED_TS
    _run(case, colours=True).close()


@pytest.mark.parametrize("k", B.CUT_KS)
def test_a_threshold_cuts_a_cycle_and_splits_a_chain(k):
    case = B.cut(k)
    t = _run(case)
    assert [len(t.unitigs(thr)[0]) - 1 for thr in (0, 1, 2, 3, 4)] == [2, 2, 2, 2, 0]
    lens = np.diff(t.unitigs(3)[0].astype(np.int64)) - (k - 1)
    assert sorted(lens.tolist()) == sorted([B.CUT_RUN[0], B.CUT_CHAIN - B.CUT_RUN[1]])
    t.close()


@pytest.mark.parametrize("k", B.CYCLE_KS)
@pytest.mark.parametrize("p", B.CYCLE_PS)
def test_cycles_beside_chains(p, k):
    case = B.cycles(k, p)
    t = _run(case, (0, 1, 2, 3))
    got = H.split(*t.unitigs(0))
    for q, strand in zip(case.circles, case.strands):
        mine = [s for s in got if len(s) == p + k - 1 and B._strand_of(q, s, p)]
        assert len(mine) == 1 and B._strand_of(q, mine[0], p) == strand  # each cycle once, on the strand of its smallest row's even vertex
    t.close()


def test_dense_link_grid():
    """every canonical 10-mer: every row a single-k-mer segment, 1 049 600 oriented ends -- k_cg_links and k_cg_emit take a second grid pass and
    begin a third, 2 * segments is the number of vertices, and every end sorts four live targets"""
    vt = B.dense()
    n, k = vt.n, B.DENSE_K
    t = BFT(k, device=0)
    t.insert_kmers(vt.packed(), 0)
    km, _ = t.extract()
    assert km.shape == vt.packed().shape and (km == vt.packed()).all()
    deg, bad = t.bidirected_degrees()
    assert bad == 0 and (deg == vt.degrees()).all()
    want = vt.graph_arrays()
    for thr in (0, 1):
        off, seqs = t.unitigs(thr)
        assert off.tolist() == [0] and len(seqs) == 0  # no row is a node
        got = t.unitig_graph(thr)
        assert [len(x) for x in got] == [len(x) for x in want[:5]]
        for name, a, b in zip(("seg_off", "seqs", "link_off", "links", "members"), got, want[:5]):
            bad_at = np.flatnonzero(a != b)
            assert len(bad_at) == 0, (thr, name, len(bad_at), bad_at[:5].tolist())
        assert _host_counts(t, thr) == want[5]
    assert _same(_graph_dev(t, k, 0, want[5]), want[:5])
    import torch
    cnt = _dev(4, torch.int64)
    t.unitigs_dev(0, 0, 0, 0, cnt.data_ptr())
    torch.cuda.synchronize()
    assert cnt.cpu().tolist() == [0, 0, 0, 0]
    t.close()
