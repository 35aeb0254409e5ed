"""Bubbles on the compacted coloured graph and the k-mer -> segment table on the GPU (bft_gpu_unitig_bubbles / _dev, bft_gpu_unitig_segment_of / _dev,
BFT.unitig_bubbles, BFT.unitig_segment_of, BFT.bubbles): exact against the model of tests/test_bubbles_host.py, which is written from the definition
alone and proves its invariants on the same cases on the CPU.  Real indexes at every key width and threshold, the hand-made situations, the planted
variants end to end with the colours of every allele; hand-made link tables, one per rule of the definition; a table just past the capped grid; caps,
NOSPACE and guard bytes; malformed input in both forms; the device forms on a user stream interleaved with the other families on one handle; the
empty graph and an index that is not canonical."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from bloomfiltertrie_amd import BFT, _lib, synth as S

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_bubbles_host as B  # noqa: E402
import test_cgraph_host as G  # noqa: E402
import test_gpu_unitigs as U  # noqa: E402  (the helpers: ingest, rows, guarded buffers)
import test_unitigs_host as H  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = U.GUARD
NONE = B.NONE


def _check_index(t, g, b):
    """the graph, its bubbles (records, order, the four counts) and its segment table, exact against the models"""
    graph = t.unitig_graph(g.t)
    assert G.check(g, graph) == []
    problems = B.check(b.reported(), t.unitig_bubbles(graph))
    assert problems == [], (t.k, g.t, problems[:5])
    seg_of, pos = t.unitig_segment_of(graph)
    want = B.segment_of(g.k, *g.arrays()[::4], len(g.m.rows))
    assert (seg_of.tolist(), pos.tolist()) == want, (t.k, g.t)
    return graph


@pytest.mark.parametrize("k", H.KS)
def test_bubbles_match_the_model_at_every_key_width(k):
    genomes, _ = H.width_case(k)
    t = U._ingest(genomes, k)
    for thr in G.THRESHOLDS:
        _check_index(t, G.graph("width_case", k, thr), B.bubbles_of("width_case", k, thr))
    # a limit on the branches: the model's answer at the substitution shape's length, and one below it
    graph = t.unitig_graph(0)
    for limit in (2 * k - 1, 2 * k - 2):
        want = B.Bubbles(k, *G.graph("width_case", k, 0).arrays()[:4], max_branch_chars=limit).reported()
        assert B.check(want, t.unitig_bubbles(graph, limit)) == []
    t.close()


@pytest.mark.parametrize("k", H.HAND_KS)
def test_hand_made_situations(k):
    genomes, _ = H.hand_case(k)
    t = U._ingest(genomes, k)
    for thr in (0, 1, 2):
        _check_index(t, G.graph("hand_case", k, thr), B.bubbles_of("hand_case", k, thr))
    t.close()


@pytest.mark.parametrize("k", B.PLANTED_KS)
def test_planted_variants_end_to_end(k):
    genomes, _, sites = B.planted_case(k)
    g = B.planted_graph(k)
    b = B.Bubbles(k, *g.arrays()[:4])
    t = U._ingest(genomes, k)
    graph = _check_index(t, g, b)
    recs, counts = t.unitig_bubbles(graph)
    assert counts.tolist()[:3] == [4, 9, 3]
    rows, _ = t.unitig_colors(graph[4], graph[0], "and")
    sets = [{x for x in range(8 * rows.shape[1]) if r[x >> 3] >> (x & 7) & 1} for r in rows]
    got = sorted(sorted(sorted(sets[x >> 1]) for x in rec[2:] if x != NONE) for rec in recs.tolist())
    assert got == sorted(groups for _, groups in sites)  # per bubble: the AND colour sets of its branches are the construction's allele groups
    inter = g.colour_sets("and")
    truth = b.reported()[0]
    for colors in (False, True):
        out = t.bubbles(colors=colors)
        assert [(x["source"], x["sink"], x["branches"]) for x in out] == [(r[0], r[1], [y for y in r[2:] if y != NONE]) for r in truth]
        assert [x["alleles"] for x in out] == [[g.spelled(y) for y in r[2:] if y != NONE] for r in truth]
        assert ("genomes" in out[0]) == colors
        if colors:
            assert [x["genomes"] for x in out] == [[sorted(inter[y >> 1]) for y in r[2:] if y != NONE] for r in truth]
    assert sorted(len(x["branches"]) for x in t.bubbles(max_branch_chars=2 * k - 1)) == [2, 2, 3]  # (the insertion's long branch is out)
    t.close()


@pytest.mark.parametrize("k", (27, 36))
def test_hand_made_link_tables(k):
    """arrays that are taken from no index, one per rule of the definition: the call reads the arrays alone (the handle's index is empty)"""
    t = BFT(k, device=0)
    for name, arrays, max_chars, n in B.hand_tables(k):
        got = t.unitig_bubbles(arrays, max_chars)
        want = B.Bubbles(k, *arrays, max_branch_chars=max_chars).reported()
        assert B.check(want, got) == [] and len(got[0]) == n, name
    t.close()


def test_grid_edge_and_ordering():
    """2S is just past the capped grid's lanes: the second grid-stride pass, a scan over several tiles, records in ascending source"""
    arrays, n = B.grid_table()
    k = 27
    assert len(arrays[2]) - 1 > B.GRID_LANES
    t = BFT(k, device=0)
    recs, counts = t.unitig_bubbles(arrays)
    assert counts.tolist() == [n, sum(2 + i % 3 for i in range(n)), 0, k]
    assert B.check(B.Bubbles(k, *arrays).reported(), (recs, counts)) == []
    t.close()


def test_caps_nospace_and_count_only():
    import torch
    k = 27
    genomes, _ = H.width_case(k)
    recs, counts = B.bubbles_of("width_case", k, 0).reported()
    n = len(recs)
    assert n >= 3
    t = U._ingest(genomes, k)
    seg_off, seqs, link_off, links, _ = t.unitig_graph(0)
    ns, nl = len(seg_off) - 1, len(links)
    lib = _lib.load()
    args = (seg_off.ctypes.data, seqs.ctypes.data, link_off.ctypes.data, links.ctypes.data, ns, nl, 0)
    cnt = (C.c_uint64 * 4)()
    assert lib.bft_gpu_unitig_bubbles(t._h, *args, None, 0, cnt) == 0 and list(cnt) == counts  # count only
    buf = np.full((n + 2) * 6, 7, dtype=np.uint32)
    for i in range(4):
        cnt[i] = 0
    assert lib.bft_gpu_unitig_bubbles(t._h, *args, buf.ctypes.data, n - 1, cnt) == -6  # BFT_GPU_E_NOSPACE: one short
    assert "too small" in lib.bft_gpu_last_error().decode() and list(cnt) == counts and (buf == 7).all()
    assert lib.bft_gpu_unitig_bubbles(t._h, *args, buf.ctypes.data, n, cnt) == 0
    assert buf[:6 * n].reshape(n, 6).tolist() == recs and (buf[6 * n:] == 7).all()
    # the device form: the records below cap, the counts always, nothing beyond
    dev = [torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a.view(np.int32) if a.dtype == np.uint32 else a).cuda() for a in (seg_off, seqs, link_off, links)]
    for cap in (n - 1, 1, 0):
        (rbuf, rptr), (cbuf, cptr) = U._guarded(torch, cap * 24), U._guarded(torch, 32)
        t.unitig_bubbles_dev(*[d.data_ptr() for d in dev], ns, nl, rptr, cap, cptr)
        torch.cuda.synchronize()
        assert cbuf.cpu().numpy()[GUARD:GUARD + 32].view(np.uint64).tolist() == counts
        assert rbuf.cpu().numpy()[GUARD:GUARD + cap * 24].view(np.uint32).reshape(cap, 6).tolist() == recs[:cap]
        assert U._guards_intact(rbuf, cap * 24) and U._guards_intact(cbuf, 32)
    (cbuf, cptr) = U._guarded(torch, 32)
    t.unitig_bubbles_dev(*[d.data_ptr() for d in dev], ns, nl, 0, 1 << 20, cptr)  # no record buffer: the cap does not count
    torch.cuda.synchronize()
    assert cbuf.cpu().numpy()[GUARD:GUARD + 32].view(np.uint64).tolist() == counts and U._guards_intact(cbuf, 32)
    t.close()


def _dev(torch, a):
    a = np.array(a)  # (a writable copy)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def test_malformed_input_in_both_forms():
    import torch
    k = 27
    t = BFT(k, device=0)
    lib = _lib.load()
    # two bubbles side by side (segments 0..3 and 4..7) and a bystander; the second is doctored
    edges = B.motif(0, 1, (2, 3)) + [(a + 8, b + 8) for a, b in B.motif(0, 1, (2, 3))]
    seg_off, seqs, link_off, links = B.table(k, 9, edges, 30)
    assert B.Bubbles(k, seg_off, seqs, link_off, links).reported()[1][0] == 2
    n2 = len(link_off) - 1

    def run_dev(so, sq, lo, lk, n_links):
        d = [_dev(torch, np.ascontiguousarray(a)) for a in (so, sq, lo, lk)]
        (rbuf, rptr), (cbuf, cptr) = U._guarded(torch, 2 * 24), U._guarded(torch, 32)
        t.unitig_bubbles_dev(*[x.data_ptr() for x in d], len(so) - 1, n_links, rptr, 2, cptr)
        torch.cuda.synchronize()
        assert U._guards_intact(rbuf, 48) and U._guards_intact(cbuf, 32)
        cnt = cbuf.cpu().numpy()[GUARD:GUARD + 32].view(np.uint64).tolist()
        return rbuf.cpu().numpy()[GUARD:GUARD + 48].view(np.uint32).reshape(2, 6)[:cnt[0]].tolist(), cnt

    def host(so, sq, lo, lk, n_links):
        cnt = (C.c_uint64 * 4)(7, 7, 7, 7)
        buf = np.full(12, 7, dtype=np.uint32)
        rc = lib.bft_gpu_unitig_bubbles(t._h, so.ctypes.data, sq.ctypes.data, lo.ctypes.data, lk.ctypes.data, len(so) - 1, n_links, 0, buf.ctypes.data, 2, cnt)
        return rc, list(cnt), buf

    first = [[0, 2, 4, 6, NONE, NONE]]
    # a target that is no oriented segment, in a branch list of the second bubble
    bad = links.copy()
    at = int(link_off[8])  # out(source of the second bubble)
    bad[at] = n2 + 5
    want = B.Bubbles(k, seg_off, seqs, link_off, bad).reported()
    assert want[0] == first and run_dev(seg_off, seqs, link_off, bad, len(bad)) == want
    rc, cnt, buf = host(seg_off, seqs, link_off, bad, len(bad))
    assert rc == -1 and "target" in lib.bft_gpu_last_error().decode() and cnt == [7] * 4 and (buf == 7).all()
    # ... and the same target as the one link of a branch (the sink) and in the sink's in-links
    for where in (int(link_off[12]), int(link_off[11])):
        bad = links.copy()
        bad[where] = NONE
        want = B.Bubbles(k, seg_off, seqs, link_off, bad).reported()
        assert want[0] == first and run_dev(seg_off, seqs, link_off, bad, len(bad)) == want
    # an over-long list: the source of the second bubble with five links
    e5 = edges + [(8, 16), (8, 17), (8, 1)]
    so5, sq5, lo5, lk5 = B.table(k, 9, e5, 30)
    assert int(lo5[9] - lo5[8]) == 5
    want = B.Bubbles(k, so5, sq5, lo5, lk5).reported()
    assert want[0] == first and run_dev(so5, sq5, lo5, lk5, len(lk5)) == want
    # offsets past n_links: the lists of the second bubble end behind the links the call may read
    short = int(link_off[8]) + 1
    want = B.Bubbles(k, seg_off, seqs, link_off, links[:short]).reported()
    assert want[0] == first and run_dev(seg_off, seqs, link_off, links, short) == want
    rc, cnt, buf = host(seg_off, seqs, link_off, links, short)
    assert rc == -1 and "last link offset" in lib.bft_gpu_last_error().decode() and cnt == [7] * 4 and (buf == 7).all()
    # link offsets that decrease, segment offsets that grow by less than k
    lo_bad = link_off.copy()
    lo_bad[9] = lo_bad[8] - np.uint64(1)
    want = B.Bubbles(k, seg_off, seqs, lo_bad, links).reported()
    assert run_dev(seg_off, seqs, lo_bad, links, len(links)) == want
    rc, cnt, buf = host(seg_off, seqs, lo_bad, links, len(links))
    assert rc == -1 and "must not decrease" in lib.bft_gpu_last_error().decode() and cnt == [7] * 4 and (buf == 7).all()
    so_bad = seg_off.copy()
    so_bad[1:] -= np.uint64(int(seg_off[1]) - (k - 1))  # (segment 0 would have k - 1 characters)
    rc, cnt, buf = host(so_bad, seqs, link_off, links, len(links))
    assert rc == -1 and "k characters" in lib.bft_gpu_last_error().decode() and cnt == [7] * 4 and (buf == 7).all()
    t.close()


def test_segment_table_caps_and_bad_members():
    import torch
    k = 27
    genomes, model = H.width_case(k)
    g = G.graph("width_case", k, 2)  # (rows below the threshold: entries that stay 0xFFFFFFFF)
    t = U._ingest(genomes, k)
    seg_off, _, _, _, members = t.unitig_graph(2)
    n, ns, nm = len(model.rows), len(seg_off) - 1, len(members)
    want_seg, want_pos = B.segment_of(k, seg_off, members, n)
    assert NONE in want_seg and ns > 2
    lib = _lib.load()
    so, po = np.full(n, 7, dtype=np.uint32), np.full(n, 7, dtype=np.uint32)
    assert lib.bft_gpu_unitig_segment_of(t._h, members.ctypes.data, nm, seg_off.ctypes.data, ns, so.ctypes.data, po.ctypes.data, n - 1) == -6  # BFT_GPU_E_NOSPACE
    assert (so == 7).all() and (po == 7).all()
    assert lib.bft_gpu_unitig_segment_of(t._h, members.ctypes.data, nm, seg_off.ctypes.data, ns, so.ctypes.data, None, n) == 0
    assert so.tolist() == want_seg and (po == 7).all()
    assert lib.bft_gpu_unitig_segment_of(t._h, members.ctypes.data, nm, seg_off.ctypes.data, ns, None, po.ctypes.data, n) == 0 and po.tolist() == want_pos
    # a member that is no vertex, offsets that are none: the host form refuses, the device form skips
    i = max(range(ns), key=lambda j: len(g.segs[j]))
    at = int(seg_off[i]) - i * (k - 1) + 1
    bad = members.copy()
    bad[at] = 2 * n
    so[:] = 7
    assert lib.bft_gpu_unitig_segment_of(t._h, bad.ctypes.data, nm, seg_off.ctypes.data, ns, so.ctypes.data, None, n) == -1 and (so == 7).all()
    assert "member" in lib.bft_gpu_last_error().decode()
    short = seg_off.copy()
    short[1:] -= np.uint64(2)
    assert lib.bft_gpu_unitig_segment_of(t._h, members.ctypes.data, nm, short.ctypes.data, ns, so.ctypes.data, None, n) == -1 and (so == 7).all()
    dm, do = _dev(torch, bad), _dev(torch, seg_off)
    row = int(members[at]) >> 1
    for cap in (n, n - 3, 0):
        (sbuf, sptr), (pbuf, pptr) = U._guarded(torch, cap * 4), U._guarded(torch, cap * 4)
        t.unitig_segment_of_dev(dm.data_ptr(), nm, do.data_ptr(), ns, sptr, pptr, cap)
        torch.cuda.synchronize()
        ws, wp = list(want_seg), list(want_pos)
        ws[row] = wp[row] = NONE  # (the bad member's own row is in no segment now)
        assert sbuf.cpu().numpy()[GUARD:GUARD + cap * 4].view(np.uint32).tolist() == ws[:cap]
        assert pbuf.cpu().numpy()[GUARD:GUARD + cap * 4].view(np.uint32).tolist() == wp[:cap]
        assert U._guards_intact(sbuf, cap * 4) and U._guards_intact(pbuf, cap * 4)
    t.close()


def test_dev_forms_on_a_user_stream_interleaved_with_other_families():
    """the scratch is the bubbles' own: between the graph, unitigs, a colour query and a prefix query on one handle, every answer is unchanged"""
    import torch
    k = 36
    genomes, model = H.width_case(k)
    g = G.graph("width_case", k, 0)
    want = B.bubbles_of("width_case", k, 0).reported()
    nb = want[1][0]
    t = U._ingest(genomes, k)
    n = len(model.rows)
    ns, nc, _, _, nl, _ = g.counts()
    nm = nc - ns * (k - 1)
    asc = model.rows[::5]
    before = U._answers(t, asc, k)
    ug_before = t.unitigs(0)
    q, _ = S.ascii_to_packed(asc, k)
    nq = len(q)
    bits_h, off_h, ids_h = t.query_colors(q)
    pref = q[:64].copy()
    po, _, _, _ = t.query_prefixes(pref, np.full(64, 20, dtype=np.uint8))
    want_seg, want_pos = B.segment_of(k, *g.arrays()[::4], n)
    P, N = len(model.unitigs(0)), sum(map(len, model.unitigs(0)))
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        dq = torch.from_numpy(q.reshape(-1).copy()).cuda()
        dbits = torch.zeros((nq + 63) // 64, dtype=torch.int64, device="cuda")
        doffc = torch.zeros(nq + 1, dtype=torch.int64, device="cuda")
        dids = torch.zeros(len(ids_h) + 1, dtype=torch.int32, device="cuda")
        dp = torch.from_numpy(pref.reshape(-1).copy()).cuda()
        dl = torch.full((64,), 20, dtype=torch.uint8, device="cuda")
        dpo = torch.zeros(65, dtype=torch.int64, device="cuda")
        dso = torch.full((ns + 1,), 7, dtype=torch.int64, device="cuda")
        dsq = torch.full((nc,), 7, dtype=torch.uint8, device="cuda")
        dlo = torch.full((2 * ns + 1,), 7, dtype=torch.int64, device="cuda")
        dlk = torch.full((nl,), 7, dtype=torch.int32, device="cuda")
        dmem = torch.full((nm,), 7, dtype=torch.int32, device="cuda")
        cnt, cnt2 = torch.full((6,), 7, dtype=torch.int64, device="cuda"), torch.full((6,), 7, dtype=torch.int64, device="cuda")
        drec, drec2 = torch.full((nb, 6), 7, dtype=torch.int32, device="cuda"), torch.full((nb, 6), 7, dtype=torch.int32, device="cuda")
        bcnt, bcnt2 = torch.full((4,), 7, dtype=torch.int64, device="cuda"), torch.full((4,), 7, dtype=torch.int64, device="cuda")
        dsegof = torch.full((n,), 7, dtype=torch.int32, device="cuda")
        dpos = torch.full((n,), 7, dtype=torch.int32, device="cuda")
        uoff = torch.full((P + 1,), 7, dtype=torch.int64, device="cuda")
        useq = torch.full((N,), 7, dtype=torch.uint8, device="cuda")
        ucnt = torch.zeros(4, dtype=torch.int64, device="cuda")
        graph_args = (dso.data_ptr(), dsq.data_ptr(), dlo.data_ptr(), dlk.data_ptr())
        t.unitig_graph_dev(*graph_args, dmem.data_ptr(), ns, nc, nl, nm, cnt.data_ptr(), stream=s.cuda_stream)
        t.unitig_bubbles_dev(*graph_args, ns, nl, drec.data_ptr(), nb, bcnt.data_ptr(), stream=s.cuda_stream)
        t.query_colors_dev(dq.data_ptr(), nq, dbits.data_ptr(), doffc.data_ptr(), dids.data_ptr(), len(ids_h) + 1, stream=s.cuda_stream)
        t.unitig_segment_of_dev(dmem.data_ptr(), nm, dso.data_ptr(), ns, dsegof.data_ptr(), dpos.data_ptr(), n, stream=s.cuda_stream)
        t.unitigs_dev(uoff.data_ptr(), useq.data_ptr(), P, N, ucnt.data_ptr(), stream=s.cuda_stream)
        t.unitig_graph_dev(0, 0, 0, 0, 0, 0, 0, 0, 0, cnt2.data_ptr(), min_shared=2, stream=s.cuda_stream)  # (the graph's scratch is rewritten ...)
        t.unitig_bubbles_dev(*graph_args, ns, nl, drec2.data_ptr(), nb, bcnt2.data_ptr(), stream=s.cuda_stream)  # (... the bubbles read the caller's arrays)
        t.query_prefixes_dev(dp.data_ptr(), dl.data_ptr(), 64, dpo.data_ptr(), 0, 0, 0, 0, 0, stream=s.cuda_stream)
    s.synchronize()
    got = (dso.cpu().numpy().astype(np.uint64), dsq.cpu().numpy(), dlo.cpu().numpy().astype(np.uint64), dlk.cpu().numpy().astype(np.uint32),
           dmem.cpu().numpy().astype(np.uint32))
    assert G.check(g, got) == [] and cnt.cpu().tolist() == g.counts() and cnt2.cpu().tolist() == G.graph("width_case", k, 2).counts()
    for rec, bc in ((drec, bcnt), (drec2, bcnt2)):
        assert B.check(want, (rec.cpu().numpy().view(np.uint32), bc.cpu().tolist())) == []
    assert dsegof.cpu().numpy().view(np.uint32).tolist() == want_seg and dpos.cpu().numpy().view(np.uint32).tolist() == want_pos
    assert H.check(model, 0, H.split(uoff.cpu().numpy(), useq.cpu().numpy())) == [] and ucnt.cpu().tolist()[:2] == [P, N]
    assert (dbits.cpu().numpy().view(np.uint8)[:len(bits_h)] == bits_h).all()
    assert (doffc.cpu().numpy().astype(np.uint64) == off_h).all()
    assert (dids.cpu().numpy()[:len(ids_h)].astype(np.uint32) == ids_h).all()
    assert (dpo.cpu().numpy().astype(np.uint64) == po).all()
    # all earlier answers are unchanged
    after = t.unitigs(0)
    assert U._answers(t, asc, k) == before and U._rows(t) == model.rows
    assert after[0].tobytes() == ug_before[0].tobytes() and after[1].tobytes() == ug_before[1].tobytes()
    t.close()


def test_empty_graph_noncanonical_index_stages_and_kernel_time():
    t = BFT(27, device=0)
    graph = t.unitig_graph()
    recs, counts = t.unitig_bubbles(graph)
    assert recs.shape == (0, 6) and counts.tolist() == [0, 0, 0, 0]
    seg_of, pos = t.unitig_segment_of(graph)
    assert len(seg_of) == len(pos) == 0 and t.bubbles(colors=True) == []
    t.close()
    # an index that is not canonical: the graph is refused, the bubble call on empty arrays gives four zeros
    t, model = U._noncanonical(27)
    assert model.noncanonical > 0
    with pytest.raises(_lib.BFTError):
        t.unitig_graph()
    with pytest.raises(_lib.BFTError):
        t.bubbles()
    empty = (np.zeros(1, dtype=np.uint64), np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.uint64), np.zeros(0, dtype=np.uint32))
    recs, counts = t.unitig_bubbles(empty)
    assert recs.shape == (0, 6) and counts.tolist() == [0, 0, 0, 0]
    t.close()
    # an index whose threshold leaves no segment
    genomes, _ = H.width_case(27)
    t2 = U._ingest(genomes, 27)
    graph = t2.unitig_graph(H.N_GENOMES + 1)
    assert t2.unitig_bubbles(graph)[1].tolist() == [0, 0, 0, 0]
    seg_of, pos = t2.unitig_segment_of(graph)
    assert (seg_of == NONE).all() and (pos == NONE).all() and len(seg_of) == t2.info()["kmers"]
    # kernel time and stages
    graph = t2.unitig_graph()
    t2.kernel_time(reset=True)
    t2.unitig_bubbles(graph)
    ms, launches = t2.kernel_time(reset=True)
    assert launches >= 3 and ms > 0
    t2.set_option("build_stages", 1)
    t2.unitig_bubbles(graph)
    names = [name for name, _, _ in t2.build_stages()]
    assert len(names) >= 3 and all(name.startswith("bubbles:") for name in names if name != "start"), names
    t2.unitig_segment_of(graph)
    names = [name for name, _, _ in t2.build_stages()]
    assert len(names) >= 2 and all(name.startswith("bubbles:") for name in names if name != "start"), names
    t2.close()
