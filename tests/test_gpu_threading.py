"""Sequence threading through the compacted coloured graph on the GPU (bft_gpu_thread_sequences / _dev, BFT.thread_sequences, BFT.thread): exact against
the model of tests/test_threading_host.py, which is written from the definition alone and proves its consequences on the same cases on the CPU.  Real
indexes at every key width and threshold, the hand-made situations, the planted variants end to end; a batch just past the capped grid; batch shapes
that put sequence boundaries around every multiple of 64 and 256 positions; caps, NOSPACE and guard bytes; malformed graph arrays in both forms; an
index that is not canonical; the empty index; the device form on a user stream interleaved with the other families on one handle."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

from bloomfiltertrie_amd import BFT, _lib, synth as S

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_bubbles_host as B  # noqa: E402
import test_cgraph_host as G  # noqa: E402
import test_gpu_unitigs as U  # noqa: E402  (the helpers: ingest, guarded buffers)
import test_threading_host as T  # noqa: E402
import test_unitigs_host as H  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = U.GUARD
NONE = T.NONE


@functools.lru_cache(maxsize=None)
def _want(case, k, t, which):
    """the model's result (computed once) for the sequence set `which` over the graph of a case"""
    g = G.graph(case, k, t) if case != "grid_case" else G.graph(case, t)
    seqs = {"width": T.width_sequences, "hand": lambda kk: T.hand_sequences(kk)[0], "batch": T.batch_shapes}[which](k) if which != "grid" else T.grid_sequences()
    return T.threading_of(g).run(seqs)


def _check(t, thr, seqs, want):
    graph = t.unitig_graph(thr)
    got = t.thread_sequences(seqs, graph)
    problems = T.check(want, got)
    assert problems == [], (t.k, thr, problems[:5])
    return graph, got


@pytest.mark.parametrize("k", H.KS)
def test_walks_match_the_model_at_every_key_width(k):
    genomes, _ = H.width_case(k)
    t = U._ingest(genomes, k)
    for thr in G.THRESHOLDS:
        _check(t, thr, T.width_sequences(k), _want("width_case", k, thr, "width"))
    t.close()


@pytest.mark.parametrize("k", H.HAND_KS)
def test_hand_made_situations(k):
    genomes, _ = H.hand_case(k)
    t = U._ingest(genomes, k)
    for thr in (0, 1, 2):
        _check(t, thr, T.hand_sequences(k)[0], _want("hand_case", k, thr, "hand"))
    t.close()


@pytest.mark.parametrize("k", B.PLANTED_KS)
def test_planted_variants_end_to_end(k):
    genomes, _, _ = B.planted_case(k)
    g = B.planted_graph(k)
    seqs = T.planted_sequences(k)
    want = T.threading_of(g).run(seqs)
    t = U._ingest(genomes, k)
    _check(t, 0, seqs, want)
    walks, walk_off, steps, _ = want
    dicts = [{"sequence": s, "start": p0, "end": p0 + nw + k - 1, "path": steps[walk_off[w]:walk_off[w + 1]], "path_start": q0, "path_end": q0 + nw + k - 1}
             for w, (s, p0, nw, q0) in enumerate(walks)]
    assert t.thread(seqs) == dicts
    # every genome, one walk end to end, through exactly the branch of each bubble whose AND row holds it
    graph = t.unitig_graph(0)
    recs, _ = t.unitig_bubbles(graph)
    rows, _ = t.unitig_colors(graph[4], graph[0], "and")
    out = t.thread([q for seqs_ in genomes for q in seqs_])
    assert [x["sequence"] for x in out] == [0, 1, 2, 3] and len(recs) == 4
    for gid, x in enumerate(out):
        segs = {y >> 1 for y in x["path"]}
        for rec in recs.tolist():
            taken = [y >> 1 for y in rec[2:] if y != NONE and y >> 1 in segs]
            assert len(taken) == 1 and rows[taken[0]][gid >> 3] >> (gid & 7) & 1
    t.close()


def test_grid_edge_and_ordering():
    """just over 524 288 positions in one call: the second grid-stride pass, a scan over many tiles, walks in ascending order"""
    genomes, _ = H.grid_case()
    seqs = T.grid_sequences()
    want = _want("grid_case", H.GRID_K, 0, "grid")
    assert want[3][2] > B.GRID_LANES
    t = U._ingest(genomes, H.GRID_K)
    _check(t, 0, seqs, want)
    t.close()


def test_batch_shapes():
    k = 27
    genomes, _ = H.width_case(k)
    t = U._ingest(genomes, k)
    graph, got = _check(t, 0, T.batch_shapes(k), _want("width_case", k, 0, "batch"))
    assert got[3][3] == 13
    # no sequence at all, and sequences without a position
    for seqs in ([], [""], ["", "ACGT", ""]):
        walks, walk_off, steps, counts = t.thread_sequences(seqs, graph)
        assert walks.shape == (0, 4) and walk_off.tolist() == [0] and len(steps) == 0 and counts.tolist() == [0] * 8
    t.close()


def _dev(torch, a):
    a = np.array(a)  # (a writable copy)
    if a.size == 0:
        a = np.zeros(1, dtype=a.dtype)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


class _DevInput:
    """device copies of a batch, a graph's arrays and a segment table"""

    def __init__(self, torch, seqs, seg_off, link_off, links, seg_of, pos, n_links=None):
        enc = [q.encode() for q in seqs]
        off = np.zeros(len(enc) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(e) for e in enc])
        self.n_seqs, self.n_chars = len(enc), int(off[-1])
        self.keep = [_dev(torch, np.frombuffer(b"".join(enc), dtype=np.uint8)), _dev(torch, off), _dev(torch, np.asarray(seg_of, dtype=np.uint32)),
                     _dev(torch, np.asarray(pos, dtype=np.uint32)), _dev(torch, np.asarray(seg_off, dtype=np.uint64)), _dev(torch, np.asarray(link_off, dtype=np.uint64)),
                     _dev(torch, np.asarray(links, dtype=np.uint32))]
        self.n_rows, self.ns = len(seg_of), len(seg_off) - 1
        self.nl = len(links) if n_links is None else n_links

    def args(self):
        d = [x.data_ptr() for x in self.keep]
        return (d[0], d[1], self.n_seqs, self.n_chars, d[2], d[3], self.n_rows, d[4], self.ns, d[5], d[6], self.nl)


def _run_dev(torch, t, inp, walks_cap, steps_cap, stream=None, outputs=(True, True, True)):
    """the device form into guarded buffers -> (walks below the cap, walk_off entries, steps below the cap, counts), guards checked"""
    sizes = (walks_cap * 32, (walks_cap + 1) * 8, steps_cap * 4)
    bufs = [U._guarded(torch, n) if on else (None, 0) for n, on in zip(sizes, outputs)]
    cbuf, cptr = U._guarded(torch, 64)
    t.thread_sequences_dev(*inp.args(), bufs[0][1], bufs[1][1], walks_cap, bufs[2][1], steps_cap, cptr, stream=stream)

    def collect():
        counts = cbuf.cpu().numpy()[GUARD:GUARD + 64].view(np.uint64).tolist()
        assert U._guards_intact(cbuf, 64)
        raw = []
        for (buf, _), n in zip(bufs, sizes):
            if buf is None:
                raw.append(None)
                continue
            assert U._guards_intact(buf, n)
            raw.append(buf.cpu().numpy()[GUARD:GUARD + n])
        nw, nst = min(counts[0], walks_cap), min(counts[1], steps_cap)
        walks = raw[0].view(np.uint64).reshape(-1, 4)[:nw].tolist() if raw[0] is not None else None
        walk_off = raw[1].view(np.uint64)[:nw + 1].tolist() if raw[1] is not None else None
        steps = raw[2].view(np.uint32)[:nst].tolist() if raw[2] is not None else None
        untouched = all((r[used:] == 7).all() for r, used in zip(raw, (nw * 32, (nw + 1) * 8, nst * 4)) if r is not None)
        return walks, walk_off, steps, counts, untouched
    return collect


def test_caps_nospace_and_count_only():
    import torch
    k = 27
    genomes, _ = H.width_case(k)
    seqs = T.width_sequences(k)
    want = _want("width_case", k, 2, "width")
    walks, walk_off, steps, counts = want
    nw, nst = len(walks), len(steps)
    assert nw >= 3 and nst > nw
    t = U._ingest(genomes, k)
    graph = t.unitig_graph(2)
    seg_of, pos = t.unitig_segment_of(graph)
    seg_off, _, link_off, links, _ = graph
    enc = [q.encode() for q in seqs]
    off = np.zeros(len(enc) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(e) for e in enc])
    blob = b"".join(enc)
    lib = _lib.load()
    args = (t._h, blob, off.ctypes.data, len(enc), seg_of.ctypes.data, pos.ctypes.data, len(seg_of), seg_off.ctypes.data, len(seg_off) - 1, link_off.ctypes.data,
            links.ctypes.data, len(links))
    cnt = (C.c_uint64 * 8)()
    assert lib.bft_gpu_thread_sequences(*args, None, None, 0, None, 0, cnt) == 0 and list(cnt) == counts  # count only
    wb, ob, sb = np.full((nw + 2) * 4, 7, dtype=np.uint64), np.full(nw + 3, 7, dtype=np.uint64), np.full(nst + 2, 7, dtype=np.uint32)
    for wcap, scap in ((nw - 1, nst), (nw, nst - 1)):  # each cap one short
        for i in range(8):
            cnt[i] = 0
        assert lib.bft_gpu_thread_sequences(*args, wb.ctypes.data, ob.ctypes.data, wcap, sb.ctypes.data, scap, cnt) == -6  # BFT_GPU_E_NOSPACE
        assert "too small" in lib.bft_gpu_last_error().decode() and list(cnt) == counts and (wb == 7).all() and (ob == 7).all() and (sb == 7).all()
    assert lib.bft_gpu_thread_sequences(*args, None, ob.ctypes.data, nw - 1, None, 0, cnt) == -6 and (ob == 7).all()  # walk_off alone needs the walks' cap
    assert lib.bft_gpu_thread_sequences(*args, None, None, 0, sb.ctypes.data, nst, cnt) == 0  # the steps alone
    assert sb[:nst].tolist() == steps and (sb[nst:] == 7).all() and (wb == 7).all() and (ob == 7).all()
    assert lib.bft_gpu_thread_sequences(*args, wb.ctypes.data, ob.ctypes.data, nw, sb.ctypes.data, nst, cnt) == 0
    assert wb[:4 * nw].reshape(nw, 4).tolist() == walks and (wb[4 * nw:] == 7).all() and ob[:nw + 1].tolist() == walk_off and (ob[nw + 1:] == 7).all()
    # the device form: what lies below the caps, the counts always, nothing beyond
    inp = _DevInput(torch, seqs, seg_off, link_off, links, seg_of, pos)
    for wcap, scap in ((nw - 1, nst - 1), (1, 1), (0, 0), (nw, nst), (nw + 5, nst + 5)):
        collect = _run_dev(torch, t, inp, wcap, scap)
        torch.cuda.synchronize()
        gw, go, gs, gc, untouched = collect()
        assert gc == counts and untouched
        assert gw == walks[:wcap] and gs == steps[:scap] and go == walk_off[:min(wcap, nw) + 1], (wcap, scap)
    for outputs in ((False, False, False), (True, False, False), (False, True, False), (False, False, True)):  # buffers that are not given: their caps do not count
        collect = _run_dev(torch, t, inp, nw, nst, outputs=outputs)
        torch.cuda.synchronize()
        gw, go, gs, gc, untouched = collect()
        assert gc == counts and untouched and (gw is None or gw == walks) and (go is None or go == walk_off) and (gs is None or gs == steps)
    t.close()


def test_malformed_graph_arrays_in_both_forms():
    """bad input against stated outcomes: the host form refuses it with nothing written, the device form applies the definition's rules"""
    import torch
    k = 27
    genomes, _ = H.width_case(k)
    g = G.graph("width_case", k, 0)
    seqs = T.width_sequences(k)
    t = U._ingest(genomes, k)
    graph = t.unitig_graph(0)
    seg_of, pos = t.unitig_segment_of(graph)
    assert G.check(g, graph) == []
    for name, (so, lo, lk, nl, sg, ps) in T.malformed(graph, seg_of.tolist(), pos.tolist(), k):
        want = T.Threading(k, g.m.row, so, lo, lk, sg, ps, n_links=nl).run(seqs)
        inp = _DevInput(torch, seqs, so, lo, lk, sg, ps, n_links=nl)
        collect = _run_dev(torch, t, inp, want[3][0], want[3][1])
        torch.cuda.synchronize()
        gw, go, gs, gc, untouched = collect()
        assert T.check(want, (gw, go, gs, gc)) == [] and untouched, name
    # the host form
    lib = _lib.load()
    seg_off, _, link_off, links, _ = graph
    enc = [q.encode() for q in seqs]
    off = np.zeros(len(enc) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(e) for e in enc])
    blob = b"".join(enc)
    ns, n2 = len(seg_off) - 1, len(link_off) - 1

    def host(so, lo, lk, nl, n_rows=len(seg_of)):
        cnt = (C.c_uint64 * 8)(*([7] * 8))
        wb, ob, sb = np.full(64, 7, dtype=np.uint64), np.full(64, 7, dtype=np.uint64), np.full(64, 7, dtype=np.uint32)
        rc = lib.bft_gpu_thread_sequences(t._h, blob, off.ctypes.data, len(enc), seg_of.ctypes.data, pos.ctypes.data, n_rows, so.ctypes.data, ns, lo.ctypes.data, lk.ctypes.data,
                                          nl, wb.ctypes.data, ob.ctypes.data, 16, sb.ctypes.data, 64, cnt)
        return rc, lib.bft_gpu_last_error().decode(), list(cnt) == [7] * 8 and (wb == 7).all() and (ob == 7).all() and (sb == 7).all()

    lo_bad = link_off.copy()
    lo_bad[9] = lo_bad[8] - np.uint64(1) if lo_bad[8] else lo_bad[10] + np.uint64(1)
    rc, msg, clean = host(seg_off, lo_bad, links, len(links))
    assert rc == -1 and "must not decrease" in msg and clean
    rc, msg, clean = host(seg_off, link_off, links, len(links) - 1)
    assert rc == -1 and "last link offset" in msg and clean
    bad = links.copy()
    bad[len(bad) // 2] = n2
    rc, msg, clean = host(seg_off, link_off, bad, len(links))
    assert rc == -1 and "target" in msg and clean
    so_bad = seg_off.copy()
    so_bad[1:] -= np.uint64(int(seg_off[1]) - (k - 1))  # (segment 0 would have k - 1 characters)
    rc, msg, clean = host(so_bad, link_off, links, len(links))
    assert rc == -1 and "k characters" in msg and clean
    rc, msg, clean = host(seg_off, link_off, links, len(links), n_rows=len(seg_of) - 1)
    assert rc == -1 and "n_rows" in msg and clean
    t.close()


def test_an_index_that_is_not_canonical():
    import torch
    k = 27
    t, model = U._noncanonical(k)
    assert model.noncanonical > 0
    n = len(model.rows)
    seqs = ["".join(model.rows[:3]), model.rows[5], "ACGTN" * 10]
    none = np.full(n, NONE, dtype=np.uint32)
    empty = (np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.uint64), np.zeros(0, dtype=np.uint32))
    want = T.Threading(k, model.row, empty[0], empty[1], empty[2], none, none, model.noncanonical).run(seqs)
    assert want[3][7] == model.noncanonical and want[3][:2] == [0, 0] and want[3][5] > 0
    lib = _lib.load()
    blob = "".join(seqs).encode()
    off = np.cumsum([0] + [len(q) for q in seqs]).astype(np.uint64)
    cnt = (C.c_uint64 * 8)()
    wb = np.full(16, 7, dtype=np.uint64)
    rc = lib.bft_gpu_thread_sequences(t._h, blob, off.ctypes.data, len(seqs), none.ctypes.data, none.ctypes.data, n, None, 0, None, None, 0, wb.ctypes.data, wb.ctypes.data, 1, None,
                                      0, cnt)
    assert rc == -4 and "not canonical" in lib.bft_gpu_last_error().decode() and list(cnt) == want[3] and (wb == 7).all()  # BFT_GPU_E_STATE, counts filled
    with pytest.raises(_lib.BFTError):
        t.thread(seqs)
    # the device form: the counts say it
    inp = _DevInput(torch, seqs, empty[0], empty[1], empty[2], none, none)
    collect = _run_dev(torch, t, inp, 4, 4)
    torch.cuda.synchronize()
    assert collect()[3] == want[3]
    t.close()


def test_empty_index_stages_and_kernel_time():
    t = BFT(27, device=0)
    graph = t.unitig_graph()
    walks, walk_off, steps, counts = t.thread_sequences(["ACGT" * 20, "", "ACGTN" * 10], graph)
    assert walks.shape == (0, 4) and walk_off.tolist() == [0] and len(steps) == 0
    assert counts.tolist() == [0, 0, 54 + 24, 24, 54, 0, 0, 0]  # every valid window is absent
    assert t.thread(["ACGT" * 20]) == []
    t.close()
    k = 27
    genomes, _ = H.width_case(k)
    t = U._ingest(genomes, k)
    seqs = T.width_sequences(k)
    graph = t.unitig_graph()
    seg_of = t.unitig_segment_of(graph)
    t.kernel_time(reset=True)
    t.thread_sequences(seqs, graph, seg_of)
    ms, launches = t.kernel_time(reset=True)
    assert launches >= 8 and ms > 0
    t.set_option("build_stages", 1)
    t.thread_sequences(seqs, graph, seg_of)
    names = [name for name, _, _ in t.build_stages()]
    assert len(names) >= 8 and all(name.startswith("threading:") for name in names if name != "start"), names
    t.close()


def test_dev_form_on_a_user_stream_interleaved_with_other_families():
    """the scratch is the threading's own: between the graph, the bubbles, a presence query and an ingest on one handle, every answer is the one of
    the call run alone"""
    import torch
    k = 36
    genomes, model = H.width_case(k)
    seqs = T.width_sequences(k)
    want = _want("width_case", k, 0, "width")
    nw, nst = want[3][0], want[3][1]
    t = U._ingest(genomes, k)
    graph = t.unitig_graph(0)
    seg_off, gseqs, link_off, links, _ = graph
    seg_of, pos = t.unitig_segment_of(graph)
    alone = t.thread_sequences(seqs, graph, (seg_of, pos))
    assert T.check(want, alone) == []
    bub_want = t.unitig_bubbles(graph)
    q, _ = S.ascii_to_packed(model.rows[::5], k)
    bits_h = t.query_presence(q)
    nq, ns, nl, nb = len(q), len(seg_off) - 1, len(links), len(bub_want[0])
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        inp = _DevInput(torch, seqs, seg_off, link_off, links, seg_of, pos)
        dgs = _dev(torch, gseqs)
        dq = torch.from_numpy(q.reshape(-1).copy()).cuda()
        dbits = torch.zeros((nq + 63) // 64, dtype=torch.int64, device="cuda")
        gcnt = torch.full((6,), 7, dtype=torch.int64, device="cuda")
        drec = torch.full((max(nb, 1), 6), 7, dtype=torch.int32, device="cuda")
        bcnt = torch.full((4,), 7, dtype=torch.int64, device="cuda")
        g0 = genomes[0][0].encode()
        dg0 = torch.from_numpy(np.frombuffer(g0, dtype=np.uint8).copy()).cuda()
        dg0off = torch.tensor([0, len(g0)], dtype=torch.int64, device="cuda")
        runs = [_run_dev(torch, t, inp, nw, nst, stream=s.cuda_stream)]
        t.unitig_graph_dev(0, 0, 0, 0, 0, 0, 0, 0, 0, gcnt.data_ptr(), min_shared=2, stream=s.cuda_stream)  # (the graph's scratch is rewritten ...)
        runs.append(_run_dev(torch, t, inp, nw, nst, stream=s.cuda_stream))  # (... the threading reads the caller's arrays and its own scratch)
        d = inp.keep
        t.unitig_bubbles_dev(d[4].data_ptr(), dgs.data_ptr(), d[5].data_ptr(), d[6].data_ptr(), ns, nl, drec.data_ptr(), nb, bcnt.data_ptr(), stream=s.cuda_stream)
        t.query_presence_dev(dq.data_ptr(), nq, dbits.data_ptr(), stream=s.cuda_stream)
        runs.append(_run_dev(torch, t, inp, nw, nst, stream=s.cuda_stream))
        # genome 0 once more into genome 0: pending insertions that the next call builds first, and the same index behind them
        t.insert_sequences_dev(dg0.data_ptr(), dg0off.data_ptr(), 1, len(g0), 0, canonical=True, stream=s.cuda_stream)
        runs.append(_run_dev(torch, t, inp, nw, nst, stream=s.cuda_stream))
    s.synchronize()
    for collect in runs:
        gw, go, gs, gc, untouched = collect()
        assert untouched and (gw, go, gs, gc) == (alone[0].tolist(), alone[1].tolist(), alone[2].tolist(), alone[3].tolist())
    assert gcnt.cpu().tolist() == G.graph("width_case", k, 2).counts()
    assert bcnt.cpu().tolist() == bub_want[1].tolist() and drec.cpu().numpy().view(np.uint32)[:nb].tolist() == bub_want[0].tolist()
    assert (dbits.cpu().numpy().view(np.uint8)[:len(bits_h)] == bits_h).all()
    assert U._rows(t) == model.rows
    again = t.thread_sequences(seqs, graph, (seg_of, pos))
    assert all(a.tolist() == b.tolist() for a, b in zip(again, alone))
    t.close()
