"""The compacted coloured graph on the GPU (bft_gpu_unitig_graph / _dev, bft_gpu_unitig_colors / _dev, BFT.unitig_graph, BFT.unitig_colors): exact
against the model of tests/test_cgraph_host.py, which is written from the definition alone and proves its invariants on the same cases on the CPU.
Key widths W = 1..4 and both T-form tail layouts at thresholds 0, 1, 2, N, N + 1; the hand-made situations (cycle self links, hairpin, both palindrome
situations, two successors on two strands, lone k-mer, a chain of 3000 k-mers); one index just past the capped grid; the whole table as one chain
and as one cycle of 1 .. 1025 k-mers; index states that all give the same graph; an index that is not canonical; caps, NOSPACE and guard bytes;
the device form on a user stream interleaved with unitigs, simple paths, colour and prefix queries; the empty index; a colour row per segment under
AND, OR and SYMDIFF, on rows wider than 8 bytes, on a segment that the reduction splits, with a bad member."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

from bloomfiltertrie_amd import BFT, _lib, synth as S

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_cgraph_host as G  # noqa: E402
import test_gpu_unitigs as U  # noqa: E402  (the helpers: ingest, rows, guarded buffers)
import test_unitigs_host as H  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = U.GUARD


def _counts(t, thr):
    cnt = (C.c_uint64 * 6)()
    _lib.check(_lib.load().bft_gpu_unitig_graph(t._h, thr, None, None, None, None, None, 0, 0, 0, 0, cnt))
    return list(cnt)


def _check_all(t, case, args, thresholds):
    for thr in thresholds:
        g = G.graph(case, *args, thr)
        if thr == thresholds[0]:
            assert U._rows(t) == g.m.rows  # (the model's row order is the library's)
        problems = G.check(g, t.unitig_graph(thr))
        assert problems == [], (t.k, thr, problems[:5])
        assert _counts(t, thr) == g.counts()


@pytest.mark.parametrize("k", H.KS)
def test_graph_matches_the_model_at_every_key_width(k):
    genomes, _ = H.width_case(k)
    t = U._ingest(genomes, k)
    _check_all(t, "width_case", (k,), G.THRESHOLDS)
    seg_off, seqs, link_off, links, members = t.unitig_graph(H.N_GENOMES + 1)
    assert seg_off.tolist() == [0] and link_off.tolist() == [0] and len(seqs) == len(links) == len(members) == 0  # an empty graph
    # the segments that are no singles: byte for byte the unitigs
    g = G.graph("width_case", k, 0)
    strings = H.split(*t.unitig_graph(0)[:2])
    assert [s for s, one in zip(strings, g.is_single) if not one] == H.split(*t.unitigs(0))
    t.close()


@pytest.mark.parametrize("k", H.HAND_KS)
def test_hand_made_situations(k):
    genomes, _ = H.hand_case(k)
    t = U._ingest(genomes, k)
    _check_all(t, "hand_case", (k,), (0, 1, 2))
    t.close()


def test_grid_edge():
    """2n vertices exceed the capped grid's threads: every vertex kernel takes a second grid-stride pass"""
    genomes, _ = H.grid_case()
    t = U._ingest(genomes, H.GRID_K)
    _check_all(t, "grid_case", (), (0,))
    assert 2 * t.info()["kmers"] > 524288
    t.close()


@pytest.mark.parametrize("k", H.WHOLE_KS)
@pytest.mark.parametrize("kind", ("chain", "cycle"))
@pytest.mark.parametrize("n", H.WHOLE_NS)
def test_whole_table_is_one_segment(n, kind, k):
    genomes, _ = H.whole_case(n, kind, k)
    t = U._ingest(genomes, k)
    _check_all(t, "whole_case", (n, kind, k), (0,))
    seg_off, _, link_off, links, members = t.unitig_graph(0)
    assert seg_off.tolist() == [0, n + k - 1] and len(members) == n
    assert (link_off.tolist(), links.tolist()) == (([0, 0, 0], []) if kind == "chain" else ([0, 1, 2], [0, 1]))
    t.close()


@pytest.mark.parametrize("state", ["compact0", "compact1", "kmer_hash0", "pending", "merge", "file", "image"])
@pytest.mark.parametrize("k", (27, 63))
def test_index_states_give_the_same_graph(state, k, tmp_path):
    genomes, _ = H.width_case(k)
    keep = []
    if state in ("compact0", "compact1", "kmer_hash0"):
        opts = {"compact0": [("compact_table", 0)], "compact1": [("compact_table", 1)], "kmer_hash0": [("kmer_hash", 0)]}[state]
        t = U._ingest(genomes, k, options=opts, build_each=True)
    elif state == "pending":
        t = U._ingest(genomes[:3], k)
        t.unitig_graph(0)
        U._ingest(genomes[3:], k, t=t, first_gid=3)  # (pending: built by the next call)
    elif state == "merge":
        a, b = U._ingest(genomes[:2], k), U._ingest(genomes[2:], k)
        t = a.merge(b)
        keep = [a, b]
    elif state == "file":
        a = U._ingest(genomes, k)
        path = str(tmp_path / "i.bft")
        a.write_bft(path)
        t = BFT.load_bft(path)
        keep = [a]
    else:
        import torch
        a = U._ingest(genomes, k)
        a.build()
        nbytes = a.image_size()
        blob = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        a.image_pack(blob.data_ptr(), nbytes)
        torch.cuda.synchronize()
        t = BFT.from_image(blob.data_ptr(), nbytes)
        keep = [a]
    g = G.graph("width_case", k, 2)
    assert G.check(g, t.unitig_graph(2)) == []  # (first: a pending genome is built by this call)
    assert G.check(G.graph("width_case", k, 0), t.unitig_graph(0)) == []
    members, seg_off = t.unitig_graph(2)[4], t.unitig_graph(2)[0]
    assert _sets(t.unitig_colors(members, seg_off, "or")[0]) == g.colour_sets("or")
    t.close()
    for x in keep:
        x.close()


def _sets(rows):
    return [{g for g in range(8 * rows.shape[1]) if r[g >> 3] >> (g & 7) & 1} for r in rows]


@pytest.mark.parametrize("k", (27, 36))
def test_refusal_on_an_index_that_is_not_canonical(k):
    import torch
    t, model = U._noncanonical(k)
    assert model.noncanonical > 0
    lib = _lib.load()
    cnt = (C.c_uint64 * 6)()
    bufs = [np.full(1 << 14, 7, dtype=np.uint64), np.full(1 << 18, 7, dtype=np.uint8), np.full(1 << 15, 7, dtype=np.uint64), np.full(1 << 16, 7, dtype=np.uint32),
            np.full(1 << 16, 7, dtype=np.uint32)]
    assert lib.bft_gpu_unitig_graph(t._h, 0, None, None, None, None, None, 0, 0, 0, 0, cnt) == -4  # BFT_GPU_E_STATE
    assert cnt[3] == model.noncanonical
    cnt[3] = 0
    assert lib.bft_gpu_unitig_graph(t._h, 0, *[b.ctypes.data for b in bufs], (1 << 14) - 1, 1 << 18, 1 << 16, 1 << 16, cnt) == -4
    assert "not canonical" in lib.bft_gpu_last_error().decode() and cnt[3] == model.noncanonical and all((b == 7).all() for b in bufs)
    # the device form: the count of non-canonical rows, nothing beyond the caps
    sizes = (48, 11 * 8, 100, 21 * 8, 50 * 4, 60 * 4)
    guarded = [U._guarded(torch, nb) for nb in sizes]
    (cbuf, cptr), (_, optr), (_, sptr), (_, lptr), (_, kptr), (_, mptr) = guarded
    t.unitig_graph_dev(optr, sptr, lptr, kptr, mptr, 10, 100, 50, 60, cptr)
    torch.cuda.synchronize()
    assert cbuf.cpu().numpy()[GUARD:GUARD + 48].view(np.uint64)[3] == model.noncanonical
    assert all(U._guards_intact(buf, nb) for (buf, _), nb in zip(guarded, sizes))
    t.close()


def test_caps_and_nospace_host_form():
    k = 27
    genomes, _ = H.width_case(k)
    g = G.graph("width_case", k, 0)
    t = U._ingest(genomes, k)
    lib = _lib.load()
    cnt = (C.c_uint64 * 6)()
    ns, nc, _, _, nl, _ = want = g.counts()
    nm = nc - ns * (k - 1)
    assert _counts(t, 0) == want and min(ns, nc, nl, nm) > 1

    def fresh():
        return [np.full(ns + 1, 7, dtype=np.uint64), np.full(nc, 7, dtype=np.uint8), np.full(2 * ns + 1, 7, dtype=np.uint64), np.full(nl, 7, dtype=np.uint32),
                np.full(nm, 7, dtype=np.uint32)]

    for short in range(4):  # each of the four caps one below the need
        caps = [ns, nc, nl, nm]
        caps[short] -= 1
        bufs = fresh()
        for i in range(6):
            cnt[i] = 0
        assert lib.bft_gpu_unitig_graph(t._h, 0, *[b.ctypes.data for b in bufs], *caps, cnt) == -6  # BFT_GPU_E_NOSPACE
        assert list(cnt) == want and all((b == 7).all() for b in bufs), short
    # a cap does not count for an output that is NULL
    bufs = fresh()
    assert lib.bft_gpu_unitig_graph(t._h, 0, bufs[0].ctypes.data, None, bufs[2].ctypes.data, None, None, ns, 0, 0, 0, cnt) == 0
    assert bufs[0][0] == 0 and bufs[0][-1] == nc and bufs[2][0] == 0 and bufs[2][-1] == nl and (np.diff(bufs[2].astype(np.int64)) >= 0).all()
    assert lib.bft_gpu_unitig_graph(t._h, 0, None, None, None, bufs[3].ctypes.data, bufs[4].ctypes.data, 0, 0, nl, nm, cnt) == 0
    assert lib.bft_gpu_unitig_graph(t._h, 0, *[b.ctypes.data for b in bufs], ns, nc, nl, nm, cnt) == 0
    assert G.check(g, bufs) == []
    t.close()


def test_caps_in_the_device_form_leave_guard_bytes():
    import torch
    k = 36
    genomes, _ = H.width_case(k)
    g = G.graph("width_case", k, 0)
    t = U._ingest(genomes, k)
    ns, nc, _, _, nl, _ = want = g.counts()
    nm = nc - ns * (k - 1)
    seg_off, seqs, link_off, links, members = g.arrays()
    # caps one below the need: seg_off holds its entries j <= ns - 1, link_off its entries j <= 2 (ns - 1)
    sizes = (48, ns * 8, nc - 1, (2 * ns - 1) * 8, (nl - 1) * 4, (nm - 1) * 4)
    guarded = [U._guarded(torch, nb) for nb in sizes]
    ptrs = [p for _, p in guarded]
    t.unitig_graph_dev(ptrs[1], ptrs[2], ptrs[3], ptrs[4], ptrs[5], ns - 1, nc - 1, nl - 1, nm - 1, ptrs[0])
    torch.cuda.synchronize()
    body = [buf.cpu().numpy()[GUARD:GUARD + nb] for (buf, _), nb in zip(guarded, sizes)]
    assert body[0].view(np.uint64).tolist() == want
    assert (body[1].view(np.uint64) == seg_off[:ns]).all() and body[2].tobytes() == seqs.tobytes()[:nc - 1]
    assert (body[3].view(np.uint64) == link_off[:2 * ns - 1]).all() and (body[4].view(np.uint32) == links[:nl - 1]).all()
    assert (body[5].view(np.uint32) == members[:nm - 1]).all()
    assert all(U._guards_intact(buf, nb) for (buf, _), nb in zip(guarded, sizes))
    # caps of zero: seg_off[0] and link_off[0] alone
    sizes = (48, 8, 0, 8, 0, 0)
    guarded = [U._guarded(torch, nb) for nb in sizes]
    ptrs = [p for _, p in guarded]
    t.unitig_graph_dev(ptrs[1], ptrs[2], ptrs[3], ptrs[4], ptrs[5], 0, 0, 0, 0, ptrs[0])
    torch.cuda.synchronize()
    body = [buf.cpu().numpy()[GUARD:GUARD + nb] for (buf, _), nb in zip(guarded, sizes)]
    assert body[0].view(np.uint64).tolist() == want and body[1].view(np.uint64)[0] == 0 and body[3].view(np.uint64)[0] == 0
    assert all(U._guards_intact(buf, nb) for (buf, _), nb in zip(guarded, sizes))
    t.close()


def test_dev_form_on_a_user_stream_interleaved_with_other_queries():
    import torch
    k = 36
    genomes, model = H.width_case(k)
    g, g2 = G.graph("width_case", k, 0), G.graph("width_case", k, 2)
    t = U._ingest(genomes, k)
    want = model.unitigs(0)
    P, N = len(want), sum(map(len, want))
    ns, nc, _, _, nl, _ = g.counts()
    nm = nc - ns * (k - 1)
    asc = model.rows[::5]
    before = U._answers(t, asc, k)
    sp_before = t.simple_paths()
    ug_before = t.unitigs(0)
    q, _ = S.ascii_to_packed(asc, k)
    n = len(q)
    bits_h, off_h, ids_h = t.query_colors(q)
    pref = q[:64].copy()
    po, _, _, _ = t.query_prefixes(pref, np.full(64, 20, dtype=np.uint8))
    SP, SN = len(sp_before), sum(map(len, sp_before))
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        dq = torch.from_numpy(q.reshape(-1).copy()).cuda()
        dbits = torch.zeros((n + 63) // 64, dtype=torch.int64, device="cuda")
        doffc = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        dids = torch.zeros(len(ids_h) + 1, dtype=torch.int32, device="cuda")
        dp = torch.from_numpy(pref.reshape(-1).copy()).cuda()
        dl = torch.full((64,), 20, dtype=torch.uint8, device="cuda")
        dpo = torch.zeros(65, dtype=torch.int64, device="cuda")
        cnt = torch.full((6,), 7, dtype=torch.int64, device="cuda")
        t.unitig_graph_dev(0, 0, 0, 0, 0, 0, 0, 0, 0, cnt.data_ptr(), stream=s.cuda_stream)  # sizing
    s.synchronize()
    assert cnt.cpu().tolist() == g.counts()
    with torch.cuda.stream(s):
        dso = torch.full((ns + 1,), 7, dtype=torch.int64, device="cuda")
        dsq = torch.full((nc,), 7, dtype=torch.uint8, device="cuda")
        dlo = torch.full((2 * ns + 1,), 7, dtype=torch.int64, device="cuda")
        dlk = torch.full((nl,), 7, dtype=torch.int32, device="cuda")
        dmem = torch.full((nm,), 7, dtype=torch.int32, device="cuda")
        uoff = torch.full((P + 1,), 7, dtype=torch.int64, device="cuda")
        useq = torch.full((N,), 7, dtype=torch.uint8, device="cuda")
        ucnt = torch.zeros(4, dtype=torch.int64, device="cuda")
        spoff = torch.full((SP + 1,), 7, dtype=torch.int64, device="cuda")
        spseq = torch.full((SN,), 7, dtype=torch.uint8, device="cuda")
        spcnt = torch.zeros(3, dtype=torch.int64, device="cuda")
        drows = torch.zeros(ns, dtype=torch.uint8, device="cuda")
        dgc = torch.zeros(ns, dtype=torch.int32, device="cuda")
        t.query_colors_dev(dq.data_ptr(), n, dbits.data_ptr(), doffc.data_ptr(), dids.data_ptr(), len(ids_h) + 1, stream=s.cuda_stream)
        t.unitig_graph_dev(dso.data_ptr(), dsq.data_ptr(), dlo.data_ptr(), dlk.data_ptr(), dmem.data_ptr(), ns, nc, nl, nm, cnt.data_ptr(), stream=s.cuda_stream)
        t.unitigs_dev(uoff.data_ptr(), useq.data_ptr(), P, N, ucnt.data_ptr(), stream=s.cuda_stream)
        t.unitig_colors_dev(dmem.data_ptr(), nm, dso.data_ptr(), ns, "or", drows.data_ptr(), dgc.data_ptr(), stream=s.cuda_stream)
        t.simple_paths_dev(spoff.data_ptr(), spseq.data_ptr(), SP, SN, spcnt.data_ptr(), stream=s.cuda_stream)
        t.query_prefixes_dev(dp.data_ptr(), dl.data_ptr(), 64, dpo.data_ptr(), 0, 0, 0, 0, 0, stream=s.cuda_stream)
        cnt2 = torch.zeros(6, dtype=torch.int64, device="cuda")
        t.unitig_graph_dev(0, 0, 0, 0, 0, 0, 0, 0, 0, cnt2.data_ptr(), min_shared=2, stream=s.cuda_stream)
    s.synchronize()
    got = (dso.cpu().numpy().astype(np.uint64), dsq.cpu().numpy(), dlo.cpu().numpy().astype(np.uint64), dlk.cpu().numpy().astype(np.uint32),
           dmem.cpu().numpy().astype(np.uint32))
    assert G.check(g, got) == []
    assert cnt2.cpu().tolist() == g2.counts()
    assert H.check(model, 0, H.split(uoff.cpu().numpy(), useq.cpu().numpy())) == [] and ucnt.cpu().tolist()[:2] == [P, N]
    assert _sets(drows.cpu().numpy().reshape(ns, 1)) == g.colour_sets("or") and dgc.cpu().tolist() == [len(x) for x in g.colour_sets("or")]
    assert H.split(spoff.cpu().numpy(), spseq.cpu().numpy()) == sp_before and spcnt.cpu().tolist()[:2] == [SP, SN]
    assert (dbits.cpu().numpy().view(np.uint8)[:len(bits_h)] == bits_h).all()
    assert (doffc.cpu().numpy().astype(np.uint64) == off_h).all()
    assert (dids.cpu().numpy()[:len(ids_h)].astype(np.uint32) == ids_h).all()
    assert (dpo.cpu().numpy().astype(np.uint64) == po).all()
    # all earlier answers are unchanged
    after = t.unitigs(0)
    assert U._answers(t, asc, k) == before and t.simple_paths() == sp_before and U._rows(t) == model.rows
    assert after[0].tobytes() == ug_before[0].tobytes() and after[1].tobytes() == ug_before[1].tobytes()
    t.close()


def test_empty_index_stages_and_kernel_time():
    t = BFT(27, device=0)
    seg_off, seqs, link_off, links, members = t.unitig_graph()
    assert seg_off.tolist() == [0] and link_off.tolist() == [0] and len(seqs) == len(links) == len(members) == 0
    assert _counts(t, 0) == [0] * 6
    t.close()
    genomes, _ = H.width_case(27)
    t2 = U._ingest(genomes, 27)
    t2.unitig_graph()
    t2.kernel_time(reset=True)
    t2.unitigs()
    _, unitig_launches = t2.kernel_time(reset=True)
    t2.unitig_graph()
    ms, launches = t2.kernel_time(reset=True)
    assert launches > unitig_launches and ms > 0
    t2.set_option("build_stages", 1)
    t2.unitig_graph()
    names = [name for name, _, _ in t2.build_stages()]
    assert names and all(name.startswith("unitig graph:") for name in names if name != "start"), names
    t2.close()


# ---- a colour row per segment ---------------------------------------------------------------------------------------------------------------------
def _check_colours(t, g):
    seg_off, _, _, _, members = t.unitig_graph(g.t)
    for op in ("and", "or", "symdiff"):
        rows, counts = t.unitig_colors(members, seg_off, op)
        want = g.colour_sets(op)
        assert _sets(rows) == want, op
        assert counts.tolist() == [len(x) for x in want], op


@pytest.mark.parametrize("t_shared", (0, 2))
def test_colours_of_the_four_genome_cases(t_shared):
    for k in (27, 64):
        genomes, _ = H.width_case(k)
        t = U._ingest(genomes, k)
        _check_colours(t, G.graph("width_case", k, t_shared))
        t.close()


def test_colours_of_single_k_mers_and_of_the_long_chain():
    k = 36
    genomes, _ = H.hand_case(k)
    g = G.graph("hand_case", k, 0)
    assert min(map(len, g.segs)) == 1 and max(map(len, g.segs)) >= 3000  # a segment of one k-mer, the chain of 3000
    t = U._ingest(genomes, k)
    _check_colours(t, g)
    t.close()


@functools.lru_cache(maxsize=None)
def many_genomes_case(k=27, n_genomes=70):
    """(genomes, model): 70 genomes, each two windows of one ancestor with SNPs of its own: colour rows of 9 bytes, sets of every size"""
    rng = np.random.default_rng(7070)
    anc = S.random_genome(1200, 7071)
    genomes = []
    for j in range(n_genomes):
        mut = S.mutate(anc, 0.01, 7100 + j)
        a, b = int(rng.integers(0, 700)), int(rng.integers(0, 700))
        genomes.append([H.text(mut[a:a + 500]), H.text(mut[b:b + 400])])
    return genomes, H.Model(H.owners_of(genomes, k), k)


def test_colours_on_rows_wider_than_eight_bytes():
    genomes, model = many_genomes_case()
    t = U._ingest(genomes, model.k)
    for thr in (0, 40):
        g = G.Graph(model, thr)
        g.invariants()
        assert G.check(g, t.unitig_graph(thr)) == []
        _check_colours(t, g)
    got = t.unitig_graph(0)
    assert t.unitig_colors(got[4], got[0], "or")[0].shape == (len(got[0]) - 1, 9)
    t.close()


def test_colours_of_a_segment_that_the_reduction_splits():
    """a segment with more members than one wavefront reduces (bft_gpu_debug_setops_plan's out[1], 65536): the split road of the colour-set algebra"""
    plan = (C.c_uint64 * 6)()
    _lib.check(_lib.load().bft_gpu_debug_setops_plan(plan))
    assert plan[1] < 10 ** 5
    k, n = 27, int(plan[1]) + 1500
    chain = H.text(S.random_genome(n + k - 1, 99))
    genomes = [[chain], [chain[:n // 2]], [chain[n // 3:n // 3 + 5000]]]
    model = H.Model(H.owners_of(genomes, k), k)
    g = G.Graph(model, 0)
    assert len(g.segs) == 1 and len(g.segs[0]) > plan[1]
    t = U._ingest(genomes, k)
    assert G.check(g, t.unitig_graph(0)) == []
    _check_colours(t, g)
    assert g.colour_sets("and") == [{0}] and g.colour_sets("symdiff") == [{1, 2}]
    t.close()


def test_a_bad_member_in_both_forms():
    import torch
    k = 27
    genomes, model = H.width_case(k)
    g = G.graph("width_case", k, 0)
    t = U._ingest(genomes, k)
    seg_off, _, _, _, members = t.unitig_graph(0)
    ns, n2 = len(seg_off) - 1, 2 * len(model.rows)
    i = max(range(ns), key=lambda j: len(g.segs[j]))
    at = int(seg_off[i]) - i * (k - 1) + 1  # the second member of the longest segment
    bad = members.copy()
    bad[at] = n2
    lib = _lib.load()
    rows = np.full(ns, 7, dtype=np.uint8)
    counts = np.full(ns, 7, dtype=np.uint32)
    assert lib.bft_gpu_unitig_colors(t._h, bad.ctypes.data, len(bad), seg_off.ctypes.data, ns, 1, rows.ctypes.data, counts.ctypes.data) == -1  # BFT_GPU_E_ARG
    assert "member" in lib.bft_gpu_last_error().decode() and (rows == 7).all() and (counts == 7).all()
    short = seg_off.copy()
    short[1:] -= 2  # (segment 0 would be shorter than k - 1 characters: fewer than no member)
    assert lib.bft_gpu_unitig_colors(t._h, members.ctypes.data, len(members), short.ctypes.data, ns, 1, rows.ctypes.data, counts.ctypes.data) == -1
    assert (rows == 7).all() and (counts == 7).all()
    # the device form: the absent k-mer -- the empty set under AND, left out of OR
    dm, do = torch.from_numpy(bad.astype(np.int64)).to(torch.int32).cuda(), torch.from_numpy(seg_off.astype(np.int64)).cuda()
    for op in ("and", "or"):
        drows = torch.zeros(ns, dtype=torch.uint8, device="cuda")
        t.unitig_colors_dev(dm.data_ptr(), len(bad), do.data_ptr(), ns, op, drows.data_ptr(), 0)
        torch.cuda.synchronize()
        want = g.colour_sets(op)
        if op == "and":
            want[i] = set()
        else:
            sets = [model.owners[model.rows[v >> 1]] for j, v in enumerate(g.segs[i]) if j != 1]
            want[i] = set().union(*sets)
        assert _sets(drows.cpu().numpy().reshape(ns, 1)) == want, op
    t.close()
