"""Canonical (bidirected) unitigs and degrees on the GPU (bft_gpu_unitigs / _dev, bft_gpu_bidirected_degrees / _dev, BFT.unitigs,
BFT.bidirected_degrees): exact against the model of tests/test_unitigs_host.py, which is written from the definition alone and proves its
invariants on the same cases on the CPU.  Key widths W = 1..4 and both T-form tail layouts; hand-made situations at odd and even k (lone k-mer,
homopolymer, palindromes, hairpin, two successor words on two strands, a palindromic successor, a circle and the same circle from its other strand,
a chain of 3000 k-mers and more whose stored strand keeps flipping); one index just past the capped grid; the whole table as one chain and as
one cycle of 1 .. 1025 k-mers (the jumps' last round); thresholds 0, 1, 2, N, N + 1; index states
that all give the same unitigs; an index that is not canonical; caps, NOSPACE and guard bytes; the device form on a user stream interleaved with
simple paths, colour and prefix queries on one handle."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from bloomfiltertrie_amd import BFT, _lib, synth as S

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_unitigs_host as H  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 64


def _ingest(genomes, k, options=(), build_each=False, t=None, first_gid=0):
    if t is None:
        t = BFT(k, device=0)
    for name, v in options:
        t.set_option(name, v)
    for j, seqs in enumerate(genomes):
        gid = t.add_genome(f"g{first_gid + j}")
        t.insert_sequences(seqs, gid, canonical=True)
        if build_each:
            t.build()
    return t


def _rows(t):
    km, _ = t.extract()
    return S.packed_to_ascii(km, t.k)


def _check_all(t, model, thresholds):
    assert _rows(t) == model.rows  # (the model's row order is the library's)
    deg, bad = t.bidirected_degrees()
    assert bad == 0 and deg.tobytes() == model.degrees()
    for thr in thresholds:
        problems = H.check(model, thr, H.split(*t.unitigs(thr)))
        assert problems == [], (t.k, thr, problems[:5])


@pytest.mark.parametrize("k", H.KS)
def test_unitigs_match_the_model_at_every_key_width(k):
    genomes, model = H.width_case(k)
    t = _ingest(genomes, k)
    _check_all(t, model, (0, 1, 2, H.N_GENOMES, H.N_GENOMES + 1))
    off, seqs = t.unitigs(H.N_GENOMES + 1)
    assert off.tolist() == [0] and len(seqs) == 0
    t.close()


@pytest.mark.parametrize("k", H.HAND_KS)
def test_hand_made_situations(k):
    genomes, model = H.hand_case(k)
    t = _ingest(genomes, k)
    t.kernel_time(reset=True)
    _check_all(t, model, (0, 1, 2))
    if "chain" in H.hand_parts(k):
        t.kernel_time(reset=True)
        t.unitigs(0)
        _, launches = t.kernel_time(reset=True)
        assert launches >= 12 + 8  # (12 rounds of jumps or more: the chain holds 3000 k-mers)
    # the circle read from its other strand: the same index, byte-identical output
    other = [[H.rc(q) if q == H.hand_parts(k)["circle"][0] else q for q in genomes[0]], genomes[1]]
    assert other != genomes
    t2 = _ingest(other, k)
    for thr in (0, 1):
        a, b = t.unitigs(thr), t2.unitigs(thr)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    t.close()
    t2.close()


def test_grid_edge():
    """2n vertices exceed the capped grid's threads: every vertex kernel takes a second grid-stride pass"""
    genomes, model = H.grid_case()
    t = _ingest(genomes, H.GRID_K)
    _check_all(t, model, (0,))
    assert 2 * t.info()["kmers"] > 524288
    t.close()


@pytest.mark.parametrize("k", H.WHOLE_KS)
@pytest.mark.parametrize("kind", ("chain", "cycle"))
@pytest.mark.parametrize("n", H.WHOLE_NS)
def test_whole_table_is_one_path(n, kind, k):
    """as tests/test_gpu_graph_edges.py's case of the same name, through the mirrored instantiations of the shared kernels"""
    genomes, model = H.whole_case(n, kind, k)
    t = _ingest(genomes, k)
    _check_all(t, model, (0, 1, 2))
    off, seqs = t.unitigs(0)
    assert off.tolist() == [0, n + k - 1] and len(seqs) == n + k - 1  # one path
    t.close()


@pytest.mark.parametrize("state", ["compact0", "compact1", "kmer_hash0", "pending", "merge", "file", "image"])
@pytest.mark.parametrize("k", (27, 63))
def test_index_states_give_the_same_unitigs(state, k, tmp_path):
    genomes, model = H.width_case(k)
    keep = []
    if state in ("compact0", "compact1", "kmer_hash0"):
        opts = {"compact0": [("compact_table", 0)], "compact1": [("compact_table", 1)], "kmer_hash0": [("kmer_hash", 0)]}[state]
        t = _ingest(genomes, k, options=opts, build_each=True)
    elif state == "pending":
        t = _ingest(genomes[:3], k)
        t.unitigs(0)
        _ingest(genomes[3:], k, t=t, first_gid=3)  # (pending: built by the next call)
    elif state == "merge":
        a, b = _ingest(genomes[:2], k), _ingest(genomes[2:], k)
        t = a.merge(b)
        keep = [a, b]
    elif state == "file":
        a = _ingest(genomes, k)
        path = str(tmp_path / "i.bft")
        a.write_bft(path)
        t = BFT.load_bft(path)
        keep = [a]
    else:
        import torch
        a = _ingest(genomes, k)
        a.build()
        nbytes = a.image_size()
        blob = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        a.image_pack(blob.data_ptr(), nbytes)
        torch.cuda.synchronize()
        t = BFT.from_image(blob.data_ptr(), nbytes)
        keep = [a]
    _check_all(t, model, (0, 2))
    t.close()
    for x in keep:
        x.close()


def _noncanonical(k):
    kmers, model = H.noncanonical_case(k)
    t = BFT(k, device=0)
    t.add_genome("g0")
    t.insert_kmers(S.ascii_to_packed(kmers, k)[0], 0)
    return t, model


def _guarded(torch, nbytes, fill=7):
    buf = torch.full((GUARD + nbytes + GUARD,), fill, dtype=torch.uint8, device="cuda")
    return buf, buf.data_ptr() + GUARD


def _guards_intact(buf, nbytes, fill=7):
    h = buf.cpu().numpy()
    return (h[:GUARD] == fill).all() and (h[GUARD + nbytes:] == fill).all()


@pytest.mark.parametrize("k", (27, 36))
def test_degrees_and_refusal_on_an_index_that_is_not_canonical(k):
    import torch
    t, model = _noncanonical(k)
    assert model.noncanonical > 0
    deg, bad = t.bidirected_degrees()
    assert _rows(t) == model.rows and bad == model.noncanonical and deg.tobytes() == model.degrees()
    lib = _lib.load()
    npaths, nchars = C.c_uint64(5), C.c_uint64(5)
    off = np.full(4096, 7, dtype=np.uint64)
    seq = np.full(1 << 16, 7, dtype=np.uint8)
    assert lib.bft_gpu_unitigs(t._h, 0, None, None, 0, 0, C.byref(npaths), C.byref(nchars)) == -4  # BFT_GPU_E_STATE
    assert lib.bft_gpu_unitigs(t._h, 0, off.ctypes.data, seq.ctypes.data, len(off) - 1, len(seq), C.byref(npaths), C.byref(nchars)) == -4
    assert "not canonical" in lib.bft_gpu_last_error().decode() and (off == 7).all() and (seq == 7).all()
    # the device form: the count of non-canonical rows, nothing beyond the caps
    cbuf, cptr = _guarded(torch, 32)
    obuf, optr = _guarded(torch, 11 * 8)
    sbuf, sptr = _guarded(torch, 100)
    dbuf, dptr = _guarded(torch, len(model.rows) - 3)
    nbuf, nptr = _guarded(torch, 8)
    t.unitigs_dev(optr, sptr, 10, 100, cptr)
    t.bidirected_degrees_dev(dptr, len(model.rows) - 3, nptr)
    torch.cuda.synchronize()
    assert cbuf.cpu().numpy()[GUARD:GUARD + 32].view(np.uint64)[3] == model.noncanonical
    assert nbuf.cpu().numpy()[GUARD:GUARD + 8].view(np.uint64)[0] == model.noncanonical
    assert dbuf.cpu().numpy()[GUARD:-GUARD].tobytes() == model.degrees()[:-3]
    for buf, nb in ((cbuf, 32), (obuf, 88), (sbuf, 100), (dbuf, len(model.rows) - 3), (nbuf, 8)):
        assert _guards_intact(buf, nb)
    t.close()


def test_caps_and_nospace_host_form():
    k = 27
    genomes, model = H.width_case(k)
    t = _ingest(genomes, k)
    want = model.unitigs(0)
    lib = _lib.load()
    npaths, nchars = C.c_uint64(), C.c_uint64()
    assert lib.bft_gpu_unitigs(t._h, 0, None, None, 0, 0, C.byref(npaths), C.byref(nchars)) == 0
    P, N = npaths.value, nchars.value
    assert P == len(want) and N == sum(map(len, want))
    off = np.full(P + 1, 7, dtype=np.uint64)
    seq = np.full(N, 7, dtype=np.uint8)
    assert lib.bft_gpu_unitigs(t._h, 0, off.ctypes.data, seq.ctypes.data, P - 1, N, C.byref(npaths), C.byref(nchars)) == -6
    assert (npaths.value, nchars.value) == (P, N) and (off == 7).all() and (seq == 7).all()
    assert lib.bft_gpu_unitigs(t._h, 0, off.ctypes.data, seq.ctypes.data, P, N - 1, C.byref(npaths), C.byref(nchars)) == -6
    assert (off == 7).all() and (seq == 7).all()
    assert lib.bft_gpu_unitigs(t._h, 0, off.ctypes.data, None, P, 0, C.byref(npaths), C.byref(nchars)) == 0
    assert off[0] == 0 and off[-1] == N and (np.diff(off.astype(np.int64)) >= k).all()
    assert lib.bft_gpu_unitigs(t._h, 0, off.ctypes.data, seq.ctypes.data, P, N, C.byref(npaths), C.byref(nchars)) == 0
    assert H.split(off, seq) == want
    n = len(model.rows)
    deg = np.full(n, 7, dtype=np.uint8)
    bad = C.c_uint64(9)
    assert lib.bft_gpu_bidirected_degrees(t._h, deg.ctypes.data, n - 1, C.byref(bad)) == -6 and (deg == 7).all()
    assert lib.bft_gpu_bidirected_degrees(t._h, None, 0, C.byref(bad)) == 0 and bad.value == 0
    assert lib.bft_gpu_bidirected_degrees(t._h, deg.ctypes.data, n, C.byref(bad)) == 0 and deg.tobytes() == model.degrees()
    t.close()


def test_caps_in_the_device_form_leave_guard_bytes():
    import torch
    k = 36
    genomes, model = H.width_case(k)
    t = _ingest(genomes, k)
    want = model.unitigs(0)
    P, N = len(want), sum(map(len, want))
    ends = np.cumsum([0] + [len(s) for s in want]).astype(np.uint64)
    # caps one below need
    cbuf, cptr = _guarded(torch, 32)
    obuf, optr = _guarded(torch, P * 8)
    sbuf, sptr = _guarded(torch, N - 1)
    t.unitigs_dev(optr, sptr, P - 1, N - 1, cptr)
    torch.cuda.synchronize()
    assert cbuf.cpu().numpy()[GUARD:GUARD + 32].view(np.uint64).tolist() == [P, N, max(map(len, want)), 0]
    assert (obuf.cpu().numpy()[GUARD:GUARD + P * 8].view(np.uint64) == ends[:P]).all()
    assert sbuf.cpu().numpy()[GUARD:GUARD + N - 1].tobytes().decode() == "".join(want)[:N - 1]
    assert _guards_intact(cbuf, 32) and _guards_intact(obuf, P * 8) and _guards_intact(sbuf, N - 1)
    # caps of zero: offsets[0] alone, no character
    obuf, optr = _guarded(torch, 8)
    sbuf, sptr = _guarded(torch, 0)
    t.unitigs_dev(optr, sptr, 0, 0, cptr)
    torch.cuda.synchronize()
    assert cbuf.cpu().numpy()[GUARD:GUARD + 24].view(np.uint64).tolist() == [P, N, max(map(len, want))]
    assert obuf.cpu().numpy()[GUARD:GUARD + 8].view(np.uint64)[0] == 0 and _guards_intact(obuf, 8) and _guards_intact(sbuf, 0)
    t.close()


def _answers(t, kmers, k):
    q, _ = S.ascii_to_packed(kmers, k)
    q = np.concatenate([q, S.snp_mutants(q[:200], k, 5)])
    bits, off, ids = t.query_colors(q)
    _, rows, _ = t.query_rows(q)
    return bits.tobytes(), off.tobytes(), ids.tobytes(), rows.tobytes()


def test_dev_form_on_a_user_stream_interleaved_with_other_queries():
    import torch
    k = 36
    genomes, model = H.width_case(k)
    t = _ingest(genomes, k)
    want, want2 = model.unitigs(0), model.unitigs(2)
    P, N = len(want), sum(map(len, want))
    asc = model.rows[::5]
    before = _answers(t, asc, k)
    sp_before = t.simple_paths()
    q, _ = S.ascii_to_packed(asc, k)
    n = len(q)
    bits_h, off_h, ids_h = t.query_colors(q)
    pref = q[:64].copy()
    po, pk, pr, pc = t.query_prefixes(pref, np.full(64, 20, dtype=np.uint8))
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
        cnt = torch.full((4,), 7, dtype=torch.int64, device="cuda")
        t.unitigs_dev(0, 0, 0, 0, cnt.data_ptr(), stream=s.cuda_stream)  # sizing
    s.synchronize()
    assert cnt.cpu().tolist() == [P, N, max(map(len, want)), 0]
    with torch.cuda.stream(s):
        doff = torch.full((P + 1,), 7, dtype=torch.int64, device="cuda")
        dseq = torch.full((N,), 7, dtype=torch.uint8, device="cuda")
        spoff = torch.full((SP + 1,), 7, dtype=torch.int64, device="cuda")
        spseq = torch.full((SN,), 7, dtype=torch.uint8, device="cuda")
        spcnt = torch.zeros(3, dtype=torch.int64, device="cuda")
        ddeg = torch.full((len(model.rows),), 7, dtype=torch.uint8, device="cuda")
        dbad = torch.full((1,), 7, dtype=torch.int64, device="cuda")
        t.query_colors_dev(dq.data_ptr(), n, dbits.data_ptr(), doffc.data_ptr(), dids.data_ptr(), len(ids_h) + 1, stream=s.cuda_stream)
        t.unitigs_dev(doff.data_ptr(), dseq.data_ptr(), P, N, cnt.data_ptr(), stream=s.cuda_stream)
        t.simple_paths_dev(spoff.data_ptr(), spseq.data_ptr(), SP, SN, spcnt.data_ptr(), stream=s.cuda_stream)
        t.query_prefixes_dev(dp.data_ptr(), dl.data_ptr(), 64, dpo.data_ptr(), 0, 0, 0, 0, 0, stream=s.cuda_stream)
        t.bidirected_degrees_dev(ddeg.data_ptr(), len(model.rows), dbad.data_ptr(), stream=s.cuda_stream)
        cnt2 = torch.zeros(4, dtype=torch.int64, device="cuda")
        t.unitigs_dev(0, 0, 0, 0, cnt2.data_ptr(), min_shared=2, stream=s.cuda_stream)
    s.synchronize()
    assert H.check(model, 0, H.split(doff.cpu().numpy(), dseq.cpu().numpy())) == []
    assert cnt2.cpu().tolist()[:2] == [len(want2), sum(map(len, want2))]
    assert H.split(spoff.cpu().numpy(), spseq.cpu().numpy()) == sp_before and spcnt.cpu().tolist()[:2] == [SP, SN]
    assert ddeg.cpu().numpy().tobytes() == model.degrees() and dbad.cpu().tolist() == [0]
    assert (dbits.cpu().numpy().view(np.uint8)[:len(bits_h)] == bits_h).all()
    assert (doffc.cpu().numpy().astype(np.uint64) == off_h).all()
    assert (dids.cpu().numpy()[:len(ids_h)].astype(np.uint32) == ids_h).all()
    assert (dpo.cpu().numpy().astype(np.uint64) == po).all()
    # all earlier answers are unchanged
    assert _answers(t, asc, k) == before and t.simple_paths() == sp_before and _rows(t) == model.rows
    t.close()


def test_empty_index_and_kernel_time():
    t = BFT(27, device=0)
    off, seqs = t.unitigs()
    assert off.tolist() == [0] and len(seqs) == 0
    deg, bad = t.bidirected_degrees()
    assert len(deg) == 0 and bad == 0
    t.close()
    genomes, _ = H.width_case(27)
    t2 = _ingest(genomes, 27)
    t2.unitigs()
    t2.kernel_time(reset=True)
    t2.unitigs()
    ms, launches = t2.kernel_time(reset=True)
    assert launches >= 10 and ms > 0
    t2.close()
