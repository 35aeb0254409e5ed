"""Insertion from sequences on the GPU (bft_gpu_insert_sequences / _dev / bft_gpu_insert_sequence_file; csrc/bft_ingest.hip): an index built through
the new calls against an index built through insert_kmers of the truth's k-mers (tests/test_ingest_cases_host.py: plain Python, no kernel) with the
same genome ids -- the same extract() (k-mers and resolved colour sets), the same k-mer and pair counts after the build, and stats equal to the
truth's four numbers.  Host form and device form, the device blob at + 0, + 1 and + 3 bytes."""
import ctypes as C

import numpy as np
import pytest

from bloomfiltertrie_amd import BFT, _lib, synth as S
from test_ingest_cases_host import BY_NAME, CASES, Truth, chunks, normalise, plan, rand_text, with_bad

pytestmark = pytest.mark.gpu

E_ARG, E_LIMIT, E_STATE = -1, -3, -4
FORMS = ("host", "dev+0", "dev+1", "dev+3")


def ingest(t, seqs, gid, canonical, min_abundance, form="host", stream=None):
    if form == "host":
        return t.insert_sequences(seqs, gid, canonical=canonical, min_abundance=min_abundance)
    import torch
    shift = int(form[4:])
    blob = b"".join(seqs)
    off = np.zeros(len(seqs) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    d_blob = torch.zeros(len(blob) + 64, dtype=torch.uint8, device="cuda")
    assert d_blob.data_ptr() % 16 == 0
    if blob:
        d_blob[shift:shift + len(blob)] = torch.frombuffer(bytearray(blob), dtype=torch.uint8).cuda()
    d_off = torch.from_numpy(off).cuda()
    torch.cuda.synchronize()
    return t.insert_sequences_dev(d_blob.data_ptr() + shift, d_off.data_ptr(), len(seqs), len(blob), gid, canonical=canonical, min_abundance=min_abundance,
                                  stream=stream)


def state(t):
    """(k-mers as sortable rows, the genome ids of each, k-mer count, pair count) of the built index"""
    t.build()
    km, cs = t.extract()
    sets = {int(c): tuple(t.colorset(int(c))) for c in np.unique(cs)}
    info = t.info()
    return km, [sets[int(c)] for c in cs], info["kmers"], info["pairs"]


def same(a, b, what=""):
    ka, sa, na, pa = state(a)
    kb, sb, nb, pb = state(b)
    assert (na, pa) == (nb, pb), what
    assert ka.shape == kb.shape and (ka == kb).all(), what
    assert sa == sb, what
    return na, pa


def reference(k, ops, options=()):
    """the index insert_kmers builds from the truth's k-mers: ops = [(genome id, packed k-mers)]"""
    r = BFT(k, device=0)
    for name, v in options:
        r.set_option(name, v)
    for gid, packed in ops:
        if len(packed):
            r.insert_kmers(packed, gid)
    return r


def run_case(c, form, options=()):
    t = BFT(c.k, device=0)
    for name, v in options:
        t.set_option(name, v)
    # a second genome of plain k-mers beside it, so that an ingest that appends nothing still leaves an index to compare
    other = S.distinct(S.kmers_of(S.random_genome(200 + c.k, 99), c.k))
    t.insert_kmers(other, 1)
    st = ingest(t, c.seqs, 0, c.canonical, c.min_abundance, form)
    assert st == c.truth.stats(), (c.name, form)
    assert t.info()["pending_pairs"] == len(other) + c.truth.appended
    r = reference(c.k, [(1, other), (0, c.truth.packed(c.k))])
    same(t, r, (c.name, form))
    if c.truth.appended == 0:  # the genome keeps no k-mer
        assert all(0 not in s for s in state(t)[1])
    t.close()
    r.close()


def _runs():
    """every case through the host form and an unaligned device blob; where the blob's alignment matters -- the encoder and the window's shifts:
    the geometry and canonical cases -- also at + 0 and + 3 bytes"""
    out = []
    for c in CASES:
        if c.name.startswith("chunk-"):
            continue
        every = c.min_abundance == 0 and not c.name.startswith(("valid-", "empty-tile", "alternating", "reads5000"))
        out += [pytest.param(c, f, id=f"{c.name}-{f}") for f in (FORMS if every else ("host", "dev+1"))]
    return out


@pytest.mark.parametrize("case,form", _runs())
def test_ingest_equals_insert_kmers_of_the_truth(case, form):
    run_case(case, form)


@pytest.mark.parametrize("case", [c for c in CASES if c.name.startswith("chunk-")], ids=repr)
def test_chunked_host_form(case):
    """"ingest_chunk_chars" at its minimum: the same index and the same stats as with the default chunk"""
    cmin = plan()[2]
    assert len(chunks([len(s) for s in case.seqs], case.k, cmin)) > 1
    run_case(case, "host", options=(("ingest_chunk_chars", cmin),))
    run_case(case, "host")
    a, b = BFT(case.k, device=0), BFT(case.k, device=0)
    a.set_option("ingest_chunk_chars", cmin)
    assert ingest(a, case.seqs, 0, case.canonical, 0) == ingest(b, case.seqs, 0, case.canonical, 0)
    same(a, b, case.name)
    a.close()
    b.close()


def test_chunk_option_bounds():
    t = BFT(27, device=0)
    cmin = plan()[2]
    t.set_option("ingest_chunk_chars", cmin)
    with pytest.raises(_lib.BFTError):
        t.set_option("ingest_chunk_chars", cmin - 1)
    t.close()


# ---- counting: the limit ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ("host", "dev+1"))
def test_counting_call_beyond_flush_pairs_is_refused(form):
    k = 27
    rng = np.random.default_rng(5)
    t = BFT(k, device=0)
    t.set_option("flush_pairs", 1024)
    first = [rand_text(300, rng)]
    ingest(t, first, 0, False, 1, form)
    pending = t.info()["pending_pairs"]
    assert pending == Truth(first, k, False, 1).appended > 0
    big = [rand_text(1025 + k - 1, rng)]  # 1025 positions
    with pytest.raises(_lib.BFTError) as e:
        ingest(t, big, 1, False, 1, form)
    assert "error %d" % E_LIMIT in str(e.value)
    assert t.info()["pending_pairs"] == pending  # the log is unchanged
    ok = [rand_text(1024 + k - 1, rng)]  # exactly flush_pairs positions: taken (a build in front: the log would pass the limit)
    assert ingest(t, ok, 1, False, 1, form) == Truth(ok, k, False, 1).stats()
    r = reference(k, [(0, Truth(first, k, False, 1).packed(k)), (1, Truth(ok, k, False, 1).packed(k))])
    same(t, r)
    t.close()
    r.close()


# ---- log states ------------------------------------------------------------------------------------------------------------------------------
def _three_steps(k, rng):
    s0, s1 = [rand_text(400, rng), with_bad(rand_text(300, rng), 150)], [rand_text(500, rng)]
    km = S.distinct(S.kmers_of(S.random_genome(600, k), k))
    return s0, km, s1


@pytest.mark.parametrize("k", (27, 63))
@pytest.mark.parametrize("composite", (1, 0))
def test_sequences_kmers_sequences_and_ids_out_of_order(k, composite):
    """sequences for genome 0, k-mers for genome 1, sequences for genome 0 again: the ids of the log no longer ascend.  k = 27 with
    "composite_log" 1 starts in the composite form (T << cgb | genome) and leaves it at the build."""
    rng = np.random.default_rng(k)
    s0, km, s1 = _three_steps(k, rng)
    t = BFT(k, device=0)
    t.set_option("composite_log", composite)
    ingest(t, s0, 0, True, 0, "host")
    t.insert_kmers(km, 1)
    ingest(t, s1, 0, True, 0, "dev+3")
    ingest(t, s1, 2, False, 2, "dev+1")
    ops = [(0, Truth(s0, k, True, 0).packed(k)), (1, km), (0, Truth(s1, k, True, 0).packed(k)), (2, Truth(s1, k, False, 2).packed(k))]
    r = reference(k, ops, options=(("composite_log", composite),))
    assert t.info()["pending_pairs"] == r.info()["pending_pairs"]
    same(t, r)
    t.close()
    r.close()


def test_genome_id_too_large_for_the_composites():
    """k = 27: 63 - 2k = 9 bits of genome id beside the key; id 600 has no room, the log leaves the composite form in front of the call"""
    k = 27
    rng = np.random.default_rng(1)
    s0, km, s1 = _three_steps(k, rng)
    for min_abundance in (0, 1):
        t = BFT(k, device=0)
        ingest(t, s0, 3, False, min_abundance, "host")
        ingest(t, s1, 600, False, min_abundance, "dev+1")
        ingest(t, s0, 601, True, min_abundance, "host")
        ops = [(3, Truth(s0, k, False, min_abundance).packed(k)), (600, Truth(s1, k, False, min_abundance).packed(k)), (601, Truth(s0, k, True, min_abundance).packed(k))]
        r = reference(k, ops)
        same(t, r)
        t.close()
        r.close()


@pytest.mark.parametrize("k", (27, 63))
@pytest.mark.parametrize("form", ("host", "dev+1"))
def test_stream_call_beyond_flush_pairs_goes_in_pieces(k, form):
    """"flush_pairs" 1024 and a call of more positions than that: pieces of whole tiles, and a build in front of a piece that would pass it"""
    rng = np.random.default_rng(k + 1)
    tile = plan()[0]
    t = BFT(k, device=0)
    t.set_option("flush_pairs", 1024)
    first = [rand_text(700, rng)]
    seqs = [rand_text(900, rng), with_bad(rand_text(2 * 1024 + 3 * tile + 5, rng), [1000, 1024 + k, 2100]), rand_text(k, rng), rand_text(300, rng)]
    assert ingest(t, first, 0, False, 0, form) == Truth(first, k, False, 0).stats()
    assert t.info()["pending_pairs"] == 700 - k + 1
    truth = Truth(seqs, k, True, 0)
    assert truth.positions > 3 * 1024
    assert ingest(t, seqs, 1, True, 0, form) == truth.stats()
    assert t.info()["pending_pairs"] <= 1024 and t.info()["kmers"] > 0  # builds happened in front of pieces
    r = reference(k, [(0, Truth(first, k, False, 0).packed(k)), (1, truth.packed(k))])
    same(t, r)
    t.close()
    r.close()


@pytest.mark.parametrize("k", (27, 72))
def test_ingest_into_a_built_index_merges(k):
    rng = np.random.default_rng(k + 2)
    s0, km, s1 = _three_steps(k, rng)
    t = BFT(k, device=0)
    t.insert_kmers(km, 0)
    ingest(t, s0, 1, False, 0, "host")
    t.build()
    built = t.info()["kmers"]
    assert built > 0 and t.info()["pending_pairs"] == 0
    ingest(t, s1, 2, True, 0, "dev+1")
    ingest(t, s0 + s1, 3, True, 2, "host")
    ops = [(0, km), (1, Truth(s0, k, False, 0).packed(k)), (2, Truth(s1, k, True, 0).packed(k)), (3, Truth(s0 + s1, k, True, 2).packed(k))]
    r = reference(k, ops)
    n, _ = same(t, r)
    assert n > built
    t.close()
    r.close()


# ---- round trip ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (27, 33, 64, 126))
@pytest.mark.parametrize("canonical", (False, True))
def test_ingested_sequences_are_found_by_query_sequences(k, canonical):
    """After a stream-path ingest, query_sequences of the same sequences with the same `canonical` finds the genome.  The threshold applies to
    ALL positions of a sequence, the skipped ones included (ceil(positions x threshold), src/bft.c:1279-1281), so at 1.0 the genome is reported
    for every sequence whose windows are all valid and never for one without a valid window; that every sequence WITH a valid window finds the
    genome is asserted at the smallest threshold."""
    c = BY_NAME[f"n-runs-k{k}"]
    rng = np.random.default_rng(k)
    seqs = c.seqs + [rand_text(150, rng) for _ in range(50)] + [rand_text(k - 1, rng), b""]
    t = BFT(k, device=0)
    t.insert_kmers(S.distinct(S.kmers_of(S.random_genome(300, 3), k)), 0)
    ingest(t, seqs, 1, canonical, 0, "host")
    got = t.query_sequences(seqs, 1.0, canonical=canonical)
    for s, g in zip(seqs, got):
        r = normalise(s)
        has_window = any("N" not in r[i:i + k] for i in range(len(r) - k + 1))
        # threshold 1.0 counts the skipped windows of a sequence against it: the genome is reported when every window is valid
        all_valid = len(r) >= k and "N" not in r
        if all_valid:
            assert 1 in g, s
        if not has_window:
            assert 1 not in g, s
    # ... and every sequence with a valid window is reported at the smallest threshold
    low = t.query_sequences(seqs, 1e-9, canonical=canonical)
    for s, g in zip(seqs, low):
        r = normalise(s)
        assert (1 in g) == any("N" not in r[i:i + k] for i in range(len(r) - k + 1)), s
    t.close()


# ---- files -----------------------------------------------------------------------------------------------------------------------------------
def test_sequence_files(tmp_path):
    k = 27
    rng = np.random.default_rng(11)
    seqs = [rand_text(200, rng), with_bad(rand_text(90, rng), 40), b"", rand_text(k, rng)]
    fa = tmp_path / "g.fa"
    fa.write_bytes(b"".join(b">s%d\n" % i + b"\n".join(s[j:j + 60] for j in range(0, len(s), 60)) + b"\n" for i, s in enumerate(seqs)))
    fq = tmp_path / "r.fq"
    fq.write_bytes(b"".join(b"@r%d\n%s\n+\n%s\n" % (i, s, b"I" * len(s)) for i, s in enumerate(seqs)))
    for path in (fa, fq):
        for canonical, c in ((False, 0), (True, 2)):
            t = BFT(k, device=0)
            truth = Truth(seqs, k, canonical, c)
            assert t.insert_sequence_file(str(path), 0, canonical=canonical, min_abundance=c) == truth.stats()
            t.insert_kmers(truth.packed(k)[:1] if truth.appended else S.kmers_of(S.random_genome(k, 1), k), 1)
            r = reference(k, [(0, truth.packed(k)), (1, truth.packed(k)[:1] if truth.appended else S.kmers_of(S.random_genome(k, 1), k))])
            same(t, r)
            t.close()
            r.close()
    t = BFT(k, device=0)
    bad = tmp_path / "neither.txt"
    bad.write_bytes(b"ACGT\n")
    for path in (bad, tmp_path / "missing.fa"):
        with pytest.raises(_lib.BFTError) as e:
            t.insert_sequence_file(str(path), 0)
        assert "error -5" in str(e.value)  # BFT_GPU_E_IO
    assert t.info()["pending_pairs"] == 0
    t.close()


# ---- errors ----------------------------------------------------------------------------------------------------------------------------------
def test_errors():
    import torch
    k = 27
    lib = _lib.load()
    rng = np.random.default_rng(3)
    seq = rand_text(100, rng)
    off = np.array([0, len(seq)], dtype=np.uint64)
    st = (C.c_uint64 * 4)()
    t = BFT(k, device=0)
    t.insert_sequences([seq], 0)
    t.build()
    # locked for marking
    t.set_marking()
    assert lib.bft_gpu_insert_sequences(t._h, seq, off.ctypes.data, 1, 0, 0, 0, st) == E_STATE
    d_blob = torch.frombuffer(bytearray(seq), dtype=torch.uint8).cuda()
    d_off = torch.from_numpy(off.astype(np.int64)).cuda()
    torch.cuda.synchronize()
    dev = lambda h, blob, offs, n, gid, stream=None: lib.bft_gpu_insert_sequences_dev(h, C.c_void_p(blob), C.c_void_p(offs), n, len(seq), 0, 0, gid, st, C.c_void_p(stream or 0))
    assert dev(t._h, d_blob.data_ptr(), d_off.data_ptr(), 1, 0) == E_STATE
    t.unset_marking()
    pending = t.info()["pending_pairs"]
    # id_genome >= 2^24
    assert lib.bft_gpu_insert_sequences(t._h, seq, off.ctypes.data, 1, 0, 0, 1 << 24, st) == E_ARG
    assert dev(t._h, d_blob.data_ptr(), d_off.data_ptr(), 1, 1 << 24) == E_ARG
    assert lib.bft_gpu_insert_sequence_file(t._h, b"/nonexistent", 0, 0, 1 << 24, st) in (E_ARG, -5)
    # decreasing offsets (host form)
    dec = np.array([0, 60, 40, 100], dtype=np.uint64)
    assert lib.bft_gpu_insert_sequences(t._h, seq, dec.ctypes.data, 3, 0, 0, 0, st) == E_ARG
    assert b"decrease" in lib.bft_gpu_last_error()
    # NULL with work
    assert lib.bft_gpu_insert_sequences(t._h, None, off.ctypes.data, 1, 0, 0, 0, st) == E_ARG
    assert lib.bft_gpu_insert_sequences(t._h, seq, None, 1, 0, 0, 0, st) == E_ARG
    assert dev(t._h, 0, d_off.data_ptr(), 1, 0) == E_ARG
    assert dev(t._h, d_blob.data_ptr(), 0, 1, 0) == E_ARG
    assert lib.bft_gpu_insert_sequences(None, seq, off.ctypes.data, 1, 0, 0, 0, st) == E_ARG
    assert lib.bft_gpu_insert_sequence_file(t._h, None, 0, 0, 0, st) == E_ARG
    # nb_seqs == 0: fine, nothing appended, NULL everything
    st[3] = 7
    assert lib.bft_gpu_insert_sequences(t._h, None, None, 0, 0, 0, 0, st) == 0 and list(st) == [0, 0, 0, 0]
    assert dev(t._h, 0, 0, 0, 0) == 0
    assert lib.bft_gpu_insert_sequences(t._h, seq, off.ctypes.data, 1, 0, 0, 0, None) == 0  # stats may be NULL
    assert t.info()["pending_pairs"] == pending + len(seq) - k + 1
    pending = t.info()["pending_pairs"]
    # a stream that is capturing
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        assert dev(t._h, d_blob.data_ptr(), d_off.data_ptr(), 1, 0, s.cuda_stream) == 0  # (a direct call on that stream first)
    s.synchronize()
    pending += len(seq) - k + 1
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        d_off.add_(0)  # (the recorded graph is not empty)
        rc = dev(t._h, d_blob.data_ptr(), d_off.data_ptr(), 1, 0, torch.cuda.current_stream().cuda_stream)
    del g  # (never replayed)
    assert rc == E_ARG
    assert t.info()["pending_pairs"] == pending
    t.close()


def test_launches_are_timed_and_stages_reported():
    k = 63
    rng = np.random.default_rng(9)
    seqs = [rand_text(3000, rng)]
    t = BFT(k, device=0)
    t.set_option("timing", 1)
    t.kernel_time()
    ingest(t, seqs, 0, True, 0)
    ms, n = t.kernel_time()
    assert n >= 4 and ms > 0  # encode, plan, count, scan, write
    ingest(t, seqs, 1, True, 2)
    ms2, n2 = t.kernel_time()
    assert n2 > n and ms2 > 0  # ... + keys, sort, run lengths, kept rows
    t.set_option("build_stages", 1)
    ingest(t, seqs, 2, False, 0)
    names = [s[0] for s in t.build_stages()]
    assert any("windows -> log rows" in x for x in names) and any("encode" in x for x in names), names
    ingest(t, seqs, 3, False, 1)
    names = [s[0] for s in t.build_stages()]
    assert any("sort" in x for x in names) and any("run lengths" in x for x in names), names
    t.close()


def test_calls_on_two_streams_share_the_scratch():
    """the ingest scratch is the handle's: calls on two streams take turns, each result is whole"""
    import torch
    k = 33
    rng = np.random.default_rng(4)
    a, b = [rand_text(5000, rng)], [rand_text(700, rng), rand_text(40, rng)]
    t = BFT(k, device=0)
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    ingest(t, a, 0, False, 0, "dev+1", sa.cuda_stream)
    ingest(t, b, 1, True, 1, "dev+3", sb.cuda_stream)
    ingest(t, a, 2, True, 0, "dev+0", sa.cuda_stream)
    ingest(t, b, 3, False, 0, "host")
    r = reference(k, [(0, Truth(a, k, False, 0).packed(k)), (1, Truth(b, k, True, 1).packed(k)), (2, Truth(a, k, True, 0).packed(k)), (3, Truth(b, k, False, 0).packed(k))])
    same(t, r)
    t.close()
    r.close()
