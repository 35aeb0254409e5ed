"""Simple paths on the GPU (bft_gpu_simple_paths / _dev, BFT.simple_paths): against ground truth computed in Python from the inserted k-mer
strings and their genome sets (the product's extract only orders the paths by row), at key widths W = 1, 2 and 4 (KS has no three-word key, k = 65..96; tests/test_gpu_graph_edges.py runs W = 3 and the other key shapes); hand-made graphs (a circular
genome, a homopolymer self-loop, a lone k-mer, a k-mer with two successors); thresholds 0, 1, 2, N and N + 1; index states (compact_table,
kmer_hash 0, pending insertions, merges, a .bft round trip) that all give the same paths; caps and NOSPACE; the device form on a user stream,
interleaved with colour and prefix queries on one handle; the handle's answers unchanged afterwards."""
import ctypes as C

import numpy as np
import pytest

from bloomfiltertrie_amd import BFT, _lib, synth as S

pytestmark = pytest.mark.gpu

KS = (9, 18, 27, 31, 36, 63, 64, 126)
N_GENOMES = 4


def _genomes(seed, length):
    """Four related genomes: an ancestor with a repeated stretch (branching at both of its ends), and SNP mutants of it."""
    rng = np.random.default_rng(seed)
    anc = S.random_genome(length, seed + 1)
    a = int(rng.integers(0, length // 3))
    b = int(rng.integers(length // 2, length - 400))
    anc[b:b + 300] = anc[a:a + 300]
    return [anc] + [S.mutate(anc, 0.01, seed + 2 + g) for g in range(N_GENOMES - 1)]


def _owners_of(kmer_lists):
    """[(ASCII k-mers, genome id)] -> {k-mer: set of genome ids}"""
    owners = {}
    for asc, gid in kmer_lists:
        for s in asc:
            owners.setdefault(s, set()).add(gid)
    return owners


def _truth(owners, k, t, row_of):
    """The simple paths of include/bft_gpu.h's definition, by dicts and sets, ordered by the row of their first k-mer."""
    def succ(x):
        return [x[1:] + c for c in "ACGT" if x[1:] + c in owners]

    def pred(x):
        return [c + x[:-1] for c in "ACGT" if c + x[:-1] in owners]

    node = {x for x in owners if len(succ(x)) <= 1 and len(pred(x)) <= 1 and len(owners[x]) >= t}
    nxt, prv = {}, {}
    for u in node:
        s = succ(u)
        if len(s) == 1:
            v = s[0]
            if v != u and v in node and len(owners[u] & owners[v]) >= t:
                nxt[u], prv[v] = v, u
    paths, seen = [], set()

    def spell(first):
        out, x = [first], first
        seen.add(x)
        while x in nxt and nxt[x] not in seen:
            x = nxt[x]
            seen.add(x)
            out.append(x[-1])
        return "".join(out)

    for x in node:
        if x not in prv:
            paths.append(spell(x))
    rest = node - seen
    while rest:  # cycles: from the k-mer of smallest row
        cyc, x = [], next(iter(rest))
        while x not in cyc:
            cyc.append(x)
            x = nxt[x]
        first = min(cyc, key=lambda y: row_of[y])
        paths.append(spell(first))
        rest -= set(cyc)
    return sorted(paths, key=lambda p: row_of[p[:k]])


def _row_of(t):
    km, _ = t.extract()
    return {s: i for i, s in enumerate(S.packed_to_ascii(km, t.k))}


def _index(k, seed=0, length=6000, options=(), merges=False):
    t = BFT(k, device=0)
    for name, v in options:
        t.set_option(name, v)
    lists = []
    for gid, g in enumerate(_genomes(seed, length)):
        assert t.add_genome(f"g{gid}") == gid
        km = S.distinct(S.kmers_of(g, k))
        t.insert_kmers(km, gid)
        if merges:
            t.build()
        lists.append((S.packed_to_ascii(km, k), gid))
    return t, _owners_of(lists)


def _answers(t, owners, k):
    """presence, colour sets and rows of a sample of stored k-mers and absent mutants"""
    asc = sorted(owners)[::7]
    q, _ = S.ascii_to_packed(asc, k)
    q = np.concatenate([q, S.snp_mutants(q[:200], k, 5)])
    bits, off, ids = t.query_colors(q)
    _, rows, _ = t.query_rows(q)  # (colour-set ids are numbered per image: not compared)
    return bits.tobytes(), off.tobytes(), ids.tobytes(), rows.tobytes()


@pytest.mark.parametrize("k", KS)
def test_simple_paths_match_ground_truth(k):
    t, owners = _index(k, seed=k)
    row_of = _row_of(t)
    for thr in (0, 1, 2, N_GENOMES, N_GENOMES + 1):
        got = t.simple_paths(thr)
        want = _truth(owners, k, thr, row_of)
        assert got == want, (k, thr, len(got), len(want))
    assert t.simple_paths(N_GENOMES + 1) == []
    t.close()


@pytest.mark.parametrize("k", (9, 27, 36, 63))
def test_hand_made_graphs(k):
    rng = np.random.default_rng(100 + k)
    circ = "".join(rng.choice(list("ACGT"), 150))
    ring = circ + circ[:k - 1]
    cycle = [ring[i:i + k] for i in range(len(circ))]
    homo = "A" * k
    lone = "".join(rng.choice(list("ACGT"), k))
    # x with one predecessor and two successors: x is in no path, its predecessor and successors are paths of their own
    x = "".join(rng.choice(list("ACGT"), k))
    fork = [x, "G" + x[:-1], x[1:] + "C", x[1:] + "T"]
    genome0 = cycle + [homo, lone]
    t = BFT(k, device=0)
    t.add_genome("g0")
    t.add_genome("g1")
    t.insert_kmers(S.ascii_to_packed(genome0, k)[0], 0)
    t.insert_kmers(S.ascii_to_packed(fork, k)[0], 1)
    owners = _owners_of([(genome0, 0), (fork, 1)])
    row_of = _row_of(t)
    got = t.simple_paths()
    assert got == _truth(owners, k, 0, row_of)
    first = min(cycle, key=lambda y: row_of[y])
    i = cycle.index(first)
    assert (circ[i:] + circ[:i] + (circ[i:] + circ[:i])[:k - 1]) in got  # the cycle, rotated to its smallest row: m + k - 1 nucleotides
    assert homo in got and lone in got
    assert not any(x in p for p in got)
    for y in fork[1:]:
        assert y in got
    assert t.simple_paths(1) == _truth(owners, k, 1, row_of)
    assert t.simple_paths(2) == []
    t.close()


@pytest.mark.parametrize("state", ["compact0", "kmer_hash0", "pending", "merges", "file"])
@pytest.mark.parametrize("k", (27, 63))
def test_index_states_give_the_same_paths(state, k, tmp_path):
    ref, owners = _index(k, seed=7)
    want = {thr: ref.simple_paths(thr) for thr in (0, 2)}
    assert want[0] == _truth(owners, k, 0, _row_of(ref))
    before = _answers(ref, owners, k)
    opts = {"compact0": [("compact_table", 0)], "kmer_hash0": [("kmer_hash", 0)]}.get(state, [])
    if state == "file":
        path = str(tmp_path / "i.bft")
        ref.write_bft(path)
        t = BFT.load_bft(path)
    elif state == "pending":
        t, _ = _index(k, seed=7)
        t.simple_paths()
        extra = S.distinct(S.kmers_of(S.random_genome(800, 99), k))
        t.insert_kmers(extra, 0)  # (pending: built by the next call)
        asc = S.packed_to_ascii(extra, k)
        owners2 = {key: set(v) for key, v in owners.items()}
        for s in asc:
            owners2.setdefault(s, set()).add(0)
        got = t.simple_paths()
        assert got == _truth(owners2, k, 0, _row_of(t))
        t.close()
        ref.close()
        return
    else:
        t, _ = _index(k, seed=7, options=opts, merges=state == "merges")
    for thr in (0, 2):
        assert t.simple_paths(thr) == want[thr]
    assert _answers(t, owners, k) == before
    t.close()
    ref.close()


def test_answers_unchanged_and_table_returns():
    k = 31
    t, owners = _index(k, seed=3)
    before = _answers(t, owners, k)
    km0, cs0 = t.extract()
    t.simple_paths(1)
    assert _answers(t, owners, k) == before
    km1, cs1 = t.extract()
    assert (km0 == km1).all() and (cs0 == cs1).all()
    t.close()


def test_caps_and_nospace():
    k = 27
    t, owners = _index(k, seed=11)
    lib = _lib.load()
    npaths, nchars = C.c_uint64(), C.c_uint64()
    assert lib.bft_gpu_simple_paths(t._h, 0, None, None, 0, 0, C.byref(npaths), C.byref(nchars)) == 0
    P, N = npaths.value, nchars.value
    want = t.simple_paths()
    assert P == len(want) and N == sum(map(len, want))
    off = np.full(P + 1, 7, dtype=np.uint64)
    seq = np.full(N, 7, dtype=np.uint8)
    assert lib.bft_gpu_simple_paths(t._h, 0, off.ctypes.data, seq.ctypes.data, P - 1, N, C.byref(npaths), C.byref(nchars)) == -6
    assert (npaths.value, nchars.value) == (P, N) and (off == 7).all() and (seq == 7).all()
    assert lib.bft_gpu_simple_paths(t._h, 0, off.ctypes.data, seq.ctypes.data, P, N - 1, C.byref(npaths), C.byref(nchars)) == -6
    assert (off == 7).all() and (seq == 7).all()
    assert lib.bft_gpu_simple_paths(t._h, 0, off.ctypes.data, None, P, 0, C.byref(npaths), C.byref(nchars)) == 0
    assert off[0] == 0 and off[-1] == N and (np.diff(off.astype(np.int64)) >= k).all()
    assert lib.bft_gpu_simple_paths(t._h, 0, off.ctypes.data, seq.ctypes.data, P, N, C.byref(npaths), C.byref(nchars)) == 0
    text = seq.tobytes().decode()
    assert [text[int(off[i]):int(off[i + 1])] for i in range(P)] == want
    assert lib.bft_gpu_simple_paths(t._h, 0, None, None, 0, 0, None, C.byref(nchars)) == -1
    t.close()


def test_dev_form_on_a_user_stream_interleaved_with_queries():
    import torch
    k = 36
    t, owners = _index(k, seed=5)
    want = t.simple_paths()
    want2 = t.simple_paths(2)
    P, N = len(want), sum(map(len, want))
    asc = sorted(owners)[::5]
    q, _ = S.ascii_to_packed(asc, k)
    n = len(q)
    bits_h, off_h, ids_h = t.query_colors(q)
    pref = q[:64].copy()
    po, pk, pr, pc = t.query_prefixes(pref, np.full(64, 20, dtype=np.uint8))
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        dq = torch.from_numpy(q.reshape(-1).copy()).cuda()
        dbits = torch.zeros((n + 63) // 64, dtype=torch.int64, device="cuda")
        doffc = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        dids = torch.zeros(len(ids_h) + 1, dtype=torch.int32, device="cuda")
        dp = torch.from_numpy(pref.reshape(-1).copy()).cuda()
        dl = torch.full((64,), 20, dtype=torch.uint8, device="cuda")
        dpo = torch.zeros(65, dtype=torch.int64, device="cuda")
        cnt = torch.full((3,), 7, dtype=torch.int64, device="cuda")
        t.simple_paths_dev(0, 0, 0, 0, cnt.data_ptr(), stream=s.cuda_stream)  # sizing
    s.synchronize()
    c = cnt.cpu().tolist()
    assert c == [P, N, max(map(len, want))]
    with torch.cuda.stream(s):
        doff = torch.full((P + 1,), 7, dtype=torch.int64, device="cuda")
        dseq = torch.full((N,), 7, dtype=torch.uint8, device="cuda")
        half = torch.full((N // 2,), 7, dtype=torch.uint8, device="cuda")
        t.query_colors_dev(dq.data_ptr(), n, dbits.data_ptr(), doffc.data_ptr(), dids.data_ptr(), len(ids_h) + 1, stream=s.cuda_stream)
        t.simple_paths_dev(doff.data_ptr(), dseq.data_ptr(), P, N, cnt.data_ptr(), stream=s.cuda_stream)
        t.query_prefixes_dev(dp.data_ptr(), dl.data_ptr(), 64, dpo.data_ptr(), 0, 0, 0, 0, 0, stream=s.cuda_stream)
        cnt2 = torch.zeros(3, dtype=torch.int64, device="cuda")
        t.simple_paths_dev(0, half.data_ptr(), 0, N // 2, cnt2.data_ptr(), min_shared=0, stream=s.cuda_stream)
        cnt3 = torch.zeros(3, dtype=torch.int64, device="cuda")
        t.simple_paths_dev(0, 0, 0, 0, cnt3.data_ptr(), min_shared=2, stream=s.cuda_stream)
    s.synchronize()
    off = doff.cpu().numpy()
    text = dseq.cpu().numpy().tobytes().decode()
    assert [text[int(off[i]):int(off[i + 1])] for i in range(P)] == want
    assert half.cpu().numpy().tobytes().decode() == "".join(want)[:N // 2]
    assert cnt2.cpu().tolist() == [P, N, max(map(len, want))]
    assert cnt3.cpu().tolist()[:2] == [len(want2), sum(map(len, want2))]
    assert (dbits.cpu().numpy().view(np.uint8)[:len(bits_h)] == bits_h).all()
    assert (doffc.cpu().numpy().astype(np.uint64) == off_h).all()
    assert (dids.cpu().numpy()[:len(ids_h)].astype(np.uint32) == ids_h).all()
    assert (dpo.cpu().numpy().astype(np.uint64) == po).all()


def test_empty_index_and_kernel_time():
    t = BFT(27, device=0)
    assert t.simple_paths() == []
    t2, _ = _index(27, seed=2)
    t2.kernel_time(reset=True)
    t2.simple_paths()
    ms, launches = t2.kernel_time(reset=True)
    assert launches >= 8 and ms > 0
    t.close()
    t2.close()
