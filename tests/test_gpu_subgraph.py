"""Sub-graphs on the GPU (bft_gpu_subgraph / _dev, BFT.subgraph): the stored subset of a shuffled batch with duplicates and absent mutants,
against ground truth -- numpy / Python sets over the inserted k-mers, not the product's own extract -- at key widths W = 1, 2 and 4 (KS has no three-word key, k = 65..96; tests/test_gpu_graph_edges.py runs W = 3 and the other key shapes); the same
image as a fresh build of the subset; the k-mer hash against its host restatement; the colour-less form; source states (compact_table,
kmer_hash 0, pending insertions, merges) left unchanged; empty and all-absent batches; a sub-graph that outlives its source, takes
insertions, merges and .bft round trips; prefix matches fed to subgraph_dev on one stream; kernel timing."""
import ctypes as C
import os

import numpy as np
import pytest

from bloomfiltertrie_amd import BFT, _lib, synth as S

pytestmark = pytest.mark.gpu

KS = (9, 18, 27, 31, 36, 63, 64, 126)
N_GENOMES = 4
# (restated from tests/test_gpu_build.py: the container image of an index)
ARRAYS = ["tk", "nodes", "bfT", "ccs", "f2w", "clus", "child", "uck", "ucrow", "ccx", "f18", "fent"]


def _random_kmers(n, k, seed):
    return S.pack_codes(np.random.default_rng(seed).integers(0, 4, (n, k), dtype=np.uint8))


def _genomes(seed, length):
    anc = S.random_genome(length, seed + 1)
    return [anc] + [S.mutate(anc, 0.02, seed + 2 + g) for g in range(N_GENOMES - 1)]


def _index(k, seed=0, length=20000, options=(), merges=False):
    """An index of N_GENOMES related genomes with names, and the ground truth {row key: sorted genome ids}.  merges: built after every genome."""
    t = BFT(k, device=0)
    for name, v in options:
        t.set_option(name, v)
    owners, per_genome = {}, []
    for gid, g in enumerate(_genomes(seed, length)):
        assert t.add_genome(f"g{gid}") == gid
        km = S.distinct(S.kmers_of(g, k))
        per_genome.append(km)
        t.insert_kmers(km, gid)
        if merges:
            t.build()
        for key in S.row_keys(km).tolist():
            owners.setdefault(key, []).append(gid)
    allk = S.distinct(np.concatenate(per_genome))
    return t, allk, owners, per_genome


def _batch(allk, k, rng, frac=0.4):
    """A shuffled batch: about frac of the stored k-mers, a third of them again, and SNP mutants that are not stored."""
    pick = allk[rng.random(len(allk)) < frac]
    dups = pick[rng.integers(0, len(pick), len(pick) // 3)]
    mut = S.snp_mutants(pick[: len(pick) // 2], k, int(rng.integers(1 << 30)))
    mut = mut[~S.member(mut, allk)]
    q = np.concatenate([pick, dups, mut])
    return q[rng.permutation(len(q))], pick, len(mut)


def _colour_map(t):
    """{row key: tuple of genome ids} of everything t stores (extract + colorset)."""
    km, cs = t.extract()
    sets = {c: tuple(int(x) for x in t.colorset(c)) for c in np.unique(cs).tolist()}
    return dict(zip(S.row_keys(km).tolist(), (sets[c] for c in cs.tolist())))


def _arrays(t):
    return {name: t.debug_array(name) for name in ARRAYS}


def _check_subgraph(t, sub, n_absent, subset, owners, n_mut, k, colors=True):
    want = {key: tuple(owners[key]) for key in S.row_keys(subset).tolist()}
    assert n_absent == n_mut
    km, _ = sub.extract()
    assert sorted(S.row_keys(km).tolist()) == sorted(want)
    cmap = _colour_map(sub)
    if colors:
        assert cmap == want
    else:
        assert set(cmap.values()) <= {(0,)} and set(cmap) == set(want)
    info = sub.info()
    assert info["kmers"] == len(want)
    assert info["pairs"] == (sum(len(v) for v in want.values()) if colors else len(want))
    assert info["colorsets"] == (len(set(want.values())) if colors else min(1, len(want)))
    assert info["genomes"] == (N_GENOMES if colors else 1)
    for g in range(info["genomes"]):
        assert sub.genome_name(g) == t.genome_name(g)


def _same_answers(t, sub, subset, k, rng):
    """Presence over a mix of kept, dropped and absent k-mers; colour lists of every kept k-mer as the source's."""
    allk, _ = t.extract()
    mix = np.concatenate([subset, allk[rng.integers(0, len(allk), 2000)], S.snp_mutants(subset[:2000], k, 7)])
    assert (S.from_bits(sub.query_presence(mix), len(mix)) == S.member(mix, subset)).all()
    b1, o1, i1 = t.query_colors(subset)
    b2, o2, i2 = sub.query_colors(subset)
    assert (b1 == b2).all() and (o1 == o2).all() and (i1 == i2).all()


@pytest.mark.parametrize("k", KS)
def test_subgraph_against_ground_truth(k):
    rng = np.random.default_rng(k)
    t, allk, owners, _ = _index(k, seed=k)
    q, pick, n_mut = _batch(allk, k, rng)
    sub, n_absent = t.subgraph(q)
    _check_subgraph(t, sub, n_absent, pick, owners, n_mut, k)
    _same_answers(t, sub, pick, k, rng)


@pytest.mark.parametrize("k", (27, 31, 63, 126))
def test_subgraph_is_the_fresh_build_of_the_subset(k):
    """The sub-graph's container image is bit-identical to that of a handle with the source's seeds and names into which the subset's k-mers
    of each genome were inserted; colour maps equal.  And the sub-graph of every stored k-mer is the source's own image."""
    rng = np.random.default_rng(100 + k)
    t, allk, owners, per_genome = _index(k, seed=k + 1)
    q, pick, _ = _batch(allk, k, rng, frac=0.3)
    sub, _ = t.subgraph(q)
    info = t.info()
    fresh = BFT(k, r1=0, r2=0)
    for g in range(N_GENOMES):
        fresh.add_genome(t.genome_name(g))
        fresh.insert_kmers(per_genome[g][S.member(per_genome[g], pick)], g)
    fresh.build()
    a, b = _arrays(sub), _arrays(fresh)
    for name in ARRAYS:
        assert a[name].shape == b[name].shape and (a[name] == b[name]).all(), name
    assert _colour_map(sub) == _colour_map(fresh)
    whole, n_absent = t.subgraph(allk[rng.permutation(len(allk))])
    assert n_absent == 0
    a, b = _arrays(whole), _arrays(t)
    for name in ARRAYS:
        assert (a[name] == b[name]).all(), name
    assert _colour_map(whole) == _colour_map(t)
    assert whole.info()["colorsets"] == info["colorsets"] and whole.info()["pairs"] == info["pairs"]


@pytest.mark.parametrize("k", (31, 63))
def test_subgraph_kmer_hash_is_canonical(k):
    """The sub-graph's k-mer hash holds its table, nothing else, line for line as the host restatement lays it out."""
    hostlib = C.CDLL(os.path.join(_lib.CSRC, "libbft_hosttest.so"))
    hostlib.bft_hosttest_kh_verify.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p,
                                               C.c_void_p, C.c_uint32]
    W = (2 * k + 63) // 64
    rng = np.random.default_rng(k)
    t, allk, _, _ = _index(k, seed=3, length=60000)
    q, _, _ = _batch(allk, k, rng, frac=0.5)
    sub, _ = t.subgraph(q)
    sub.set_option("compact_table", 0)
    kh = np.ascontiguousarray(sub.debug_array("kh", np.uint64))
    tk = np.ascontiguousarray(sub.debug_array("tk", np.uint64).reshape(-1, W))
    tcol = np.ascontiguousarray(sub.debug_array("tcol", np.uint32))
    ovk = np.ascontiguousarray(sub.debug_array("kh_ovf_k", np.uint64))
    ovv = np.ascontiguousarray(sub.debug_array("kh_ovf_v", np.uint32))
    bt = sub.build_time()
    assert int(bt["kmer_hash_lines"]) > 0
    rc = hostlib.bft_hosttest_kh_verify(tk.ctypes.data, tcol.ctypes.data, len(tk), k, sub.info()["colorsets"], 55, int(bt["kmer_hash_maxd"]), kh.ctypes.data,
                                        len(kh) // 8, ovk.ctypes.data, ovv.ctypes.data, int(bt["kmer_hash_overflow"]))
    assert rc == 1, rc


@pytest.mark.parametrize("k", (27, 64))
def test_colourless_form(k):
    rng = np.random.default_rng(k + 5)
    t, allk, owners, _ = _index(k, seed=k + 2)
    q, pick, n_mut = _batch(allk, k, rng)
    sub, n_absent = t.subgraph(q, colors=False)
    _check_subgraph(t, sub, n_absent, pick, owners, n_mut, k, colors=False)
    assert sub.genome_name(0) == "g0"
    _, o, ids = sub.query_colors(pick)
    assert (np.diff(o.astype(np.int64)) == 1).all() and (ids == 0).all()


@pytest.mark.parametrize("state", ["compact0", "compact1", "kmer_hash0", "pending", "merges"])
def test_source_states(state):
    """Whatever state the source is in, the sub-graph is right and the source's image and colour map are what they were (pending insertions:
    what the source's own build of them gives)."""
    k = 31
    rng = np.random.default_rng(len(state))
    opts = {"compact0": [("compact_table", 0)], "compact1": [("compact_table", 1)], "kmer_hash0": [("kmer_hash", 0)]}.get(state, [])
    t, allk, owners, _ = _index(k, seed=11, options=opts, merges=state == "merges")
    if state == "pending":
        t.build()
        extra = _random_kmers(3000, k, 99)
        t.insert_kmers(extra, 1)
        assert t.info()["pending_pairs"] > 0
        for key in S.row_keys(extra).tolist():
            owners[key] = sorted(set(owners.get(key, [])) | {1})
        allk = S.distinct(np.concatenate([allk, extra]))
        q, pick, n_mut = _batch(allk, k, rng)
        sub, n_absent = t.subgraph(q)
        assert t.info()["pending_pairs"] == 0
        before_arrays, before_map = _arrays(t), _colour_map(t)
    else:
        before_arrays, before_map = _arrays(t), _colour_map(t)
        q, pick, n_mut = _batch(allk, k, rng)
        sub, n_absent = t.subgraph(q)
    _check_subgraph(t, sub, n_absent, pick, owners, n_mut, k)
    _same_answers(t, sub, pick, k, rng)
    after = _arrays(t)
    for name in ARRAYS:
        assert (after[name] == before_arrays[name]).all(), name
    assert _colour_map(t) == before_map == {key: tuple(v) for key, v in owners.items()}


def test_edge_cases(tmp_path):
    k = 27
    rng = np.random.default_rng(1)
    t, allk, owners, _ = _index(k, seed=5)
    for q in (np.zeros((0, S.kmer_bytes(k)), np.uint8), S.snp_mutants(allk[:500], k, 3)):
        q = q[~S.member(q, allk)]
        sub, n_absent = t.subgraph(q)
        assert n_absent == len(q) and sub.info()["kmers"] == 0
        assert not S.from_bits(sub.query_presence(allk[:1000]), 1000).any()
        sub.close()
    q, pick, _ = _batch(allk, k, rng)
    sub, _ = t.subgraph(q)
    t.close()  # (the sub-graph shares nothing with its source)
    want = {key: tuple(owners[key]) for key in S.row_keys(pick).tolist()}
    assert _colour_map(sub) == want
    more = _random_kmers(2000, k, 8)
    sub.insert_kmers(more, 3)
    sub.build()
    sub.insert_kmers(pick[:100], 1)
    for key in S.row_keys(more).tolist():
        want[key] = tuple(sorted(set(want.get(key, ())) | {3}))
    for key in S.row_keys(pick[:100]).tolist():
        want[key] = tuple(sorted(set(want[key]) | {1}))
    assert _colour_map(sub) == want
    path = str(tmp_path / "sub.bft")
    sub.write_bft(path)
    back = BFT.load_bft(path)
    assert _colour_map(back) == want
    mix = np.concatenate([pick, more, S.snp_mutants(pick[:500], k, 4)])
    assert (back.query_presence(mix) == sub.query_presence(mix)).all()


@pytest.mark.parametrize("k", (18, 36))
def test_prefix_matches_to_subgraph_dev(k):
    """query_prefixes_dev -> subgraph_dev on one stream, the k-mers never copied to the host: exactly the prefix's matches, with their colour
    sets; the host call on the same k-mers gives the same sub-graph."""
    import torch
    rng = np.random.default_rng(k)
    t, allk, owners, _ = _index(k, seed=21)
    nb = S.kmer_bytes(k)
    pref = allk[:1].copy()
    codes = S.unpack_codes(allk, k)
    want = allk[codes[:, 0] == S.unpack_codes(pref, k)[0, 0]]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        dp = torch.from_numpy(pref.reshape(-1).copy()).cuda()
        dl = torch.ones(1, dtype=torch.uint8, device="cuda")
        doff = torch.zeros(2, dtype=torch.int64, device="cuda")
        t.query_prefixes_dev(dp.data_ptr(), dl.data_ptr(), 1, doff.data_ptr(), 0, 0, 0, 0, 0, stream=s.cuda_stream)
    s.synchronize()
    m = int(doff[1].item())  # (the count: sizes the buffer)
    assert m == len(want)
    with torch.cuda.stream(s):
        dk = torch.full((m * nb,), 0xAB, dtype=torch.uint8, device="cuda")
        t.query_prefixes_dev(dp.data_ptr(), dl.data_ptr(), 1, doff.data_ptr(), dk.data_ptr(), 0, 0, m, 0, stream=s.cuda_stream)
        sub, n_absent = t.subgraph_dev(dk.data_ptr(), m, stream=s.cuda_stream)
    s.synchronize()
    assert n_absent == 0
    truth = {key: tuple(owners[key]) for key in S.row_keys(want).tolist()}
    assert _colour_map(sub) == truth
    hsub, n_absent = t.subgraph(want[rng.permutation(len(want))])
    assert n_absent == 0 and _colour_map(hsub) == truth
    a, b = _arrays(sub), _arrays(hsub)
    for name in ARRAYS:
        assert (a[name] == b[name]).all(), name


def test_kernel_timing_counts_the_new_launches():
    k = 31
    t, allk, _, _ = _index(k, seed=2)
    t.build()
    t.kernel_time(reset=True)
    t.kernel_time(reset=True)
    sub, _ = t.subgraph(allk[::3])
    ms, n = t.kernel_time(reset=True)
    assert n >= 6 and ms > 0  # lookup, compaction, sort, scan, scatter, dictionary launches
    t.set_option("build_stages", 1)
    sub, _ = t.subgraph(allk[::3])
    names = [st[0] for st in sub.build_stages()]
    assert any(nm.startswith("sub-graph: lookup") for nm in names) and any(nm.startswith("containers") for nm in names), names
