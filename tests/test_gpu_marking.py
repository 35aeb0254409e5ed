"""Vertex marking on the GPU (bft_gpu_marks_*, BFT.set_marking .. BFT.reach) against plain-Python ground truth (test_marking_host.MarkModel: a dict
from k-mer to flag, the adjacency of the inserted k-mers, a literal model of the reference's BFS / BFS_subgraph loops): the packed layout and the
atomicity of batched sets at every key width and at sizes around the 16 rows of a flag word; test-and-set with every k-mer repeated 64 times;
reach on hand-made graphs, with barriers, several seeds and other flag values; sub-graphs with the boundary rows of BFS_subgraph; the number of
launches (independent of the data; fewer with the cached forest); the state rules; the device forms on a caller's stream."""
import ctypes as C

import numpy as np
import pytest

from bloomfiltertrie_amd import BFT, _lib, synth as S

from test_gpu_components import _owners_of, _row_of
from test_marking_host import MarkModel

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -4


def _rand_index(k, n, seed):
    """An index of exactly n random k-mers in one genome; (handle, packed k-mers in row order)."""
    km = S.distinct(S.pack_codes(np.random.default_rng(seed).integers(0, 4, size=(n + 8, k), dtype=np.uint8)))[:n]
    assert len(km) == n
    t = BFT(k, device=0)
    t.insert_kmers(km, 0)
    rows, _ = t.extract()
    return t, rows


def _unpack(packed, n):
    b = np.asarray(packed, dtype=np.uint8)
    return np.stack([(b >> s) & 3 for s in (0, 2, 4, 6)], axis=1).reshape(-1)[:n]


@pytest.mark.parametrize("k", (9, 27, 31, 63, 99, 126))
def test_packing_and_atomic_sets(k):
    """Per-k-mer flags row % 4 written by ONE shuffled batch: the 16 rows of a word are written by different lanes, and all must land."""
    for n in (1, 15, 16, 17, 33, 1000):
        t, rows = _rand_index(k, n, 1000 * k + n)
        t.set_marking()
        assert t.read_flags().tolist() == [0] * ((n + 3) // 4)
        want = (np.arange(n) % 4).astype(np.uint8)
        perm = np.random.default_rng(n).permutation(n)
        assert t.set_flags(rows[perm], want[perm]) == 0
        assert (t.get_flags(rows) == want).all()
        packed = t.read_flags()
        assert len(packed) == (n + 3) // 4 and (_unpack(packed, n) == want).all()
        if n % 4:
            assert packed[-1] >> (2 * (n % 4)) == 0  # (the bits behind the last row)
        counts = t.flag_counts()
        assert counts.tolist() == [int((want == f).sum()) for f in range(4)]
        for mask in range(1, 16):
            km, r = t.select_flagged(mask)
            sel = np.nonzero((mask >> want) & 1)[0]
            assert r.tolist() == sel.tolist() and (km == rows[sel]).all(), (n, mask)
        asc, r = t.select_flagged(0b0100, ascii=True)
        assert asc == S.packed_to_ascii(rows[want == 2], k)
        # the array out and in again
        t.fill_flags(3)
        assert t.flag_counts().tolist() == [0, 0, 0, n]
        t.write_flags(packed)
        assert (t.get_flags(rows) == want).all()
        t.close()


def test_one_flag_for_a_batch_with_repeats_and_absent_kmers():
    k = 27
    t, rows = _rand_index(k, 40, 5)
    t.set_marking()
    rng = np.random.default_rng(6)
    before = (np.arange(40) % 3).astype(np.uint8)
    t.set_flags(rows, before)
    named = rng.integers(0, 40, size=4096)
    named = named[named % 5 != 0]  # (rows 0, 5, 10 .. are never named)
    absent = S.pack_codes(rng.integers(0, 4, size=(7, k), dtype=np.uint8))
    assert not S.member(absent, rows).any()
    batch = np.concatenate([rows[named], absent])
    batch = batch[rng.permutation(len(batch))]
    assert t.set_flags(batch, 3) == 7
    want = before.copy()
    want[np.unique(named)] = 3
    assert (t.get_flags(rows) == want).all()
    got = t.get_flags(np.concatenate([absent, rows[:3]]))
    assert got.tolist() == [0xFF] * 7 + want[:3].tolist()
    n_abs = C.c_uint64()
    out = np.zeros(len(batch), dtype=np.uint8)
    _lib.check(_lib.load().bft_gpu_marks_get(t._h, batch.ctypes.data, len(batch), out.ctypes.data, C.byref(n_abs)))
    assert n_abs.value == 7 and int((out == 0xFF).sum()) == 7
    # every single flag value, over what the batch before left
    for f in (0, 1, 2, 3):
        t.set_flags(rows[named], f)
        want[np.unique(named)] = f
        assert (t.get_flags(rows) == want).all(), f
    t.close()


def test_test_and_set_has_one_winner_per_kmer():
    k = 31
    n, rep = 300, 64
    t, rows = _rand_index(k, n, 9)
    t.set_marking()
    before = (np.arange(n) % 3 == 0).astype(np.uint8) * 2  # every third row holds 2, the others 0
    t.set_flags(rows, before)
    idx = np.repeat(np.arange(n), rep)
    idx = idx[np.random.default_rng(10).permutation(len(idx))]
    won = t.test_and_set(rows[idx], 0, 1)
    winners = np.bincount(idx, weights=won, minlength=n).astype(int)
    assert winners.tolist() == [0 if before[r] else 1 for r in range(n)]
    assert set(won.tolist()) <= {0, 1} and int(won.sum()) == int((before == 0).sum())
    want = np.where(before == 0, 1, before)
    assert (t.get_flags(rows) == want).all()
    assert int(t.test_and_set(rows[idx], 0, 1).sum()) == 0  # (nothing holds 0 any more)
    assert (t.get_flags(rows) == want).all()
    t.close()


def _hand_made(k):
    """Two disjoint chains, a cycle, a chain with a branch, a homopolymer (its own neighbour) and a lone k-mer, all in genome 0.
    Returns (handle, model, row_of, named k-mers)."""
    rng = np.random.default_rng(100 + k)

    def seq(n):
        return rng.integers(0, 4, size=n, dtype=np.uint8)

    chain1, chain2, circle, trunk, lone = seq(k + 59), seq(k + 39), seq(50), seq(k + 79), seq(k)
    circle = np.resize(circle, 50 + k - 1)  # (50 k-mers that close on themselves; the period is shorter than k at k = 63)
    twig = np.concatenate([trunk[30:30 + k - 1], seq(25)])  # leaves the trunk behind its k-mer 29
    homo = np.zeros(k, dtype=np.uint8)
    parts = {"chain1": chain1, "chain2": chain2, "circle": circle, "trunk": trunk, "twig": twig, "homo": homo, "lone": lone}
    asc = {name: S.packed_to_ascii(S.kmers_of(g, k), k) for name, g in parts.items()}
    every = sorted({x for lst in asc.values() for x in lst})
    t = BFT(k, device=0)
    t.insert_kmers(S.ascii_to_packed(every, k)[0], 0)
    model = MarkModel({x: {0} for x in every})
    return t, model, _row_of(t), asc


def _same(t, model, row_of):
    assert t.read_flags().tolist() == model.packed(row_of).tolist()


def _reach(t, model, row_of, seeds, **kw):
    got_new, got_counts = t.reach(S.ascii_to_packed(seeds, t.k)[0], **kw)
    want_new, want_counts = model.reach(seeds, **{("ids" if a == "genome_ids" else a): v for a, v in kw.items()})
    assert got_new.tolist() == want_new, (seeds, kw)
    assert got_counts.tolist() == want_counts, (seeds, kw)
    _same(t, model, row_of)
    return got_new, got_counts


@pytest.mark.parametrize("k", (27, 63))
def test_reach_on_hand_made_graphs(k):
    t, model, row_of, asc = _hand_made(k)
    t.set_marking()
    absent = "ACGT" * 40
    absent = absent[:k]
    assert absent not in row_of
    # one component at a time, the whole flag array compared after every call
    new, cnt = _reach(t, model, row_of, [asc["chain1"][7]])
    assert new.tolist() == [1] and cnt.tolist() == [len(asc["chain1"]), 0, 0]
    _reach(t, model, row_of, [asc["chain1"][0]])           # already painted: nothing new
    new, cnt = _reach(t, model, row_of, [asc["circle"][3]])
    assert cnt[0] == 50
    # the branch: the twig is reached from the trunk
    new, cnt = _reach(t, model, row_of, [asc["twig"][-1]])
    assert cnt[0] == len(set(asc["trunk"]) | set(asc["twig"]))
    # three seeds of one component, an absent one, the homopolymer and the lone k-mer
    new, cnt = _reach(t, model, row_of, [asc["chain2"][5], absent, asc["chain2"][0], asc["chain2"][-1], asc["homo"][0], asc["lone"][0]])
    assert new.tolist() == [1, 0, 0, 0, 1, 1] and cnt.tolist() == [len(asc["chain2"]) + 2, 0, 1]
    assert t.flag_counts().tolist() == [0, len(row_of), 0, 0]
    # barriers: flag 2 on two inner k-mers of chain1; from one end the walk (through 1, to 3) stops there and the far side stays 1
    bar = [asc["chain1"][20], asc["chain1"][40]]
    t.set_flags(S.ascii_to_packed(bar, k)[0], 2)
    for x in bar:
        model.flag[x] = 2
    new, cnt = _reach(t, model, row_of, [asc["chain1"][0]], through=1, to=3)
    assert cnt.tolist() == [20, 0, 0]
    assert model.flag[asc["chain1"][19]] == 3 and model.flag[asc["chain1"][21]] == 1 and model.flag[asc["chain1"][41]] == 1
    # through the barrier's own value, then back to 0 over everything that holds 3
    _reach(t, model, row_of, bar, through=2, to=0)
    _reach(t, model, row_of, [asc["chain1"][5], asc["chain1"][30]], through=3, to=0)
    # boundary = 1 without ids is BFS: nothing outside the component is touched
    _reach(t, model, row_of, [asc["chain1"][50]], through=1, to=2, boundary=True)
    t.close()


def _three_genomes(k=27):
    """An ancestor, a mutant and a mosaic, as tests/test_ref_api_components.py builds them."""
    anc = S.random_genome(700, 51)
    mut = S.mutate(anc, 0.03, 52)
    third = S.random_genome(400, 53)
    third[:120] = anc[200:320]
    third[120:220] = anc[400:500]
    t = BFT(k, device=0)
    lists = []
    for gid, g in enumerate((anc, mut, third)):
        km = S.distinct(S.kmers_of(g, k))
        t.insert_kmers(km, gid)
        lists.append((S.packed_to_ascii(km, k), gid))
    return t, _owners_of(lists)


@pytest.mark.parametrize("ids", ((0,), (0, 1), (1, 2)))
def test_subgraph_reach_is_bfs_subgraph_seed_by_seed(ids):
    t, owners = _three_genomes()
    row_of = _row_of(t)
    order = sorted(row_of, key=row_of.get)
    n_comp = int(len(t.components(ids)[1]))
    t.set_marking()
    # seed by seed in row order, as nb_connected_components does: the flags are the model's after EVERY call
    model = MarkModel(owners)
    total = 0
    for x in order:
        if model.flag[x] != 0:
            continue  # (the callback returns before any GPU work; the reach itself is checked on visited seeds below)
        new, _ = _reach(t, model, row_of, [x], genome_ids=ids, boundary=True)
        total += int(new[0])
    assert total == n_comp
    assert _reach(t, model, row_of, order[:50], genome_ids=ids, boundary=True)[0].sum() == 0
    # all seeds in one call: same flags, and seed_new sums to the number of components
    t.fill_flags(0)
    model = MarkModel(owners)
    new, cnt = _reach(t, model, row_of, order, genome_ids=ids, boundary=True)
    assert int(new.sum()) == n_comp and cnt[2] == 0
    # boundary = 0: the members alone
    t.fill_flags(0)
    model = MarkModel(owners)
    new, cnt = _reach(t, model, row_of, order, genome_ids=ids, boundary=False)
    assert int(new.sum()) == n_comp and cnt[1] == 0 and cnt[0] == sum(1 for x in owners if set(ids) <= owners[x])
    t.close()


def test_subgraph_reach_with_more_ids_than_one_membership_launch():
    k = 27
    anc = S.random_genome(600, 61)
    t = BFT(k, device=0)
    lists = []
    for gid in range(80):
        km = S.distinct(S.kmers_of(S.mutate(anc, 0.002, 700 + gid), k))
        t.insert_kmers(km, gid)
        lists.append((S.packed_to_ascii(km, k), gid))
    owners = _owners_of(lists)
    row_of = _row_of(t)
    order = sorted(row_of, key=row_of.get)
    ids = tuple(range(70))
    assert 0 < sum(1 for x in owners if set(ids) <= owners[x]) < len(owners)
    n_comp = int(len(t.components(ids)[1]))
    t.set_marking()
    model = MarkModel(owners)
    new, _ = _reach(t, model, row_of, order, genome_ids=ids, boundary=True)
    assert int(new.sum()) == n_comp
    t.close()


def _launches(t, fn):
    t.kernel_time(reset=True)
    out = fn()
    return t.kernel_time(reset=True)[1], out


def test_launches_do_not_depend_on_the_data_and_the_forest_is_cached():
    k = 27
    small, rows_small = _rand_index(k, 40, 5)
    small.set_marking()
    n_small, _ = _launches(small, lambda: small.reach(rows_small[:1]))
    small.close()
    genome = S.random_genome(200_000, 77)
    km = S.kmers_of(genome, k)
    t = BFT(k, device=0)
    t.insert_kmers(km, 0)
    t.set_marking()  # (builds what is pending)
    n = t.info()["kmers"]
    mid = km[100_000:100_001]
    first, (new, cnt) = _launches(t, lambda: t.reach(mid))
    assert first == n_small and first > 0
    assert new.tolist() == [1] and cnt.tolist() == [n, 0, 0]  # (one chain -- 2 x 10^5 levels for a frontier -- painted in that many launches)
    assert t.flag_counts().tolist() == [0, n, 0, 0]
    second, (new, cnt) = _launches(t, lambda: t.reach(mid))
    assert second < first and new.tolist() == [0] and cnt.tolist() == [0, 0, 0]
    assert t.flag_counts().tolist() == [0, n, 0, 0]
    # a set in between drops the forest: the first count again, and the k-mers given back to 0 are found again
    t.set_flags(km[:1000], 0)
    third, (new, cnt) = _launches(t, lambda: t.reach(km[5:6]))
    n_back = len(S.distinct(km[:1000]))
    assert third == first and new.tolist() == [1] and cnt.tolist() == [n_back, 0, 0]
    assert t.flag_counts().tolist() == [0, n, 0, 0]
    t.close()


def test_state_rules():
    k = 27
    lib = _lib.load()
    t, rows = _rand_index(k, 100, 21)
    n = len(rows)
    buf = np.zeros(n, dtype=np.uint8)
    cnt = np.zeros(4, dtype=np.uint64)
    nb = C.c_uint64()
    # not marking: every marks call is E_STATE
    assert lib.bft_gpu_marks_set(t._h, rows.ctypes.data, n, None, 1, None) == E_STATE
    assert lib.bft_gpu_marks_get(t._h, rows.ctypes.data, n, buf.ctypes.data, None) == E_STATE
    assert lib.bft_gpu_marks_test_and_set(t._h, rows.ctypes.data, n, 0, 1, buf.ctypes.data, None) == E_STATE
    assert lib.bft_gpu_marks_fill(t._h, 1) == E_STATE
    assert lib.bft_gpu_marks_counts(t._h, cnt.ctypes.data) == E_STATE
    assert lib.bft_gpu_marks_select(t._h, 1, None, None, None, 0, C.byref(nb)) == E_STATE
    assert lib.bft_gpu_marks_reach(t._h, rows.ctypes.data, 1, None, 0, 0, 1, 0, buf.ctypes.data, cnt.ctypes.data) == E_STATE
    assert lib.bft_gpu_marks_read(t._h, None, 0, C.byref(nb)) == E_STATE
    assert lib.bft_gpu_marks_write(t._h, buf.ctypes.data, (n + 3) // 4) == E_STATE
    assert lib.bft_gpu_marks_end(t._h) == 0  # (unset_marking on a graph that is not marking changes nothing)
    t.set_marking()
    presence = t.query_presence(rows).copy()
    comps = t.components()[1].tolist()
    # locked: insert, build and add_genome are E_STATE, and the answers stay
    other = S.pack_codes(np.random.default_rng(3).integers(0, 4, size=(5, k), dtype=np.uint8))
    assert lib.bft_gpu_insert_kmers(t._h, other.ctypes.data, 5, 0) == E_STATE
    assert lib.bft_gpu_build(t._h) == E_STATE
    assert lib.bft_gpu_add_genome(t._h, b"late", None) == E_STATE
    assert t.info()["kmers"] == n and (t.query_presence(rows) == presence).all() and t.components()[1].tolist() == comps
    assert not S.from_bits(t.query_presence(other), 5).any()
    # arguments
    assert lib.bft_gpu_marks_set(t._h, rows.ctypes.data, n, None, 4, None) == E_ARG
    bad = np.full(n, 1, dtype=np.uint8)
    bad[17] = 4
    assert lib.bft_gpu_marks_set(t._h, rows.ctypes.data, n, bad.ctypes.data, 0, None) == E_ARG
    assert lib.bft_gpu_marks_fill(t._h, 4) == E_ARG
    assert lib.bft_gpu_marks_test_and_set(t._h, rows.ctypes.data, n, 0, 4, buf.ctypes.data, None) == E_ARG
    assert lib.bft_gpu_marks_test_and_set(t._h, rows.ctypes.data, n, 2, 2, buf.ctypes.data, None) == E_ARG
    assert lib.bft_gpu_marks_reach(t._h, rows.ctypes.data, 1, None, 0, 1, 1, 0, buf.ctypes.data, cnt.ctypes.data) == E_ARG
    assert lib.bft_gpu_marks_reach(t._h, rows.ctypes.data, 1, None, 0, 0, 4, 0, buf.ctypes.data, cnt.ctypes.data) == E_ARG
    ids = np.array([1, 1], dtype=np.uint32)
    assert lib.bft_gpu_marks_reach(t._h, rows.ctypes.data, 1, ids.ctypes.data, 2, 0, 1, 0, buf.ctypes.data, cnt.ctypes.data) == E_ARG
    assert lib.bft_gpu_marks_select(t._h, 16, None, None, None, 0, C.byref(nb)) == E_ARG
    assert t.flag_counts().tolist() == [n, 0, 0, 0]  # (nothing of the above wrote a flag)
    # select: the cap rule of bft_gpu_kmers_by_count
    t.set_flags(rows[:30], 2)
    out_rows = np.zeros(30, dtype=np.uint32)
    assert lib.bft_gpu_marks_select(t._h, 4, None, None, out_rows.ctypes.data, 29, C.byref(nb)) == -6 and nb.value == 30 and not out_rows.any()
    assert lib.bft_gpu_marks_select(t._h, 4, None, None, out_rows.ctypes.data, 30, C.byref(nb)) == 0 and out_rows.tolist() == list(range(30))
    # begin twice keeps the flags; end then begin gives zeros; the graph is unlocked in between
    t.set_marking()
    assert t.flag_counts().tolist() == [n - 30, 0, 30, 0]
    t.unset_marking()
    assert lib.bft_gpu_marks_counts(t._h, cnt.ctypes.data) == E_STATE
    t.insert_kmers(other, 0)
    t.set_marking()
    assert t.info()["kmers"] == n + 5 and t.flag_counts().tolist() == [n + 5, 0, 0, 0]
    t.close()  # (bft_gpu_free releases the marks of a handle that is still marking)


def test_device_forms_on_a_caller_stream_match_the_host_forms():
    import torch
    k = 27
    t, owners = _three_genomes(k)
    rows, _ = t.extract()
    n = len(rows)
    host = BFT(k, device=0)
    for gid in range(3):
        host.insert_kmers(S.ascii_to_packed([x for x in owners if gid in owners[x]], k)[0], gid)
    assert (host.extract()[0] == rows).all()
    t.set_marking()
    host.set_marking()
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    rng = np.random.default_rng(8)
    batch = rows[rng.integers(0, n, size=5000)]
    seeds = rows[rng.integers(0, n, size=64)]
    with torch.cuda.stream(stream):
        d_batch = torch.from_numpy(batch).to(dev)
        d_one = torch.from_numpy(rows[::3].copy()).to(dev)
        d_seeds = torch.from_numpy(seeds).to(dev)
        d_rows = torch.from_numpy(rows).to(dev)
        d_get = torch.zeros(n, dtype=torch.uint8, device=dev)
        d_won = torch.zeros(len(batch), dtype=torch.uint8, device=dev)
        d_abs = torch.zeros(1, dtype=torch.int64, device=dev)
        d_counts = torch.zeros(4, dtype=torch.int64, device=dev)
        d_reach = torch.zeros(3, dtype=torch.int64, device=dev)
        d_new = torch.zeros(len(seeds), dtype=torch.uint8, device=dev)
        d_bits = torch.zeros((n + 63) // 64 * 8, dtype=torch.uint8, device=dev)  # (whole 64-bit words)
        d_sel = torch.zeros(n, dtype=torch.int32, device=dev)
        d_nsel = torch.zeros(1, dtype=torch.int64, device=dev)
        d_cc = torch.zeros(3, dtype=torch.int64, device=dev)
        s = stream.cuda_stream
        # interleaved with presence and component queries on the same handle, nothing synchronised in between
        t.set_flags_dev(d_one.data_ptr(), len(d_one), flag=2, d_absent_ptr=d_abs.data_ptr(), stream=s)
        t.query_presence_dev(d_rows.data_ptr(), n, d_bits.data_ptr(), stream=s)
        t.test_and_set_dev(d_batch.data_ptr(), len(batch), 0, 3, d_won.data_ptr(), stream=s)
        t.components_dev(0, 0, 0, d_cc.data_ptr(), stream=s)
        t.reach_dev(d_seeds.data_ptr(), len(seeds), d_new.data_ptr(), d_reach.data_ptr(), genome_ids=(0, 1), through=3, to=1, boundary=True, stream=s)
        t.get_flags_dev(d_rows.data_ptr(), n, d_get.data_ptr(), stream=s)
        t.flag_counts_dev(d_counts.data_ptr(), stream=s)
        t.select_flagged_dev(0b1010, 0, 0, d_sel.data_ptr(), n, d_nsel.data_ptr(), stream=s)
    stream.synchronize()
    assert host.set_flags(rows[::3], 2) == 0 and int(d_abs[0]) == 0
    won = host.test_and_set(batch, 0, 3)
    assert int(won.sum()) == int(d_won.sum().item())  # (which entry of a repeated k-mer wins is free; how many win is not)
    h_new, h_reach = host.reach(seeds, genome_ids=(0, 1), through=3, to=1, boundary=True)
    assert d_new.cpu().numpy().tolist() == h_new.tolist() and d_reach.cpu().numpy().tolist() == h_reach.tolist()
    assert (d_get.cpu().numpy() == host.get_flags(rows)).all()
    assert d_counts.cpu().numpy().tolist() == host.flag_counts().tolist()
    h_sel = host.select_flagged(0b1010)[1]
    assert int(d_nsel[0]) == len(h_sel) and d_sel.cpu().numpy()[:len(h_sel)].tolist() == h_sel.tolist()
    assert S.from_bits(d_bits.cpu().numpy(), n).all()
    assert int(d_cc[0]) == len(host.components()[1])
    assert t.read_flags().tolist() == host.read_flags().tolist()
    # a capture is refused, and records nothing of the library's
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream):
        d_nsel.zero_()  # (the recorded graph is not empty)
        rc = _lib.load().bft_gpu_marks_get_dev(t._h, d_rows.data_ptr(), n, d_get.data_ptr(), None, torch.cuda.current_stream().cuda_stream)
    del g  # (never replayed)
    assert rc == E_ARG
    assert t.read_flags().tolist() == host.read_flags().tolist()
    t.close()
    host.close()
