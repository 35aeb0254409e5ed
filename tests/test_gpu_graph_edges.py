"""The whole-graph features -- simple paths (bft_paths.hip), connected components (bft_components.hip), reach and boundary marks (bft_marking.hip),
sub-graph builds (bft_subgraph.hip) and pan-genome emission (bft_pangenome.hip), all over bft_for_each_successor / sp_top (bft_succ.h) -- against
ground truth at every key shape, id width, cycle shape, jump depth and table end, and over a table that takes a second grid pass.  The cases and
their truth come from tests/test_graph_cases_host.py, which proves on the CPU that every case reaches the regime it is named after; the truth's
rows are in the order of the T-form digits, not of the product's extract(), and every index is first checked to extract in that order with
those colour sets.  Everything is compared exactly: the paths and the {paths, characters, longest} of the sizing call; labels, sizes and the
three counts of the components; the whole flag array after every reach; the k-mers and colour sets of a sub-graph; rows, packed k-mers and
ASCII of the pan-genome classes."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_graph_cases_host as H  # noqa: E402

from bloomfiltertrie_amd import BFT, _lib  # noqa: E402

pytestmark = pytest.mark.gpu


def _build(tr):
    """the handle of a truth; extract() must be in the truth's order, so that "row" means the same on both sides"""
    t = BFT(tr.k, device=0)
    for gid, km in tr.inserts():
        t.insert_kmers(km, gid)
    km, cs = t.extract()
    assert km.shape == tr.packed.shape and (km == tr.packed).all()
    uniq, inv = np.unique(cs, return_inverse=True)
    held = np.zeros((len(uniq), len(tr.gids)), dtype=bool)
    for i, c in enumerate(uniq):
        held[i, [tr.gids.index(g) for g in t.colorset(int(c))]] = True
    assert (held[inv] == tr.member).all()
    return t


def _sizing(t, thr):
    """{paths, characters, longest} of the sizing call (no buffers)"""
    import torch
    cnt = torch.full((3,), 7, dtype=torch.int64, device=torch.device("cuda", 0))
    t.simple_paths_dev(0, 0, 0, 0, cnt.data_ptr(), min_shared=thr)
    torch.cuda.synchronize()
    return cnt.cpu().tolist()


def _paths(t, tr, thresholds):
    for thr in thresholds:
        got, want = t.simple_paths(thr), tr.paths(thr)
        assert len(got) == len(want) and got == want, (tr.k, thr, len(got), len(want), [i for i, (a, b) in enumerate(zip(got, want)) if a != b][:3])
        assert _sizing(t, thr) == tr.path_counts(thr), (tr.k, thr)


def _components(t, tr, id_lists):
    lib = _lib.load()
    for ids in id_lists:
        labels, sizes = t.components(ids)
        wl, ws = tr.components(ids)
        assert (labels == wl).all(), (tr.k, ids, int((labels != wl).sum()), np.flatnonzero(labels != wl)[:5])
        assert sizes.dtype == np.uint64 and sizes.tolist() == ws.tolist(), (tr.k, ids)
        a = np.ascontiguousarray(ids, dtype=np.uint32)
        cnt = np.zeros(3, dtype=np.uint64)
        assert lib.bft_gpu_components(t._h, a.ctypes.data if len(a) else None, len(a), None, 0, None, 0, cnt.ctypes.data) == 0
        assert cnt.tolist() == tr.component_counts(ids), (tr.k, ids)


def _id_lists(tr):
    """(), one id, two ids, an id past the last genome"""
    g = tr.gids
    return [(), (g[-1],), (tr.G,)] + ([(g[0], g[1])] if len(g) > 1 else []) + ([(g[1],)] if len(g) > 1 else [])


def _reach(t, tr, seed=0):
    """reach from a few seeds, an absent one among them, with and without genome ids, with the boundary: the whole flag array after every call"""
    model, row_of = tr.model(), tr.row_of
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, tr.N, 6).tolist()
    absent = tr.absent(1, seed + 1)
    g = tr.gids
    t.set_marking()

    def call(seed_rows, with_absent=False, **kw):
        seeds = tr.packed[seed_rows]
        names = [tr.strings[r] for r in seed_rows]
        if with_absent:
            seeds = np.concatenate([seeds[:1], H.pack(absent), seeds[1:]])
            names = names[:1] + [H.text(absent[0])] + names[1:]
        got_new, got_counts = t.reach(np.ascontiguousarray(seeds), **kw)
        want_new, want_counts = model.reach(names, **{("ids" if a == "genome_ids" else a): v for a, v in kw.items()})
        assert got_new.tolist() == want_new and got_counts.tolist() == want_counts, (tr.k, seed_rows, kw, got_counts.tolist(), want_counts)
        assert t.read_flags().tolist() == model.packed(row_of).tolist(), (tr.k, seed_rows, kw)

    call(rows[:2], with_absent=True)
    call(rows[2:4], genome_ids=(g[-1],), through=0, to=2)
    call(rows[3:6] + rows[:1], genome_ids=(g[0],), through=0, to=3, boundary=True)
    call([0, tr.N - 1], through=1, to=2)
    call(rows[4:6] + [tr.N // 2], through=0, to=1, boundary=True)
    counts = np.bincount(np.array([model.flag[s] for s in tr.strings]), minlength=4)
    assert t.flag_counts().tolist() == counts.tolist()
    t.unset_marking()


def _subgraph(t, tr):
    """every third row plus absent k-mers, shuffled, some twice"""
    rows = np.arange(0, tr.N, 3)
    absent = H.pack(tr.absent(7, 3))
    batch = np.concatenate([tr.packed[rows], absent, tr.packed[rows[:5]]])
    batch = np.ascontiguousarray(batch[np.random.default_rng(tr.k).permutation(len(batch))])
    sub, n_absent = t.subgraph(batch)
    assert n_absent == 7
    km, cs = sub.extract()
    assert km.shape == tr.packed[rows].shape and (km == tr.packed[rows]).all()
    sets = {int(c): tuple(sub.colorset(int(c))) for c in np.unique(cs)}
    want = tr.sets()
    assert [sets[int(c)] for c in cs] == [want[r] for r in rows]
    sub.close()


def _classes(t, tr):
    asc, rows = t.kmers_by_count(1, tr.G, ascii=True)  # (the binding refuses an ASCII k-mer without its NUL)
    assert rows.dtype == np.uint32 and rows.tolist() == list(range(tr.N)) and asc == tr.strings
    for lo, hi in ((1, 1), (2, tr.G), (len(tr.gids), len(tr.gids)), (2, 2)):
        km, rows = t.kmers_by_count(lo, hi)
        want = tr.by_count(lo, hi)
        assert rows.tolist() == want.tolist() and (km == tr.packed[want]).all(), (tr.k, lo, hi)
        asc, rows = t.kmers_by_count(lo, hi, ascii=True)
        assert rows.tolist() == want.tolist() and asc == [tr.strings[r] for r in want]


def _graph(tr, thresholds=None):
    """paths, components and reach of a truth"""
    t = _build(tr)
    _paths(t, tr, thresholds if thresholds is not None else (0, 1, 2, len(tr.gids) + 1))
    _components(t, tr, _id_lists(tr))
    _reach(t, tr)
    return t


@pytest.mark.parametrize("k", H.KEY_SHAPES)
def test_key_shapes_run_all_five_features(k):
    tr = H.key_shape(k)
    t = _graph(tr, (0, 1, 2, 3, 4))
    _subgraph(t, tr)
    _classes(t, tr)
    _paths(t, tr, (0,))  # and the handle answers as before
    t.close()


@pytest.mark.parametrize("k", H.DENSE_KS)
def test_dense_successor_intervals(k):
    tr = H.dense(k)
    t = _graph(tr)
    labels, _ = t.components()
    succ = tr.ev[tr.eu == tr.u]
    assert len(set(labels[succ].tolist()) | {int(labels[tr.u])}) == 1  # u and its four successors: one component
    t.close()


@pytest.mark.parametrize("table", H.ENDS_TABLES)
@pytest.mark.parametrize("k", H.ENDS_KS)
def test_table_ends_and_empty_buckets(k, table):
    _graph(H.ends(k, table)).close()


@pytest.mark.parametrize("k", H.CYCLE_KS)
@pytest.mark.parametrize("p", H.CYCLE_PS)
def test_cycles(p, k):
    tr = H.cycles(k, p)
    t = _graph(tr)
    got = t.simple_paths()
    for period, rows in zip(tr.periods, tr.cycle_rows):
        i = next(i for i, x in enumerate(H.ring(period, k)) if H.text(x) == tr.strings[rows[0]])
        turn = np.roll(period, -i)
        assert H.text(np.resize(turn, p + k - 1)) in got  # the cycle from its k-mer of smallest row, p + k - 1 nucleotides
    t.close()


@pytest.mark.parametrize("k", H.WHOLE_KS)
@pytest.mark.parametrize("kind", ("chain", "cycle"))
@pytest.mark.parametrize("n", H.WHOLE_NS)
def test_whole_table_is_one_path(n, kind, k):
    tr = H.whole_table(n, kind, k)
    t = _graph(tr)
    assert _sizing(t, 0) == [1, n + k - 1, n + k - 1]  # one path, longest == n + k - 1
    assert len(t.simple_paths()[0]) == n + k - 1
    labels, sizes = t.components()
    assert sizes.tolist() == [n] and (labels == 0).all()  # one component
    t.close()


@pytest.mark.parametrize("k", H.CUT_KS)
def test_min_shared_cuts_a_cycle_and_an_edge(k):
    tr = H.cut(k)
    t = _graph(tr, (0, 1, 2, 3, 4))
    two = t.simple_paths(2)
    assert len(two) == 4 and tr.chain[H.CUT_ODD] in two
    assert any(s.startswith(tr.cycle[H.CUT_GAP + 1]) and s.endswith(tr.cycle[H.CUT_GAP - 1]) for s in two)
    t.close()


@pytest.mark.parametrize("t_shared", H.SHARED_TS)
def test_shared_id_lists_at_the_threshold(t_shared):
    tr = H.shared(t_shared)
    t = _build(tr)
    _paths(t, tr, sorted({0, 1, 2, 7, 20, t_shared - 1, t_shared, t_shared + 1, 24, 25, H.SHARED_G + 1} - {-1}))
    ids = tr.sets()[tr.row_of[tr.pairs[0][0]]]
    _components(t, tr, [(), ids[:1], ids[:2], ids, (H.SHARED_G,)])
    _reach(t, tr)
    t.close()


def test_id_widths_give_the_same_answers():
    """the cut graph with dictionary ids of one, two and four bytes (no call reports the width: the labellings put the largest id below 2^8,
    2^16 and above)"""
    answers = []
    for tr in H.id_widths():
        t = _graph(tr, (0, 1, 2, 3, 4))
        _subgraph(t, tr)
        ans = [t.simple_paths(thr) for thr in (0, 1, 2, 3)]
        for slots in ((), (0,), (1,), (2,), (0, 1), (1, 2), (0, 1, 2)):
            labels, sizes = t.components([tr.gids[s] for s in slots])
            ans.append((labels.tolist(), sizes.tolist()))
        t.set_marking()
        seeds = np.ascontiguousarray(tr.packed[[3, 40, 60]])
        for kw in (dict(genome_ids=(tr.gids[1],)), dict(genome_ids=(tr.gids[0], tr.gids[1]), to=2, boundary=True), dict(genome_ids=(tr.gids[2],), to=3, boundary=True)):
            new, cnt = t.reach(seeds, **kw)
            ans.append((new.tolist(), cnt.tolist(), t.read_flags().tolist()))
        t.unset_marking()
        answers.append(ans)
        t.close()
    assert answers[0] == answers[1] == answers[2]


def test_second_grid_pass():
    """2048 * 256 + 300 rows: every one-row-per-lane kernel loops.  One build; paths at t = 0 and 2, components of the whole graph and of genome
    1, one reach per big component, the rows of the pan-genome classes."""
    tr = H.grid()
    t = _build(tr)
    assert t.info()["kmers"] == tr.N == H.GRID_CAP + H.GRID_LOOSE
    _paths(t, tr, (0, 2))
    _components(t, tr, [(), (1,)])
    labels, sizes = tr.components()
    t.set_marking()
    flags = np.zeros(tr.N, dtype=np.uint8)
    for name in ("linear", "circular"):
        c = labels[tr.seed_rows[name]]
        new, cnt = t.reach(H.pack(tr.seeds[name][None]))
        assert new.tolist() == [1] and cnt.tolist() == [int(sizes[c]), 0, 0]
        flags[labels == c] = 1
        assert t.flag_counts().tolist() == [int((flags == 0).sum()), int((flags == 1).sum()), 0, 0]
        assert (t.read_flags() == H.pack_flags(flags)).all()
    # the sub-graph of genome 1 with its boundary, from the linear genome: the k-mers behind the stretch are another component and stay 1
    a, b = tr.stretch
    l1, s1 = tr.components((1,))
    c = l1[tr.seed_rows["linear"]]
    new, cnt = t.reach(H.pack(tr.seeds["linear"][None]), genome_ids=(1,), through=1, to=2, boundary=True)
    assert new.tolist() == [1] and cnt.tolist() == [int(s1[c]), 1, 0] and int(s1[c]) == a  # (one boundary row: the stretch's first k-mer)
    assert t.flag_counts().tolist() == [H.GRID_LOOSE, tr.N - H.GRID_LOOSE - a - 1, a + 1, 0]
    t.unset_marking()
    for lo, hi in ((1, 1), (2, 2), (1, 2)):
        km, rows = t.kmers_by_count(lo, hi)
        want = tr.by_count(lo, hi)
        assert len(rows) == len(want) and (rows == want).all() and (km == tr.packed[want]).all()
    t.close()
