"""CPU-side tests (no GPU) of the case sets that tests/test_gpu_merge.py runs through the run merge (csrc/bft_merge.hip): the table of
(old id set X, run id set Y) pairs that reaches every regime of k_u_pairs / wave_union / union_len, the placement splits, and the
scripted chain of merges.  The generators live here so that a machine without a GPU can check that the cases still hold what they are
meant to hold: when the kernel's thresholds or the table change, this file fails until the case set covers every regime again."""
import numpy as np
import pytest

from bloomfiltertrie_amd import synth as S

LANES = 64  # wave_union holds the shorter list one id per lane; two lists beyond that take union_len
LEN_X = (0, 1, 2, 63, 64, 65, 127, 128, 129, 200)  # 0: a k-mer new in the run (a1 = 0)
LEN_Y = (0, 1, 2, 63, 64, 65, 128, 129, 200)       # 0: an index row the run does not touch
RELATIONS = ("interleaved", "y_below_x", "y_above_x", "y_in_x", "x_in_y", "half")
REPS = 3  # independent draws of the whole table: ~3000 k-mers
LAYOUTS = ("dense", "wide2", "wide4")
# (k, layout) of the GPU test: W = 1, 1 (pairs, not composites), 2, 3, 4; the three id layouts at k = 27
UNION_PARAMS = [(27, "dense"), (27, "wide2"), (27, "wide4"), (31, "dense"), (63, "dense"), (99, "dense"), (126, "dense")]


def kmers_for(n, k, seed):
    """n distinct packed k-mers of a random genome"""
    km = S.distinct(S.kmers_of(S.random_genome(n + k + 63, seed), k))
    assert len(km) >= n
    return np.ascontiguousarray(km[:n])


def id_pools(layout, rng):
    """(old, new): the id values an old set may hold, and those only a run may bring.  dense: 0..511, all of them old.  wide2: the old ids
    fill one byte, run-only ids from 256 up (the resident ids go from 1 to 2 bytes in the merge).  wide4: the old ids fill two bytes
    (65535 among them), run-only ids from 65536 up (2 to 4 bytes)."""
    if layout == "dense":
        return np.arange(512, dtype=np.int64), np.zeros(0, np.int64)
    if layout == "wide2":
        return np.arange(256, dtype=np.int64), 256 + np.sort(rng.choice(60000, 300, replace=False)).astype(np.int64)
    assert layout == "wide4"
    old = np.sort(np.concatenate([rng.choice(65535, 255, replace=False), [65535]])).astype(np.int64)
    return old, 65536 + np.sort(rng.choice(4465, 300, replace=False)).astype(np.int64)


def _pick(rng, pool, n):
    return np.sort(rng.choice(pool, n, replace=False)) if n else np.zeros(0, np.int64)


def make_pair(rng, old, new, lx, ly, rel):
    """One (X, Y) of the lengths and relation asked for, X from `old`, Y from `old` + `new`; None where the pools have no room for it
    (y_below_x / long subsets in the wide layouts: every X id is below 256 there)."""
    both = np.concatenate([old, new])  # (sorted: every new id is above every old one)
    if lx == 0 or ly == 0:
        return _pick(rng, old, lx), _pick(rng, both, ly)
    if rel == "y_in_x":
        if ly > lx:
            return None
        x = _pick(rng, old, lx)
        return x, _pick(rng, x, ly)
    if rel == "x_in_y":
        if lx > ly:
            return None
        x = _pick(rng, old, lx)
        return x, np.sort(np.concatenate([x, _pick(rng, np.setdiff1d(both, x), ly - lx)]))
    if rel == "y_below_x":
        if lx + ly > len(old):
            return None
        s = _pick(rng, old, lx + ly)
        return s[ly:], s[:ly]
    if rel == "y_above_x":
        x = _pick(rng, np.intersect1d(old, both[:len(both) - ly]), lx)
        return x, _pick(rng, both[both > x[-1]], ly)
    if rel == "interleaved":
        x = _pick(rng, old, lx)
        return x, _pick(rng, np.setdiff1d(both, x), ly)
    assert rel == "half"
    c = max(1, min(lx, ly) // 2)
    x = _pick(rng, old, lx)
    return x, np.sort(np.concatenate([_pick(rng, x, c), _pick(rng, np.setdiff1d(both, x), ly - c)]))


def union_cases(layout, seed):
    """The table: a list of dicts {x, y (sorted tuples of ids), lx, ly, rel, mult}.  Every (|X|, |Y|, relation) the pools have room for,
    REPS times; every fourth cell also lends its X to a pair with another Y and its Y to a pair with another X (rel "shared_x" /
    "shared_y"), so that one old set meets several run sets and the other way round.  mult: the k-mers that carry the pair, 1 or 3."""
    rng = np.random.default_rng(seed)
    old, new = id_pools(layout, rng)
    both = np.concatenate([old, new])
    cases = []

    def add(x, y, lx, ly, rel):
        cases.append(dict(x=tuple(int(v) for v in x), y=tuple(int(v) for v in y), lx=lx, ly=ly, rel=rel, mult=1 if len(cases) % 2 else 3))

    cell = 0
    for _ in range(REPS):
        for lx in LEN_X:
            for ly in LEN_Y:
                if lx == 0 and ly == 0:
                    continue
                for rel in (RELATIONS if lx and ly else ("none",)):
                    p = make_pair(rng, old, new, lx, ly, rel)
                    if p is None:
                        continue
                    x, y = p
                    add(x, y, lx, ly, rel)
                    cell += 1
                    if cell % 4:
                        continue
                    if lx:  # the same old set under another run set (an untouched row's set too: ly == 0)
                        add(x, _pick(rng, both, ly or LANES + 1), lx, ly or LANES + 1, "shared_x")
                    if ly:
                        add(_pick(rng, old, lx or 2), y, lx or 2, ly, "shared_y")
    return cases


def union_truth(k, layout):
    """(kmers, x_of, y_of, meta): the distinct k-mers of the case, the old and the run id tuple of each, and (|X|, |Y|, relation) of each
    for messages.  The assignment of cases to k-mers is shuffled."""
    seed = 1000 * k + LAYOUTS.index(layout)
    cases = union_cases(layout, seed)
    n = sum(c["mult"] for c in cases)
    km = kmers_for(n, k, seed)
    perm = np.random.default_rng(seed + 1).permutation(n)
    x_of, y_of, meta = [None] * n, [None] * n, [None] * n
    i = 0
    for c in cases:
        for _ in range(c["mult"]):
            r = int(perm[i])
            x_of[r], y_of[r], meta[r] = c["x"], c["y"], (c["lx"], c["ly"], c["rel"])
            i += 1
    return km, x_of, y_of, meta


def phases_of(km, id_lists):
    """Insert calls genome by genome, ascending: [(genome id, packed k-mers whose list holds it)]"""
    rows = {}
    for r, ids in enumerate(id_lists):
        for g in ids:
            rows.setdefault(g, []).append(r)
    return [(g, np.ascontiguousarray(km[np.array(rows[g])])) for g in sorted(rows)]


def regime_conditions(x_of, y_of):
    """What the table must hold before the GPU sees it: {condition: number of pairs (or old sets) that meet it}"""
    out = dict.fromkeys(["both_long", "short_64_long_above_128", "short_64_long_tops_it", "new_kmer_long_run", "union_is_x", "union_is_y",
                         "old_set_left_no_row", "old_set_keeps_a_row"], 0)
    untouched = {}
    for x, y in zip(x_of, y_of):
        lx, ly = len(x), len(y)
        out["both_long"] += lx > LANES and ly > LANES
        short, long_ = (x, y) if lx <= ly else (y, x)
        out["short_64_long_above_128"] += len(short) == LANES and len(long_) > 2 * LANES
        # (an id of the long list above all 64 lanes' ids, with a lane id the long list lacks: the count of new ids below it is popcount(fresh))
        out["short_64_long_tops_it"] += len(short) == LANES and len(long_) > LANES and long_[-1] > short[-1] and bool(set(short) - set(long_))
        out["new_kmer_long_run"] += lx == 0 and ly > LANES
        out["union_is_x"] += ly > 0 and set(y) <= set(x)
        out["union_is_y"] += lx > 0 and set(x) <= set(y)
        if lx:
            untouched[x] = untouched.get(x, False) or ly == 0
    out["old_set_left_no_row"] = sum(1 for v in untouched.values() if not v)
    out["old_set_keeps_a_row"] = sum(1 for v in untouched.values() if v)
    return out


@pytest.mark.parametrize("k,layout", UNION_PARAMS)
def test_union_table_holds_every_regime(k, layout):
    km, x_of, y_of, meta = union_truth(k, layout)
    assert len(km) == len(S.distinct(km)) and 2500 <= len(km) <= 3600
    for name, n in regime_conditions(x_of, y_of).items():
        assert n >= 1, name
    assert sum(1 for y in y_of if y) > 512  # run rows: more than two blocks of k_u_pairs
    ids = set()
    seen = set()
    for x, y, (lx, ly, rel) in zip(x_of, y_of, meta):
        assert (len(x), len(y)) == (lx, ly) and lx + ly > 0
        assert list(x) == sorted(set(x)) and list(y) == sorted(set(y))
        u = set(x) | set(y)
        sx, sy = set(x), set(y)
        want = {"none": lx + ly, "interleaved": lx + ly, "y_below_x": lx + ly, "y_above_x": lx + ly, "y_in_x": lx, "x_in_y": ly,
                "half": lx + ly - max(1, min(lx, ly) // 2)}.get(rel)
        if want is not None:  # (shared_x / shared_y draw the second list at random: any overlap)
            assert len(u) == want, (lx, ly, rel)
        if rel == "y_below_x":
            assert y[-1] < x[0]
        if rel == "y_above_x":
            assert y[0] > x[-1]
        if rel == "interleaved" and min(lx, ly) >= 63 and layout == "dense":
            assert y[0] < x[-1] and x[0] < y[-1] and not (sx & sy)
        seen.add((lx, ly, rel))
        ids |= u
    # every length pair occurs, under every relation that has room in the layout's pools
    for lx in LEN_X:
        for ly in LEN_Y:
            if lx and ly:
                assert (lx, ly, "interleaved") in seen and (lx, ly, "y_above_x") in seen and (lx, ly, "half") in seen
                assert ((lx, ly, "y_in_x") in seen) == (ly <= lx) and ((lx, ly, "x_in_y") in seen) == (lx <= ly)
                assert ((lx, ly, "y_below_x") in seen) == (layout == "dense" or lx + ly <= 256)
            elif lx or ly:
                assert (lx, ly, "none") in seen
    assert any(m[2] == "shared_x" for m in meta) and any(m[2] == "shared_y" for m in meta)
    xs_with = {}
    for x, y in zip(x_of, y_of):
        if x and y:
            xs_with.setdefault(x, set()).add(y)
    assert any(len(v) > 1 for v in xs_with.values())  # one old set under several run sets
    mults = {}
    for x, y in zip(x_of, y_of):
        mults[(x, y)] = mults.get((x, y), 0) + 1
    assert 1 in mults.values() and max(mults.values()) >= 3  # heads alone and heads with followers
    assert len(ids) <= 600
    old_ids = {g for x in x_of for g in x}
    run_only = {g for y in y_of for g in y} - old_ids
    if layout == "wide2":
        assert max(old_ids) < 256 and max(run_only) >= 256 and max(ids) < 65536
    if layout == "wide4":
        assert 256 <= max(old_ids) < 65536 and max(run_only) >= 65536
    if layout == "dense":
        assert max(ids) < 256 * 2
    # the insert calls carry exactly the table
    back = {}
    for g, part in phases_of(km, x_of):
        for row in part:
            back.setdefault(row.tobytes(), []).append(g)
    assert back == {km[r].tobytes(): list(x) for r, x in enumerate(x_of) if x}


# ---- placement: how the rows of the merged table split into the index's and the run's ------------------------------------------------
PLACEMENT_KS = (27, 32, 45, 64, 99, 126)
PLACEMENT_WAYS = ("run_first_third", "run_last_third", "run_every_second", "run_subset_of_index", "run_copy_of_index", "run_one_below",
                  "run_one_above", "run_one_present", "index_one_kmer", "run_new_before_present")
PLACEMENT_N = 1100  # rows: thirds of more than one 256-row block


def placement_split(way, n, rng):
    """(index rows, run rows) as ascending row numbers of the whole table's n rows"""
    every = np.arange(n)
    if way == "run_first_third":  # every insertion lands at position 0
        return every[n // 3:], every[:n // 3]
    if way == "run_last_third":   # every insertion lands at position n_a
        return every[:n - n // 3], every[n - n // 3:]
    if way == "run_every_second":  # one insertion per gap
        return every[0::2], every[1::2]
    if way == "run_subset_of_index":  # nothing is inserted; only colours change
        return every, np.sort(rng.choice(n, n // 3, replace=False))
    if way == "run_copy_of_index":
        return every, every
    if way == "run_one_below":
        return every[1:], every[:1]
    if way == "run_one_above":
        return every[:-1], every[-1:]
    if way == "run_one_present":
        return every, every[n // 2:n // 2 + 1]
    if way == "index_one_kmer":
        return every[n // 2:n // 2 + 1], np.delete(every, n // 2)
    assert way == "run_new_before_present"  # rows 3i+1 are new, rows 3i+2 in both: an insertion right before a row the run also touches
    return every[every % 3 != 1], every[every % 3 != 0]


def placement_sets(way, n, seed):
    """(index rows, run rows, x_of, y_of): random non-empty subsets of genomes {0, 1, 2} on the index's rows and of {3, 4} on the run's
    (of the same genomes, the same sets, for the copy), per row of the whole table; () where a side does not hold the row"""
    rng = np.random.default_rng(seed)
    ia, ib = placement_split(way, n, rng)
    subsets_a = [(0,), (1,), (2,), (0, 1), (0, 2), (1, 2), (0, 1, 2)]
    subsets_b = [(3,), (4,), (3, 4)]
    x_of, y_of = [()] * n, [()] * n
    for r in ia:
        x_of[r] = subsets_a[int(rng.integers(len(subsets_a)))]
    for r in ib:
        y_of[r] = x_of[r] if way == "run_copy_of_index" else subsets_b[int(rng.integers(len(subsets_b)))]
    return ia, ib, x_of, y_of


@pytest.mark.parametrize("way", PLACEMENT_WAYS)
def test_placement_splits_are_what_their_names_say(way):
    n = PLACEMENT_N
    ia, ib, x_of, y_of = placement_sets(way, n, 5)
    assert len(np.union1d(ia, ib)) == n and (np.diff(ia) > 0).all() and (np.diff(ib) > 0).all()
    new = np.setdiff1d(ib, ia)  # the rows the merge inserts
    pos = np.searchsorted(ia, new)  # index rows below each
    assert all(bool(x_of[r]) == (r in set(ia.tolist())) for r in range(n)) and all(bool(y_of[r]) == (r in set(ib.tolist())) for r in range(n))
    if way == "run_first_third":
        assert len(new) == len(ib) > 256 and (pos == 0).all()
    elif way == "run_last_third":
        assert len(new) == len(ib) > 256 and (pos == len(ia)).all()
    elif way == "run_every_second":
        assert len(new) == len(ib) and len(np.unique(pos)) == len(pos) and pos[-1] == len(ia)
    elif way == "run_subset_of_index":
        assert len(new) == 0 and 256 < len(ib) < n
    elif way == "run_copy_of_index":
        assert len(new) == 0 and len(ib) == n and x_of == y_of
    elif way == "run_one_below":
        assert len(ib) == 1 and pos.tolist() == [0]
    elif way == "run_one_above":
        assert len(ib) == 1 and pos.tolist() == [len(ia)]
    elif way == "run_one_present":
        assert len(ib) == 1 and len(new) == 0
    elif way == "index_one_kmer":
        assert len(ia) == 1 and len(new) == n - 1 and 0 < pos.sum() < len(pos)  # insertions on both sides of the one row
    else:
        both = np.intersect1d(ia, ib)
        assert len(new) > 256 and len(both) > 256 and np.isin(new + 1, both)[:-1].all()  # (cnt > 0 at an index row the run holds)


# ---- a chain of merges on one handle: the old lists are themselves unions --------------------------------------------------------------
CHAIN_KS = (27, 63)
CHAIN_GROUPS = dict(A=40, B=40, C=40, N=40, S=30, S2=30, D=300, L=300, L2=40)  # k-mers per group


def chain_script():
    """[build] of [(genome id, groups)] insert calls, in call order.
      merge 2 (build 2)  genome 12 lands on every row of S: the old set {10, 11} loses its last row
      merge 3            {10} + {11} on S2 brings the list {10, 11} back as a union; {1, 2} + {3} on A, {1, 3} + {2} on B, the untouched
                         {1, 2, 3} of C and the new k-mers N inserted with {1, 2, 3} are one set; the insert calls arrive with ids descending
                         (as in build 2), so the run takes the general sort
      merge 4            70 genomes on L, whose rows carry 70 already (two long lists), 10 of them on L2 as new k-mers
      merge 5            genome 0 on every row: every old set loses its rows, an id below all the others joins lists of 1 .. 141 ids"""
    b1 = [(1, "ABC"), (2, "AC"), (3, "BC"), (10, ("S", "S2")), (11, ("S",))] + [(g, ("L",)) for g in range(100, 170)]
    b2 = [(20, ("D",)), (12, ("S",))]
    b3 = [(11, ("S2",)), (3, "AN"), (2, "BN"), (1, "N")]
    b4 = [(g, ("L", "L2") if g >= 260 else ("L",)) for g in range(200, 270)]
    b5 = [(0, tuple(CHAIN_GROUPS))]
    return [b1, b2, b3, b4, b5]


def chain_rows():
    rows, at = {}, 0
    for name, n in CHAIN_GROUPS.items():
        rows[name] = np.arange(at, at + n)
        at += n
    return rows, at


def chain_truth_after(n_builds):
    """{row: sorted id tuple} after the first n_builds builds of the script"""
    rows, _ = chain_rows()
    sets = {}
    for build in chain_script()[:n_builds]:
        for g, groups in build:
            for name in groups:
                for r in rows[name]:
                    sets.setdefault(int(r), set()).add(g)
    return {r: tuple(sorted(v)) for r, v in sets.items()}


def test_chain_script_does_what_it_says():
    script = chain_script()
    assert len(script) == 5
    rows, _ = chain_rows()
    t = [chain_truth_after(i) for i in range(len(script) + 1)]
    lists = [set(x.values()) for x in t]
    # an old set loses its last row in merge 2 and its list comes back as a union in merge 3
    assert (10, 11) in lists[1] and (10, 11) not in lists[2] and (10, 11) in lists[3]
    assert {t[2][int(r)] for r in rows["S2"]} == {(10,)} and {t[3][int(r)] for r in rows["S2"]} == {(10, 11)}
    # two different (old, run) pairs, an untouched row and a new k-mer: one set
    assert {t[2][int(r)] for r in rows["A"]} == {(1, 2)} and {t[2][int(r)] for r in rows["B"]} == {(1, 3)} and {t[2][int(r)] for r in rows["C"]} == {(1, 2, 3)}
    assert all(int(r) not in t[2] for r in rows["N"])
    assert {t[3][int(r)] for n in "ABCN" for r in rows[n]} == {(1, 2, 3)}
    # ids descending within builds 2 and 3
    for b in script[1:3]:
        gids = [g for g, _ in b]
        assert gids == sorted(gids, reverse=True) and len(gids) > 1
    # a run of more than 64 genomes on rows that carry more than 64
    assert all(len(t[3][int(r)]) > LANES for r in rows["L"]) and len({g for g, _ in script[3]}) > LANES
    assert all(len(t[4][int(r)]) == 140 for r in rows["L"])
    assert all(v[0] == 0 for v in t[5].values())


# ---- flush-driven merges: 150 genomes of one short ancestor, most k-mers on more than 64 of them -------------------------------------------
FLUSH_K, FLUSH_GENOMES, FLUSH_PAIRS = 27, 150, 30000


def flush_genomes():
    """[distinct packed k-mers of genome g]: a 3000-nt ancestor, two clades of 75 genomes whose founders differ from it at a dozen places
    (k-mers on ~75 ids, next to the ancestor's on ~150), and a private SNP in every third genome or so.  A SNP makes 27 k-mers of its own, so
    private mutations must stay rare for most k-mers to be carried by more than 64 genomes: 150 genomes at a rate of 0.002 would bring
    eight private k-mers for every shared one."""
    k = FLUSH_K
    anc = S.random_genome(3000 + k - 1, 271)
    founders = [S.mutate(anc, 0.004, 41), S.mutate(anc, 0.004, 42)]
    return [S.distinct(S.kmers_of(S.mutate(founders[g % 2], 0.0001, 500 + g), k)) for g in range(FLUSH_GENOMES)]


def flush_order():
    """the insert calls' genome ids: out of order, five genomes twice"""
    order = np.random.default_rng(9).permutation(FLUSH_GENOMES).tolist()
    return order + order[:5]


def flush_truth(genomes):
    sets = {}
    for g, km in enumerate(genomes):
        for row in km:
            sets.setdefault(row.tobytes(), set()).add(g)
    return {kk: tuple(sorted(v)) for kk, v in sets.items()}


def test_flush_case_has_long_lists_and_enough_flushes():
    genomes = flush_genomes()
    truth = flush_truth(genomes)
    sizes = np.array([len(v) for v in truth.values()])
    assert (sizes > LANES).sum() > len(truth) // 2  # most k-mers carry more than 64 ids
    assert len({v for v in truth.values() if len(v) > LANES}) >= 10  # and not all the same list
    assert (sizes == 1).any() and ((sizes > LANES) & (sizes < 100)).any() and (sizes > 140).any()
    order = flush_order()
    assert sorted(set(order)) == list(range(FLUSH_GENOMES)) and len(order) == FLUSH_GENOMES + 5
    assert max(len(g) for g in genomes) <= FLUSH_PAIRS  # (no call is split)
    # the log holds fewer than FLUSH_PAIRS pairs: at least this many flushes before the last build
    pending, flushes = 0, 0
    for g in order:
        if pending and pending + len(genomes[g]) > FLUSH_PAIRS:
            flushes, pending = flushes + 1, 0
        pending += len(genomes[g])
    assert flushes >= 10
