"""The run merge (csrc/bft_merge.hip) against ground truth: a second build places the run's k-mers among the index's rows
(k_merge_search / count / old / new) and rebuilds every colour set as the union of an old id list and a run id list (k_u_pairs:
wave_union with one list of at most 64 ids held one per lane, union_len when both are longer).  The truth is plain Python everywhere,
{packed k-mer bytes: sorted tuple of genome ids} of what was inserted; the library is read through extract(), colorset(), info() and
query_colors().  Every test builds the same content twice -- `merged` in several builds on one handle, `whole` in one -- and checks
both against the truth and against each other (_check).  The case sets and the conditions they must hold are in
tests/test_merge_cases_host.py, which checks them without a GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_merge_cases_host as H  # noqa: E402
from test_gpu_build import ARRAYS, _colour_map  # noqa: E402

from bloomfiltertrie_amd import BFT, synth as S  # noqa: E402

pytestmark = pytest.mark.gpu


def _mismatches(got, truth, meta):
    """the first few k-mers whose id list is not the truth's, with what the case table says about them"""
    out = []
    for key, want in truth.items():
        have = got.get(key)
        if have != want:
            out.append(dict(case=meta.get(key) if meta else None, want_len=len(want), got_len=None if have is None else len(have),
                            missing=sorted(set(want) - set(have or ()))[:8], extra=sorted(set(have or ()) - set(want))[:8],
                            got_sorted=have is not None and list(have) == sorted(set(have))))
            if len(out) == 6:
                break
    extra_kmers = len(set(got) - set(truth))
    return f"{sum(1 for kk, v in truth.items() if got.get(kk) != v)} k-mers differ, {extra_kmers} k-mers not in the truth; first: {out}"


def _check(merged, whole, truth, meta=None, seed=0):
    """Everything a merged handle must be: truth: {k-mer bytes: sorted id tuple}; meta: {k-mer bytes: (|X|, |Y|, relation)} for messages"""
    mm, nsm = _colour_map(merged)
    mw, nsw = _colour_map(whole)
    # 1. the colour map is the truth's and the single build's
    assert mm == truth, _mismatches(mm, truth, meta)
    assert mw == truth, "the single build: " + _mismatches(mw, truth, meta)
    # 2. counts
    im, iw = merged.info(), whole.info()
    n_sets = len(set(truth.values()))
    assert im["kmers"] == iw["kmers"] == len(truth)
    assert im["pairs"] == iw["pairs"] == sum(len(v) for v in truth.values())
    assert im["colorsets"] == iw["colorsets"] == n_sets == nsm == nsw
    assert im["pending_pairs"] == 0 and iw["pending_pairs"] == 0
    for f in ("nodes", "ccs", "prefixes", "child_nodes", "genomes"):
        assert im[f] == iw[f], f
    # 3. the dictionary: no orphan set, every list strictly ascending, no list twice
    km, cs = merged.extract()
    assert np.unique(cs).tolist() == list(range(n_sets))
    lists = [tuple(merged.colorset(c)) for c in range(n_sets)]
    for c, ids in enumerate(lists):
        assert len(ids) > 0 and all(a < b for a, b in zip(ids, ids[1:])), (c, ids[:10])
    assert len(set(lists)) == n_sets
    # 4. the containers are a function of the k-mer set alone
    for name in ARRAYS:
        a, b = merged.debug_array(name), whole.debug_array(name)
        assert a.shape == b.shape and (a == b).all(), name
    # 5. the committed (narrowed) dictionary through a query: ~500 stored k-mers and a few absent ones
    rng = np.random.default_rng(seed)
    pick = rng.choice(len(km), min(500, len(km)), replace=False)
    absent = S.snp_mutants(km[pick[:40]], merged.k, seed + 1)
    q = np.ascontiguousarray(np.concatenate([km[pick], absent]))
    for t in (merged, whole):
        bits, off, ids = t.query_colors(q)
        present = S.from_bits(bits, len(q))
        for i in range(len(q)):
            want = truth.get(q[i].tobytes(), ())
            assert bool(present[i]) == bool(want), i
            assert tuple(ids[int(off[i]):int(off[i + 1])].tolist()) == want, (i, meta.get(q[i].tobytes()) if meta else None)
        assert int(off[-1]) == len(ids)


def _insert(t, calls):
    for g, part in calls:
        t.insert_kmers(part, g)


# ---- 1. union regimes --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,layout", H.UNION_PARAMS)
def test_union_regimes_against_ground_truth(k, layout):
    """Every (|X|, |Y|, relation) of the case table -- one list on the lanes and the other streamed in chunks of 64 (one ragged chunk,
    whole chunks, several), a lane list of exactly 64 ids, two lists beyond 64 (the serial merge), an empty old list (a new k-mer), an
    untouched row -- side by side in the wavefronts of k_u_pairs, at every key width; under the wide layouts the resident ids are
    widened (1 -> 2 bytes, 2 -> 4 bytes) by the same merge."""
    km, x_of, y_of, meta_rows = H.union_truth(k, layout)
    for name, n in H.regime_conditions(x_of, y_of).items():  # conditions on the generator, not on the library
        assert n >= 1, name
    assert sum(1 for y in y_of if y) > 512
    truth = {km[r].tobytes(): tuple(sorted(set(x_of[r]) | set(y_of[r]))) for r in range(len(km))}
    meta = {km[r].tobytes(): meta_rows[r] for r in range(len(km))}
    p1, p2 = H.phases_of(km, x_of), H.phases_of(km, y_of)
    merged, whole = BFT(k), BFT(k)
    _insert(merged, p1)
    merged.build()
    if layout != "dense":  # the old ids are resident in 1 byte (wide2) / 2 bytes (wide4) before the merge ...
        fp, n_ids = merged.footprint(), sum(len(set(x)) for x in set(x_of))
        assert (fp["colorset_dictionary"] - 4 * (merged.info()["colorsets"] + 1)) // n_ids == (1 if layout == "wide2" else 2)
    _insert(merged, p2)
    assert merged.info()["pending_pairs"] == sum(len(y) for y in y_of)
    merged.build()
    if layout != "dense":  # ... and in 2 / 4 bytes after it
        n_ids = sum(len(v) for v in set(truth.values()))
        assert (merged.footprint()["colorset_dictionary"] - 4 * (merged.info()["colorsets"] + 1)) // n_ids == (2 if layout == "wide2" else 4)
    _insert(whole, p1)
    _insert(whole, p2)
    whole.build()
    _check(merged, whole, truth, meta, seed=k)
    merged.close()
    whole.close()


# ---- 2. placement edges ------------------------------------------------------------------------------------------------------------------
_ROW_ORDER = {}


def _rows_in_table_order(k):
    """PLACEMENT_N distinct k-mers in the order of the table's rows: extract() copies the stored k-mers in ascending T-form order
    (include/bft_gpu.h), which is the order of `tk`"""
    if k not in _ROW_ORDER:
        t = BFT(k)
        t.insert_kmers(H.kmers_for(H.PLACEMENT_N, k, 77 + k), 0)
        t.build()
        km, _ = t.extract()
        assert len(km) == H.PLACEMENT_N and len(t.debug_array("tk")) == H.PLACEMENT_N * 8 * ((2 * k + 63) // 64)
        bits, at, _ = t.query_rows(km)  # (and the library agrees: k-mer i of the extraction is row i of the table)
        assert S.from_bits(bits, len(km)).all() and (at == np.arange(len(km))).all()
        t.close()
        _ROW_ORDER[k] = np.ascontiguousarray(km)
    return _ROW_ORDER[k]


@pytest.mark.parametrize("way", H.PLACEMENT_WAYS)
@pytest.mark.parametrize("k", H.PLACEMENT_KS)
def test_placement_edges_against_ground_truth(k, way):
    """The rows of the merged table split into the index's and the run's so that every insertion lands before the first index row, after
    the last one (cnt[n_a]), one per gap, nowhere (the index holds the whole run: only colours change, or nothing at all), or the run /
    the index is a single k-mer; at every key width."""
    rows = _rows_in_table_order(k)
    n = len(rows)
    ia, ib, x_of, y_of = H.placement_sets(way, n, 1000 + k)
    truth = {rows[r].tobytes(): tuple(sorted(set(x_of[r]) | set(y_of[r]))) for r in range(n)}
    meta = {rows[r].tobytes(): (len(x_of[r]), len(y_of[r]), f"{way} row {r}") for r in range(n)}
    p1, p2 = H.phases_of(rows, x_of), H.phases_of(rows, y_of)
    merged, whole = BFT(k), BFT(k)
    _insert(merged, p1)
    merged.build()
    before = merged.info()
    assert before["kmers"] == len(ia)
    map_before = _colour_map(merged)
    _insert(merged, p2)
    merged.build()
    after = merged.info()
    assert after["kmers"] == n
    if way == "run_copy_of_index":  # nothing changes at all: the same sets under the same ids, no duplicate set
        assert _colour_map(merged) == map_before
        for f in ("kmers", "pairs", "colorsets", "genomes", "nodes", "ccs", "prefixes", "child_nodes"):
            assert after[f] == before[f], f
    _insert(whole, p1)
    _insert(whole, p2)
    whole.build()
    ek, _ = merged.extract()
    assert (ek == rows).all()  # the merged table's rows are in the single build's order
    _check(merged, whole, truth, meta, seed=k)
    merged.close()
    whole.close()


# ---- 3. chains of merges -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", H.CHAIN_KS)
def test_chain_of_merges_against_ground_truth(k):
    """Five builds on one handle (the script and what each merge is for: chain_script in tests/test_merge_cases_host.py): an old set that
    loses its last row leaves the dictionary and its list comes back as a union one merge later; the same set reached by two different
    (old, run) pairs, an untouched row and a new k-mer gets one id; insert calls with descending ids; a run of 70 genomes on rows that
    carry 70.  The colour map is the truth's after every build."""
    rows, n = H.chain_rows()
    km = H.kmers_for(n, k, 300 + k)
    script = H.chain_script()
    merged, whole = BFT(k), BFT(k)
    for b, build in enumerate(script):
        for g, groups in build:
            part = np.ascontiguousarray(np.concatenate([km[rows[name]] for name in groups]))
            merged.insert_kmers(part, g)
            whole.insert_kmers(part, g)
        merged.build()
        t = H.chain_truth_after(b + 1)
        truth = {km[r].tobytes(): ids for r, ids in t.items()}
        meta = {km[r].tobytes(): (f"after build {b + 1}", r) for r in t}
        got, n_sets = _colour_map(merged)
        assert got == truth, _mismatches(got, truth, meta)
        lists = {tuple(merged.colorset(c)) for c in range(merged.info()["colorsets"])}
        assert lists == set(truth.values()) and n_sets == len(lists) == merged.info()["colorsets"]  # no orphan, no duplicate
        assert ((10, 11) in lists) == (b in (0, 2, 3))  # gone with its last row in merge 2, back as a union in merge 3
        if b == 2:  # two (old, run) pairs, an untouched row, a new k-mer: one id
            ek, ecs = merged.extract()
            ids_of = {ek[i].tobytes(): int(ecs[i]) for i in range(len(ek))}
            assert len({ids_of[km[r].tobytes()] for name in "ABCN" for r in rows[name]}) == 1
    whole.build()
    _check(merged, whole, truth, meta, seed=k)
    merged.close()
    whole.close()


# ---- 4. flush-driven merges with long lists ----------------------------------------------------------------------------------------------
def test_flush_driven_merges_with_long_lists_against_ground_truth():
    """The shape of test_insertions_merge_into_the_index_without_a_pair_bound with 150 genomes of a short ancestor at a low mutation rate
    (flush_genomes in tests/test_merge_cases_host.py): most k-mers carry more than 64 ids, and "flush_pairs" makes the insert series merge
    its log into the index more than ten times, so long old lists meet runs of a few genomes again and again."""
    k = H.FLUSH_K
    genomes = H.flush_genomes()
    truth = H.flush_truth(genomes)
    assert sum(1 for v in truth.values() if len(v) > H.LANES) > len(truth) // 2  # (a condition on the generator)
    merged, whole = BFT(k), BFT(k)
    merged.set_option("flush_pairs", H.FLUSH_PAIRS)
    merges, pending = 0, 0
    for g in H.flush_order():
        whole.insert_kmers(genomes[g], g)
        merged.insert_kmers(genomes[g], g)
        now = merged.info()["pending_pairs"]
        merges += now < pending + len(genomes[g])  # the log was merged into the index before this call's pairs went in
        pending = now
    assert merges >= 10, merges
    merged.build()
    whole.build()
    _check(merged, whole, truth, {kk: (len(v),) for kk, v in truth.items()}, seed=4)
    merged.close()
    whole.close()
