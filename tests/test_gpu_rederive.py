"""Everything a handle derives from its committed image -- flat forms, root tables, k-mer hash, the walk's view of it, node prefix hash, launch
shape, the compact table -- re-derived through every option that touches it, on ONE handle, in an order that crosses the dependencies between
them (run on the MI355X box with -m gpu).  After every bft_gpu_set_option: what footprint() and build_time() say exists against the rules read
from the code, info() against its values after the build, and presence, colour ids and one sequence query against plain-Python truth.  At three
points the image is packed and unpacked into a replica that answers the same batch (bft_gpu_image_unpack derives everything afresh), and at the
end a build runs with a pending log on the handle whose options were changed (the tail of bft_commit_image)."""
import numpy as np
import pytest

from bloomfiltertrie_amd import BFT, synth as S

pytestmark = pytest.mark.gpu

FLAT_MIN_DEFAULT = 3584  # BFT_TRESH_SUF_PREF (csrc/bft_image.h)
RSPEC_BYTES = (1 << 18) // 8  # one bit per root prefix for the walk (d_rspec): counted under "kmer_hash", allocated once, kept when the hash goes
DEFAULTS = {"kmer_hash": 1, "walk_hash": 0, "node_hash": 1, "root_direct": 3, "root_quartiles": 1, "compact_table": 1, "kmer_hash_load": 55,
            "flat_min": FLAT_MIN_DEFAULT}
# every re-derive option through every value it accepts ...
STEPS = [("kmer_hash", 0), ("kmer_hash", 1), ("walk_hash", 1), ("walk_hash", 0), ("node_hash", 0), ("node_hash", 2), ("node_hash", 1),
         ("root_direct", 0), ("root_direct", 1), ("root_direct", 2), ("root_direct", 3), ("root_quartiles", 0), ("root_quartiles", 1),
         ("compact_table", 0), ("compact_table", 1), ("kmer_hash_load", 30), ("kmer_hash_load", 55), ("flat_min", 1), ("flat_min", FLAT_MIN_DEFAULT),
         # ... the root tables and the hash's occupancy again while the walk answers through the hash's regions (rspec and the node hash in play) ...
         ("walk_hash", 1), ("root_direct", 0), ("root_direct", 3), ("kmer_hash_load", 30), ("walk_hash", 0), ("kmer_hash_load", 55),
         # ... and the hash off and on again while the table is compact
         ("kmer_hash", 0), ("kmer_hash", 1)]
REPLICA_AFTER = (0, 10, len(STEPS) - 1)  # no k-mer hash and the table resident; root tables just re-derived; the end (table dropped)
REDERIVES_FROM_TABLE = ("kmer_hash", "kmer_hash_load", "root_direct", "root_quartiles", "flat_min")


class Truth:
    """the inserted (k-mer, genome) pairs as a sorted key table and a membership matrix"""

    def __init__(self, k, pairs):
        self.k = k
        allk = np.concatenate([km for km, _ in pairs])
        gids = np.concatenate([np.full(len(km), g, np.int64) for km, g in pairs])
        self.keys, first, inv = np.unique(S.row_keys(allk), return_index=True, return_inverse=True)
        self.kmers = allk[first]
        self.member = np.zeros((len(self.keys), 3), dtype=bool)
        self.member[inv.reshape(-1), gids] = True

    def members(self, packed):
        q = S.row_keys(np.ascontiguousarray(packed))
        pos = np.minimum(np.searchsorted(self.keys, q), len(self.keys) - 1)
        m = self.member[pos].copy()
        m[~(self.keys[pos] == q)] = False
        return m

    def colors(self, packed):
        m = self.members(packed)
        off = np.zeros(len(m) + 1, np.uint64)
        off[1:] = np.cumsum(m.sum(axis=1))
        return S.to_bits(m.any(axis=1)), off, np.nonzero(m)[1].astype(np.uint32)

    def sequence(self, codes, thr):
        m = self.members(S.pack_codes(np.lib.stride_tricks.sliding_window_view(codes, self.k)))
        cnt = m.sum(axis=0)
        return np.flatnonzero((cnt >= np.ceil(len(m) * thr)) & (cnt > 0)).tolist()


def _data(k):
    """3 genomes over ~3 x 10^4 k-mers under a dozen 9-mer prefixes on two levels (child nodes below the root), plus the k-mers of a short genome
    (the sequence query's), and what the last step inserts"""
    rng = np.random.default_rng(k)
    deep = S.low_entropy_kmers(30000, k, 12, seed=4 + k, levels=2)
    mask = rng.random((len(deep), 3)) < 0.6
    mask[~mask.any(axis=1), 0] = True
    anc = S.random_genome(3000, 20 + k)
    pairs = [(np.ascontiguousarray(deep[mask[:, g]]), g) for g in range(3)]
    pairs += [(S.distinct(S.kmers_of(anc, k)), 0), (S.distinct(S.kmers_of(S.mutate(anc, 0.01, 21 + k), k)), 1)]
    late = [(S.low_entropy_kmers(4000, k, 12, seed=5 + k, levels=2), 2), (np.ascontiguousarray(deep[::7]), 1)]
    return pairs, late, anc


@pytest.mark.parametrize("k", [27, 45])  # one-word and two-word keys (the two branches of bft_ensure_table)
def test_every_rederive_option_on_one_handle(k):
    import torch
    pairs, late, anc = _data(k)
    gt = Truth(k, pairs)
    rng = np.random.default_rng(100 + k)
    q = np.ascontiguousarray(np.concatenate([gt.kmers[rng.integers(0, len(gt.kmers), 2048)],
                                             S.snp_mutants(gt.kmers[rng.integers(0, len(gt.kmers), 2048)], k, 7)]))
    read = anc[500:500 + k + 40]
    asc = bytes(S._ASCII[read]).decode()
    t = BFT(k)
    for km, g in pairs:
        t.insert_kmers(km, g)
    t.build()
    info0 = t.info()
    assert info0["nodes"] > 1 and info0["root_ccs"] > 0, info0  # (else the node hash and the root tables are never derived)
    assert info0["kmers"] == len(gt.keys) and info0["genomes"] == 3

    def answers(h, truth, what):
        eb, eoff, eids = truth.colors(q)
        assert 0.4 < S.from_bits(eb, len(q)).mean() < 0.6
        assert (h.query_presence(q) == eb).all(), what
        b, off, ids = h.query_colors(q)
        assert (b == eb).all() and (off == eoff).all() and (ids == eids).all(), what
        want = truth.sequence(read, 0.5)
        assert want and h.query_sequences([asc], 0.5) == [want], what

    def rules(h, opts, what, table_before=None, name=None):
        fp, bt = h.footprint(), h.build_time()
        kh = bool(opts["kmer_hash"])
        assert (bt["kmer_hash_lines"] > 0) == kh, (what, bt["kmer_hash_lines"])
        # (off: nothing but the walk's root-prefix bitmap, where one was ever made, stays under this entry)
        assert (fp["kmer_hash"] > RSPEC_BYTES) if kh else (fp["kmer_hash"] in (0, RSPEC_BYTES)), (what, fp["kmer_hash"])
        nph = opts["node_hash"] == 2 or (opts["node_hash"] == 1 and (not kh or bool(opts["walk_hash"])))
        assert (fp["node_prefix_hash"] > 0) == nph, (what, fp["node_prefix_hash"])
        assert (bt["node_hash_keys"] > 0) == nph, (what, bt["node_hash_keys"])
        rd = opts["root_direct"]
        assert bt["root_tables"] in ((1.0, 2.0) if rd == 3 else (float(rd),)), (what, bt["root_tables"])
        table = (fp["kmer_table"], fp["colorset_per_kmer"])
        if not (opts["compact_table"] and kh):
            assert table[0] > 0 and table[1] > 0, (what, table)  # nothing else holds the k-mers and their colour sets
        elif name in REDERIVES_FROM_TABLE or name == "compact_table" or name is None:
            assert table == (0, 0), (what, table)  # brought back for the derivation where it was away, and dropped again
        else:
            assert table == table_before, (what, table, table_before)  # "node_hash", "walk_hash": the table stays as it was, resident or away
        inf = h.info()
        for key, v in info0.items():
            if key not in ("image_bytes", "pending_pairs"):
                assert inf[key] == v, (what, key, inf[key], v)
        assert inf["pending_pairs"] == 0, what

    def replica(what):
        n = t.image_size()
        blob = torch.empty(n, dtype=torch.uint8, device="cuda:0")
        t.image_pack(blob.data_ptr(), n)
        with BFT.from_image(blob.data_ptr(), n, device=0) as r:
            rules(r, DEFAULTS, what)  # (a replica starts from the default options)
            answers(r, gt, what)

    opts = dict(DEFAULTS)
    rules(t, opts, "after the build")
    answers(t, gt, "after the build")
    for i, (name, value) in enumerate(STEPS):
        what = (k, i, name, value, dict(opts))
        fp = t.footprint()
        before = (fp["kmer_table"], fp["colorset_per_kmer"])
        t.set_option(name, value)
        opts[name] = value
        rules(t, opts, what, before, name)
        answers(t, gt, what)
        if i in REPLICA_AFTER:
            replica(what + ("replica",))
    assert opts == DEFAULTS

    # a pending log, one flat_min toggle on the built image, then a query: the build it triggers commits on the handle whose options were changed
    for km, g in late:
        t.insert_kmers(km, g)
    assert t.info()["pending_pairs"] > 0
    t.set_option("flat_min", 1)
    gt2 = Truth(k, pairs + late)
    assert (t.query_presence(q) == gt2.colors(q)[0]).all()
    info0 = t.info()
    assert info0["kmers"] == len(gt2.keys) and info0["pending_pairs"] == 0 and info0["nodes"] > 1
    rules(t, dict(DEFAULTS, flat_min=1), (k, "after the build with a pending log"))
    answers(t, gt2, (k, "after the build with a pending log"))
    t.close()
