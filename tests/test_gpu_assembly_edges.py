"""The trie assembly (csrc/bft_assemble.hip) at every edge, against a decoder of its image.

The cases, the truth of the table, the model of the CC assignment and the decoder are tests/test_assembly_cases_host.py's (no GPU: it also shows
that each case reaches its regime).  Here every case is built on the device -- two or three insert batches in shuffled order, with duplicates
across them -- and, exactly:
  * `tk` is the truth's table and the decoded image is the model's structure (the decoder reads the arrays from the layout alone and rejects an
    image that breaks it);
  * every array is bit-identical to the host restatement (csrc/bft_index.cpp), at the default flat threshold and at flat_min = 1;
  * info() reports the model's counters;
  * query_rows answers set membership and the rank in the truth's order for every member (a sample of the big cases), the SNP neighbours of forty
    members at every position and k-mers that leave a member behind each level -- through the containers ("kmer_hash", "root_direct", "node_hash"
    0), through the containers with every CC flat, and with the options at their defaults.
The assembly is a list of steps (Depth, step_* in csrc/bft_assemble.hip) and a build stage ends only where a step ends: the last test holds the stage
sequence of eight cases and the bytes of every stage to a recorded table (tests/golden/assembly_stage_tables.json).
Apart from `grid` (2048 * 256 + 300 rows: a second grid pass) and the cases whose regime is a size, a case is a few hundred to a few thousand rows."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_assembly_cases_host as H  # noqa: E402

from bloomfiltertrie_amd import BFT, synth as S  # noqa: E402

pytestmark = pytest.mark.gpu

_NODES = {}  # case name -> the structure decoded from the device's image


def _queries(case):
    """[m, k] codes: members, SNP neighbours, k-mers that leave a member behind each level, random k-mers"""
    t, k = case.table, case.k
    rng = np.random.default_rng(t.n + k)
    out = [rng.integers(0, 4, (50, k), dtype=np.uint8)]
    if t.n:
        codes = S.unpack_codes(case.packed, k)
        out.append(codes if t.n <= 6000 else codes[np.unique(np.concatenate([[0, t.n - 1], rng.choice(t.n, 4000, replace=False)]))])
        base = codes[rng.choice(t.n, min(t.n, 40), replace=False)]
        snp = np.repeat(base, 3 * k, axis=0)
        at = np.arange(len(snp))
        pos, sub = np.tile(np.repeat(np.arange(k), 3), len(base)), np.tile(np.array([1, 2, 3], dtype=np.uint8), k * len(base))
        snp[at, pos] = (snp[at, pos] + sub) & 3
        out.append(snp)
        for cut in range(9, k, 9):
            leave = base[:20].copy()
            leave[:, cut:] = rng.integers(0, 4, (len(leave), k - cut), dtype=np.uint8)
            out.append(leave)
    return np.concatenate(out)


def _device_arrays(t):
    return {name: t.debug_array(name) for name in H.ARRAYS}


def _same_bytes(got, host):
    for name in H.ARRAYS:
        assert got[name].shape == host[name].shape, (name, got[name].shape, host[name].shape)
        assert (got[name] == host[name]).all(), name


@pytest.mark.parametrize("name", list(H.CASES))
def test_assembly_case(name):
    case = H.CASES[name]
    k, table = case.k, case.table
    km = S.pack_codes(case.codes) if len(case.codes) else np.zeros((0, (2 * k + 7) // 8), dtype=np.uint8)
    km = np.ascontiguousarray(km[np.random.default_rng(len(km)).permutation(len(km))])
    t = BFT(k)
    for part in np.array_split(km, 3 if len(km) % 2 else 2):
        t.insert_kmers(np.ascontiguousarray(part), 0)
    t.insert_kmers(np.ascontiguousarray(km[: len(km) // 3]), 0)
    t.build()
    # the image: the truth's table, the model's containers, the host restatement's bytes, the model's counters
    arr = _device_arrays(t)
    assert np.array_equal(arr["tk"].view(np.uint64).reshape(-1, table.W), table.words)
    got = H.decode(arr, k, flat_min=H.TRESH)
    assert H.diff(got, case.model) is None, H.diff(got, case.model)
    _NODES[name] = got
    _same_bytes(arr, H.host_arrays(case.packed, k))
    info, want = t.info(), H.counters(case.model)
    assert {f: info[f] for f in H.INFO} == want and info["kmers"] == table.n and info["k"] == k
    # the readers
    q = _queries(case)
    present, rows = table.rows_of(q)
    assert present.sum() >= min(table.n, 4000) and not present.all()
    bits, pq = np.packbits(present, bitorder="little"), S.pack_codes(q)

    def ask(how):
        b, r, _ = t.query_rows(pq)
        assert (b == bits).all(), (how, "presence")
        assert (r == rows).all(), (how, "rows")
    ask("defaults")
    for opt in ("kmer_hash", "root_direct", "node_hash"):
        t.set_option(opt, 0)
    ask("containers")
    t.set_option("flat_min", 1)  # every CC flat
    arr = _device_arrays(t)
    assert H.diff(H.decode(arr, k, flat_min=1), case.model) is None
    _same_bytes(arr, H.host_arrays(case.packed, k, flat_min=1))
    ask("containers, every CC flat")
    t.set_option("kmer_hash", 1)
    t.set_option("root_direct", 2)
    t.set_option("node_hash", 1)
    ask("defaults, every CC flat")
    t.close()


@pytest.mark.parametrize("T", (0,) + H.ASSIGN_TS)
def test_both_assignment_kernels_build_the_same_node(T):
    """k_assign_cc_one (the node is the only one of its depth) and k_assign_cc (one of three) cut the same node into the same CCs: the model's"""
    found = []
    for variant in ("only", "three"):
        name = "assign_%d_%s" % (T, variant)
        if name not in _NODES:
            test_assembly_case(name)
        found.append([nd for nd in _NODES[name] if nd["path"] == (H.X0,)][0])
    a, b = found
    shift = int(b["ccs"][0]["pref"][0, 2] - a["ccs"][0]["pref"][0, 2])
    moved = {"path": a["path"], "uc": a["uc"] + shift, "ccs": [{**c, "pref": c["pref"] + np.array([0, 0, shift, 0])} for c in a["ccs"]]}
    assert H.node_diff(moved, b) is None, H.node_diff(moved, b)
    assert len(a["ccs"]) >= 2


# the smallest cases that walk every branch of the depth loop: no k-mers; one depth that is also the last; two depths; a remainder behind the last
# level; many CCs beside a small node; three, seven (two-word keys) and fourteen depths (four words)
STAGE_CASES = ("ends_k9_n0", "root_256", "child_cc_3584", "rem26", "ncc_side", "depth_k27", "depth_k63", "depth_k126")
STAGE_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "assembly_stage_tables.json")


def stage_table(name):
    """[[stage name, algorithmic bytes]] of one build of the case: every k-mer in one batch, "build_stages" on"""
    case = H.CASES[name]
    t = BFT(case.k)
    t.set_option("build_stages", 1)
    t.insert_kmers(np.ascontiguousarray(case.packed), 0)
    t.build()
    out = [[nm, by] for nm, _, by in t.build_stages()]
    t.close()
    return out


@pytest.mark.parametrize("name", STAGE_CASES)
def test_build_stage_table_is_the_parents(name):
    """The build's stages, in order, with the bytes each one's formula gives, are the ones recorded before the assembly was cut into steps
    (tests/golden/assembly_stage_tables.json): a step that crosses a stage boundary or a byte formula that drifts shows here.  The bytes are
    doubles computed from integers: compared with ==."""
    with open(STAGE_GOLDEN) as f:
        want = json.load(f)[name]
    got = stage_table(name)
    assert len(want) > 0 and got == want, [(g, w) for g, w in zip(got, want) if g != w] or (len(got), len(want))
