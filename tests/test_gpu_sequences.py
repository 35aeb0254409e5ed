"""Sequence queries (bft_gpu_query_sequences / bft_gpu_query_sequences_dev: k_seq_encode, k_seq_plan, the scan, k_seq_tiles, k_seq_kh or
k_seq_walk8 / k_seq_walk6, k_seq_tally) against ground truth at every encoder, plan, tally and walk edge.  The cases and the truth come
from tests/test_sequence_cases_host.py, which checks on the CPU that every case reaches the regime it is there for.  Every check runs
through the host call (lists of genome ids) and through the device call (rows written into a buffer pre-filled with 0xFF or 0x55, every
bit compared, the padding bits of the last byte included), with the k-mer hash answering and with the container walk answering."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_sequence_cases_host as H  # noqa: E402

from bloomfiltertrie_amd import BFT  # noqa: E402

pytestmark = pytest.mark.gpu
_FILL = [0xFF]


def _build(stored):
    t = BFT(stored.k)
    for g, packed in stored.phases():
        t.insert_kmers(packed, g)
    t.build()
    assert t.info()["kmers"] == len(stored.sets)
    return t


def _modes(t, modes=(True, False)):
    """the handle with the k-mer hash answering (k_seq_kh), then with the container walk answering (k_seq_walk8 / k_seq_walk6)"""
    for hashed in modes:
        t.set_option("kmer_hash", 1 if hashed else 0)
        lines = t.build_time()["kmer_hash_lines"]
        assert (lines > 0) if hashed else (lines == 0), (hashed, lines)
        yield hashed


def _dev_rows(t, reads, thr, canonical, G, shift=0):
    """the device call on a blob that starts `shift` bytes behind a 32-byte boundary, N on both sides of it"""
    import torch
    dev = torch.device("cuda", 0)
    blob = b"".join(reads)
    buf = torch.full((len(blob) + 128,), ord("N"), dtype=torch.uint8, device=dev)
    at = (-buf.data_ptr()) % 32 + 32 + shift
    if blob:
        buf[at:at + len(blob)] = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).to(dev)
    off = np.zeros(len(reads) + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in reads])
    d_off = torch.from_numpy(off).to(dev)
    _FILL[0] ^= 0xAA  # 0x55, 0xFF, 0x55, ...
    rows = torch.full((len(reads), (G + 7) // 8), _FILL[0], dtype=torch.uint8, device=dev)
    t.query_sequences_dev(buf.data_ptr() + at, d_off.data_ptr(), len(reads), len(blob), thr, rows.data_ptr(), canonical,
                          torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rows.cpu().numpy()


def _check(t, case, G, shifts=(0,), host=True, what=""):
    assert t.info()["genomes"] == G
    for canonical, thr in case.runs():
        want = case.truth(thr, canonical)
        if host:
            got = t.query_sequences(case.reads, thr, canonical)
            bad = [i for i in range(len(want)) if got[i] != want[i]]
            assert not bad, (what, "host", canonical, thr, bad[:5], [(got[i], want[i]) for i in bad[:2]])
        rows = H.expected_rows(want, G)
        for shift in shifts:
            got = _dev_rows(t, case.reads, thr, canonical, G, shift)
            bad = np.flatnonzero((got != rows).any(axis=1))
            assert not len(bad), (what, "device", canonical, thr, shift, bad[:5].tolist(),
                                  [(np.flatnonzero(np.unpackbits(got[i], bitorder="little")).tolist()[:8], want[i][:8]) for i in bad[:2]])


@pytest.mark.parametrize("k", H.ENCODER_KS)
def test_encoder_byte_table(k):
    """Every byte value between stored flanks (byte 0 and the bytes from 0x80 up included: the Python mirror passes the blob with its
    length, nothing is left out): exactly ACGTUacgtu give windows over the byte, any other byte costs exactly the k windows over it.  The
    device call takes the blob 0, 1, 15 and 16 bytes behind a 32-byte boundary at totals of 0, 1 and 31 (mod 32) characters: the 32-byte
    loads, the byte path, and the real characters of a ragged last word.  What the encoder writes for the filler behind them is not
    observed: seq_window masks those bits off for every window."""
    t = _build(H.encoder_case(k, 0).stored)
    try:
        for hashed in _modes(t):
            for tail in H.ENCODER_TAILS:
                _check(t, H.encoder_case(k, tail), 5, shifts=H.ENCODER_SHIFTS, what=(hashed, tail))
    finally:
        t.close()


@pytest.mark.parametrize("k", H.BADCHAR_KS)
def test_bad_character_at_every_word_offset(k):
    """An N at the first, second, 31st .. 34th, 64th .. 66th, last but one and last character of a read that starts at offset 0, 1 and 31
    (mod 32) of the blob, N right before and right behind every read: window i is dead iff i <= p < i + k.  The thresholds 1 / m, 1.0
    and right below / above every true count make one wrongly dead or wrongly live window flip a bit."""
    case = H.badchar_case(k)
    t = _build(case.stored)
    try:
        for hashed in _modes(t):
            _check(t, case, 1, what=hashed)
    finally:
        t.close()


@pytest.mark.parametrize("k", H.PLAN_KS)
def test_plan_and_tile_edges(k):
    """Reads that start at positions 64, 65, 127, 128, 256 and 1024; runs of 300 reads without a position at the start, in front of a tile
    boundary and at the end; a read of 6000 nt; reads of exactly k; batches without any position (with and without characters: every row
    zero over the pre-filled buffer); batches of one read; 20 000 reads of k .. k + 5 characters whose genome differs between the two reads
    one wavefront of k_seq_tally handles."""
    cases = H.plan_case(k)
    t = _build(cases["edges"].stored)
    try:
        for hashed in _modes(t):
            for name, case in cases.items():
                _check(t, case, 2, what=(hashed, name))
    finally:
        t.close()


def test_tally_runs_and_set_sizes():
    """Runs of one colour set over positions 60..70 and 120..135 of a read, runs of 1, 2, 64, 65, 129 and 300 positions, sets of 1, 7, 8, 9, 16,
    17, 64 and 65 genomes; thresholds 1.0, 0.1 (m = 30, m = 10), 0.28 (m = 25, m = 50: the double product lies above the exact one), 1e-9
    and per read c / m of a true count with the doubles next to it."""
    case = H.tally_case()
    G = case.stored.n_genomes()
    t = _build(case.stored)
    try:
        for hashed in _modes(t):
            _check(t, case, G, what=hashed)
    finally:
        t.close()


def _assert_dictionary_id_bytes(t, stored, id_bytes):
    """the dictionary holds its offsets (4 bytes per set, and one) and its ids, id_bytes each: not a byte more"""
    lists = {tuple(sorted(v)) for v in stored.sets.values()}
    assert t.info()["colorsets"] == len(lists)
    assert t.footprint()["colorset_dictionary"] == 4 * (len(lists) + 1) + id_bytes * sum(len(s) for s in lists)


@pytest.mark.parametrize("G", H.WINDOW_GS + ("wide",))
def test_tally_genome_windows_and_id_widths(G):
    """G genomes around the tally's 2048-genome window: one window, its last genome, three windows, the last partial byte of a row.  The genomes
    next to every window edge and the last one are hit; genome j of one window is hit without genome j of the next.  wide: the genome ids 0, 1,
    255, 256, 65535, 65536 and 70001 -- the dictionary's ids are resident in four bytes, a read takes 35 genome windows."""
    case = H.wide_case() if G == "wide" else H.window_case(G)
    n_genomes, id_bytes = (70002, 4) if G == "wide" else (G, 2)
    t = _build(case.stored)
    try:
        _assert_dictionary_id_bytes(t, case.stored, id_bytes)
        for hashed in _modes(t):
            _check(t, case, n_genomes, what=hashed)
    finally:
        t.close()


@pytest.mark.parametrize("shape", H.WALK_SHAPES)
@pytest.mark.parametrize("k", H.WALK_KS)
def test_walk_sequence_kernels_one_and_two_words(k, shape):
    """k_seq_walk8<1> (k = 18, 27, 31) and k_seq_walk6<2> (k = 36, 63) without the k-mer hash, both strands, on the reads of the plan test.
    tiny: fewer than 255 k-mers, no CC at the root -- the unstaged form.  normal and deep (child nodes asserted): the staged form, first as
    built -- the root's derived tables answer the root level and nothing of the root is copied --, then with "root_direct" 0
    (root_tables == 0 asserted): the root's Bloom filter and CCs are staged into LDS and read from there."""
    case = H.walk_case(k, shape)
    t = _build(case.stored)
    try:
        info = t.info()
        if shape == "tiny":
            assert info["root_ccs"] == 0 and info["kmers"] < 255
        else:
            assert 1 <= info["root_ccs"] <= H.ROOT_MAX_CC
        if shape == "deep":
            assert info["child_nodes"] > 0
        G = case.stored.n_genomes()
        for hashed in _modes(t, modes=(False,)):
            _check(t, case, G, what=(shape, "as built"))
            t.set_option("root_direct", 0)
            assert t.build_time()["root_tables"] == 0 and t.build_time()["kmer_hash_lines"] == 0
            _check(t, case, G, what=(shape, "root_direct 0"))
    finally:
        t.close()
