#!/usr/bin/env python3
"""Sequence threading through bft_gpu_thread_sequences_dev on the config-3-sized canonical index of tools/bench_cgraph.py (100 genomes of 2 Mbp,
k = 27, workloads.PanGenome, ingested canonically), beside two yardsticks in the same run whose code is the parent's: bft_gpu_query_sequences_dev on
the same blobs, and bft_gpu_unitig_segment_of_dev (one dependent lower bound per k-mer of the index).  Two batches: (a) the genomes themselves, one
sequence each; (b) reads of 150 characters sampled from them with 1 % substitutions.  Per batch: the whole call with every output between HIP events
after a warm-up call of the same shape, mean of `reps`; positions per second; the ratio to each yardstick; GPU time per stage from one more call
with "build_stages", and the share of the locate stage.  One JSON line per measurement.
usage: bench_threading.py [reps] [genomes] [genome_len] [reads]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from bloomfiltertrie_amd import BFT, workloads as W  # noqa: E402

args = [int(a) for a in sys.argv[1:] if a.isdigit()]
reps = args[0] if len(args) > 0 else 5
genomes = args[1] if len(args) > 1 else 100
glen = args[2] if len(args) > 2 else 2_000_000
n_reads = args[3] if len(args) > 3 else 1_000_000
K, READ = 27, 150
dev = torch.device("cuda", 0)
st = torch.cuda.current_stream().cuda_stream


def timed(call):
    call()  # warm-up of the timed shape
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def stages_of(t, call):
    t.set_option("build_stages", 1)
    call()
    torch.cuda.synchronize()
    out = [{"stage": nm, "ms": round(sms, 4), "alg_bytes": by, "GB/s": round(by / sms / 1e6, 1) if sms > 0 and by else None} for nm, sms, by in t.build_stages()]
    t.set_option("build_stages", 0)
    return out


def graph_and_table(t):
    """the device arrays of the graph at t = 0 and its segment table; ms of bft_gpu_unitig_segment_of_dev (a yardstick)"""
    cnt = torch.zeros(6, dtype=torch.int64, device=dev)
    t.unitig_graph_dev(0, 0, 0, 0, 0, 0, 0, 0, 0, cnt.data_ptr(), stream=st)
    torch.cuda.synchronize()
    ns, nc, _, bad, nl, _ = [int(v) for v in cnt.cpu().tolist()]
    assert bad == 0
    nm = nc - ns * (t.k - 1)
    so = torch.zeros(ns + 1, dtype=torch.int64, device=dev)
    sq = torch.zeros(max(nc, 1), dtype=torch.uint8, device=dev)
    lo = torch.zeros(2 * ns + 1, dtype=torch.int64, device=dev)
    lk = torch.zeros(max(nl, 1), dtype=torch.int32, device=dev)
    mem = torch.zeros(max(nm, 1), dtype=torch.int32, device=dev)
    t.unitig_graph_dev(so.data_ptr(), sq.data_ptr(), lo.data_ptr(), lk.data_ptr(), mem.data_ptr(), ns, nc, nl, nm, cnt.data_ptr(), stream=st)
    seg_of = torch.zeros(n_kmers, dtype=torch.int32, device=dev)
    pos = torch.zeros(n_kmers, dtype=torch.int32, device=dev)
    ms = timed(lambda: t.unitig_segment_of_dev(mem.data_ptr(), nm, so.data_ptr(), ns, seg_of.data_ptr(), pos.data_ptr(), n_kmers, stream=st))
    print(json.dumps({"call": "bft_gpu_unitig_segment_of_dev", "k": t.k, "genomes": genomes, "kmers": n_kmers, "segments": ns, "links": nl, "members": nm,
                      "ms": round(ms, 3), "members_per_s": round(nm / (ms / 1e3), 1)}), flush=True)
    del sq, mem
    return (so, lo, lk, seg_of, pos), (ns, nl), ms


def thread(t, what, blob, off, n_seqs, graph, sizes, segof_ms):
    so, lo, lk, seg_of, pos = graph
    ns, nl = sizes
    n_chars = int(blob.numel())
    common = (blob.data_ptr(), off.data_ptr(), n_seqs, n_chars, seg_of.data_ptr(), pos.data_ptr(), n_kmers, so.data_ptr(), ns, lo.data_ptr(), lk.data_ptr(), nl)
    cnt = torch.zeros(8, dtype=torch.int64, device=dev)
    t.thread_sequences_dev(*common, 0, 0, 0, 0, 0, cnt.data_ptr(), stream=st)
    torch.cuda.synchronize()
    c = [int(v) for v in cnt.cpu().tolist()]
    nw, nst, positions = c[0], c[1], c[2]
    assert c[7] == 0 and c[5] == 0 and c[6] == 0  # t = 0 on a canonical index: no row outside a segment, no break between located neighbours
    walks = torch.zeros((max(nw, 1), 4), dtype=torch.int64, device=dev)
    woff = torch.zeros(nw + 1, dtype=torch.int64, device=dev)
    steps = torch.zeros(max(nst, 1), dtype=torch.int32, device=dev)
    call = lambda: t.thread_sequences_dev(*common, walks.data_ptr(), woff.data_ptr(), nw, steps.data_ptr(), nst, cnt.data_ptr(), stream=st)
    ms = timed(call)
    # sanity on the whole output: the counts again, offsets that ascend to n_steps, walks in ascending (s, p) inside their sequences, positions
    # accounted for: located ones are the walks' n_w
    assert [int(v) for v in cnt.cpu().tolist()] == c
    assert int(woff[0]) == 0 and int(woff[-1]) == nst and bool((woff[1:] > woff[:-1]).all())
    if nw:
        key = walks[:nw, 0] * (1 << 32) + walks[:nw, 1]
        assert bool((key[1:] > key[:-1]).all())
        lens = off[1:] - off[:-1]
        assert bool((walks[:nw, 1] + walks[:nw, 2] + (t.k - 1) <= lens[walks[:nw, 0]]).all())
        assert int(walks[:nw, 2].sum()) == positions - c[3] - c[4] and int((steps[:nst].long() & 0xFFFFFFFF).max()) < 2 * ns
    # the yardstick on the same blob: the sequence queries (colour sets of every position, tallied per sequence)
    rows = torch.zeros((n_seqs, (genomes + 7) // 8), dtype=torch.uint8, device=dev)
    q_ms = timed(lambda: t.query_sequences_dev(blob.data_ptr(), off.data_ptr(), n_seqs, n_chars, 0.5, rows.data_ptr(), canonical=True, stream=st))
    stages = stages_of(t, call)
    total = sum(s["ms"] for s in stages if s["stage"].startswith("threading:"))
    locate = next(s["ms"] for s in stages if s["stage"] == "threading: locate")
    print(json.dumps({"call": "bft_gpu_thread_sequences_dev", "batch": what, "k": t.k, "genomes": genomes, "kmers": n_kmers, "segments": ns, "sequences": n_seqs,
                      "chars": n_chars, "positions": positions, "invalid": c[3], "absent": c[4], "walks": nw, "steps": nst, "ms": round(ms, 3),
                      "positions_per_s": round(positions / (ms / 1e3), 1), "query_sequences_ms": round(q_ms, 3), "ratio_to_query_sequences": round(ms / q_ms, 4),
                      "segment_of_ms": round(segof_ms, 3), "ratio_to_segment_of": round(ms / segof_ms, 4),
                      "ratio_to_segment_of_per_lookup": round((ms / positions) / (segof_ms / n_kmers), 4), "locate_ms": locate,
                      "locate_share_of_stages": round(locate / total, 4), "locate_dominates": bool(locate > total / 2), "stages": stages}), flush=True)


t0 = time.perf_counter()
pan = W.PanGenome(genomes, glen, 0.01, 4242, dev)
t = BFT(K)
ascii_of = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
one = torch.tensor([0, glen], dtype=torch.int64, device=dev)
texts = []
for g in range(genomes):
    seq = ascii_of[pan.genome(g).long()]
    t.add_genome(f"g{g}")
    t.insert_sequences_dev(seq.data_ptr(), one.data_ptr(), 1, glen, g, canonical=True, stream=st)
    texts.append(seq)
t.build()
n_kmers = int(t.info()["kmers"])
print(json.dumps({"index": "config-3-sized, canonical", "genomes": genomes, "genome_len": glen, "kmers": n_kmers, "setup_s": round(time.perf_counter() - t0, 1)}),
      flush=True)
graph, sizes, segof_ms = graph_and_table(t)
# (a) the genomes themselves
blob = torch.cat(texts)
off = torch.arange(genomes + 1, dtype=torch.int64, device=dev) * glen
thread(t, "the indexed genomes", blob, off, genomes, graph, sizes, segof_ms)
# (b) reads of 150 characters with 1 % substitutions
gen = torch.Generator(device=dev)
gen.manual_seed(99)
start = torch.randint(0, genomes * glen - READ, (n_reads,), generator=gen, device=dev)
start = torch.minimum(start, (start // glen) * glen + (glen - READ))  # (inside one genome)
reads = blob[(start[:, None] + torch.arange(READ, device=dev)[None, :]).reshape(-1)].clone()
hit = torch.rand(reads.numel(), generator=gen, device=dev) < 0.01
code = torch.zeros(256, dtype=torch.int64, device=dev)
code[list(b"ACGT")] = torch.arange(4, device=dev)
shift = torch.randint(1, 4, (int(hit.sum()),), generator=gen, device=dev)
reads[hit] = ascii_of[(code[reads[hit].long()] + shift) % 4]
roff = torch.arange(n_reads + 1, dtype=torch.int64, device=dev) * READ
del blob, texts
thread(t, f"reads of {READ} characters, 1 % substitutions", reads, roff, n_reads, graph, sizes, segof_ms)
t.close()
