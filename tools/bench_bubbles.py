#!/usr/bin/env python3
"""Bubbles and the k-mer -> segment table through bft_gpu_unitig_bubbles_dev and bft_gpu_unitig_segment_of_dev on the config-3-sized canonical index
of tools/bench_cgraph.py (100 genomes of 2 Mbp, k = 27, workloads.PanGenome, ingested canonically), beside the yardstick: bft_gpu_unitig_graph_dev on
the same index in the same run, whose code is the parent's.  Per call (the graph at t = 0; the bubbles without a limit and with max_branch_chars =
2k - 1; the segment table): the whole call between HIP events after a warm-up call of the same shape, mean of `reps`; the ratio to the yardstick and to
its "link targets" stage; GPU time per stage from one more call with "build_stages".  One JSON line per measurement.
usage: bench_bubbles.py [reps] [genomes] [genome_len]"""
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
K = 27
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


def graph(t):
    """the yardstick: ms of bft_gpu_unitig_graph_dev at t = 0 with every output, its stages, and the device arrays the other calls read"""
    cnt = torch.zeros(6, dtype=torch.int64, device=dev)
    t.unitig_graph_dev(0, 0, 0, 0, 0, 0, 0, 0, 0, cnt.data_ptr(), stream=st)
    torch.cuda.synchronize()
    ns, nc, longest, bad, nl, singles = [int(v) for v in cnt.cpu().tolist()]
    assert bad == 0
    nm = nc - ns * (t.k - 1)
    so = torch.zeros(ns + 1, dtype=torch.int64, device=dev)
    sq = torch.zeros(max(nc, 1), dtype=torch.uint8, device=dev)
    lo = torch.zeros(2 * ns + 1, dtype=torch.int64, device=dev)
    lk = torch.zeros(max(nl, 1), dtype=torch.int32, device=dev)
    mem = torch.zeros(max(nm, 1), dtype=torch.int32, device=dev)
    call = lambda: t.unitig_graph_dev(so.data_ptr(), sq.data_ptr(), lo.data_ptr(), lk.data_ptr(), mem.data_ptr(), ns, nc, nl, nm, cnt.data_ptr(), stream=st)
    ms = timed(call)
    stages = stages_of(t, call)
    links_ms = next(s["ms"] for s in stages if s["stage"] == "unitig graph: link targets")
    print(json.dumps({"call": "bft_gpu_unitig_graph_dev", "k": t.k, "genomes": genomes, "kmers": n_kmers, "min_shared": 0, "segments": ns, "singles": singles,
                      "chars": nc, "links": nl, "members": nm, "ms": round(ms, 3), "link_targets_ms": links_ms, "stages": stages}), flush=True)
    return (so, sq, lo, lk, mem), (ns, nc, nl, nm), ms, links_ms


def bubbles(t, arrays, sizes, limit, yard_ms, links_ms):
    so, sq, lo, lk, _ = arrays
    ns, _, nl, _ = sizes
    cnt = torch.zeros(4, dtype=torch.int64, device=dev)
    t.unitig_bubbles_dev(so.data_ptr(), sq.data_ptr(), lo.data_ptr(), lk.data_ptr(), ns, nl, 0, 0, cnt.data_ptr(), max_branch_chars=limit, stream=st)
    torch.cuda.synchronize()
    nb, branches, subst, longest = [int(v) for v in cnt.cpu().tolist()]
    rec = torch.zeros((max(nb, 1), 6), dtype=torch.int32, device=dev)
    call = lambda: t.unitig_bubbles_dev(so.data_ptr(), sq.data_ptr(), lo.data_ptr(), lk.data_ptr(), ns, nl, rec.data_ptr(), nb, cnt.data_ptr(), max_branch_chars=limit,
                                        stream=st)
    ms = timed(call)
    # sanity on the whole output: sources ascending and the reported mirror, every branch a link of its source, the branches' one link is the sink
    r = rec[:nb].long() & 0xFFFFFFFF
    assert [int(v) for v in cnt.cpu().tolist()] == [nb, branches, subst, longest]
    if nb:
        assert bool((r[1:, 0] > r[:-1, 0]).all()) and bool((r[:, 0] < (r[:, 1] ^ 1)).all())
        assert int((r[:, 2:] != 0xFFFFFFFF).sum()) == branches and bool((lo[r[:, 0] + 1] - lo[r[:, 0]] == (r[:, 2:] != 0xFFFFFFFF).sum(1)).all())
        assert bool((lk[lo[r[:, 0]]].long() == r[:, 2]).all()) and bool((lk[lo[r[:, 2]]].long() == r[:, 1]).all())
        lens = (so[(r[:, 2] >> 1) + 1] - so[r[:, 2] >> 1])
        assert int(lens.max()) <= longest and (limit == 0 or longest <= limit)
    print(json.dumps({"call": "bft_gpu_unitig_bubbles_dev", "k": t.k, "genomes": genomes, "kmers": n_kmers, "segments": ns, "links": nl, "max_branch_chars": limit,
                      "bubbles": nb, "branches": branches, "substitution_shaped": subst, "longest_branch": longest, "ms": round(ms, 3),
                      "graph_ms": round(yard_ms, 3), "ratio_to_graph": round(ms / yard_ms, 4), "link_targets_ms": links_ms,
                      "ratio_to_link_targets": round(ms / links_ms, 4), "oriented_segments_per_s": round(2 * ns / (ms / 1e3), 1),
                      "stages": stages_of(t, call)}), flush=True)
    return nb


def segment_table(t, arrays, sizes, yard_ms, links_ms):
    so, _, _, _, mem = arrays
    ns, _, _, nm = sizes
    seg_of = torch.zeros(n_kmers, dtype=torch.int32, device=dev)
    pos = torch.zeros(n_kmers, dtype=torch.int32, device=dev)
    call = lambda: t.unitig_segment_of_dev(mem.data_ptr(), nm, so.data_ptr(), ns, seg_of.data_ptr(), pos.data_ptr(), n_kmers, stream=st)
    ms = timed(call)
    # sanity: at t = 0 every row lies in one segment, and the table inverts the members
    s, p = seg_of.long() & 0xFFFFFFFF, pos.long() & 0xFFFFFFFF
    assert nm == n_kmers and int(s.max()) < 2 * ns
    moff = so[:-1] - torch.arange(ns, device=dev) * (t.k - 1)
    back = mem[(moff[s >> 1] + p)].long()
    assert bool((back == 2 * torch.arange(n_kmers, device=dev) + (s & 1)).all())
    print(json.dumps({"call": "bft_gpu_unitig_segment_of_dev", "k": t.k, "genomes": genomes, "kmers": n_kmers, "segments": ns, "members": nm, "ms": round(ms, 3),
                      "graph_ms": round(yard_ms, 3), "ratio_to_graph": round(ms / yard_ms, 4), "link_targets_ms": links_ms,
                      "ratio_to_link_targets": round(ms / links_ms, 4), "members_per_s": round(nm / (ms / 1e3), 1), "stages": stages_of(t, call)}), flush=True)


t0 = time.perf_counter()
pan = W.PanGenome(genomes, glen, 0.01, 4242, dev)
t = BFT(K)
ascii_of = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
off = torch.tensor([0, glen], dtype=torch.int64, device=dev)
for g in range(genomes):
    seq = ascii_of[pan.genome(g).long()]
    t.add_genome(f"g{g}")
    t.insert_sequences_dev(seq.data_ptr(), off.data_ptr(), 1, glen, g, canonical=True, stream=st)
t.build()
n_kmers = int(t.info()["kmers"])
print(json.dumps({"index": "config-3-sized, canonical", "genomes": genomes, "genome_len": glen, "kmers": n_kmers, "setup_s": round(time.perf_counter() - t0, 1)}),
      flush=True)
arrays, sizes, yard_ms, links_ms = graph(t)
n_all = bubbles(t, arrays, sizes, 0, yard_ms, links_ms)
n_short = bubbles(t, arrays, sizes, 2 * K - 1, yard_ms, links_ms)
assert n_short <= n_all
segment_table(t, arrays, sizes, yard_ms, links_ms)
t.close()
