#!/usr/bin/env python3
"""The compacted coloured graph through bft_gpu_unitig_graph_dev and bft_gpu_unitig_colors_dev on the config-3-sized canonical index of
tools/bench_unitigs.py (100 genomes of 2 Mbp, k = 27, workloads.PanGenome, ingested canonically), beside the yardstick: bft_gpu_unitigs_dev on the
same index in the same run, whose code is the parent's.  Per call (the graph at t = 0 and t = (int)(0.9 * genomes), the colours under OR and AND over
the graph of t = 0): the whole call between HIP events after a warm-up call of the same shape, mean of `reps`; the ratio to the yardstick of the same
threshold; GPU time per stage from one more call with "build_stages".  One JSON line per measurement.
usage: bench_cgraph.py [reps] [genomes] [genome_len]"""
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


def unitigs(t, thr):
    """the yardstick: ms of bft_gpu_unitigs_dev with both outputs"""
    cnt = torch.zeros(4, dtype=torch.int64, device=dev)
    t.unitigs_dev(0, 0, 0, 0, cnt.data_ptr(), min_shared=thr, stream=st)
    torch.cuda.synchronize()
    n_paths, n_chars, longest, bad = [int(v) for v in cnt.cpu().tolist()]
    assert bad == 0
    off = torch.zeros(n_paths + 1, dtype=torch.int64, device=dev)
    seq = torch.zeros(max(n_chars, 1), dtype=torch.uint8, device=dev)
    call = lambda: t.unitigs_dev(off.data_ptr(), seq.data_ptr(), n_paths, n_chars, cnt.data_ptr(), min_shared=thr, stream=st)
    ms = timed(call)
    st_ = stages_of(t, call)
    print(json.dumps({"call": "bft_gpu_unitigs_dev", "k": t.k, "genomes": genomes, "kmers": n_kmers, "min_shared": thr, "paths": n_paths, "chars": n_chars,
                      "longest": longest, "ms": round(ms, 3), "stages": st_}), flush=True)
    return ms, off, seq


def graph(t, thr, yard_ms, u_off, u_seq):
    cnt = torch.zeros(6, dtype=torch.int64, device=dev)
    t.unitig_graph_dev(0, 0, 0, 0, 0, 0, 0, 0, 0, cnt.data_ptr(), min_shared=thr, stream=st)
    torch.cuda.synchronize()
    ns, nc, longest, bad, nl, singles = [int(v) for v in cnt.cpu().tolist()]
    assert bad == 0
    nm = nc - ns * (t.k - 1)
    so = torch.zeros(ns + 1, dtype=torch.int64, device=dev)
    sq = torch.zeros(max(nc, 1), dtype=torch.uint8, device=dev)
    lo = torch.zeros(2 * ns + 1, dtype=torch.int64, device=dev)
    lk = torch.zeros(max(nl, 1), dtype=torch.int32, device=dev)
    mem = torch.zeros(max(nm, 1), dtype=torch.int32, device=dev)
    call = lambda: t.unitig_graph_dev(so.data_ptr(), sq.data_ptr(), lo.data_ptr(), lk.data_ptr(), mem.data_ptr(), ns, nc, nl, nm, cnt.data_ptr(), min_shared=thr,
                                      stream=st)
    ms = timed(call)
    # sanity on the whole output: offsets, every row once, link targets in range and ascending per list, the unitigs inside the segments
    assert int(so[0]) == 0 and int(so[-1]) == nc and int(lo[0]) == 0 and int(lo[-1]) == nl
    lens = so[1:] - so[:-1]
    assert bool((lens >= t.k).all()) and int((lens == t.k).sum()) >= singles
    rows = torch.sort(mem[:nm].long() >> 1).values
    assert nm == 0 or bool((rows[1:] > rows[:-1]).all())
    assert thr > 0 or nm == n_kmers
    assert nl == 0 or (int(lk[:nl].min()) >= 0 and int(lk[:nl].max()) < 2 * ns)
    n_unitigs = len(u_off) - 1
    assert ns - singles == n_unitigs and nc - singles * t.k == int(u_off[-1])
    print(json.dumps({"call": "bft_gpu_unitig_graph_dev", "k": t.k, "genomes": genomes, "kmers": n_kmers, "min_shared": thr, "segments": ns, "singles": singles,
                      "chars": nc, "links": nl, "members": nm, "longest": longest, "ms": round(ms, 3), "unitigs_ms": round(yard_ms, 3),
                      "ratio_to_unitigs": round(ms / yard_ms, 3), "kmers_per_s": round(n_kmers / (ms / 1e3), 1), "stages": stages_of(t, call)}), flush=True)
    return so, mem, ns, nm


def colours(t, op, so, mem, ns, nm, yard_ms):
    rb = (genomes + 7) // 8
    rows = torch.zeros(max(ns * rb, 1), dtype=torch.uint8, device=dev)
    gc = torch.zeros(max(ns, 1), dtype=torch.int32, device=dev)
    call = lambda: t.unitig_colors_dev(mem.data_ptr(), nm, so.data_ptr(), ns, op, rows.data_ptr(), gc.data_ptr(), stream=st)
    ms = timed(call)
    pop = int(gc[:ns].long().sum())
    assert 0 <= int(gc[:ns].min()) and int(gc[:ns].max()) <= genomes
    print(json.dumps({"call": "bft_gpu_unitig_colors_dev", "op": op, "segments": ns, "members": nm, "genomes_in_rows": pop, "ms": round(ms, 3),
                      "unitigs_ms": round(yard_ms, 3), "ratio_to_unitigs": round(ms / yard_ms, 3), "members_per_s": round(nm / (ms / 1e3), 1),
                      "stages": stages_of(t, call)}), flush=True)
    return pop


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
first = None
for thr in (0, int(0.9 * genomes)):
    yard_ms, u_off, u_seq = unitigs(t, thr)
    out = graph(t, thr, yard_ms, u_off.cpu(), u_seq)
    if first is None:
        first = out + (yard_ms,)
so, mem, ns, nm, yard0 = first
p_or = colours(t, "or", so, mem, ns, nm, yard0)
p_and = colours(t, "and", so, mem, ns, nm, yard0)
assert p_and <= p_or
t.close()
