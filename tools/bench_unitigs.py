#!/usr/bin/env python3
"""Canonical (bidirected) unitigs through bft_gpu_unitigs_dev on a config-3-sized index (100 genomes of 2 Mbp, k = 27, workloads.PanGenome) ingested
CANONICALLY from the genomes' sequences (bft_gpu_insert_sequences_dev, canonical = 1), beside the yardstick: bft_gpu_simple_paths_dev on the same
index, which handles half the vertices with one search per row.  Per call and threshold (t = 0 and (int)(0.9 * genomes)): the whole call between
HIP events after a warm-up call of the same shape, GPU time per stage ("build_stages"), paths, characters, the longest path, stored k-mers per
second; bft_gpu_bidirected_degrees_dev alone as well.  One JSON line per measurement.
usage: bench_unitigs.py [reps] [genomes] [genome_len]"""
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
    out = [{"stage": nm, "ms": round(sms, 4), "alg_bytes": by, "GB/s": round(by / sms / 1e6, 1) if sms > 0 else None} for nm, sms, by in t.build_stages()]
    t.set_option("build_stages", 0)
    return out


def measure(t, what, n_counts, dev_call):
    n_kmers = int(t.info()["kmers"])
    for thr in (0, int(0.9 * genomes)):
        cnt = torch.zeros(n_counts, dtype=torch.int64, device=dev)
        dev_call(0, 0, 0, 0, cnt.data_ptr(), min_shared=thr, stream=st)  # the sizes first
        torch.cuda.synchronize()
        c = [int(v) for v in cnt.cpu().tolist()]
        n_paths, n_chars, longest = c[:3]
        assert n_counts == 3 or c[3] == 0  # (the index is canonical)
        off = torch.zeros(n_paths + 1, dtype=torch.int64, device=dev)
        seq = torch.zeros(max(n_chars, 1), dtype=torch.uint8, device=dev)
        call = lambda: dev_call(off.data_ptr(), seq.data_ptr(), n_paths, n_chars, cnt.data_ptr(), min_shared=thr, stream=st)
        ms = timed(call)
        o = off.cpu()
        assert int(o[0]) == 0 and int(o[-1]) == n_chars and bool(((o[1:] - o[:-1]) >= t.k).all())
        print(json.dumps({"call": what, "k": t.k, "genomes": genomes, "kmers": n_kmers, "min_shared": thr, "paths": n_paths, "chars": n_chars,
                          "longest": longest, "ms": round(ms, 3), "kmers_per_s": round(n_kmers / (ms / 1e3), 1), "stages": stages_of(t, call)}), flush=True)


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
print(json.dumps({"index": "config-3-sized, canonical", "genomes": genomes, "genome_len": glen, "kmers": int(t.info()["kmers"]),
                  "setup_s": round(time.perf_counter() - t0, 1)}), flush=True)
measure(t, "bft_gpu_unitigs_dev", 4, t.unitigs_dev)
measure(t, "bft_gpu_simple_paths_dev", 3, t.simple_paths_dev)
n = int(t.info()["kmers"])
deg = torch.zeros(n, dtype=torch.uint8, device=dev)
bad = torch.zeros(1, dtype=torch.int64, device=dev)
call = lambda: t.bidirected_degrees_dev(deg.data_ptr(), n, bad.data_ptr(), stream=st)
ms = timed(call)
hist = torch.bincount(deg.long(), minlength=256).cpu().tolist()
print(json.dumps({"call": "bft_gpu_bidirected_degrees_dev", "kmers": n, "ms": round(ms, 3), "kmers_per_s": round(n / (ms / 1e3), 1), "noncanonical": int(bad.cpu()[0]),
                  "degree_bytes": {f"0x{b:02x}": c for b, c in enumerate(hist) if c}, "stages": stages_of(t, call)}), flush=True)
t.close()
